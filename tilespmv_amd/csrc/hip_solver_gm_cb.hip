// hip_solver_gm_cb.hip — GMRES with the Krylov basis stored as 4-byte floats in the fp64 library (tilespmv_gmres_create_basis(..., TILESPMV_GMRES_BASIS_FLOAT); DESIGN.md §3.14,
// INTEGRATION.md §4l): the five kernels of hip_solver_gm.h that touch the basis (k_gm_dots, k_gm_orth1, k_gm_orth2, k_gm_next, k_gm_update) with BT = float, and the launch
// sequences around them.  All arithmetic, w, x, b, the Hessenberg column and every scalar stay double; a basis vector costs half the bytes in every kernel that reads it and in
// the workspace.  The fp32 library has no narrow form: this file is empty there.
#ifndef TILESPMV_F32
#include "hip_solver_gm.h"

namespace tilespmv {

const GmForm *gm_float_form() { return gm_form<float>(); }

}  // namespace tilespmv
#endif
