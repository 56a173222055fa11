// hip_kernels_lean.hip — the lean instantiations of the unit-stream kernel (hip_units_kernel.h under UNITS_LEAN), here under the name k_units_lean, for classic plans in which no
// unit is a row unit (DevStream::unit_facts; hip_plan.h unit_lean_form): entry mode 0 / 2 x 12-byte / dictionary descriptors x the value forms of the build (fp64: val_t, floats,
// halves; fp32: val_t) x "some unit is derived" / "none is" — 24 kernels in the fp64 library, 8 in the fp32 one.  16 strips per workgroup, nontemporal streams.
// A file of its own so that hip_kernels.hip and hip_kernels_half.hip keep their kernels and their names.
#include <hip/hip_runtime.h>

#include "hip_plan.h"
#include "hip_plan_internal.h"

#define UNITS_KERNEL k_units_lean   // this file's name for the kernel template of hip_units_kernel.h ...
#define UNITS_LEAN 1                // ... in its lean form: <UB, entry mode, strips, dictionary, nontemporal, value form, derived units>
#include "hip_units_kernel.h"

namespace tilespmv {

// the unit-stream launch of a plan whose lean form is `form` (1: derived units present, 2: none), called by launch_tiles_stream, which runs the whole-tile passes behind it
hipError_t launch_units_lean(const DevPlan &P, const DevStream &S, int form, int entry_mode, int wg_strips, int lds_pad_bytes, int xcd_chunk, const val_t *x, val_t *y, hipStream_t st)
{
    if (form != unit_lean_form(S, entry_mode, wg_strips) || form < 1) return hipErrorInvalidValue;   // (the caller asks the same function)
#define TSPMV_KL(W, CD, VF, DV) hipLaunchKernelGGL((k_units_lean<TILESPMV_UB, W, 16, CD, true, VF, DV>), dim3((unsigned)((S.ntasks + 15) / 16)), dim3(256), (size_t)lds_pad_bytes, st, S, P.rowA, P.colA, xcd_chunk, P.partial, x, y)
#define TSPMV_KL_DV(W, CD, VF) do { if (form == 1) TSPMV_KL(W, CD, VF, true); else TSPMV_KL(W, CD, VF, false); } while (0)
#define TSPMV_KL_CD(W, VF) do { if (S.cb_bits > 0) TSPMV_KL_DV(W, true, VF); else TSPMV_KL_DV(W, false, VF); } while (0)
#define TSPMV_KL_W(VF) do { if (entry_mode == 2) TSPMV_KL_CD(2, VF); else TSPMV_KL_CD(0, VF); } while (0)
#if !defined(TILESPMV_F32)
    if (S.uval_narrow == 2) TSPMV_KL_W(2);
    else if (S.uval_narrow == 1) TSPMV_KL_W(1);
    else
#endif
    TSPMV_KL_W(0);
#undef TSPMV_KL_W
#undef TSPMV_KL_CD
#undef TSPMV_KL_DV
#undef TSPMV_KL
    return hipGetLastError();
}

}  // namespace tilespmv
