// hip_kernels_half.hip — fp64 build only: the four instantiations of the unit-stream kernel (hip_units_kernel.h), here under the name k_units_half, for plans whose unit values are stored as halves
// (DevStream::uval_narrow 2, plan_tile_ops.h value_halvable): entry mode 0 / 2 x 12-byte / dictionary descriptors, like the float forms in hip_kernels.hip.
// A file of its own so that hip_kernels.hip compiles to what it compiled to before these existed.
#include <hip/hip_runtime.h>

#include "hip_plan.h"
#include "hip_plan_internal.h"

#if !defined(TILESPMV_F32)
#define UNITS_KERNEL k_units_half   // this file's name for the kernel template of hip_units_kernel.h ...
#define UNITS_NARROW_FORM 2         // ... whose NARROW instantiations read halves here
#include "hip_units_kernel.h"
#endif

namespace tilespmv {

// the unit-stream launch of a 2-byte plan (called by launch_tiles_stream, which runs the whole-tile passes behind it)
hipError_t launch_units_half(const DevPlan &P, const DevStream &S, int entry_mode, int wg_strips, int lds_pad_bytes, int xcd_chunk, const val_t *x, val_t *y, hipStream_t st)
{
#if !defined(TILESPMV_F32)
    if (S.uval_narrow != 2 || S.pooled || !S.nt_stream || entry_mode == 1 || wg_strips != 16) return hipErrorInvalidValue;   // the builder gives no other plan halves
#define TSPMV_KH(W, CD) hipLaunchKernelGGL((k_units_half<TILESPMV_UB, W, 16, CD, true, false, false, true>), dim3((unsigned)((S.ntasks + 15) / 16)), dim3(256), (size_t)lds_pad_bytes, st, S, P.rowA, P.colA, xcd_chunk, P.partial, x, y)
    if (entry_mode == 2) { if (S.cb_bits > 0) TSPMV_KH(2, true); else TSPMV_KH(2, false); }
    else { if (S.cb_bits > 0) TSPMV_KH(0, true); else TSPMV_KH(0, false); }
#undef TSPMV_KH
    return hipGetLastError();
#else
    (void)P; (void)S; (void)entry_mode; (void)wg_strips; (void)lds_pad_bytes; (void)xcd_chunk; (void)x; (void)y; (void)st;
    return hipErrorInvalidValue;   // the fp32 build has no narrow plans
#endif
}

}  // namespace tilespmv
