// hip_precond.hip — a block-Jacobi preconditioner for the CG and BiCGStab solvers (tilespmv_block_jacobi_*).
//
// M is the block diagonal of A for consecutive blocks of bs rows (1 <= bs <= 16; block k = rows and columns [k bs, min((k + 1) bs, rows)), the last one short when rows % bs != 0).
// The object holds M^-1 in the value type, plane-major: plane j (j < bs) is a vector of `rows` elements padded to a multiple of 256 bytes, plane_j[i] = (M^-1)[i][blockstart(i) + j],
// 0 where the block is short.  Two kernels:
//   k_bj_build   one 16-lane strip per block (four blocks per wavefront, 8 per workgroup): [B | I] in LDS as 16 x 33 doubles (the extraction indexes by a run-time column: a register
//                array would go to scratch), lane = row extracts (duplicates added in storage order), then Gauss-Jordan with partial pivoting in double: every lane of the strip
//                scans the pivot column (the largest magnitude, ties to the lowest row), lane = column swaps the two rows and divides the pivot row, lane = row eliminates.  A short
//                block (and a strip behind the last block) is padded by the identity to bs x bs, so every strip of a workgroup takes the same path through the barriers and the
//                padding never mixes with the block: a zero never beats a pivot candidate, and its multipliers are exact zeros.  A pivot that is exactly 0 or not finite at any
//                step: the block's inverse is the identity, and the device counter is incremented (an integer atomic; its value does not depend on the order).
//   k_bj_apply   z = M^-1 r with the walk of hip_solver_common.h (solver_parts(rows) workgroups, trips of SV_U * SVB lane vectors, the scalar tail by thread 0 of workgroup 0).  Per
//                trip the workgroup stages in LDS the slab of r that the trip's blocks cover (the trip's rows widened to whole blocks, clamped to rows; 16-byte loads, scalar ones
//                for elements of the vector's tail), then every lane forms z_i = sum_j plane_j[i] r[blockstart(i) + j], j ascending, in double, rounded once.  r is read from
//                memory once, each plane once, z written once: bs + 2 elements per row.  The lanes of one block read the same LDS word for a given j (a broadcast); neighbouring
//                blocks are bs words apart.  The trip loop is SV_FOR_TRIPS' walk with the trip's first lane vector as its variable: it holds barriers, so every thread of the
//                workgroup makes every trip of the workgroup.  The <true> form also leaves one partial sum of r.z per workgroup (double, block_sum: the number of partials and the
//                order of the additions are fixed by `rows` alone), for CG.
// No kernel uses scratch.  Out of scope: MINRES (it needs a positive definite M, and the diagonal blocks of an indefinite matrix are not), multi-RHS CG (the apply would need the
// row-major [rows][nvec] layout), CGLS.
#include <hip/hip_runtime.h>

#include "hip_precond.h"

namespace tilespmv {
namespace {

constexpr int BJ_MAX = 16;                              // the largest block, and the lanes of a strip
constexpr int BJ_WG = 128;                              // threads of k_bj_build: 8 strips
constexpr int BJ_LD = 2 * BJ_MAX + 1;                   // doubles per row of [B | B^-1] (odd: the rows of a strip start in different banks)
constexpr int BJ_TRIP = SV_U * SVB;                     // lane vectors of a trip
// elements of the slab: a trip's, BJ_MAX - 1 on either side for whole blocks, SV_VPL - 1 on either side for whole lane vectors, BJ_MAX zeros behind a short last block
constexpr int BJ_SLAB = BJ_TRIP * SV_VPL + 64;
static_assert(TILESPMV_BJ_MAX_PARTIALS == SV_MAX_PARTS, "the header's bound on the partials");
static_assert(2 * (BJ_MAX - 1) + 2 * (SV_VPL - 1) + BJ_MAX <= 64 && BJ_SLAB % SV_VPL == 0, "slab");

__global__ __launch_bounds__(BJ_WG) void k_bj_build(long long rows, int bs, long long blocks, long long plane, const int *__restrict__ rp, const int *__restrict__ ci,
                                                    const val_t *__restrict__ v, val_t *__restrict__ inv, int *__restrict__ singular)
{
    __shared__ double sm[BJ_WG / BJ_MAX][BJ_MAX][BJ_LD];
    const int l = threadIdx.x & (BJ_MAX - 1);
    const long long k = (long long)blockIdx.x * (BJ_WG / BJ_MAX) + (threadIdx.x / BJ_MAX), row0 = k * bs;
    const int nb = k < blocks ? (int)std::min<long long>(bs, rows - row0) : 0;   // rows of this strip's block
    double(*a)[BJ_LD] = sm[threadIdx.x / BJ_MAX];
    // lane = row: [B | I], rows and columns from nb on are the identity's
    for (int c = 0; c < 2 * BJ_MAX; c++) a[l][c] = ((c == l && l >= nb) || c == BJ_MAX + l) ? 1.0 : 0.0;
    if (l < nb)
        for (long long e = rp[row0 + l]; e < rp[row0 + l + 1]; e++) {
            const long long c = (long long)ci[e] - row0;
            if (c >= 0 && c < nb) a[l][c] += (double)v[e];
        }
    __syncthreads();
    bool bad = false;   // (the same in every lane of the strip: all of them read the same column)
    for (int kk = 0; kk < bs; kk++) {
        int p = kk;
        double piv = a[kk][kk], best = fabs(piv);
        for (int i = kk + 1; i < bs; i++) {
            const double t = a[i][kk];
            if (fabs(t) > best) { best = fabs(t); piv = t; p = i; }
        }
        bad = bad || piv == 0.0 || !isfinite(piv);
        __syncthreads();
        if (l < bs)   // lane = column, of B and of the inverse: rows kk and p change places, the pivot row is divided
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int c = l + h * BJ_MAX;
                const double t = a[p][c] / piv;
                if (p != kk) a[p][c] = a[kk][c];
                a[kk][c] = t;
            }
        __syncthreads();
        if (l < bs && l != kk) {   // lane = row
            const double f = a[l][kk];
            for (int c = 0; c < bs; c++) {
                a[l][c] -= f * a[kk][c];
                a[l][BJ_MAX + c] -= f * a[kk][BJ_MAX + c];
            }
        }
        __syncthreads();
    }
    if (l < nb)
        for (int j = 0; j < bs; j++) inv[(long long)j * plane + row0 + l] = bad ? (val_t)(j == l ? 1 : 0) : (val_t)a[l][BJ_MAX + j];
    if (bad && l == 0 && nb > 0) atomicAdd(singular, 1);
}

template <bool DOT>
__global__ __launch_bounds__(SVB) void k_bj_apply(long long n, int bs, long long plane, const val_t *__restrict__ inv, const val_t *__restrict__ r, val_t *__restrict__ z,
                                                  double *__restrict__ prz)
{
    __shared__ svec_t slab_v[BJ_SLAB / SV_VPL];
    __shared__ double s[SVB / 64];
    val_t *const slab = reinterpret_cast<val_t *>(slab_v);
    const long long nv = n / SV_VPL;
    double arz = 0.0;
    for (long long tb = (long long)blockIdx.x * BJ_TRIP; tb < nv; tb += (long long)gridDim.x * BJ_TRIP) {
        // the trip's rows [e0, e1), their blocks' rows [s0, s1), the lane vectors [vlo, vhi) that hold them; slab[e - o0] = r[e]
        const long long e0 = tb * SV_VPL, e1 = std::min<long long>(tb + BJ_TRIP, nv) * SV_VPL;
        const long long s0 = e0 / bs * bs, s1 = std::min<long long>(n, (e1 + bs - 1) / bs * bs);
        const long long vlo = s0 / SV_VPL, vhi = std::min<long long>((s1 + SV_VPL - 1) / SV_VPL, nv), o0 = vlo * SV_VPL;
        for (long long w = vlo + threadIdx.x; w < vhi; w += SVB) slab_v[w - vlo] = lanes(r)[w];
        for (long long e = nv * SV_VPL + threadIdx.x; e < s1; e += SVB) slab[e - o0] = r[e];
        if (s1 == n && threadIdx.x < BJ_MAX) slab[s1 - o0 + threadIdx.x] = (val_t)0;   // behind a short last block (its planes hold 0 there)
        __syncthreads();
        long long vi[SV_U];
        int at[SV_U][SV_VPL];   // where the block of element q of lane vector u starts in the slab
        double acc[SV_U][SV_VPL];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            vi[u] = tb + u * SVB + threadIdx.x;
#pragma unroll
            for (int q = 0; q < SV_VPL; q++) {
                const unsigned i = (unsigned)(vi[u] * SV_VPL + q);
                at[u][q] = vi[u] < nv ? (int)((long long)(i / (unsigned)bs * (unsigned)bs) - o0) : 0;
                acc[u][q] = 0.0;
            }
        }
        for (int j0 = 0; j0 < bs; j0 += 4) {
            svec_t pv[4][SV_U];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int u = 0; u < SV_U; u++)
                    if (j0 + t < bs && vi[u] < nv) pv[t][u] = lanes(inv + (long long)(j0 + t) * plane)[vi[u]];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int u = 0; u < SV_U; u++)
                    if (j0 + t < bs && vi[u] < nv)
#pragma unroll
                        for (int q = 0; q < SV_VPL; q++) acc[u][q] += (double)pv[t][u][q] * (double)slab[at[u][q] + j0 + t];
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++)
            if (vi[u] < nv) {
                svec_t vz;
#pragma unroll
                for (int q = 0; q < SV_VPL; q++) {
                    vz[q] = (val_t)acc[u][q];
                    if (DOT) arz += (double)slab[vi[u] * SV_VPL + q - o0] * (double)vz[q];
                }
                lanes(z)[vi[u]] = vz;
            }
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) {
            const long long b0 = i / bs * bs;
            double a = 0.0;
            for (int j = 0; j < bs && b0 + j < n; j++) a += (double)inv[(long long)j * plane + i] * (double)r[b0 + j];
            const val_t zi = (val_t)a;
            z[i] = zi;
            if (DOT) arz += (double)r[i] * (double)zi;
        }
    if (DOT) {
        const double t = block_sum(arz, s);
        if (threadIdx.x == 0) prz[blockIdx.x] = t;
    }
}

}  // namespace

void block_jacobi_launch(const tilespmv_block_jacobi *bj, const val_t *r, val_t *z, double *prz, hipStream_t st)
{
    if (prz) hipLaunchKernelGGL(k_bj_apply<true>, dim3(bj->np), dim3(SVB), 0, st, bj->rows, bj->bs, bj->plane, bj->inv, r, z, prz);
    else hipLaunchKernelGGL(k_bj_apply<false>, dim3(bj->np), dim3(SVB), 0, st, bj->rows, bj->bs, bj->plane, bj->inv, r, z, (double *)nullptr);
}

}  // namespace tilespmv

using namespace tilespmv;

extern "C" int tilespmv_block_jacobi_create(tilespmv_block_jacobi **bj, int rows, int block_size)
{
    if (bj) *bj = nullptr;
    if (!bj || rows <= 0 || block_size < 1 || block_size > BJ_MAX) return (int)hipErrorInvalidValue;
    const size_t plane_bytes = ((size_t)rows * sizeof(val_t) + 255) / 256 * 256;
    DeviceBlock blk;
    const hipError_t e = blk.alloc((size_t)block_size * plane_bytes + 256);
    if (e != hipSuccess) return (int)e;
    auto *b = new tilespmv_block_jacobi();
    b->rows = rows; b->bs = block_size; b->blocks = ((long long)rows + block_size - 1) / block_size;
    b->plane = (long long)(plane_bytes / sizeof(val_t)); b->np = solver_parts(rows); b->bytes = (size_t)block_size * plane_bytes + 256;
    b->inv = blk.take<val_t>((size_t)block_size * plane_bytes);
    b->singular = blk.take<int>(256);
    *bj = b;
    return 0;
}

extern "C" void tilespmv_block_jacobi_destroy(tilespmv_block_jacobi *bj)
{
    if (!bj) return;
    (void)hipFree(bj->inv);
    delete bj;
}

extern "C" int tilespmv_block_jacobi_update(tilespmv_block_jacobi *bj, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, void *stream)
{
    if (!bj || !d_csrRowPtr || !d_csrColIdx || !d_csrVal) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(bj->singular, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const int per_wg = BJ_WG / BJ_MAX;
    hipLaunchKernelGGL(k_bj_build, dim3((unsigned)((bj->blocks + per_wg - 1) / per_wg)), dim3(BJ_WG), 0, st, bj->rows, bj->bs, bj->blocks, bj->plane, d_csrRowPtr, d_csrColIdx,
                       d_csrVal, bj->inv, bj->singular);
    return (int)hipGetLastError();
}

static int bj_apply(const tilespmv_block_jacobi *bj, const val_t *d_r, val_t *d_z, double *d_partials, bool dot, void *stream)
{
    if (!bj || !d_r || !d_z || d_r == d_z || misaligned(d_r) || misaligned(d_z) || (dot && !d_partials)) return (int)hipErrorInvalidValue;
    block_jacobi_launch(bj, d_r, d_z, dot ? d_partials : nullptr, (hipStream_t)stream);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_block_jacobi_apply(const tilespmv_block_jacobi *bj, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, void *stream)
{
    return bj_apply(bj, d_r, d_z, nullptr, false, stream);
}

extern "C" int tilespmv_block_jacobi_apply_dot(const tilespmv_block_jacobi *bj, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, double *d_partials, void *stream)
{
    return bj_apply(bj, d_r, d_z, d_partials, true, stream);
}

extern "C" int tilespmv_block_jacobi_info(const tilespmv_block_jacobi *bj, void *stream, long long *out)
{
    if (!bj || !out) return (int)hipErrorInvalidValue;
    int singular = 0;
    const hipError_t e = read_scalars(&singular, bj->singular, sizeof(singular), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    out[TILESPMV_BJ_INFO_ROWS] = bj->rows;
    out[TILESPMV_BJ_INFO_BLOCK_SIZE] = bj->bs;
    out[TILESPMV_BJ_INFO_BLOCKS] = bj->blocks;
    out[TILESPMV_BJ_INFO_SINGULAR_BLOCKS] = singular;
    out[TILESPMV_BJ_INFO_DEVICE_BYTES] = (long long)bj->bytes;
    out[TILESPMV_BJ_INFO_DOT_PARTIALS] = bj->np;
    return 0;
}
