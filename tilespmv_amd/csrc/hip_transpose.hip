// hip_transpose.hip — A^T of a CSR on the device (tilespmv_csr_transpose_device, and the TILESPMV_CREATE_TRANSPOSE paths of Tile_create_device and the device plan builders;
// DESIGN.md §3.6).  The definition is tilespmv_csr_transpose's (include/tilespmv.h): A's entries in CSR order, stably sorted by column.
//   1. column histogram into rpT (int atomics), the (column, position) pairs written beside it
//   2. exclusive scan of the counts in place (prims::scan_int): rpT
//   3. ONE stable radix sort of the pairs over ceil(log2(colA)) key bits (prims::sort_pairs_u32_int — the instantiation hip_plan_device.hip already uses)
//   4. the row of every entry (binary search of the row pointer, written into the key buffer the sort no longer needs)
//   5. gathers: ciT[k] = row of entry order[k], vT[k] = v[order[k]], srcT[k] = base + order[k]
// Scratch: two key and two position buffers (16 bytes per nonzero) + the sort's temporary storage; allocated here and freed before returning (the call synchronises).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hip_prims.h"
#include "hip_tile_create.h"

namespace tilespmv {
namespace {

constexpr int TB = 256;
inline unsigned tr_blocks(long long n) { return (unsigned)std::max<long long>(1, (n + TB - 1) / TB); }

// the column counts and the sort's input pairs; a column outside [0, colA) sets *bad and counts nowhere (its pair is sorted as column 0: the output is garbage, never out of bounds)
__global__ __launch_bounds__(TB) void k_tr_hist(long long nnz, const int *__restrict__ ci0, int colA, int *__restrict__ cnt, unsigned *__restrict__ key, int *__restrict__ pos,
                                                int *__restrict__ bad)
{
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= nnz) return;
    int c = ci0[i];
    if (c < 0 || c >= colA) { atomicOr(bad, 1); c = 0; }
    else atomicAdd(cnt + c, 1);
    key[i] = (unsigned)c;
    pos[i] = (int)i;
}

// a decreasing row pointer sets *bad
__global__ __launch_bounds__(TB) void k_tr_check_rp(int rowA, const int *__restrict__ rp, int *__restrict__ bad)
{
    const long long r = (long long)blockIdx.x * TB + threadIdx.x;
    if (r < rowA && rp[r + 1] < rp[r]) atomicOr(bad, 1);
}

// row of entry i (position base + i): the last r with rp[r] <= base + i.  Neighbouring threads walk the same path of the search: their loads coalesce
__global__ __launch_bounds__(TB) void k_tr_rowid(long long nnz, int rowA, const int *__restrict__ rp, long long base, int *__restrict__ rowid)
{
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= nnz) return;
    const long long at = base + i;
    int lo = 0, hi = rowA;   // invariant: rp[lo] <= at < rp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)rp[mid] <= at) lo = mid; else hi = mid;
    }
    rowid[i] = lo;
}

__global__ __launch_bounds__(TB) void k_tr_gather(long long nnz, const int *__restrict__ order, const int *__restrict__ rowid, const val_t *__restrict__ v0, long long base,
                                                  int *__restrict__ ciT, val_t *__restrict__ vT, int *__restrict__ srcT)
{
    const long long k = (long long)blockIdx.x * TB + threadIdx.x;
    if (k >= nnz) return;
    const int j = order[k];
    ciT[k] = rowid[j];
    if (vT) vT[k] = v0[j];
    if (srcT) srcT[k] = (int)(base + j);
}

}  // namespace

hipError_t csr_transpose_dev(int rowA, int colA, const int *rp, long long base, long long nnz, const int *ci0, const val_t *v0, int *rpT, int *ciT, val_t *vT, int *srcT,
                             hipStream_t st)
{
    hipError_t e = hipMemsetAsync(rpT, 0, ((size_t)colA + 1) * sizeof(int), st);
    if (e != hipSuccess || nnz == 0) return e == hipSuccess ? hipStreamSynchronize(st) : e;
    unsigned bits = 0;
    while (bits < 31 && (1ll << bits) < (long long)colA) bits++;
    bits = std::max(bits, 1u);
    unsigned *key_a = nullptr, *key_b = nullptr; int *pos_a = nullptr, *pos_b = nullptr, *bad = nullptr;
    void *sort_tmp = nullptr, *scan_tmp = nullptr;
    size_t sort_b = 0, scan_b = 0;
    unsigned *k_cur, *k_alt; int *p_cur, *p_alt;
    auto done = [&](hipError_t r) {
        for (void *q : {(void *)key_a, (void *)key_b, (void *)pos_a, (void *)pos_b, (void *)bad, sort_tmp, scan_tmp}) if (q) (void)hipFree(q);
        if (r != hipSuccess) (void)hipGetLastError();
        return r;
    };
    e = hipMalloc((void **)&key_a, (size_t)nnz * sizeof(unsigned));
    if (e == hipSuccess) e = hipMalloc((void **)&key_b, (size_t)nnz * sizeof(unsigned));
    if (e == hipSuccess) e = hipMalloc((void **)&pos_a, (size_t)nnz * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&pos_b, (size_t)nnz * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&bad, sizeof(int));
    k_cur = key_a; k_alt = key_b; p_cur = pos_a; p_alt = pos_b;
    if (e == hipSuccess) e = prims::sort_pairs_u32_int(nullptr, sort_b, k_cur, k_alt, p_cur, p_alt, (size_t)nnz, 0u, bits, st);
    if (e == hipSuccess) e = prims::scan_int(nullptr, scan_b, rpT, rpT, (size_t)colA + 1, st);
    if (e == hipSuccess) e = hipMalloc(&sort_tmp, std::max<size_t>(sort_b, 16));
    if (e == hipSuccess) e = hipMalloc(&scan_tmp, std::max<size_t>(scan_b, 16));
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e != hipSuccess) return done(e);
    hipLaunchKernelGGL(k_tr_hist, dim3(tr_blocks(nnz)), dim3(TB), 0, st, nnz, ci0, colA, rpT, key_a, pos_a, bad);
    hipLaunchKernelGGL(k_tr_check_rp, dim3(tr_blocks(rowA)), dim3(TB), 0, st, rowA, rp, bad);
    e = hipGetLastError();
    if (e == hipSuccess) e = prims::scan_int(scan_tmp, scan_b, rpT, rpT, (size_t)colA + 1, st);
    if (e == hipSuccess) e = prims::sort_pairs_u32_int(sort_tmp, sort_b, k_cur, k_alt, p_cur, p_alt, (size_t)nnz, 0u, bits, st);
    if (e != hipSuccess) return done(e);
    int *rowid = reinterpret_cast<int *>(k_cur);   // (the sorted keys are not needed: rpT holds the column boundaries)
    hipLaunchKernelGGL(k_tr_rowid, dim3(tr_blocks(nnz)), dim3(TB), 0, st, nnz, rowA, rp, base, rowid);
    hipLaunchKernelGGL(k_tr_gather, dim3(tr_blocks(nnz)), dim3(TB), 0, st, nnz, p_cur, rowid, v0, base, ciT, v0 ? vT : nullptr, srcT);
    e = hipGetLastError();
    int h_bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h_bad) e = hipErrorInvalidValue;
    return done(e);
}

DevCsrT::~DevCsrT()
{
    for (void *q : {(void *)rp, (void *)ci, (void *)src, (void *)v, (void *)valA}) if (q) (void)hipFree(q);
}

int devcsr_transpose(DevCsrT *T, int rowA, int colA, const int *rp, const int *ci, const val_t *v, bool csr_on_device, bool want_values, bool want_src, bool keep_values_of_a)
{
    long long base = 0, nnz = 0;
    if (csr_on_device) {
        int ends[2] = {0, 0};
        if (hipMemcpy(&ends[0], rp, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&ends[1], rp + rowA, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError(); return -3;
        }
        base = ends[0]; nnz = (long long)ends[1] - base;
    } else { base = rp[0]; nnz = (long long)rp[rowA] - base; }
    if (base < 0 || nnz < 0) { fprintf(stderr, "tilespmv: transpose: the row pointer decreases\n"); return -3; }
    T->rows = colA; T->cols = rowA; T->base = base; T->nnz = nnz;
    const size_t n1 = (size_t)std::max<long long>(nnz, 1);
    int *d_rp = nullptr, *d_ci = nullptr; val_t *d_v = nullptr;   // A on the device: the caller's arrays, or uploaded ones (block positions: entry j at index j - base)
    hipError_t e = hipMalloc((void **)&T->rp, ((size_t)colA + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&T->ci, n1 * sizeof(int));
    if (e == hipSuccess && want_src) e = hipMalloc((void **)&T->src, n1 * sizeof(int));
    if (e == hipSuccess && want_values) e = hipMalloc((void **)&T->v, n1 * sizeof(val_t));
    const val_t *v0 = nullptr;
    const int *ci0 = nullptr;
    if (e == hipSuccess) {
        if (csr_on_device) { d_rp = const_cast<int *>(rp); ci0 = ci + base; v0 = want_values ? v + base : nullptr; }
        else {
            e = hipMalloc((void **)&d_rp, ((size_t)rowA + 1) * sizeof(int));
            if (e == hipSuccess) e = hipMalloc((void **)&d_ci, n1 * sizeof(int));
            if (e == hipSuccess && (want_values || keep_values_of_a)) e = hipMalloc((void **)&d_v, n1 * sizeof(val_t));
            if (e == hipSuccess) e = hipMemcpy(d_rp, rp, ((size_t)rowA + 1) * sizeof(int), hipMemcpyHostToDevice);
            if (e == hipSuccess && nnz) e = hipMemcpy(d_ci, ci + base, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice);
            if (e == hipSuccess && nnz && d_v) e = hipMemcpy(d_v, v + base, (size_t)nnz * sizeof(val_t), hipMemcpyHostToDevice);
            ci0 = d_ci; v0 = want_values ? d_v : nullptr;
        }
    }
    if (e == hipSuccess) e = csr_transpose_dev(rowA, colA, d_rp, base, nnz, ci0, v0, T->rp, T->ci, T->v, T->src, (hipStream_t)0);
    if (!csr_on_device) {
        if (d_rp) (void)hipFree(d_rp);
        if (d_ci) (void)hipFree(d_ci);
        if (d_v && keep_values_of_a && e == hipSuccess) T->valA = d_v;
        else if (d_v) (void)hipFree(d_v);
    }
    if (e != hipSuccess) {
        fprintf(stderr, "tilespmv: transpose on the device: %s%s\n", hipGetErrorString(e), e == hipErrorInvalidValue ? " (a column index outside [0, colA) or a decreasing row pointer?)" : "");
        (void)hipGetLastError();
        return -3;
    }
    return 0;
}

}  // namespace tilespmv

extern "C" int tilespmv_csr_transpose_device(int rowA, int colA, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_PTR_TYPE *d_rowPtrT,
                                             int *d_colIdxT, MAT_VAL_TYPE *d_valT, int *d_srcT, void *stream)
{
    if (rowA < 0 || colA < 0 || !d_csrRowPtr || !d_rowPtrT) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    int ends[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(&ends[0], d_csrRowPtr, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], d_csrRowPtr + rowA, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    const long long base = ends[0], nnz = (long long)ends[1] - base;
    if (base < 0 || nnz < 0) return (int)hipErrorInvalidValue;
    if (nnz > 0 && (!d_csrColIdx || !d_colIdxT || (d_valT && !d_csrVal))) return (int)hipErrorInvalidValue;
    return (int)tilespmv::csr_transpose_dev(rowA, colA, d_csrRowPtr, base, nnz, d_csrColIdx ? d_csrColIdx + base : nullptr, d_valT ? d_csrVal + base : nullptr, d_rowPtrT,
                                            d_colIdxT, d_valT, d_srcT, st);
}
