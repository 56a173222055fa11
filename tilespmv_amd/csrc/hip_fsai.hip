// hip_fsai.hip — a factorised sparse approximate inverse preconditioner for the CG solver (tilespmv_fsai_*).
//
// G is sparse and lower triangular on the pattern of A's lower triangle with G A G^T ~ I (Kolotilina-Yeremin); M^-1 = G^T G.  Row i of G holds the stored columns <= i of row i of
// A, the TILESPMV_FSAI_MAX_ROW nearest the diagonal where there are more.  With P those m columns, S = A[P, P] (read from the lower triangle of A alone) and S y = e_m,
// row i of G is y / sqrt(y_m): row i of G A G^T then has a unit diagonal.  The object holds G as a CSR and two value-mapped plans of it (G, and G^T through
// TILESPMV_CREATE_TRANSPOSE); z = G^T (G r) is two products.  The kernels:
//   k_fsai_rows     one thread per row of A: the input's promise (row pointer inside [0, nnz] and ascending, columns strictly ascending and < rows, a stored diagonal), the
//                   length of the row of G, where its pattern starts in A's arrays; integer atomics for the flag, the longest row and the truncated rows.
//   k_fsai_fill     one thread per row: the column indices of G.
//   k_fsai_values   <M>, M = 8, 16, 32, 48, 64 >= the longest row of G: one-wavefront workgroups, a group of M lanes per row and 64 / M rows per wavefront up to M = 32, one
//                   row per wavefront above (M = 48: 19 KB of LDS where M = 64 takes 34 KB — twice the wavefronts per CU for the 42-entry rows of a 3-dof hexahedral mesh).
//                   S is assembled in LDS in double (both builds), M rows of M + 1 doubles (the odd stride in doubles puts the rows of a column on different banks): lane j
//                   walks the lower part of row P[j] of A from its diagonal leftwards down to column P[0], FS_BATCH entries per trip with their loads issued together, and
//                   finds each column in P[0 .. j] by a binary search of a fixed number of steps; only the lower triangle of S is written, the factorisation reads nothing else.  S = L L^T column by column (left-looking), lane = row: at step k every lane from k
//                   on forms the dot product of its row of L with row k over the columns before k (j ascending, in a register: the inner loop only loads) and the sum of
//                   squares of row k, hence the pivot; lane k keeps the pivot's root in a separate array (the diagonal of S stays, the others read it in the same step), the
//                   lanes below write their entry of column k; one barrier per step.  L^T y = e_m / L_mm by columns: lane k forms y_k, a shuffle hands it to the lanes left
//                   of it.  g = y / sqrt(y_m), rounded to the value type once.  The loops run to the longest row of the wavefront, so that every lane reaches every barrier
//                   and every shuffle.  A pivot that is not > 0 or not finite (the last lane of the row sees every pivot): the row of G is that of point Jacobi (zeros,
//                   1 / sqrt(a_ii) on the diagonal where a_ii > 0, 1 otherwise) and the device counter is incremented (an integer atomic: its value does not depend on the order).
//   k_fsai_dot      the partial sums of r.z, sv_dot's walk (hip_solver_common.h): solver_parts(rows) of them, their number and the order of every addition fixed by `rows`.
// No atomics on values, every sum in a fixed order: two runs give the same bytes.  No kernel uses scratch.
#include <hip/hip_runtime.h>

#include <climits>

#include "hip_fsai.h"
#include "hip_prims.h"

namespace tilespmv {
namespace {

constexpr int FS_MAX = TILESPMV_FSAI_MAX_ROW;
constexpr int FS_BATCH = 8;                             // entries of a row of A that a lane of k_fsai_values loads at a time
enum { FS_BAD = 0, FS_LONGEST = 1, FS_TRUNCATED = 2, FS_FALLBACK = 3, FS_COUNTERS = 4 };
static_assert(FS_MAX == 64, "a row of G is served by the lanes of one wavefront");
static_assert(TILESPMV_FSAI_MAX_PARTIALS == SV_MAX_PARTS, "the header's bound on the partials");

__global__ __launch_bounds__(SVB) void k_fsai_rows(int rows, int nnz, const int *__restrict__ rp, const int *__restrict__ ci, int *__restrict__ len, int *__restrict__ first,
                                                   int *__restrict__ counters)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    const int a = rp[i], b = rp[i + 1];
    bool ok = a >= 0 && b >= a && b <= nnz && (i != 0 || a == 0) && (i != rows - 1 || b == nnz);
    int diag = -1;
    if (ok) {
        int prev = -1;
        for (int e = a; e < b; e++) {
            const int c = ci[e];
            if (c <= prev || c >= rows) ok = false;
            if (c == (int)i) diag = e;
            prev = c;
        }
    }
    if (!ok || diag < 0) {
        len[i] = 0; first[i] = 0;
        atomicOr(&counters[FS_BAD], 1);
        return;
    }
    const int lower = diag - a + 1, m = min(lower, FS_MAX);
    len[i] = m;
    first[i] = diag - m + 1;
    if (m > __atomic_load_n(&counters[FS_LONGEST], __ATOMIC_RELAXED)) atomicMax(&counters[FS_LONGEST], m);
    if (lower > FS_MAX) atomicAdd(&counters[FS_TRUNCATED], 1);
}

__global__ __launch_bounds__(SVB) void k_fsai_fill(int rows, const int *__restrict__ ci, const int *__restrict__ gp, const int *__restrict__ first, int *__restrict__ gci)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    const int g0 = gp[i], m = gp[i + 1] - g0, e0 = first[i];
    for (int j = 0; j < m; j++) gci[g0 + j] = ci[e0 + j];
}

template <int M>
__global__ __launch_bounds__(64) void k_fsai_values(long long rows, const int *__restrict__ rp, const int *__restrict__ ci, const val_t *__restrict__ v, const int *__restrict__ gp,
                                                    const int *__restrict__ first, const int *__restrict__ gci, val_t *__restrict__ gval, int *__restrict__ fallback)
{
    constexpr int W = M <= 32 ? M : 64;   // lanes of a group: the power of two that holds M (M = 48: the lanes from 48 on have no row of S)
    constexpr int LD = M + 1, GROUPS = 64 / W;
    __shared__ double sm[GROUPS][M][LD];
    __shared__ double dg[GROUPS][M];
    __shared__ int pat[GROUPS][M];
    const int grp = threadIdx.x / W, l = threadIdx.x % W;
    const long long i = (long long)blockIdx.x * GROUPS + grp;
    const int g0 = i < rows ? gp[i] : 0, m = i < rows ? gp[i + 1] - g0 : 0;   // (a group behind the last row: no row, m = 0; m <= M, so a lane from M on is never below m)
    double(*S)[LD] = sm[grp];
    double *D = dg[grp];
    int *P = pat[grp];
    int mmax = m;   // the longest row of the wavefront (every lane of a group holds its m)
#pragma unroll
    for (int o = 32; o >= W; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o, 64));
    // lane = row of S: zeros in the lower triangle, then the entries of row P[l] of A whose columns are in P
    if (l < M) P[l] = l < m ? gci[g0 + l] : INT_MAX;
    if (l < m)
#pragma unroll 1
        for (int c = 0; c <= l; c++) S[l][c] = 0.0;
    __syncthreads();
    if (l < m) {
        const int c = P[l], p0 = P[0], lo = rp[c];
        // from the diagonal of row c leftwards, FS_BATCH entries at a time: their loads are issued together (positions left of the row's start are clamped to it and skipped),
        // and their searches are independent of each other
        for (int e = first[c] + (gp[c + 1] - gp[c]) - 1; e >= lo; e -= FS_BATCH) {
            int q[FS_BATCH];
            double w[FS_BATCH];
#pragma unroll
            for (int u = 0; u < FS_BATCH; u++) {
                const int at = max(e - u, lo);
                q[u] = ci[at];
                w[u] = (double)v[at];
            }
#pragma unroll
            for (int u = 0; u < FS_BATCH; u++) {
                if (e - u < lo || q[u] < p0) continue;
                int a = 0;   // the number of pattern columns below q[u] among P[0 .. l - 1] (q[u] <= c = P[l]), in a fixed number of steps
#pragma unroll
                for (int s = W / 2; s >= 1; s >>= 1)
                    if (a + s <= l && P[a + s - 1] < q[u]) a += s;
                if (P[a] == q[u]) S[l][a] = w[u];
            }
            if (q[FS_BATCH - 1] < p0) break;   // (ascending columns: everything further left is smaller still)
        }
    }
    __syncthreads();
    // S = L L^T, column by column: L below the diagonal in place, the diagonal of L in D (the diagonal of S stays: every lane from k on reads it at step k)
    const int last = max(m - 1, 0);
    bool bad = false;   // (lane `last` takes part in every step: it sees every pivot)
#pragma unroll 1
    for (int k = 0; k < mmax; k++) {
        if (k < m && l >= k && l < m) {
            double ad = 0.0, ar = 0.0;
#pragma unroll 4
            for (int j = 0; j < k; j++) {
                const double lk = S[k][j];
                ad += lk * lk;
                ar += S[l][j] * lk;
            }
            const double d = S[k][k] - ad;
            bad = bad || !(d > 0.0) || !isfinite(d);
            const double piv = sqrt(d);
            if (l == k) D[k] = piv;
            else S[l][k] = (S[l][k] - ar) / piv;
        }
        __syncthreads();
    }
    bad = __shfl((int)bad, last, W) != 0;
    // L^T y = e_m / L_mm by columns, from the last one
    double acc = (m > 0 && l == last) ? 1.0 / D[last] : 0.0, y = 0.0;
#pragma unroll 1
    for (int k = mmax - 1; k >= 0; k--) {
        const bool in = k < m;
        const double yk = __shfl((in && l == k) ? acc / D[k] : 0.0, k, W);
        if (l == k) y = yk;
        if (in && l < k) acc -= S[k][l] * yk;
    }
    const double ym = __shfl(y, last, W);
    if (l < m) {
        double g = y / sqrt(ym);
        if (bad) {
            const double aii = (double)v[first[i] + m - 1];
            g = l != last ? 0.0 : aii > 0.0 ? 1.0 / sqrt(aii) : 1.0;
        }
        gval[g0 + l] = (val_t)g;
    }
    if (bad && l == 0 && m > 0) atomicAdd(fallback, 1);
}

__global__ __launch_bounds__(SVB) void k_fsai_dot(long long n, const val_t *__restrict__ r, const val_t *__restrict__ z, double *__restrict__ prz)
{
    __shared__ double s[SVB / 64];
    double acc = 0.0;
    sv_dot(n, gridDim.x, r, z, [&](auto a, auto b) { sv_mac(acc, a, b); });
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) prz[blockIdx.x] = t;
}

template <int M> void launch_values(const tilespmv_fsai *f, const int *rp, const int *ci, const val_t *v, hipStream_t st)
{
    const long long per_wg = M <= 32 ? 64 / M : 1;
    hipLaunchKernelGGL(k_fsai_values<M>, dim3((unsigned)((f->rows + per_wg - 1) / per_wg)), dim3(64), 0, st, f->rows, rp, ci, v, f->gp, f->first, f->gci, f->gval,
                       f->counters + FS_FALLBACK);
}

// the values of G from the values of A, into f->gval: the counter of the fallback rows is rewritten
hipError_t values(const tilespmv_fsai *f, const int *rp, const int *ci, const val_t *v, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(f->counters + FS_FALLBACK, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    if (f->longest <= 8) launch_values<8>(f, rp, ci, v, st);
    else if (f->longest <= 16) launch_values<16>(f, rp, ci, v, st);
    else if (f->longest <= 32) launch_values<32>(f, rp, ci, v, st);
    else if (f->longest <= 48) launch_values<48>(f, rp, ci, v, st);
    else launch_values<64>(f, rp, ci, v, st);
    return hipGetLastError();
}

unsigned row_blocks(long long rows) { return (unsigned)((rows + SVB - 1) / SVB); }

}  // namespace

int fsai_launch(tilespmv_fsai *f, const val_t *r, val_t *z, double *prz, hipStream_t st)
{
    int rc = tilespmv_plan_spmv(f->G, r, f->t, (void *)st);
    if (rc == 0) rc = tilespmv_plan_spmv(f->GT, f->t, z, (void *)st);
    if (rc != 0 || !prz) return rc;
    hipLaunchKernelGGL(k_fsai_dot, dim3(f->np), dim3(SVB), 0, st, f->rows, r, (const val_t *)z, prz);
    return (int)hipGetLastError();
}

}  // namespace tilespmv

using namespace tilespmv;

extern "C" void tilespmv_fsai_destroy(tilespmv_fsai *f)
{
    if (!f) return;
    if (f->G) tilespmv_plan_destroy(f->G);
    if (f->GT) tilespmv_plan_destroy(f->GT);
    if (f->values) (void)hipFree(f->values);
    if (f->pattern) (void)hipFree(f->pattern);
    delete f;
}

extern "C" int tilespmv_fsai_create(tilespmv_fsai **out, int rows, MAT_PTR_TYPE nnz, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal,
                                    const tilespmv_plan_options *opts, void *stream)
{
    if (out) *out = nullptr;
    if (!out || rows <= 0 || nnz <= 0 || !d_csrRowPtr || !d_csrColIdx || !d_csrVal) return (int)hipErrorInvalidValue;
    if (tilespmv_device_count() <= 0) return (int)hipErrorNoDevice;
    const hipStream_t st = (hipStream_t)stream;
    const size_t rp_bytes = ((size_t)(rows + 1) * sizeof(int) + 255) / 256 * 256, first_bytes = ((size_t)rows * sizeof(int) + 255) / 256 * 256;
    DeviceBlock pat;
    hipError_t e = pat.alloc(rp_bytes + first_bytes + 256);
    if (e != hipSuccess) return (int)e;
    auto *f = new tilespmv_fsai();
    f->rows = rows; f->np = solver_parts(rows); f->pattern = pat.base;
    f->gp = pat.take<int>(rp_bytes);
    f->first = pat.take<int>(first_bytes);
    f->counters = pat.take<int>(256);
    f->bytes = rp_bytes + first_bytes + 256;
    void *scan_tmp = nullptr;
    const auto fail = [&](int rc) {
        (void)hipGetLastError();
        if (scan_tmp) (void)hipFree(scan_tmp);
        tilespmv_fsai_destroy(f);
        return rc;
    };
    // the promise, the lengths of G's rows (gp[rows] = 0 from the allocation), their exclusive scan in place
    size_t scan_b = 0;
    e = prims::scan_int(nullptr, scan_b, f->gp, f->gp, (size_t)rows + 1, st);
    if (e == hipSuccess) e = hipMalloc(&scan_tmp, std::max<size_t>(scan_b, 16));
    if (e != hipSuccess) return fail((int)e);
    hipLaunchKernelGGL(k_fsai_rows, dim3(row_blocks(rows)), dim3(SVB), 0, st, rows, (int)nnz, d_csrRowPtr, d_csrColIdx, f->gp, f->first, f->counters);
    e = hipGetLastError();
    if (e == hipSuccess) e = prims::scan_int(scan_tmp, scan_b, f->gp, f->gp, (size_t)rows + 1, st);
    int counters[FS_COUNTERS] = {0, 0, 0, 0}, gnnz = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&gnnz, f->gp + rows, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = read_scalars(counters, f->counters, sizeof(counters), st);
    if (e != hipSuccess) return fail((int)e);
    (void)hipFree(scan_tmp);
    scan_tmp = nullptr;
    if (counters[FS_BAD] || gnnz <= 0) return fail((int)hipErrorInvalidValue);
    f->gnnz = gnnz; f->longest = counters[FS_LONGEST]; f->truncated = counters[FS_TRUNCATED];
    const size_t ci_bytes = ((size_t)gnnz * sizeof(int) + 255) / 256 * 256, val_bytes = ((size_t)gnnz * sizeof(val_t) + 255) / 256 * 256;
    DeviceBlock val;
    e = val.alloc(ci_bytes + val_bytes + vec_bytes(rows));
    if (e != hipSuccess) return fail((int)e);
    f->values = val.base;
    f->gci = val.take<int>(ci_bytes);
    f->gval = val.take<val_t>(val_bytes);
    f->t = val.take<val_t>(vec_bytes(rows));
    f->bytes += ci_bytes + val_bytes + vec_bytes(rows);
    hipLaunchKernelGGL(k_fsai_fill, dim3(row_blocks(rows)), dim3(SVB), 0, st, rows, d_csrColIdx, f->gp, f->first, f->gci);
    e = hipGetLastError();
    if (e == hipSuccess) e = values(f, d_csrRowPtr, d_csrColIdx, d_csrVal, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the plan builders work on their own streams)
    if (e != hipSuccess) return fail((int)e);
    const unsigned flags = TILESPMV_CREATE_QUIET | TILESPMV_CREATE_VALUE_MAP;
    int rc = tilespmv_plan_create_from_device_csr(&f->G, rows, rows, gnnz, f->gp, f->gci, f->gval, flags, opts);
    if (rc == 0) rc = tilespmv_plan_create_from_device_csr(&f->GT, rows, rows, gnnz, f->gp, f->gci, f->gval, flags | TILESPMV_CREATE_TRANSPOSE, opts);
    if (rc != 0 || !f->G || !f->GT) return fail(rc ? rc : (int)hipErrorUnknown);
    *out = f;
    return 0;
}

extern "C" int tilespmv_fsai_update(tilespmv_fsai *f, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, void *stream)
{
    if (!f || !d_csrRowPtr || !d_csrColIdx || !d_csrVal) return (int)hipErrorInvalidValue;
    const hipError_t e = values(f, d_csrRowPtr, d_csrColIdx, d_csrVal, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const int rc = tilespmv_plan_update_values(f->G, f->gval, stream);
    return rc ? rc : tilespmv_plan_update_values(f->GT, f->gval, stream);
}

static int fsai_apply(tilespmv_fsai *f, const val_t *d_r, val_t *d_z, double *d_partials, bool dot, void *stream)
{
    if (!f || !d_r || !d_z || d_r == d_z || misaligned(d_r) || misaligned(d_z) || (dot && !d_partials)) return (int)hipErrorInvalidValue;
    return fsai_launch(f, d_r, d_z, dot ? d_partials : nullptr, (hipStream_t)stream);
}

extern "C" int tilespmv_fsai_apply(tilespmv_fsai *f, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, void *stream) { return fsai_apply(f, d_r, d_z, nullptr, false, stream); }

extern "C" int tilespmv_fsai_apply_dot(tilespmv_fsai *f, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, double *d_partials, void *stream)
{
    return fsai_apply(f, d_r, d_z, d_partials, true, stream);
}

extern "C" int tilespmv_fsai_factor_csr(const tilespmv_fsai *f, const MAT_PTR_TYPE **d_rowPtr, const int **d_colIdx, const MAT_VAL_TYPE **d_val, MAT_PTR_TYPE *nnz)
{
    if (!f || !d_rowPtr || !d_colIdx || !d_val || !nnz) return (int)hipErrorInvalidValue;
    *d_rowPtr = f->gp; *d_colIdx = f->gci; *d_val = f->gval; *nnz = (MAT_PTR_TYPE)f->gnnz;
    return 0;
}

extern "C" int tilespmv_fsai_info(const tilespmv_fsai *f, void *stream, long long *out)
{
    if (!f || !out) return (int)hipErrorInvalidValue;
    int fallback = 0;
    const hipError_t e = read_scalars(&fallback, f->counters + FS_FALLBACK, sizeof(fallback), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    long long bytes = (long long)f->bytes, info[TILESPMV_INFO_COUNT];
    for (const tilespmv_plan *p : {f->G, f->GT}) {
        tilespmv_plan_info(p, info);
        bytes += info[TILESPMV_INFO_DEVICE_BYTES] + info[TILESPMV_INFO_VALUE_MAP_BYTES];
    }
    out[TILESPMV_FSAI_INFO_ROWS] = f->rows;
    out[TILESPMV_FSAI_INFO_NNZ] = f->gnnz;
    out[TILESPMV_FSAI_INFO_LONGEST_ROW] = f->longest;
    out[TILESPMV_FSAI_INFO_TRUNCATED_ROWS] = f->truncated;
    out[TILESPMV_FSAI_INFO_FALLBACK_ROWS] = fallback;
    out[TILESPMV_FSAI_INFO_DEVICE_BYTES] = bytes;
    out[TILESPMV_FSAI_INFO_DOT_PARTIALS] = f->np;
    return 0;
}
