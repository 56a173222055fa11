// hip_solver_mv.hip — conjugate gradients on nvec systems in lock-step around the multi-vector product (tilespmv_cg_multi_*).
//
// The recurrences, sums, guards and ownership rules are those of hip_solver.hip, once per COLUMN: B, X, r, p, Ap are row-major [rows][NVEC] (the layout of tilespmv_plan_spmm),
// so the matrix is streamed once per iteration for all NVEC systems.  One iteration is that product and three streaming kernels, templated on NVEC in {2, 4, 8}:
//   k_cgm_dot        reads p, Ap                     partial sums of p.Ap, one per workgroup and column
//   k_cgm_update     reads p, Ap, x, r (, dinv)      alpha_c = rho_c / (p.Ap)_c;  x += alpha p;  r -= alpha Ap;  partial sums of r.r and (Jacobi) r.z per column
//   k_cgm_direction  reads r, p (, dinv)             beta_c = rho_new_c / rho_c;  p = z + beta p
// 11 rows NVEC vector elements per iteration (+ 2 rows of dinv with Jacobi: dinv is shared by the columns and read once per lane vector).
//
// The vectors are walked as flat streams of n = rows * NVEC elements in 16-byte lane vectors by the walk of hip_solver_common.h (SV_FOR_TRIPS); flat element e belongs to column
// e % NVEC.  A workgroup's trip stride (SV_U * SVB lane vectors), SVB and 64 are multiples of the lane vectors per row (LPR = NVEC / SV_VPL when NVEC >= SV_VPL), so a thread meets
// the same columns in every trip: (threadIdx.x % LPR) * SV_VPL + q for element q of its lane vectors.  In fp32 with NVEC = 2 a lane vector holds two rows and element q is column
// q % 2.  Either way a thread keeps KC = min(SV_VPL, NVEC) accumulators and as many alpha / beta, all indexed at compile time.
// Sums per column: the wave tree runs over the shuffle offsets 32 .. LPR (lanes LPR apart hold the same columns), the four wave sums are added in wave order through LDS, one
// partial per workgroup and column is written ([workgroup][NVEC]).  The consuming kernel folds the np * NVEC partials itself: thread t adds flat partials t, t + SVB, ... (all of
// column t % NVEC), the wave tree stops at offset NVEC, the four wave sums are added in wave order.  Every workgroup does the same additions in the same order; the number of
// partials (solver_parts(rows * NVEC), hip_solver_common.h) and every addition order are functions of (rows, NVEC) alone.  No atomics, no finishing launch, no occupancy query.
//
// The scalar block is one CgmScal per column; the fields of hip_solver.hip's CgScal keep their one writing kernel each (k_cgm_dot: rho; k_cgm_update: breakdown; k_cgm_direction:
// rr, iterations; k_cgm_begin_fold: all), and
//   frozen      k_cgm_freeze (one workgroup, launched by tilespmv_cg_multi_solve between two blocks of iterations; set), k_cgm_begin_fold (cleared)     read by k_cgm_dot, k_cgm_direction
// Under the flag k_cgm_dot hands out rho = 0 for the column, which is the rho = 0 guard: alpha = beta = 0, x and r keep their bits, and k_cgm_direction leaves its iteration count.
#include <hip/hip_runtime.h>

#include "hip_solver_common.h"

namespace tilespmv {
namespace {

constexpr int MAX_NVEC = TILESPMV_MAX_NVEC;

struct CgmScal {
    double rho, rr, bb;
    int iterations, breakdown, frozen, pad;
};

template <int NVEC> struct Cols {
    static constexpr int LPR = NVEC >= SV_VPL ? NVEC / SV_VPL : 1;   // lane vectors per row (1 when a lane vector holds whole rows)
    static constexpr int KC = NVEC >= SV_VPL ? SV_VPL : NVEC;        // columns a thread meets
    static constexpr int RPL = NVEC >= SV_VPL ? 1 : SV_VPL / NVEC;   // rows per lane vector
    // the first of this thread's KC consecutive columns
    static __device__ __forceinline__ int first() { return NVEC >= SV_VPL ? ((int)threadIdx.x % LPR) * SV_VPL : 0; }
};

// The workgroup's sums of the per-thread accumulators, by column: left in s[wave * NVEC + column], four values per column (col_total adds them).
template <int NVEC> __device__ __forceinline__ void block_cols(const double (&acc)[Cols<NVEC>::KC], double *s)
{
    constexpr int LPR = Cols<NVEC>::LPR, KC = Cols<NVEC>::KC;
    double w[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o >= LPR; o >>= 1) v += __shfl_down(v, o, 64);
        w[k] = v;
    }
    __syncthreads();   // (s may still be read from an earlier reduction)
    const int lane = threadIdx.x & 63;
    if (lane < LPR) {
#pragma unroll
        for (int k = 0; k < KC; k++) s[(threadIdx.x >> 6) * NVEC + lane * KC + k] = w[k];
    }
    __syncthreads();
}
// The sums of np partials per column ([np][nvec]), the same additions in every workgroup: left in s as by block_cols.
__device__ __forceinline__ void fold_cols(const double *__restrict__ part, int np, int nvec, double *s)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < np * nvec; i += SVB) a += part[i];
    for (int o = 32; o >= nvec; o >>= 1) a += __shfl_down(a, o, 64);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    if (lane < nvec) s[(threadIdx.x >> 6) * nvec + lane] = a;
    __syncthreads();
}
__device__ __forceinline__ double col_total(const double *s, int nvec, int c)
{
    return ((s[c] + s[nvec + c]) + s[2 * nvec + c]) + s[3 * nvec + c];
}
// one partial per workgroup and column
template <int NVEC> __device__ __forceinline__ void write_partials(const double *s, double *__restrict__ part)
{
    if (threadIdx.x < NVEC) part[(long long)blockIdx.x * NVEC + threadIdx.x] = col_total(s, NVEC, threadIdx.x);
}

// dinv of the rows of lane vector v, element for element: one scalar load when the lane vector lies within a row, an 8-byte pair in fp32 with NVEC = 2
template <int NVEC> __device__ __forceinline__ svec_t load_dinv(const val_t *__restrict__ dinv, long long v)
{
    svec_t d;
    if constexpr (Cols<NVEC>::RPL == 1) {
        d = dinv[v / Cols<NVEC>::LPR];
    } else {
        typedef val_t pair_t __attribute__((ext_vector_type(Cols<NVEC>::RPL)));
        const pair_t t = reinterpret_cast<const pair_t *>(dinv)[v];
#pragma unroll
        for (int q = 0; q < SV_VPL; q++) d[q] = t[q / NVEC];
    }
    return d;
}

// Element ranges as SV_FOR_TRIPS has them, over the flat stream; its n % SV_VPL tail elements (fp32, NVEC = 2, odd rows: one row) belong to thread 0 of workgroup 0, whose columns
// start at 0.

template <int NVEC>
__global__ __launch_bounds__(SVB) void k_cgm_dot(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, double *__restrict__ ppap, const double *__restrict__ prz,
                                                 int np, CgmScal *__restrict__ S)
{
    constexpr int KC = Cols<NVEC>::KC;
    __shared__ double s[(SVB / 64) * NVEC];
    const long long nv = n / SV_VPL;
    double acc[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) acc[k] = 0.0;
    SV_FOR_TRIPS(base, nv, gridDim.x) {
        svec_t a[SV_U], b[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) { a[u] = lanes(p)[v]; b[u] = lanes(Ap)[v]; }
            else { a[u] = (val_t)0; b[u] = (val_t)0; }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++)
#pragma unroll
            for (int q = 0; q < SV_VPL; q++) acc[q % KC] += (double)a[u][q] * (double)b[u][q];
    }
    if constexpr (NVEC < SV_VPL) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < KC; k++) {
                const long long i = nv * SV_VPL + k;
                if (i < n) acc[k] += (double)p[i] * (double)Ap[i];
            }
        }
    }
    block_cols<NVEC>(acc, s);
    write_partials<NVEC>(s, ppap);
    if (blockIdx.x == 0) {   // rho of this iteration, for the two kernels that follow
        fold_cols(prz, np, NVEC, s);
        if (threadIdx.x < NVEC) S[threadIdx.x].rho = (S[threadIdx.x].breakdown || S[threadIdx.x].frozen) ? 0.0 : col_total(s, NVEC, threadIdx.x);
    }
}

template <int NVEC>
__global__ __launch_bounds__(SVB) void k_cgm_update(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, val_t *__restrict__ x, val_t *__restrict__ r,
                                                    const val_t *__restrict__ dinv, const double *__restrict__ ppap, double *__restrict__ prr, double *__restrict__ prz, int np,
                                                    CgmScal *__restrict__ S)
{
    constexpr int KC = Cols<NVEC>::KC, LPR = Cols<NVEC>::LPR;
    __shared__ double s[(SVB / 64) * NVEC];
    const int c0 = Cols<NVEC>::first();
    fold_cols(ppap, np, NVEC, s);
    val_t alpha[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) {
        const double pap = col_total(s, NVEC, c0 + k), rho = S[c0 + k].rho;
        const bool broke = rho < 0.0 || (rho > 0.0 && !(pap > 0.0));
        alpha[k] = (val_t)((rho > 0.0 && pap > 0.0) ? rho / pap : 0.0);
        if (broke && blockIdx.x == 0 && threadIdx.x < LPR) S[c0 + k].breakdown = 1;   // (threads 0 .. LPR - 1 hold each column once)
    }
    svec_t av;
#pragma unroll
    for (int q = 0; q < SV_VPL; q++) av[q] = alpha[q % KC];
    const long long nv = n / SV_VPL;
    double arr[KC], arz[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) { arr[k] = 0.0; arz[k] = 0.0; }
    SV_FOR_TRIPS(base, nv, gridDim.x) {
        svec_t vp[SV_U], va[SV_U], vx[SV_U], vr[SV_U], vd[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) {
                vp[u] = lanes(p)[v]; va[u] = lanes(Ap)[v];
                vx[u] = lanes(x)[v]; vr[u] = lanes(r)[v];
                if (dinv) vd[u] = load_dinv<NVEC>(dinv, v);
            }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) {
                const svec_t nx = vx[u] + av * vp[u], nr = vr[u] - av * va[u];
                lanes(x)[v] = nx;
                lanes(r)[v] = nr;
#pragma unroll
                for (int q = 0; q < SV_VPL; q++) {
                    arr[q % KC] += (double)nr[q] * (double)nr[q];
                    if (dinv) arz[q % KC] += (double)nr[q] * (double)(val_t)(vd[u][q] * nr[q]);
                }
            }
        }
    }
    if constexpr (NVEC < SV_VPL) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < KC; k++) {
                const long long i = nv * SV_VPL + k;
                if (i < n) {
                    const val_t nr = r[i] - alpha[k] * Ap[i];
                    x[i] = x[i] + alpha[k] * p[i];
                    r[i] = nr;
                    arr[k] += (double)nr * (double)nr;
                    if (dinv) arz[k] += (double)nr * (double)(val_t)(dinv[i / NVEC] * nr);
                }
            }
        }
    }
    block_cols<NVEC>(arr, s);
    write_partials<NVEC>(s, prr);
    if (dinv) {   // (plain CG: r.z is r.r, and prz is prr)
        block_cols<NVEC>(arz, s);
        write_partials<NVEC>(s, prz);
    }
}

template <int NVEC>
__global__ __launch_bounds__(SVB) void k_cgm_direction(long long n, const val_t *__restrict__ r, val_t *__restrict__ p, const val_t *__restrict__ dinv,
                                                       const double *__restrict__ prr, const double *__restrict__ prz, int np, CgmScal *__restrict__ S)
{
    constexpr int KC = Cols<NVEC>::KC;
    __shared__ double s[(SVB / 64) * NVEC];
    const int c0 = Cols<NVEC>::first();
    fold_cols(prz, np, NVEC, s);
    val_t beta[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) {
        const double rho_new = col_total(s, NVEC, c0 + k), rho = S[c0 + k].rho;
        beta[k] = (val_t)((rho > 0.0 && !S[c0 + k].breakdown) ? rho_new / rho : 0.0);
    }
    if (blockIdx.x == 0) {   // what the host reads
        if (dinv) fold_cols(prr, np, NVEC, s);
        if (threadIdx.x < NVEC) {
            S[threadIdx.x].rr = col_total(s, NVEC, threadIdx.x);
            if (!S[threadIdx.x].frozen) S[threadIdx.x].iterations = S[threadIdx.x].iterations + 1;
        }
    }
    svec_t bv;
#pragma unroll
    for (int q = 0; q < SV_VPL; q++) bv[q] = beta[q % KC];
    const long long nv = n / SV_VPL;
    SV_FOR_TRIPS(base, nv, gridDim.x) {
        svec_t vr[SV_U], vp[SV_U], vd[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) {
                vr[u] = lanes(r)[v]; vp[u] = lanes(p)[v];
                if (dinv) vd[u] = load_dinv<NVEC>(dinv, v);
            }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) {
                const svec_t z = dinv ? vd[u] * vr[u] : vr[u];
                lanes(p)[v] = z + bv * vp[u];
            }
        }
    }
    if constexpr (NVEC < SV_VPL) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < KC; k++) {
                const long long i = nv * SV_VPL + k;
                if (i < n) p[i] = (dinv ? (val_t)(dinv[i / NVEC] * r[i]) : r[i]) + beta[k] * p[i];
            }
        }
    }
}

// the start of a solve: r = B - A X (AX holds the product), p = z, partial sums of r.r, r.z and b.b per column
template <int NVEC>
__global__ __launch_bounds__(SVB) void k_cgm_begin(long long n, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ r, val_t *__restrict__ p,
                                                   const val_t *__restrict__ dinv, double *__restrict__ prr, double *__restrict__ prz, double *__restrict__ pbb)
{
    constexpr int KC = Cols<NVEC>::KC;
    __shared__ double s[(SVB / 64) * NVEC];
    const long long nv = n / SV_VPL;
    double arr[KC], arz[KC], abb[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) { arr[k] = 0.0; arz[k] = 0.0; abb[k] = 0.0; }
    SV_FOR_TRIPS(base, nv, gridDim.x) {
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) {
                const svec_t vb = lanes(b)[v], nr = vb - lanes(Ax)[v];
                const svec_t z = dinv ? load_dinv<NVEC>(dinv, v) * nr : nr;
                lanes(r)[v] = nr;
                lanes(p)[v] = z;
#pragma unroll
                for (int q = 0; q < SV_VPL; q++) {
                    arr[q % KC] += (double)nr[q] * (double)nr[q];
                    arz[q % KC] += (double)nr[q] * (double)z[q];
                    abb[q % KC] += (double)vb[q] * (double)vb[q];
                }
            }
        }
    }
    if constexpr (NVEC < SV_VPL) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < KC; k++) {
                const long long i = nv * SV_VPL + k;
                if (i < n) {
                    const val_t nr = b[i] - Ax[i], z = dinv ? (val_t)(dinv[i / NVEC] * nr) : nr;
                    r[i] = nr; p[i] = z;
                    arr[k] += (double)nr * (double)nr; arz[k] += (double)nr * (double)z; abb[k] += (double)b[i] * (double)b[i];
                }
            }
        }
    }
    block_cols<NVEC>(arr, s);
    write_partials<NVEC>(s, prr);
    block_cols<NVEC>(abb, s);
    write_partials<NVEC>(s, pbb);
    if (dinv) {
        block_cols<NVEC>(arz, s);
        write_partials<NVEC>(s, prz);
    }
}
// ... and its scalars (one workgroup; prz is prr in plain CG)
__global__ __launch_bounds__(SVB) void k_cgm_begin_fold(const double *__restrict__ prr, const double *__restrict__ prz, const double *__restrict__ pbb, int np, int nvec,
                                                        CgmScal *__restrict__ S)
{
    __shared__ double s[(SVB / 64) * MAX_NVEC];
    const int c = threadIdx.x < nvec ? threadIdx.x : 0;
    fold_cols(prr, np, nvec, s);
    const double rr = col_total(s, nvec, c);
    fold_cols(prz, np, nvec, s);
    const double rz = col_total(s, nvec, c);
    fold_cols(pbb, np, nvec, s);
    const double bb = col_total(s, nvec, c);
    if (threadIdx.x < nvec) {
        CgmScal v;
        v.rho = rz; v.rr = rr; v.bb = bb; v.iterations = 0; v.breakdown = 0; v.frozen = 0; v.pad = 0;
        S[threadIdx.x] = v;
    }
}

// tilespmv_cg_multi_solve, between two blocks of iterations: the columns of `mask` are final
__global__ __launch_bounds__(64) void k_cgm_freeze(CgmScal *__restrict__ S, int nvec, unsigned mask)
{
    if (threadIdx.x < nvec && ((mask >> threadIdx.x) & 1u)) S[threadIdx.x].frozen = 1;
}
// ... and the columns of `mask` (b = 0) are 0
__global__ __launch_bounds__(SVB) void k_cgm_zero_columns(long long rows, int nvec, unsigned mask, val_t *__restrict__ x)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    for (int c = 0; c < nvec; c++)
        if ((mask >> c) & 1u) x[i * nvec + c] = (val_t)0;
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_cg_multi {
    tilespmv_plan *plan = nullptr;
    tilespmv_cg *single = nullptr;   // nvec = 1: tilespmv_cg_* itself
    long long rows = 0, n = 0;       // n = rows * nvec
    int nvec = 0, np = 0;
    const val_t *dinv = nullptr;     // borrowed
    void *block = nullptr;           // the one allocation: r, p, Ap, the partial-sum arrays, the scalar blocks
    val_t *r = nullptr, *p = nullptr, *Ap = nullptr;
    double *ppap = nullptr, *prr = nullptr, *prz = nullptr, *pbb = nullptr;
    CgmScal *S = nullptr;
};

namespace {

template <int NVEC> void launch_begin(const tilespmv_cg_multi *c, const val_t *B, hipStream_t st)
{
    hipLaunchKernelGGL(k_cgm_begin<NVEC>, dim3(c->np), dim3(SVB), 0, st, c->n, B, c->Ap, c->r, c->p, c->dinv, c->prr, c->prz, c->pbb);
}
template <int NVEC> void launch_iteration(const tilespmv_cg_multi *c, val_t *X, hipStream_t st)
{
    hipLaunchKernelGGL(k_cgm_dot<NVEC>, dim3(c->np), dim3(SVB), 0, st, c->n, c->p, c->Ap, c->ppap, c->prz, c->np, c->S);
    hipLaunchKernelGGL(k_cgm_update<NVEC>, dim3(c->np), dim3(SVB), 0, st, c->n, c->p, c->Ap, X, c->r, c->dinv, c->ppap, c->prr, c->prz, c->np, c->S);
    hipLaunchKernelGGL(k_cgm_direction<NVEC>, dim3(c->np), dim3(SVB), 0, st, c->n, c->r, c->p, c->dinv, c->prr, c->prz, c->np, c->S);
}

// the scalar blocks of all columns, after a synchronisation of the stream
int read_columns(const tilespmv_cg_multi *c, hipStream_t st, tilespmv_cg_state *cols /* [nvec], whole structs */)
{
    CgmScal h[MAX_NVEC];
    const hipError_t e = read_scalars(h, c->S, sizeof(CgmScal) * c->nvec, st);
    if (e != hipSuccess) return (int)e;
    for (int j = 0; j < c->nvec; j++) cols[j] = cg_state_of(h[j]);
    return 0;
}

}  // namespace

extern "C" int tilespmv_cg_multi_create(tilespmv_cg_multi **cg, tilespmv_plan *plan, int nvec, const MAT_VAL_TYPE *d_dinv)
{
    if (cg) *cg = nullptr;
    if (nvec != 1 && nvec != 2 && nvec != 4 && nvec != 8) return (int)hipErrorInvalidValue;   // (before the plan is touched)
    const long long rows = square_system(cg, plan, d_dinv);
    if (!rows) return (int)hipErrorInvalidValue;
    if (nvec == 1) {
        tilespmv_cg *one = nullptr;
        const int rc = tilespmv_cg_create(&one, plan, d_dinv);
        if (rc) return rc;
        auto *c = new tilespmv_cg_multi();
        c->plan = plan; c->single = one; c->rows = c->n = rows; c->nvec = 1;
        *cg = c;
        return 0;
    }
    int rc = tilespmv_plan_reserve_spmm(plan, nvec);   // plans that multiply one right-hand side at a time: their scratch now, so that iterate never allocates
    if (rc) return rc;
    const size_t vec = vec_bytes(rows, nvec), parts = SV_PARTS_BYTES * nvec, scal = ((size_t)nvec * sizeof(CgmScal) + 255) / 256 * 256;
    DeviceBlock blk;
    const hipError_t e = blk.alloc(3 * vec + 4 * parts + scal);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_cg_multi();
    c->plan = plan; c->rows = rows; c->nvec = nvec; c->n = rows * nvec; c->np = solver_parts(c->n); c->dinv = d_dinv; c->block = blk.base;
    c->r = blk.take<val_t>(vec);
    c->p = blk.take<val_t>(vec);
    c->Ap = blk.take<val_t>(vec);
    c->ppap = blk.take<double>(parts);
    c->prr = blk.take<double>(parts);
    double *const rz = blk.take<double>(parts);
    c->prz = d_dinv ? rz : c->prr;
    c->pbb = blk.take<double>(parts);
    c->S = blk.take<CgmScal>(scal);
    *cg = c;
    return 0;
}

extern "C" void tilespmv_cg_multi_destroy(tilespmv_cg_multi *cg)
{
    if (!cg) return;
    if (cg->single) tilespmv_cg_destroy(cg->single);
    if (cg->block) (void)hipFree(cg->block);
    delete cg;
}

extern "C" int tilespmv_cg_multi_begin(tilespmv_cg_multi *cg, const MAT_VAL_TYPE *d_B, MAT_VAL_TYPE *d_X, void *stream)
{
    if (!cg || !d_B || !d_X || misaligned(d_B) || misaligned(d_X)) return (int)hipErrorInvalidValue;
    if (cg->single) return tilespmv_cg_begin(cg->single, d_B, d_X, stream);
    const hipStream_t st = (hipStream_t)stream;
    const int rc = tilespmv_plan_spmm(cg->plan, d_X, cg->Ap, cg->nvec, stream);
    if (rc) return rc;
    switch (cg->nvec) {
    case 2: launch_begin<2>(cg, d_B, st); break;
    case 4: launch_begin<4>(cg, d_B, st); break;
    default: launch_begin<8>(cg, d_B, st); break;
    }
    hipLaunchKernelGGL(k_cgm_begin_fold, dim3(1), dim3(SVB), 0, st, cg->prr, cg->prz, cg->pbb, cg->np, cg->nvec, cg->S);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_cg_multi_iterate(tilespmv_cg_multi *cg, MAT_VAL_TYPE *d_X, int count, void *stream)
{
    if (!cg || !d_X || misaligned(d_X) || count < 0) return (int)hipErrorInvalidValue;
    if (cg->single) return tilespmv_cg_iterate(cg->single, d_X, count, stream);
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++) {
        const int rc = tilespmv_plan_spmm(cg->plan, cg->p, cg->Ap, cg->nvec, stream);
        if (rc) return rc;
        switch (cg->nvec) {
        case 2: launch_iteration<2>(cg, d_X, st); break;
        case 4: launch_iteration<4>(cg, d_X, st); break;
        default: launch_iteration<8>(cg, d_X, st); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int tilespmv_cg_multi_state_read(tilespmv_cg_multi *cg, void *stream, tilespmv_cg_state *out)
{
    if (!cg || !out || out->size < 3 * sizeof(int)) return (int)hipErrorInvalidValue;
    if (cg->single) return tilespmv_cg_state_read(cg->single, stream, out);
    tilespmv_cg_state cols[MAX_NVEC];
    const int rc = read_columns(cg, (hipStream_t)stream, cols);
    if (rc) return rc;
    const unsigned stride = out->size;
    for (int j = 0; j < cg->nvec; j++) put_versioned(out, stride, j, cols[j]);
    return 0;
}

extern "C" int tilespmv_cg_multi_solve(tilespmv_cg_multi *cg, const MAT_VAL_TYPE *d_B, MAT_VAL_TYPE *d_X, double rtol, int maxiter, int check_every, void *stream,
                                       tilespmv_cg_state *out)
{
    if (!cg || !out || out->size < sizeof(tilespmv_cg_state) || maxiter < 0) return (int)hipErrorInvalidValue;
    if (cg->single) return tilespmv_cg_solve(cg->single, d_B, d_X, rtol, maxiter, check_every, stream, out);
    if (check_every < 1) check_every = 1;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned stride = out->size, all = (1u << cg->nvec) - 1u;
    int rc = tilespmv_cg_multi_begin(cg, d_B, d_X, stream);
    if (rc) return rc;
    unsigned final_mask = 0;   // columns whose out[] entry stands: frozen on the device, they ride through the product and change no more
    int done = 0;              // iterations issued = the count of every column that still runs
    for (;;) {
        tilespmv_cg_state cols[MAX_NVEC];
        rc = read_columns(cg, st, cols);
        if (rc) return rc;
        unsigned fresh = 0, zero = 0;
        for (int j = 0; j < cg->nvec; j++) {
            const unsigned bit = 1u << j;
            if (final_mask & bit) continue;
            tilespmv_cg_state s = cols[j];
            if (s.status == TILESPMV_CG_BREAKDOWN) fresh |= bit;
            else if (s.bb == 0.0) { s.rr = 0.0; s.status = TILESPMV_CG_CONVERGED; fresh |= bit; zero |= bit; }   // b = 0: the solution is 0
            else if (s.rr <= rtol * rtol * s.bb) { s.status = TILESPMV_CG_CONVERGED; fresh |= bit; }
            else s.status = done >= maxiter ? TILESPMV_CG_MAXITER : TILESPMV_CG_RUNNING;
            put_versioned(out, stride, j, s);
        }
        final_mask |= fresh;
        const bool last = final_mask == all || done >= maxiter;
        if (fresh && !last) hipLaunchKernelGGL(k_cgm_freeze, dim3(1), dim3(64), 0, st, cg->S, cg->nvec, fresh);
        if (zero) hipLaunchKernelGGL(k_cgm_zero_columns, dim3((unsigned)((cg->rows + SVB - 1) / SVB)), dim3(SVB), 0, st, cg->rows, cg->nvec, zero, d_X);
        if ((fresh && !last) || zero) {
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        if (last) return zero ? (int)hipStreamSynchronize(st) : 0;
        const int k = std::min(check_every, maxiter - done);
        rc = tilespmv_cg_multi_iterate(cg, d_X, k, stream);
        if (rc) return rc;
        done += k;
    }
}
