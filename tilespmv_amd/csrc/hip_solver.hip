// hip_solver.hip — conjugate gradients around a resident plan (tilespmv_cg_*, tilespmv_csr_diagonal_device).
//
// One iteration is the plan's own product Ap = A p (tilespmv_plan_spmv: whatever launch form the plan has) and three streaming kernels:
//   k_cg_dot        reads p, Ap                     partial sums of p.Ap, one per workgroup
//   k_cg_update     reads p, Ap, x, r (, dinv)      alpha = rho / p.Ap;  x += alpha p;  r -= alpha Ap;  partial sums of r.r and (Jacobi) r.z, z = dinv o r
//   k_cg_direction  reads r, p (, dinv)             beta = rho_new / rho;  p = z + beta p  (z recomputed from r and dinv, never stored)
// 11 n vector elements per iteration (13 n with Jacobi).  No scalar ever visits the host: a reducing kernel writes one partial per workgroup and the CONSUMING kernel folds
// the partials itself — every workgroup the same additions in the same order, so all of them hold the same bits of alpha / beta; no finishing launch, no atomics.  The number
// of partials (cg_parts) and which elements a thread adds depend on n alone, the wave and workgroup reductions are fixed trees: the order of every sum is fixed by the problem size.
// Partial sums and scalars are double in both builds; alpha and beta are rounded to the value type once, where they multiply.
//
// The scalar block (CgScal) has ONE writing kernel per field and no kernel reads a field it (or a concurrent workgroup of it) writes:
//   rho         k_cg_dot, workgroup 0 (fold of the r.z partials the previous update left; 0 after a breakdown)      read by k_cg_update, k_cg_direction
//   breakdown   k_cg_update, workgroup 0 (set, never cleared)                                                        read by k_cg_dot (workgroup 0), k_cg_direction
//   rr, iterations   k_cg_direction, workgroup 0 (iterations: read and written by that workgroup alone)              read by the host (tilespmv_cg_state_read)
//   all of them      k_cg_begin_fold (one workgroup), at the start of a solve
// Guards (data-dependent branches, no host round trip): rho = 0 -> alpha = beta = 0, x and r stay as they are; rho > 0 and not p.Ap > 0 (or rho < 0: a preconditioner that is not
// positive definite) -> breakdown is set, alpha = beta = 0 in this and every later iteration, x keeps its last good value.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hip_plan_internal.h"

namespace tilespmv {
namespace {

constexpr int CGB = 256;                              // threads per workgroup
constexpr int CG_VPL = 16 / (int)sizeof(val_t);       // elements per 16-byte lane load (2 in fp64, 4 in fp32)
constexpr int CG_U = 2;                               // vectors per lane and trip: a workgroup's trip covers CG_U * CGB consecutive vectors
constexpr int CG_MAX_PARTS = 1024;                    // partial sums = workgroups of the streaming kernels: 4 per CU on 256 CUs
typedef val_t cvec_t __attribute__((ext_vector_type(CG_VPL)));

struct CgScal {
    double rho, rr, bb;
    int iterations, breakdown;
};

// workgroups (= partial sums) for n elements: a function of n alone
inline int cg_parts(long long n)
{
    const long long trips = (n / CG_VPL + (long long)CG_U * CGB - 1) / ((long long)CG_U * CGB);
    return (int)std::max<long long>(1, std::min<long long>(CG_MAX_PARTS, trips));
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// the workgroup's sum, returned to every thread: wave trees, then the four wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double *s)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((s[0] + s[1]) + s[2]) + s[3];
    __syncthreads();
    return t;
}
// the sum of np partials, the same additions in every workgroup
__device__ __forceinline__ double fold(const double *__restrict__ part, int np, double *s)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += CGB) a += part[i];
    return block_sum(a, s);
}

// Element ranges: full 16-byte vectors [0, nv) are walked in trips of CG_U * CGB by workgroup blockIdx.x, blockIdx.x + gridDim.x, ...; the n % CG_VPL elements behind them belong
// to thread 0 of workgroup 0 (scalar accesses: nothing past element n - 1 of a caller's vector is touched).
#define CG_FOR_TRIPS(base) for (long long base = (long long)blockIdx.x * (CG_U * CGB) + threadIdx.x; base < nv; base += (long long)gridDim.x * (CG_U * CGB))

__global__ __launch_bounds__(CGB) void k_cg_dot(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, double *__restrict__ ppap, const double *__restrict__ prz,
                                                int np, CgScal *__restrict__ S)
{
    __shared__ double s[CGB / 64];
    const long long nv = n / CG_VPL;
    double acc = 0.0;
    CG_FOR_TRIPS(base) {
        cvec_t a[CG_U], b[CG_U];
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) { a[u] = reinterpret_cast<const cvec_t *>(p)[v]; b[u] = reinterpret_cast<const cvec_t *>(Ap)[v]; }
            else { a[u] = (val_t)0; b[u] = (val_t)0; }
        }
#pragma unroll
        for (int u = 0; u < CG_U; u++)
#pragma unroll
            for (int q = 0; q < CG_VPL; q++) acc += (double)a[u][q] * (double)b[u][q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * CG_VPL; i < n; i++) acc += (double)p[i] * (double)Ap[i];
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) ppap[blockIdx.x] = t;
    if (blockIdx.x == 0) {   // rho of this iteration, for the two kernels that follow
        const double rho = fold(prz, np, s);
        if (threadIdx.x == 0) S->rho = S->breakdown ? 0.0 : rho;
    }
}

__global__ __launch_bounds__(CGB) void k_cg_update(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, val_t *__restrict__ x, val_t *__restrict__ r,
                                                   const val_t *__restrict__ dinv, const double *__restrict__ ppap, double *__restrict__ prr, double *__restrict__ prz, int np,
                                                   CgScal *__restrict__ S)
{
    __shared__ double s[CGB / 64];
    const double pap = fold(ppap, np, s), rho = S->rho;
    const bool broke = rho < 0.0 || (rho > 0.0 && !(pap > 0.0));
    const val_t alpha = (val_t)((rho > 0.0 && pap > 0.0) ? rho / pap : 0.0);
    if (broke && blockIdx.x == 0 && threadIdx.x == 0) S->breakdown = 1;
    const long long nv = n / CG_VPL;
    double arr = 0.0, arz = 0.0;
    CG_FOR_TRIPS(base) {
        cvec_t vp[CG_U], va[CG_U], vx[CG_U], vr[CG_U], vd[CG_U];
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) {
                vp[u] = reinterpret_cast<const cvec_t *>(p)[v]; va[u] = reinterpret_cast<const cvec_t *>(Ap)[v];
                vx[u] = reinterpret_cast<const cvec_t *>(x)[v]; vr[u] = reinterpret_cast<const cvec_t *>(r)[v];
                if (dinv) vd[u] = reinterpret_cast<const cvec_t *>(dinv)[v];
            }
        }
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) {
                const cvec_t nx = vx[u] + alpha * vp[u], nr = vr[u] - alpha * va[u];
                reinterpret_cast<cvec_t *>(x)[v] = nx;
                reinterpret_cast<cvec_t *>(r)[v] = nr;
#pragma unroll
                for (int q = 0; q < CG_VPL; q++) {
                    arr += (double)nr[q] * (double)nr[q];
                    if (dinv) arz += (double)nr[q] * (double)(val_t)(vd[u][q] * nr[q]);
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * CG_VPL; i < n; i++) {
            const val_t nr = r[i] - alpha * Ap[i];
            x[i] = x[i] + alpha * p[i];
            r[i] = nr;
            arr += (double)nr * (double)nr;
            if (dinv) arz += (double)nr * (double)(val_t)(dinv[i] * nr);
        }
    const double trr = block_sum(arr, s);
    if (threadIdx.x == 0) prr[blockIdx.x] = trr;
    if (dinv) {   // (plain CG: r.z is r.r, and prz is prr)
        const double trz = block_sum(arz, s);
        if (threadIdx.x == 0) prz[blockIdx.x] = trz;
    }
}

__global__ __launch_bounds__(CGB) void k_cg_direction(long long n, const val_t *__restrict__ r, val_t *__restrict__ p, const val_t *__restrict__ dinv,
                                                      const double *__restrict__ prr, const double *__restrict__ prz, int np, CgScal *__restrict__ S)
{
    __shared__ double s[CGB / 64];
    const double rho_new = fold(prz, np, s), rho = S->rho;
    const val_t beta = (val_t)((rho > 0.0 && !S->breakdown) ? rho_new / rho : 0.0);
    if (blockIdx.x == 0) {   // what the host reads
        const double rr = dinv ? fold(prr, np, s) : rho_new;
        if (threadIdx.x == 0) { S->rr = rr; S->iterations = S->iterations + 1; }
    }
    const long long nv = n / CG_VPL;
    CG_FOR_TRIPS(base) {
        cvec_t vr[CG_U], vp[CG_U], vd[CG_U];
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) {
                vr[u] = reinterpret_cast<const cvec_t *>(r)[v]; vp[u] = reinterpret_cast<const cvec_t *>(p)[v];
                if (dinv) vd[u] = reinterpret_cast<const cvec_t *>(dinv)[v];
            }
        }
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) {
                const cvec_t z = dinv ? vd[u] * vr[u] : vr[u];
                reinterpret_cast<cvec_t *>(p)[v] = z + beta * vp[u];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * CG_VPL; i < n; i++) p[i] = (dinv ? (val_t)(dinv[i] * r[i]) : r[i]) + beta * p[i];
}

// the start of a solve: r = b - A x (Ax holds the product), p = z, partial sums of r.r, r.z and b.b
__global__ __launch_bounds__(CGB) void k_cg_begin(long long n, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ r, val_t *__restrict__ p,
                                                  const val_t *__restrict__ dinv, double *__restrict__ prr, double *__restrict__ prz, double *__restrict__ pbb)
{
    __shared__ double s[CGB / 64];
    const long long nv = n / CG_VPL;
    double arr = 0.0, arz = 0.0, abb = 0.0;
    CG_FOR_TRIPS(base) {
#pragma unroll
        for (int u = 0; u < CG_U; u++) {
            const long long v = base + u * CGB;
            if (v < nv) {
                const cvec_t vb = reinterpret_cast<const cvec_t *>(b)[v], nr = vb - reinterpret_cast<const cvec_t *>(Ax)[v];
                const cvec_t z = dinv ? reinterpret_cast<const cvec_t *>(dinv)[v] * nr : nr;
                reinterpret_cast<cvec_t *>(r)[v] = nr;
                reinterpret_cast<cvec_t *>(p)[v] = z;
#pragma unroll
                for (int q = 0; q < CG_VPL; q++) {
                    arr += (double)nr[q] * (double)nr[q];
                    arz += (double)nr[q] * (double)z[q];
                    abb += (double)vb[q] * (double)vb[q];
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * CG_VPL; i < n; i++) {
            const val_t nr = b[i] - Ax[i], z = dinv ? (val_t)(dinv[i] * nr) : nr;
            r[i] = nr; p[i] = z;
            arr += (double)nr * (double)nr; arz += (double)nr * (double)z; abb += (double)b[i] * (double)b[i];
        }
    const double trr = block_sum(arr, s), trz = block_sum(arz, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) {
        prr[blockIdx.x] = trr; pbb[blockIdx.x] = tbb;
        if (dinv) prz[blockIdx.x] = trz;
    }
}
// ... and its scalars (one workgroup)
__global__ __launch_bounds__(CGB) void k_cg_begin_fold(const double *__restrict__ prr, const double *__restrict__ prz, const double *__restrict__ pbb, int np, CgScal *__restrict__ S)
{
    __shared__ double s[CGB / 64];
    const double rr = fold(prr, np, s), rz = fold(prz, np, s), bb = fold(pbb, np, s);
    if (threadIdx.x == 0) { S->rho = rz; S->rr = rr; S->bb = bb; S->iterations = 0; S->breakdown = 0; }
}

// one row per thread: the stored entries (i, i), added in storage order
__global__ __launch_bounds__(CGB) void k_csr_diagonal(int rows, const int *__restrict__ rp, const int *__restrict__ ci, const val_t *__restrict__ v, val_t *__restrict__ out, int invert)
{
    const long long i = (long long)blockIdx.x * CGB + threadIdx.x;
    if (i >= rows) return;
    double a = 0.0;
    for (long long k = rp[i]; k < rp[i + 1]; k++)
        if (ci[k] == (int)i) a += (double)v[k];
    const val_t d = (val_t)a;
    out[i] = !invert ? d : d == (val_t)0 ? (val_t)1 : (val_t)1 / d;
}

inline bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_cg {
    tilespmv_plan *plan = nullptr;
    long long n = 0;
    int np = 0;
    const val_t *dinv = nullptr;   // borrowed
    void *block = nullptr;         // the one allocation: r, p, Ap, the partial-sum arrays, the scalar block
    val_t *r = nullptr, *p = nullptr, *Ap = nullptr;
    double *ppap = nullptr, *prr = nullptr, *prz = nullptr, *pbb = nullptr;
    CgScal *S = nullptr;
};

extern "C" int tilespmv_cg_create(tilespmv_cg **cg, tilespmv_plan *plan, const MAT_VAL_TYPE *d_dinv)
{
    if (cg) *cg = nullptr;
    if (!cg || !plan) return (int)hipErrorInvalidValue;
    const long long n = plan->matrix_rows;
    if (n <= 0 || plan->dev.colA != n || plan->dev.f_row0 != 0 || plan->dev.f_rows != n) return (int)hipErrorInvalidValue;   // square, whole matrix
    if (misaligned(d_dinv)) return (int)hipErrorInvalidValue;
    const size_t vec = ((size_t)(n + 16) * sizeof(val_t) + 255) / 256 * 256, parts = (size_t)CG_MAX_PARTS * sizeof(double);
    const size_t bytes = 3 * vec + 4 * parts + 256;
    void *blk = nullptr;
    hipError_t e = hipMalloc(&blk, bytes);
    if (e == hipSuccess) e = hipMemset(blk, 0, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (blk) (void)hipFree(blk);
        return (int)e;
    }
    auto *c = new tilespmv_cg();
    c->plan = plan; c->n = n; c->np = cg_parts(n); c->dinv = d_dinv; c->block = blk;
    char *at = (char *)blk;
    c->r = (val_t *)at; at += vec;
    c->p = (val_t *)at; at += vec;
    c->Ap = (val_t *)at; at += vec;
    c->ppap = (double *)at; at += parts;
    c->prr = (double *)at; at += parts;
    c->prz = d_dinv ? (double *)at : c->prr; at += parts;
    c->pbb = (double *)at; at += parts;
    c->S = (CgScal *)at;
    *cg = c;
    return 0;
}

extern "C" void tilespmv_cg_destroy(tilespmv_cg *cg)
{
    if (!cg) return;
    (void)hipFree(cg->block);
    delete cg;
}

extern "C" int tilespmv_cg_begin(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!cg || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = tilespmv_plan_spmv(cg->plan, d_x, cg->Ap, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cg_begin, dim3(cg->np), dim3(CGB), 0, st, cg->n, d_b, cg->Ap, cg->r, cg->p, cg->dinv, cg->prr, cg->prz, cg->pbb);
    hipLaunchKernelGGL(k_cg_begin_fold, dim3(1), dim3(CGB), 0, st, cg->prr, cg->prz, cg->pbb, cg->np, cg->S);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_cg_iterate(tilespmv_cg *cg, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!cg || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++) {
        const int rc = tilespmv_plan_spmv(cg->plan, cg->p, cg->Ap, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cg_dot, dim3(cg->np), dim3(CGB), 0, st, cg->n, cg->p, cg->Ap, cg->ppap, cg->prz, cg->np, cg->S);
        hipLaunchKernelGGL(k_cg_update, dim3(cg->np), dim3(CGB), 0, st, cg->n, cg->p, cg->Ap, d_x, cg->r, cg->dinv, cg->ppap, cg->prr, cg->prz, cg->np, cg->S);
        hipLaunchKernelGGL(k_cg_direction, dim3(cg->np), dim3(CGB), 0, st, cg->n, cg->r, cg->p, cg->dinv, cg->prr, cg->prz, cg->np, cg->S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int tilespmv_cg_state_read(tilespmv_cg *cg, void *stream, tilespmv_cg_state *out)
{
    if (!cg || !out || out->size < 3 * sizeof(int)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    CgScal h;
    hipError_t e = hipMemcpyAsync(&h, cg->S, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    tilespmv_cg_state s;
    s.size = out->size;
    s.iterations = h.iterations;
    s.status = h.breakdown ? TILESPMV_CG_BREAKDOWN : h.rr == 0.0 ? TILESPMV_CG_CONVERGED : TILESPMV_CG_RUNNING;
    s.rr = h.rr; s.bb = h.bb;
    memcpy(out, &s, std::min<size_t>(out->size, sizeof(s)));   // (a caller built against a shorter struct gets the fields it knows)
    return 0;
}

extern "C" int tilespmv_cg_solve(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                                 tilespmv_cg_state *out)
{
    if (!cg || !out || out->size < sizeof(tilespmv_cg_state) || maxiter < 0) return (int)hipErrorInvalidValue;
    if (check_every < 1) check_every = 1;
    int rc = tilespmv_cg_begin(cg, d_b, d_x, stream);
    if (rc) return rc;
    for (;;) {
        rc = tilespmv_cg_state_read(cg, stream, out);
        if (rc) return rc;
        if (out->status == TILESPMV_CG_BREAKDOWN) return 0;
        if (out->bb == 0.0) {   // b = 0: the solution is 0
            const hipError_t e = hipMemsetAsync(d_x, 0, (size_t)cg->n * sizeof(val_t), (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
            out->rr = 0.0; out->status = TILESPMV_CG_CONVERGED;
            return (int)hipStreamSynchronize((hipStream_t)stream);
        }
        if (out->rr <= rtol * rtol * out->bb) { out->status = TILESPMV_CG_CONVERGED; return 0; }
        if (out->iterations >= maxiter) { out->status = TILESPMV_CG_MAXITER; return 0; }
        rc = tilespmv_cg_iterate(cg, d_x, std::min(check_every, maxiter - out->iterations), stream);
        if (rc) return rc;
    }
}

extern "C" int tilespmv_csr_diagonal_device(int rows, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_VAL_TYPE *d_out, int invert,
                                            void *stream)
{
    if (rows < 0 || (rows > 0 && (!d_csrRowPtr || !d_csrColIdx || !d_csrVal || !d_out))) return (int)hipErrorInvalidValue;
    if (tilespmv_device_count() <= 0) return (int)hipErrorNoDevice;
    if (rows > 0)
        hipLaunchKernelGGL(k_csr_diagonal, dim3((unsigned)((rows + CGB - 1) / CGB)), dim3(CGB), 0, (hipStream_t)stream, rows, d_csrRowPtr, d_csrColIdx, d_csrVal, d_out, invert);
    return (int)hipGetLastError();
}
