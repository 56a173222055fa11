// hip_solver_gm.hip — restarted GMRES for square nonsymmetric systems around a resident plan (tilespmv_gmres_*).
//
// Right-preconditioned GMRES(m), m = restart, M^-1 = diag(dinv) (Jacobi; dinv = NULL: zhat = V_j) or a block-Jacobi object.  The orthogonalisation is classical Gram-Schmidt applied
// twice: a pass needs all of its dot products before it can subtract, so each pass is two streaming kernels whatever j is (modified Gram-Schmidt: j + 1 dependent reductions), and
// the second pass is what keeps the fp32 build orthogonal.  One inner iteration with k = j + 1 basis vectors is the plan product w = A zhat (tilespmv_plan_spmv) and FOUR kernels:
//   k_gm_dots    reads w, V_0..V_j                              partial sums of h1 = V^T w, one per sum and workgroup
//   k_gm_orth1   reads w, V_0..V_j; folds h1                    w' = w - V h1, stored over w;  partial sums of h2 = V^T w'
//   k_gm_orth2   reads w', V_0..V_j; folds h2                   w'' = w' - V h2, stored over w';  partial sums of |w''|^2
//   k_gm_next    reads w''; folds the norm                      V_{j+1} = w'' / h_{j+1,j} (, zhat = dinv o V_{j+1});  workgroup 0: column j of the Hessenberg matrix (h1 + h2,
//                                                               h_{j+1,j}), the j stored Givens rotations applied to it, the new rotation, g, rr, j, the iteration count
// A cycle is CLOSED by k_gm_solve (one workgroup: R y = g by back substitution in double, R and g staged in LDS) and k_gm_update (x += dinv o sum_i y_i V_i; with a block object
// u = sum_i y_i V_i, k_bj_apply, k_gm_axpy) and OPENED by the product A x, k_gm_resid (r = b - A x with the partial sums of r.r) and k_gm_next in its open role (V_0 = r / beta,
// g_0 = beta, j = 0).  After an open rr is a recomputed |b - A x|^2.
// Vector elements read or written per inner iteration beside the product, BY COUNT, with each basis vector counted once per kernel: 3 k + 7 (dots k + 1 | orth1 k + 2 | orth2
// k + 2 | next 2), 3 k + 9 with dinv (its read and the store of zhat in k_gm_next); the mean over a full cycle is 1.5 (restart + 1) + 7.  With a block object zhat comes from
// k_bj_apply after k_gm_next (bs + 2 more).  A close moves k + 2 (+ 1 with dinv), an open 3 + 2 beside its product.
// WHAT THE REGISTERS ADD TO THAT COUNT: a thread cannot hold 65 double accumulators (an array indexed by a loop variable is scratch memory), so the dot products run over the basis
// in groups of GM_GROUP = 8 vectors whose accumulators are named registers, and every group walks w again: ceil(k / 8) - 1 re-reads of w in k_gm_dots and in k_gm_orth1.  In
// k_gm_orth1 the dot products need the finished w', so its second phase reads V again (k more) and w' ceil(k / 8) times.  A thread reads back only what it stored itself; the
// re-reads of w come out of the cache while a workgroup's share of w fits there.  By count with the re-reads: 4 k + 2 ceil(k / 8) + 6.
// THE FOLD: a consumer folds k sums, not one: every workgroup reads k P doubles, all of them 8 k P^2 bytes out of the cache, where the kernel's vectors are k B bytes (B = the
// bytes of one vector).  These kernels have their own workgroup count P = gm_parts(rows), a function of rows alone: at most 256 up to B = 32 MiB, 512 up to 128 MiB, 1024 beyond —
// the fold, 8 P^2 / B of the vector traffic, is at most 1/16 from B = 8 MiB on (1 M rows in fp64, where 1024 partials would read as much as the vectors) and 1/4 at worst, at
// 2 MiB, where a kernel is bound by its launch.  MEASURED (scripts/gmres_time.py, profiles/gmres_fused_ab.txt): with 256 workgroups everywhere a 16.8 M-row fp64 system took 3.14 ms per inner iteration of GMRES(30),
// with 1024 there 1.96 ms — one workgroup per CU does not keep enough loads in flight.  A fold is done by the four waves in turn, each sum by one wave in a fixed order: the same
// bits in every workgroup, no finishing launch, no atomics.
// The scalar tail, block_sum and the walk over a vector are those of hip_solver_common.h: k_gm_next, k_gm_resid and k_gm_axpy hand their body to sv_walk; gm_group_dots, gm_subtract
// and k_gm_update loop over the basis inside a trip and write SV_FOR_TRIPS and the tail out.  h1_i, h2_i, 1 / h_{j+1,j}, 1 / beta and y_i are formed in double and rounded to the value
// type once, where they multiply.
//
// The scalar block (GmScal) and the small arrays have ONE writing kernel per field, and no kernel reads a field that it (or a concurrent workgroup of it) writes:
//   jc, act                         k_gm_dots, workgroup 0 (the column of this iteration and whether it runs: live, no breakdown, j < restart)
//                                                                                                  read by k_gm_orth1, k_gm_orth2, k_gm_next
//   j, live, rr, iterations, breakdown, R, cs, sn, g   k_gm_next, workgroup 0 (iterations, breakdown, R, cs, sn, g: read and written by that workgroup alone; breakdown is set, never
//                                   cleared; the open role writes j = 0, live, rr, g_0 and reads breakdown)
//                                                                                                  read by k_gm_dots, k_gm_solve, k_gm_update, k_gm_axpy, the host (rr, iterations, breakdown)
//   y                               k_gm_solve                                                     read by k_gm_update
//   bb, and iterations = 0, breakdown = 0   k_gm_begin_fold (one workgroup), at the start of a solve
// Guards (exact tests, data-dependent uniform branches, no host round trip):
//   rr = 0 at an open, or the breakdown flag      the cycle is not live: inner iterations and the close write no vector, x keeps its bits
//   h_{j+1,j} = 0 with gamma != 0                 the lucky termination: the rotation is applied (rr = 0), V_{j+1} is not formed, the cycle is closed early (live = 0, j counts the
//                                                 columns done); the close uses them
//   gamma = 0                                     breakdown; nothing is written in this or any later iteration or close, x keeps its last good value
//   j = restart without a close in between        (a replayed graph, misused) the iteration writes nothing: the column index never passes restart
// The iteration counter advances in every inner iteration whatever the guards did.
#include <hip/hip_runtime.h>

#include "hip_precond.h"
#include "hip_solver_common.h"

namespace tilespmv {
namespace {

constexpr int GM_MAX_RESTART = TILESPMV_GMRES_MAX_RESTART;
constexpr int GM_MAX_PARTS = 256;     // workgroups (= partials per sum) of these kernels for vectors below 32 MiB (gm_parts)
constexpr int GM_GROUP = 8;           // basis vectors whose dot products a thread accumulates at a time

struct GmScal {
    double rr, bb;
    int iterations, breakdown;
    int j, live;      // columns done in this cycle; the cycle takes further columns
    int jc, act;      // this iteration's column; it runs
};

// Workgroups (= partials per sum) of these kernels, a function of rows alone.  A fold of k sums reads 8 k P^2 bytes over all P workgroups, the kernel's vectors k B bytes, B = the
// bytes of one vector: P = 256 up to B = 32 MiB, 512 up to 128 MiB, 1024 beyond keeps the fold at or below 1/16 of the vector traffic from B = 8 MiB on.
inline int gm_parts(long long rows)
{
    const long long bytes = rows * (long long)sizeof(val_t);
    const int cap = bytes >= (128ll << 20) ? 4 * GM_MAX_PARTS : bytes >= (32ll << 20) ? 2 * GM_MAX_PARTS : GM_MAX_PARTS;
    return std::min(cap, solver_parts(rows));
}

// k sums of np partials each (sum i at part + i * np) into hs[0 .. k): sum i by wave i % 4, every lane its partials in ascending order, then the wave tree
__device__ __forceinline__ void fold_many(const double *__restrict__ part, int np, int k, double *hs)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = wave; i < k; i += SVB / 64) {
        double a = 0.0;
        for (int p = lane; p < np; p += 64) a += part[(size_t)i * np + p];
        a = wave_sum(a);
        if (lane == 0) hs[i] = a;
    }
    __syncthreads();
}

// partial sums of CNT dot products w.V_c, V_c = Vg + c * stride, one per workgroup at pd[c * np + blockIdx.x]
template <int CNT>
__device__ __forceinline__ void gm_group_dots(long long n, const val_t *w, const val_t *Vg, long long stride, double *pd, int np, double *s)
{
    const long long nv = n / SV_VPL;
    double acc[CNT];
#pragma unroll
    for (int c = 0; c < CNT; c++) acc[c] = 0.0;
    SV_FOR_TRIPS(base, nv, gridDim.x) {
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long i = base + u * SVB;
            if (i < nv) {
                const svec_t a = lanes(w)[i];
                svec_t v[CNT];
#pragma unroll
                for (int c = 0; c < CNT; c++) v[c] = lanes(Vg + c * stride)[i];
#pragma unroll
                for (int c = 0; c < CNT; c++)
#pragma unroll
                    for (int q = 0; q < SV_VPL; q++) acc[c] += (double)a[q] * (double)v[c][q];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++)
#pragma unroll
            for (int c = 0; c < CNT; c++) acc[c] += (double)w[i] * (double)Vg[c * stride + i];
#pragma unroll
    for (int c = 0; c < CNT; c++) {
        const double t = block_sum(acc[c], s);
        if (threadIdx.x == 0) pd[(size_t)c * np + blockIdx.x] = t;
    }
}

// partial sums of w.V_i for i < k, in groups of GM_GROUP
__device__ __forceinline__ void gm_dots(long long n, const val_t *w, const val_t *V, long long stride, int k, double *pd, int np, double *s)
{
    int c0 = 0;
    for (; c0 + GM_GROUP <= k; c0 += GM_GROUP) gm_group_dots<GM_GROUP>(n, w, V + c0 * stride, stride, pd + (size_t)c0 * np, np, s);
    const val_t *Vg = V + c0 * stride;
    double *pg = pd + (size_t)c0 * np;
    switch (k - c0) {
    case 1: gm_group_dots<1>(n, w, Vg, stride, pg, np, s); break;
    case 2: gm_group_dots<2>(n, w, Vg, stride, pg, np, s); break;
    case 3: gm_group_dots<3>(n, w, Vg, stride, pg, np, s); break;
    case 4: gm_group_dots<4>(n, w, Vg, stride, pg, np, s); break;
    case 5: gm_group_dots<5>(n, w, Vg, stride, pg, np, s); break;
    case 6: gm_group_dots<6>(n, w, Vg, stride, pg, np, s); break;
    case 7: gm_group_dots<7>(n, w, Vg, stride, pg, np, s); break;
    default: break;
    }
}

// w -= sum_{c < k} h_c V_c, c ascending, h_c = hs[c] rounded to the value type; returns the thread's share of |w|^2 of the new w
__device__ __forceinline__ double gm_subtract(long long n, val_t *w, const val_t *V, long long stride, int k, const double *hs)
{
    const long long nv = n / SV_VPL;
    double acc = 0.0;
    SV_FOR_TRIPS(base, nv, gridDim.x) {
        svec_t a[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long i = base + u * SVB;
            if (i < nv) a[u] = lanes(w)[i];
            else a[u] = (val_t)0;
        }
#pragma unroll 4
        for (int c = 0; c < k; c++) {
            const val_t h = (val_t)hs[c];
            const val_t *Vc = V + c * stride;
#pragma unroll
            for (int u = 0; u < SV_U; u++) {
                const long long i = base + u * SVB;
                if (i < nv) a[u] -= h * lanes(Vc)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long i = base + u * SVB;
            if (i < nv) {
                lanes(w)[i] = a[u];
#pragma unroll
                for (int q = 0; q < SV_VPL; q++) acc += (double)a[u][q] * (double)a[u][q];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) {
            val_t a = w[i];
            for (int c = 0; c < k; c++) a -= (val_t)hs[c] * V[c * stride + i];
            w[i] = a;
            acc += (double)a * (double)a;
        }
    return acc;
}

__global__ __launch_bounds__(SVB) void k_gm_dots(long long n, const val_t *w, const val_t *V, long long stride, double *pd1, int np, int restart, GmScal *S)
{
    __shared__ double s[SVB / 64];
    const int j = S->j;
    const bool act = S->live && !S->breakdown && j >= 0 && j < restart;
    if (blockIdx.x == 0 && threadIdx.x == 0) { S->jc = j; S->act = act ? 1 : 0; }   // for the three kernels that follow
    if (!act) return;
    gm_dots(n, w, V, stride, j + 1, pd1, np, s);
}

__global__ __launch_bounds__(SVB) void k_gm_orth1(long long n, val_t *w, const val_t *V, long long stride, const double *__restrict__ pd1, double *pd2, int np, const GmScal *S)
{
    __shared__ double s[SVB / 64];
    __shared__ double hs[GM_MAX_RESTART + 1];
    if (!S->act) return;
    const int k = S->jc + 1;
    fold_many(pd1, np, k, hs);
    (void)gm_subtract(n, w, V, stride, k, hs);
    gm_dots(n, w, V, stride, k, pd2, np, s);      // (every thread reads back the elements of w' it stored itself)
}

__global__ __launch_bounds__(SVB) void k_gm_orth2(long long n, val_t *w, const val_t *V, long long stride, const double *__restrict__ pd2, double *__restrict__ pnorm, int np,
                                                  const GmScal *S)
{
    __shared__ double s[SVB / 64];
    __shared__ double hs[GM_MAX_RESTART + 1];
    if (!S->act) return;
    const int k = S->jc + 1;
    fold_many(pd2, np, k, hs);
    const double t = block_sum(gm_subtract(n, w, V, stride, k, hs), s);
    if (threadIdx.x == 0) pnorm[blockIdx.x] = t;
}


// The end of an inner iteration (open = 0): V_{j+1} = w'' / h_{j+1,j} (, zhat = dinv o V_{j+1}) and workgroup 0's scalars.  The end of an open (open = 1): rr = |r|^2 whatever the
// flags say, V_0 = r / beta (, zhat), g_0 = beta, j = 0.
__global__ __launch_bounds__(SVB) void k_gm_next(long long n, const val_t *__restrict__ w, val_t *__restrict__ V, long long stride, const val_t *__restrict__ dinv,
                                                 val_t *__restrict__ zhat, const double *__restrict__ pd1, const double *__restrict__ pd2, const double *__restrict__ pnorm, int np,
                                                 int open, GmScal *S, double *__restrict__ R, double *__restrict__ cs, double *__restrict__ sn, double *__restrict__ g)
{
    __shared__ double s[SVB / 64];
    __shared__ double h1[GM_MAX_RESTART + 1], h2[GM_MAX_RESTART + 1];
    const bool run = open || S->act;
    const int jc = open ? -1 : S->jc;
    const double nrm2 = run ? fold(pnorm, np, s) : 0.0;
    const double hh = sqrt(nrm2);
    const bool form = run && hh != 0.0 && !(open && S->breakdown);
    if (blockIdx.x == 0) {
        if (open) {
            if (threadIdx.x == 0) { S->rr = nrm2; S->j = 0; S->live = form ? 1 : 0; g[0] = hh; }
        } else {
            if (run) {
                fold_many(pd1, np, jc + 1, h1);
                fold_many(pd2, np, jc + 1, h2);
            }
            if (threadIdx.x == 0) {
                if (run) {
                    for (int i = 0; i <= jc; i++) h1[i] += h2[i];
                    for (int i = 0; i < jc; i++) {   // the stored rotations
                        const double a = h1[i], b = h1[i + 1];
                        h1[i] = cs[i] * a + sn[i] * b;
                        h1[i + 1] = -sn[i] * a + cs[i] * b;
                    }
                    const double gamma = hypot(h1[jc], hh);
                    if (gamma == 0.0) {
                        S->breakdown = 1;
                        S->live = 0;
                    } else {
                        const double c = h1[jc] / gamma, sg = hh / gamma, gj = g[jc];
                        for (int i = 0; i < jc; i++) R[i + GM_MAX_RESTART * jc] = h1[i];
                        R[jc + GM_MAX_RESTART * jc] = gamma;
                        cs[jc] = c; sn[jc] = sg;
                        const double gn = -sg * gj;
                        g[jc + 1] = gn; g[jc] = c * gj;
                        S->rr = gn * gn;
                        S->j = jc + 1;
                        if (hh == 0.0) S->live = 0;   // the lucky termination: closed early
                    }
                }
                S->iterations = S->iterations + 1;
            }
        }
    }
    if (!form) return;
    const val_t scale = (val_t)(1.0 / hh);
    val_t *__restrict__ Vn = V + (long long)(jc + 1) * stride;
    sv_walk(n, gridDim.x, [&](auto at) {
        const auto v = scale * at(w);
        at.put(Vn, v);
        if (dinv) at.put(zhat, at(dinv) * v);
    });
}

// r = b - A x over the product (w holds A x) with the partial sums of r.r; at the start of a solve (bcopy != NULL) also the solver's copy of b and the partial sums of b.b
__global__ __launch_bounds__(SVB) void k_gm_resid(long long n, const val_t *__restrict__ b, val_t *__restrict__ bcopy, val_t *__restrict__ w, double *__restrict__ pnorm,
                                                  double *__restrict__ pbb)
{
    __shared__ double s[SVB / 64];
    double arr = 0.0, abb = 0.0;
    sv_walk(n, gridDim.x, [&](auto at) {
        const auto vb = at(b), nr = vb - at(w);
        at.put(w, nr);
        if (bcopy) at.put(bcopy, vb);
        sv_mac(arr, nr, nr);
        sv_mac(abb, vb, vb);
    });
    const double trr = block_sum(arr, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) {
        pnorm[blockIdx.x] = trr;
        if (pbb) pbb[blockIdx.x] = tbb;
    }
}
// ... and the scalars of the start of a solve (one workgroup)
__global__ __launch_bounds__(SVB) void k_gm_begin_fold(const double *__restrict__ pbb, int np, GmScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double bb = fold(pbb, np, s);
    if (threadIdx.x == 0) { S->bb = bb; S->iterations = 0; S->breakdown = 0; }
}

// the columns a close uses: none after a breakdown
__device__ __forceinline__ int gm_close_columns(const GmScal *S, int restart) { return S->breakdown ? 0 : min(max(S->j, 0), restart); }

// R y = g for the k columns done (one workgroup): column i gives y_i = g_i / R_ii, then g_t -= R_ti y_i for t < i, i descending — R (column-major) and g staged in LDS
__global__ __launch_bounds__(SVB) void k_gm_solve(const double *__restrict__ R, const double *__restrict__ g, double *__restrict__ y, int restart, const GmScal *__restrict__ S)
{
    __shared__ double Rs[GM_MAX_RESTART * GM_MAX_RESTART];
    __shared__ double gs[GM_MAX_RESTART];
    const int k = gm_close_columns(S, restart);
    if (k == 0) return;
    for (int i = threadIdx.x; i < k * GM_MAX_RESTART; i += SVB) Rs[i] = R[i];
    if ((int)threadIdx.x < k) gs[threadIdx.x] = g[threadIdx.x];
    __syncthreads();
    for (int i = k - 1; i >= 0; i--) {
        if (threadIdx.x == 0) gs[i] = gs[i] / Rs[i + GM_MAX_RESTART * i];
        __syncthreads();
        if ((int)threadIdx.x < i) gs[threadIdx.x] -= Rs[threadIdx.x + GM_MAX_RESTART * i] * gs[i];
        __syncthreads();
    }
    if ((int)threadIdx.x < k) y[threadIdx.x] = gs[threadIdx.x];
}

// u = sum_{i < k} y_i V_i, i ascending;  out != NULL: stored there (the block object's apply follows), else x += dinv o u (dinv = NULL: x += u)
__global__ __launch_bounds__(SVB) void k_gm_update(long long n, val_t *__restrict__ x, const val_t *__restrict__ V, long long stride, const val_t *__restrict__ dinv,
                                                   const double *__restrict__ y, val_t *__restrict__ out, int restart, const GmScal *__restrict__ S)
{
    __shared__ val_t ys[GM_MAX_RESTART];
    const int k = gm_close_columns(S, restart);
    if (k == 0) return;
    if ((int)threadIdx.x < k) ys[threadIdx.x] = (val_t)y[threadIdx.x];
    __syncthreads();
    const long long nv = n / SV_VPL;
    SV_FOR_TRIPS(base, nv, gridDim.x) {
        svec_t a[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) a[u] = (val_t)0;
#pragma unroll 4
        for (int c = 0; c < k; c++) {
            const val_t yc = ys[c];
            const val_t *Vc = V + c * stride;
#pragma unroll
            for (int u = 0; u < SV_U; u++) {
                const long long i = base + u * SVB;
                if (i < nv) a[u] += yc * lanes(Vc)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long i = base + u * SVB;
            if (i < nv) {
                if (out) lanes(out)[i] = a[u];
                else lanes(x)[i] = lanes(x)[i] + (dinv ? lanes(dinv)[i] * a[u] : a[u]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) {
            val_t a = (val_t)0;
            for (int c = 0; c < k; c++) a += ys[c] * V[c * stride + i];
            if (out) out[i] = a;
            else x[i] = x[i] + (dinv ? dinv[i] * a : a);
        }
}

// x += z under the guards of a close (z = M^-1 u of a block object)
__global__ __launch_bounds__(SVB) void k_gm_axpy(long long n, val_t *__restrict__ x, const val_t *__restrict__ z, int restart, const GmScal *__restrict__ S)
{
    if (gm_close_columns(S, restart) == 0) return;
    sv_walk(n, gridDim.x, [&](auto at) { at.put(x, at(x) + at(z)); });
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_gmres {
    tilespmv_plan *plan = nullptr;   // borrowed
    long long n = 0, stride = 0;     // stride: elements from one basis vector to the next
    int np = 0, restart = 0;
    int pos = 0;                     // inner iterations issued in the open cycle: the host's cycle position (begin and flush reset it)
    const val_t *dinv = nullptr;     // borrowed
    const tilespmv_block_jacobi *bj = nullptr;   // borrowed (tilespmv_gmres_create_block; then dinv is NULL and zhat is filled by k_bj_apply)
    void *block = nullptr;           // the one allocation: the basis, the work vectors, the partial sums, R, the rotations, g, y, the scalar block
    val_t *V = nullptr, *w = nullptr, *b = nullptr;
    val_t *zhat = nullptr;           // a vector only with a preconditioner; without, the product reads V_j
    double *pd1 = nullptr, *pd2 = nullptr, *pnorm = nullptr, *pbb = nullptr, *R = nullptr, *cs = nullptr, *sn = nullptr, *g = nullptr, *y = nullptr;
    GmScal *S = nullptr;
};

// the two creates: a diagonal (d_dinv, may be NULL) or a block-Jacobi object (bj), never both
static int gm_create(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const val_t *d_dinv, const tilespmv_block_jacobi *bj)
{
    if (restart < 1 || restart > GM_MAX_RESTART) {   // (before the plan is looked at)
        if (gs) *gs = nullptr;
        return (int)hipErrorInvalidValue;
    }
    const long long n = square_system(gs, plan, d_dinv);
    if (!n || (bj && bj->rows != n)) return (int)hipErrorInvalidValue;
    const int np = gm_parts(n);
    const size_t parts = ((size_t)np * sizeof(double) + 255) / 256 * 256, sums = (size_t)(restart + 1) * parts, vec = vec_bytes(n);
    const size_t rbytes = (size_t)GM_MAX_RESTART * GM_MAX_RESTART * sizeof(double), small = 768;   // small: up to GM_MAX_RESTART + 1 doubles, rounded to 256
    const bool hats = d_dinv || bj;
    DeviceBlock blk;
    const hipError_t e = blk.alloc((size_t)(restart + 3 + (hats ? 1 : 0)) * vec + 2 * sums + 2 * parts + rbytes + 4 * small + 256);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_gmres();
    c->plan = plan; c->n = n; c->stride = (long long)(vec / sizeof(val_t)); c->np = np; c->restart = restart; c->dinv = d_dinv; c->bj = bj; c->block = blk.base;
    c->V = blk.take<val_t>((size_t)(restart + 1) * vec);
    c->w = blk.take<val_t>(vec);
    c->b = blk.take<val_t>(vec);
    c->zhat = hats ? blk.take<val_t>(vec) : nullptr;
    c->pd1 = blk.take<double>(sums);
    c->pd2 = blk.take<double>(sums);
    c->pnorm = blk.take<double>(parts);
    c->pbb = blk.take<double>(parts);
    c->R = blk.take<double>(rbytes);
    c->cs = blk.take<double>(small);
    c->sn = blk.take<double>(small);
    c->g = blk.take<double>(small);
    c->y = blk.take<double>(small);
    c->S = blk.take<GmScal>(256);
    *gs = c;
    return 0;
}

// the end of an open or of an inner iteration: slot `slot` of the basis from w (, zhat)
static void gm_next(tilespmv_gmres *gs, int slot, hipStream_t st)
{
    hipLaunchKernelGGL(k_gm_next, dim3(gs->np), dim3(SVB), 0, st, gs->n, gs->w, gs->V, gs->stride, gs->dinv, gs->dinv ? gs->zhat : (val_t *)nullptr, gs->pd1, gs->pd2, gs->pnorm, gs->np,
                       slot == 0 ? 1 : 0, gs->S, gs->R, gs->cs, gs->sn, gs->g);
    if (gs->bj) block_jacobi_launch(gs->bj, gs->V + slot * gs->stride, gs->zhat, nullptr, st);   // zhat = M^-1 V_slot (under a guard that froze the basis: unused)
}

// open a cycle from the x in d_x; b: the caller's at the start of a solve (copied, b.b summed), else the solver's copy
static int gm_open(tilespmv_gmres *gs, const val_t *b, const val_t *d_x, hipStream_t st)
{
    const int rc = tilespmv_plan_spmv(gs->plan, d_x, gs->w, (void *)st);
    if (rc) return rc;
    const bool first = b != gs->b;
    hipLaunchKernelGGL(k_gm_resid, dim3(gs->np), dim3(SVB), 0, st, gs->n, b, first ? gs->b : (val_t *)nullptr, gs->w, gs->pnorm, first ? gs->pbb : (double *)nullptr);
    if (first) hipLaunchKernelGGL(k_gm_begin_fold, dim3(1), dim3(SVB), 0, st, gs->pbb, gs->np, gs->S);
    gm_next(gs, 0, st);
    gs->pos = 0;
    return (int)hipGetLastError();
}

// close the cycle: x += M^-1 (V y) over the columns done
static void gm_close(tilespmv_gmres *gs, val_t *d_x, hipStream_t st)
{
    const dim3 grid(gs->np), wg(SVB);
    hipLaunchKernelGGL(k_gm_solve, dim3(1), wg, 0, st, gs->R, gs->g, gs->y, gs->restart, gs->S);
    hipLaunchKernelGGL(k_gm_update, grid, wg, 0, st, gs->n, d_x, gs->V, gs->stride, gs->dinv, gs->y, gs->bj ? gs->w : (val_t *)nullptr, gs->restart, gs->S);
    if (gs->bj) {
        block_jacobi_launch(gs->bj, gs->w, gs->zhat, nullptr, st);
        hipLaunchKernelGGL(k_gm_axpy, grid, wg, 0, st, gs->n, d_x, gs->zhat, gs->restart, gs->S);
    }
}

extern "C" int tilespmv_gmres_create(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const MAT_VAL_TYPE *d_dinv)
{
    return gm_create(gs, plan, restart, d_dinv, nullptr);
}

extern "C" int tilespmv_gmres_create_block(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const tilespmv_block_jacobi *bj)
{
    if (!bj) {
        if (gs) *gs = nullptr;
        return (int)hipErrorInvalidValue;
    }
    return gm_create(gs, plan, restart, nullptr, bj);
}

extern "C" void tilespmv_gmres_destroy(tilespmv_gmres *gs) { destroy_solver(gs); }

extern "C" int tilespmv_gmres_begin(tilespmv_gmres *gs, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!gs || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    return gm_open(gs, d_b, d_x, (hipStream_t)stream);
}

extern "C" int tilespmv_gmres_iterate(tilespmv_gmres *gs, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!gs || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(gs->np), wg(SVB);
    for (int i = 0; i < count; i++) {
        int rc = tilespmv_plan_spmv(gs->plan, gs->zhat ? gs->zhat : gs->V + gs->pos * gs->stride, gs->w, stream);   // w = A M^-1 V_j
        if (rc) return rc;
        hipLaunchKernelGGL(k_gm_dots, grid, wg, 0, st, gs->n, gs->w, gs->V, gs->stride, gs->pd1, gs->np, gs->restart, gs->S);
        hipLaunchKernelGGL(k_gm_orth1, grid, wg, 0, st, gs->n, gs->w, gs->V, gs->stride, gs->pd1, gs->pd2, gs->np, gs->S);
        hipLaunchKernelGGL(k_gm_orth2, grid, wg, 0, st, gs->n, gs->w, gs->V, gs->stride, gs->pd2, gs->pnorm, gs->np, gs->S);
        gm_next(gs, gs->pos + 1, st);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        if (++gs->pos == gs->restart) {   // the cycle is full
            gm_close(gs, d_x, st);
            rc = gm_open(gs, gs->b, d_x, st);
            if (rc) return rc;
        }
    }
    return 0;
}

extern "C" int tilespmv_gmres_flush(tilespmv_gmres *gs, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!gs || !d_x || misaligned(d_x)) return (int)hipErrorInvalidValue;
    gm_close(gs, d_x, (hipStream_t)stream);
    return gm_open(gs, gs->b, d_x, (hipStream_t)stream);
}

extern "C" int tilespmv_gmres_state_read(tilespmv_gmres *gs, void *stream, tilespmv_cg_state *out)
{
    if (!gs) return (int)hipErrorInvalidValue;
    return state_read(gs->S, (hipStream_t)stream, out, cg_state_of<GmScal>);
}

extern "C" int tilespmv_gmres_solve(tilespmv_gmres *gs, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                                    tilespmv_cg_state *out)
{
    if (!gs) return (int)hipErrorInvalidValue;
    int rc = solve_loop<RrBbTest>(
        out, d_x, gs->n, rtol, maxiter, check_every, (hipStream_t)stream, [&] { return tilespmv_gmres_begin(gs, d_b, d_x, stream); },
        [&] { return tilespmv_gmres_state_read(gs, stream, out); }, [&](int count) { return tilespmv_gmres_iterate(gs, d_x, count, stream); });
    if (rc || out->bb == 0.0) return rc;   // (b = 0: x is 0 and rr says so)
    // x is current only after a close: flush, and report the recomputed |b - A x|^2 of the x that is returned under the status and the count of the decision
    const int status = out->status, iterations = out->iterations;
    rc = tilespmv_gmres_flush(gs, d_x, stream);
    if (!rc) rc = tilespmv_gmres_state_read(gs, stream, out);
    if (!rc) { out->status = status; out->iterations = iterations; }
    return rc;
}
