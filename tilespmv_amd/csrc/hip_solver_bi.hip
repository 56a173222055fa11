// hip_solver_bi.hip — BiCGStab for square nonsymmetric systems around a resident plan (tilespmv_bicgstab_*).
//
// Right-preconditioned BiCGStab, M^-1 = diag(dinv) (Jacobi; dinv = NULL: phat = p, shat = s).  One iteration is the two plan products v = A phat and t = A shat
// (tilespmv_plan_spmv: whatever launch form the plan has) and five streaming kernels:
//   k_bi_dot1       reads rhat, v                        partial sums of sigma = rhat.v, one per workgroup
//   k_bi_half       reads r, v (, dinv)                  alpha = rho / sigma;  s = r - alpha v, stored over r (, shat = dinv o s)
//   k_bi_dot2       reads t, s                           partial sums of t.s and t.t
//   k_bi_update     reads x, phat, s (, shat), t, rhat   omega = t.s / t.t;  x += alpha phat + omega shat;  r = s - omega t;  partial sums of r.r and rho' = rhat.r
//   k_bi_direction  reads r, p, v (, dinv)               beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v) (, phat = dinv o p)
// Vector elements read or written per iteration beside the two products, BY COUNT: 18 n (rhat v | r v r | t s | x phat s t rhat x r | r p v p); Jacobi adds dinv and the store of
// shat in the half step, the read of shat in the update, dinv and the store of phat in the direction: 23 n.  s lives in r; phat and shat are vectors only with a preconditioner:
// 5 work vectors (r, rhat, p, v, t), 7 with Jacobi.
// With a block-Jacobi object (tilespmv_bicgstab_create_block; hip_precond.hip) the kernels run with dinv = NULL and phat, shat are filled by k_bj_apply: phat = M^-1 p
// at the end of begin and after k_bi_direction, shat = M^-1 s after k_bi_half — 7 work vectors, 18 n + 2 (bs + 2) n elements.  Under a guard that froze the vectors the applies write the
// same bits again.
// The launch shape and the partial sums with their fixed order of additions are those of hip_solver_common.h, and so is the walk over a vector: every kernel here hands its body,
// written once for lane vectors and tail elements alike, to sv_dot, sv_walk_loaded or sv_walk.  The number of partials is solver_parts(n).  alpha, omega and beta are formed in double and rounded to the value type once, where they multiply.
//
// The scalar block (BiScal) has ONE writing kernel per field and no kernel reads a field it (or a concurrent workgroup of it) writes:
//   rho, live          k_bi_dot1, workgroup 0 (rho: fold of the rhat.r partials the previous update left; live: |r|^2 != 0, folded from that update's r.r partials, and no breakdown)
//                                                                                                  read by k_bi_half, k_bi_dot2 (workgroup 0), k_bi_update, k_bi_direction
//   alpha, half_broke  k_bi_dot2, workgroup 0 (alpha = rho / sigma, 0 unless live, rho != 0 and sigma != 0; half_broke: live, and rho = 0 or sigma = 0)
//                                                                                                  read by k_bi_update, k_bi_direction
//   rr, iterations, breakdown   k_bi_direction, workgroup 0 (iterations and breakdown: read and written by that workgroup alone; breakdown is set, never cleared)
//                                                                                                  read by the host (tilespmv_bicgstab_state_read); breakdown by k_bi_dot1 (workgroup 0)
//   all of them, and bb          k_bi_begin_fold (one workgroup), at the start of a solve
// k_bi_half folds the sigma partials itself (it is their first consumer); omega is folded by both kernels that use it.
// Guards (exact-zero tests, data-dependent uniform branches, no host round trip):
//   not live (|r|^2 = 0 at the start of the iteration, or the breakdown flag)   the half step, the update and the direction write nothing: x, r, p keep their bits
//   live, and rho = 0 or sigma = 0                                              breakdown; nothing is written in this or any later iteration, x keeps its last good value
//   t.t = 0 or t.s = 0                                                          omega = 0: x += alpha phat, r = s, p is left as it is; |r|^2 = 0 then: converged at the half step,
//                                                                               |r|^2 != 0: breakdown (omega = 0 with a live residual)
// The iteration counter advances in every iteration whatever the guards did.
#include <hip/hip_runtime.h>

#include "hip_precond.h"
#include "hip_solver_common.h"

namespace tilespmv {
namespace {

struct BiScal {
    double rho, alpha, rr, bb;
    int live, half_broke, iterations, breakdown;
};

__device__ __forceinline__ double bi_omega(double ts, double tt) { return (tt == 0.0 || ts == 0.0) ? 0.0 : ts / tt; }

__global__ __launch_bounds__(SVB) void k_bi_dot1(long long n, const val_t *__restrict__ rhat, const val_t *__restrict__ v, double *__restrict__ psig, const double *__restrict__ prho,
                                                 const double *__restrict__ prr, int np, BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    double acc = 0.0;
    sv_dot(n, gridDim.x, rhat, v, [&](auto a, auto b) { sv_mac(acc, a, b); });
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) psig[blockIdx.x] = t;
    if (blockIdx.x == 0) {   // rho of this iteration and whether it runs at all, for the kernels that follow
        const double rho = fold(prho, np, s), rr = fold(prr, np, s);
        if (threadIdx.x == 0) { S->rho = rho; S->live = (rr != 0.0 && !S->breakdown) ? 1 : 0; }
    }
}

// s = r - alpha v over r (, shat = dinv o s)
template <class T> struct BiHalf { T r, v, d; };
__global__ __launch_bounds__(SVB) void k_bi_half(long long n, val_t *__restrict__ r, const val_t *__restrict__ v, const val_t *__restrict__ dinv, val_t *__restrict__ shat,
                                                 const double *__restrict__ psig, int np, const BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double sigma = fold(psig, np, s), rho = S->rho;
    if (!S->live || rho == 0.0 || sigma == 0.0) return;
    const val_t alpha = (val_t)(rho / sigma);
    sv_walk_loaded<BiHalf>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.r = at(r); t.v = at(v);
            if (dinv) t.d = at(dinv);
        },
        [&](auto at, const auto &t) {
            const auto ns = t.r - alpha * t.v;
            at.put(r, ns);
            if (dinv) at.put(shat, t.d * ns);
        });
}

__global__ __launch_bounds__(SVB) void k_bi_dot2(long long n, const val_t *__restrict__ t, const val_t *__restrict__ sv, double *__restrict__ pts, double *__restrict__ ptt,
                                                 const double *__restrict__ psig, int np, BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    double ats = 0.0, att = 0.0;
    sv_dot(n, gridDim.x, t, sv, [&](auto a, auto b) { sv_mac(ats, a, b); sv_mac(att, a, a); });
    const double tts = block_sum(ats, s), ttt = block_sum(att, s);
    if (threadIdx.x == 0) { pts[blockIdx.x] = tts; ptt[blockIdx.x] = ttt; }
    if (blockIdx.x == 0) {   // alpha as the half step formed it, for the two kernels that follow
        const double sigma = fold(psig, np, s), rho = S->rho;
        const bool go = S->live && rho != 0.0 && sigma != 0.0;
        if (threadIdx.x == 0) { S->alpha = go ? rho / sigma : 0.0; S->half_broke = (S->live && !go) ? 1 : 0; }
    }
}

// x += alpha phat + omega shat;  r = s - omega t (s lives in r; shat = NULL: shat is s)
template <class T> struct BiUpdate { T x, phat, s, shat, t, rhat; };
__global__ __launch_bounds__(SVB) void k_bi_update(long long n, val_t *__restrict__ x, const val_t *__restrict__ phat, val_t *__restrict__ r, const val_t *__restrict__ shat,
                                                   const val_t *__restrict__ t, const val_t *__restrict__ rhat, const double *__restrict__ pts, const double *__restrict__ ptt,
                                                   double *__restrict__ prr, double *__restrict__ prho, int np, const BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    if (!S->live || S->half_broke) return;
    const double ts = fold(pts, np, s), tt = fold(ptt, np, s);
    const val_t alpha = (val_t)S->alpha, omega = (val_t)bi_omega(ts, tt);
    double arr = 0.0, arho = 0.0;
    sv_walk_loaded<BiUpdate>(
        n, gridDim.x,
        [&](auto at, auto &v) {
            v.x = at(x); v.phat = at(phat); v.s = at(r); v.t = at(t); v.rhat = at(rhat);
            if (shat) v.shat = at(shat);
        },
        [&](auto at, const auto &v) {
            const auto sh = shat ? v.shat : v.s;
            const auto nx = v.x + alpha * v.phat + omega * sh, nr = v.s - omega * v.t;
            at.put(x, nx);
            at.put(r, nr);
            sv_mac(arr, nr, nr);
            sv_mac(arho, v.rhat, nr);
        });
    const double trr = block_sum(arr, s), trho = block_sum(arho, s);
    if (threadIdx.x == 0) { prr[blockIdx.x] = trr; prho[blockIdx.x] = trho; }
}

// p = r + beta (p - omega v) (, phat = dinv o p)
template <class T> struct BiDirection { T r, p, v, d; };
__global__ __launch_bounds__(SVB) void k_bi_direction(long long n, const val_t *__restrict__ r, val_t *__restrict__ p, const val_t *__restrict__ v, const val_t *__restrict__ dinv,
                                                      val_t *__restrict__ phat, const double *__restrict__ pts, const double *__restrict__ ptt, const double *__restrict__ prr,
                                                      const double *__restrict__ prho, int np, BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const bool go = S->live && !S->half_broke;
    double om = 0.0;
    if (go) {
        const double ts = fold(pts, np, s), tt = fold(ptt, np, s);
        om = bi_omega(ts, tt);
    }
    if (blockIdx.x == 0) {   // what the host reads (a skipped update left its r.r partials: the same |r|^2 again)
        const double rr = fold(prr, np, s);
        if (threadIdx.x == 0) {
            S->rr = rr;
            S->iterations = S->iterations + 1;
            if (S->half_broke || (go && om == 0.0 && rr != 0.0)) S->breakdown = 1;
        }
    }
    if (!go || om == 0.0) return;
    const double rho_new = fold(prho, np, s);
    const val_t beta = (val_t)((rho_new / S->rho) * (S->alpha / om)), omega = (val_t)om;
    sv_walk_loaded<BiDirection>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.r = at(r); t.p = at(p); t.v = at(v);
            if (dinv) t.d = at(dinv);
        },
        [&](auto at, const auto &t) {
            const auto np_ = t.r + beta * (t.p - omega * t.v);
            at.put(p, np_);
            if (dinv) at.put(phat, t.d * np_);
        });
}

// the start of a solve: r = rhat = p = b - A x (Ax holds the product) (, phat = dinv o p), partial sums of r.r (= rhat.r) and b.b
__global__ __launch_bounds__(SVB) void k_bi_begin(long long n, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ r, val_t *__restrict__ rhat,
                                                  val_t *__restrict__ p, const val_t *__restrict__ dinv, val_t *__restrict__ phat, double *__restrict__ prr, double *__restrict__ prho,
                                                  double *__restrict__ pbb)
{
    __shared__ double s[SVB / 64];
    double arr = 0.0, abb = 0.0;
    sv_walk(n, gridDim.x, [&](auto at) {
        const auto vb = at(b), nr = vb - at(Ax);
        at.put(r, nr);
        at.put(rhat, nr);
        at.put(p, nr);
        if (dinv) at.put(phat, at(dinv) * nr);
        sv_mac(arr, nr, nr);
        sv_mac(abb, vb, vb);
    });
    const double trr = block_sum(arr, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) { prr[blockIdx.x] = trr; prho[blockIdx.x] = trr; pbb[blockIdx.x] = tbb; }
}
// ... and its scalars (one workgroup)
__global__ __launch_bounds__(SVB) void k_bi_begin_fold(const double *__restrict__ prr, const double *__restrict__ pbb, int np, BiScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double rr = fold(prr, np, s), bb = fold(pbb, np, s);
    if (threadIdx.x == 0) {
        S->rho = rr; S->alpha = 0.0; S->rr = rr; S->bb = bb;
        S->live = 0; S->half_broke = 0; S->iterations = 0; S->breakdown = 0;
    }
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_bicgstab {
    tilespmv_plan *plan = nullptr;   // borrowed
    long long n = 0;
    int np = 0;
    const val_t *dinv = nullptr;     // borrowed
    const tilespmv_block_jacobi *bj = nullptr;   // borrowed (tilespmv_bicgstab_create_block; then dinv is NULL, and phat and shat are filled by k_bj_apply, hip_precond.hip)
    void *block = nullptr;           // the one allocation: the work vectors, the partial-sum arrays, the scalar block
    val_t *r = nullptr, *rhat = nullptr, *p = nullptr, *v = nullptr, *t = nullptr;
    val_t *phat = nullptr, *shat = nullptr;   // vectors of their own with a preconditioner; without: phat is p, shat is NULL (s itself, in r)
    double *psig = nullptr, *pts = nullptr, *ptt = nullptr, *prr = nullptr, *prho = nullptr, *pbb = nullptr;
    BiScal *S = nullptr;
};

// the two creates: a diagonal (d_dinv, may be NULL) or a block-Jacobi object (bj), never both
static int bi_create(tilespmv_bicgstab **bs, tilespmv_plan *plan, const val_t *d_dinv, const tilespmv_block_jacobi *bj)
{
    const long long n = square_system(bs, plan, d_dinv);
    if (!n || (bj && bj->rows != n)) return (int)hipErrorInvalidValue;
    const size_t vec = vec_bytes(n), parts = SV_PARTS_BYTES;
    const bool hats = d_dinv || bj;
    DeviceBlock blk;
    const hipError_t e = blk.alloc((hats ? 7 : 5) * vec + 6 * parts + 256);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_bicgstab();
    c->plan = plan; c->n = n; c->np = solver_parts(n); c->dinv = d_dinv; c->bj = bj; c->block = blk.base;
    c->r = blk.take<val_t>(vec);
    c->rhat = blk.take<val_t>(vec);
    c->p = blk.take<val_t>(vec);
    c->v = blk.take<val_t>(vec);
    c->t = blk.take<val_t>(vec);
    c->phat = hats ? blk.take<val_t>(vec) : c->p;
    c->shat = hats ? blk.take<val_t>(vec) : nullptr;
    c->psig = blk.take<double>(parts);
    c->pts = blk.take<double>(parts);
    c->ptt = blk.take<double>(parts);
    c->prr = blk.take<double>(parts);
    c->prho = blk.take<double>(parts);
    c->pbb = blk.take<double>(parts);
    c->S = blk.take<BiScal>(256);
    *bs = c;
    return 0;
}

extern "C" int tilespmv_bicgstab_create(tilespmv_bicgstab **bs, tilespmv_plan *plan, const MAT_VAL_TYPE *d_dinv)
{
    return bi_create(bs, plan, d_dinv, nullptr);
}

extern "C" int tilespmv_bicgstab_create_block(tilespmv_bicgstab **bs, tilespmv_plan *plan, const tilespmv_block_jacobi *bj)
{
    if (!bj) {
        if (bs) *bs = nullptr;
        return (int)hipErrorInvalidValue;
    }
    return bi_create(bs, plan, nullptr, bj);
}

extern "C" void tilespmv_bicgstab_destroy(tilespmv_bicgstab *bs) { destroy_solver(bs); }

extern "C" int tilespmv_bicgstab_begin(tilespmv_bicgstab *bs, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!bs || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = tilespmv_plan_spmv(bs->plan, d_x, bs->v, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bi_begin, dim3(bs->np), dim3(SVB), 0, st, bs->n, d_b, bs->v, bs->r, bs->rhat, bs->p, bs->dinv, bs->dinv ? bs->phat : (val_t *)nullptr, bs->prr, bs->prho,
                       bs->pbb);
    hipLaunchKernelGGL(k_bi_begin_fold, dim3(1), dim3(SVB), 0, st, bs->prr, bs->pbb, bs->np, bs->S);
    if (bs->bj) block_jacobi_launch(bs->bj, bs->p, bs->phat, nullptr, st);   // phat = M^-1 p
    return (int)hipGetLastError();
}

extern "C" int tilespmv_bicgstab_iterate(tilespmv_bicgstab *bs, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!bs || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(bs->np), wg(SVB);
    val_t *const phat_out = bs->dinv ? bs->phat : (val_t *)nullptr;
    for (int i = 0; i < count; i++) {
        int rc = tilespmv_plan_spmv(bs->plan, bs->phat, bs->v, stream);                        // v = A phat
        if (rc) return rc;
        hipLaunchKernelGGL(k_bi_dot1, grid, wg, 0, st, bs->n, bs->rhat, bs->v, bs->psig, bs->prho, bs->prr, bs->np, bs->S);
        hipLaunchKernelGGL(k_bi_half, grid, wg, 0, st, bs->n, bs->r, bs->v, bs->dinv, bs->shat, bs->psig, bs->np, bs->S);
        if (bs->bj) block_jacobi_launch(bs->bj, bs->r, bs->shat, nullptr, st);               // shat = M^-1 s (under a guard that froze the vectors: the same bits again)
        rc = tilespmv_plan_spmv(bs->plan, bs->shat ? bs->shat : bs->r, bs->t, stream);        // t = A shat
        if (rc) return rc;
        hipLaunchKernelGGL(k_bi_dot2, grid, wg, 0, st, bs->n, bs->t, bs->r, bs->pts, bs->ptt, bs->psig, bs->np, bs->S);
        hipLaunchKernelGGL(k_bi_update, grid, wg, 0, st, bs->n, d_x, bs->phat, bs->r, bs->shat, bs->t, bs->rhat, bs->pts, bs->ptt, bs->prr, bs->prho, bs->np, bs->S);
        hipLaunchKernelGGL(k_bi_direction, grid, wg, 0, st, bs->n, bs->r, bs->p, bs->v, bs->dinv, phat_out, bs->pts, bs->ptt, bs->prr, bs->prho, bs->np, bs->S);
        if (bs->bj) block_jacobi_launch(bs->bj, bs->p, bs->phat, nullptr, st);               // phat = M^-1 p
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int tilespmv_bicgstab_state_read(tilespmv_bicgstab *bs, void *stream, tilespmv_cg_state *out)
{
    if (!bs) return (int)hipErrorInvalidValue;
    return state_read(bs->S, (hipStream_t)stream, out, cg_state_of<BiScal>);
}

extern "C" int tilespmv_bicgstab_solve(tilespmv_bicgstab *bs, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                                       tilespmv_cg_state *out)
{
    if (!bs) return (int)hipErrorInvalidValue;
    return solve_loop<RrBbTest>(
        out, d_x, bs->n, rtol, maxiter, check_every, (hipStream_t)stream, [&] { return tilespmv_bicgstab_begin(bs, d_b, d_x, stream); },
        [&] { return tilespmv_bicgstab_state_read(bs, stream, out); }, [&](int count) { return tilespmv_bicgstab_iterate(bs, d_x, count, stream); });
}
