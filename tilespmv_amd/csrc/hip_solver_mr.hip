// hip_solver_mr.hip — MINRES for square symmetric systems that may be indefinite, around a resident plan (tilespmv_minres_*, tilespmv_csr_abs_diagonal_device; DESIGN.md §3.11,
// INTEGRATION.md §4i).
//
// Preconditioned Paige-Saunders MINRES, M^-1 = diag(minv) with minv > 0 (minv = NULL: z = r2).  The Lanczos vector v = z / beta is never stored: V holds z itself, the product input
// at an address that never changes, and every consumer multiplies by 1 / beta (rounded to the value type once).  One iteration is the plan product y = A z (tilespmv_plan_spmv:
// whatever launch form the plan has) and three streaming kernels:
//   k_mr_dot      reads V, y                                        partial sums of alfa = v.(y / beta), one per workgroup
//   k_mr_lanczos  reads y, r1, r2 (, minv)                          y' = y / beta - (beta / oldb) r1 - (alfa / beta) r2, stored over r1;  partial sums of beta'^2 = y'.(minv o y')
//   k_mr_update   reads V, w, w2, x, y' (, minv)                    the rotation;  w' = (v - oldeps w2 - delta w) / gamma, stored over w2;  x += phi w';  V = z' = minv o y'
// Vector elements read or written per iteration beside the product, BY COUNT: 14 n (V y | y r1 r2 y' | V w w2 x y' w' x V); minv adds its read in the Lanczos step and in the update:
// 16 n.  z' is recomputed in the update from y' and minv instead of being stored and read back.  6 work vectors with or without minv (y, V, two of r, two of w) of n + 16 elements,
// and 16.25 KB of partial sums and scalars.
// The three-term history is not rotated on the host (a captured iterate(k) has its pointers baked in) and not shifted by copies either: the kernels choose roles from the parity of
// the DEVICE-side iteration counter.  In an iteration of parity p, r2 is R[p], r1 is R[1 - p] and receives y' (the next r2); w is W[p], w2 is W[1 - p] and receives w'.
// The launch shape and the partial sums with their fixed order of additions are those of hip_solver_common.h, and so is the walk over a vector: every kernel here hands its body,
// written once for lane vectors and tail elements alike, to sv_dot, sv_walk_loaded or sv_walk.  The number of partials is solver_parts(n).  1/beta, alfa/beta, beta/oldb, oldeps, delta, 1/gamma and phi are formed in double and rounded to the value type once, where they multiply.
//
// The scalar block (MrScal) has ONE writing kernel per field and no kernel reads a field it (or a concurrent workgroup of it) writes:
//   at (beta, oldb, dbar, epsln, phibar, cs, sn), parity, live   k_mr_dot, workgroup 0: the recurrence as the previous iteration left it (a copy of `next`), the parity of the
//                                                                iteration counter, and live = phibar != 0 and no breakdown        read by k_mr_lanczos, k_mr_update
//   next (the same seven), rr, iterations, breakdown             k_mr_update, workgroup 0, from `at` and the folded alfa and beta'^2 (iterations and breakdown: read and written by
//                                                                that workgroup alone; breakdown is set, never cleared)
//                                                                read by k_mr_dot (next.beta: every workgroup) and the host (tilespmv_minres_state_read)
//   all of them, and bb                                          k_mr_begin_fold (one workgroup), at the start of a solve
// k_mr_lanczos folds the alfa partials itself (it is their first consumer); k_mr_update folds them again, and the beta'^2 partials.
// Guards (exact tests, data-dependent uniform branches, no host round trip):
//   not live (phibar = 0 at the start of the iteration, or the breakdown flag)   the Lanczos step and the update write nothing: x keeps its bits (b = 0; beta' = 0, the lucky end)
//   r2.z < 0 in begin, y'.z' < 0                                                 M is not positive definite: breakdown; the update writes nothing in this or any later iteration
//   gamma = 0                                                                    A is singular on this Krylov space, the system incompatible: breakdown, the same way
// The iteration counter advances in every iteration whatever the guards did.
#include <hip/hip_runtime.h>

#include "hip_solver_common.h"

namespace tilespmv {
namespace {

struct MrRec {
    double beta, oldb, dbar, epsln, phibar, cs, sn;
};
struct MrScal {
    MrRec next;
    double rr, bb;
    int iterations, breakdown;
    MrRec at;
    int parity, live;
};

__device__ __forceinline__ double mr_inverse(double a) { return a == 0.0 ? 0.0 : 1.0 / a; }

__global__ __launch_bounds__(SVB) void k_mr_dot(long long n, const val_t *__restrict__ V, const val_t *__restrict__ y, double *__restrict__ palfa, MrScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const val_t ib = (val_t)mr_inverse(S->next.beta);
    double acc = 0.0;
    sv_dot(n, gridDim.x, V, y, [&](auto a, auto b) { sv_mac(acc, ib * a, ib * b); });
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) {
        palfa[blockIdx.x] = t;
        if (blockIdx.x == 0) {   // where the recurrence stands, for the two kernels that follow
            S->at = S->next;
            S->parity = S->iterations & 1;
            S->live = (S->next.phibar != 0.0 && !S->breakdown) ? 1 : 0;
        }
    }
}

// y' = y / beta - (beta / oldb) r1 - (alfa / beta) r2 over r1;  partial sums of y'.(minv o y')
template <class T> struct MrLanczos { T y, r1, r2, d; };
__global__ __launch_bounds__(SVB) void k_mr_lanczos(long long n, const val_t *__restrict__ y, val_t *__restrict__ Ra, val_t *__restrict__ Rb, const val_t *__restrict__ minv,
                                                    const double *__restrict__ palfa, double *__restrict__ pbeta, int np, const MrScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    if (!S->live) return;
    const double alfa = fold(palfa, np, s), beta = S->at.beta, oldb = S->at.oldb;
    const val_t ib = (val_t)(1.0 / beta), c1 = (val_t)(oldb != 0.0 ? beta / oldb : 0.0), c2 = (val_t)(alfa / beta);
    const val_t *const r2 = S->parity ? Rb : Ra;
    val_t *const r1 = S->parity ? Ra : Rb;
    double acc = 0.0;
    sv_walk_loaded<MrLanczos>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.y = at(y); t.r1 = at(r1); t.r2 = at(r2);
            if (minv) t.d = at(minv);
        },
        [&](auto at, const auto &t) {
            const auto ny = ib * t.y - c1 * t.r1 - c2 * t.r2;
            at.put(r1, ny);
            sv_mac(acc, ny, minv ? t.d * ny : ny);
        });
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) pbeta[blockIdx.x] = t;
}

// the rotation;  w' = (v - oldeps w2 - delta w) / gamma over w2;  x += phi w';  V = minv o y'
template <class T> struct MrUpdate { T x, v, w, w2, yn, d; };
__global__ __launch_bounds__(SVB) void k_mr_update(long long n, val_t *__restrict__ x, val_t *__restrict__ V, val_t *__restrict__ Wa, val_t *__restrict__ Wb,
                                                   const val_t *__restrict__ Ra, const val_t *__restrict__ Rb, const val_t *__restrict__ minv, const double *__restrict__ palfa,
                                                   const double *__restrict__ pbeta, int np, MrScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!S->live) {
        if (first) S->iterations = S->iterations + 1;
        return;
    }
    const double alfa = fold(palfa, np, s), bsq = fold(pbeta, np, s);
    const MrRec c = S->at;
    const double betan = bsq < 0.0 ? 0.0 : sqrt(bsq);
    const double oldeps = c.epsln, delta = c.cs * c.dbar + c.sn * alfa, gbar = c.sn * c.dbar - c.cs * alfa, gamma = hypot(gbar, betan);
    if (bsq < 0.0 || gamma == 0.0) {
        if (first) { S->breakdown = 1; S->iterations = S->iterations + 1; }
        return;
    }
    const double cs = gbar / gamma, sn = betan / gamma, phi64 = cs * c.phibar, phibar = sn * c.phibar;
    if (first) {
        MrRec r;
        r.beta = betan; r.oldb = c.beta; r.dbar = -c.cs * betan; r.epsln = c.sn * betan; r.phibar = phibar; r.cs = cs; r.sn = sn;
        S->next = r;
        S->rr = phibar * phibar;
        S->iterations = S->iterations + 1;
    }
    const val_t ib = (val_t)(1.0 / c.beta), oe = (val_t)oldeps, de = (val_t)delta, ig = (val_t)(1.0 / gamma), phi = (val_t)phi64;
    const val_t *const w = S->parity ? Wb : Wa, *const yn = S->parity ? Ra : Rb;
    val_t *const w2 = S->parity ? Wa : Wb;
    sv_walk_loaded<MrUpdate>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.x = at(x); t.v = at(V); t.w = at(w); t.w2 = at(w2); t.yn = at(yn);
            if (minv) t.d = at(minv);
        },
        [&](auto at, const auto &t) {
            const auto nw = (ib * t.v - oe * t.w2 - de * t.w) * ig;
            at.put(w2, nw);
            at.put(x, t.x + phi * nw);
            at.put(V, minv ? t.d * t.yn : t.yn);
        });
}

// the start of a solve: r2 = b - A x (Ax holds the product) into R[0], V = z = minv o r2, r1 = w = w2 = 0, partial sums of r2.z and b.(minv o b)
__global__ __launch_bounds__(SVB) void k_mr_begin(long long n, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ Ra, val_t *__restrict__ Rb,
                                                  val_t *__restrict__ V, val_t *__restrict__ Wa, val_t *__restrict__ Wb, const val_t *__restrict__ minv, double *__restrict__ prz,
                                                  double *__restrict__ pbb)
{
    __shared__ double s[SVB / 64];
    double arz = 0.0, abb = 0.0;
    sv_walk(n, gridDim.x, [&](auto at) {
        const auto vb = at(b), nr = vb - at(Ax);
        auto nz = nr, mb = vb, zero = nr;
        if (minv) { const auto vd = at(minv); nz = vd * nr; mb = vd * vb; }
        zero = (val_t)0;
        at.put(Ra, nr);
        at.put(V, nz);
        at.put(Rb, zero); at.put(Wa, zero); at.put(Wb, zero);
        sv_mac(arz, nr, nz);
        sv_mac(abb, vb, mb);
    });
    const double trz = block_sum(arz, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) { prz[blockIdx.x] = trz; pbb[blockIdx.x] = tbb; }
}
// ... and its scalars (one workgroup).  rr is the sum r2.z itself, not the square of its root
__global__ __launch_bounds__(SVB) void k_mr_begin_fold(const double *__restrict__ prz, const double *__restrict__ pbb, int np, MrScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double rz = fold(prz, np, s), bb = fold(pbb, np, s);
    if (threadIdx.x == 0) {
        const double beta = rz < 0.0 ? 0.0 : sqrt(rz);
        MrRec r;
        r.beta = beta; r.oldb = 0.0; r.dbar = 0.0; r.epsln = 0.0; r.phibar = beta; r.cs = -1.0; r.sn = 0.0;
        S->next = r; S->at = r;
        S->rr = rz; S->bb = bb;
        S->iterations = 0; S->breakdown = rz < 0.0 ? 1 : 0; S->parity = 0; S->live = 0;
    }
}

// one row per thread: the stored entries (i, i), added in storage order; the absolute value of the sum
__global__ __launch_bounds__(SVB) void k_csr_abs_diagonal(int rows, const int *__restrict__ rp, const int *__restrict__ ci, const val_t *__restrict__ v, val_t *__restrict__ out,
                                                          int invert)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    double a = 0.0;
    for (long long k = rp[i]; k < rp[i + 1]; k++)
        if (ci[k] == (int)i) a += (double)v[k];
    const val_t d = (val_t)fabs(a);
    out[i] = !invert ? d : SV_INVERSE_OR_ONE(d);
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_minres {
    tilespmv_plan *plan = nullptr;   // borrowed
    long long n = 0;
    int np = 0;
    const val_t *minv = nullptr;     // borrowed
    void *block = nullptr;           // the one allocation: the work vectors, the partial-sum arrays, the scalar block
    val_t *y = nullptr, *V = nullptr, *Ra = nullptr, *Rb = nullptr, *Wa = nullptr, *Wb = nullptr;
    double *palfa = nullptr, *pbeta = nullptr;   // begin: b.(minv o b) and r2.z
    MrScal *S = nullptr;
};

extern "C" int tilespmv_minres_create(tilespmv_minres **ms, tilespmv_plan *plan, const MAT_VAL_TYPE *d_minv)
{
    const long long n = square_system(ms, plan, d_minv);
    if (!n) return (int)hipErrorInvalidValue;
    const size_t vec = vec_bytes(n), parts = SV_PARTS_BYTES;
    static_assert(sizeof(MrScal) <= 256, "the scalar block has 256 bytes");
    DeviceBlock blk;
    const hipError_t e = blk.alloc(6 * vec + 2 * parts + 256);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_minres();
    c->plan = plan; c->n = n; c->np = solver_parts(n); c->minv = d_minv; c->block = blk.base;
    c->y = blk.take<val_t>(vec);
    c->V = blk.take<val_t>(vec);
    c->Ra = blk.take<val_t>(vec);
    c->Rb = blk.take<val_t>(vec);
    c->Wa = blk.take<val_t>(vec);
    c->Wb = blk.take<val_t>(vec);
    c->palfa = blk.take<double>(parts);
    c->pbeta = blk.take<double>(parts);
    c->S = blk.take<MrScal>(256);
    *ms = c;
    return 0;
}

extern "C" void tilespmv_minres_destroy(tilespmv_minres *ms) { destroy_solver(ms); }

extern "C" int tilespmv_minres_begin(tilespmv_minres *ms, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!ms || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = tilespmv_plan_spmv(ms->plan, d_x, ms->y, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mr_begin, dim3(ms->np), dim3(SVB), 0, st, ms->n, d_b, ms->y, ms->Ra, ms->Rb, ms->V, ms->Wa, ms->Wb, ms->minv, ms->pbeta, ms->palfa);
    hipLaunchKernelGGL(k_mr_begin_fold, dim3(1), dim3(SVB), 0, st, ms->pbeta, ms->palfa, ms->np, ms->S);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_minres_iterate(tilespmv_minres *ms, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!ms || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ms->np), wg(SVB);
    for (int i = 0; i < count; i++) {
        const int rc = tilespmv_plan_spmv(ms->plan, ms->V, ms->y, stream);                        // y = A z
        if (rc) return rc;
        hipLaunchKernelGGL(k_mr_dot, grid, wg, 0, st, ms->n, ms->V, ms->y, ms->palfa, ms->S);
        hipLaunchKernelGGL(k_mr_lanczos, grid, wg, 0, st, ms->n, ms->y, ms->Ra, ms->Rb, ms->minv, ms->palfa, ms->pbeta, ms->np, ms->S);
        hipLaunchKernelGGL(k_mr_update, grid, wg, 0, st, ms->n, d_x, ms->V, ms->Wa, ms->Wb, ms->Ra, ms->Rb, ms->minv, ms->palfa, ms->pbeta, ms->np, ms->S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int tilespmv_minres_state_read(tilespmv_minres *ms, void *stream, tilespmv_cg_state *out)
{
    if (!ms) return (int)hipErrorInvalidValue;
    return state_read(ms->S, (hipStream_t)stream, out, cg_state_of<MrScal>);
}

extern "C" int tilespmv_minres_solve(tilespmv_minres *ms, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                                     tilespmv_cg_state *out)
{
    if (!ms) return (int)hipErrorInvalidValue;
    return solve_loop<RrBbTest>(
        out, d_x, ms->n, rtol, maxiter, check_every, (hipStream_t)stream, [&] { return tilespmv_minres_begin(ms, d_b, d_x, stream); },
        [&] { return tilespmv_minres_state_read(ms, stream, out); }, [&](int count) { return tilespmv_minres_iterate(ms, d_x, count, stream); });
}

extern "C" int tilespmv_csr_abs_diagonal_device(int rows, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_VAL_TYPE *d_out, int invert,
                                                void *stream)
{
    return launch_per_row(k_csr_abs_diagonal, rows, d_csrRowPtr, d_csrColIdx, false, d_csrVal, d_out, invert, stream);
}
