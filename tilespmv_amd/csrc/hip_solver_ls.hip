// hip_solver_ls.hip — CGLS least squares around the resident plans of A and A^T (tilespmv_cgls_*, tilespmv_csr_row_sqnorms_device).
//
// min |A x - b|^2 + damp^2 |x|^2 for a rows x cols matrix of any shape and rank: conjugate gradients on (A^T A + damp^2 I) x = A^T b without ever forming A^T A, optionally
// preconditioned by a positive diagonal z = cinv o s (cinv_j = 1 / |a_j|^2: Jacobi on the normal equations).  r, q have `rows` elements, p, s have `cols`.
// One iteration is the two plan products (q = A p, s = A^T r: tilespmv_plan_spmv, whatever launch form each plan has) and four streaming kernels:
//   k_ls_dot        reads q (, p)                   partial sums of q.q (and, damped, p.p), one per workgroup
//   k_ls_update     reads p, x, q, r                alpha = gamma / delta, delta = q.q + damp^2 p.p;  x += alpha p;  r -= alpha q;  partial sums of r.r
//   k_ls_normal     reads s (, x, cinv)             (damped) s -= damp^2 x, stored;  partial sums of s.s and (cinv) s.z, z = cinv o s
//   k_ls_direction  reads s, p (, cinv)             beta = gamma' / gamma;  p = z + beta p  (z recomputed from s and cinv, never stored)
// Vector elements read or written per iteration beside the two products, BY COUNT: 4 rows + 7 cols with damp = 0 and cinv = NULL (q | p x x q r r | s | s p p);
// damping adds 3 cols (p in the dot; x read and s stored in the normal pass), cinv adds 2 cols (read in the normal and the direction pass).
// The loop of torch operations it replaces (operator.cgls) moves 7 rows + 12 cols in about a dozen launches.
//
// The launch shape and the partial sums with their fixed order of additions are those of hip_solver_common.h, and so is the walk over a vector: every kernel here hands its body,
// written once for lane vectors and tail elements alike, to sv_dot, sv_walk_loaded or sv_walk.  Row-length sums
// (q.q, r.r, b.b) have npr = solver_parts(rows) partials, column-length sums (p.p, s.s, s.z) npc = solver_parts(cols).  A kernel that walks both lengths is launched over
// max(npr, npc) workgroups, so every walk here is guarded: the workgroups from the vector's own count on skip it.  alpha, beta and damp^2 are rounded to the value type once,
// where they multiply.
//
// The scalar block (LsScal) has ONE writing kernel per field and no kernel reads a field it (or a concurrent workgroup of it) writes:
//   gamma            k_ls_dot, workgroup 0 (fold of the s.z partials the previous normal pass left; 0 after a breakdown)    read by k_ls_update, k_ls_direction
//   breakdown        k_ls_update, workgroup 0 (set, never cleared)                                                          read by k_ls_dot (workgroup 0), k_ls_direction
//   nn, rr, iterations   k_ls_direction, workgroup 0 (iterations: read and written by that workgroup alone)                 read by the host (tilespmv_cgls_state_read)
//   damp2            k_ls_begin_r, workgroup 0 (the damp of tilespmv_cgls_begin holds for the iterations that follow)       read by k_ls_dot, k_ls_update, k_ls_normal
//   nn0, bb, and every field but damp2 at the start of a solve   k_ls_begin_fold (one workgroup)
// Guards (data-dependent branches, no host round trip): gamma = 0 -> alpha = beta = 0, x and r stay as they are; gamma < 0 (a cinv that is not positive), or gamma > 0 without
// delta > 0 -> breakdown is set, alpha = beta = 0 in this and every later iteration, x keeps its last good value.
#include <hip/hip_runtime.h>

#include "hip_solver_common.h"

namespace tilespmv {
namespace {

struct LsScal {
    double gamma, nn, nn0, rr, bb, damp2;
    int iterations, breakdown;
};

// partial sums of v.v over n elements
__device__ __forceinline__ double sq_partial(long long n, const val_t *__restrict__ v, int nwg)
{
    double acc = 0.0;
    if ((int)blockIdx.x < nwg) sv_dot(n, nwg, v, v, [&](auto a, auto) { sv_mac(acc, a, a); });
    return acc;
}

__global__ __launch_bounds__(SVB) void k_ls_dot(long long rows, long long cols, const val_t *__restrict__ q, const val_t *__restrict__ p, double *__restrict__ pqq,
                                                double *__restrict__ ppp, const double *__restrict__ psz, int npr, int npc, LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const bool damped = S->damp2 != 0.0;
    const double tq = block_sum(sq_partial(rows, q, npr), s);
    if (threadIdx.x == 0 && (int)blockIdx.x < npr) pqq[blockIdx.x] = tq;
    if (damped) {
        const double tp = block_sum(sq_partial(cols, p, npc), s);
        if (threadIdx.x == 0 && (int)blockIdx.x < npc) ppp[blockIdx.x] = tp;
    }
    if (blockIdx.x == 0) {   // gamma of this iteration, for the two kernels that consume it
        const double g = fold(psz, npc, s);
        if (threadIdx.x == 0) S->gamma = S->breakdown ? 0.0 : g;
    }
}

template <class T> struct LsAxpy { T a, y; };   // y +- alpha a
__global__ __launch_bounds__(SVB) void k_ls_update(long long rows, long long cols, const val_t *__restrict__ p, const val_t *__restrict__ q, val_t *__restrict__ x,
                                                   val_t *__restrict__ r, const double *__restrict__ pqq, const double *__restrict__ ppp, double *__restrict__ prr, int npr, int npc,
                                                   LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double d2 = S->damp2, gamma = S->gamma;
    double delta = fold(pqq, npr, s);
    if (d2 != 0.0) delta += d2 * fold(ppp, npc, s);
    const bool broke = gamma < 0.0 || (gamma > 0.0 && !(delta > 0.0));
    const val_t alpha = (val_t)((gamma > 0.0 && delta > 0.0) ? gamma / delta : 0.0);
    if (broke && blockIdx.x == 0 && threadIdx.x == 0) S->breakdown = 1;
    if ((int)blockIdx.x < npc)
        sv_walk_loaded<LsAxpy>(
            cols, npc, [&](auto at, auto &t) { t.a = at(p); t.y = at(x); }, [&](auto at, const auto &t) { at.put(x, t.y + alpha * t.a); });
    double arr = 0.0;
    if ((int)blockIdx.x < npr)
        sv_walk_loaded<LsAxpy>(
            rows, npr, [&](auto at, auto &t) { t.a = at(q); t.y = at(r); },
            [&](auto at, const auto &t) {
                const auto nr = t.y - alpha * t.a;
                at.put(r, nr);
                sv_mac(arr, nr, nr);
            });
    const double trr = block_sum(arr, s);
    if (threadIdx.x == 0 && (int)blockIdx.x < npr) prr[blockIdx.x] = trr;
}

// The normal residual s = A^T r (the product left it) - damp^2 x, its squared norm and s.z.  plain != 0: s as it stands, no damping, no cinv (|A^T b|^2 at the start of a solve).
// p_out != NULL (the start of a solve): p = z as well.
template <class T> struct LsNormal { T s, x, c; };
__global__ __launch_bounds__(SVB) void k_ls_normal(long long cols, val_t *__restrict__ sv, const val_t *__restrict__ x, const val_t *__restrict__ cinv_, double *__restrict__ pss,
                                                   double *__restrict__ psz, val_t *__restrict__ p_out, int plain, int npc, const LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const val_t d2 = plain ? (val_t)0 : (val_t)S->damp2;
    const val_t *__restrict__ cinv = plain ? nullptr : cinv_;
    const bool damped = d2 != (val_t)0;
    double ass = 0.0, asz = 0.0;
    if ((int)blockIdx.x < npc)
        sv_walk_loaded<LsNormal>(
            cols, npc,
            [&](auto at, auto &t) {
                t.s = at(sv);
                if (damped) t.x = at(x);
                if (cinv) t.c = at(cinv);
            },
            [&](auto at, const auto &t) {
                auto ns = t.s;
                if (damped) { ns = t.s - d2 * t.x; at.put(sv, ns); }
                const auto z = cinv ? t.c * ns : ns;
                if (p_out) at.put(p_out, z);
                sv_mac(ass, ns, ns);
                if (cinv) sv_mac(asz, ns, z);
            });
    const double tss = block_sum(ass, s);
    if (threadIdx.x == 0) pss[blockIdx.x] = tss;
    if (cinv) {   // (without cinv: s.z is s.s, and psz is pss)
        const double tsz = block_sum(asz, s);
        if (threadIdx.x == 0) psz[blockIdx.x] = tsz;
    }
}

template <class T> struct LsDirection { T s, p, c; };
__global__ __launch_bounds__(SVB) void k_ls_direction(long long cols, const val_t *__restrict__ sv, val_t *__restrict__ p, const val_t *__restrict__ cinv,
                                                      const double *__restrict__ pss, const double *__restrict__ psz, const double *__restrict__ prr, int npr, int npc,
                                                      LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double g_new = fold(psz, npc, s), gamma = S->gamma;
    const val_t beta = (val_t)((gamma > 0.0 && !S->breakdown) ? g_new / gamma : 0.0);
    if (blockIdx.x == 0) {   // what the host reads
        const double nn = cinv ? fold(pss, npc, s) : g_new, rr = fold(prr, npr, s);
        if (threadIdx.x == 0) { S->nn = nn; S->rr = rr; S->iterations = S->iterations + 1; }
    }
    if ((int)blockIdx.x < npc)
        sv_walk_loaded<LsDirection>(
            cols, npc,
            [&](auto at, auto &t) {
                t.s = at(sv); t.p = at(p);
                if (cinv) t.c = at(cinv);
            },
            [&](auto at, const auto &t) {
                const auto z = cinv ? t.c * t.s : t.s;
                at.put(p, z + beta * t.p);
            });
}

// the start of a solve: r = b - A x (Ax holds the product), partial sums of r.r and b.b; the damping of this solve goes into the scalar block
__global__ __launch_bounds__(SVB) void k_ls_begin_r(long long rows, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ r, double *__restrict__ prr,
                                                    double *__restrict__ pbb, double damp2, int npr, LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    double arr = 0.0, abb = 0.0;
    if ((int)blockIdx.x < npr)
        sv_walk(rows, npr, [&](auto at) {
            const auto vb = at(b), nr = vb - at(Ax);
            at.put(r, nr);
            sv_mac(arr, nr, nr);
            sv_mac(abb, vb, vb);
        });
    if (blockIdx.x == 0 && threadIdx.x == 0) S->damp2 = damp2;
    const double trr = block_sum(arr, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) { prr[blockIdx.x] = trr; pbb[blockIdx.x] = tbb; }
}
// ... and its scalars (one workgroup)
__global__ __launch_bounds__(SVB) void k_ls_begin_fold(const double *__restrict__ pss, const double *__restrict__ psz, const double *__restrict__ pn0, const double *__restrict__ prr,
                                                       const double *__restrict__ pbb, int npr, int npc, LsScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double ss = fold(pss, npc, s), sz = fold(psz, npc, s), n0 = fold(pn0, npc, s), rr = fold(prr, npr, s), bb = fold(pbb, npr, s);
    if (threadIdx.x == 0) { S->gamma = sz; S->nn = ss; S->nn0 = n0; S->rr = rr; S->bb = bb; S->iterations = 0; S->breakdown = 0; }
}

// one row per thread: the squares of the row's stored values, added in storage order (through src: the rows of A^T as positions of A's value array = A's column norms)
__global__ __launch_bounds__(SVB) void k_csr_row_sqnorms(int rows, const int *__restrict__ rp, const int *__restrict__ src, const val_t *__restrict__ v, val_t *__restrict__ out,
                                                         int invert)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    double a = 0.0;
    for (long long k = rp[i]; k < rp[i + 1]; k++) {
        const double e = (double)v[src ? (long long)src[k] : k];
        a += e * e;
    }
    const val_t d = (val_t)a;
    out[i] = !invert ? d : SV_INVERSE_OR_ONE(d);
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_cgls {
    tilespmv_plan *A = nullptr, *AT = nullptr;   // borrowed
    long long rows = 0, cols = 0;
    int npr = 0, npc = 0, grid = 0;              // partials of row-length and of column-length sums; workgroups of the kernels that walk both lengths
    const val_t *cinv = nullptr;                 // borrowed
    void *block = nullptr;                       // the one allocation: r, q, p, s, the partial-sum arrays, the scalar block
    val_t *r = nullptr, *q = nullptr, *p = nullptr, *s = nullptr;
    double *pqq = nullptr, *ppp = nullptr, *prr = nullptr, *pss = nullptr, *psz = nullptr, *pbb = nullptr, *pn0 = nullptr;
    LsScal *S = nullptr;
};

extern "C" int tilespmv_cgls_create(tilespmv_cgls **ls, tilespmv_plan *plan_A, tilespmv_plan *plan_AT, const MAT_VAL_TYPE *d_cinv)
{
    if (ls) *ls = nullptr;
    if (!ls || !plan_A || !plan_AT) return (int)hipErrorInvalidValue;
    const long long rows = plan_A->matrix_rows, cols = plan_A->dev.colA;
    if (rows <= 0 || cols <= 0 || !whole_plan(plan_A, rows, cols) || !whole_plan(plan_AT, cols, rows)) return (int)hipErrorInvalidValue;   // whole plans of a rows x cols matrix and its transpose
    if (misaligned(d_cinv)) return (int)hipErrorInvalidValue;
    const size_t vr = vec_bytes(rows), vc = vec_bytes(cols), parts = SV_PARTS_BYTES;
    DeviceBlock blk;
    const hipError_t e = blk.alloc(2 * vr + 2 * vc + 7 * parts + 256);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_cgls();
    c->A = plan_A; c->AT = plan_AT; c->rows = rows; c->cols = cols; c->cinv = d_cinv; c->block = blk.base;
    c->npr = solver_parts(rows); c->npc = solver_parts(cols); c->grid = std::max(c->npr, c->npc);
    c->r = blk.take<val_t>(vr);
    c->q = blk.take<val_t>(vr);
    c->p = blk.take<val_t>(vc);
    c->s = blk.take<val_t>(vc);
    c->pqq = blk.take<double>(parts);
    c->ppp = blk.take<double>(parts);
    c->prr = blk.take<double>(parts);
    c->pss = blk.take<double>(parts);
    double *const sz = blk.take<double>(parts);
    c->psz = d_cinv ? sz : c->pss;
    c->pbb = blk.take<double>(parts);
    c->pn0 = blk.take<double>(parts);
    c->S = blk.take<LsScal>(256);
    *ls = c;
    return 0;
}

extern "C" void tilespmv_cgls_destroy(tilespmv_cgls *ls) { destroy_solver(ls); }

extern "C" int tilespmv_cgls_begin(tilespmv_cgls *ls, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double damp, void *stream)
{
    if (!ls || !d_b || !d_x || misaligned(d_b) || misaligned(d_x) || !(damp * damp >= 0.0) || !(damp * damp < 1e300)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    int rc = tilespmv_plan_spmv(ls->A, d_x, ls->q, stream);                       // q = A x
    if (rc) return rc;
    hipLaunchKernelGGL(k_ls_begin_r, dim3(ls->npr), dim3(SVB), 0, st, ls->rows, d_b, ls->q, ls->r, ls->prr, ls->pbb, damp * damp, ls->npr, ls->S);
    rc = tilespmv_plan_spmv(ls->AT, d_b, ls->s, stream);                          // s = A^T b, for |A^T b|^2 alone
    if (rc) return rc;
    hipLaunchKernelGGL(k_ls_normal, dim3(ls->npc), dim3(SVB), 0, st, ls->cols, ls->s, d_x, ls->cinv, ls->pn0, ls->pn0, (val_t *)nullptr, 1, ls->npc, ls->S);
    rc = tilespmv_plan_spmv(ls->AT, ls->r, ls->s, stream);                        // s = A^T r
    if (rc) return rc;
    hipLaunchKernelGGL(k_ls_normal, dim3(ls->npc), dim3(SVB), 0, st, ls->cols, ls->s, d_x, ls->cinv, ls->pss, ls->psz, ls->p, 0, ls->npc, ls->S);
    hipLaunchKernelGGL(k_ls_begin_fold, dim3(1), dim3(SVB), 0, st, ls->pss, ls->psz, ls->pn0, ls->prr, ls->pbb, ls->npr, ls->npc, ls->S);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_cgls_iterate(tilespmv_cgls *ls, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!ls || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++) {
        int rc = tilespmv_plan_spmv(ls->A, ls->p, ls->q, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_ls_dot, dim3(ls->grid), dim3(SVB), 0, st, ls->rows, ls->cols, ls->q, ls->p, ls->pqq, ls->ppp, ls->psz, ls->npr, ls->npc, ls->S);
        hipLaunchKernelGGL(k_ls_update, dim3(ls->grid), dim3(SVB), 0, st, ls->rows, ls->cols, ls->p, ls->q, d_x, ls->r, ls->pqq, ls->ppp, ls->prr, ls->npr, ls->npc, ls->S);
        rc = tilespmv_plan_spmv(ls->AT, ls->r, ls->s, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_ls_normal, dim3(ls->npc), dim3(SVB), 0, st, ls->cols, ls->s, d_x, ls->cinv, ls->pss, ls->psz, (val_t *)nullptr, 0, ls->npc, ls->S);
        hipLaunchKernelGGL(k_ls_direction, dim3(ls->npc), dim3(SVB), 0, st, ls->cols, ls->s, ls->p, ls->cinv, ls->pss, ls->psz, ls->prr, ls->npr, ls->npc, ls->S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// the scalar block as a whole tilespmv_cgls_state: converged is nn = 0, the normal residual
static tilespmv_cgls_state cgls_state_of(const LsScal &h)
{
    tilespmv_cgls_state s;
    memset(&s, 0, sizeof(s));
    s.size = sizeof(s);
    s.iterations = h.iterations;
    s.status = device_status(h.breakdown, h.nn);
    s.nn = h.nn; s.nn0 = h.nn0; s.rr = h.rr; s.bb = h.bb;
    return s;
}
// the convergence test of tilespmv_cgls_solve: nn <= rtol^2 nn0, and A^T b = 0 (b = 0, or b orthogonal to the range of A) has the solution 0, whose residual is b
struct NormalTest {
    static double residual(const tilespmv_cgls_state &s) { return s.nn; }
    static double scale(const tilespmv_cgls_state &s) { return s.nn0; }
    static void at_zero_scale(tilespmv_cgls_state &s) { s.nn = 0.0; s.rr = s.bb; }
};

extern "C" int tilespmv_cgls_state_read(tilespmv_cgls *ls, void *stream, tilespmv_cgls_state *out)
{
    if (!ls) return (int)hipErrorInvalidValue;
    return state_read(ls->S, (hipStream_t)stream, out, cgls_state_of);
}

extern "C" int tilespmv_cgls_solve(tilespmv_cgls *ls, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double damp, double rtol, int maxiter, int check_every, void *stream,
                                   tilespmv_cgls_state *out)
{
    if (!ls) return (int)hipErrorInvalidValue;
    return solve_loop<NormalTest>(
        out, d_x, ls->cols, rtol, maxiter, check_every, (hipStream_t)stream, [&] { return tilespmv_cgls_begin(ls, d_b, d_x, damp, stream); },
        [&] { return tilespmv_cgls_state_read(ls, stream, out); }, [&](int count) { return tilespmv_cgls_iterate(ls, d_x, count, stream); });
}

extern "C" int tilespmv_csr_row_sqnorms_device(int rows, const MAT_PTR_TYPE *d_rowPtr, const int *d_src, const MAT_VAL_TYPE *d_val, MAT_VAL_TYPE *d_out, int invert, void *stream)
{
    return launch_per_row(k_csr_row_sqnorms, rows, d_rowPtr, d_src, true, d_val, d_out, invert, stream);
}
