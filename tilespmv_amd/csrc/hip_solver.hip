// hip_solver.hip — conjugate gradients around a resident plan (tilespmv_cg_*, tilespmv_csr_diagonal_device).
//
// One iteration is the plan's own product Ap = A p (tilespmv_plan_spmv: whatever launch form the plan has) and three streaming kernels:
//   k_cg_dot        reads p, Ap                     partial sums of p.Ap, one per workgroup
//   k_cg_update     reads p, Ap, x, r (, dinv)      alpha = rho / p.Ap;  x += alpha p;  r -= alpha Ap;  partial sums of r.r and (Jacobi) r.z, z = dinv o r
//   k_cg_direction  reads r, p (, dinv)             beta = rho_new / rho;  p = z + beta p  (z recomputed from r and dinv, never stored)
// With a block-Jacobi object (tilespmv_cg_create_block; hip_precond.hip) z is a stored vector: k_cg_update runs with dinv = NULL (r.r partials only), k_bj_apply forms
// z = M^-1 r and the r.z partials, and k_cg_zstep replaces k_cg_direction — four launches, (13 + bs) n elements.  The kernels above are the same code either way.
// An FSAI object (tilespmv_cg_create_fsai; hip_fsai.hip) takes the same stored-z path: z = G^T (G r) by its two plans and one pass for the r.z partials.
// 11 n vector elements per iteration (13 n with Jacobi).  The launch shape and the partial sums with their fixed order of additions are those of hip_solver_common.h, and so is the
// walk over a vector: every kernel here hands its body, written once for lane vectors and tail elements alike, to sv_dot, sv_walk_loaded (the kernels of the iteration: a trip's loads
// before its arithmetic) or sv_walk.  The number of partials is solver_parts(n).  alpha and beta are rounded to the value type once, where they multiply.
//
// The scalar block (CgScal) has ONE writing kernel per field and no kernel reads a field it (or a concurrent workgroup of it) writes:
//   rho         k_cg_dot, workgroup 0 (fold of the r.z partials the previous update left; 0 after a breakdown)      read by k_cg_update, k_cg_direction
//   breakdown   k_cg_update, workgroup 0 (set, never cleared)                                                        read by k_cg_dot (workgroup 0), k_cg_direction
//   rr, iterations   k_cg_direction (k_cg_zstep with a block preconditioner), workgroup 0 (iterations: read and written by that workgroup alone)              read by the host (tilespmv_cg_state_read)
//   all of them      k_cg_begin_fold (one workgroup), at the start of a solve
// Guards (data-dependent branches, no host round trip): rho = 0 -> alpha = beta = 0, x and r stay as they are; rho > 0 and not p.Ap > 0 (or rho < 0: a preconditioner that is not
// positive definite) -> breakdown is set, alpha = beta = 0 in this and every later iteration, x keeps its last good value.
#include <hip/hip_runtime.h>

#include "hip_fsai.h"
#include "hip_precond.h"
#include "hip_solver_common.h"

namespace tilespmv {
namespace {

struct CgScal {
    double rho, rr, bb;
    int iterations, breakdown;
};

__global__ __launch_bounds__(SVB) void k_cg_dot(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, double *__restrict__ ppap, const double *__restrict__ prz,
                                                int np, CgScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    double acc = 0.0;
    sv_dot(n, gridDim.x, p, Ap, [&](auto a, auto b) { sv_mac(acc, a, b); });
    const double t = block_sum(acc, s);
    if (threadIdx.x == 0) ppap[blockIdx.x] = t;
    if (blockIdx.x == 0) {   // rho of this iteration, for the two kernels that follow
        const double rho = fold(prz, np, s);
        if (threadIdx.x == 0) S->rho = S->breakdown ? 0.0 : rho;
    }
}

template <class T> struct CgUpdate { T p, Ap, x, r, d; };
__global__ __launch_bounds__(SVB) void k_cg_update(long long n, const val_t *__restrict__ p, const val_t *__restrict__ Ap, val_t *__restrict__ x, val_t *__restrict__ r,
                                                   const val_t *__restrict__ dinv, const double *__restrict__ ppap, double *__restrict__ prr, double *__restrict__ prz, int np,
                                                   CgScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double pap = fold(ppap, np, s), rho = S->rho;
    const bool broke = rho < 0.0 || (rho > 0.0 && !(pap > 0.0));
    const val_t alpha = (val_t)((rho > 0.0 && pap > 0.0) ? rho / pap : 0.0);
    if (broke && blockIdx.x == 0 && threadIdx.x == 0) S->breakdown = 1;
    double arr = 0.0, arz = 0.0;
    sv_walk_loaded<CgUpdate>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.p = at(p); t.Ap = at(Ap); t.x = at(x); t.r = at(r);
            if (dinv) t.d = at(dinv);
        },
        [&](auto at, const auto &t) {
            const auto nx = t.x + alpha * t.p, nr = t.r - alpha * t.Ap;
            at.put(x, nx);
            at.put(r, nr);
            sv_mac(arr, nr, nr);
            if (dinv) sv_mac(arz, nr, t.d * nr);
        });
    const double trr = block_sum(arr, s);
    if (threadIdx.x == 0) prr[blockIdx.x] = trr;
    if (dinv) {   // (plain CG: r.z is r.r, and prz is prr)
        const double trz = block_sum(arz, s);
        if (threadIdx.x == 0) prz[blockIdx.x] = trz;
    }
}

template <class T> struct CgDirection { T r, p, d; };
__global__ __launch_bounds__(SVB) void k_cg_direction(long long n, const val_t *__restrict__ r, val_t *__restrict__ p, const val_t *__restrict__ dinv,
                                                      const double *__restrict__ prr, const double *__restrict__ prz, int np, CgScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double rho_new = fold(prz, np, s), rho = S->rho;
    const val_t beta = (val_t)((rho > 0.0 && !S->breakdown) ? rho_new / rho : 0.0);
    if (blockIdx.x == 0) {   // what the host reads
        const double rr = dinv ? fold(prr, np, s) : rho_new;
        if (threadIdx.x == 0) { S->rr = rr; S->iterations = S->iterations + 1; }
    }
    sv_walk_loaded<CgDirection>(
        n, gridDim.x,
        [&](auto at, auto &t) {
            t.r = at(r); t.p = at(p);
            if (dinv) t.d = at(dinv);
        },
        [&](auto at, const auto &t) {
            const auto z = dinv ? t.d * t.r : t.r;
            at.put(p, z + beta * t.p);
        });
}

// the start of a solve: r = b - A x (Ax holds the product), p = z, partial sums of r.r, r.z and b.b
__global__ __launch_bounds__(SVB) void k_cg_begin(long long n, const val_t *__restrict__ b, const val_t *__restrict__ Ax, val_t *__restrict__ r, val_t *__restrict__ p,
                                                  const val_t *__restrict__ dinv, double *__restrict__ prr, double *__restrict__ prz, double *__restrict__ pbb)
{
    __shared__ double s[SVB / 64];
    double arr = 0.0, arz = 0.0, abb = 0.0;
    sv_walk(n, gridDim.x, [&](auto at) {
        const auto vb = at(b), nr = vb - at(Ax);
        const auto z = dinv ? at(dinv) * nr : nr;
        at.put(r, nr);
        at.put(p, z);
        sv_mac(arr, nr, nr);
        sv_mac(arz, nr, z);
        sv_mac(abb, vb, vb);
    });
    const double trr = block_sum(arr, s), trz = block_sum(arz, s), tbb = block_sum(abb, s);
    if (threadIdx.x == 0) {
        prr[blockIdx.x] = trr; pbb[blockIdx.x] = tbb;
        if (dinv) prz[blockIdx.x] = trz;
    }
}
// ... and its scalars (one workgroup)
__global__ __launch_bounds__(SVB) void k_cg_begin_fold(const double *__restrict__ prr, const double *__restrict__ prz, const double *__restrict__ pbb, int np, CgScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double rr = fold(prr, np, s), rz = fold(prz, np, s), bb = fold(pbb, np, s);
    if (threadIdx.x == 0) { S->rho = rz; S->rr = rr; S->bb = bb; S->iterations = 0; S->breakdown = 0; }
}

// one row per thread: the stored entries (i, i), added in storage order
__global__ __launch_bounds__(SVB) void k_csr_diagonal(int rows, const int *__restrict__ rp, const int *__restrict__ ci, const val_t *__restrict__ v, val_t *__restrict__ out, int invert)
{
    const long long i = (long long)blockIdx.x * SVB + threadIdx.x;
    if (i >= rows) return;
    double a = 0.0;
    for (long long k = rp[i]; k < rp[i + 1]; k++)
        if (ci[k] == (int)i) a += (double)v[k];
    const val_t d = (val_t)a;
    out[i] = !invert ? d : SV_INVERSE_OR_ONE(d);
}

// the direction with a STORED z (block Jacobi: z = M^-1 r and the r.z partials come from k_bj_apply, hip_precond.hip): beta = rho_new / rho;  p = z + beta p.  The scalars are
// k_cg_direction's, with rr folded from the r.r partials of k_cg_update (k_cg_direction with z in r's place would take rr = rho_new).
template <class T> struct CgZstep { T z, p; };
__global__ __launch_bounds__(SVB) void k_cg_zstep(long long n, const val_t *__restrict__ z, val_t *__restrict__ p, const double *__restrict__ prr, const double *__restrict__ prz,
                                                  int np, CgScal *__restrict__ S)
{
    __shared__ double s[SVB / 64];
    const double rho_new = fold(prz, np, s), rho = S->rho;
    const val_t beta = (val_t)((rho > 0.0 && !S->breakdown) ? rho_new / rho : 0.0);
    if (blockIdx.x == 0) {   // what the host reads
        const double rr = fold(prr, np, s);
        if (threadIdx.x == 0) { S->rr = rr; S->iterations = S->iterations + 1; }
    }
    sv_walk_loaded<CgZstep>(
        n, gridDim.x, [&](auto at, auto &t) { t.z = at(z); t.p = at(p); }, [&](auto at, const auto &t) { at.put(p, t.z + beta * t.p); });
}

}  // namespace
}  // namespace tilespmv

using namespace tilespmv;

struct tilespmv_cg {
    tilespmv_plan *plan = nullptr;
    long long n = 0;
    int np = 0;
    const val_t *dinv = nullptr;   // borrowed
    const tilespmv_block_jacobi *bj = nullptr;   // borrowed (tilespmv_cg_create_block; then dinv is NULL and z is a vector)
    tilespmv_fsai *fsai = nullptr;               // borrowed (tilespmv_cg_create_fsai; likewise)
    void *block = nullptr;         // the one allocation: r, p, Ap (, z), the partial-sum arrays, the scalar block
    val_t *r = nullptr, *p = nullptr, *Ap = nullptr, *z = nullptr;
    double *ppap = nullptr, *prr = nullptr, *prz = nullptr, *pbb = nullptr;
    CgScal *S = nullptr;
};

// the three creates: a diagonal (d_dinv, may be NULL), a block-Jacobi object (bj) or an FSAI object (fsai), never two of them; with an object z is a stored vector
static int cg_create(tilespmv_cg **cg, tilespmv_plan *plan, const val_t *d_dinv, const tilespmv_block_jacobi *bj, tilespmv_fsai *fsai)
{
    const long long n = square_system(cg, plan, d_dinv);
    if (!n || (bj && bj->rows != n) || (fsai && fsai->rows != n)) return (int)hipErrorInvalidValue;
    const size_t vec = vec_bytes(n), parts = SV_PARTS_BYTES;
    const bool stored_z = bj || fsai;
    DeviceBlock blk;
    const hipError_t e = blk.alloc((stored_z ? 4 : 3) * vec + 4 * parts + 256);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_cg();
    c->plan = plan; c->n = n; c->np = solver_parts(n); c->dinv = d_dinv; c->bj = bj; c->fsai = fsai; c->block = blk.base;
    c->r = blk.take<val_t>(vec);
    c->p = blk.take<val_t>(vec);
    c->Ap = blk.take<val_t>(vec);
    if (stored_z) c->z = blk.take<val_t>(vec);
    c->ppap = blk.take<double>(parts);
    c->prr = blk.take<double>(parts);
    double *const rz = blk.take<double>(parts);
    c->prz = (d_dinv || stored_z) ? rz : c->prr;
    c->pbb = blk.take<double>(parts);
    c->S = blk.take<CgScal>(256);
    *cg = c;
    return 0;
}

extern "C" int tilespmv_cg_create(tilespmv_cg **cg, tilespmv_plan *plan, const MAT_VAL_TYPE *d_dinv)
{
    return cg_create(cg, plan, d_dinv, nullptr, nullptr);
}

extern "C" int tilespmv_cg_create_block(tilespmv_cg **cg, tilespmv_plan *plan, const tilespmv_block_jacobi *bj)
{
    if (!bj) {
        if (cg) *cg = nullptr;
        return (int)hipErrorInvalidValue;
    }
    return cg_create(cg, plan, nullptr, bj, nullptr);
}

extern "C" int tilespmv_cg_create_fsai(tilespmv_cg **cg, tilespmv_plan *plan, tilespmv_fsai *f)
{
    if (!f) {
        if (cg) *cg = nullptr;
        return (int)hipErrorInvalidValue;
    }
    return cg_create(cg, plan, nullptr, nullptr, f);
}

// z = M^-1 r and the r.z partials by the solver's object (a stored z: cg->z is not NULL)
static int cg_precondition(const tilespmv_cg *cg, val_t *z, hipStream_t st)
{
    if (cg->fsai) return fsai_launch(cg->fsai, cg->r, z, cg->prz, st);
    block_jacobi_launch(cg->bj, cg->r, z, cg->prz, st);
    return 0;
}

extern "C" void tilespmv_cg_destroy(tilespmv_cg *cg) { destroy_solver(cg); }

extern "C" int tilespmv_cg_begin(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!cg || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = tilespmv_plan_spmv(cg->plan, d_x, cg->Ap, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cg_begin, dim3(cg->np), dim3(SVB), 0, st, cg->n, d_b, cg->Ap, cg->r, cg->p, cg->dinv, cg->prr, cg->prz, cg->pbb);
    if (cg->z) {   // p = z = M^-1 r, and the r.z partials
        const int rcz = cg_precondition(cg, cg->p, st);
        if (rcz) return rcz;
    }
    hipLaunchKernelGGL(k_cg_begin_fold, dim3(1), dim3(SVB), 0, st, cg->prr, cg->prz, cg->pbb, cg->np, cg->S);
    return (int)hipGetLastError();
}

extern "C" int tilespmv_cg_iterate(tilespmv_cg *cg, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!cg || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < count; i++) {
        const int rc = tilespmv_plan_spmv(cg->plan, cg->p, cg->Ap, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cg_dot, dim3(cg->np), dim3(SVB), 0, st, cg->n, cg->p, cg->Ap, cg->ppap, cg->prz, cg->np, cg->S);
        hipLaunchKernelGGL(k_cg_update, dim3(cg->np), dim3(SVB), 0, st, cg->n, cg->p, cg->Ap, d_x, cg->r, cg->dinv, cg->ppap, cg->prr, cg->prz, cg->np, cg->S);
        if (cg->z) {   // (k_cg_update left the r.r partials only)
            const int rcz = cg_precondition(cg, cg->z, st);
            if (rcz) return rcz;
            hipLaunchKernelGGL(k_cg_zstep, dim3(cg->np), dim3(SVB), 0, st, cg->n, cg->z, cg->p, cg->prr, cg->prz, cg->np, cg->S);
        } else
            hipLaunchKernelGGL(k_cg_direction, dim3(cg->np), dim3(SVB), 0, st, cg->n, cg->r, cg->p, cg->dinv, cg->prr, cg->prz, cg->np, cg->S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int tilespmv_cg_state_read(tilespmv_cg *cg, void *stream, tilespmv_cg_state *out)
{
    if (!cg) return (int)hipErrorInvalidValue;
    return state_read(cg->S, (hipStream_t)stream, out, cg_state_of<CgScal>);
}

extern "C" int tilespmv_cg_solve(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                                 tilespmv_cg_state *out)
{
    if (!cg) return (int)hipErrorInvalidValue;
    return solve_loop<RrBbTest>(
        out, d_x, cg->n, rtol, maxiter, check_every, (hipStream_t)stream, [&] { return tilespmv_cg_begin(cg, d_b, d_x, stream); },
        [&] { return tilespmv_cg_state_read(cg, stream, out); }, [&](int count) { return tilespmv_cg_iterate(cg, d_x, count, stream); });
}

extern "C" int tilespmv_csr_diagonal_device(int rows, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_VAL_TYPE *d_out, int invert,
                                            void *stream)
{
    return launch_per_row(k_csr_diagonal, rows, d_csrRowPtr, d_csrColIdx, false, d_csrVal, d_out, invert, stream);
}
