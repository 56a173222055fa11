// hip_solver_gm.hip — the entry points tilespmv_gmres_*  and the form of the solver whose basis is stored in the value type: the kernels and launch
// sequences of hip_solver_gm.h with BT = val_t.  The narrow form of tilespmv_gmres_create_basis is hip_solver_gm_cb.hip's; this file reaches it through its GmForm alone.
#include "hip_solver_gm.h"

using namespace tilespmv;

// bytes of one stored basis vector of `rows` elements of `basis_bytes` each inside the allocation: 16 rows of slack, rounded to 256 (vec_bytes for the value type)
static size_t gm_basis_vec_bytes(long long rows, int basis_bytes) { return ((size_t)(rows + 16) * (size_t)basis_bytes + 255) / 256 * 256; }

// what basis_bytes asks for: sizeof(val_t) (0 and the value type's own size), 4 in the fp64 library, or 0: refuse
static int gm_basis_of(int basis_bytes)
{
    if (basis_bytes == TILESPMV_GMRES_BASIS_VALUE || basis_bytes == (int)sizeof(val_t)) return (int)sizeof(val_t);
#ifndef TILESPMV_F32
    if (basis_bytes == TILESPMV_GMRES_BASIS_FLOAT) return TILESPMV_GMRES_BASIS_FLOAT;
#endif
    return 0;
}

// the creates: a diagonal (d_dinv, may be NULL) or a block-Jacobi object (bj), never both; basis_bytes as tilespmv_gmres_create_basis takes it
static int gm_create(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const val_t *d_dinv, const tilespmv_block_jacobi *bj, int basis_bytes)
{
    const int basis = gm_basis_of(basis_bytes);
    if (restart < 1 || restart > GM_MAX_RESTART || !basis || (d_dinv && bj)) {   // (before the plan is looked at)
        if (gs) *gs = nullptr;
        return (int)hipErrorInvalidValue;
    }
    const long long n = square_system(gs, plan, d_dinv);
    if (!n || (bj && bj->rows != n)) return (int)hipErrorInvalidValue;
    const bool narrow_basis = basis != (int)sizeof(val_t);
    const int np = gm_parts(n);
    const size_t parts = ((size_t)np * sizeof(double) + 255) / 256 * 256, sums = (size_t)(restart + 1) * parts, vec = vec_bytes(n), bvec = gm_basis_vec_bytes(n, basis);
    const size_t rbytes = (size_t)GM_MAX_RESTART * GM_MAX_RESTART * sizeof(double), small = 768;   // small: up to GM_MAX_RESTART + 1 doubles, rounded to 256
    const bool hats = d_dinv || bj, cur = narrow_basis && !d_dinv;   // zhat; vcur
    const size_t bytes = (size_t)(restart + 1) * bvec + (size_t)(2 + (hats ? 1 : 0) + (cur ? 1 : 0)) * vec + 2 * sums + 2 * parts + rbytes + 4 * small + 256;
    DeviceBlock blk;
    const hipError_t e = blk.alloc(bytes);
    if (e != hipSuccess) return (int)e;
    auto *c = new tilespmv_gmres();
    c->plan = plan; c->n = n; c->stride = (long long)(bvec / (size_t)basis); c->np = np; c->restart = restart; c->dinv = d_dinv; c->bj = bj; c->block = blk.base;
    c->basis_bytes = basis; c->bytes = bytes;
#ifndef TILESPMV_F32
    c->form = narrow_basis ? gm_float_form() : gm_form<val_t>();
#else
    c->form = gm_form<val_t>();
#endif
    c->V = blk.take<char>((size_t)(restart + 1) * bvec);
    c->w = blk.take<val_t>(vec);
    c->b = blk.take<val_t>(vec);
    c->zhat = hats ? blk.take<val_t>(vec) : nullptr;
    c->vcur = cur ? blk.take<val_t>(vec) : nullptr;
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

extern "C" int tilespmv_gmres_create(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const MAT_VAL_TYPE *d_dinv)
{
    return gm_create(gs, plan, restart, d_dinv, nullptr, TILESPMV_GMRES_BASIS_VALUE);
}

extern "C" int tilespmv_gmres_create_block(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const tilespmv_block_jacobi *bj)
{
    if (!bj) {
        if (gs) *gs = nullptr;
        return (int)hipErrorInvalidValue;
    }
    return gm_create(gs, plan, restart, nullptr, bj, TILESPMV_GMRES_BASIS_VALUE);
}

extern "C" int tilespmv_gmres_create_basis(tilespmv_gmres **gs, tilespmv_plan *plan, int restart, const MAT_VAL_TYPE *d_dinv, const tilespmv_block_jacobi *bj, int basis_bytes)
{
    return gm_create(gs, plan, restart, d_dinv, bj, basis_bytes);
}

extern "C" int tilespmv_gmres_basis_bytes(const tilespmv_gmres *gs) { return gs ? gs->basis_bytes : 0; }

extern "C" size_t tilespmv_gmres_workspace_bytes(const tilespmv_gmres *gs) { return gs ? gs->bytes : 0; }

extern "C" void tilespmv_gmres_destroy(tilespmv_gmres *gs) { destroy_solver(gs); }

extern "C" int tilespmv_gmres_begin(tilespmv_gmres *gs, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!gs || !d_b || !d_x || misaligned(d_b) || misaligned(d_x)) return (int)hipErrorInvalidValue;
    return gs->form->open(gs, d_b, d_x, (hipStream_t)stream);
}

extern "C" int tilespmv_gmres_iterate(tilespmv_gmres *gs, MAT_VAL_TYPE *d_x, int count, void *stream)
{
    if (!gs || !d_x || misaligned(d_x) || count < 0) return (int)hipErrorInvalidValue;
    return gs->form->iterate(gs, d_x, count, (hipStream_t)stream);
}

extern "C" int tilespmv_gmres_flush(tilespmv_gmres *gs, MAT_VAL_TYPE *d_x, void *stream)
{
    if (!gs || !d_x || misaligned(d_x)) return (int)hipErrorInvalidValue;
    gs->form->close(gs, d_x, (hipStream_t)stream);
    return gs->form->open(gs, gs->b, d_x, (hipStream_t)stream);
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
    const auto begin = [&] { return tilespmv_gmres_begin(gs, d_b, d_x, stream); };
    const auto read = [&] { return tilespmv_gmres_state_read(gs, stream, out); };
    const auto iterate = [&](int count) { return tilespmv_gmres_iterate(gs, d_x, count, stream); };
    int rc;
    if (gs->basis_bytes == (int)sizeof(val_t)) {
        rc = solve_loop<RrBbTest>(out, d_x, gs->n, rtol, maxiter, check_every, (hipStream_t)stream, begin, read, iterate);
    } else {
        // A narrow basis: inside a cycle the true residual stops near eps32 x the residual the cycle began with while the recurrence's rr keeps falling, so CONVERGED is accepted
        // on a recomputed rr alone: flush, read again, test again; a failed test carries on from the fresh cycle.
        rc = solve_loop<RrBbTest>(out, d_x, gs->n, rtol, maxiter, check_every, (hipStream_t)stream, begin, read, iterate, [&](bool &accepted) {
            if (gs->pos == 0) return 0;      // (the state read is that of an open)
            int e = tilespmv_gmres_flush(gs, d_x, stream);
            if (!e) e = read();
            if (!e) accepted = out->status != TILESPMV_CG_BREAKDOWN && out->rr <= rtol * rtol * out->bb;
            return e;
        });
        if (!rc && gs->pos == 0) return rc;      // the decision was taken on a flushed state: x is current and rr is its recomputed residual
    }
    if (rc || out->bb == 0.0) return rc;   // (b = 0: x is 0 and rr says so)
    // x is current only after a close: flush, and report the recomputed |b - A x|^2 of the x that is returned under the status and the count of the decision
    const int status = out->status, iterations = out->iterations;
    rc = tilespmv_gmres_flush(gs, d_x, stream);
    if (!rc) rc = tilespmv_gmres_state_read(gs, stream, out);
    if (!rc) { out->status = status; out->iterations = iterations; }
    return rc;
}
