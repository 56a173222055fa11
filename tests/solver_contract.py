"""Five promises that every single-system device-resident solver makes (tilespmv_{cg,cgls,bicgstab,minres,gmres}_*; include/tilespmv.h),
each written once:

  the sums have a fixed order; begin and iterate can be captured into a HIP graph; a solver follows a value refresh of its plan and of its borrowed diagonal; create refuses what
  it must; nothing behind the end of a caller's vector is touched.

SOLVERS is the table of what differs: the class and its entry point, the mirror, the named inputs, the diagonal on the host and on the device, the counts and the caps, each
value where the solver's own test had it.  tests/test_gpu_solver_contract.py runs graph capture and past-the-end for every row of the table; fixed order, value refresh and the
refusals are still called from the tests of those names in tests/test_gpu_{cg,cgls,bicgstab,minres,gmres}.py, which keep their node ids until they can move too.  This module
imports no test file.  Plans are created with deterministic=1, placement_tries=1 and sixteen sentinel elements stand behind every device vector (tests/gpu_solver_util.py)."""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import bicgstab_mirror
import cg_mirror
import cgls_mirror
import gmres_mirror
import gpu_solver_util as U
import minres_mirror
from gpu_solver_util import PRODUCT_TOL
from tilespmv_amd import _lib, api, generators as G


# ---- what the table is made of
def _diagonal_on_device(fn):
    """The device-side builder of a square solver's diagonal, api.csr_diagonal_device or api.csr_abs_diagonal_device, as fill(values, out, stream)."""
    def prepare(torch, dims, rpd, cid, dt):
        return lambda vd, out, st: fn(dims[0], rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=True, stream=st, dtype=dt)
    return prepare


def _column_scaling_on_device(torch, dims, rpd, cid, dt):
    """CGLS: cinv through the srcT of one device transposition of the pattern."""
    rpT, srcT = U.transpose_pattern(torch, dims[0], dims[1], rpd, cid, dt)
    return lambda vd, out, st: api.csr_row_sqnorms_device(dims[1], rpT.data_ptr(), srcT.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=True, stream=st, dtype=dt)


def _spsolve(M):
    return lambda dims, rp, ci, vt, b: M.spsolve_x(dims[0], rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _reversed_start(M):
    return lambda nx, dt: (0.01 * M.rhs(nx)[::-1]).astype(dt)


def _random_5003(case, dt):
    """5003 rows (3 mod 4: a scalar tail in both value types), 5 random off-diagonal entries per row in (-1, 1) and a diagonal of 8."""
    n = 5003
    rng = np.random.default_rng(29)
    r, c = np.repeat(np.arange(n), 5), rng.integers(0, n, n * 5)
    off = r != c
    _, _, rp, ci = G.from_coo(n, n, np.concatenate([r[off], np.arange(n)]), np.concatenate([c[off], np.arange(n)]))
    rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
    rows = np.repeat(np.arange(n), np.diff(rp))
    return [("5003 rows", (n,), rp, ci, np.where(ci == rows, 8.0, rng.uniform(-1, 1, len(ci))).astype(dt))]


def _cg_past_inputs(case, dt):
    """A row count that is a multiple of 16 and one that leaves a partial 16-byte vector at the end (2067 rows), degree + 1 on the diagonal (Gershgorin puts the condition number
    below 50)."""
    out = []
    for label, (m, n, rp, ci) in (("fem12", G.fem_hex(12, 12, 12, 3)), ("tri53x39", G.tri_mesh(53, 39))):
        assert m == n and (label == "fem12" or n % 4 == 3)
        rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
        out.append((label, (n,), rp, ci, cg_mirror.spd_values(n, rp, ci).astype(dt)))
    return out


def _cgls_past_inputs(case, dt):
    """Row and column counts that are multiples neither of 16 nor of the lane vector width."""
    rows, cols = case["shape"]
    assert rows % 4 == 3 or cols % 4 == 3
    rng = np.random.default_rng(29)
    k = min(rows, cols)
    _, _, rp, ci = G.from_coo(rows, cols, np.concatenate([np.repeat(np.arange(rows), 5), np.arange(k)]), np.concatenate([rng.integers(0, cols, rows * 5), np.arange(k)]))
    return [("%d x %d" % (rows, cols), (rows, cols), rp, ci, (rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))).astype(dt))]


def _cg_early(torch, dt, plan, A, b, dinv, dims, label):
    """Three iterations against the mirror, within 100 x the per-product tolerance.  (b, x, the diagonal, the solver: the solve that follows runs on this handle.)"""
    n, st, jacobi = dims[0], U.stream(torch), dinv is not None
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    dd = U.vec(torch, dinv, n, dt) if jacobi else None
    m3 = cg_mirror.Mirror(A, dt, dinv); m3.begin(b); m3.iterate(3)
    cg = api.CG(plan, dd.data_ptr() if jacobi else None)
    cg.begin(bd.data_ptr(), xd.data_ptr(), st)
    cg.iterate(xd.data_ptr(), 3, st)
    s = cg.state(st)
    dx = U.relerr(U.host(xd, n), m3.x)
    print("%s %s jacobi=%s: 3 iterations, |x - mirror| / |mirror| = %.3g, rr %.6g (mirror %.6g)" % (label, dt, jacobi, dx, s["rr"], m3.rr))
    assert dx <= 100 * PRODUCT_TOL[dt] and abs(s["rr"] - m3.rr) <= 100 * PRODUCT_TOL[dt] * m3.rr
    return bd, xd, dd, cg


def _cgls_early(torch, dt, op, A, b, cinv, dims, label):
    """Three damped, column-scaled iterations against the mirror, within 100 x the per-product tolerance.  (b, x, cinv, the solver: the solve that follows runs on this handle.)"""
    (rows, cols), st = dims, U.stream(torch)
    m3 = cgls_mirror.Mirror(A, dt, cinv); m3.begin(b, damp=0.5); m3.iterate(3)
    bd, xd, cd = U.vec(torch, b, rows, dt), U.vec(torch, None, cols, dt), U.vec(torch, cinv, cols, dt)
    ls = api.CGLS(op.A, op.AT, cd.data_ptr())
    ls.begin(bd.data_ptr(), xd.data_ptr(), 0.5, st)
    ls.iterate(xd.data_ptr(), 3, st)
    s = ls.state(st)
    dx = U.relerr(U.host(xd, cols), m3.x)
    print("%s %s: 3 iterations, |x - mirror| / |mirror| = %.3g, nn %.6g (mirror %.6g)" % (label, dt, dx, s["nn"], m3.nn))
    assert dx <= 100 * PRODUCT_TOL[dt] and U.dist(s["nn"], m3.nn) <= 100 * PRODUCT_TOL[dt] and U.dist(s["rr"], m3.rr) <= 100 * PRODUCT_TOL[dt]
    return bd, xd, cd, ls


def _square_refusals(spec, torch, dt, stack):
    """A non-square plan (a rectangular operator's A), a shard plan, a misaligned diagonal; an aligned diagonal is accepted.  (refused, accepted, what must stay alive)."""
    (n,), rp, ci, vt, b = _system(spec, spec.refuse_input, dt)
    half = n // 2
    op = stack.enter_context(U.square_op(n, rp, ci, vt, dt))
    rect = stack.enter_context(U.rect_op(half, n, rp[: half + 1].copy(), ci[: rp[half]].copy(), vt[: rp[half]].copy(), dt))
    shard = U.square_plan(n, rp, ci, vt, dt, tilerow_end=((n + 15) // 16) // 2)
    stack.callback(shard.close)
    d = U.vec(torch, np.ones(n + 1), n + 1, dt)
    r = (8,) if spec.restarted else ()
    refused = [("non-square plan", (rect.A,) + r + (None,)), ("shard plan", (shard,) + r + (None,)),
               ("misaligned %s" % spec.diagonal, (op.A,) + r + (d.data_ptr() + dt.itemsize,))]
    return refused, [(op.A,) + r + (d.data_ptr(),)], (op, d)


def _gmres_refusals(spec, torch, dt, stack):
    """... and restart 0 and 65; restart 1 and 64 are accepted."""
    refused, _, (op, d) = _square_refusals(spec, torch, dt, stack)
    return refused + [("restart 0", (op.A, 0, None)), ("restart 65", (op.A, 65, None))], [(op.A, restart, d.data_ptr()) for restart in (1, 64)], (op, d)


def _cg_refusals(spec, torch, dt, stack):
    """CG's own shard and its wide plan (the band 2048 x 4096), on Plan.from_csr; the misaligned and the aligned diagonal as for the other square solvers."""
    (n,), rp, ci, vt, b = _system(spec, spec.refuse_input, dt)
    plan = U.square_plan(n, rp, ci, vt, dt)
    shard = U.square_plan(n, rp, ci, vt, dt, tilerow_end=(n // 16) // 2)
    m, nc, brp, bci = G.band(2048, 40, ncols=4096)
    wide = api.Plan.from_csr(m, nc, len(bci), brp, bci, G.real_values(len(bci), dt), dtype=dt, deterministic=1, placement_tries=1)
    for p in (plan, shard, wide):
        stack.callback(p.close)
    d = U.vec(torch, np.ones(n + 1), n + 1, dt)
    return [("shard plan", (shard, None)), ("non-square plan", (wide, None)), ("misaligned dinv", (plan, d.data_ptr() + dt.itemsize))], [(plan, d.data_ptr())], (d,)


def _cgls_refusals(spec, torch, dt, stack):
    """A plan in the other one's place (the shapes no longer match), a shard plan in either place, a misaligned cinv.  Both plans exchanged is not among the refusals: the second
    half of tests/test_gpu_cgls.py::test_create_refuses_what_it_must."""
    (rows, cols), rp, ci, vt, b = _system(spec, spec.refuse_input, dt)
    op = stack.enter_context(U.rect_op(rows, cols, rp, ci, vt, dt))
    shard = api.Plan.from_csr(rows, cols, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, tilerow_end=(rows // 16) // 2)
    shardT = api.Plan.from_csr(rows, cols, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, transpose=True, tilerow_end=((cols + 15) // 16) // 2)
    stack.callback(shard.close); stack.callback(shardT.close)
    cinv = U.vec(torch, np.ones(cols + 1), cols + 1, dt)
    refused = [("A in the place of A^T", (op.A, op.A, None)), ("A^T in the place of A", (op.AT, op.AT, None)), ("shard of A", (shard, op.AT, None)),
               ("shard of A^T", (op.A, shardT, None)), ("misaligned cinv", (op.A, op.AT, cinv.data_ptr() + dt.itemsize))]
    return refused, [(op.A, op.AT, cinv.data_ptr())], (cinv,)


# ---- the table.  Every value stands where the solver's own test had it.
#   api, create          the class and the C entry point; its arguments are those of the class: the plans' handles, restart where there is one, the diagonal's address
#   operator, plans      what holds the plans (CG: a Plan.from_csr plan; the others: a SparseOperator) and the plans the solver takes from it
#   diagonal, host_diagonal, device_diagonal    the borrowed preconditioner: its name, numpy's, and the library's builder on the device
#   current              what makes x current before it is read: GMRES holds the iterate only after a close, so a flush
#   order                fixed order: the input, with or without the diagonal, iterate(count) or solve(maxiter), which of two separately created operators serves each run (CG:
#                        both plans alive together; the others: one after the other), the status
#   graph                capture: the input, x0, the count of begin + iterate(count), the counts of an iterate captured ALONE and replayed twice behind an eager begin (GMRES:
#                        behind the replay of begin + iterate(count))
#   refresh              value refresh: the two value sets of one pattern, the cap (None: 2 x the mirror's count, and the mirror's error is the yardstick), warm or cold, the reference
#   refusals             what create refuses and accepts
#   past, past_...       behind the end: the cases (None: the solver has no such test), their matrices, the early comparison (None: the ``_early`` of the solver's test file,
#                        which tests/test_gpu_solver_contract.py hands in), the cap of the solve and the reference
SOLVERS = {
    "cg": SimpleNamespace(
        M=cg_mirror, api=api.CG, create="tilespmv_cg_create", restarted=False, damped=False,
        operator=lambda dims, *a, **kw: U.square_plan(dims[0], *a, **kw), plans=lambda plan: (plan,),
        diagonal="dinv", host_diagonal=lambda dims, rp, ci, vt, dt: (dt.type(1) / cg_mirror.scipy_csr(dims[0], rp, ci, vt).diagonal().astype(dt)).astype(dt),
        device_diagonal=_diagonal_on_device(api.csr_diagonal_device), current=lambda s, xd, st: None,
        order=dict(input="fem12", diagonal=False, maxiter=500, operators=(0, 0, 1), together=True, status=api.CG_CONVERGED),
        # alone: 8 is CG's own (replayed twice: the iterates 8 and 16); the odd 3 is MINRES's, gained
        graph=dict(input="lap128", diagonal=False, x0=lambda nx, dt: np.zeros(nx, dtype=dt), count=8, alone=(8, 3)),
        refresh=dict(inputs=("lap128", "lap128_scaled"), maxiter=None, warm=False, reference=_spsolve(cg_mirror),
                     each="%s: %d iterations (mirror %d), error vs spsolve %.3g (mirror %.3g)", line=None),
        refuse_input="lap128", refusals=_cg_refusals,
        past=[dict(id="plain", diagonal=False), dict(id="jacobi")], past_inputs=_cg_past_inputs, past_early=_cg_early, past_solve=dict(maxiter=500),
        past_reference=_spsolve(cg_mirror)),
    "cgls": SimpleNamespace(
        M=cgls_mirror, api=api.CGLS, create="tilespmv_cgls_create", restarted=False, damped=True,
        operator=lambda dims, *a, **kw: U.rect_op(dims[0], dims[1], *a, **kw), plans=lambda op: (op.A, op.AT),
        diagonal="cinv", host_diagonal=lambda dims, rp, ci, vt, dt: cgls_mirror.column_cinv(cgls_mirror.scipy_csr(dims[0], dims[1], rp, ci, vt), dt),
        device_diagonal=_column_scaling_on_device, current=lambda s, xd, st: None,
        order=dict(input="tall", diagonal=True, damp=0.5, count=20, operators=(0, 1), status=None),      # (with damping and cinv, so that every sum takes part)
        graph=dict(input="tall", diagonal=False, damp=0.5, x0=lambda nx, dt: (0.01 * cgls_mirror.rhs(nx)).astype(dt), count=8, alone=(3,)),      # (alone: gained)
        refresh=dict(inputs=("tall", "tall_scaled"), maxiter=200, warm=True,
                     reference=lambda dims, rp, ci, vt, b: cgls_mirror.lsqr_x(cgls_mirror.scipy_csr(dims[0], dims[1], rp, ci, vt), b, scale_columns=True),
                     line="%(dt)s: refreshed %(refreshed)d iterations, fresh %(fresh)d; error vs lsqr %(error).3g"),
        refuse_input="tall", refusals=_cgls_refusals,
        past=[dict(id="5003x1237", shape=(5003, 1237)), dict(id="1237x5003", shape=(1237, 5003))], past_inputs=_cgls_past_inputs, past_early=_cgls_early,
        past_solve=dict(maxiter=500, damp=0.5),
        past_reference=lambda dims, rp, ci, vt, b: cgls_mirror.lsqr_x(cgls_mirror.scipy_csr(dims[0], dims[1], rp, ci, vt), b, 0.5)),
    "bicgstab": SimpleNamespace(
        M=bicgstab_mirror, api=api.BiCGStab, create="tilespmv_bicgstab_create", restarted=False, damped=False,
        operator=lambda dims, *a, **kw: U.square_op(dims[0], *a, **kw), plans=lambda op: (op.A,),
        diagonal="dinv", host_diagonal=lambda dims, rp, ci, vt, dt: bicgstab_mirror.inverse_diagonal(dims[0], rp, ci, vt, dt),
        device_diagonal=_diagonal_on_device(api.csr_diagonal_device), current=lambda s, xd, st: None,
        order=dict(input="convdiff67_scaled", diagonal=True, count=20, operators=(0, 1), status=api.CG_RUNNING),
        graph=dict(input="convdiff67", diagonal=True, x0=_reversed_start(bicgstab_mirror), count=8, alone=(3,)),      # (alone: gained)
        refresh=dict(inputs=("convdiff67", "convdiff67_scaled"), maxiter=500, warm=True, reference=_spsolve(bicgstab_mirror),
                     line="%(dt)s: refreshed %(refreshed)d iterations, fresh %(fresh)d; error vs spsolve %(error).3g"),
        refuse_input="convdiff67", refusals=_square_refusals,
        past=[dict(id="5003")], past_inputs=_random_5003, past_early=None, past_solve=dict(maxiter=200), past_reference=_spsolve(bicgstab_mirror)),
    "minres": SimpleNamespace(
        M=minres_mirror, api=api.MINRES, create="tilespmv_minres_create", restarted=False, damped=False,
        operator=lambda dims, *a, **kw: U.square_op(dims[0], *a, **kw), plans=lambda op: (op.A,),
        diagonal="minv", host_diagonal=lambda dims, rp, ci, vt, dt: minres_mirror.inverse_abs_diagonal(dims[0], rp, ci, vt, dt),
        device_diagonal=_diagonal_on_device(api.csr_abs_diagonal_device), current=lambda s, xd, st: None,
        order=dict(input="saddlec47_scaled", diagonal=True, count=20, operators=(0, 1), status=api.CG_RUNNING),
        # alone: an odd count, so the second replay starts with the roles of the two history buffers exchanged: a history rotated by pointers on the host would be frozen into the
        # graph and fail here
        graph=dict(input="saddlec47_scaled", diagonal=True, x0=_reversed_start(minres_mirror), count=8, alone=(3,)),
        refresh=dict(inputs=("saddlec47", "saddlec47_scaled"), maxiter=1000, warm=True, reference=_spsolve(minres_mirror),
                     line="%(dt)s: first %(first)d iterations, refreshed %(refreshed)d, fresh %(fresh)d; error vs spsolve %(error).3g"),
        refuse_input="saddle47", refusals=_square_refusals,
        past=None),      # MINRES never had a past-the-end test of its own: its _early holds the sentinels in every early test (tests/test_gpu_minres.py).  A gap, kept as it was
    "gmres": SimpleNamespace(
        M=gmres_mirror, api=api.GMRES, create="tilespmv_gmres_create", restarted=True, damped=False,
        operator=lambda dims, *a, **kw: U.square_op(dims[0], *a, **kw), plans=lambda op: (op.A,),
        diagonal="dinv", host_diagonal=lambda dims, rp, ci, vt, dt: gmres_mirror.inverse_diagonal(dims[0], rp, ci, vt, dt),
        device_diagonal=_diagonal_on_device(api.csr_diagonal_device), current=lambda s, xd, st: s.flush(xd.data_ptr(), st),
        order=dict(input="convdiff67_colscaled", diagonal=True, restart=8, count=2 * 8 + 3, operators=(0, 1), status=api.CG_RUNNING),
        # the host keeps the cycle position, so a captured iterate replays correctly only when captured at a cycle boundary with a count that is a multiple of
        # restart: no odd count here.  count = restart; alone = restart, replayed twice behind each replay of begin + iterate(restart): the iterates 2 x restart and 3 x restart
        graph=dict(input="convdiff67", diagonal=True, restart=6, x0=_reversed_start(gmres_mirror), count=6, alone=(6,), behind_whole=True),
        refresh=dict(inputs=("convdiff67", "convdiff67_colscaled"), restart=16, maxiter=800, warm=True, reference=_spsolve(gmres_mirror),
                     line="%(dt)s: refreshed %(refreshed)d iterations, fresh %(fresh)d; error vs spsolve %(error).3g"),
        refuse_input="convdiff67", refusals=_gmres_refusals,
        past=[dict(id="5003")], past_inputs=_random_5003, past_early=None, past_solve=dict(maxiter=200, restart=8), past_reference=_spsolve(gmres_mirror)),
}


def _system(spec, name, dt):
    """A named input of the solver's mirror: ((n,) or (rows, cols), rp, ci, values, b)."""
    *dims, rp, ci, v = spec.M.problem(name)
    return tuple(dims), rp, ci, v.astype(dt), spec.M.rhs(dims[0]).astype(dt)


def _solver(spec, op, d, c):
    """The solver on an operator's plans with the diagonal d (a device vector or None) and the restart of a promise's entry c."""
    return spec.api(*spec.plans(op), *((c["restart"],) if spec.restarted else ()), None if d is None else d.data_ptr())


def _begin(spec, s, c, bd, xd, st):
    s.begin(bd.data_ptr(), xd.data_ptr(), *((c.get("damp", 0.0),) if spec.damped else ()), st)


def _solve(spec, s, c, bd, xd, st, dt, maxiter):
    return s.solve(bd.data_ptr(), xd.data_ptr(), rtol=spec.M.RTOL[dt], maxiter=maxiter, stream=st, **({"damp": c["damp"]} if "damp" in c else {}))


# ---- the promises
def sums_have_a_fixed_order(torch, name, dtype):
    """Solvers on two separately created deterministic operators of one matrix (CG: two solves on one plan and one on a second): bit-identical x and state, after iterate(count)
    or after a solve."""
    dt, spec = np.dtype(dtype), SOLVERS[name]
    c, st = spec.order, U.stream(torch)
    dims, rp, ci, vt, b = _system(spec, c["input"], dt)
    nb, nx = dims[0], dims[-1]
    d = U.vec(torch, spec.host_diagonal(dims, rp, ci, vt, dt), nx, dt) if c["diagonal"] else None
    bd = U.vec(torch, b, nb, dt)
    together = [spec.operator(dims, rp, ci, vt, dt) for _ in range(2)] if c.get("together") else None
    results = []
    for k in c["operators"]:
        op = together[k] if together else spec.operator(dims, rp, ci, vt, dt)
        xd = U.vec(torch, None, nx, dt)
        with _solver(spec, op, d, c) as s:
            if "maxiter" in c:
                state = _solve(spec, s, c, bd, xd, st, dt, c["maxiter"])
            else:
                _begin(spec, s, c, bd, xd, st)
                s.iterate(xd.data_ptr(), c["count"], st)
                spec.current(s, xd, st)
                state = s.state(st)
                assert state["iterations"] == c["count"]
        assert c["status"] is None or state["status"] == c["status"]
        results.append((U.host(xd, nx), state))
        U.intact((xd, nx))
        if not together:
            op.close()
    for op in together or ():
        op.close()
    for x, state in results[1:]:
        assert np.array_equal(x, results[0][0]) and state == results[0][1]
    assert results[0][0].any()
    U.intact((bd, nb), *(((d, nx),) if d is not None else ()))


def begin_and_iterate_are_capturable_into_a_hip_graph(torch, name, dtype):
    """Captured with torch's graph API on a side stream (one linear chain, as tests/test_gpu_parity.py captures the product).
    (a) begin + iterate(count), replayed twice from the same x0: each replay equals the eager run bit for bit, x and state.
    (b) begin eager, then a captured iterate(k) ALONE replayed twice: after each replay x and the state equal an eager begin + iterate of as many iterations, run as k + k and as
    one iterate(2 k).  The table says which k: an odd one wherever the solver keeps no host-side position (so the second replay starts at the other parity).  GMRES: the two replays
    follow each replay of (a) instead, and equal eager iterate(count) + iterate(2 k)."""
    dt, spec = np.dtype(dtype), SOLVERS[name]
    c = spec.graph
    dims, rp, ci, vt, b = _system(spec, c["input"], dt)
    nb, nx = dims[0], dims[-1]
    x0 = c["x0"](nx, dt)
    count, behind_whole = c["count"], c.get("behind_whole", False)
    op = spec.operator(dims, rp, ci, vt, dt)
    bd, xd = U.vec(torch, b, nb, dt), U.vec(torch, x0, nx, dt)
    d = U.vec(torch, spec.host_diagonal(dims, rp, ci, vt, dt), nx, dt) if c["diagonal"] else None
    s = _solver(spec, op, d, c)
    want = {}      # iterations -> (x, state) of the eager runs

    def begin(st):
        xd[:nx].copy_(torch.from_numpy(x0))
        _begin(spec, s, c, bd, xd, st)

    def eager(steps, st):
        begin(st)
        done = 0
        for k in steps:
            s.iterate(xd.data_ptr(), k, st); done += k
            got = (U.host(xd, nx), s.state(st))
            assert done not in want or (np.array_equal(got[0], want[done][0]) and got[1] == want[done][1])      # (however the iterations were batched)
            want[done] = got

    def equals_the_eager_run(done):
        state = s.state(U.stream(torch))
        assert np.array_equal(U.host(xd, nx), want[done][0]) and state == want[done][1]
        assert state["iterations"] == done and state["status"] == api.CG_RUNNING

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    whole, alone = torch.cuda.CUDAGraph(), {k: torch.cuda.CUDAGraph() for k in c["alone"]}
    with torch.cuda.stream(side):
        st = side.cuda_stream
        eager([count], st)                                        # (uncaptured: the comparisons, and the warm-up)
        for k in alone:
            lead = [count] if behind_whole else []
            eager(lead + [k, k], st)
            eager(lead + [2 * k] + ([count - 2 * k] if not behind_whole and 2 * k < count else []), st)      # (MINRES's own: iterate(6), then 2 more to the 8 of (a))
        xd[:nx].copy_(torch.from_numpy(x0))
        side.synchronize()
        with torch.cuda.graph(whole, stream=side):
            _begin(spec, s, c, bd, xd, st)
            s.iterate(xd.data_ptr(), count, st)
        for k, graph in alone.items():                            # (GMRES: the host's cycle position is 0 here, a cycle boundary)
            with torch.cuda.graph(graph, stream=side):
                s.iterate(xd.data_ptr(), k, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(U.host(xd, nx), x0)                     # (captured, not run)
    for _ in range(2):                                            # (a)
        xd[:nx].copy_(torch.from_numpy(x0))
        torch.cuda.synchronize()
        whole.replay(); torch.cuda.synchronize()
        equals_the_eager_run(count)
        for k, graph in alone.items() if behind_whole else ():    # (b) of GMRES
            for done in (count + k, count + 2 * k):
                graph.replay(); torch.cuda.synchronize()
                equals_the_eager_run(done)
    for k, graph in () if behind_whole else alone.items():        # (b)
        begin(U.stream(torch))
        torch.cuda.synchronize()
        for done in (k, 2 * k):
            graph.replay(); torch.cuda.synchronize()
            equals_the_eager_run(done)
    iterates = [x0] + [want[done][0] for done in sorted(want)]
    assert all(not np.array_equal(p, q) for i, p in enumerate(iterates) for q in iterates[:i])
    del whole, alone, graph
    s.close()
    op.close()
    U.intact((bd, nb), (xd, nx), *(((d, nx),) if d is not None else ()))


def value_refresh(torch, name, dtype):
    """an operator with a value map solves with the first value set; update_values to the second (the same pattern), the diagonal recomputed on the
    device into the SAME array, then a second solve on the untouched solver, warm-started from the first solution (CG: from zero).  The result equals, bit for bit on these
    deterministic plans, that of an operator built fresh from the new values and started from the same x, and it is right: within 100 x rtol of the reference (CG: both solves
    within 2 x the mirror's count and 10 x the mirror's own error against spsolve)."""
    dt, spec = np.dtype(dtype), SOLVERS[name]
    c, st, rtol = spec.refresh, U.stream(torch), SOLVERS[name].M.RTOL[dt]
    dims, rp, ci, v1, b = _system(spec, c["inputs"][0], dt)
    v2 = _system(spec, c["inputs"][1], dt)[3]
    nb, nx = dims[0], dims[-1]
    mirrored = []      # per value set (the mirror's count, the reference, the mirror's error) where the mirror is the yardstick
    if c["maxiter"] is None:
        for vt in (v1, v2):
            xm, itm, stm, relm = spec.M.Mirror(spec.M.scipy_csr(*dims, rp, ci, vt), dt, spec.host_diagonal(dims, rp, ci, vt, dt)).solve(b, rtol=rtol, maxiter=5000, check_every=1)
            assert stm == spec.M.CONVERGED
            xs = c["reference"](dims, rp, ci, vt, b)
            mirrored.append((itm, xs, U.relerr(xm, xs)))

    def solve(s, x, k):
        state = _solve(spec, s, c, bd, x, st, dt, c["maxiter"] or 2 * mirrored[k][0])
        assert state["status"] == api.CG_CONVERGED
        return state

    def judged_by_the_mirror(state, k):
        if mirrored:
            itm, xs, errm = mirrored[k]
            err = U.relerr(U.host(xd, nx), xs)
            print(c["each"] % (dt, state["iterations"], itm, err, errm))
            assert err <= 10 * errm

    rpd, cid, v1d = U.device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    fill = spec.device_diagonal(torch, dims, rpd, cid, dt)
    d, bd, xd = U.vec(torch, None, nx, dt), U.vec(torch, b, nb, dt), U.vec(torch, None, nx, dt)
    op = spec.operator(dims, rp, ci, v1, dt, value_map=True)
    fill(v1d, d, st)
    with _solver(spec, op, d, c) as s:
        s1 = solve(s, xd, 0)
        judged_by_the_mirror(s1, 0)
        x1 = U.host(xd, nx)
        op.update_values(v2d.data_ptr(), st)
        fill(v2d, d, st)
        if not c["warm"]:
            xd[:nx].zero_()
        s2 = solve(s, xd, 1)      # (warm: x holds the first solution)
        judged_by_the_mirror(s2, 1)
        x2 = U.host(xd, nx)
    op.close()
    fresh = spec.operator(dims, rp, ci, v2, dt, value_map=True)
    xf = U.vec(torch, x1 if c["warm"] else None, nx, dt)
    with _solver(spec, fresh, d, c) as s:
        sf = solve(s, xf, 1)
    fresh.close()
    assert s2 == sf and np.array_equal(x2, U.host(xf, nx))
    if not mirrored:
        error = U.relerr(x2, c["reference"](dims, rp, ci, v2, b))
        print(c["line"] % dict(dt=dt, first=s1["iterations"], refreshed=s2["iterations"], fresh=sf["iterations"], error=error))
        assert error <= 100 * rtol
    U.intact((d, nx), (bd, nb), (xd, nx), (xf, nx))


def create_refuses_what_it_must(torch, name, dtype):
    """What the solver's row of the table lists as refused: hipErrorInvalidValue and no handle from the C entry point, ValueError from the class.  What it lists as accepted (an
    aligned diagonal; GMRES: restart 1 and 64) gives a handle."""
    dt, spec = np.dtype(dtype), SOLVERS[name]
    lib = _lib.load(dt)
    with contextlib.ExitStack() as stack:
        refused, accepted, _alive = spec.refusals(spec, torch, dt, stack)      # (_alive: the device vectors behind the addresses, held to the end)
        for label, args in refused:
            h = C.c_void_p(1)
            rc = getattr(lib, spec.create)(C.byref(h), *[a.h if isinstance(a, api.Plan) else a for a in args[:-1]], C.c_void_p(args[-1]))
            print("%s %s: rc %d, handle %s" % (dt, label, rc, h.value))
            assert rc == api.HIP_ERROR_INVALID_VALUE and not h, label
            with pytest.raises(ValueError):
                spec.api(*args)
        for args in accepted:
            with spec.api(*args) as s:
                assert s.h


def nothing_is_touched_past_the_end(torch, name, dtype, early=None, **case):
    """b, x and the diagonal with 16 sentinel elements behind them, on row (and column) counts that leave a partial lane vector at the end: the solver's early iterations equal the
    mirror's, the sentinels survive a solve with the diagonal, b and the diagonal are unchanged, and the solve is right: within 100 x rtol of the reference.  ``early`` stands in
    where the table has no early comparison.  CG and CGLS solve on the handle that ran the early iterations; the ``_early`` of BiCGStab and GMRES closes its own, so theirs is a second."""
    dt, spec = np.dtype(dtype), SOLVERS[name]
    c, st = spec.past_solve, U.stream(torch)
    for label, dims, rp, ci, vt in spec.past_inputs(case, dt):
        nb, nx = dims[0], dims[-1]
        A = spec.M.scipy_csr(*dims, rp, ci, vt)
        b = spec.M.rhs(nb).astype(dt)
        diagonal = spec.host_diagonal(dims, rp, ci, vt, dt) if case.get("diagonal", True) else None
        op = spec.operator(dims, rp, ci, vt, dt)
        bd, xd, dd, s = (spec.past_early or early)(torch, dt, op, A, b, diagonal, dims, label)
        xd[:nx].zero_()
        with s or _solver(spec, op, dd, c) as s:
            state = _solve(spec, s, c, bd, xd, st, dt, c["maxiter"])
        assert state["status"] == api.CG_CONVERGED
        assert U.relerr(U.host(xd, nx), spec.past_reference(dims, rp, ci, vt, b)) <= 100 * spec.M.RTOL[dt]
        U.intact((bd, nb), (xd, nx), *(((dd, nx),) if dd is not None else ()))
        assert np.array_equal(U.host(bd, nb), b) and (dd is None or np.array_equal(U.host(dd, nx), diagonal))
        op.close()
