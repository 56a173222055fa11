"""The restarted GMRES solver in the library on the GPU (tilespmv_gmres_*; include/tilespmv.h) against its numpy mirror (tests/gmres_mirror.py, itself checked by
tests/test_gmres_cpu.py) and scipy's direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless a test says otherwise.

Iterate for iterate the GPU is compared with the mirror after a few inner iterations and a flush (x is current only after a close), to 100 x the per-product tolerance: the bound
of the other solvers' early iterations.  GMRES minimises the residual over a Krylov space, so the iterate after a close depends little on how the basis was rounded; the two ends of
the restart range are held to the same bound after two cycles.  Further on, a solve is judged by its end: status, the recomputed residual, the error against spsolve.

What this solver promises like every other one is written once in tests/solver_contract.py, whose table has this solver's inputs and counts: graph capture and nothing
touched past the end run from tests/test_gpu_solver_contract.py; the fixed order of the sums, value refresh and the refusals of create are the tests of those names here."""
import ctypes as C

import numpy as np
import pytest

import block_jacobi_mirror as BJ
import gmres_mirror as M
import gpu_solver_util as U
import solver_contract as K
import solver_sizes as SS
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api
from tilespmv_amd.operator import SparseOperator, gmres as torch_gmres

pytestmark = pytest.mark.gpu

RESTART = 16
_CACHE = {}


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _true_rel(A, b, x):
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(b64 - A.astype(np.float64) @ x.astype(np.float64)) / np.linalg.norm(b64))


def _residual_rounding(A, b, x, dt):
    """How far apart the norms of b - A x formed in the value type (the library) and in float64 (_true_rel) may lie, relative to |b|: (entries per row + 2) (eps + eps64)
    | |A| |x| + |b| | / |b| — the standard bound of a rounded residual, once for each of the two (the sums behind the norms are double)."""
    A64, x64, b64 = abs(A.astype(np.float64)), abs(x.astype(np.float64)), abs(b.astype(np.float64))
    per_row = int(np.diff(A.indptr).max())
    return float((per_row + 2) * (np.finfo(dt).eps + np.finfo(np.float64).eps) * np.linalg.norm(A64 @ x64 + b64) / np.linalg.norm(b64))


def _solved(name, dtype):
    """The mirror's solve (restart 16; Jacobi on the column-scaled input) of a named input and the direct solution, computed once per value type and left unchanged:
    (xs, mirror iterations, mirror error, the mirror's true relative residual)."""
    dt = np.dtype(dtype)
    if (name, dt) not in _CACHE:
        n, rp, ci, vt, b = _system(name, dt)
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = M.inverse_diagonal(n, rp, ci, vt, dt) if name.endswith("_colscaled") else None
        xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = M.Mirror(A, dt, RESTART, dinv).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[(name, dt)] = (xs, itm, U.relerr(xm, xs), _true_rel(A, b, xm))
    return _CACHE[(name, dt)]


def _early(torch, dt, mirror, b, make_solver, n, label, steps=(3, 2)):
    """begin; rr after the first of ``steps`` inner iterations, before any flush; after all of them and a flush x and the state — against ``mirror``.  Bound: 100 x the per-product
    tolerance (the bound of tests/test_gpu_bicgstab.py: another summation order over a few iterations); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    mirror.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    st = U.stream(torch)
    with make_solver() as gm:
        gm.begin(bd.data_ptr(), xd.data_ptr(), st)
        s0 = gm.state(st)
        print("%s %s begin: rr %.3g bb %.3g" % (label, dt, U.dist(s0["rr"], mirror.rr), U.dist(s0["bb"], mirror.bb)))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(U.dist(s0["rr"], mirror.rr), U.dist(s0["bb"], mirror.bb)) <= bound
        done = 0
        for step in steps:
            gm.iterate(xd.data_ptr(), step, st); mirror.iterate(step); done += step
            s = gm.state(st)
            drr = U.dist(s["rr"], mirror.rr)
            print("%s %s after %d iterations: rr %.3g (bound %.3g)" % (label, dt, done, drr, bound))
            assert s["iterations"] == done == mirror.iterations and s["status"] == api.CG_RUNNING == mirror.status()
            assert drr <= bound
        gm.flush(xd.data_ptr(), st); mirror.flush()
        s = gm.state(st)
        dx, drr = U.relerr(U.host(xd, n), mirror.x.astype(np.float64)), U.dist(s["rr"], mirror.rr)
        print("%s %s after the flush: |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)" % (label, dt, dx, drr, bound))
        assert s["iterations"] == done and s["status"] == api.CG_RUNNING == mirror.status()
        assert dx <= bound and drr <= bound
    U.intact((xd, n))
    assert np.array_equal(U.host(bd, n), b)
    return bd, xd


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    """restart 8: rr after iterate(3), rr after two more, then x and rr after a flush."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.Mirror(M.scipy_csr(n, rp, ci, vt), dt, 8), b, lambda: api.GMRES(op.A, 8), n, "convdiff67")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kw", [("convdiff67", {}), ("convdom67", {}), ("shiftskew67", {}), ("convdom67", dict(deterministic=-1, placement_tries=-1))])
def test_solves(torch_cuda, name, kw, dtype):
    """tilespmv_gmres_solve with restart 16 and maxiter = 2 x the mirror's count: CONVERGED, an error against spsolve within 10 x the mirror's own, and a reported sqrt(rr / bb)
    that is the recomputed residual of the returned x: it equals the one recomputed on the host up to the rounding of a residual formed in the value type, and it is at most
    max(RTOL, 2 x the mirror's true residual).  The last case is the builder's default (timed) plans, whatever form they pick."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    A = M.scipy_csr(n, rp, ci, vt)
    xs, itm, errm, truem = _solved(name, dt)
    with U.square_op(n, rp, ci, vt, dt, **kw) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.GMRES(op.A, RESTART) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=U.stream(torch))
        x = U.host(xd, n)
    err, true, slack = U.relerr(x, xs), _true_rel(A, b, x), _residual_rounding(A, b, x, dt)
    print("%s %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.4g, recomputed on the host %.4g (rounding of a residual %.3g; mirror's true %.4g), error %.3g (mirror %.3g)"
          % (name, dt, kw, s["iterations"], itm, s["relative_residual"], true, slack, truem, err, errm))
    assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    assert abs(s["relative_residual"] - true) <= slack
    assert s["relative_residual"] <= max(M.RTOL[dt], 2 * truem)
    U.intact((xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi(torch_cuda, dtype):
    """convdiff67_colscaled: dinv from tilespmv_csr_diagonal_device(invert) equals numpy's; right-preconditioned GMRES converges within 2 x the mirror's count to an error within
    10 x the mirror's; the plain solver on the same plan is still running after 4 x the preconditioned count."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67_colscaled", dt)
    xs, itm, errm, truem = _solved("convdiff67_colscaled", dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    dinv = U.vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    assert np.array_equal(U.host(dinv, n), M.inverse_diagonal(n, rp, ci, vt, dt))
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.GMRES(op.A, RESTART, dinv.data_ptr()) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s: Jacobi GMRES %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm and s["relative_residual"] <= max(M.RTOL[dt], 2 * truem)
        assert err <= 10 * errm
        xd[:n].zero_()
        with api.GMRES(op.A, RESTART) as gm:
            sp = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=4 * s["iterations"], stream=stream)
        print("%s: plain GMRES on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, sp["iterations"], sp["status_name"], sp["relative_residual"]))
        assert sp["status"] == api.CG_MAXITER and sp["iterations"] == 4 * s["iterations"] and sp["relative_residual"] >= 100 * M.RTOL[dt]
    U.intact((dinv, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_jacobi(torch_cuda, dtype):
    """tilespmv_gmres_create_block on the nonsymmetric FEM input of tests/test_gpu_block_jacobi.py: early iterations equal the mirror with the block planes; bs = 3 converges
    (error within 10 x the mirror's) where point Jacobi at the same number of iterations has not; bs = 1 is point Jacobi to the early-iteration bound."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, v = BJ.problem("femblk10_ns")
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    A = M.scipy_csr(n, rp, ci, vt)
    P, _ = BJ.update(n, rp, ci, vt, 3, dt)
    xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
    xm, itm, stm, relm = M.BlockMirror(A, dt, RESTART, P).solve(b, rtol=M.RTOL[dt], maxiter=1000, check_every=1)
    assert stm == M.CONVERGED
    errm = U.relerr(xm, xs)
    csr = U.device_csr(torch, rp, ci, vt)
    bound = 100 * PRODUCT_TOL[dt]
    with U.square_op(n, rp, ci, vt, dt) as op, api.BlockJacobi(n, 3, dt) as bj3, api.BlockJacobi(n, 1, dt) as bj1:
        bj3.update(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), stream)
        bj1.update(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), stream)
        bd, xd = _early(torch, dt, M.BlockMirror(A, dt, 8, P), b, lambda: api.GMRES(op.A, 8, block=bj3), n, "femblk10_ns bs=3")
        xd[:n].zero_()
        with api.GMRES(op.A, RESTART, block=bj3) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s: block Jacobi GMRES %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        dinv = U.vec(torch, None, n, dt)
        api.csr_diagonal_device(n, csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
        xd[:n].zero_()
        with api.GMRES(op.A, RESTART, dinv.data_ptr()) as gm:
            sp = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=s["iterations"], check_every=8, stream=stream)
        print("%s: point Jacobi on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, sp["iterations"], sp["status_name"], sp["relative_residual"]))
        assert sp["status"] == api.CG_MAXITER and sp["iterations"] == s["iterations"]
        # bs = 1 against d_dinv: five iterations and a flush
        got = []
        for make in (lambda: api.GMRES(op.A, 8, block=bj1), lambda: api.GMRES(op.A, 8, dinv.data_ptr())):
            xd[:n].zero_()
            with make() as gm:
                gm.begin(bd.data_ptr(), xd.data_ptr(), stream)
                gm.iterate(xd.data_ptr(), 5, stream)
                gm.flush(xd.data_ptr(), stream)
                got.append((U.host(xd, n), gm.state(stream)))
        (x1, s1), (xp, spj) = got
        print("%s: bs = 1 against point Jacobi: x %.3g, rr %.3g (bound %.3g)" % (dt, U.relerr(x1, xp.astype(np.float64)), U.dist(s1["rr"], spj["rr"]), bound))
        assert xp.any() and U.relerr(x1, xp.astype(np.float64)) <= bound and U.dist(s1["rr"], spj["rr"]) <= bound and s1["iterations"] == spj["iterations"] == 5
        with pytest.raises(ValueError):
            api.GMRES(op.A, 8, dinv.data_ptr(), block=bj3)
        with api.BlockJacobi(n + 1, 3, dt) as other:
            h = C.c_void_p(1)
            assert _lib.load(dt).tilespmv_gmres_create_block(C.byref(h), op.A.h, 8, other.h) == api.HIP_ERROR_INVALID_VALUE and not h


@pytest.mark.parametrize("dtype", DTYPES)
def test_restart_boundaries(torch_cuda, dtype):
    """restart = 5: iterate(5) + iterate(5), iterate(10) and ten iterate(1) are the same bits on a deterministic plan.  restart = 1 and restart = 64 (the last group of the basis
    loop, every slot of the partial arrays) run two cycles and more and agree with the mirror to the early bound."""
    torch, dt = torch_cuda, np.dtype(dtype)
    st = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    A = M.scipy_csr(n, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        got = []
        for batches in ((5, 5), (10,), (1,) * 10):
            xd[:n].zero_()
            with api.GMRES(op.A, 5) as gm:
                gm.begin(bd.data_ptr(), xd.data_ptr(), st)
                for c in batches:
                    gm.iterate(xd.data_ptr(), c, st)
                got.append((U.host(xd, n), gm.state(st)))
        m = M.Mirror(A, dt, 5); m.begin(b); m.iterate(10)
        for x, s in got:
            assert s["iterations"] == 10 and np.array_equal(x, got[0][0]) and s["rr"] == got[0][1]["rr"] and x.any()
        assert U.relerr(got[0][0], m.x.astype(np.float64)) <= 100 * PRODUCT_TOL[dt]      # (after two closes x is current)
        for restart, count in ((1, 3), (64, 2 * 64 + 3)):
            _early(torch, dt, M.Mirror(A, dt, restart), b, lambda: api.GMRES(op.A, restart), n, "restart %d" % restart, steps=(count - 1, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_transposed_plan_solves_the_transposed_system(torch_cuda, dtype):
    """api.GMRES(op.AT): five iterations and a flush equal the mirror of A^T."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.Mirror(M.scipy_csr(n, rp, ci, vt).T.tocsr(), dt, 8), b, lambda: api.GMRES(op.AT, 8), n, "convdiff67^T")


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """b = 0; rr = 0 exactly at begin (skew from its exact solution) stops every change; the lucky termination (A = 2 I, b = 4 e_k) closes the cycle early and gives 2 e_k bit for
    bit; gamma = 0 (nilpotent) raises the breakdown flag and leaves x alone; maxiter cuts the last block and solve's flush makes x and rr current."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    # b = 0
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        zero, xd = U.vec(torch, None, n, dt), U.vec(torch, b, n, dt)
        with api.GMRES(op.A, 8) as gm:
            s = gm.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and s["rr"] == 0.0 and not U.host(xd, n).any()
            gm.begin(zero.data_ptr(), xd.data_ptr(), stream)
            gm.iterate(xd.data_ptr(), 16, stream)
            gm.flush(xd.data_ptr(), stream)
            s = gm.state(stream)
            x = U.host(xd, n)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and not x.any()
        # maxiter cuts the last block; the flush of solve: x is the iterate of iteration 13, rr its recomputed residual
        bd = U.vec(torch, b, n, dt)
        A = M.scipy_csr(n, rp, ci, vt)
        xm, itm, stm, relm = M.Mirror(A, dt, 8).solve(b, rtol=M.RTOL[dt], maxiter=13, check_every=8)
        for check_every in (8, 0):
            xd[:n].zero_()
            with api.GMRES(op.A, 8) as gm:
                s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=13, check_every=check_every, stream=stream)
            x = U.host(xd, n)
            assert s["iterations"] == 13 and s["status"] == api.CG_MAXITER == stm
            assert U.relerr(x, xm.astype(np.float64)) <= 100 * PRODUCT_TOL[dt] and U.dist(s["relative_residual"], relm) <= 100 * PRODUCT_TOL[dt]
            assert abs(s["relative_residual"] - _true_rel(A, b, x)) <= _residual_rounding(A, b, x, dt)
    # skew from x0 = -A b, its exact integer solution
    n, rp, ci, v = M.problem("skew")
    b = M.skew_rhs(n)
    x0 = (-(M.scipy_csr(n, rp, ci, v) @ b)).astype(dt)
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        with api.GMRES(op.A, 8) as gm:
            gm.begin(bd.data_ptr(), xd.data_ptr(), stream)
            s = gm.state(stream)
            assert s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and s["bb"] == float(b @ b)
            gm.iterate(xd.data_ptr(), 16, stream)
            s = gm.state(stream)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and np.array_equal(U.host(xd, n), x0)
            # ... and from zeros GMRES needs two iterations where BiCGStab breaks down
            xd[:n].zero_()
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=1, stream=stream)
            assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 and U.relerr(U.host(xd, n), x0.astype(np.float64)) <= 100 * M.RTOL[dt]
    # A = 2 I, b = 4 e_k: everything is exact
    n, rp, ci, v = M.problem("2I")
    e = np.zeros(n); e[1234] = 1.0
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, 4 * e, n, dt), U.vec(torch, None, n, dt)
        with api.GMRES(op.A, 8) as gm:
            gm.begin(bd.data_ptr(), xd.data_ptr(), stream)
            gm.iterate(xd.data_ptr(), 1, stream)
            s = gm.state(stream)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()      # (x waits for the close)
            gm.iterate(xd.data_ptr(), 5, stream)
            gm.flush(xd.data_ptr(), stream)
            s = gm.state(stream)
            assert s["iterations"] == 6 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), (2 * e).astype(dt))
    # nilpotent: A V_0 = 0 exactly
    n, rp, ci, v = M.problem("nilpotent")
    b, x0 = M.nilpotent_rhs(n).astype(dt), np.zeros(n, dtype=dt)
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        with api.GMRES(op.A, 8) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(U.host(xd, n), x0) and s["rr"] == float(b.astype(np.float64) @ b.astype(np.float64))
            gm.iterate(xd.data_ptr(), 9, stream)      # ... past a cycle's end: the close and the open leave x alone
            s = gm.state(stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 17 and np.array_equal(U.host(xd, n), x0)


TIER_512_ROWS = (32 << 20) // 8 + 3      # an fp64 vector of 32 MiB and a scalar tail: the first size with 512 workgroups


@pytest.mark.parametrize("rows,dtype", [(None, np.float64), (None, np.float32), (TIER_512_ROWS, np.float64)])
def test_past_the_workgroup_cap(torch_cuda, rows, dtype):
    """solver_sizes.capped_n rows (1 052 249 / 2 104 499): the 256 workgroups of these kernels walk their share in several sweeps, the last trip is a partial one and the scalar
    tail is the longest.  4 194 307 rows in fp64: the first size at which the kernels run with 512 workgroups and partials per sum (the arrays of partials are sized by that
    count; in fp32 the same code would need 8.4 M rows, and 1024 workgroups 16.8 M: scripts/gmres_time.py compares those with the torch loop).  On the nonsymmetric tridiagonal
    (-1.5, 3, -0.5) with a diagonal preconditioner that varies from row to row: five iterations and a flush equal the mirror's."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, v = SS.nonsymmetric_tridiagonal(rows or SS.capped_n(dt))
    vt, dinv = v.astype(dt), SS.diagonal_preconditioner(n).astype(dt)
    b = SS.exact_rhs(n).astype(dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        dd = U.vec(torch, dinv, n, dt)
        _early(torch, dt, M.Mirror(M.scipy_csr(n, rp, ci, vt), dt, 4, dinv), b, lambda: api.GMRES(op.A, 4, dd.data_ptr()), n, "%d rows" % n)
        U.intact((dd, n))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SS.TINY_N)
def test_tiny_systems(torch_cuda, n, dtype):
    """1, 2, 3 and 5 rows (no full lane vector, or one and a tail; a Krylov space that is exhausted inside the first cycle): the solve converges to the dense solution and touches
    nothing behind the vectors."""
    torch, dt = torch_cuda, np.dtype(dtype)
    _, rp, ci, v = SS.tridiagonal(n, -1.5, 3.0, -0.5) if n > 1 else SS.two_identity(1)
    vt, b = v.astype(dt), (np.arange(n) + 1.0).astype(dt)
    xs = np.linalg.solve(M.scipy_csr(n, rp, ci, vt).toarray().astype(np.float64), b.astype(np.float64))
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.GMRES(op.A, 8) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=16, check_every=1, stream=U.stream(torch))
        print("%d rows %s: %s" % (n, dt, s))
        assert s["status"] == api.CG_CONVERGED and s["iterations"] <= n and s["relative_residual"] <= M.RTOL[dt]
        assert U.relerr(U.host(xd, n), xs) <= 100 * M.RTOL[dt]
        U.intact((xd, n), (bd, n))


# ---- the promises shared with the other solvers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """tests/solver_contract.py: bit-identical x and state on separately created deterministic operators (convdiff67_colscaled, Jacobi, restart 8, 2 x 8 + 3 iterations and a flush)."""
    K.sums_have_a_fixed_order(torch_cuda, "gmres", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """tests/solver_contract.py: update_values and the diagonal recomputed into the same array; the untouched solver equals one on a fresh operator bit for bit."""
    K.value_refresh(torch_cuda, "gmres", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """tests/solver_contract.py: a non-square plan, a shard plan, a misaligned dinv, restart 0 and 65: hipErrorInvalidValue, no handle, ValueError from the class."""
    K.create_refuses_what_it_must(torch_cuda, "gmres", dtype)


def test_sparse_operator_gmres_agrees_with_the_torch_loop(torch_cuda):
    """shiftskew67 in fp64 (the input BiCGStab does not solve): the method and the module-level loop are both within 1e-8 of spsolve; the info keys are those of cg; wrong length,
    dtype or shape raises."""
    torch = torch_cuda
    dt = np.dtype(np.float64)
    n, rp, ci, vt, b = _system("shiftskew67", dt)
    xs = _solved("shiftskew67", dt)[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, placement_tries=1) as op:
        x, info = op.gmres(bd, rtol=1e-12, maxiter=2000, restart=RESTART)
        xt, infot = torch_gmres(op, bd, tol=1e-12, maxiter=2000, restart=RESTART)
        print("library %s, torch loop %s" % (info, infot))
        assert info["converged"] and info["status"] == "converged" and infot["converged"], (info, infot)
        assert set(info) == {"iterations", "residual", "relative_residual", "converged", "status"}
        assert abs(info["iterations"] - infot["iterations"]) <= 8 + 3      # (the same method: the library looks every 8 iterations; 3: what rounding may move the count by)
        for got in (x.cpu().numpy(), xt.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs), (np.linalg.norm(got - xs), info, infot)
        n2, rp2, ci2, v2, b2 = _system("convdiff67_colscaled", dt)
    xs2 = _solved("convdiff67_colscaled", dt)[0]
    b2d = torch.from_numpy(b2).cuda()
    with SparseOperator(n2, n2, rp2, ci2, v2, placement_tries=1) as op:
        dinv = torch.from_numpy(M.inverse_diagonal(n2, rp2, ci2, v2, dt)).cuda()
        xj, infoj = op.gmres(b2d, rtol=1e-12, maxiter=2000, restart=RESTART, dinv=dinv)
        xtj, infotj = torch_gmres(op, b2d, tol=1e-12, maxiter=2000, restart=RESTART, dinv=dinv)
        assert infoj["converged"] and infotj["converged"]
        for got in (xj.cpu().numpy(), xtj.cpu().numpy()):
            assert np.linalg.norm(got - xs2) <= 1e-8 * np.linalg.norm(xs2)
        for bad in (b2d[:-1], b2d.float(), b2d.reshape(-1, 1)):
            with pytest.raises(ValueError):
                op.gmres(bad)
        with pytest.raises(ValueError):
            op.gmres(b2d, dinv=torch.ones(n2 + 1, dtype=b2d.dtype, device="cuda"))
        with pytest.raises(ValueError):
            op.gmres(b2d, restart=65)
