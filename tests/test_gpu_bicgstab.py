"""The BiCGStab solver in the library on the GPU (tilespmv_bicgstab_*; include/tilespmv.h) against its numpy mirror (tests/bicgstab_mirror.py, itself checked by
tests/test_bicgstab_cpu.py) and scipy's direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless a test says otherwise.

The GPU is compared with the mirror iterate for iterate only after 1 and 3 iterations (measured there: ~2e-16 in fp64, ~8e-8 in fp32, relative, in x): BiCGStab amplifies
rounding differences quickly — two summation orders of the fp64 mirror itself differ by 2e-16 in x after 3 iterations and by 9e-13 after 20.  Further on, a solve is judged by its
end: status, residual, error against spsolve.

What this solver promises like every other one is written once in tests/solver_contract.py, whose table has this solver's inputs and counts: graph capture and nothing
touched past the end run from tests/test_gpu_solver_contract.py; the fixed order of the sums, value refresh and the refusals of create are the tests of those names here."""
import numpy as np
import pytest

import bicgstab_mirror as M
import gpu_solver_util as U
import solver_contract as K
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import api
from tilespmv_amd.operator import SparseOperator, bicgstab as torch_bicgstab

pytestmark = pytest.mark.gpu

_CACHE = {}


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _solved(name, dtype):
    """The mirror's solve of a named input and the direct solution, computed once per value type: (xs, mirror iterations, mirror error).  Jacobi on the scaled input."""
    dt = np.dtype(dtype)
    if (name, dt) not in _CACHE:
        n, rp, ci, vt, b = _system(name, dt)
        dinv = M.inverse_diagonal(n, rp, ci, vt, dt) if name.endswith("_scaled") else None
        xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[(name, dt)] = (xs, itm, U.relerr(xm, xs))
    return _CACHE[(name, dt)]


def _early(torch, dt, A, b, plan, dinv, n, label):
    """x and rr after 1 and after 3 iterations against the mirror of A.  Bound: 100 x the per-product tolerance (the bound of tests/test_gpu_cg.py and test_gpu_cgls.py: another
    summation order over a few iterations); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    m = M.Mirror(A, dt, dinv)
    m.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    dd = None if dinv is None else U.vec(torch, dinv, n, dt)
    with api.BiCGStab(plan, None if dd is None else dd.data_ptr()) as bs:
        bs.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
        s0 = bs.state(U.stream(torch))
        print("%s %s begin: rr %.3g bb %.3g" % (label, dt, U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)) <= bound
        done = 0
        for step in (1, 2):
            bs.iterate(xd.data_ptr(), step, U.stream(torch)); m.iterate(step); done += step
            s = bs.state(U.stream(torch))
            dx = U.relerr(U.host(xd, n), m.x.astype(np.float64))
            drr = U.dist(s["rr"], m.rr)
            print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)" % (label, dt, done, dx, drr, bound))
            assert s["iterations"] == done == m.iterations and s["status"] == api.CG_RUNNING == m.status()
            assert dx <= bound and drr <= bound
    return bd, xd, dd


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt), b, op.A, None, n, "convdiff67")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [{}, dict(deterministic=-1, placement_tries=-1)])
def test_solves(torch_cuda, kw, dtype):
    """tilespmv_bicgstab_solve on convdiff67 with maxiter = 2 x the mirror's count: CONVERGED, sqrt(rr / bb) <= rtol, and an error against spsolve within 10 x the mirror's own.
    The second case is the builder's default (timed) plans, whatever form they pick."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    xs, itm, errm = _solved("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt, **kw) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=U.stream(torch))
        x = U.host(xd, n)
    err = U.relerr(x, xs)
    print("convdiff67 %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error %.3g (mirror %.3g)" % (dt, kw, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi(torch_cuda, dtype):
    """convdiff67_scaled: dinv from tilespmv_csr_diagonal_device(invert) equals numpy's; preconditioned BiCGStab converges within 2 x the mirror's count to an error within 10 x
    the mirror's; the plain solver on the same plan is still running at that cap."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67_scaled", dt)
    xs, itm, errm = _solved("convdiff67_scaled", dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    dinv = U.vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    assert np.array_equal(U.host(dinv, n), M.inverse_diagonal(n, rp, ci, vt, dt))
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.BiCGStab(op.A, dinv.data_ptr()) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s: Jacobi BiCGStab %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:n].zero_()
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain BiCGStab on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    U.intact((dinv, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_transposed_plan_solves_the_transposed_system(torch_cuda, dtype):
    """api.BiCGStab(op.AT): three iterations equal the mirror of A^T."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt).T.tocsr(), b, op.AT, None, n, "convdiff67^T")


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """rr = 0 exactly (b = 0; A = 2 I after one iteration, at the half step) stops the changes; sigma = 0 exactly (skew) raises the breakdown flag and leaves x alone."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    # b = 0
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        zero, xd = U.vec(torch, None, n, dt), U.vec(torch, b, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()
            bs.begin(zero.data_ptr(), xd.data_ptr(), stream)
            bs.iterate(xd.data_ptr(), 16, stream)
            s = bs.state(stream)
            x = U.host(xd, n)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
    # A = 2 I: alpha = 1/2 exactly, s = 0, t.t = 0 -> omega = 0: converged at the half step
    n, rp, ci, v = M.problem("2I")
    b = M.rhs(n).astype(dt)
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.BiCGStab(op.A) as bs:
            bs.begin(bd.data_ptr(), xd.data_ptr(), stream)
            bs.iterate(xd.data_ptr(), 1, stream)
            s = bs.state(stream)
            x1 = U.host(xd, n)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
            bs.iterate(xd.data_ptr(), 16, stream)
            s = bs.state(stream)
            assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), x1)
    # skew: rhat.v = b.A b = 0 exactly in the first iteration
    n, rp, ci, v = M.problem("skew")
    b, x0 = M.skew_rhs(n).astype(dt), np.zeros(n, dtype=dt)
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(U.host(xd, n), x0) and s["rr"] == float(b.astype(np.float64) @ b.astype(np.float64))


# ---- the promises shared with the other solvers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """tests/solver_contract.py: bit-identical x and state on separately created deterministic operators (convdiff67_scaled, Jacobi, 20 iterations)."""
    K.sums_have_a_fixed_order(torch_cuda, "bicgstab", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """tests/solver_contract.py: update_values and the diagonal recomputed into the same array; the untouched solver equals one on a fresh operator bit for bit."""
    K.value_refresh(torch_cuda, "bicgstab", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """tests/solver_contract.py: a non-square plan, a shard plan, a misaligned dinv: hipErrorInvalidValue, no handle, ValueError from the class."""
    K.create_refuses_what_it_must(torch_cuda, "bicgstab", dtype)


def test_sparse_operator_bicgstab_agrees_with_the_torch_loop(torch_cuda):
    """convdiff67 in fp64: the method and the module-level loop are both within 1e-8 of spsolve; the info keys are those of cg; wrong length, dtype or shape raises."""
    torch = torch_cuda
    dt = np.dtype(np.float64)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    xs = _solved("convdiff67", dt)[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, placement_tries=1) as op:
        x, info = op.bicgstab(bd, rtol=1e-12, maxiter=1000)
        xt, infot = torch_bicgstab(op, bd, tol=1e-12, maxiter=1000)
        print("library %s, torch loop %s" % (info, infot))
        assert info["converged"] and info["status"] == "converged" and infot["converged"], (info, infot)
        assert set(info) == {"iterations", "residual", "relative_residual", "converged", "status"}
        for got in (x.cpu().numpy(), xt.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs), (np.linalg.norm(got - xs), info, infot)
        dinv = torch.from_numpy(M.inverse_diagonal(n, rp, ci, vt, dt)).cuda()
        xj, infoj = op.bicgstab(bd, rtol=1e-12, maxiter=1000, dinv=dinv, x0=x)
        xtj, infotj = torch_bicgstab(op, bd, tol=1e-12, maxiter=1000, dinv=dinv)
        assert infoj["converged"] and infotj["converged"]
        for got in (xj.cpu().numpy(), xtj.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs)
        for bad in (bd[:-1], bd.float(), bd.reshape(-1, 1)):
            with pytest.raises(ValueError):
                op.bicgstab(bad)
        with pytest.raises(ValueError):
            op.bicgstab(bd, dinv=torch.ones(n + 1, dtype=bd.dtype, device="cuda"))
