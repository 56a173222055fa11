"""The solver in the library on the GPU (tilespmv_cg_*, tilespmv_csr_diagonal_device; include/tilespmv.h) against its numpy mirror (tests/cg_mirror.py, itself
checked by tests/test_cg_cpu.py) and scipy's direct solution.  Plans are created with deterministic=1, placement_tries=1 through Plan.from_csr unless a test says otherwise.

What this solver promises like every other one is written once in tests/solver_contract.py, whose table has this solver's inputs and counts: graph capture and nothing
touched past the end run from tests/test_gpu_solver_contract.py; the fixed order of the sums, value refresh and the refusals of create are the tests of those names here."""
import numpy as np
import pytest

import cg_mirror as M
import gpu_solver_util as U
import solver_contract as K
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import api

pytestmark = pytest.mark.gpu


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    return n, rp, ci, vt, b


def _xs(n, rp, ci, vt, b):
    return M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    """Tri-mesh input (Gershgorin: spectrum in [1, 13], nothing is amplified): x and rr after 1 and after 3 iterations.  Bound: 100 x the per-product tolerance (three iterations of
    another summation order: ordered tree here, pairwise in numpy); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("tri200", dt)
    m = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt)
    m.begin(b)
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
        s0 = cg.state(U.stream(torch))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert abs(s0["bb"] - m.bb) <= 100 * PRODUCT_TOL[dt] * m.bb and abs(s0["rr"] - m.rr) <= 100 * PRODUCT_TOL[dt] * m.rr
        done = 0
        for step in (1, 2):
            cg.iterate(xd.data_ptr(), step, U.stream(torch)); m.iterate(step); done += step
            s = cg.state(U.stream(torch))
            x = U.host(xd, n)
            dx = float(np.linalg.norm(x.astype(np.float64) - m.x.astype(np.float64)) / np.linalg.norm(m.x.astype(np.float64)))
            drr = abs(s["rr"] - m.rr) / m.rr
            print("%s after %d iterations: |x - mirror| / |mirror| = %.3g, |rr - mirror| / mirror = %.3g (bound %.3g)" % (dt, done, dx, drr, 100 * PRODUCT_TOL[dt]))
            assert s["iterations"] == done and s["status"] == api.CG_RUNNING
            assert dx <= 100 * PRODUCT_TOL[dt] and drr <= 100 * PRODUCT_TOL[dt]
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kw", [("lap128", {}), ("tri200", {}), ("fem12", {}), ("lap128", dict(deterministic=-1, placement_tries=-1))])
def test_solves(torch_cuda, name, kw, dtype):
    """tilespmv_cg_solve with maxiter = 2 x the mirror's count: CONVERGED, sqrt(rr / bb) <= rtol, and an error against the direct solution within 10 x the mirror's own (the
    mirror of the same value type is the yardstick; x 10 because CG carries rounding differences forward over hundreds of iterations).  The last case is the builder's
    default plan, whatever form it picks."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    xs = _xs(n, rp, ci, vt, b)
    xm, itm, stm, relm = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    plan = U.square_plan(n, rp, ci, vt, dt, **kw)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=U.stream(torch))
    x = U.host(xd, n)
    err, errm = U.relerr(x, xs), U.relerr(xm, xs)
    print("%s %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (name, dt, kw, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi(torch_cuda, dtype):
    """The scaled Laplacian (diagonal over six decades): the inverse diagonal from tilespmv_csr_diagonal_device, Jacobi-PCG within 2 x the mirror's count, and plain CG on the
    same plan still running at that cap."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("lap128_scaled", dt)
    A = M.scipy_csr(n, rp, ci, vt)
    want = (dt.type(1) / A.diagonal().astype(dt)).astype(dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    dinv = U.vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=U.stream(torch), dtype=dt)
    torch.cuda.synchronize()
    got = U.host(dinv, n)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("%s: inverse diagonal, largest difference %.3g ulp, %d of %d bit-equal" % (dt, ulps.max(), int((got == want).sum()), n))
    assert ulps.max() <= 1.0
    U.intact((dinv, n))
    xs = _xs(n, rp, ci, vt, b)
    xm, itm, stm, relm = M.Mirror(A, dt, want).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan, dinv.data_ptr()) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=U.stream(torch))
    err, errm = U.relerr(U.host(xd, n), xs), U.relerr(xm, xs)
    print("%s: Jacobi-PCG %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    xd[:n].zero_()
    with api.CG(plan) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=U.stream(torch))
    print("%s: plain CG on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
    assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_diagonal_with_a_duplicate_and_a_missing_entry(torch_cuda, dtype):
    """The header: duplicates added, 0 where no entry is stored; inverted: 1 where the sum is 0."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rp = np.array([0, 3, 4, 6, 6], dtype=np.int32)                 # row 0: (0,0) twice; row 1: no diagonal; row 2: (2,2) + (2,3); row 3: empty
    ci = np.array([0, 1, 0, 3, 2, 3], dtype=np.int32)
    v = np.array([1.5, 7.0, 2.5, 9.0, -8.0, 3.0], dtype=dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, v)
    for invert, want in ((False, [4.0, 0.0, -8.0, 0.0]), (True, [0.25, 1.0, -0.125, 1.0])):
        out = U.vec(torch, None, 4, dt)
        api.csr_diagonal_device(4, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=invert, stream=U.stream(torch), dtype=dt)
        torch.cuda.synchronize()
        assert np.array_equal(U.host(out, 4), np.array(want, dtype=dt)), (invert, U.host(out, 4))
        U.intact((out, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """rho = 0 exactly (b = 0; A = 2 I after one iteration) stops the changes, p.Ap < 0 (a negative definite matrix) raises the breakdown flag and leaves x alone: ordinary
    data-dependent branches."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    # b = 0, x = 0
    n, rp, ci, vt, b = _system("lap128", dt)
    plan = U.square_plan(n, rp, ci, vt, dt)
    zero, xd = U.vec(torch, None, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        s = cg.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
        assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()
        cg.begin(zero.data_ptr(), xd.data_ptr(), stream)
        cg.iterate(xd.data_ptr(), 16, stream)
        s = cg.state(stream)
        x = U.host(xd, n)
        assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED
        assert np.isfinite(x).all() and not x.any()
    # A = -(the Laplacian): p.Ap < 0 in the first iteration
    x0 = M.rhs(n)[::-1].astype(dt)
    neg = U.square_plan(n, rp, ci, -vt, dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
    with api.CG(neg) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
        assert np.array_equal(U.host(xd, n), x0)
    neg.close(); plan.close()
    # A = 2 I: one iteration gives r = 0 exactly (alpha = 1/2 is exact)
    n = 4096
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dt)
    b = M.rhs(n).astype(dt)
    plan = U.square_plan(n, rp, ci, v, dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
        cg.iterate(xd.data_ptr(), 1, stream)
        s = cg.state(stream)
        x1 = U.host(xd, n)
        assert s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
        cg.iterate(xd.data_ptr(), 16, stream)
        s = cg.state(stream)
        assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), x1)
    plan.close()


# ---- the promises shared with the other solvers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """tests/solver_contract.py: bit-identical x and state on separately created deterministic operators (fem12: two solves on one plan and one on a second)."""
    K.sums_have_a_fixed_order(torch_cuda, "cg", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi_follows_a_value_update(torch_cuda, dtype):
    """tests/solver_contract.py: update_values and the diagonal recomputed into the same array; the untouched solver equals one on a fresh operator bit for bit."""
    K.value_refresh(torch_cuda, "cg", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_and_non_square_plans_are_refused(torch_cuda, dtype):
    """tests/solver_contract.py: a shard, a non-square plan, a misaligned dinv: hipErrorInvalidValue, no handle, ValueError from the class."""
    K.create_refuses_what_it_must(torch_cuda, "cg", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_operator_cg_is_the_library_solver(torch_cuda, dtype):
    from tilespmv_amd.operator import SparseOperator
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("fem12", dt)
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, deterministic=1, placement_tries=1) as op:
        x, info = op.cg(bd, rtol=M.RTOL[dt], maxiter=500)
        xd = U.vec(torch, None, n, dt)
        with api.CG(op.A) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
        assert info["converged"] and info["status"] == "converged" and info["iterations"] == s["iterations"] and info["relative_residual"] <= M.RTOL[dt]
        assert np.array_equal(x.cpu().numpy(), U.host(xd, n))
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = torch.from_numpy((dt.type(1) / A.diagonal().astype(dt)).astype(dt)).cuda()
        xj, infoj = op.cg(bd, rtol=M.RTOL[dt], maxiter=500, dinv=dinv)
        assert infoj["converged"] and infoj["iterations"] <= info["iterations"]
        xs = _xs(n, rp, ci, vt, b)
        assert U.relerr(xj.cpu().numpy(), xs) <= 100 * M.RTOL[dt]      # (diagonally dominant, condition number below 50: the error stays within two decades of the residual)
        # a transposed plan qualifies when square (of a symmetric matrix it multiplies by A itself)
        xd[:n].zero_()
        with api.CG(op.AT) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
        assert s["status"] == api.CG_CONVERGED and U.relerr(U.host(xd, n), xs) <= 100 * M.RTOL[dt]
