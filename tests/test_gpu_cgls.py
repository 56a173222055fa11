"""The least-squares solver in the library on the GPU (tilespmv_cgls_*, tilespmv_csr_row_sqnorms_device; include/tilespmv.h) against its numpy mirror
(tests/cgls_mirror.py, itself checked by tests/test_cgls_cpu.py) and scipy's LSQR / direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless
a test says otherwise.

What this solver promises like every other one is written once in tests/solver_contract.py, whose table has this solver's inputs and counts: graph capture and nothing
touched past the end run from tests/test_gpu_solver_contract.py; the fixed order of the sums, value refresh and the refusals of create are the tests of those names here."""
import numpy as np
import pytest

import cgls_mirror as M
import gpu_solver_util as U
import solver_contract as K
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import api, generators as G
from tilespmv_amd.operator import SparseOperator, cgls as torch_cgls

pytestmark = pytest.mark.gpu


def _system(name, dtype):
    dt = np.dtype(dtype)
    rows, cols, rp, ci, v = M.problem(name)
    return rows, cols, rp, ci, v.astype(dt), M.rhs(rows).astype(dt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    """tall: x, nn and rr after 1 and after 3 iterations.  Bound: 100 x the per-product tolerance (the bound of tests/test_gpu_cg.py: another summation order over a few
    iterations); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    m = M.Mirror(M.scipy_csr(rows, cols, rp, ci, vt), dt)
    m.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    with U.rect_op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.0, U.stream(torch))
            s0 = ls.state(U.stream(torch))
            print("%s begin: nn %.3g nn0 %.3g rr %.3g bb %.3g" % (dt, U.dist(s0["nn"], m.nn), U.dist(s0["nn0"], m.nn0), U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)))
            assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
            assert max(U.dist(s0["nn"], m.nn), U.dist(s0["nn0"], m.nn0), U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)) <= bound
            done = 0
            for step in (1, 2):
                ls.iterate(xd.data_ptr(), step, U.stream(torch)); m.iterate(step); done += step
                s = ls.state(U.stream(torch))
                dx = U.relerr(U.host(xd, cols), m.x.astype(np.float64))
                dnn, drr = U.dist(s["nn"], m.nn), U.dist(s["rr"], m.rr)
                print("%s after %d iterations: |x - mirror| / |mirror| = %.3g, nn %.3g, rr %.3g (bound %.3g)" % (dt, done, dx, dnn, drr, bound))
                assert s["iterations"] == done and s["status"] == api.CG_RUNNING
                assert dx <= bound and dnn <= bound and drr <= bound


def _reference(name, A, b, damp):
    if name == "square":
        import scipy.sparse.linalg as spla
        return spla.spsolve(A.astype(np.float64).tocsc(), b.astype(np.float64))
    return M.lsqr_x(A, b, damp)


def _solve_case(torch, name, dt, damp, kw):
    rows, cols, rp, ci, vt, b = _system(name, dt)
    A = M.scipy_csr(rows, cols, rp, ci, vt)
    xs = _reference(name, A, b, damp)
    xm, itm, stm, relm = M.Mirror(A, dt).solve(b, damp=damp, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    with U.rect_op(rows, cols, rp, ci, vt, dt, **kw) as op:
        bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), damp=damp, rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=U.stream(torch))
        x = U.host(xd, cols)
    err, errm = U.relerr(x, xs), U.relerr(xm, xs)
    print("%s %s damp %g %s: GPU %d iterations (mirror %d), sqrt(nn/nn0) %.3g, error %.3g (mirror %.3g)" % (name, dt, damp, kw, s["iterations"], itm, s["relative_normal_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_normal_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kw", [("tall", {}), ("wide", {}), ("square", {}), ("stacked", {}), ("tall", dict(deterministic=-1, placement_tries=-1))])
def test_solves(torch_cuda, name, kw, dtype):
    """tilespmv_cgls_solve with maxiter = 2 x the mirror's count: CONVERGED, sqrt(nn / nn0) <= rtol, and an error against the LSQR (wide: minimum-norm) / direct solution within
    10 x the mirror's own (the mirror of the same value type is the yardstick).  The last case is the builder's default (timed) plans, whatever form they pick."""
    _solve_case(torch_cuda, name, np.dtype(dtype), 0.0, kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_damping(torch_cuda, name, dtype):
    """damp = 2 against lsqr(damp=2), by the rule of test_solves."""
    _solve_case(torch_cuda, name, np.dtype(dtype), 2.0, {})


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_scaling(torch_cuda, dtype):
    """tall_scaled: cinv = 1 / |a_j|^2 from one device transposition of the pattern and tilespmv_csr_row_sqnorms_device through srcT equals numpy's column sums of squares;
    preconditioned CGLS within 2 x the mirror's count; the plain solver on the same plans still running at that cap.  wide: empty columns give 1."""
    torch, dt = torch_cuda, np.dtype(dtype)
    tol = 1e-14 if dt == np.float64 else 1e-6
    stream = U.stream(torch)
    # empty columns
    rows, cols, rp, ci, vt, b = _system("wide", dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    rpT, srcT = U.transpose_pattern(torch, rows, cols, rpd, cid, dt)
    for invert in (False, True):
        out = U.vec(torch, None, cols, dt)
        api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=invert, stream=stream, dtype=dt)
        torch.cuda.synchronize()
        sq = np.bincount(ci, weights=vt.astype(np.float64) ** 2, minlength=cols)
        empty = sq == 0
        want = np.where(empty, 1.0, 1.0 / np.where(empty, 1.0, sq)) if invert else sq
        got = U.host(out, cols).astype(np.float64)
        assert empty.sum() > 0 and np.array_equal(got[empty], want[empty])
        assert (np.abs(got - want)[~empty] / want[~empty]).max() <= tol
        U.intact((out, cols))
    # without src: plain row norms of A
    out = U.vec(torch, None, rows, dt)
    api.csr_row_sqnorms_device(rows, rpd.data_ptr(), None, vd.data_ptr(), out.data_ptr(), stream=stream, dtype=dt)
    torch.cuda.synchronize()
    rowsq = np.bincount(np.repeat(np.arange(rows), np.diff(rp)), weights=vt.astype(np.float64) ** 2, minlength=rows)
    assert (np.abs(U.host(out, rows) - rowsq) / rowsq).max() <= tol
    # the scaled input
    rows, cols, rp, ci, vt, b = _system("tall_scaled", dt)
    A = M.scipy_csr(rows, cols, rp, ci, vt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    rpT, srcT = U.transpose_pattern(torch, rows, cols, rpd, cid, dt)
    cinv = U.vec(torch, None, cols, dt)
    api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), vd.data_ptr(), cinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    want = 1.0 / np.bincount(ci, weights=vt.astype(np.float64) ** 2, minlength=cols)
    rel = (np.abs(U.host(cinv, cols) - want) / want).max()
    print("%s: cinv through srcT, largest relative difference from numpy %.3g (bound %.3g)" % (dt, rel, tol))
    assert rel <= tol
    xs = M.lsqr_x(A, b, scale_columns=True)
    xm, itm, stm, relm = M.Mirror(A, dt, M.column_cinv(A, dt)).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    with U.rect_op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT, cinv.data_ptr()) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err, errm = U.relerr(U.host(xd, cols), xs), U.relerr(xm, xs)
        print("%s: column-scaled CGLS %d iterations (mirror %d), sqrt(nn/nn0) %.3g, error vs lsqr %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_normal_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_normal_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:cols].zero_()
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain CGLS on the same plans: %d iterations, status %s, sqrt(nn/nn0) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_normal_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    U.intact((cinv, cols))


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """gamma = 0 exactly (b = 0; b orthogonal to the range of A; A = 2 I after one iteration) stops the changes, a negative cinv raises the breakdown flag and leaves x alone."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    x0 = M.rhs(cols)[::-1].astype(dt)
    with U.rect_op(rows, cols, rp, ci, vt, dt) as op:
        # b = 0
        zero, xd = U.vec(torch, None, rows, dt), U.vec(torch, x0, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not U.host(xd, cols).any()
            ls.begin(zero.data_ptr(), xd.data_ptr(), 0.0, stream)
            ls.iterate(xd.data_ptr(), 16, stream)
            s = ls.state(stream)
            x = U.host(xd, cols)
            assert s["iterations"] == 16 and s["nn"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
        # a negative cinv: gamma < 0 in the first iteration
        neg = U.vec(torch, -M.column_cinv(M.scipy_csr(rows, cols, rp, ci, vt), dt), cols, dt)
        bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, x0, cols, dt)
        with api.CGLS(op.A, op.AT, neg.data_ptr()) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(U.host(xd, cols), x0)
    # b orthogonal to the range of A, from a non-zero start
    n = 4099
    A, bo = M.orthogonal_case(n, dt)
    with U.rect_op(2 * n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, dt) as op:
        bd, xd = U.vec(torch, bo, 2 * n, dt), U.vec(torch, M.rhs(n), n, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
        assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and s["nn0"] == 0.0 and not U.host(xd, n).any()
    # A = 2 I: one iteration gives s = 0 exactly (alpha = 1/4 is exact)
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dt)
    b = M.rhs(n).astype(dt)
    with U.rect_op(n, n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.CGLS(op.A, op.AT) as ls:
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.0, stream)
            ls.iterate(xd.data_ptr(), 1, stream)
            s = ls.state(stream)
            x1 = U.host(xd, n)
            assert s["nn"] == 0.0 and s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
            ls.iterate(xd.data_ptr(), 16, stream)
            s = ls.state(stream)
            assert s["iterations"] == 17 and s["nn"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), x1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """tests/solver_contract.py: a plan in the other one's place (the shapes no longer match), a shard plan in either place, a misaligned cinv: hipErrorInvalidValue, no handle.
    Both plans exchanged — create(plan_AT, plan_A) — is NOT among the refusals: the two shapes still match each other, the library sees no vector length, and the pair is the
    legitimate solver of min |A^T y - c|; the test checks that it is exactly that (three iterations against the mirror of A^T)."""
    K.create_refuses_what_it_must(torch_cuda, "cgls", dtype)
    torch, dt = torch_cuda, np.dtype(dtype)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    with U.rect_op(rows, cols, rp, ci, vt, dt) as op:
        c_rhs = M.rhs(cols).astype(dt)
        m = M.Mirror(M.scipy_csr(rows, cols, rp, ci, vt).T.tocsr(), dt); m.begin(c_rhs); m.iterate(3)
        cd, yd = U.vec(torch, c_rhs, cols, dt), U.vec(torch, None, rows, dt)
        with api.CGLS(op.AT, op.A) as ls:
            ls.begin(cd.data_ptr(), yd.data_ptr(), 0.0, U.stream(torch))
            ls.iterate(yd.data_ptr(), 3, U.stream(torch))
            s = ls.state(U.stream(torch))
        dy = U.relerr(U.host(yd, rows), m.x.astype(np.float64))
        print("%s exchanged plans: 3 iterations of the transposed problem, |y - mirror| / |mirror| = %.3g" % (dt, dy))
        assert s["iterations"] == 3 and dy <= 100 * PRODUCT_TOL[dt] and U.dist(s["nn"], m.nn) <= 100 * PRODUCT_TOL[dt]
    U.intact((cd, cols), (yd, rows))


# ---- the promises shared with the other solvers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """tests/solver_contract.py: bit-identical x and state on separately created deterministic operators (tall, cinv, damp 0.5, 20 iterations)."""
    K.sums_have_a_fixed_order(torch_cuda, "cgls", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """tests/solver_contract.py: update_values and the diagonal recomputed into the same array; the untouched solver equals one on a fresh operator bit for bit."""
    K.value_refresh(torch_cuda, "cgls", dtype)


def test_sparse_operator_cgls_agrees_with_the_torch_loop(torch_cuda):
    """The 4000 x 300 matrix of tests/test_gpu_transpose.py::test_cgls_reaches_the_least_squares_solution, built the same way: the method and the module-level loop are both
    within 1e-8 of numpy.linalg.lstsq."""
    torch = torch_cuda
    rng = np.random.default_rng(13)
    rows, cols = 4000, 300
    r, c = np.repeat(np.arange(rows), 6), rng.integers(0, cols, rows * 6)
    r = np.concatenate([r, np.arange(cols)]); c = np.concatenate([c, np.arange(cols)])   # every column held
    _, _, rp, ci = G.from_coo(rows, cols, r, c)
    nnz = int(rp[rows])
    v = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    dense = np.zeros((rows, cols)); np.add.at(dense, (np.repeat(np.arange(rows), np.diff(rp)), ci), v)
    b = rng.standard_normal(rows)
    want = np.linalg.lstsq(dense, b, rcond=None)[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(rows, cols, rp, ci, v, placement_tries=1) as op:
        x, info = op.cgls(bd, rtol=1e-12, maxiter=500)
        xt, infot = torch_cgls(op, bd, tol=1e-13, maxiter=500)
        assert info["converged"] and info["status"] == "converged" and infot["converged"], (info, infot)
        assert set(info) == {"iterations", "normal_residual", "relative_normal_residual", "residual", "converged", "status"}
        for got in (x.cpu().numpy(), xt.cpu().numpy()):
            assert np.linalg.norm(got - want) <= 1e-8 * np.linalg.norm(want), (np.linalg.norm(got - want), info, infot)
        print("library %d iterations, torch loop %d; residual %.6g vs %.6g" % (info["iterations"], infot["iterations"], info["residual"], infot["residual"]))
        assert abs(info["residual"] - infot["residual"]) <= 1e-8 * infot["residual"]
        xd, infod = op.cgls(bd, rtol=1e-12, maxiter=500, damp=1.0, cinv=torch.ones(cols, dtype=bd.dtype, device="cuda"))
        wantd = np.linalg.solve(dense.T @ dense + np.eye(cols), dense.T @ b)
        assert infod["converged"] and np.linalg.norm(xd.cpu().numpy() - wantd) <= 1e-8 * np.linalg.norm(wantd)
        for bad in (bd[:-1], bd.float(), bd.reshape(-1, 1)):
            with pytest.raises(ValueError):
                op.cgls(bad)
        with pytest.raises(ValueError):
            op.cgls(bd, cinv=torch.ones(cols + 1, dtype=bd.dtype, device="cuda"))
