"""The least-squares solver in the library on the GPU (tilespmv_cgls_*, tilespmv_csr_row_sqnorms_device; include/tilespmv.h) against its numpy mirror
(tests/cgls_mirror.py, itself checked by tests/test_cgls_cpu.py) and scipy's LSQR / direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless
a test says otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cgls_mirror as M
from tilespmv_amd import _lib, api, generators as G
from tilespmv_amd.operator import SparseOperator, cgls as torch_cgls

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
PRODUCT_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # README: the project's per-product tolerance on real-valued data
SENTINEL = 777.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _op(rows, cols, rp, ci, v, dtype, **kw):
    kw.setdefault("deterministic", 1)
    kw.setdefault("placement_tries", 1)
    return SparseOperator(rows, cols, rp, ci, np.ascontiguousarray(v, dtype=dtype), dtype=dtype, **kw)


def _vec(torch, a, n, dtype):
    """A device vector of n elements with 16 sentinel elements behind it (the whole tensor)."""
    t = torch.full((n + 16,), SENTINEL, dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device="cuda")
    if a is None:
        t[:n].zero_()
    else:
        t[:n].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)))
    return t


def _host(t, n):
    return t.cpu().numpy()[:n].copy()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _system(name, dtype):
    dt = np.dtype(dtype)
    rows, cols, rp, ci, v = M.problem(name)
    return rows, cols, rp, ci, v.astype(dt), M.rhs(rows).astype(dt)


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def _dist(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    """tall: x, nn and rr after 1 and after 3 iterations.  Bound: 100 x the per-product tolerance (the bound of tests/test_gpu_cg.py: another summation order over a few
    iterations); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    m = M.Mirror(M.scipy_csr(rows, cols, rp, ci, vt), dt)
    m.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    with _op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, rows, dt), _vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.0, _stream(torch))
            s0 = ls.state(_stream(torch))
            print("%s begin: nn %.3g nn0 %.3g rr %.3g bb %.3g" % (dt, _dist(s0["nn"], m.nn), _dist(s0["nn0"], m.nn0), _dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)))
            assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
            assert max(_dist(s0["nn"], m.nn), _dist(s0["nn0"], m.nn0), _dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)) <= bound
            done = 0
            for step in (1, 2):
                ls.iterate(xd.data_ptr(), step, _stream(torch)); m.iterate(step); done += step
                s = ls.state(_stream(torch))
                dx = _relerr(_host(xd, cols), m.x.astype(np.float64))
                dnn, drr = _dist(s["nn"], m.nn), _dist(s["rr"], m.rr)
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
    with _op(rows, cols, rp, ci, vt, dt, **kw) as op:
        bd, xd = _vec(torch, b, rows, dt), _vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), damp=damp, rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=_stream(torch))
        x = _host(xd, cols)
    err, errm = _relerr(x, xs), _relerr(xm, xs)
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


def _device_csr(torch, rp, ci, v):
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()


def _transpose_pattern(torch, rows, cols, rpd, cid, dt):
    """rpT and srcT of the pattern, by tilespmv_csr_transpose_device (no values gathered): what a caller keeps for the column scaling."""
    nnz = cid.numel()
    rpT = torch.zeros(cols + 1, dtype=torch.int32, device="cuda")
    ciT = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    srcT = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    api.csr_transpose_device(rows, cols, rpd.data_ptr(), cid.data_ptr(), None, rpT.data_ptr(), ciT.data_ptr(), None, srcT.data_ptr(), dtype=dt, stream=_stream(torch))
    return rpT, srcT


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_scaling(torch_cuda, dtype):
    """tall_scaled: cinv = 1 / |a_j|^2 from one device transposition of the pattern and tilespmv_csr_row_sqnorms_device through srcT equals numpy's column sums of squares;
    preconditioned CGLS within 2 x the mirror's count; the plain solver on the same plans still running at that cap.  wide: empty columns give 1."""
    torch, dt = torch_cuda, np.dtype(dtype)
    tol = 1e-14 if dt == np.float64 else 1e-6
    stream = _stream(torch)
    # empty columns
    rows, cols, rp, ci, vt, b = _system("wide", dt)
    rpd, cid, vd = _device_csr(torch, rp, ci, vt)
    rpT, srcT = _transpose_pattern(torch, rows, cols, rpd, cid, dt)
    for invert in (False, True):
        out = _vec(torch, None, cols, dt)
        api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=invert, stream=stream, dtype=dt)
        torch.cuda.synchronize()
        sq = np.bincount(ci, weights=vt.astype(np.float64) ** 2, minlength=cols)
        empty = sq == 0
        want = np.where(empty, 1.0, 1.0 / np.where(empty, 1.0, sq)) if invert else sq
        got = _host(out, cols).astype(np.float64)
        assert empty.sum() > 0 and np.array_equal(got[empty], want[empty])
        assert (np.abs(got - want)[~empty] / want[~empty]).max() <= tol
        assert (out.cpu().numpy()[cols:] == SENTINEL).all()
    # without src: plain row norms of A
    out = _vec(torch, None, rows, dt)
    api.csr_row_sqnorms_device(rows, rpd.data_ptr(), None, vd.data_ptr(), out.data_ptr(), stream=stream, dtype=dt)
    torch.cuda.synchronize()
    rowsq = np.bincount(np.repeat(np.arange(rows), np.diff(rp)), weights=vt.astype(np.float64) ** 2, minlength=rows)
    assert (np.abs(_host(out, rows) - rowsq) / rowsq).max() <= tol
    # the scaled input
    rows, cols, rp, ci, vt, b = _system("tall_scaled", dt)
    A = M.scipy_csr(rows, cols, rp, ci, vt)
    rpd, cid, vd = _device_csr(torch, rp, ci, vt)
    rpT, srcT = _transpose_pattern(torch, rows, cols, rpd, cid, dt)
    cinv = _vec(torch, None, cols, dt)
    api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), vd.data_ptr(), cinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    want = 1.0 / np.bincount(ci, weights=vt.astype(np.float64) ** 2, minlength=cols)
    rel = (np.abs(_host(cinv, cols) - want) / want).max()
    print("%s: cinv through srcT, largest relative difference from numpy %.3g (bound %.3g)" % (dt, rel, tol))
    assert rel <= tol
    xs = M.lsqr_x(A, b, scale_columns=True)
    xm, itm, stm, relm = M.Mirror(A, dt, M.column_cinv(A, dt)).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    with _op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, rows, dt), _vec(torch, None, cols, dt)
        with api.CGLS(op.A, op.AT, cinv.data_ptr()) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err, errm = _relerr(_host(xd, cols), xs), _relerr(xm, xs)
        print("%s: column-scaled CGLS %d iterations (mirror %d), sqrt(nn/nn0) %.3g, error vs lsqr %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_normal_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_normal_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:cols].zero_()
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain CGLS on the same plans: %d iterations, status %s, sqrt(nn/nn0) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_normal_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    assert (cinv.cpu().numpy()[cols:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """an operator with a value map solves with tall's values; update_values to tall_scaled's (the same pattern), cinv recomputed through srcT into the SAME
    array, then a warm-started solve.  The result equals, bit for bit on these deterministic plans, that of an operator built fresh from the new values and started from the same x."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    rows, cols, rp, ci, v1, b = _system("tall", dt)
    v2 = _system("tall_scaled", dt)[4]
    rpd, cid, v1d = _device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    rpT, srcT = _transpose_pattern(torch, rows, cols, rpd, cid, dt)
    cinv, bd, xd = _vec(torch, None, cols, dt), _vec(torch, b, rows, dt), _vec(torch, None, cols, dt)
    with _op(rows, cols, rp, ci, v1, dt, value_map=True) as op:
        api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), v1d.data_ptr(), cinv.data_ptr(), invert=True, stream=stream, dtype=dt)
        with api.CGLS(op.A, op.AT, cinv.data_ptr()) as ls:
            s1 = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=200, stream=stream)
            assert s1["status"] == api.CG_CONVERGED
            x1 = _host(xd, cols)
            op.update_values(v2d.data_ptr(), stream)
            api.csr_row_sqnorms_device(cols, rpT.data_ptr(), srcT.data_ptr(), v2d.data_ptr(), cinv.data_ptr(), invert=True, stream=stream, dtype=dt)
            s2 = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=200, stream=stream)      # (warm: x holds the first solution)
            x2 = _host(xd, cols)
    with _op(rows, cols, rp, ci, v2, dt, value_map=True) as fresh:
        xf = _vec(torch, x1, cols, dt)
        with api.CGLS(fresh.A, fresh.AT, cinv.data_ptr()) as ls:
            sf = ls.solve(bd.data_ptr(), xf.data_ptr(), rtol=M.RTOL[dt], maxiter=200, stream=stream)
    A2 = M.scipy_csr(rows, cols, rp, ci, v2)
    xs = M.lsqr_x(A2, b, scale_columns=True)
    print("%s: refreshed %d iterations, fresh %d; error vs lsqr %.3g" % (dt, s2["iterations"], sf["iterations"], _relerr(x2, xs)))
    assert s2["status"] == api.CG_CONVERGED and sf["status"] == api.CG_CONVERGED
    assert s2["iterations"] == sf["iterations"] and s2["nn"] == sf["nn"] and np.array_equal(x2, _host(xf, cols))
    assert _relerr(x2, xs) <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two solvers on two separately created deterministic operators: bit-identical x, nn and rr after 20 iterations (with damping and cinv, so that every sum takes part)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    cinv = _vec(torch, M.column_cinv(M.scipy_csr(rows, cols, rp, ci, vt), dt), cols, dt)
    bd = _vec(torch, b, rows, dt)
    results = []
    for _ in range(2):
        with _op(rows, cols, rp, ci, vt, dt) as op:
            xd = _vec(torch, None, cols, dt)
            with api.CGLS(op.A, op.AT, cinv.data_ptr()) as ls:
                ls.begin(bd.data_ptr(), xd.data_ptr(), 0.5, _stream(torch))
                ls.iterate(xd.data_ptr(), 20, _stream(torch))
                s = ls.state(_stream(torch))
            results.append((_host(xd, cols), s))
    (xa, sa), (xb, sb) = results
    assert sa["iterations"] == 20 and np.array_equal(xa, xb) and sa["nn"] == sb["nn"] and sa["rr"] == sb["rr"] and xa.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, dtype):
    """begin + iterate(8) captured with torch's graph API on a side stream (one linear chain, as tests/test_gpu_cg.py captures iterate) and replayed twice from the same x0:
    each replay equals the eager run bit for bit."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    x0 = (0.01 * M.rhs(cols)).astype(dt)
    with _op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, rows, dt), _vec(torch, x0, cols, dt)
        ls = api.CGLS(op.A, op.AT)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = side.cuda_stream
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.5, st)
            ls.iterate(xd.data_ptr(), 8, st)                      # (uncaptured: the comparison, and the warm-up)
            s8 = ls.state(st); x8 = _host(xd, cols)
            xd[:cols].copy_(torch.from_numpy(x0))
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                ls.begin(bd.data_ptr(), xd.data_ptr(), 0.5, st)
                ls.iterate(xd.data_ptr(), 8, st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert np.array_equal(_host(xd, cols), x0)                # (captured, not run)
        for _ in range(2):
            xd[:cols].copy_(torch.from_numpy(x0))
            torch.cuda.synchronize()
            graph.replay(); torch.cuda.synchronize()
            s = ls.state(_stream(torch))
            assert np.array_equal(_host(xd, cols), x8)
            assert s["iterations"] == 8 and s["nn"] == s8["nn"] and s["rr"] == s8["rr"] and s["status"] == api.CG_RUNNING
        del graph
        ls.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """gamma = 0 exactly (b = 0; b orthogonal to the range of A; A = 2 I after one iteration) stops the changes, a negative cinv raises the breakdown flag and leaves x alone."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    x0 = M.rhs(cols)[::-1].astype(dt)
    with _op(rows, cols, rp, ci, vt, dt) as op:
        # b = 0
        zero, xd = _vec(torch, None, rows, dt), _vec(torch, x0, cols, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not _host(xd, cols).any()
            ls.begin(zero.data_ptr(), xd.data_ptr(), 0.0, stream)
            ls.iterate(xd.data_ptr(), 16, stream)
            s = ls.state(stream)
            x = _host(xd, cols)
            assert s["iterations"] == 16 and s["nn"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
        # a negative cinv: gamma < 0 in the first iteration
        neg = _vec(torch, -M.column_cinv(M.scipy_csr(rows, cols, rp, ci, vt), dt), cols, dt)
        bd, xd = _vec(torch, b, rows, dt), _vec(torch, x0, cols, dt)
        with api.CGLS(op.A, op.AT, neg.data_ptr()) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(_host(xd, cols), x0)
    # b orthogonal to the range of A, from a non-zero start
    n = 4099
    A, bo = M.orthogonal_case(n, dt)
    with _op(2 * n, n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, dt) as op:
        bd, xd = _vec(torch, bo, 2 * n, dt), _vec(torch, M.rhs(n), n, dt)
        with api.CGLS(op.A, op.AT) as ls:
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
        assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and s["nn0"] == 0.0 and not _host(xd, n).any()
    # A = 2 I: one iteration gives s = 0 exactly (alpha = 1/4 is exact)
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dt)
    b = M.rhs(n).astype(dt)
    with _op(n, n, rp, ci, v, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.CGLS(op.A, op.AT) as ls:
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.0, stream)
            ls.iterate(xd.data_ptr(), 1, stream)
            s = ls.state(stream)
            x1 = _host(xd, n)
            assert s["nn"] == 0.0 and s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
            ls.iterate(xd.data_ptr(), 16, stream)
            s = ls.state(stream)
            assert s["iterations"] == 17 and s["nn"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(_host(xd, n), x1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """A plan in the other one's place (the shapes no longer match), a shard plan in either place, a misaligned cinv: hipErrorInvalidValue, no handle.
    Both plans exchanged — create(plan_AT, plan_A) — is NOT among the refusals: the two shapes still match each other, the library sees no vector length, and the pair is the
    legitimate solver of min |A^T y - c|; the test checks that it is exactly that (three iterations against the mirror of A^T)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    rows, cols, rp, ci, vt, b = _system("tall", dt)
    with _op(rows, cols, rp, ci, vt, dt) as op:
        shard = api.Plan.from_csr(rows, cols, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, tilerow_end=(rows // 16) // 2)
        shardT = api.Plan.from_csr(rows, cols, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, transpose=True, tilerow_end=((cols + 15) // 16) // 2)
        cinv = _vec(torch, np.ones(cols + 1), cols + 1, dt)
        cases = (("A in the place of A^T", op.A, op.A, None), ("A^T in the place of A", op.AT, op.AT, None), ("shard of A", shard, op.AT, None),
                 ("shard of A^T", op.A, shardT, None), ("misaligned cinv", op.A, op.AT, cinv.data_ptr() + dt.itemsize))
        for label, pa, pat, c in cases:
            h = C.c_void_p(1)
            rc = lib.tilespmv_cgls_create(C.byref(h), pa.h, pat.h, C.c_void_p(c))
            print("%s %s: rc %d, handle %s" % (dt, label, rc, h.value))
            assert rc == api.HIP_ERROR_INVALID_VALUE and not h, label
            with pytest.raises(ValueError):
                api.CGLS(pa, pat, c)
        with api.CGLS(op.A, op.AT, cinv.data_ptr()) as ls:      # (aligned: accepted)
            assert ls.h
        shard.close(); shardT.close()
        # both exchanged: the solver of the transposed problem
        c_rhs = M.rhs(cols).astype(dt)
        m = M.Mirror(M.scipy_csr(rows, cols, rp, ci, vt).T.tocsr(), dt); m.begin(c_rhs); m.iterate(3)
        cd, yd = _vec(torch, c_rhs, cols, dt), _vec(torch, None, rows, dt)
        with api.CGLS(op.AT, op.A) as ls:
            ls.begin(cd.data_ptr(), yd.data_ptr(), 0.0, _stream(torch))
            ls.iterate(yd.data_ptr(), 3, _stream(torch))
            s = ls.state(_stream(torch))
        dy = _relerr(_host(yd, rows), m.x.astype(np.float64))
        print("%s exchanged plans: 3 iterations of the transposed problem, |y - mirror| / |mirror| = %.3g" % (dt, dy))
        assert s["iterations"] == 3 and dy <= 100 * PRODUCT_TOL[dt] and _dist(s["nn"], m.nn) <= 100 * PRODUCT_TOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(5003, 1237), (1237, 5003)])
def test_nothing_is_touched_past_the_end(torch_cuda, rows, cols, dtype):
    """b, x and cinv with 16 sentinel elements behind them, on row and column counts that are multiples neither of 16 nor of the lane vector width: the sentinels survive a damped,
    column-scaled solve, b and cinv are unchanged, and three iterations equal the mirror's."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    assert rows % 4 == 3 or cols % 4 == 3
    rng = np.random.default_rng(29)
    k = min(rows, cols)
    _, _, rp, ci = G.from_coo(rows, cols, np.concatenate([np.repeat(np.arange(rows), 5), np.arange(k)]), np.concatenate([rng.integers(0, cols, rows * 5), np.arange(k)]))
    vt = (rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))).astype(dt)
    A = M.scipy_csr(rows, cols, rp, ci, vt)
    b, cinv = M.rhs(rows).astype(dt), M.column_cinv(A, dt)
    m3 = M.Mirror(A, dt, cinv); m3.begin(b, damp=0.5); m3.iterate(3)
    with _op(rows, cols, rp, ci, vt, dt) as op:
        bd, xd, cd = _vec(torch, b, rows, dt), _vec(torch, None, cols, dt), _vec(torch, cinv, cols, dt)
        with api.CGLS(op.A, op.AT, cd.data_ptr()) as ls:
            ls.begin(bd.data_ptr(), xd.data_ptr(), 0.5, stream)
            ls.iterate(xd.data_ptr(), 3, stream)
            s = ls.state(stream)
            dx = _relerr(_host(xd, cols), m3.x.astype(np.float64))
            print("%d x %d %s: 3 iterations, |x - mirror| / |mirror| = %.3g, nn %.6g (mirror %.6g)" % (rows, cols, dt, dx, s["nn"], m3.nn))
            assert dx <= 100 * PRODUCT_TOL[dt] and _dist(s["nn"], m3.nn) <= 100 * PRODUCT_TOL[dt] and _dist(s["rr"], m3.rr) <= 100 * PRODUCT_TOL[dt]
            xd[:cols].zero_()
            s = ls.solve(bd.data_ptr(), xd.data_ptr(), damp=0.5, rtol=M.RTOL[dt], maxiter=500, stream=stream)
        assert s["status"] == api.CG_CONVERGED
        assert _relerr(_host(xd, cols), M.lsqr_x(A, b, 0.5)) <= 100 * M.RTOL[dt]
        for t, n in ((bd, rows), (xd, cols), (cd, cols)):
            assert (t.cpu().numpy()[n:] == SENTINEL).all()
        assert np.array_equal(_host(bd, rows), b) and np.array_equal(_host(cd, cols), cinv)


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
