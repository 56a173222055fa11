"""The solver in the library on the GPU (tilespmv_cg_*, tilespmv_csr_diagonal_device; include/tilespmv.h) against its numpy mirror (tests/cg_mirror.py, itself
checked by tests/test_cg_cpu.py) and scipy's direct solution.  Plans are created with deterministic=1, placement_tries=1 through Plan.from_csr unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import cg_mirror as M
from tilespmv_amd import _lib, api, generators as G

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
PRODUCT_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # README: the project's per-product tolerance on real-valued data
SENTINEL = 777.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _plan(n, rp, ci, v, dtype, **kw):
    kw.setdefault("deterministic", 1)
    kw.setdefault("placement_tries", 1)
    return api.Plan.from_csr(n, n, len(ci), rp, ci, np.ascontiguousarray(v, dtype=dtype), dtype=dtype, **kw)


def _vec(torch, a, n, dtype):
    """A device vector of n elements with 16 sentinel elements behind it: (whole tensor, data_ptr)."""
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
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    return n, rp, ci, vt, b


def _xs(n, rp, ci, vt, b):
    return M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    """Tri-mesh input (Gershgorin: spectrum in [1, 13], nothing is amplified): x and rr after 1 and after 3 iterations.  Bound: 100 x the per-product tolerance (three iterations of
    another summation order: ordered tree here, pairwise in numpy); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("tri200", dt)
    m = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt)
    m.begin(b)
    plan = _plan(n, rp, ci, vt, dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
        s0 = cg.state(_stream(torch))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert abs(s0["bb"] - m.bb) <= 100 * PRODUCT_TOL[dt] * m.bb and abs(s0["rr"] - m.rr) <= 100 * PRODUCT_TOL[dt] * m.rr
        done = 0
        for step in (1, 2):
            cg.iterate(xd.data_ptr(), step, _stream(torch)); m.iterate(step); done += step
            s = cg.state(_stream(torch))
            x = _host(xd, n)
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
    plan = _plan(n, rp, ci, vt, dt, **kw)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=_stream(torch))
    x = _host(xd, n)
    err, errm = _relerr(x, xs), _relerr(xm, xs)
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
    rpd, cid, vd = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(vt).cuda()
    dinv = _vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=_stream(torch), dtype=dt)
    torch.cuda.synchronize()
    got = _host(dinv, n)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("%s: inverse diagonal, largest difference %.3g ulp, %d of %d bit-equal" % (dt, ulps.max(), int((got == want).sum()), n))
    assert ulps.max() <= 1.0
    assert (dinv.cpu().numpy()[n:] == SENTINEL).all()
    xs = _xs(n, rp, ci, vt, b)
    xm, itm, stm, relm = M.Mirror(A, dt, want).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
    assert stm == M.CONVERGED
    plan = _plan(n, rp, ci, vt, dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with api.CG(plan, dinv.data_ptr()) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=_stream(torch))
    err, errm = _relerr(_host(xd, n), xs), _relerr(xm, xs)
    print("%s: Jacobi-PCG %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    xd[:n].zero_()
    with api.CG(plan) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=_stream(torch))
    print("%s: plain CG on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
    assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi_follows_a_value_update(torch_cuda, dtype):
    """INTEGRATION.md §4e, Jacobi with a value map: the plan is created from the Laplacian with TILESPMV_CREATE_VALUE_MAP, the solver with a borrowed inverse diagonal; then the
    values become the scaled Laplacian's (tilespmv_plan_update_values) and the diagonal is taken again into the SAME array: the solver, untouched, now solves the new system."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, v1, b = _system("lap128", dt)
    v2 = _system("lap128_scaled", dt)[3]
    rpd, cid = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    v1d, v2d = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    plan = _plan(n, rp, ci, v1, dt, value_map=True)
    dinv, bd, xd = _vec(torch, None, n, dt), _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), v1d.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    with api.CG(plan, dinv.data_ptr()) as cg:
        for vt, vd in ((v1, v1d), (v2, v2d)):
            if vd is v2d:
                plan.update_values(vd.data_ptr(), stream)
                api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
            A = M.scipy_csr(n, rp, ci, vt)
            xm, itm, stm, relm = M.Mirror(A, dt, (dt.type(1) / A.diagonal().astype(dt)).astype(dt)).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
            xd[:n].zero_()
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
            xs = _xs(n, rp, ci, vt, b)
            err, errm = _relerr(_host(xd, n), xs), _relerr(xm, xs)
            print("%s: %d iterations (mirror %d), error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, err, errm))
            assert stm == M.CONVERGED and s["status"] == api.CG_CONVERGED and err <= 10 * errm
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_diagonal_with_a_duplicate_and_a_missing_entry(torch_cuda, dtype):
    """The header: duplicates added, 0 where no entry is stored; inverted: 1 where the sum is 0."""
    torch, dt = torch_cuda, np.dtype(dtype)
    rp = np.array([0, 3, 4, 6, 6], dtype=np.int32)                 # row 0: (0,0) twice; row 1: no diagonal; row 2: (2,2) + (2,3); row 3: empty
    ci = np.array([0, 1, 0, 3, 2, 3], dtype=np.int32)
    v = np.array([1.5, 7.0, 2.5, 9.0, -8.0, 3.0], dtype=dt)
    rpd, cid, vd = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    for invert, want in ((False, [4.0, 0.0, -8.0, 0.0]), (True, [0.25, 1.0, -0.125, 1.0])):
        out = _vec(torch, None, 4, dt)
        api.csr_diagonal_device(4, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), out.data_ptr(), invert=invert, stream=_stream(torch), dtype=dt)
        torch.cuda.synchronize()
        assert np.array_equal(_host(out, 4), np.array(want, dtype=dt)), (invert, _host(out, 4))
        assert (out.cpu().numpy()[4:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two solves on one plan and one on a second plan of the same matrix: bit-identical x, equal iteration counts and residuals."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("fem12", dt)
    bd = _vec(torch, b, n, dt)
    results = []
    plan = _plan(n, rp, ci, vt, dt)
    plan2 = _plan(n, rp, ci, vt, dt)
    for p in (plan, plan, plan2):
        xd = _vec(torch, None, n, dt)
        with api.CG(p) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=_stream(torch))
        assert s["status"] == api.CG_CONVERGED
        results.append((_host(xd, n), s["iterations"], s["rr"]))
    for x, it, rr in results[1:]:
        assert np.array_equal(x, results[0][0]) and it == results[0][1] and rr == results[0][2]
    plan.close(); plan2.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_iterate_is_capturable_into_a_hip_graph(torch_cuda, dtype):
    """iterate(8) captured with torch's graph API on a side stream as tests/test_gpu_parity.py captures the product (one linear chain), replayed, and compared bit for bit with
    uncaptured iterations from the same begin; a second replay continues the solve."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("lap128", dt)
    plan = _plan(n, rp, ci, vt, dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    cg = api.CG(plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        st = side.cuda_stream
        cg.begin(bd.data_ptr(), xd.data_ptr(), st)
        cg.iterate(xd.data_ptr(), 8, st)                      # (uncaptured: the comparison, and the warm-up)
        s8 = cg.state(st); x8 = _host(xd, n)
        cg.iterate(xd.data_ptr(), 8, st)
        s16 = cg.state(st); x16 = _host(xd, n)
        xd[:n].zero_()
        cg.begin(bd.data_ptr(), xd.data_ptr(), st)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cg.iterate(xd.data_ptr(), 8, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not _host(xd, n).any()                             # (captured, not run)
    for want_x, want_s in ((x8, s8), (x16, s16)):
        graph.replay(); torch.cuda.synchronize()
        s = cg.state(_stream(torch))
        assert np.array_equal(_host(xd, n), want_x)
        assert s["iterations"] == want_s["iterations"] and s["rr"] == want_s["rr"] and s["status"] == api.CG_RUNNING
    del graph
    cg.close(); plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """rho = 0 exactly (b = 0; A = 2 I after one iteration) stops the changes, p.Ap < 0 (a negative definite matrix) raises the breakdown flag and leaves x alone: ordinary
    data-dependent branches."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    # b = 0, x = 0
    n, rp, ci, vt, b = _system("lap128", dt)
    plan = _plan(n, rp, ci, vt, dt)
    zero, xd = _vec(torch, None, n, dt), _vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        s = cg.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
        assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not _host(xd, n).any()
        cg.begin(zero.data_ptr(), xd.data_ptr(), stream)
        cg.iterate(xd.data_ptr(), 16, stream)
        s = cg.state(stream)
        x = _host(xd, n)
        assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED
        assert np.isfinite(x).all() and not x.any()
    # A = -(the Laplacian): p.Ap < 0 in the first iteration
    x0 = M.rhs(n)[::-1].astype(dt)
    neg = _plan(n, rp, ci, -vt, dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
    with api.CG(neg) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
        assert np.array_equal(_host(xd, n), x0)
    neg.close(); plan.close()
    # A = 2 I: one iteration gives r = 0 exactly (alpha = 1/2 is exact)
    n = 4096
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dt)
    b = M.rhs(n).astype(dt)
    plan = _plan(n, rp, ci, v, dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
        cg.iterate(xd.data_ptr(), 1, stream)
        s = cg.state(stream)
        x1 = _host(xd, n)
        assert s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
        cg.iterate(xd.data_ptr(), 16, stream)
        s = cg.state(stream)
        assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(_host(xd, n), x1)
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_and_non_square_plans_are_refused(torch_cuda, dtype):
    dt = np.dtype(dtype)
    lib = _lib.load(dt)
    n, rp, ci, vt, b = _system("lap128", dt)
    shard = _plan(n, rp, ci, vt, dt, tilerow_end=(n // 16) // 2)
    m, nc, brp, bci = G.band(2048, 40, ncols=4096)
    wide = api.Plan.from_csr(m, nc, len(bci), brp, bci, G.real_values(len(bci), dt), dtype=dt, deterministic=1, placement_tries=1)
    for plan in (shard, wide):
        h = C.c_void_p(1)
        assert lib.tilespmv_cg_create(C.byref(h), plan.h, None) == api.HIP_ERROR_INVALID_VALUE and not h
        with pytest.raises(ValueError):
            api.CG(plan)
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("jacobi", [False, True])
def test_nothing_is_written_past_the_end(torch_cuda, jacobi, dtype):
    """x, b (and dinv) with 16 sentinel elements behind them, on a row count that is a multiple of 16 and on one that leaves a partial 16-byte vector at the end (2067 rows):
    the sentinels survive a solve, and the odd-sized solve is right."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    for label, (m, n, rp, ci) in (("fem12", G.fem_hex(12, 12, 12, 3)), ("tri53x39", G.tri_mesh(53, 39))):
        assert m == n and (label == "fem12" or n % 4 == 3)
        rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
        vt, b = M.spd_values(n, rp, ci).astype(dt), M.rhs(n).astype(dt)
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = (dt.type(1) / A.diagonal().astype(dt)).astype(dt) if jacobi else None
        plan = _plan(n, rp, ci, vt, dt)
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        dd = _vec(torch, dinv, n, dt) if jacobi else None
        m3 = M.Mirror(A, dt, dinv); m3.begin(b); m3.iterate(3)
        with api.CG(plan, dd.data_ptr() if jacobi else None) as cg:
            cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
            cg.iterate(xd.data_ptr(), 3, stream)
            s = cg.state(stream)
            x3 = _host(xd, n)
            dx = float(np.linalg.norm(x3.astype(np.float64) - m3.x.astype(np.float64)) / np.linalg.norm(m3.x.astype(np.float64)))
            print("%s %s jacobi=%s: 3 iterations, |x - mirror| / |mirror| = %.3g, rr %.6g (mirror %.6g)" % (label, dt, jacobi, dx, s["rr"], m3.rr))
            assert dx <= 100 * PRODUCT_TOL[dt] and abs(s["rr"] - m3.rr) <= 100 * PRODUCT_TOL[dt] * m3.rr
            xd[:n].zero_()
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
        assert s["status"] == api.CG_CONVERGED
        xs = _xs(n, rp, ci, vt, b)
        assert _relerr(_host(xd, n), xs) <= 100 * M.RTOL[dt]      # (degree + 1 on the diagonal: Gershgorin puts the condition number below 50)
        for t in (bd, xd) + ((dd,) if jacobi else ()):
            assert (t.cpu().numpy()[n:] == SENTINEL).all(), label
        assert np.array_equal(_host(bd, n), b)
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_operator_cg_is_the_library_solver(torch_cuda, dtype):
    from tilespmv_amd.operator import SparseOperator
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("fem12", dt)
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, deterministic=1, placement_tries=1) as op:
        x, info = op.cg(bd, rtol=M.RTOL[dt], maxiter=500)
        xd = _vec(torch, None, n, dt)
        with api.CG(op.A) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=_stream(torch))
        assert info["converged"] and info["status"] == "converged" and info["iterations"] == s["iterations"] and info["relative_residual"] <= M.RTOL[dt]
        assert np.array_equal(x.cpu().numpy(), _host(xd, n))
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = torch.from_numpy((dt.type(1) / A.diagonal().astype(dt)).astype(dt)).cuda()
        xj, infoj = op.cg(bd, rtol=M.RTOL[dt], maxiter=500, dinv=dinv)
        assert infoj["converged"] and infoj["iterations"] <= info["iterations"]
        xs = _xs(n, rp, ci, vt, b)
        assert _relerr(xj.cpu().numpy(), xs) <= 100 * M.RTOL[dt]      # (diagonally dominant, condition number below 50: the error stays within two decades of the residual)
        # a transposed plan qualifies when square (of a symmetric matrix it multiplies by A itself)
        xd[:n].zero_()
        with api.CG(op.AT) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=_stream(torch))
        assert s["status"] == api.CG_CONVERGED and _relerr(_host(xd, n), xs) <= 100 * M.RTOL[dt]
