"""The BiCGStab solver in the library on the GPU (tilespmv_bicgstab_*; include/tilespmv.h) against its numpy mirror (tests/bicgstab_mirror.py, itself checked by
tests/test_bicgstab_cpu.py) and scipy's direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless a test says otherwise.

The GPU is compared with the mirror iterate for iterate only after 1 and 3 iterations (measured there: ~2e-16 in fp64, ~8e-8 in fp32, relative, in x): BiCGStab amplifies
rounding differences quickly — two summation orders of the fp64 mirror itself differ by 2e-16 in x after 3 iterations and by 9e-13 after 20.  Further on, a solve is judged by its
end: status, residual, error against spsolve."""
import ctypes as C

import numpy as np
import pytest

import bicgstab_mirror as M
from tilespmv_amd import _lib, api, generators as G
from tilespmv_amd.operator import SparseOperator, bicgstab as torch_bicgstab

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
PRODUCT_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # README: the project's per-product tolerance on real-valued data
SENTINEL = 777.0
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _op(n, rp, ci, v, dtype, **kw):
    kw.setdefault("deterministic", 1)
    kw.setdefault("placement_tries", 1)
    return SparseOperator(n, n, rp, ci, np.ascontiguousarray(v, dtype=dtype), dtype=dtype, **kw)


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
        _CACHE[(name, dt)] = (xs, itm, _relerr(xm, xs))
    return _CACHE[(name, dt)]


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def _dist(a, b):
    return abs(a - b) / abs(b)


def _device_csr(torch, rp, ci, v):
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()


def _early(torch, dt, A, b, plan, dinv, n, label):
    """x and rr after 1 and after 3 iterations against the mirror of A.  Bound: 100 x the per-product tolerance (the bound of tests/test_gpu_cg.py and test_gpu_cgls.py: another
    summation order over a few iterations); a wrong sign, a stale scalar or a swapped vector is an O(1) difference."""
    m = M.Mirror(A, dt, dinv)
    m.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    dd = None if dinv is None else _vec(torch, dinv, n, dt)
    with api.BiCGStab(plan, None if dd is None else dd.data_ptr()) as bs:
        bs.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
        s0 = bs.state(_stream(torch))
        print("%s %s begin: rr %.3g bb %.3g" % (label, dt, _dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(_dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)) <= bound
        done = 0
        for step in (1, 2):
            bs.iterate(xd.data_ptr(), step, _stream(torch)); m.iterate(step); done += step
            s = bs.state(_stream(torch))
            dx = _relerr(_host(xd, n), m.x.astype(np.float64))
            drr = _dist(s["rr"], m.rr)
            print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)" % (label, dt, done, dx, drr, bound))
            assert s["iterations"] == done == m.iterations and s["status"] == api.CG_RUNNING == m.status()
            assert dx <= bound and drr <= bound
    return bd, xd, dd


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_equal_the_mirror(torch_cuda, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with _op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt), b, op.A, None, n, "convdiff67")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [{}, dict(deterministic=-1, placement_tries=-1)])
def test_solves(torch_cuda, kw, dtype):
    """tilespmv_bicgstab_solve on convdiff67 with maxiter = 2 x the mirror's count: CONVERGED, sqrt(rr / bb) <= rtol, and an error against spsolve within 10 x the mirror's own.
    The second case is the builder's default (timed) plans, whatever form they pick."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    xs, itm, errm = _solved("convdiff67", dt)
    with _op(n, rp, ci, vt, dt, **kw) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=_stream(torch))
        x = _host(xd, n)
    err = _relerr(x, xs)
    print("convdiff67 %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error %.3g (mirror %.3g)" % (dt, kw, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi(torch_cuda, dtype):
    """convdiff67_scaled: dinv from tilespmv_csr_diagonal_device(invert) equals numpy's; preconditioned BiCGStab converges within 2 x the mirror's count to an error within 10 x
    the mirror's; the plain solver on the same plan is still running at that cap."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, vt, b = _system("convdiff67_scaled", dt)
    xs, itm, errm = _solved("convdiff67_scaled", dt)
    rpd, cid, vd = _device_csr(torch, rp, ci, vt)
    dinv = _vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    assert np.array_equal(_host(dinv, n), M.inverse_diagonal(n, rp, ci, vt, dt))
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.BiCGStab(op.A, dinv.data_ptr()) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err = _relerr(_host(xd, n), xs)
        print("%s: Jacobi BiCGStab %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:n].zero_()
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain BiCGStab on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    assert (dinv.cpu().numpy()[n:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_transposed_plan_solves_the_transposed_system(torch_cuda, dtype):
    """api.BiCGStab(op.AT): three iterations equal the mirror of A^T."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with _op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt).T.tocsr(), b, op.AT, None, n, "convdiff67^T")


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """an operator with a value map solves with convdiff67's values; update_values to convdiff67_scaled's (the same pattern), the inverse diagonal recomputed
    into the SAME array, then a warm-started solve.  The result equals, bit for bit on these deterministic plans, that of an operator built fresh from the new values and started
    from the same x."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, v1, b = _system("convdiff67", dt)
    v2 = _system("convdiff67_scaled", dt)[3]
    xs, itm, errm = _solved("convdiff67_scaled", dt)
    rpd, cid, v1d = _device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    dinv, bd, xd = _vec(torch, None, n, dt), _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with _op(n, rp, ci, v1, dt, value_map=True) as op:
        api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), v1d.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
        with api.BiCGStab(op.A, dinv.data_ptr()) as bs:
            s1 = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
            assert s1["status"] == api.CG_CONVERGED
            x1 = _host(xd, n)
            op.update_values(v2d.data_ptr(), stream)
            api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), v2d.data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
            s2 = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)      # (warm: x holds the first solution)
            x2 = _host(xd, n)
    with _op(n, rp, ci, v2, dt, value_map=True) as fresh:
        xf = _vec(torch, x1, n, dt)
        with api.BiCGStab(fresh.A, dinv.data_ptr()) as bs:
            sf = bs.solve(bd.data_ptr(), xf.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
    print("%s: refreshed %d iterations, fresh %d; error vs spsolve %.3g" % (dt, s2["iterations"], sf["iterations"], _relerr(x2, xs)))
    assert s2["status"] == api.CG_CONVERGED and sf["status"] == api.CG_CONVERGED
    assert s2["iterations"] == sf["iterations"] and s2["rr"] == sf["rr"] and np.array_equal(x2, _host(xf, n))
    assert _relerr(x2, xs) <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two solvers on two separately created deterministic operators, Jacobi: bit-identical x and rr after 20 iterations."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67_scaled", dt)
    dinv = _vec(torch, M.inverse_diagonal(n, rp, ci, vt, dt), n, dt)
    bd = _vec(torch, b, n, dt)
    results = []
    for _ in range(2):
        with _op(n, rp, ci, vt, dt) as op:
            xd = _vec(torch, None, n, dt)
            with api.BiCGStab(op.A, dinv.data_ptr()) as bs:
                bs.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
                bs.iterate(xd.data_ptr(), 20, _stream(torch))
                s = bs.state(_stream(torch))
            results.append((_host(xd, n), s))
    (xa, sa), (xb, sb) = results
    assert sa["iterations"] == 20 and sa["status"] == api.CG_RUNNING and np.array_equal(xa, xb) and sa["rr"] == sb["rr"] and xa.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, dtype):
    """begin + iterate(8) captured with torch's graph API on a side stream (one linear chain, as tests/test_gpu_cgls.py captures them) and replayed twice from the same x0:
    each replay equals the eager run bit for bit."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    x0 = (0.01 * M.rhs(n)[::-1]).astype(dt)
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
        dinv = _vec(torch, M.inverse_diagonal(n, rp, ci, vt, dt), n, dt)
        bs = api.BiCGStab(op.A, dinv.data_ptr())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = side.cuda_stream
            bs.begin(bd.data_ptr(), xd.data_ptr(), st)
            bs.iterate(xd.data_ptr(), 8, st)                      # (uncaptured: the comparison, and the warm-up)
            s8 = bs.state(st); x8 = _host(xd, n)
            xd[:n].copy_(torch.from_numpy(x0))
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                bs.begin(bd.data_ptr(), xd.data_ptr(), st)
                bs.iterate(xd.data_ptr(), 8, st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert np.array_equal(_host(xd, n), x0)                   # (captured, not run)
        for _ in range(2):
            xd[:n].copy_(torch.from_numpy(x0))
            torch.cuda.synchronize()
            graph.replay(); torch.cuda.synchronize()
            s = bs.state(_stream(torch))
            assert np.array_equal(_host(xd, n), x8) and not np.array_equal(x8, x0)
            assert s["iterations"] == 8 and s["rr"] == s8["rr"] and s["status"] == api.CG_RUNNING
        del graph
        bs.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """rr = 0 exactly (b = 0; A = 2 I after one iteration, at the half step) stops the changes; sigma = 0 exactly (skew) raises the breakdown flag and leaves x alone."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    # b = 0
    n, rp, ci, vt, b = _system("convdiff67", dt)
    with _op(n, rp, ci, vt, dt) as op:
        zero, xd = _vec(torch, None, n, dt), _vec(torch, b, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not _host(xd, n).any()
            bs.begin(zero.data_ptr(), xd.data_ptr(), stream)
            bs.iterate(xd.data_ptr(), 16, stream)
            s = bs.state(stream)
            x = _host(xd, n)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
    # A = 2 I: alpha = 1/2 exactly, s = 0, t.t = 0 -> omega = 0: converged at the half step
    n, rp, ci, v = M.problem("2I")
    b = M.rhs(n).astype(dt)
    with _op(n, rp, ci, v, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.BiCGStab(op.A) as bs:
            bs.begin(bd.data_ptr(), xd.data_ptr(), stream)
            bs.iterate(xd.data_ptr(), 1, stream)
            s = bs.state(stream)
            x1 = _host(xd, n)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and np.array_equal(x1, b / dt.type(2))
            bs.iterate(xd.data_ptr(), 16, stream)
            s = bs.state(stream)
            assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(_host(xd, n), x1)
    # skew: rhat.v = b.A b = 0 exactly in the first iteration
    n, rp, ci, v = M.problem("skew")
    b, x0 = M.skew_rhs(n).astype(dt), np.zeros(n, dtype=dt)
    with _op(n, rp, ci, v, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
        with api.BiCGStab(op.A) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(_host(xd, n), x0) and s["rr"] == float(b.astype(np.float64) @ b.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """A non-square plan (a rectangular operator's A), a shard plan, a misaligned dinv: hipErrorInvalidValue, no handle; api.BiCGStab raises ValueError.  An aligned dinv is
    accepted."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    n, rp, ci, vt, b = _system("convdiff67", dt)
    half = n // 2
    keep = ci[: rp[half]]
    with _op(n, rp, ci, vt, dt) as op, SparseOperator(half, n, rp[: half + 1].copy(), keep.copy(), vt[: rp[half]].copy(), dtype=dt, deterministic=1, placement_tries=1) as rect:
        shard = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, tilerow_end=((n + 15) // 16) // 2)
        dinv = _vec(torch, np.ones(n + 1), n + 1, dt)
        cases = (("non-square plan", rect.A, None), ("shard plan", shard, None), ("misaligned dinv", op.A, dinv.data_ptr() + dt.itemsize))
        for label, plan, d in cases:
            h = C.c_void_p(1)
            rc = lib.tilespmv_bicgstab_create(C.byref(h), plan.h, C.c_void_p(d))
            print("%s %s: rc %d, handle %s" % (dt, label, rc, h.value))
            assert rc == api.HIP_ERROR_INVALID_VALUE and not h, label
            with pytest.raises(ValueError):
                api.BiCGStab(plan, d)
        with api.BiCGStab(op.A, dinv.data_ptr()) as bs:      # (aligned: accepted)
            assert bs.h
        shard.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_is_touched_past_the_end(torch_cuda, dtype):
    """5003 rows (3 mod 4: a scalar tail in both value types), 5 random off-diagonal entries per row in (-1, 1) and a diagonal of 8: three Jacobi iterations equal the mirror's;
    b, x and dinv with 16 sentinel elements behind them survive a Jacobi solve, b and dinv unchanged."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n = 5003
    rng = np.random.default_rng(29)
    r, c = np.repeat(np.arange(n), 5), rng.integers(0, n, n * 5)
    off = r != c
    _, _, rp, ci = G.from_coo(n, n, np.concatenate([r[off], np.arange(n)]), np.concatenate([c[off], np.arange(n)]))
    rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
    rows = np.repeat(np.arange(n), np.diff(rp))
    vt = np.where(ci == rows, 8.0, rng.uniform(-1, 1, len(ci))).astype(dt)
    A = M.scipy_csr(n, rp, ci, vt)
    b, dinv = M.rhs(n).astype(dt), M.inverse_diagonal(n, rp, ci, vt, dt)
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd, dd = _early(torch, dt, A, b, op.A, dinv, n, "5003 rows")
        xd[:n].zero_()
        with api.BiCGStab(op.A, dd.data_ptr()) as bs:
            s = bs.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=200, stream=stream)
        assert s["status"] == api.CG_CONVERGED
        assert _relerr(_host(xd, n), M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))) <= 100 * M.RTOL[dt]
        for t in (bd, xd, dd):
            assert (t.cpu().numpy()[n:] == SENTINEL).all()
        assert np.array_equal(_host(bd, n), b) and np.array_equal(_host(dd, n), dinv)


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
