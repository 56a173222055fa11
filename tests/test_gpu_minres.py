"""The MINRES solver in the library on the GPU (tilespmv_minres_*, tilespmv_csr_abs_diagonal_device; include/tilespmv.h) against its numpy mirror
(tests/minres_mirror.py, itself checked by tests/test_minres_cpu.py) and scipy's direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless a
test says otherwise; sixteen sentinel elements stand behind every caller vector.

The GPU is compared with the mirror iterate for iterate only after 1 and 3 iterations, within 100 x the per-product tolerance (the bound of the sibling files; two summation orders
of the fp64 mirror differ by <= 3e-15 there).  The library multiplies A z by the rounded 1 / beta where the mirror multiplies A by the rounded v = z / beta: one rounding per element
apart.  Further on, a solve is judged by its end: status, residual, error against spsolve."""
import ctypes as C

import numpy as np
import pytest

import minres_mirror as M
import solver_sizes as Z
from tilespmv_amd import _lib, api
from tilespmv_amd.operator import SparseOperator, minres as torch_minres

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


def _intact(*tensors_and_lengths):
    for t, n in tensors_and_lengths:
        assert (t.cpu().numpy()[n:] == SENTINEL).all(), "a sentinel behind a caller vector was overwritten"


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _minv_of(name, n, rp, ci, vt, dt):
    return M.inverse_abs_diagonal(n, rp, ci, vt, dt) if name.endswith("_scaled") else None


def _solved(name, dtype, rhs="rhs"):
    """The mirror's solve of a named input and the direct solution, computed once per value type: (xs, mirror iterations, mirror error).  minv = 1 / |diag| on the scaled input."""
    dt = np.dtype(dtype)
    if (name, dt, rhs) not in _CACHE:
        n, rp, ci, vt, b = _system(name, dt)
        if rhs == "zero_block":
            b = M.zero_block_rhs(n).astype(dt)
        minv = _minv_of(name, n, rp, ci, vt, dt)
        xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt, minv).solve(b, rtol=M.RTOL[dt], maxiter=5000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[(name, dt, rhs)] = (xs, itm, _relerr(xm, xs))
    return _CACHE[(name, dt, rhs)]


def _relerr(x, xs):
    xs = np.asarray(xs, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(x, dtype=np.float64) - xs) / np.linalg.norm(xs))


def _dist(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _device_csr(torch, rp, ci, v):
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()


def _early(torch, dt, A, b, plan, minv, n, label, x0=None):
    """x, rr and bb after begin, 1 and 3 iterations against the mirror of A.  Bound: 100 x the per-product tolerance; a wrong sign, a stale scalar, a swapped vector or a wrong
    parity of the history is an O(1) difference."""
    m = M.Mirror(A, dt, minv)
    m.begin(b, x0)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
    dd = None if minv is None else _vec(torch, minv, n, dt)
    with api.MINRES(plan, None if dd is None else dd.data_ptr()) as ms:
        ms.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
        s0 = ms.state(_stream(torch))
        print("%s %s begin: rr %.3g bb %.3g" % (label, dt, _dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(_dist(s0["rr"], m.rr), _dist(s0["bb"], m.bb)) <= bound
        done = 0
        for step in (1, 2):
            ms.iterate(xd.data_ptr(), step, _stream(torch)); m.iterate(step); done += step
            s = ms.state(_stream(torch))
            dx = _relerr(_host(xd, n), m.x)
            drr, dbb = _dist(s["rr"], m.rr), _dist(s["bb"], m.bb)
            print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g, bb %.3g (bound %.3g)" % (label, dt, done, dx, drr, dbb, bound))
            assert s["iterations"] == done == m.iterations and s["status"] == api.CG_RUNNING == m.status()
            assert dx <= bound and drr <= bound and dbb <= bound
    assert np.array_equal(_host(bd, n), b)
    _intact((bd, n), (xd, n), *(((dd, n),) if dd is not None else ()))
    return bd, xd, dd


# ---- early iterations
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["saddle47", "saddlec47_scaled"])
def test_early_iterations_equal_the_mirror(torch_cuda, name, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    with _op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt), b, op.A, _minv_of(name, n, rp, ci, vt, dt), n, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_on_the_transposed_plan(torch_cuda, dtype):
    """api.MINRES(op.AT): a square transposed plan qualifies; K^T = K, so three iterations equal the mirror of K."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("saddle47", dt)
    with _op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt).T.tocsr(), b, op.AT, None, n, "saddle47^T")


# ---- solves
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [{}, dict(deterministic=-1, placement_tries=-1)])
def test_solves(torch_cuda, kw, dtype):
    """tilespmv_minres_solve on saddle47 with maxiter = 2 x the mirror's count: CONVERGED, sqrt(rr / bb) <= rtol, and an error against spsolve within 10 x the mirror's own.
    The second case is the builder's default (timed) plans, whatever form they pick."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("saddle47", dt)
    xs, itm, errm = _solved("saddle47", dt)
    with _op(n, rp, ci, vt, dt, **kw) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=_stream(torch))
        x = _host(xd, n)
    err = _relerr(x, xs)
    print("saddle47 %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error %.3g (mirror %.3g)" % (dt, kw, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    _intact((bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_preconditioner(torch_cuda, dtype):
    """saddlec47_scaled: minv from tilespmv_csr_abs_diagonal_device(invert) equals numpy's 1 / |diag| bit for bit; preconditioned MINRES converges within 2 x the mirror's count to
    an error within 10 x the mirror's; the plain solver on the same plan is at MAXITER at that cap."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, vt, b = _system("saddlec47_scaled", dt)
    xs, itm, errm = _solved("saddlec47_scaled", dt)
    rpd, cid, vd = _device_csr(torch, rp, ci, vt)
    minv = _vec(torch, None, n, dt)
    api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), minv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    want = M.inverse_abs_diagonal(n, rp, ci, vt, dt)
    assert np.array_equal(_host(minv, n), want) and (want > 0).all()
    plain = _vec(torch, None, n, dt)      # (invert = 0: |d| itself; 552 of the signed diagonal entries are negative)
    api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), plain.data_ptr(), invert=False, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    diag = M.scipy_csr(n, rp, ci, vt).diagonal()
    assert np.array_equal(_host(plain, n), np.abs(diag)) and (diag < 0).sum() == 552
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.MINRES(op.A, minv.data_ptr()) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err = _relerr(_host(xd, n), xs)
        print("%s: preconditioned MINRES %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:n].zero_()
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain MINRES on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    _intact((minv, n), (plain, n), (bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_breaks_down_and_minres_solves_it(torch_cuda, dtype):
    """saddle47 with b on the zero block: p.Ap = b.K b = 0 exactly in CG's first iteration — api.CG reports BREAKDOWN with x untouched; api.MINRES on the same plan converges."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, vt, _ = _system("saddle47", dt)
    b = M.zero_block_rhs(n).astype(dt)
    xs, itm, errm = _solved("saddle47", dt, "zero_block")
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.CG(op.A) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        assert s["status"] == api.CG_BREAKDOWN and not _host(xd, n).any(), s
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        err = _relerr(_host(xd, n), xs)
        print("%s: MINRES %d iterations (mirror %d), error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and err <= 10 * errm
    _intact((bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_residual_never_increases(torch_cuda, dtype):
    """40 single iterations on saddle47, rr read after each."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, vt, b = _system("saddle47", dt)
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.MINRES(op.A) as ms:
            ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
            rr = [ms.state(stream)["rr"]]
            for _ in range(40):
                ms.iterate(xd.data_ptr(), 1, stream)
                rr.append(ms.state(stream)["rr"])
    print("%s: rr from %.6g to %.6g over 40 iterations" % (dt, rr[0], rr[-1]))
    assert all(a >= c for a, c in zip(rr, rr[1:])) and rr[-1] < 0.5 * rr[0] and rr[-1] > 0


# ---- guards
@pytest.mark.parametrize("dtype", DTYPES)
def test_guards(torch_cuda, dtype):
    """phibar = 0 exactly (b = 0; pow2I after one iteration: the lucky termination) stops the changes; gamma = 0 exactly (singular) and a negative minv raise the breakdown flag and
    leave x alone."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    # b = 0
    n, rp, ci, vt, b = _system("saddle47", dt)
    with _op(n, rp, ci, vt, dt) as op:
        zero, xd = _vec(torch, None, n, dt), _vec(torch, b, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not _host(xd, n).any()
            ms.begin(zero.data_ptr(), xd.data_ptr(), stream)
            ms.iterate(xd.data_ptr(), 16, stream)
            s = ms.state(stream)
            x = _host(xd, n)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
        _intact((zero, n), (xd, n))
    # pow2I: bb = 262144, beta = 512, alfa = 2, y' = 0, beta' = 0, gamma = 2: x = 4 and rr = 0 after one iteration, exact in both value types
    n, rp, ci, v = M.problem("pow2I")
    with _op(n, rp, ci, v, dt) as op:
        bd, xd = _vec(torch, np.full(n, 8.0), n, dt), _vec(torch, None, n, dt)
        with api.MINRES(op.A) as ms:
            ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
            s = ms.state(stream)
            assert s["bb"] == 262144.0 and s["rr"] == 262144.0 and s["status"] == api.CG_RUNNING
            ms.iterate(xd.data_ptr(), 1, stream)
            s = ms.state(stream)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and s["bb"] == 262144.0 and s["status"] == api.CG_CONVERGED and np.array_equal(_host(xd, n), np.full(n, 4.0, dtype=dt))
            ms.iterate(xd.data_ptr(), 16, stream)
            s = ms.state(stream)
            assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(_host(xd, n), np.full(n, 4.0, dtype=dt))
        # minv = -1: r2.z < 0 in begin
        x0 = M.rhs(n).astype(dt)
        neg, xd = _vec(torch, -np.ones(n), n, dt), _vec(torch, x0, n, dt)
        with api.MINRES(op.A, neg.data_ptr()) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 0 and np.array_equal(_host(xd, n), x0)
            ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
            ms.iterate(xd.data_ptr(), 5, stream)
            s = ms.state(stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 5 and np.array_equal(_host(xd, n), x0)
        _intact((bd, n), (xd, n), (neg, n))
    # singular: A b = 0 exactly: alfa = 0, y' = 0, beta' = 0, gamma = 0 in the first iteration
    n, rp, ci, v = M.problem("singular")
    b, x0 = M.singular_rhs(n).astype(dt), np.zeros(n, dtype=dt)
    with _op(n, rp, ci, v, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(_host(xd, n), x0) and s["rr"] == 2049.0
        _intact((bd, n), (xd, n))


# ---- reproducibility, graphs, value refresh
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two solvers on two separately created deterministic operators, preconditioned: bit-identical x and rr after 20 iterations."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("saddlec47_scaled", dt)
    minv = _vec(torch, M.inverse_abs_diagonal(n, rp, ci, vt, dt), n, dt)
    bd = _vec(torch, b, n, dt)
    results = []
    for _ in range(2):
        with _op(n, rp, ci, vt, dt) as op:
            xd = _vec(torch, None, n, dt)
            with api.MINRES(op.A, minv.data_ptr()) as ms:
                ms.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
                ms.iterate(xd.data_ptr(), 20, _stream(torch))
                s = ms.state(_stream(torch))
            results.append((_host(xd, n), s))
    (xa, sa), (xb, sb) = results
    assert sa["iterations"] == 20 and sa["status"] == api.CG_RUNNING and np.array_equal(xa, xb) and sa["rr"] == sb["rr"] and xa.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, dtype):
    """Captured with torch's graph API on a side stream (one linear chain, as tests/test_gpu_bicgstab.py captures them).
    (a) begin + iterate(8), replayed twice from the same x0: each replay equals the eager run bit for bit.
    (b) begin eager, then a captured iterate(3) ALONE replayed twice: equal to an eager begin + iterate(6) bit for bit.  An odd count, so the second replay starts with the roles
    of the two history buffers exchanged: a history rotated by pointers on the host would be frozen into the graph and fail here."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("saddlec47_scaled", dt)
    x0 = (0.01 * M.rhs(n)[::-1]).astype(dt)
    with _op(n, rp, ci, vt, dt) as op:
        bd, xd = _vec(torch, b, n, dt), _vec(torch, x0, n, dt)
        minv = _vec(torch, M.inverse_abs_diagonal(n, rp, ci, vt, dt), n, dt)
        ms = api.MINRES(op.A, minv.data_ptr())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph, graph3 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = side.cuda_stream
            ms.begin(bd.data_ptr(), xd.data_ptr(), st)
            ms.iterate(xd.data_ptr(), 6, st)                      # (uncaptured: the comparisons, and the warm-up)
            s6 = ms.state(st); x6 = _host(xd, n)
            ms.iterate(xd.data_ptr(), 2, st)
            s8 = ms.state(st); x8 = _host(xd, n)
            xd[:n].copy_(torch.from_numpy(x0))
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                ms.begin(bd.data_ptr(), xd.data_ptr(), st)
                ms.iterate(xd.data_ptr(), 8, st)
            with torch.cuda.graph(graph3, stream=side):
                ms.iterate(xd.data_ptr(), 3, st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert np.array_equal(_host(xd, n), x0)                   # (captured, not run)
        for _ in range(2):                                        # (a)
            xd[:n].copy_(torch.from_numpy(x0))
            torch.cuda.synchronize()
            graph.replay(); torch.cuda.synchronize()
            s = ms.state(_stream(torch))
            assert np.array_equal(_host(xd, n), x8) and not np.array_equal(x8, x0)
            assert s["iterations"] == 8 and s["rr"] == s8["rr"] and s["status"] == api.CG_RUNNING
        xd[:n].copy_(torch.from_numpy(x0))                        # (b)
        ms.begin(bd.data_ptr(), xd.data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        graph3.replay(); torch.cuda.synchronize()
        assert ms.state(_stream(torch))["iterations"] == 3
        graph3.replay(); torch.cuda.synchronize()
        s = ms.state(_stream(torch))
        assert s["iterations"] == 6 and s["rr"] == s6["rr"] and np.array_equal(_host(xd, n), x6) and not np.array_equal(x6, x8)
        del graph, graph3
        ms.close()
    _intact((bd, n), (xd, n), (minv, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """an operator with a value map solves with saddlec47's values; update_values to saddlec47_scaled's (the same pattern), minv recomputed into the SAME array,
    then a warm-started solve.  The result equals, bit for bit on these deterministic plans, that of an operator built fresh from the new values and started from the same x."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n, rp, ci, v1, b = _system("saddlec47", dt)
    v2 = _system("saddlec47_scaled", dt)[3]
    xs, itm, errm = _solved("saddlec47_scaled", dt)
    rpd, cid, v1d = _device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    minv, bd, xd = _vec(torch, None, n, dt), _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with _op(n, rp, ci, v1, dt, value_map=True) as op:
        api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), v1d.data_ptr(), minv.data_ptr(), invert=True, stream=stream, dtype=dt)
        with api.MINRES(op.A, minv.data_ptr()) as ms:
            s1 = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=1000, stream=stream)
            assert s1["status"] == api.CG_CONVERGED
            x1 = _host(xd, n)
            op.update_values(v2d.data_ptr(), stream)
            api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), v2d.data_ptr(), minv.data_ptr(), invert=True, stream=stream, dtype=dt)
            s2 = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=1000, stream=stream)      # (warm: x holds the first solution)
            x2 = _host(xd, n)
    with _op(n, rp, ci, v2, dt, value_map=True) as fresh:
        xf = _vec(torch, x1, n, dt)
        with api.MINRES(fresh.A, minv.data_ptr()) as ms:
            sf = ms.solve(bd.data_ptr(), xf.data_ptr(), rtol=M.RTOL[dt], maxiter=1000, stream=stream)
    print("%s: first %d iterations, refreshed %d, fresh %d; error vs spsolve %.3g" % (dt, s1["iterations"], s2["iterations"], sf["iterations"], _relerr(x2, xs)))
    assert s2["status"] == api.CG_CONVERGED and sf["status"] == api.CG_CONVERGED
    assert s2["iterations"] == sf["iterations"] and s2["rr"] == sf["rr"] and np.array_equal(x2, _host(xf, n))
    assert _relerr(x2, xs) <= 100 * M.RTOL[dt]
    _intact((minv, n), (bd, n), (xd, n), (xf, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """A non-square plan (a rectangular operator's A), a shard plan, a misaligned minv: hipErrorInvalidValue, no handle; api.MINRES raises ValueError.  An aligned minv is
    accepted."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    n, rp, ci, vt, b = _system("saddle47", dt)
    half = n // 2
    keep = ci[: rp[half]]
    with _op(n, rp, ci, vt, dt) as op, SparseOperator(half, n, rp[: half + 1].copy(), keep.copy(), vt[: rp[half]].copy(), dtype=dt, deterministic=1, placement_tries=1) as rect:
        shard = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1, tilerow_end=((n + 15) // 16) // 2)
        minv = _vec(torch, np.ones(n + 1), n + 1, dt)
        cases = (("non-square plan", rect.A, None), ("shard plan", shard, None), ("misaligned minv", op.A, minv.data_ptr() + dt.itemsize))
        for label, plan, d in cases:
            h = C.c_void_p(1)
            rc = lib.tilespmv_minres_create(C.byref(h), plan.h, C.c_void_p(d))
            print("%s %s: rc %d, handle %s" % (dt, label, rc, h.value))
            assert rc == api.HIP_ERROR_INVALID_VALUE and not h, label
            with pytest.raises(ValueError):
                api.MINRES(plan, d)
        with api.MINRES(op.A, minv.data_ptr()) as ms:      # (aligned: accepted)
            assert ms.h
        shard.close()


# ---- sizes: past the cap of 1024 partial sums, at 300 partials, below one lane vector (tests/solver_sizes.py)
@pytest.fixture(scope="module")
def built():
    """Plans shared by the size tests: key -> (plan, host data), closed at the end."""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    yield get
    for plan, _ in cache.values():
        plan.close()


def _square(built, kind, n, dt):
    def make():
        _, rp, ci, v = (M.indefinite_tridiagonal if kind == "indefinite" else Z.two_identity)(n)
        vt = np.ascontiguousarray(v, dtype=dt)
        return api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1), (n, rp, ci, vt)
    return built((kind, n, np.dtype(dt).name), make)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_identity_at_the_capped_size(torch_cuda, built, dtype):
    """A = 2 I at the capped n, b in the nonzero integers of [-30, 30]: begin gives bb == rr == the integer sum of the squares, exactly (every partial sum is an integer below
    2^53 in any order).  One iteration gives x = b / 2 up to the roundings of 1/beta, v, 1/gamma, w, phi and x: within 4 ulp in every element."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = _stream(torch)
    n = Z.capped_n(dt)
    plan, _ = _square(built, "2I", n, dt)
    b64 = Z.exact_rhs(n)
    bb = Z.exact_bb(b64)
    b, half = b64.astype(dt), (b64 / 2).astype(dt)
    bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
    with api.MINRES(plan) as ms:
        ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
        s0 = ms.state(stream)
        assert s0["bb"] == bb and s0["rr"] == bb and s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING, (s0, bb)
        ms.iterate(xd.data_ptr(), 1, stream)
        s1 = ms.state(stream)
        x1 = _host(xd, n)
    ulps = np.abs(x1.astype(np.float64) - half.astype(np.float64)) / np.spacing(np.abs(half)).astype(np.float64)
    print("%s: n = %d, largest distance of x from b / 2: %.3g ulp at element %d; rr after one iteration %.3g of bb" % (dt, n, ulps.max(), int(ulps.argmax()), s1["rr"] / bb))
    assert s1["iterations"] == 1 and s1["bb"] == bb and s1["status"] in (api.CG_RUNNING, api.CG_CONVERGED)
    assert ulps.max() <= 4
    assert np.array_equal(_host(bd, n), b)
    _intact((bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["capped", "fold2"])
def test_the_sizes_equal_the_mirror(torch_cuda, built, case, dtype):
    """indefinite_tridiagonal at n = 1 052 249 / 2 104 499 (two sweeps of every streaming kernel, a partial last trip, the longest scalar tail) and 307 201 / 614 403 (300
    partials: a fold in two passes), minv = a positive diagonal that varies with the row, from x0 != 0: begin, 1 and 3 iterations against the mirror."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n = Z.single_n(case, dt)
    plan, (_, rp, ci, vt) = _square(built, "indefinite", n, dt)
    b, x0 = M.rhs(n).astype(dt), (0.25 * M.rhs(n)[::-1]).astype(dt)
    minv = Z.diagonal_preconditioner(n).astype(dt)
    bd, xd, dd = _early(torch, dt, M.scipy_csr(n, rp, ci, vt), b, plan, minv, n, "indefinite tridiagonal %s" % case, x0=x0)
    assert np.array_equal(_host(dd, n), minv)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_systems(torch_cuda, dtype):
    """n in {1, 2, 3, 5}: with n < 2 (fp64) / n < 4 (fp32) there is no lane vector at all and thread 0 of workgroup 0 owns every element.  Solved to the mirror's rtol; the error
    against numpy's dense float64 solution within 10 x the mirror's own (counted as at least one unit roundoff: tests/test_gpu_solver_sizes.py::_yardstick)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    floor = float(np.finfo(dt).eps) / 2
    for n in Z.TINY_N:
        _, rp, ci, v = M.indefinite_tridiagonal(n)
        vt, b = v.astype(dt), M.rhs(n).astype(dt)
        A = M.scipy_csr(n, rp, ci, vt)
        xs = np.linalg.solve(A.toarray().astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=50, check_every=1)
        assert stm == M.CONVERGED
        plan = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1)
        bd, xd = _vec(torch, b, n, dt), _vec(torch, None, n, dt)
        with api.MINRES(plan) as ms:
            st = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm + 2, check_every=1, stream=_stream(torch))
        err, errm = _relerr(_host(xd, n), xs), _relerr(xm, xs)
        print("n = %d %s: %d iterations (mirror %d), error against the dense float64 solution %.3g (mirror %.3g)" % (n, dt, st["iterations"], itm, err, errm))
        assert st["status"] == api.CG_CONVERGED and st["relative_residual"] <= M.RTOL[dt], (n, st)
        assert err <= 10 * max(errm, floor), (n, err, errm)
        assert np.array_equal(_host(bd, n), b)
        _intact((bd, n), (xd, n))
        plan.close()


# ---- the Python method and the torch loop
def test_sparse_operator_minres_agrees_with_the_torch_loop(torch_cuda):
    """saddle47 in fp64: the method and the module-level loop are both within 1e-8 of spsolve; the info keys are those of bicgstab; wrong length, dtype or shape raises."""
    torch = torch_cuda
    dt = np.dtype(np.float64)
    n, rp, ci, vt, b = _system("saddle47", dt)
    xs = _solved("saddle47", dt)[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, placement_tries=1) as op:
        x, info = op.minres(bd, rtol=1e-12, maxiter=2000)
        xt, infot = torch_minres(op, bd, tol=1e-12, maxiter=2000)
        print("library %s, torch loop %s" % (info, infot))
        assert info["converged"] and info["status"] == "converged" and infot["converged"], (info, infot)
        assert set(info) == {"iterations", "residual", "relative_residual", "converged", "status"}
        for got in (x.cpu().numpy(), xt.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs), (np.linalg.norm(got - xs), info, infot)
    n, rp, ci, vt, b = _system("saddlec47_scaled", dt)
    xs = _solved("saddlec47_scaled", dt)[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, placement_tries=1) as op:
        minv = torch.from_numpy(M.inverse_abs_diagonal(n, rp, ci, vt, dt)).cuda()
        xj, infoj = op.minres(bd, rtol=1e-12, maxiter=2000, minv=minv)
        xtj, infotj = torch_minres(op, bd, tol=1e-12, maxiter=2000, minv=minv)
        print("with minv: library %s, torch loop %s" % (infoj, infotj))
        assert infoj["converged"] and infotj["converged"]
        for got in (xj.cpu().numpy(), xtj.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs), (np.linalg.norm(got - xs), infoj, infotj)
        xw, infow = op.minres(bd, rtol=1e-12, maxiter=2000, minv=minv, x0=xj)      # (a warm start from the solution)
        assert infow["converged"] and infow["iterations"] < infoj["iterations"] and np.linalg.norm(xw.cpu().numpy() - xs) <= 1e-8 * np.linalg.norm(xs)
        for bad in (bd[:-1], bd.float(), bd.reshape(-1, 1)):
            with pytest.raises(ValueError):
                op.minres(bad)
        with pytest.raises(ValueError):
            op.minres(bd, minv=torch.ones(n + 1, dtype=bd.dtype, device="cuda"))
