"""The multi-right-hand-side solver on the GPU (tilespmv_cg_multi_*; include/tilespmv.h): per column against the numpy mirror of the single solver
(tests/cg_mirror.py) and scipy's direct solution, on the eight right-hand sides of tests/cg_multi_cases.py (checked by tests/test_cg_multi_cpu.py).  Plans are created with
deterministic=1, placement_tries=1 through Plan.from_csr unless a test says otherwise.  All bounds are those of tests/test_gpu_cg.py: PRODUCT_TOL and M.RTOL."""
import ctypes as C

import numpy as np
import pytest

import cg_mirror as M
import cg_multi_cases as MC
import gpu_solver_util as U
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api, generators as G

pytestmark = pytest.mark.gpu


def _xs(n, rp, ci, vt, b):
    return M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _mirror_solves(A, dt, B, cols, dinv=None):
    """[(x, iterations, status, error vs spsolve is the caller's)] of the mirror, column by column, check_every = 1."""
    return [M.Mirror(A, dt, dinv).solve(B[:, j], rtol=M.RTOL[dt], maxiter=5000, check_every=1) for j in cols]


def _check_columns(label, dt, n, rp, ci, vt, B, X, states, mirrors):
    """The per-column bounds of a solve: CONVERGED, sqrt(rr / bb) <= rtol, iterations <= 2 x the mirror's, error vs spsolve <= 10 x the mirror's own."""
    for j, (s, (xm, itm, stm, relm)) in enumerate(zip(states, mirrors)):
        assert stm == M.CONVERGED
        if not B[:, j].any():
            assert s["status"] == api.CG_CONVERGED and s["iterations"] == 0 and s["rr"] == 0.0 and not X[:, j].any(), (label, j, s)
            continue
        xs = _xs(n, rp, ci, vt, B[:, j])
        err, errm = U.relerr(X[:, j], xs), U.relerr(xm, xs)
        print("%s %s column %d: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (label, dt, j, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm, (label, j, s, itm)
        assert err <= 10 * errm, (label, j, err, errm)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [8, 4, 2])
def test_early_iterations_equal_the_mirror_per_column(torch_cuda, nvec, dtype):
    """tri200 (spectrum in [1, 13]): x and rr of every column after 1 and after 3 iterations.  Bound: 100 x the per-product tolerance, as for the single solver (three iterations
    of another summation order).  Column 1 (A 1 = 1 exactly) is at r = 0 and x = 1 after one iteration and stays; column 2 (zeros) stays at 0."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B8 = MC.system("tri200", dt)
    B = np.ascontiguousarray(B8[:, :nvec])
    A = M.scipy_csr(n, rp, ci, vt)
    mirrors = [M.Mirror(A, dt) for _ in range(nvec)]
    for j, m in enumerate(mirrors):
        m.begin(B[:, j])
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, xd = U.vec(torch, B, n, dt, nvec), U.vec(torch, None, n, dt, nvec)
    tol = 100 * PRODUCT_TOL[dt]
    with api.CGMulti(plan, nvec) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
        s0 = cg.state(U.stream(torch))
        assert len(s0) == nvec
        for j, m in enumerate(mirrors):
            assert s0[j]["iterations"] == 0
            if m.bb > 0:
                assert s0[j]["status"] == api.CG_RUNNING and abs(s0[j]["bb"] - m.bb) <= tol * m.bb and abs(s0[j]["rr"] - m.rr) <= tol * m.rr, (j, s0[j], m.bb)
            else:
                assert s0[j]["bb"] == 0.0 and s0[j]["rr"] == 0.0
        done = 0
        for step in (1, 2):
            cg.iterate(xd.data_ptr(), step, U.stream(torch)); done += step
            s = cg.state(U.stream(torch))
            X = U.host(xd, n)
            for j, m in enumerate(mirrors):
                m.iterate(step)
                assert s[j]["iterations"] == done
                if j == 1:
                    assert s[j]["rr"] == 0.0 and s[j]["status"] == api.CG_CONVERGED and np.array_equal(X[:, j], np.ones(n, dtype=dt))
                elif j == 2:
                    assert s[j]["rr"] == 0.0 and not X[:, j].any()
                else:
                    mx = m.x.astype(np.float64)
                    dx = float(np.linalg.norm(X[:, j].astype(np.float64) - mx) / np.linalg.norm(mx))
                    drr = abs(s[j]["rr"] - m.rr) / m.rr
                    print("%s nvec %d column %d after %d iterations: |x - mirror| / |mirror| = %.3g, |rr - mirror| / mirror = %.3g (bound %.3g)" % (dt, nvec, j, done, dx, drr, tol))
                    assert s[j]["status"] == api.CG_RUNNING and dx <= tol and drr <= tol, (j, done, dx, drr)
    U.intact((bd, n), (xd, n))
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [2, 4, 8])
@pytest.mark.parametrize("name,kw", [("lap128", {}), ("tri200", {}), ("fem12", {})])
def test_solves(torch_cuda, name, kw, nvec, dtype):
    """tilespmv_cg_multi_solve, maxiter = 2 x the slowest mirror column, check_every = 1 (a column that is done after one iteration has a mirror count of 1): every
    column CONVERGED, sqrt(rr / bb) <= rtol AT RETURN (the freeze), iterations <= 2 x that column's mirror count, error against the direct solution within 10 x the mirror's own."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B8 = MC.system(name, dt)
    # nvec 2: columns 0 and 1; nvec 4: 0-3 (with the zero column); nvec 8: all
    B = np.ascontiguousarray(B8[:, :nvec])
    mirrors = _mirror_solves(M.scipy_csr(n, rp, ci, vt), dt, B, range(nvec))
    plan = U.square_plan(n, rp, ci, vt, dt, **kw)
    bd, xd = U.vec(torch, B, n, dt, nvec), U.vec(torch, None, n, dt, nvec)
    with api.CGMulti(plan, nvec) as cg:
        states = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * max(m[1] for m in mirrors), check_every=1, stream=U.stream(torch))
    _check_columns("%s nvec %d" % (name, nvec), dt, n, rp, ci, vt, B, U.host(xd, n), states, mirrors)
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_on_the_default_plan(torch_cuda, dtype):
    """The builder's default plan (deterministic=-1, placement_tries=-1), whatever form and multi-vector kernel it picks: lap128, all eight columns."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("lap128", dt)
    mirrors = _mirror_solves(M.scipy_csr(n, rp, ci, vt), dt, B, range(8))
    plan = U.square_plan(n, rp, ci, vt, dt, deterministic=-1, placement_tries=-1)
    bd, xd = U.vec(torch, B, n, dt, 8), U.vec(torch, None, n, dt, 8)
    with api.CGMulti(plan, 8) as cg:
        states = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * max(m[1] for m in mirrors), check_every=8, stream=U.stream(torch))
    _check_columns("lap128 default plan", dt, n, rp, ci, vt, B, U.host(xd, n), states, mirrors)
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi(torch_cuda, dtype):
    """The scaled Laplacian at nvec 4 with the inverse diagonal from tilespmv_csr_diagonal_device (one array, shared by the columns): the per-column bounds against
    Mirror(A, dt, dinv); plain CG on the same plan ends MAXITER at the cap (columns 0 and 3)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B8 = MC.system("lap128_scaled", dt)
    B = np.ascontiguousarray(B8[:, :4])
    A = M.scipy_csr(n, rp, ci, vt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    dinv = U.vec(torch, None, n, dt)
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=U.stream(torch), dtype=dt)
    torch.cuda.synchronize()
    mirrors = _mirror_solves(A, dt, B, range(4), U.host(dinv, n))
    cap = 2 * max(m[1] for m in mirrors)
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, xd = U.vec(torch, B, n, dt, 4), U.vec(torch, None, n, dt, 4)
    with api.CGMulti(plan, 4, dinv.data_ptr()) as cg:
        states = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=cap, stream=U.stream(torch))
    _check_columns("lap128_scaled Jacobi", dt, n, rp, ci, vt, B, U.host(xd, n), states, mirrors)
    U.intact((dinv, n))
    xd[:n].zero_()
    with api.CGMulti(plan, 4) as cg:
        states = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=cap, stream=U.stream(torch))
    for j, s in enumerate(states):
        print("%s: plain CG, column %d: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, j, s["iterations"], s["status_name"], s["relative_residual"]))
        if j == 2:
            assert s["status"] == api.CG_CONVERGED and s["iterations"] == 0
        elif j != 1:      # (column 1, S A S 1, is smooth: the mirror's plain CG has it within 5 x rtol at the cap in fp32 — too close to assert on; columns 0 and 3 sit at 4 to 5)
            assert s["status"] == api.CG_MAXITER and s["iterations"] == cap, (j, s)
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_converged_columns_are_frozen(torch_cuda, dtype):
    """lap128, nvec 8, check_every = 8: the columns stop at different checks (multiples of 8; column 1 before column 0, column 2 at 0), and column 1 does not change by a bit
    while the others run on: a second solve that ends at column 1's count returns the same x[:, 1]."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("lap128", dt)
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, xd = U.vec(torch, B, n, dt, 8), U.vec(torch, None, n, dt, 8)
    with api.CGMulti(plan, 8) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2000, check_every=8, stream=U.stream(torch))
        X = U.host(xd, n)
        its = [c["iterations"] for c in s]
        print(dt, "iterations per column:", its)
        assert all(c["status"] == api.CG_CONVERGED and c["relative_residual"] <= M.RTOL[dt] for c in s)
        assert all(i % 8 == 0 for i in its) and its[2] == 0 and 0 < its[1] < its[0]
        # the device's own scalars after the solve agree with what solve returned: frozen columns kept their count and their rr
        after = cg.state(U.stream(torch))
        for j in range(8):
            if j != 2:
                assert after[j]["iterations"] == its[j] and after[j]["rr"] == s[j]["rr"], (j, after[j], s[j])
        xd[:n].zero_()
        s2 = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=its[1], check_every=8, stream=U.stream(torch))
        X2 = U.host(xd, n)
        assert s2[1]["status"] == api.CG_CONVERGED and s2[1]["iterations"] == its[1] and s2[1]["rr"] == s[1]["rr"]
        assert s2[0]["status"] == api.CG_MAXITER and s2[0]["iterations"] == its[1]
        assert np.array_equal(X2[:, 1], X[:, 1])
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order_and_columns_are_independent(torch_cuda, dtype):
    """On a plan whose multi-vector product is bit-reproducible (asserted): two solves on one plan and one on a second plan give bit-identical X, rr and iterations; and
    replacing the other columns of B leaves x[:, 0] as it was."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("lap128", dt)
    B = np.ascontiguousarray(B[:, :4])
    plan, plan2 = U.square_plan(n, rp, ci, vt, dt), U.square_plan(n, rp, ci, vt, dt)
    bd = U.vec(torch, B, n, dt, 4)
    ys = []
    for p in (plan, plan, plan2):
        yd = U.vec(torch, None, n, dt, 4)
        p.spmm(bd.data_ptr(), yd.data_ptr(), 4, U.stream(torch))
        torch.cuda.synchronize()
        ys.append(U.host(yd, n))
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2]), "the precondition: Plan.spmm is bit-reproducible on this plan"
    results = []
    for p in (plan, plan, plan2):
        xd = U.vec(torch, None, n, dt, 4)
        with api.CGMulti(p, 4) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2000, stream=U.stream(torch))
        assert all(c["status"] == api.CG_CONVERGED for c in s)
        results.append((U.host(xd, n), [c["iterations"] for c in s], [c["rr"] for c in s]))
    for X, it, rr in results[1:]:
        assert np.array_equal(X, results[0][0]) and it == results[0][1] and rr == results[0][2]
    # other neighbours: a breakdown-free but very different batch (scaled, permuted, a zero column)
    B2 = B.copy()
    B2[:, 1] = 1e6 * B[::-1, 3]; B2[:, 2] = B[:, 1]; B2[:, 3] = 0
    b2d, xd = U.vec(torch, B2, n, dt, 4), U.vec(torch, None, n, dt, 4)
    with api.CGMulti(plan, 4) as cg:
        s = cg.solve(b2d.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2000, stream=U.stream(torch))
    assert s[0]["iterations"] == results[0][1][0] and s[0]["rr"] == results[0][2][0]
    assert np.array_equal(U.host(xd, n)[:, 0], results[0][0][:, 0])
    plan.close(); plan2.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nvec_1_is_the_single_solver(torch_cuda, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("fem12", dt)
    b = np.ascontiguousarray(B[:, 0])
    plan = U.square_plan(n, rp, ci, vt, dt)
    bd, x1, xm = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt), U.vec(torch, None, n, dt)
    with api.CG(plan) as cg:
        s1 = cg.solve(bd.data_ptr(), x1.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
    with api.CGMulti(plan, 1) as cg:
        sm = cg.solve(bd.data_ptr(), xm.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
        assert len(sm) == 1 and sm[0] == s1 and s1["status"] == api.CG_CONVERGED
        assert np.array_equal(U.host(xm, n), U.host(x1, n))
        xm[:n].zero_()
        cg.begin(bd.data_ptr(), xm.data_ptr(), U.stream(torch)); cg.iterate(xm.data_ptr(), 5, U.stream(torch))
        st5 = cg.state(U.stream(torch))
    x1[:n].zero_()
    with api.CG(plan) as cg:
        cg.begin(bd.data_ptr(), x1.data_ptr(), U.stream(torch)); cg.iterate(x1.data_ptr(), 5, U.stream(torch))
        assert [cg.state(U.stream(torch))] == st5
    assert np.array_equal(U.host(xm, n), U.host(x1, n))
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kw", [{}, dict(mv_native=0)])
def test_iterate_is_capturable_into_a_hip_graph(torch_cuda, kw, dtype):
    """iterate(8) captured with torch's graph API on a side stream as tests/test_gpu_cg.py captures the single solver (one linear chain), replayed twice and compared bit for bit
    with uncaptured iterations from the same begin.  mv_native=0 forces the one-vector-at-a-time product, whose scratch create must have reserved."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("lap128", dt)
    B = np.ascontiguousarray(B[:, :4])
    plan = U.square_plan(n, rp, ci, vt, dt, **kw)
    bd, xd = U.vec(torch, B, n, dt, 4), U.vec(torch, None, n, dt, 4)
    cg = api.CGMulti(plan, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        st = side.cuda_stream
        cg.begin(bd.data_ptr(), xd.data_ptr(), st)
        cg.iterate(xd.data_ptr(), 8, st)                      # (uncaptured: the comparison, and the warm-up)
        s8 = cg.state(st); x8 = U.host(xd, n)
        cg.iterate(xd.data_ptr(), 8, st)
        s16 = cg.state(st); x16 = U.host(xd, n)
        xd[:n].zero_()
        cg.begin(bd.data_ptr(), xd.data_ptr(), st)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cg.iterate(xd.data_ptr(), 8, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not U.host(xd, n).any()                             # (captured, not run)
    for want_x, want_s in ((x8, s8), (x16, s16)):
        graph.replay(); torch.cuda.synchronize()
        s = cg.state(U.stream(torch))
        assert np.array_equal(U.host(xd, n), want_x)
        assert s == want_s and s[0]["status"] == api.CG_RUNNING and s[0]["iterations"] == want_s[0]["iterations"]
    del graph
    cg.close(); plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards_per_column(torch_cuda, dtype):
    """A = 2 I with a zero column, ordinary columns and a start vector: every non-zero column is at r = 0 exactly after one iteration (alpha = 1/2 is exact) and stays, the zero
    column stays at 0; solve zeroes the x of a zero column whatever the start vector was.  A = -(the Laplacian): p.Ap < 0 in every column in the first iteration — BREAKDOWN at
    the first check, x untouched."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n = 4096
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dt)
    B = MC.columns(n, M.scipy_csr(n, rp, ci, v.astype(np.float64)))[:, [0, 2, 3, 7]].astype(dt)      # (column 1 of the batch is zero)
    B = np.ascontiguousarray(B)
    plan = U.square_plan(n, rp, ci, v, dt)
    bd, xd = U.vec(torch, B, n, dt, 4), U.vec(torch, None, n, dt, 4)
    with api.CGMulti(plan, 4) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
        cg.iterate(xd.data_ptr(), 1, stream)
        s = cg.state(stream)
        X1 = U.host(xd, n)
        assert all(c["rr"] == 0.0 and c["iterations"] == 1 for c in s) and np.array_equal(X1, B / dt.type(2))
        cg.iterate(xd.data_ptr(), 16, stream)
        s = cg.state(stream)
        assert all(c["rr"] == 0.0 and c["iterations"] == 17 and c["status"] == api.CG_CONVERGED for c in s) and np.array_equal(U.host(xd, n), X1)
        x0 = np.ascontiguousarray(np.tile(M.rhs(n)[:, None], (1, 4)).astype(dt))
        xd[:n].copy_(torch.from_numpy(x0))
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        X = U.host(xd, n)
        assert s[1]["status"] == api.CG_CONVERGED and s[1]["iterations"] == 0 and s[1]["rr"] == 0.0 and not X[:, 1].any()
        for j in (0, 2, 3):
            assert s[j]["status"] == api.CG_CONVERGED and s[j]["iterations"] == 8 and s[j]["relative_residual"] <= M.RTOL[dt], (j, s[j])
            assert U.relerr(X[:, j], B[:, j].astype(np.float64) / 2) <= 100 * PRODUCT_TOL[dt]
    plan.close()
    n, rp, ci, vt, B8 = MC.system("lap128", dt)
    B = np.ascontiguousarray(B8[:, [0, 3, 5, 7]])
    x0 = np.ascontiguousarray(np.stack([M.rhs(n)[::-1], M.rhs(n), 2 * M.rhs(n)[::-1], np.ones(n)], axis=1).astype(dt))
    neg = U.square_plan(n, rp, ci, -vt, dt)
    bd, xd = U.vec(torch, B, n, dt, 4), U.vec(torch, x0, n, dt, 4)
    with api.CGMulti(neg, 4) as cg:
        s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        assert all(c["status"] == api.CG_BREAKDOWN and c["iterations"] == 8 for c in s), s      # (the first check)
        assert np.array_equal(U.host(xd, n), x0)
    neg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("nvec", [2, 8])
def test_nothing_is_touched_past_the_end(torch_cuda, nvec, jacobi, dtype):
    """B, X (and dinv) with 16 sentinel rows behind them, on fem12 and on tri_mesh(53, 39) (2067 rows: in fp32 with nvec 2 the flat arrays end in half a 16-byte vector): the
    sentinels survive a solve, B is unchanged, and the odd-sized solve is within 100 x rtol of the direct solution."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    for label, (m, n, rp, ci) in (("fem12", G.fem_hex(12, 12, 12, 3)), ("tri53x39", G.tri_mesh(53, 39))):
        assert m == n and (label == "fem12" or n == 2067)
        rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
        v = M.spd_values(n, rp, ci)
        vt = v.astype(dt)
        B = np.ascontiguousarray(MC.columns(n, M.scipy_csr(n, rp, ci, v))[:, :nvec].astype(dt))
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = (dt.type(1) / A.diagonal().astype(dt)).astype(dt) if jacobi else None
        plan = U.square_plan(n, rp, ci, vt, dt)
        bd, xd = U.vec(torch, B, n, dt, nvec), U.vec(torch, None, n, dt, nvec)
        dd = U.vec(torch, dinv, n, dt) if jacobi else None
        m3 = M.Mirror(A, dt, dinv); m3.begin(B[:, 0]); m3.iterate(3)
        with api.CGMulti(plan, nvec, dd.data_ptr() if jacobi else None) as cg:
            cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
            cg.iterate(xd.data_ptr(), 3, stream)
            s = cg.state(stream)
            x3 = U.host(xd, n)[:, 0]
            dx = float(np.linalg.norm(x3.astype(np.float64) - m3.x.astype(np.float64)) / np.linalg.norm(m3.x.astype(np.float64)))
            print("%s %s nvec %d jacobi=%s: 3 iterations, column 0 |x - mirror| / |mirror| = %.3g, rr %.6g (mirror %.6g)" % (label, dt, nvec, jacobi, dx, s[0]["rr"], m3.rr))
            assert dx <= 100 * PRODUCT_TOL[dt] and abs(s[0]["rr"] - m3.rr) <= 100 * PRODUCT_TOL[dt] * m3.rr
            xd[:n].zero_()
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
        X = U.host(xd, n)
        for j in range(nvec):
            assert s[j]["status"] == api.CG_CONVERGED, (label, j, s[j])
            if B[:, j].any():
                assert U.relerr(X[:, j], _xs(n, rp, ci, vt, B[:, j])) <= 100 * M.RTOL[dt], (label, j)      # (degree + 1 on the diagonal: condition number below 50)
        U.intact((bd, n), (xd, n), *(((dd, n),) if jacobi else ()))
        assert np.array_equal(U.host(bd, n), B)
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(torch_cuda, dtype):
    """Shards, non-square plans, misaligned arrays and other nvec: hipErrorInvalidValue from the library, ValueError from api.CGMulti."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    n, rp, ci, vt, B = MC.system("lap128", dt)
    shard = U.square_plan(n, rp, ci, vt, dt, tilerow_end=(n // 16) // 2)
    m, nc, brp, bci = G.band(2048, 40, ncols=4096)
    wide = api.Plan.from_csr(m, nc, len(bci), brp, bci, G.real_values(len(bci), dt), dtype=dt, deterministic=1, placement_tries=1)
    for plan in (shard, wide):
        for nvec in (1, 4):
            h = C.c_void_p(1)
            assert lib.tilespmv_cg_multi_create(C.byref(h), plan.h, nvec, None) == api.HIP_ERROR_INVALID_VALUE and not h
            with pytest.raises(ValueError):
                api.CGMulti(plan, nvec)
        plan.close()
    plan = U.square_plan(n, rp, ci, vt, dt)
    for nvec in (0, 3, 16):
        with pytest.raises(ValueError):
            api.CGMulti(plan, nvec)
    bd, xd, dd = U.vec(torch, B[:, :2], n, dt, 2), U.vec(torch, None, n, dt, 2), U.vec(torch, np.ones(n), n, dt)
    off = dt.itemsize
    with pytest.raises(ValueError):
        api.CGMulti(plan, 2, dd.data_ptr() + off)
    with api.CGMulti(plan, 2) as cg:
        with pytest.raises(ValueError):
            cg.begin(bd.data_ptr() + off, xd.data_ptr(), U.stream(torch))
        with pytest.raises(ValueError):
            cg.begin(bd.data_ptr(), xd.data_ptr() + off, U.stream(torch))
        with pytest.raises(ValueError):
            cg.iterate(xd.data_ptr() + off, 1, U.stream(torch))
        with pytest.raises(ValueError):
            cg.solve(bd.data_ptr(), xd.data_ptr() + off, stream=U.stream(torch))
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_operator_cg_with_a_matrix_of_right_hand_sides(torch_cuda, dtype):
    """SparseOperator.cg with b of shape (rows, 3) and (rows, 11): column for column the results of api.CGMulti on the padded groups (SparseOperator.cg_groups); a 1-D b gives
    what it gave before."""
    from tilespmv_amd.operator import SparseOperator
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, B8 = MC.system("fem12", dt)
    B11 = np.ascontiguousarray(np.concatenate([B8, B8[::-1, :3]], axis=1))
    assert SparseOperator.cg_groups(3) == [(0, 3, 4)] and SparseOperator.cg_groups(11) == [(0, 8, 8), (8, 3, 4)]
    with SparseOperator(n, n, rp, ci, vt, deterministic=1, placement_tries=1) as op:
        for k in (3, 11):
            B = np.ascontiguousarray(B11[:, :k])
            X, infos = op.cg(torch.from_numpy(B).cuda(), rtol=M.RTOL[dt], maxiter=500)
            assert tuple(X.shape) == (n, k) and len(infos) == k
            Xh = X.cpu().numpy()
            for g, w, nvec in SparseOperator.cg_groups(k):
                Bg = np.zeros((n, nvec), dtype=dt)
                Bg[:, :w] = B[:, g:g + w]
                bd, xd = U.vec(torch, Bg, n, dt, nvec), U.vec(torch, None, n, dt, nvec)
                with api.CGMulti(op.A, nvec) as cg:
                    s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
                Xg = U.host(xd, n)
                assert not Xg[:, w:].any() and all(c["iterations"] == 0 and c["status"] == api.CG_CONVERGED for c in s[w:])      # the padding
                for j in range(w):
                    info = infos[g + j]
                    assert np.array_equal(Xh[:, g + j], Xg[:, j]), (k, g + j)
                    assert info["iterations"] == s[j]["iterations"] and info["relative_residual"] == s[j]["relative_residual"] and info["status"] == s[j]["status_name"]
                    assert info["converged"] and info["relative_residual"] <= M.RTOL[dt]
        b = torch.from_numpy(np.ascontiguousarray(B8[:, 0])).cuda()
        x, info = op.cg(b, rtol=M.RTOL[dt], maxiter=500)
        xd = U.vec(torch, None, n, dt)
        with api.CG(op.A) as cg:
            s = cg.solve(b.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=U.stream(torch))
        assert isinstance(info, dict) and x.dim() == 1 and info["iterations"] == s["iterations"] and np.array_equal(x.cpu().numpy(), U.host(xd, n))
        # a whole group in place: (rows, 4) needs no copies
        X4, infos4 = op.cg(torch.from_numpy(np.ascontiguousarray(B8[:, :4])).cuda(), rtol=M.RTOL[dt], maxiter=500)
        assert all(i["converged"] for i in infos4) and np.array_equal(X4.cpu().numpy()[:, :3], op.cg(torch.from_numpy(np.ascontiguousarray(B8[:, :3])).cuda(), rtol=M.RTOL[dt], maxiter=500)[0].cpu().numpy())
