"""The four device-resident solvers (tilespmv_cg_*, tilespmv_cg_multi_*, tilespmv_cgls_*, tilespmv_bicgstab_*) at the sizes where the shared walk of
tilespmv_amd/csrc/hip_solver_common.h changes regime: past the cap of 1024 partial sums (a second sweep of every streaming kernel, with a partial last trip and a scalar tail),
at 300 partials (a fold in two passes), with one of CGLS's two lengths capped and the other not, and below one 16-byte lane vector.  tests/solver_sizes.py has the sizes,
tests/test_solver_sizes_cpu.py proves which regime each reaches.

Three kinds of check: against the numpy mirrors of the older solver files with their bound (100 x PRODUCT_TOL, tests/test_gpu_cg.py); exact cases on A = 2 I with integer data,
compared with array_equal and == (no tolerance: every partial sum is an integer below 2^53 in any order); tiny systems solved to convergence against a dense float64 solution.
Sixteen sentinel elements stand behind every caller vector.  Plans are created with deterministic=1, placement_tries=1."""
import numpy as np
import pytest

import bicgstab_mirror as BM
import cg_mirror as M
import cg_multi_cases as MC
import cgls_mirror as LM
import gpu_solver_util as U
import solver_sizes as Z
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import api
from tilespmv_amd.operator import SparseOperator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_cross_forms.py)."""
    import torch
    torch.zeros(1, device="cuda")
    yield


@pytest.fixture(scope="module")
def built():
    """Plans and operators shared by the tests of this file: key -> (object, host data), closed at the end."""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    yield get
    for obj, _ in cache.values():
        obj.close()


MATRICES = {"spd": Z.spd_tridiagonal, "nonsym": Z.nonsymmetric_tridiagonal, "2I": Z.two_identity}


def _square(built, kind, n, dt):
    """(plan, (n, rp, ci, values in dt)) of a named n x n matrix."""
    def make():
        _, rp, ci, v = MATRICES[kind](n)
        vt = np.ascontiguousarray(v, dtype=dt)
        return api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1), (n, rp, ci, vt)
    return built((kind, n, np.dtype(dt).name), make)


def _scattered(built, case, dt):
    """(operator, (rows, cols, rp, ci, values in dt)) of cgls_mirror._scattered at the tall / wide shape."""
    def make():
        rows, cols = Z.cgls_shape(case, dt)
        rp, ci, v = LM._scattered(rows, cols)
        rp, ci, vt = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=dt)
        return SparseOperator(rows, cols, rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1), (rows, cols, rp, ci, vt)
    return built(("scattered", case, np.dtype(dt).name), make)


# ---- against the mirrors
def _steps_equal_the_mirror(torch, label, dt, solver, mirror, begin, bd, b, xd, x0, nx, keys0, keys, repeat, bound=None):
    """begin, iterate(1), iterate(2) on the GPU and on the mirror: x and the state's scalars after every step within `bound` (100 x PRODUCT_TOL unless the caller measured
    another one); with `repeat`, a second begin + iterate(3) on the same handle gives the same bits.  Returns the largest differences seen."""
    stream = U.stream(torch)
    bound = 100 * PRODUCT_TOL[dt] if bound is None else bound
    begin()
    s0 = solver.state(stream)
    d0 = max(U.dist(s0[k], getattr(mirror, k)) for k in keys0)
    print("%s %s begin: largest relative difference of %s = %.3g (bound %.3g)" % (label, dt, "/".join(keys0), d0, bound))
    assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
    assert d0 <= bound
    done, worst = 0, d0
    for step in (1, 2):
        solver.iterate(xd.data_ptr(), step, stream); mirror.iterate(step); done += step
        s = solver.state(stream)
        x = U.host(xd, nx)
        dx = U.relerr(x, mirror.x)
        dk = max(U.dist(s[k], getattr(mirror, k)) for k in keys)
        print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, %s %.3g (bound %.3g)" % (label, dt, done, dx, "/".join(keys), dk, bound))
        assert s["iterations"] == done and s["status"] == api.CG_RUNNING
        assert dx <= bound and dk <= bound
        worst = max(worst, dx, dk)
    if repeat:
        xd[:nx].copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=dt)))
        begin()
        solver.iterate(xd.data_ptr(), 3, stream)
        s2 = solver.state(stream)
        assert np.array_equal(U.host(xd, nx), x) and all(s2[k] == s[k] for k in keys) and s2["iterations"] == 3
    assert np.array_equal(U.host(bd, len(b)), b)
    return worst


SINGLE_CASES = [("capped", False), ("capped", True), ("fold2", False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,preconditioned", SINGLE_CASES)
def test_cg_equals_the_mirror(torch_cuda, built, case, preconditioned, dtype):
    """Tridiagonal (-1, 3, -1) at n = 1 052 249 / 2 104 499 (two sweeps) and 307 201 / 614 403 (300 partials), from x0 != 0; the preconditioned variant uses a diagonal that varies
    with the row.  First run on the MI355X, |x - mirror| / |mirror| and the difference of rr after three iterations: fp64 capped 1.6e-16 / 4.7e-16, preconditioned 1.9e-16 / 0,
    fold2 1.4e-16 / 1.3e-16; fp32 capped 7.4e-08 / 2.2e-11, preconditioned 7.4e-08 / 6.2e-10, fold2 7.4e-08 / 2.2e-10."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n = Z.single_n(case, dt)
    plan, (_, rp, ci, vt) = _square(built, "spd", n, dt)
    b, x0 = M.rhs(n).astype(dt), (0.25 * M.rhs(n)[::-1]).astype(dt)
    dinv = Z.diagonal_preconditioner(n).astype(dt) if preconditioned else None
    m = M.Mirror(M.scipy_csr(n, rp, ci, vt), dt, dinv)
    m.begin(b, x0)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
    dd = U.vec(torch, dinv, n, dt) if preconditioned else None
    with api.CG(plan, dd.data_ptr() if preconditioned else None) as cg:
        _steps_equal_the_mirror(torch, "CG %s%s" % (case, " preconditioned" if preconditioned else ""), dt, cg, m,
                                lambda: cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch)), bd, b, xd, x0, n, ("bb", "rr"), ("rr",), case == "capped")
    U.intact((bd, n), (xd, n), *(((dd, n),) if preconditioned else ()))
    if preconditioned:
        assert np.array_equal(U.host(dd, n), dinv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,preconditioned", SINGLE_CASES)
def test_bicgstab_equals_the_mirror(torch_cuda, built, case, preconditioned, dtype):
    """Tridiagonal (-1.5, 3, -0.5) at the sizes of test_cg_equals_the_mirror.  First run on the MI355X, |x - mirror| / |mirror| and the difference of rr after three iterations: fp64 capped
    1.7e-16 / 0, preconditioned 1.6e-16 / 0, fold2 1.8e-16 / 1.6e-16; fp32 capped 8.7e-08 / 3.8e-10, preconditioned 8.8e-08 / 7.7e-09, fold2 8.8e-08 / 4.7e-09."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n = Z.single_n(case, dt)
    plan, (_, rp, ci, vt) = _square(built, "nonsym", n, dt)
    b, x0 = BM.rhs(n).astype(dt), (0.25 * BM.rhs(n)[::-1]).astype(dt)
    dinv = Z.diagonal_preconditioner(n).astype(dt) if preconditioned else None
    m = BM.Mirror(BM.scipy_csr(n, rp, ci, vt), dt, dinv)
    m.begin(b, x0)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
    dd = U.vec(torch, dinv, n, dt) if preconditioned else None
    with api.BiCGStab(plan, dd.data_ptr() if preconditioned else None) as bs:
        _steps_equal_the_mirror(torch, "BiCGStab %s%s" % (case, " preconditioned" if preconditioned else ""), dt, bs, m,
                                lambda: bs.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch)), bd, b, xd, x0, n, ("bb", "rr"), ("rr",), case == "capped")
    U.intact((bd, n), (xd, n), *(((dd, n),) if preconditioned else ()))
    if preconditioned:
        assert np.array_equal(U.host(dd, n), dinv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,preconditioned", [("tall", False), ("tall", True), ("wide", False)])
def test_cgls_equals_the_mirror(torch_cuda, built, case, preconditioned, dtype):
    """cgls_mirror._scattered at 1 052 249 x 307 201 (fp32: 2 104 499 x 614 403; npr = 1024, npc = 300: a grid of 1024 with 724 workgroups idle on the column walks) and at the
    swapped shape; the preconditioned variant takes cinv = 1 / |a_j|^2.  First run on the MI355X, |x - mirror| / |mirror| and the larger difference of nn and rr after three iterations:
    fp64 tall 2.5e-16 / 0, with cinv 2.6e-16 / 3.6e-16, wide 2.0e-16 / 0; fp32 tall 1.2e-07 / 1.7e-09, with cinv 1.3e-07 / 2.5e-09, wide 8.8e-08 / 1.8e-09."""
    torch, dt = torch_cuda, np.dtype(dtype)
    op, (rows, cols, rp, ci, vt) = _scattered(built, case, dt)
    A = LM.scipy_csr(rows, cols, rp, ci, vt)
    b, x0 = LM.rhs(rows).astype(dt), (0.25 * LM.rhs(cols)[::-1]).astype(dt)
    cinv = LM.column_cinv(A, dt) if preconditioned else None
    m = LM.Mirror(A, dt, cinv)
    m.begin(b, x0)
    bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, x0, cols, dt)
    cd = U.vec(torch, cinv, cols, dt) if preconditioned else None
    with api.CGLS(op.A, op.AT, cd.data_ptr() if preconditioned else None) as ls:
        _steps_equal_the_mirror(torch, "CGLS %s%s" % (case, " with cinv" if preconditioned else ""), dt, ls, m,
                                lambda: ls.begin(bd.data_ptr(), xd.data_ptr(), 0.0, U.stream(torch)), bd, b, xd, x0, cols, ("bb", "rr", "nn", "nn0"), ("nn", "rr"), True)
    U.intact((bd, rows), (xd, cols), *(((cd, cols),) if preconditioned else ()))
    if preconditioned:
        assert np.array_equal(U.host(cd, cols), cinv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,nvec,preconditioned", [(c, k, False) for c, k in Z.MULTI_CASES] + [("capped", 8, True)])
def test_cg_multi_equals_the_mirror_per_column(torch_cuda, built, case, nvec, preconditioned, dtype):
    """Tridiagonal (-1, 3, -1), the first nvec right-hand sides of tests/cg_multi_cases.py, X0 != 0: every column against the mirror of the single solver after begin, 1 and 3
    iterations.  The flat stream rows x nvec has 526 124 lane vectors (two sweeps; fp32 with nvec = 2: 1 052 249 rows, the tail is one row) or 153 600 (300 partials per
    column).  First run on the MI355X, largest difference of x or rr over the columns and steps: fp64 capped nvec 8 / 4 / 2: 2.7e-15 / 2.6e-15 / 5.7e-16, fold2 2.9e-15,
    preconditioned 2.4e-15; fp32 1.3e-06 / 1.3e-06 / 8.6e-08, fold2 1.3e-06, preconditioned 1.2e-06."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    bound = 100 * PRODUCT_TOL[dt]
    rows = Z.multi_rows(case, nvec, dt)
    plan, (_, rp, ci, vt) = _square(built, "spd", rows, dt)
    A = M.scipy_csr(rows, rp, ci, vt)
    B = np.ascontiguousarray(MC.columns(rows, A.astype(np.float64))[:, :nvec].astype(dt))
    X0 = np.ascontiguousarray((0.25 / nvec * np.outer(M.rhs(rows)[::-1], np.arange(1, nvec + 1))).astype(dt))   # (no column starts at its solution: the zero column of B too is RUNNING)
    dinv = Z.diagonal_preconditioner(rows).astype(dt) if preconditioned else None
    mirrors = [M.Mirror(A, dt, dinv) for _ in range(nvec)]
    for j, m in enumerate(mirrors):
        m.begin(B[:, j], X0[:, j])
    bd, xd = U.vec(torch, B, rows, dt, nvec), U.vec(torch, X0, rows, dt, nvec)
    dd = U.vec(torch, dinv, rows, dt) if preconditioned else None
    worst = 0.0
    with api.CGMulti(plan, nvec, dd.data_ptr() if preconditioned else None) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
        s0 = cg.state(stream)
        for j, m in enumerate(mirrors):
            d0 = max(U.dist(s0[j]["bb"], m.bb), U.dist(s0[j]["rr"], m.rr))
            assert s0[j]["iterations"] == 0 and s0[j]["status"] == api.CG_RUNNING and d0 <= bound, (j, s0[j], m.bb, m.rr)
            worst = max(worst, d0)
        done = 0
        for step in (1, 2):
            cg.iterate(xd.data_ptr(), step, stream); done += step
            s = cg.state(stream)
            X = U.host(xd, rows)
            for j, m in enumerate(mirrors):
                m.iterate(step)
                dx, drr = U.relerr(X[:, j], m.x), U.dist(s[j]["rr"], m.rr)
                print("CGMulti %s nvec %d %s column %d after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)" % (case, nvec, dt, j, done, dx, drr, bound))
                assert s[j]["iterations"] == done and s[j]["status"] == api.CG_RUNNING
                assert dx <= bound and drr <= bound, (j, dx, drr)
                worst = max(worst, dx, drr)
        if case == "capped":
            xd[:rows].copy_(torch.from_numpy(X0))
            cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
            cg.iterate(xd.data_ptr(), 3, stream)
            s2 = cg.state(stream)
            assert np.array_equal(U.host(xd, rows), X) and [c["rr"] for c in s2] == [c["rr"] for c in s]
    print("CGMulti %s nvec %d %s%s: largest difference %.3g" % (case, nvec, dt, " preconditioned" if preconditioned else "", worst))
    assert np.array_equal(U.host(bd, rows), B)
    U.intact((bd, rows), (xd, rows), *(((dd, rows),) if preconditioned else ()))


# ---- exact cases: A = 2 I, integer data, no tolerance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("solver", ["cg", "cg_dinv", "bicgstab", "cgls"])
def test_two_identity_is_solved_exactly(torch_cuda, built, solver, dtype):
    """A = 2 I at the capped n, b in the nonzero integers of [-30, 30]: bb is the integer sum of the squares; one iteration gives x = b / 2 and a residual of exactly 0 (CG:
    alpha = 1/2; with dinv = 1/2: alpha = 1; BiCGStab: alpha = 1/2, s = 0, omega = 0, converged at the half step; CGLS: alpha = 1/4), status CONVERGED, and sixteen more
    iterations change nothing.  An element dropped, visited twice or left unwritten by any sweep changes x or one of the integer sums."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n = Z.capped_n(dt)
    plan, _ = _square(built, "2I", n, dt)
    b64 = Z.exact_rhs(n)
    bb = Z.exact_bb(b64)
    b, half = b64.astype(dt), (b64 / 2).astype(dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    dd = U.vec(torch, np.full(n, 0.5), n, dt) if solver == "cg_dinv" else None
    if solver in ("cg", "cg_dinv"):
        s = api.CG(plan, dd.data_ptr() if dd is not None else None)
    elif solver == "bicgstab":
        s = api.BiCGStab(plan)
    else:
        s = api.CGLS(plan, plan)          # (2 I is its own transpose)
    norm = "nn" if solver == "cgls" else "rr"
    with s:
        if solver == "cgls":
            s.begin(bd.data_ptr(), xd.data_ptr(), 0.0, stream)
        else:
            s.begin(bd.data_ptr(), xd.data_ptr(), stream)
        s0 = s.state(stream)
        assert s0["bb"] == bb and s0["rr"] == bb and s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING, (s0, bb)
        if solver == "cgls":
            assert s0["nn"] == 4 * bb and s0["nn0"] == 4 * bb
        s.iterate(xd.data_ptr(), 1, stream)
        s1 = s.state(stream)
        x1 = U.host(xd, n)
        assert np.array_equal(x1, half), "%d elements of x differ from b / 2, the first at %d" % (int((x1 != half).sum()), int(np.argmax(x1 != half)))
        assert s1[norm] == 0.0 and s1["rr"] == 0.0 and s1["bb"] == bb and s1["iterations"] == 1 and s1["status"] == api.CG_CONVERGED, s1
        s.iterate(xd.data_ptr(), 16, stream)
        s17 = s.state(stream)
        assert s17["iterations"] == 17 and s17[norm] == 0.0 and s17["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), half)
    assert np.array_equal(U.host(bd, n), b)
    U.intact((bd, n), (xd, n), *(((dd, n),) if dd is not None else ()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [8, 4, 2])
@pytest.mark.parametrize("zero_column", [False, True])
def test_two_identity_is_solved_exactly_per_column(torch_cuda, built, nvec, zero_column, dtype):
    """A = 2 I on the capped multi-RHS sizes, B[:, c] = (c + 1) x the cyclic shift of b by c + 1 rows: bb_c = (c + 1)^2 bb, so a partial sum that lands in the wrong column shows
    as a swapped bb; after one iteration X = B / 2, rr = 0 and CONVERGED in every column.  alpha = 1/2 in every column of 2 I, so a ROTATED alpha would pass: with
    `zero_column` the last column but one is 0 (its alpha is 0 by the rho = 0 guard, its state CONVERGED from the start) and its neighbours still have to reach B / 2."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    rows = Z.multi_rows("capped", nvec, dt)
    plan, _ = _square(built, "2I", rows, dt)
    B64 = Z.exact_columns(rows, nvec)
    if zero_column:
        B64[:, nvec - 2] = 0
    bbs = [Z.exact_bb(B64[:, c]) for c in range(nvec)]
    B, half = np.ascontiguousarray(B64.astype(dt)), np.ascontiguousarray((B64 / 2).astype(dt))
    bd, xd = U.vec(torch, B, rows, dt, nvec), U.vec(torch, None, rows, dt, nvec)
    with api.CGMulti(plan, nvec) as cg:
        cg.begin(bd.data_ptr(), xd.data_ptr(), stream)
        s0 = cg.state(stream)
        assert [c["bb"] for c in s0] == bbs and [c["rr"] for c in s0] == bbs, (s0, bbs)
        assert [c["status"] for c in s0] == [api.CG_RUNNING if v else api.CG_CONVERGED for v in bbs]
        for count, total in ((1, 1), (16, 17)):
            cg.iterate(xd.data_ptr(), count, stream)
            s = cg.state(stream)
            X = U.host(xd, rows)
            bad = [c for c in range(nvec) if not np.array_equal(X[:, c], half[:, c])]
            assert bad == [], "columns %s differ from B / 2 after %d iterations" % (bad, total)
            assert all(c["rr"] == 0.0 and c["status"] == api.CG_CONVERGED and c["iterations"] == total for c in s) and [c["bb"] for c in s] == bbs, s
    assert np.array_equal(U.host(bd, rows), B)
    U.intact((bd, rows), (xd, rows))


# ---- below one lane vector
def _yardstick(label, dt, err, errm):
    """The yardstick of the older solver files: the error against the float64 solution within 10 x the mirror's own.  On a system of a few unknowns the mirror's x can be the
    float64 solution rounded to the value type, or that solution itself: an error of 0 (first run on the MI355X: rows = 2, nvec = 8, column 4 in fp64 and column 5 in fp32, the
    GPU at 2.9e-17 and 3.8e-08).  No x in the value type is owed less than one unit roundoff (2^-53, 2^-24), so the mirror's error counts as at least that."""
    floor = float(np.finfo(dt).eps) / 2
    print("%s %s: error against the dense float64 solution %.3g (mirror %.3g)" % (label, dt, err, errm))
    assert err <= 10 * max(errm, floor), (label, err, errm)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_tiny_systems(torch_cuda, solver, dtype):
    """n in {1, 2, 3, 5}: with n < 2 (fp64) / n < 4 (fp32) there is no lane vector at all and thread 0 of workgroup 0 owns every element.  Solved to the mirrors' rtol; the error
    against numpy's dense float64 solution within 10 x the mirror's own."""
    torch, dt = torch_cuda, np.dtype(dtype)
    Mir, Solver, matrix = (M, api.CG, Z.spd_tridiagonal) if solver == "cg" else (BM, api.BiCGStab, Z.nonsymmetric_tridiagonal)
    for n in Z.TINY_N:
        _, rp, ci, v = matrix(n)
        vt, b = v.astype(dt), Mir.rhs(n).astype(dt)
        A = Mir.scipy_csr(n, rp, ci, vt)
        xs = np.linalg.solve(A.toarray().astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = Mir.Mirror(A, dt).solve(b, rtol=Mir.RTOL[dt], maxiter=50, check_every=1)
        assert stm == Mir.CONVERGED
        plan = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1)
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with Solver(plan) as s:
            st = s.solve(bd.data_ptr(), xd.data_ptr(), rtol=Mir.RTOL[dt], maxiter=2 * itm + 2, check_every=1, stream=U.stream(torch))
        assert st["status"] == api.CG_CONVERGED and st["relative_residual"] <= Mir.RTOL[dt], (n, st)
        _yardstick("%s n = %d, %d iterations (mirror %d)" % (solver, n, st["iterations"], itm), dt, U.relerr(U.host(xd, n), xs), U.relerr(xm, xs))
        assert np.array_equal(U.host(bd, n), b)
        U.intact((bd, n), (xd, n))
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_multi_systems(torch_cuda, dtype):
    """rows in {1, 2, 3, 5} x nvec in {2, 4, 8}: in fp32, one row of two columns is a flat stream without a lane vector.  Every column by the rule of test_tiny_systems; a zero
    column is CONVERGED at 0 iterations with x = 0."""
    torch, dt = torch_cuda, np.dtype(dtype)
    for rows in Z.TINY_N:
        _, rp, ci, v = Z.spd_tridiagonal(rows)
        vt = v.astype(dt)
        A = M.scipy_csr(rows, rp, ci, vt)
        B8 = MC.columns(rows, A.astype(np.float64))
        plan = api.Plan.from_csr(rows, rows, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1)
        for nvec in Z.TINY_NVEC:
            B = np.ascontiguousarray(B8[:, :nvec].astype(dt))
            mirrors = [M.Mirror(A, dt).solve(B[:, j], rtol=M.RTOL[dt], maxiter=50, check_every=1) for j in range(nvec)]
            bd, xd = U.vec(torch, B, rows, dt, nvec), U.vec(torch, None, rows, dt, nvec)
            with api.CGMulti(plan, nvec) as cg:
                states = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * max(m[1] for m in mirrors) + 2, check_every=1, stream=U.stream(torch))
            X = U.host(xd, rows)
            for j, (st, (xm, itm, stm, relm)) in enumerate(zip(states, mirrors)):
                assert stm == M.CONVERGED and st["status"] == api.CG_CONVERGED and st["relative_residual"] <= M.RTOL[dt], (rows, nvec, j, st)
                if not B[:, j].any():
                    assert st["iterations"] == 0 and not X[:, j].any()
                    continue
                xs = np.linalg.solve(A.toarray().astype(np.float64), B[:, j].astype(np.float64))
                _yardstick("multi rows = %d nvec = %d column %d" % (rows, nvec, j), dt, U.relerr(X[:, j], xs), U.relerr(xm, xs))
            assert np.array_equal(U.host(bd, rows), B)
            U.intact((bd, rows), (xd, rows))
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_least_squares(torch_cuda, dtype):
    """(rows, cols) in {(1, 1), (3, 2), (2, 3), (5, 3)}, dense and of full rank: against numpy's float64 least-squares solution (the minimum-norm one for 2 x 3, which CGLS
    reaches from x = 0), by the rule of test_tiny_systems."""
    torch, dt = torch_cuda, np.dtype(dtype)
    for rows, cols in Z.TINY_CGLS:
        rp, ci, v, _ = Z.tiny_cgls_matrix(rows, cols)
        vt, b = v.astype(dt), LM.rhs(rows).astype(dt)
        A = LM.scipy_csr(rows, cols, rp, ci, vt)
        xs = np.linalg.lstsq(A.toarray().astype(np.float64), b.astype(np.float64), rcond=None)[0]
        xm, itm, stm, relm = LM.Mirror(A, dt).solve(b, rtol=LM.RTOL[dt], maxiter=50, check_every=1)
        assert stm == LM.CONVERGED
        with SparseOperator(rows, cols, rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1) as op:
            bd, xd = U.vec(torch, b, rows, dt), U.vec(torch, None, cols, dt)
            with api.CGLS(op.A, op.AT) as ls:
                st = ls.solve(bd.data_ptr(), xd.data_ptr(), damp=0.0, rtol=LM.RTOL[dt], maxiter=2 * itm + 2, check_every=1, stream=U.stream(torch))
            assert st["status"] == api.CG_CONVERGED and st["relative_normal_residual"] <= LM.RTOL[dt], (rows, cols, st)
            _yardstick("CGLS %d x %d, %d iterations (mirror %d)" % (rows, cols, st["iterations"], itm), dt, U.relerr(U.host(xd, cols), xs), U.relerr(xm, xs))
            assert np.array_equal(U.host(bd, rows), b)
            U.intact((bd, rows), (xd, cols))
