"""The MINRES solver in the library on the GPU (tilespmv_minres_*, tilespmv_csr_abs_diagonal_device; include/tilespmv.h) against its numpy mirror
(tests/minres_mirror.py, itself checked by tests/test_minres_cpu.py) and scipy's direct solutions.  Plans come from SparseOperator(..., deterministic=1, placement_tries=1) unless a
test says otherwise; sixteen sentinel elements stand behind every caller vector.

The GPU is compared with the mirror iterate for iterate only after 1 and 3 iterations, within 100 x the per-product tolerance (the bound of the sibling files; two summation orders
of the fp64 mirror differ by <= 3e-15 there).  The library multiplies A z by the rounded 1 / beta where the mirror multiplies A by the rounded v = z / beta: one rounding per element
apart.  Further on, a solve is judged by its end: status, residual, error against spsolve.

What this solver promises like every other one is written once in tests/solver_contract.py, whose table has this solver's inputs and counts: graph capture and nothing
touched past the end run from tests/test_gpu_solver_contract.py; the fixed order of the sums, value refresh and the refusals of create are the tests of those names here."""
import numpy as np
import pytest

import gpu_solver_util as U
import minres_mirror as M
import solver_contract as K
import solver_sizes as Z
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import api
from tilespmv_amd.operator import SparseOperator, minres as torch_minres

pytestmark = pytest.mark.gpu

_CACHE = {}


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
        _CACHE[(name, dt, rhs)] = (xs, itm, U.relerr(xm, xs))
    return _CACHE[(name, dt, rhs)]


def _early(torch, dt, A, b, plan, minv, n, label, x0=None):
    """x, rr and bb after begin, 1 and 3 iterations against the mirror of A.  Bound: 100 x the per-product tolerance; a wrong sign, a stale scalar, a swapped vector or a wrong
    parity of the history is an O(1) difference."""
    m = M.Mirror(A, dt, minv)
    m.begin(b, x0)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
    dd = None if minv is None else U.vec(torch, minv, n, dt)
    with api.MINRES(plan, None if dd is None else dd.data_ptr()) as ms:
        ms.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
        s0 = ms.state(U.stream(torch))
        print("%s %s begin: rr %.3g bb %.3g" % (label, dt, U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(U.dist(s0["rr"], m.rr), U.dist(s0["bb"], m.bb)) <= bound
        done = 0
        for step in (1, 2):
            ms.iterate(xd.data_ptr(), step, U.stream(torch)); m.iterate(step); done += step
            s = ms.state(U.stream(torch))
            dx = U.relerr(U.host(xd, n), m.x)
            drr, dbb = U.dist(s["rr"], m.rr), U.dist(s["bb"], m.bb)
            print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g, bb %.3g (bound %.3g)" % (label, dt, done, dx, drr, dbb, bound))
            assert s["iterations"] == done == m.iterations and s["status"] == api.CG_RUNNING == m.status()
            assert dx <= bound and drr <= bound and dbb <= bound
    assert np.array_equal(U.host(bd, n), b)
    U.intact((bd, n), (xd, n), *(((dd, n),) if dd is not None else ()))
    return bd, xd, dd


# ---- early iterations
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["saddle47", "saddlec47_scaled"])
def test_early_iterations_equal_the_mirror(torch_cuda, name, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        _early(torch, dt, M.scipy_csr(n, rp, ci, vt), b, op.A, _minv_of(name, n, rp, ci, vt, dt), n, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_iterations_on_the_transposed_plan(torch_cuda, dtype):
    """api.MINRES(op.AT): a square transposed plan qualifies; K^T = K, so three iterations equal the mirror of K."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("saddle47", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
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
    with U.square_op(n, rp, ci, vt, dt, **kw) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=U.stream(torch))
        x = U.host(xd, n)
    err = U.relerr(x, xs)
    print("saddle47 %s %s: GPU %d iterations (mirror %d), sqrt(rr/bb) %.3g, error %.3g (mirror %.3g)" % (dt, kw, s["iterations"], itm, s["relative_residual"], err, errm))
    assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    U.intact((bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_preconditioner(torch_cuda, dtype):
    """saddlec47_scaled: minv from tilespmv_csr_abs_diagonal_device(invert) equals numpy's 1 / |diag| bit for bit; preconditioned MINRES converges within 2 x the mirror's count to
    an error within 10 x the mirror's; the plain solver on the same plan is at MAXITER at that cap."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("saddlec47_scaled", dt)
    xs, itm, errm = _solved("saddlec47_scaled", dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    minv = U.vec(torch, None, n, dt)
    api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), minv.data_ptr(), invert=True, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    want = M.inverse_abs_diagonal(n, rp, ci, vt, dt)
    assert np.array_equal(U.host(minv, n), want) and (want > 0).all()
    plain = U.vec(torch, None, n, dt)      # (invert = 0: |d| itself; 552 of the signed diagonal entries are negative)
    api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), plain.data_ptr(), invert=False, stream=stream, dtype=dt)
    torch.cuda.synchronize()
    diag = M.scipy_csr(n, rp, ci, vt).diagonal()
    assert np.array_equal(U.host(plain, n), np.abs(diag)) and (diag < 0).sum() == 552
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.MINRES(op.A, minv.data_ptr()) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s: preconditioned MINRES %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        xd[:n].zero_()
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
        print("%s: plain MINRES on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, s["iterations"], s["status_name"], s["relative_residual"]))
        assert s["status"] == api.CG_MAXITER and s["iterations"] == 2 * itm
    U.intact((minv, n), (plain, n), (bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_breaks_down_and_minres_solves_it(torch_cuda, dtype):
    """saddle47 with b on the zero block: p.Ap = b.K b = 0 exactly in CG's first iteration — api.CG reports BREAKDOWN with x untouched; api.MINRES on the same plan converges."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, _ = _system("saddle47", dt)
    b = M.zero_block_rhs(n).astype(dt)
    xs, itm, errm = _solved("saddle47", dt, "zero_block")
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.CG(op.A) as cg:
            s = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
        assert s["status"] == api.CG_BREAKDOWN and not U.host(xd, n).any(), s
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s: MINRES %d iterations (mirror %d), error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and err <= 10 * errm
    U.intact((bd, n), (xd, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_residual_never_increases(torch_cuda, dtype):
    """40 single iterations on saddle47, rr read after each."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("saddle47", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
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
    stream = U.stream(torch)
    # b = 0
    n, rp, ci, vt, b = _system("saddle47", dt)
    with U.square_op(n, rp, ci, vt, dt) as op:
        zero, xd = U.vec(torch, None, n, dt), U.vec(torch, b, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(zero.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()
            ms.begin(zero.data_ptr(), xd.data_ptr(), stream)
            ms.iterate(xd.data_ptr(), 16, stream)
            s = ms.state(stream)
            x = U.host(xd, n)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.isfinite(x).all() and not x.any()
        U.intact((zero, n), (xd, n))
    # pow2I: bb = 262144, beta = 512, alfa = 2, y' = 0, beta' = 0, gamma = 2: x = 4 and rr = 0 after one iteration, exact in both value types
    n, rp, ci, v = M.problem("pow2I")
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, np.full(n, 8.0), n, dt), U.vec(torch, None, n, dt)
        with api.MINRES(op.A) as ms:
            ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
            s = ms.state(stream)
            assert s["bb"] == 262144.0 and s["rr"] == 262144.0 and s["status"] == api.CG_RUNNING
            ms.iterate(xd.data_ptr(), 1, stream)
            s = ms.state(stream)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and s["bb"] == 262144.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), np.full(n, 4.0, dtype=dt))
            ms.iterate(xd.data_ptr(), 16, stream)
            s = ms.state(stream)
            assert s["iterations"] == 17 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), np.full(n, 4.0, dtype=dt))
        # minv = -1: r2.z < 0 in begin
        x0 = M.rhs(n).astype(dt)
        neg, xd = U.vec(torch, -np.ones(n), n, dt), U.vec(torch, x0, n, dt)
        with api.MINRES(op.A, neg.data_ptr()) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 0 and np.array_equal(U.host(xd, n), x0)
            ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
            ms.iterate(xd.data_ptr(), 5, stream)
            s = ms.state(stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 5 and np.array_equal(U.host(xd, n), x0)
        U.intact((bd, n), (xd, n), (neg, n))
    # singular: A b = 0 exactly: alfa = 0, y' = 0, beta' = 0, gamma = 0 in the first iteration
    n, rp, ci, v = M.problem("singular")
    b, x0 = M.singular_rhs(n).astype(dt), np.zeros(n, dtype=dt)
    with U.square_op(n, rp, ci, v, dt) as op:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        with api.MINRES(op.A) as ms:
            s = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(U.host(xd, n), x0) and s["rr"] == 2049.0
        U.intact((bd, n), (xd, n))


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
    stream = U.stream(torch)
    n = Z.capped_n(dt)
    plan, _ = _square(built, "2I", n, dt)
    b64 = Z.exact_rhs(n)
    bb = Z.exact_bb(b64)
    b, half = b64.astype(dt), (b64 / 2).astype(dt)
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with api.MINRES(plan) as ms:
        ms.begin(bd.data_ptr(), xd.data_ptr(), stream)
        s0 = ms.state(stream)
        assert s0["bb"] == bb and s0["rr"] == bb and s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING, (s0, bb)
        ms.iterate(xd.data_ptr(), 1, stream)
        s1 = ms.state(stream)
        x1 = U.host(xd, n)
    ulps = np.abs(x1.astype(np.float64) - half.astype(np.float64)) / np.spacing(np.abs(half)).astype(np.float64)
    print("%s: n = %d, largest distance of x from b / 2: %.3g ulp at element %d; rr after one iteration %.3g of bb" % (dt, n, ulps.max(), int(ulps.argmax()), s1["rr"] / bb))
    assert s1["iterations"] == 1 and s1["bb"] == bb and s1["status"] in (api.CG_RUNNING, api.CG_CONVERGED)
    assert ulps.max() <= 4
    assert np.array_equal(U.host(bd, n), b)
    U.intact((bd, n), (xd, n))


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
    assert np.array_equal(U.host(dd, n), minv)


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
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.MINRES(plan) as ms:
            st = ms.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm + 2, check_every=1, stream=U.stream(torch))
        err, errm = U.relerr(U.host(xd, n), xs), U.relerr(xm, xs)
        print("n = %d %s: %d iterations (mirror %d), error against the dense float64 solution %.3g (mirror %.3g)" % (n, dt, st["iterations"], itm, err, errm))
        assert st["status"] == api.CG_CONVERGED and st["relative_residual"] <= M.RTOL[dt], (n, st)
        assert err <= 10 * max(errm, floor), (n, err, errm)
        assert np.array_equal(U.host(bd, n), b)
        U.intact((bd, n), (xd, n))
        plan.close()


# ---- the promises shared with the other solvers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_have_a_fixed_order(torch_cuda, dtype):
    """tests/solver_contract.py: bit-identical x and state on separately created deterministic operators (saddlec47_scaled, minv, 20 iterations)."""
    K.sums_have_a_fixed_order(torch_cuda, "minres", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """tests/solver_contract.py: update_values and the diagonal recomputed into the same array; the untouched solver equals one on a fresh operator bit for bit."""
    K.value_refresh(torch_cuda, "minres", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, dtype):
    """tests/solver_contract.py: a non-square plan, a shard plan, a misaligned minv: hipErrorInvalidValue, no handle, ValueError from the class."""
    K.create_refuses_what_it_must(torch_cuda, "minres", dtype)


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
