"""GMRES with the Krylov basis stored as floats in the fp64 library, on the GPU (tilespmv_gmres_create_basis; include/tilespmv.h) against the compressed numpy
mirror (tests/gmres_cb_mirror.py, itself checked by tests/test_gmres_cb_cpu.py), the uncompressed mirror and scipy's direct solutions.  Plans come from tests/gpu_solver_util.py
with deterministic = 1.  fp64 carries the content; the fp32 cases check that basis = 4 is the identity there.

THE BOUND OF AN EARLY COMPARISON is that of tests/test_gpu_gmres.py::_early, 100 x the per-product tolerance.  One thing can break it that is no bug: the GPU's sums have another
order than numpy's, and a difference of one ulp of a double can carry an entry of w'' / h across a rounding boundary of float32; that entry of the stored basis then differs by a
float32 ulp.  Where the bound fails, _early runs the mirror again with its dot products in a permuted order (the mirror's own ``order`` argument): if the mirror itself, against
itself, cannot hold the bound under another order, no implementation can, and the comparison takes 4 x float32 eps instead.  Anything else is a bug."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import block_jacobi_mirror as BJ
import gmres_cb_mirror as CB
import gmres_mirror as M
import gpu_solver_util as U
import solver_contract as K
import solver_sizes as SS
from gpu_solver_util import DTYPES, PRODUCT_TOL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api
from tilespmv_amd.operator import SparseOperator, gmres as torch_gmres

pytestmark = pytest.mark.gpu

F64 = np.dtype(np.float64)
RESTART = 16
RTOL = 1e-10
FLIPPED = 4 * float(np.finfo(np.float32).eps)
INPUTS = ["convdiff67", "convdom67", "shiftskew67", "convdiff67_colscaled"]
_CACHE = {}


def _gm(plan, restart, d=None, block=None):
    return api.GMRES(plan, restart, d, block=block, basis=4)


def _system(name, dtype=F64):
    dt = np.dtype(dtype)
    n, rp, ci, v = CB.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _true_rel(A, b, x):
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(b64 - A.astype(np.float64) @ x.astype(np.float64)) / np.linalg.norm(b64))


def _residual_rounding(A, b, x, dt):
    """tests/test_gpu_gmres.py: how far apart the norms of b - A x formed in the value type and in float64 may lie, relative to |b|."""
    A64, x64, b64 = abs(A.astype(np.float64)), abs(x.astype(np.float64)), abs(b.astype(np.float64))
    per_row = int(np.diff(A.indptr).max())
    return float((per_row + 2) * (np.finfo(dt).eps + np.finfo(np.float64).eps) * np.linalg.norm(A64 @ x64 + b64) / np.linalg.norm(b64))


def _solved(name):
    """The compressed mirror's solve (fp64 values, restart 16; Jacobi on the column-scaled input) of a named input and the direct solution, computed once and left unchanged:
    (xs, mirror iterations, mirror error, the mirror's true relative residual)."""
    if name not in _CACHE:
        n, rp, ci, vt, b = _system(name)
        A = M.scipy_csr(n, rp, ci, vt)
        dinv = M.inverse_diagonal(n, rp, ci, vt, F64) if name.endswith("_colscaled") else None
        xs = M.spsolve_x(n, rp, ci, vt, b)
        xm, itm, stm, relm = CB.Mirror(A, F64, RESTART, dinv).solve(b, rtol=RTOL, maxiter=5000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[name] = (xs, itm, U.relerr(xm, xs), _true_rel(A, b, xm))
    return _CACHE[name]


def _held(far, bound, own, label):
    """The rule of the module's docstring: ``far`` (the GPU's distance from the mirror) is within ``bound``, or the mirror's distance from itself under permuted sums, own(),
    is not either and ``far`` is within what flipped float roundings explain."""
    if far <= bound:
        return
    itself = own()
    print("%s: the mirror against itself with permuted sums: %.3g; the GPU against the mirror %.3g (bound %.3g; flipped float roundings allow %.3g)" % (label, itself, far, bound, FLIPPED))
    assert itself > bound, "the mirror holds the bound under another order of the sums: the GPU's %.3g is a bug" % far
    assert far <= FLIPPED


def _early(torch, dt, make_mirror, b, make_solver, n, label, steps=(3, 2)):
    """begin; rr after each of ``steps`` inner iterations, before any flush; after all of them and a flush x and the state — against make_mirror(order = None), the compressed
    mirror.  Bound: the module's docstring.  Returns (b and x on the device, x on the host)."""
    def mirrored(order):
        m = make_mirror(order)
        m.begin(b)
        seen = [(m.rr, m.bb)]
        for step in steps:
            m.iterate(step)
            seen.append((m.rr, m.iterations, m.status()))
        m.flush()
        return m, seen

    mirror, seen = mirrored(None)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    st = U.stream(torch)
    far = []      # every distance from the mirror
    with make_solver() as gm:
        gm.begin(bd.data_ptr(), xd.data_ptr(), st)
        s0 = gm.state(st)
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        far += [U.dist(s0["rr"], seen[0][0]), U.dist(s0["bb"], seen[0][1])]
        done = 0
        for step, (rr, iterations, status) in zip(steps, seen[1:]):
            gm.iterate(xd.data_ptr(), step, st); done += step
            s = gm.state(st)
            assert s["iterations"] == done == iterations and s["status"] == api.CG_RUNNING == status
            far.append(U.dist(s["rr"], rr))
        gm.flush(xd.data_ptr(), st)
        s = gm.state(st)
        x = U.host(xd, n)
        assert s["iterations"] == done and s["status"] == api.CG_RUNNING == mirror.status()
        far += [U.relerr(x, mirror.x.astype(np.float64)), U.dist(s["rr"], mirror.rr)]
    print("%s %s: begin rr %.3g bb %.3g; rr after the steps %s; after the flush |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)"
          % (label, dt, far[0], far[1], ", ".join("%.3g" % f for f in far[2:-2]), far[-2], far[-1], bound))
    def own():
        permuted, seenp = mirrored(np.random.default_rng(11).permutation(n))
        return max([U.dist(seenp[0][0], seen[0][0])] + [U.dist(p[0], q[0]) for p, q in zip(seenp[1:], seen[1:])] +
                   [U.relerr(permuted.x, mirror.x.astype(np.float64)), U.dist(permuted.rr, mirror.rr)])

    _held(max(far), bound, own, "%s %s" % (label, dt))
    U.intact((xd, n))
    assert np.array_equal(U.host(bd, n), b)
    return bd, xd, x


# ---- the recurrence
def test_early_iterates_equal_the_compressed_mirror_and_not_the_plain_one(torch_cuda):
    """convdiff67, restart 8: rr after iterate(3), rr after two more, then x and rr after a flush equal the compressed mirror's; the same x lies at least 1e-9 from the
    UNcompressed mirror's (the two mirrors differ by 3.1e-8 .. 3.7e-8 on the four inputs): the basis really is rounded, and the product reads the rounded vector."""
    torch = torch_cuda
    n, rp, ci, vt, b = _system("convdiff67")
    A = M.scipy_csr(n, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, F64) as op:
        bd, xd, x = _early(torch, F64, lambda order: CB.Mirror(A, F64, 8, order=order), b, lambda: _gm(op.A, 8), n, "convdiff67")
    plain = M.Mirror(A, F64, 8); plain.begin(b); plain.iterate(5); plain.flush()
    apart = U.relerr(x, plain.x)
    print("convdiff67: the GPU's x against the uncompressed mirror's: %.3g" % apart)
    assert 1e-9 <= apart <= 1e-6


@pytest.mark.parametrize("name", INPUTS)
def test_solves(torch_cuda, name):
    """tilespmv_gmres_solve with the float basis, restart 16 and maxiter = 2 x the compressed mirror's count, judged as tests/test_gpu_gmres.py::test_solves judges the value
    form: CONVERGED, an error against spsolve within 10 x the mirror's own, a reported sqrt(rr / bb) that equals the one recomputed on the host up to the rounding of a residual
    and is at most max(RTOL, 2 x the mirror's true residual) — and at most one restart more iterations than the GPU's own value-basis solve of the same plan."""
    torch = torch_cuda
    n, rp, ci, vt, b = _system(name)
    A = M.scipy_csr(n, rp, ci, vt)
    xs, itm, errm, truem = _solved(name)
    with U.square_op(n, rp, ci, vt, F64) as op:
        bd, xd = U.vec(torch, b, n, F64), U.vec(torch, None, n, F64)
        dd = U.vec(torch, M.inverse_diagonal(n, rp, ci, vt, F64), n, F64) if name.endswith("_colscaled") else None
        d = None if dd is None else dd.data_ptr()
        with _gm(op.A, RESTART, d) as gm:
            assert gm.basis_bytes == 4
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=2 * itm, check_every=8, stream=U.stream(torch))
        x = U.host(xd, n)
        xd[:n].zero_()
        with api.GMRES(op.A, RESTART, d) as gm:
            sv = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=2 * itm, check_every=8, stream=U.stream(torch))
    err, true, slack = U.relerr(x, xs), _true_rel(A, b, x), _residual_rounding(A, b, x, F64)
    print("%s: float basis %d iterations on the GPU (value basis %d; compressed mirror %d), sqrt(rr/bb) %.4g, recomputed on the host %.4g (rounding of a residual %.3g; mirror's "
          "true %.4g), error %.3g (mirror %.3g)" % (name, s["iterations"], sv["iterations"], itm, s["relative_residual"], true, slack, truem, err, errm))
    assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm
    assert err <= 10 * errm
    assert abs(s["relative_residual"] - true) <= slack
    assert s["relative_residual"] <= max(RTOL, 2 * truem)
    assert sv["status"] == api.CG_CONVERGED and s["iterations"] <= sv["iterations"] + RESTART
    U.intact((xd, n))


def test_the_floor_of_one_cycle_and_the_solve_rule(torch_cuda):
    """shiftskew67_d4, restart 64.  After begin, iterate(40), flush the recomputed sqrt(rr / bb) is within a factor 4 of the compressed mirror's (2.7e-8), while the recurrence
    said 1e-14 or less before the flush.  solve(rtol = 1e-10) returns CONVERGED with a recomputed residual <= 1e-10 within 2 x the mirror's count: a solve that decided on the
    recurrence's rr would return the x of the floor."""
    torch = torch_cuda
    st = U.stream(torch)
    n, rp, ci, vt, b = _system("shiftskew67_d4")
    A = M.scipy_csr(n, rp, ci, vt)
    mirror = CB.Mirror(A, F64, 64); mirror.begin(b); mirror.iterate(40); mirror.flush()
    with U.square_op(n, rp, ci, vt, F64) as op:
        bd, xd = U.vec(torch, b, n, F64), U.vec(torch, None, n, F64)
        with _gm(op.A, 64) as gm:
            gm.begin(bd.data_ptr(), xd.data_ptr(), st)
            gm.iterate(xd.data_ptr(), 40, st)
            recurrence = gm.state(st)["relative_residual"]
            gm.flush(xd.data_ptr(), st)
            s = gm.state(st)
            print("after 40 iterations the recurrence says %.3g; recomputed after the flush %.3g (mirror %.3g), on the host %.3g"
                  % (recurrence, s["relative_residual"], mirror.rel(), _true_rel(A, b, U.host(xd, n))))
            assert recurrence <= 1e-14 and s["iterations"] == 40
            assert mirror.rel() / 4 <= s["relative_residual"] <= 4 * mirror.rel()
            for check_every in (1, 8):
                xm, itm, stm, relm = CB.Mirror(A, F64, 64).solve(b, rtol=RTOL, maxiter=500, check_every=check_every)
                xd[:n].zero_()
                s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=2 * itm, check_every=check_every, stream=st)
                x = U.host(xd, n)
                true, slack = _true_rel(A, b, x), _residual_rounding(A, b, x, F64)
                print("check_every %d: %d iterations (mirror %d), sqrt(rr/bb) %.3g, on the host %.3g" % (check_every, s["iterations"], itm, s["relative_residual"], true))
                assert stm == M.CONVERGED and s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm
                assert s["relative_residual"] <= RTOL and true <= RTOL + slack
        U.intact((xd, n), (bd, n))


# ---- preconditioners
def test_jacobi(torch_cuda):
    """convdiff67_colscaled with d_dinv: zhat = dinv o widen(Vhat).  Early iterations equal the compressed Jacobi mirror; the solve is test_solves[convdiff67_colscaled]."""
    torch = torch_cuda
    n, rp, ci, vt, b = _system("convdiff67_colscaled")
    A, dinv = M.scipy_csr(n, rp, ci, vt), M.inverse_diagonal(n, rp, ci, vt, F64)
    with U.square_op(n, rp, ci, vt, F64) as op:
        dd = U.vec(torch, dinv, n, F64)
        _early(torch, F64, lambda order: CB.Mirror(A, F64, 8, dinv, order=order), b, lambda: _gm(op.A, 8, dd.data_ptr()), n, "convdiff67_colscaled Jacobi")
        U.intact((dd, n))
        assert np.array_equal(U.host(dd, n), dinv)


def test_block_jacobi(torch_cuda):
    """femblk10_ns with api.BlockJacobi(bs = 3): vcur = widen(Vhat) is the input of the apply.  Early iterations equal the compressed block mirror; the solve converges within
    2 x the mirror's count to an error within 10 x the mirror's; d_dinv together with block raises."""
    torch = torch_cuda
    stream = U.stream(torch)
    n, rp, ci, v = BJ.problem("femblk10_ns")
    vt, b = v.astype(F64), M.rhs(n).astype(F64)
    A = M.scipy_csr(n, rp, ci, vt)
    P, _ = BJ.update(n, rp, ci, vt, 3, F64)
    xs = M.spsolve_x(n, rp, ci, vt, b)
    xm, itm, stm, relm = CB.BlockMirror(A, F64, RESTART, P).solve(b, rtol=RTOL, maxiter=1000, check_every=1)
    assert stm == M.CONVERGED
    errm = U.relerr(xm, xs)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, F64) as op, api.BlockJacobi(n, 3, F64) as bj3:
        bj3.update(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), stream)
        bd, xd, _ = _early(torch, F64, lambda order: CB.BlockMirror(A, F64, 8, P, order=order), b, lambda: _gm(op.A, 8, block=bj3), n, "femblk10_ns bs=3")
        xd[:n].zero_()
        with _gm(op.A, RESTART, block=bj3) as gm:
            assert gm.workspace_bytes == CB.workspace_bytes(n, RESTART, 8, 4, "block")
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=2 * itm, check_every=8, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("block Jacobi, float basis: %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * itm and s["relative_residual"] <= RTOL
        assert err <= 10 * errm
        U.intact((xd, n))
        dinv = U.vec(torch, None, n, F64)
        with pytest.raises(ValueError):
            _gm(op.A, 8, dinv.data_ptr(), block=bj3)
        h = C.c_void_p(1)
        assert _lib.load(F64).tilespmv_gmres_create_basis(C.byref(h), op.A.h, 8, C.c_void_p(dinv.data_ptr()), bj3.h, 4) == api.HIP_ERROR_INVALID_VALUE and not h


# ---- edges
@pytest.mark.parametrize("restart,count", [(1, 3), (64, 2 * 64 + 3)])
def test_restart_1_and_64(torch_cuda, restart, count):
    """The two ends of the restart range (the last group of the basis loop, every slot of the float basis and of the partial arrays) over two cycles and more, against the
    compressed mirror."""
    torch = torch_cuda
    n, rp, ci, vt, b = _system("convdiff67")
    A = M.scipy_csr(n, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, F64) as op:
        _early(torch, F64, lambda order: CB.Mirror(A, F64, restart, order=order), b, lambda: _gm(op.A, restart), n, "restart %d" % restart, steps=(count - 1, 1))


def test_restart_boundaries_batch_alike(torch_cuda):
    """restart = 5: iterate(5) + iterate(5), iterate(10) and ten iterate(1) are the same bits on a deterministic plan."""
    torch = torch_cuda
    st = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67")
    with U.square_op(n, rp, ci, vt, F64) as op:
        bd, xd = U.vec(torch, b, n, F64), U.vec(torch, None, n, F64)
        got = []
        for batches in ((5, 5), (10,), (1,) * 10):
            xd[:n].zero_()
            with _gm(op.A, 5) as gm:
                gm.begin(bd.data_ptr(), xd.data_ptr(), st)
                for c in batches:
                    gm.iterate(xd.data_ptr(), c, st)
                got.append((U.host(xd, n), gm.state(st)))
        for x, s in got:
            assert s["iterations"] == 10 and np.array_equal(x, got[0][0]) and s == got[0][1] and x.any()


@pytest.mark.parametrize("n", SS.TINY_N)
def test_tiny_systems(torch_cuda, n):
    """1, 2, 3 and 5 rows (no full lane vector, or one and a tail: with odd rows the scalar tail reads and writes a float): the solve converges to the dense solution and touches
    nothing behind the vectors.  A Krylov space of n dimensions is exhausted after n iterations, at the floor of that cycle (eps32 x the condition number, below 1e-5 here), so
    the second cycle of n reaches 1e-10: at most 2 n iterations."""
    torch = torch_cuda
    _, rp, ci, v = SS.tridiagonal(n, -1.5, 3.0, -0.5) if n > 1 else SS.two_identity(1)
    vt, b = v.astype(F64), (np.arange(n) + 1.0).astype(F64)
    xs = np.linalg.solve(M.scipy_csr(n, rp, ci, vt).toarray(), b)
    with U.square_op(n, rp, ci, vt, F64) as op:
        bd, xd = U.vec(torch, b, n, F64), U.vec(torch, None, n, F64)
        with _gm(op.A, 8) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=16, check_every=1, stream=U.stream(torch))
        print("%d rows: %s" % (n, s))
        assert s["status"] == api.CG_CONVERGED and s["iterations"] <= 2 * n and s["relative_residual"] <= RTOL
        assert U.relerr(U.host(xd, n), xs) <= 100 * RTOL
        U.intact((xd, n), (bd, n))


TIER_512_ROWS = (32 << 20) // 8 + 3      # tests/test_gpu_gmres.py: the first size with 512 workgroups, and a scalar tail


@pytest.mark.parametrize("rows", [None, TIER_512_ROWS])
def test_past_the_workgroup_cap(torch_cuda, rows):
    """solver_sizes.capped_n rows (1 052 249: several sweeps, a partial last trip, the scalar tail) and 4 194 307 rows (512 workgroups and partials per sum), on the nonsymmetric
    tridiagonal with a diagonal preconditioner that varies from row to row: five iterations and a flush equal the compressed mirror's."""
    torch = torch_cuda
    n, rp, ci, v = SS.nonsymmetric_tridiagonal(rows or SS.capped_n(F64))
    dinv, b = SS.diagonal_preconditioner(n), SS.exact_rhs(n)
    A = M.scipy_csr(n, rp, ci, v)
    with U.square_op(n, rp, ci, v, F64) as op:
        dd = U.vec(torch, dinv, n, F64)
        with _gm(op.A, 4, dd.data_ptr()) as gm:
            assert gm.workspace_bytes == CB.workspace_bytes(n, 4, 8, 4, "dinv")
        _early(torch, F64, lambda order: CB.Mirror(A, F64, 4, dinv, order=order), b, lambda: _gm(op.A, 4, dd.data_ptr()), n, "%d rows" % n)
        U.intact((dd, n))


def test_the_transposed_plan_solves_the_transposed_system(torch_cuda):
    torch = torch_cuda
    n, rp, ci, vt, b = _system("convdiff67")
    AT = M.scipy_csr(n, rp, ci, vt).T.tocsr()
    with U.square_op(n, rp, ci, vt, F64) as op:
        _early(torch, F64, lambda order: CB.Mirror(AT, F64, 8, order=order), b, lambda: _gm(op.AT, 8), n, "convdiff67^T")


# ---- guards
def test_guards(torch_cuda):
    """b = 0; the lucky termination (A = 2 I, b = 4 e_k: e_k is a float, everything is exact) closes the cycle early and gives 2 e_k bit for bit; gamma = 0 (nilpotent) raises the
    breakdown flag and leaves x alone; maxiter cuts the last block and solve's flush makes x and rr current."""
    torch = torch_cuda
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67")
    with U.square_op(n, rp, ci, vt, F64) as op:
        zero, xd = U.vec(torch, None, n, F64), U.vec(torch, b, n, F64)
        with _gm(op.A, 8) as gm:
            s = gm.solve(zero.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=100, stream=stream)
            assert s["iterations"] == 0 and s["status"] == api.CG_CONVERGED and s["rr"] == 0.0 and not U.host(xd, n).any()
            gm.begin(zero.data_ptr(), xd.data_ptr(), stream)
            gm.iterate(xd.data_ptr(), 16, stream)
            gm.flush(xd.data_ptr(), stream)
            s = gm.state(stream)
            assert s["iterations"] == 16 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()
        bd = U.vec(torch, b, n, F64)
        A = M.scipy_csr(n, rp, ci, vt)
        xm, itm, stm, relm = CB.Mirror(A, F64, 8).solve(b, rtol=RTOL, maxiter=13, check_every=8)
        for check_every in (8, 0):
            xd[:n].zero_()
            with _gm(op.A, 8) as gm:
                s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=13, check_every=check_every, stream=stream)
            x = U.host(xd, n)
            assert s["iterations"] == 13 and s["status"] == api.CG_MAXITER == stm
            def own():
                xp, _, _, relp = CB.Mirror(A, F64, 8, order=np.random.default_rng(11).permutation(n)).solve(b, rtol=RTOL, maxiter=13, check_every=8)
                return max(U.relerr(xp, xm), U.dist(relp, relm))
            _held(max(U.relerr(x, xm), U.dist(s["relative_residual"], relm)), 100 * PRODUCT_TOL[F64], own, "maxiter 13")
            assert abs(s["relative_residual"] - _true_rel(A, b, x)) <= _residual_rounding(A, b, x, F64)
    n, rp, ci, v = M.problem("2I")
    e = np.zeros(n); e[1234] = 1.0
    with U.square_op(n, rp, ci, v, F64) as op:
        bd, xd = U.vec(torch, 4 * e, n, F64), U.vec(torch, None, n, F64)
        with _gm(op.A, 8) as gm:
            gm.begin(bd.data_ptr(), xd.data_ptr(), stream)
            gm.iterate(xd.data_ptr(), 1, stream)
            s = gm.state(stream)
            assert s["iterations"] == 1 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and not U.host(xd, n).any()      # (x waits for the close)
            gm.iterate(xd.data_ptr(), 5, stream)
            gm.flush(xd.data_ptr(), stream)
            s = gm.state(stream)
            assert s["iterations"] == 6 and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED and np.array_equal(U.host(xd, n), 2 * e)
    n, rp, ci, v = M.problem("nilpotent")
    b, x0 = M.nilpotent_rhs(n), np.zeros(n)
    with U.square_op(n, rp, ci, v, F64) as op:
        bd, xd = U.vec(torch, b, n, F64), U.vec(torch, x0, n, F64)
        with _gm(op.A, 8) as gm:
            s = gm.solve(bd.data_ptr(), xd.data_ptr(), rtol=RTOL, maxiter=100, check_every=8, stream=stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 8      # (the first check)
            assert np.array_equal(U.host(xd, n), x0) and s["rr"] == float(b @ b)
            gm.iterate(xd.data_ptr(), 9, stream)
            s = gm.state(stream)
            assert s["status"] == api.CG_BREAKDOWN and s["iterations"] == 17 and np.array_equal(U.host(xd, n), x0)


def test_an_overrun_captured_cycle_leaves_x_alone(torch_cuda):
    """A = 2 I, b = 4 e_k, restart 8: a captured iterate(8) replayed three times behind an eager begin.  The first replay terminates luckily in its first column and its close
    gives 2 e_k exactly; its open finds rr = 0, so the two replays that overrun convergence change x by no bit while the iteration count goes on."""
    torch = torch_cuda
    n, rp, ci, v = M.problem("2I")
    e = np.zeros(n); e[1234] = 1.0
    with U.square_op(n, rp, ci, v, F64) as op:
        bd, xd = U.vec(torch, 4 * e, n, F64), U.vec(torch, None, n, F64)
        gm = _gm(op.A, 8)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = side.cuda_stream
            gm.begin(bd.data_ptr(), xd.data_ptr(), st)      # (uncaptured: the warm-up)
            gm.iterate(xd.data_ptr(), 8, st)
            side.synchronize()
            xd[:n].zero_()
            gm.begin(bd.data_ptr(), xd.data_ptr(), st)      # the cycle position is 0: a boundary
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                gm.iterate(xd.data_ptr(), 8, st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert not U.host(xd, n).any()      # (captured, not run)
        for replay in (1, 2, 3):
            graph.replay(); torch.cuda.synchronize()
            s = gm.state(U.stream(torch))
            assert s["iterations"] == 8 * replay and s["rr"] == 0.0 and s["status"] == api.CG_CONVERGED
            assert np.array_equal(U.host(xd, n), 2 * e)
        del graph
        gm.close()
        U.intact((xd, n), (bd, n))


# ---- the five promises of tests/solver_contract.py, on a copy of the table's "gmres" row made here
def _past_early(torch, dt, op, A, b, dinv, dims, label):
    """Three and five iterations of restart 8 and a flush against the compressed mirror, as the ``_gmres_early`` of tests/test_gpu_solver_contract.py."""
    dd = U.vec(torch, dinv, dims[0], dt)
    return _early(torch, dt, lambda order: CB.Mirror(A, dt, 8, dinv, order=order), b, lambda: _gm(op.A, 8, dd.data_ptr()), dims[0], label)[:2] + (dd, None)


@pytest.fixture
def contract_row():
    """The "gmres" row with the float basis and the compressed mirror under the key "gmres_cb", for the length of one test; ``create`` is tilespmv_gmres_create_basis(...,
    bj = NULL, 4) bound on the loaded libraries under a name the table can call with tilespmv_gmres_create's arguments."""
    def create_basis_4(lib):
        return lambda h, plan, restart, d: lib.tilespmv_gmres_create_basis(h, plan, restart, d, None, 4)
    libs = [_lib.load(dt) for dt in DTYPES]
    for lib in libs:
        lib.gmres_create_float_basis = create_basis_4(lib)
    K.SOLVERS["gmres_cb"] = SimpleNamespace(**{**vars(K.SOLVERS["gmres"]), "M": CB, "api": functools.partial(api.GMRES, basis=4), "create": "gmres_create_float_basis",
                                               "past_early": _past_early})
    yield "gmres_cb"
    del K.SOLVERS["gmres_cb"]
    for lib in libs:
        del lib.gmres_create_float_basis


def test_sums_have_a_fixed_order(torch_cuda, contract_row):
    K.sums_have_a_fixed_order(torch_cuda, contract_row, F64)


def test_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, contract_row):
    K.begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, contract_row, F64)


def test_value_refresh(torch_cuda, contract_row):
    K.value_refresh(torch_cuda, contract_row, F64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refuses_what_it_must(torch_cuda, contract_row, dtype):
    K.create_refuses_what_it_must(torch_cuda, contract_row, dtype)


def test_nothing_is_touched_past_the_end(torch_cuda, contract_row):
    for case in K.SOLVERS[contract_row].past:
        K.nothing_is_touched_past_the_end(torch_cuda, contract_row, F64, **{k: v for k, v in case.items() if k != "id"})


# ---- identity, the attributes, the operator
@pytest.mark.parametrize("dtype", DTYPES)
def test_basis_0_and_the_value_types_size_are_the_plain_solver(torch_cuda, dtype):
    """create_basis(..., 0) and create_basis(..., sizeof value) — 4 in the fp32 library — give x and state bit-identical to tilespmv_gmres_create after 19 iterations of restart 8
    and a flush, with d_dinv and with a block object; basis_bytes and workspace_bytes are those of the header; 2, 3, 16 and the other library's size raise ValueError."""
    torch, dt = torch_cuda, np.dtype(dtype)
    st = U.stream(torch)
    n, rp, ci, vt, b = _system("convdiff67_colscaled", dt)
    dinv = M.inverse_diagonal(n, rp, ci, vt, dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op, api.BlockJacobi(n, 3, dt) as bj:
        bj.update(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), st)
        bd, xd, dd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt), U.vec(torch, dinv, n, dt)
        for kw, precond in ((dict(d_dinv=None), None), (dict(d_dinv=dd.data_ptr()), "dinv"), (dict(block=bj), "block")):
            got = []
            for basis in (None, 0, "value", dt.itemsize) + (("float32",) if dt == np.float32 else ()):
                xd[:n].zero_()
                with api.GMRES(op.A, 8, basis=basis, **kw) as gm:
                    assert gm.basis_bytes == dt.itemsize and gm.workspace_bytes == CB.workspace_bytes(n, 8, dt.itemsize, dt.itemsize, precond)
                    gm.begin(bd.data_ptr(), xd.data_ptr(), st)
                    gm.iterate(xd.data_ptr(), 19, st)
                    gm.flush(xd.data_ptr(), st)
                    got.append((U.host(xd, n), gm.state(st)))
            for x, s in got[1:]:
                assert np.array_equal(x, got[0][0]) and s == got[0][1] and s["iterations"] == 19 and x.any()
            if dt == np.float64:
                with api.GMRES(op.A, 8, basis="float32", **kw) as gm:
                    assert gm.basis_bytes == 4 and gm.workspace_bytes == CB.workspace_bytes(n, 8, 8, 4, precond)
        for bad in (2, 3, 16, 8 if dt == np.float32 else 2, "float16"):
            with pytest.raises(ValueError):
                api.GMRES(op.A, 8, basis=bad)
        U.intact((xd, n), (bd, n), (dd, n))


def test_sparse_operator_gmres_agrees_with_the_torch_loop(torch_cuda):
    """shiftskew67 in fp64 with basis = "float32": the method and the module-level loop (a float32 basis tensor used widened) are both within 1e-8 of spsolve, as
    tests/test_gpu_gmres.py holds the plain form; with Jacobi on the column-scaled input too; a bad basis raises."""
    torch = torch_cuda
    n, rp, ci, vt, b = _system("shiftskew67")
    xs = _solved("shiftskew67")[0]
    bd = torch.from_numpy(b).cuda()
    with SparseOperator(n, n, rp, ci, vt, placement_tries=1) as op:
        x, info = op.gmres(bd, rtol=1e-12, maxiter=2000, restart=RESTART, basis="float32")
        xt, infot = torch_gmres(op, bd, tol=1e-12, maxiter=2000, restart=RESTART, basis="float32")
        print("library %s, torch loop %s" % (info, infot))
        assert info["converged"] and info["status"] == "converged" and infot["converged"], (info, infot)
        assert set(info) == {"iterations", "residual", "relative_residual", "converged", "status"}
        assert abs(info["iterations"] - infot["iterations"]) <= 8 + 3      # (the same method: the library looks every 8 iterations; 3: what rounding may move the count by)
        for got in (x.cpu().numpy(), xt.cpu().numpy()):
            assert np.linalg.norm(got - xs) <= 1e-8 * np.linalg.norm(xs), (np.linalg.norm(got - xs), info, infot)
        with pytest.raises(ValueError):
            op.gmres(bd, basis=2)
        with pytest.raises(ValueError):
            torch_gmres(op, bd, basis="float16")
    n2, rp2, ci2, v2, b2 = _system("convdiff67_colscaled")
    xs2 = _solved("convdiff67_colscaled")[0]
    b2d = torch.from_numpy(b2).cuda()
    with SparseOperator(n2, n2, rp2, ci2, v2, placement_tries=1) as op:
        dinv = torch.from_numpy(M.inverse_diagonal(n2, rp2, ci2, v2, F64)).cuda()
        xj, infoj = op.gmres(b2d, rtol=1e-12, maxiter=2000, restart=RESTART, dinv=dinv, basis=4)
        xtj, infotj = torch_gmres(op, b2d, tol=1e-12, maxiter=2000, restart=RESTART, dinv=dinv, basis=4)
        assert infoj["converged"] and infotj["converged"]
        for got in (xj.cpu().numpy(), xtj.cpu().numpy()):
            assert np.linalg.norm(got - xs2) <= 1e-8 * np.linalg.norm(xs2)
