"""The host-side driver around the kernels of the six device-resident solvers (tilespmv_{cg,cg_multi,cgls,bicgstab,minres,gmres}_{state_read,solve}; include/tilespmv.h,
DESIGN.md §3.7): the versioned state struct with a short or a long ``size``, the refusals of ``*_solve``, ``maxiter = 0``, the ``check_every < 1`` clamp, the clipping of the last
batch of iterations and the zero right-hand side.  What the iterations compute is the business of tests/test_gpu_{cg,cg_multi,cgls,bicgstab,minres,gmres}.py.

One matrix for all: the SPD tridiagonal with 2.5 on the diagonal and -1 beside it, n = 37 (odd: both builds walk the scalar tail; one workgroup), through SparseOperator
(deterministic=1, placement_tries=1), b = cg_mirror.rhs(n).  cg_multi runs with nvec = 2: column 1 is b, column 0 is b reversed, or zero where a test says "zero column"; gmres
with restart 16, as tests/test_gpu_gmres.py.
The library is called through ``op.A.lib`` with ctypes and raw byte buffers, so that state structs of any length are possible.  No case here launches anything it should not:
every refused call returns before a launch."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import cg_mirror as M
import gpu_solver_util as U
from gpu_solver_util import DTYPES, SENTINEL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api

pytestmark = pytest.mark.gpu

N, NVEC, RESTART = 37, 2, 16
SOLVERS = ["cg", "cg_multi", "cgls", "bicgstab", "minres", "gmres"]
INVALID = api.HIP_ERROR_INVALID_VALUE
FILL, GUARD = 0xA5, 32      # every byte of a state buffer before a call; bytes behind the last struct
HEAD = 3 * C.sizeof(C.c_int)   # size, iterations, status: the shortest struct state_read serves


def _tridiagonal():
    rows = np.repeat(np.arange(N), 3)
    cols = rows + np.tile([-1, 0, 1], N)
    keep = (cols >= 0) & (cols < N)
    rows, ci = rows[keep], cols[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
    return np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.where(ci == rows, 2.5, -1.0)


@pytest.fixture(scope="module")
def ops(torch_cuda):
    """The operator of each value type, shared by every test of the module."""
    rp, ci, v = _tridiagonal()
    made = {np.dtype(dt): U.square_op(N, rp, ci, v, dt) for dt in DTYPES}
    yield made
    for op in made.values():
        op.close()


@functools.lru_cache(maxsize=None)
def _column_reference(dtname):
    """For the solved column beside a zero column: (error of the numpy mirror against the direct solution, the direct solution); x0 = ones, rtol = 1e-8, computed once."""
    dt = np.dtype(dtname)
    rp, ci, v = _tridiagonal()
    vt, b = v.astype(dt), M.rhs(N).astype(dt)
    xm, _, status, _ = M.Mirror(M.scipy_csr(N, rp, ci, vt), dt).solve(b, x0=np.ones(N), rtol=1e-8, maxiter=5000, check_every=1)
    assert status == M.CONVERGED
    xs = M.spsolve_x(N, rp, ci, vt.astype(np.float64), b.astype(np.float64))
    return float(np.linalg.norm(xm.astype(np.float64) - xs) / np.linalg.norm(xs)), xs


def _vp(a):
    return C.c_void_p(a)


class Driver:
    """One solver's C entry points on the operator's plans, with the caller's bytes as the state."""

    def __init__(self, name, op, torch):
        self.name, self.lib, self.torch = name, op.A.lib, torch
        self.State = _lib.CGLSState if name == "cgls" else _lib.CGState
        self.count = NVEC if name == "cg_multi" else 1      # state structs per call
        self.damp = (0.0,) if name == "cgls" else ()
        self.tdt = U.tdt(torch, op.dtype)
        self.dt = op.dtype
        self.h = C.c_void_p()
        create = self._fn("create")
        if name == "cg_multi":
            rc = create(C.byref(self.h), op.A.h, NVEC, None)
        elif name == "cgls":
            rc = create(C.byref(self.h), op.A.h, op.AT.h, None)
        elif name == "gmres":
            rc = create(C.byref(self.h), op.A.h, RESTART, None)
        else:
            rc = create(C.byref(self.h), op.A.h, None)
        assert rc == 0 and self.h

    def _fn(self, what):
        return getattr(self.lib, "tilespmv_%s_%s" % (self.name, what))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._fn("destroy")(self.h)

    def stream(self):
        return U.stream(self.torch)

    # ---- device vectors: N elements (cg_multi: N rows of NVEC) with 16 sentinel rows behind them
    def vec(self, a):
        shape = (N, NVEC) if self.count > 1 else (N,)
        t = self.torch.full((N + 16,) + shape[1:], SENTINEL, dtype=self.tdt, device="cuda")
        t[:N].copy_(self.torch.from_numpy(np.array(np.broadcast_to(a, shape), dtype=self.dt)))
        return t

    def rhs(self, zero_column=False):
        """b; for cg_multi column 1 is b and column 0 is b reversed, or zero."""
        b = M.rhs(N)
        if self.count == 1:
            return self.vec(b)
        return self.vec(np.stack([np.zeros(N) if zero_column else b[::-1], b], axis=1))

    def bits(self, t):
        """Every bit of a device vector, sentinel rows included."""
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint64 if self.dt == np.float64 else np.uint32).copy()

    # ---- state buffers
    def buffer(self, stride, size=None):
        """``count`` structs ``stride`` bytes apart and GUARD bytes behind them, every byte FILL; then the first struct's ``size`` (default: the stride)."""
        nbytes = stride * self.count + GUARD
        buf = (C.c_ubyte * nbytes)(*([FILL] * nbytes))
        C.c_uint.from_buffer(buf).value = stride if size is None else size
        return buf

    def states(self, buf, stride):
        """The whole structs of a buffer whose stride is at least the struct's size."""
        return [self.State.from_buffer_copy(bytes(buf)[j * stride: j * stride + C.sizeof(self.State)]) for j in range(self.count)]

    # ---- the entry points
    def begin(self, b, x):
        return self._fn("begin")(self.h, _vp(b.data_ptr()), _vp(x.data_ptr()), *self.damp, _vp(self.stream()))

    def iterate(self, x, count):
        return self._fn("iterate")(self.h, _vp(x.data_ptr()), count, _vp(self.stream()))

    def current(self, x):
        """After ``iterate``, before x is read.  GMRES holds the iterate in x only after a close, and ``tilespmv_gmres_solve`` ends with a flush: so a flush;
        nothing for the others."""
        return self._fn("flush")(self.h, _vp(x.data_ptr()), _vp(self.stream())) if self.name == "gmres" else 0

    def state_read(self, buf):
        return self._fn("state_read")(self.h, _vp(self.stream()), C.cast(buf, C.POINTER(self.State)))

    def solve(self, b, x, buf, rtol, maxiter, check_every):
        return self._fn("solve")(self.h, _vp(b.data_ptr()), _vp(x.data_ptr()), *self.damp, rtol, maxiter, check_every, _vp(self.stream()), C.cast(buf, C.POINTER(self.State)))

    def solved(self, b, x, rtol, maxiter, check_every):
        """solve with whole structs: (return code, the states)."""
        full = C.sizeof(self.State)
        buf = self.buffer(full)
        rc = self.solve(b, x, buf, rtol, maxiter, check_every)
        assert bytes(buf)[full * self.count:] == bytes([FILL]) * GUARD
        return rc, self.states(buf, full)


@pytest.fixture(params=DTYPES, ids=lambda d: np.dtype(d).name)
def dt(request):
    return np.dtype(request.param)


@pytest.mark.parametrize("name", SOLVERS)
def test_state_read_serves_a_short_struct(torch_cuda, ops, name, dt):
    """size = 12: iterations and status arrive, size stays 12, and no byte from offset 12 on changes (cg_multi: the structs are 12 bytes apart, the guard behind the last one is
    untouched).  size = 8: hipErrorInvalidValue and an untouched buffer."""
    with Driver(name, ops[dt], torch_cuda) as d:
        b, x = d.rhs(), d.vec(0.0)
        assert d.begin(b, x) == 0
        for done in (0, 2):
            if done:
                assert d.iterate(x, done) == 0
            buf = d.buffer(HEAD)
            assert d.state_read(buf) == 0
            raw = bytes(buf)
            for j in range(d.count):
                assert struct.unpack_from("Iii", raw, j * HEAD) == (HEAD, done, api.CG_RUNNING), (name, j, done)
            assert raw[HEAD * d.count:] == bytes([FILL]) * GUARD
        buf = d.buffer(HEAD, size=8)
        before = bytes(buf)
        assert d.state_read(buf) == INVALID and bytes(buf) == before


def test_cg_multi_serves_a_long_stride(torch_cuda, ops, dt):
    """stride = sizeof(tilespmv_cg_state) + 8, state_read and solve: every element's size is the stride, its fields are those a call with whole structs returns, and its 8 bytes
    of padding and the guard keep their bytes."""
    full = C.sizeof(_lib.CGState)
    stride = full + 8
    with Driver("cg_multi", ops[dt], torch_cuda) as d:
        b = d.rhs()
        for call in ("state_read", "solve"):
            results = []
            for s in (full, stride):
                x, buf = d.vec(0.0), d.buffer(s)
                if call == "solve":
                    assert d.solve(b, x, buf, 1e-8, 200, 4) == 0
                else:
                    assert d.begin(b, x) == 0 and d.iterate(x, 3) == 0 and d.state_read(buf) == 0
                raw = bytes(buf)
                assert raw[s * NVEC:] == bytes([FILL]) * GUARD
                for j in range(NVEC):
                    assert raw[j * s + full: (j + 1) * s] == bytes([FILL]) * (s - full), (call, j)
                results.append([(st.size, st.iterations, st.status, st.rr, st.bb) for st in d.states(buf, s)])
            for j in range(NVEC):
                assert results[0][j][0] == full and results[1][j][0] == stride
                assert results[0][j][1:] == results[1][j][1:] and results[1][j][1] > 0, (call, j, results)
                assert results[1][j][2] == (api.CG_CONVERGED if call == "solve" else api.CG_RUNNING)


@pytest.mark.parametrize("name", SOLVERS)
def test_solve_refuses_before_it_touches_x(torch_cuda, ops, name, dt):
    """A state struct 8 bytes short of the whole one, and maxiter = -1: hipErrorInvalidValue, and x keeps its bits."""
    with Driver(name, ops[dt], torch_cuda) as d:
        full = C.sizeof(d.State)
        b, x = d.rhs(), d.vec(M.rhs(N)[::-1] if d.count == 1 else np.stack([M.rhs(N), M.rhs(N)[::-1]], axis=1))
        before = d.bits(x)
        assert d.solve(b, x, d.buffer(full, size=full - 8), 1e-8, 100, 4) == INVALID
        assert np.array_equal(d.bits(x), before)
        assert d.solve(b, x, d.buffer(full), 1e-8, -1, 4) == INVALID
        assert np.array_equal(d.bits(x), before)


@pytest.mark.parametrize("name", SOLVERS)
def test_maxiter_zero(torch_cuda, ops, name, dt):
    """maxiter = 0, b != 0, x0 = 0: success, MAXITER at 0 iterations, x keeps its bits."""
    with Driver(name, ops[dt], torch_cuda) as d:
        b, x = d.rhs(), d.vec(0.0)
        before = d.bits(x)
        rc, states = d.solved(b, x, 1e-8, 0, 4)
        assert rc == 0 and all(s.status == api.CG_MAXITER and s.iterations == 0 for s in states), [(s.status, s.iterations) for s in states]
        assert np.array_equal(d.bits(x), before)


@pytest.mark.parametrize("name", SOLVERS)
def test_check_every_below_one_is_one(torch_cuda, ops, name, dt):
    """rtol = 0, maxiter = 6: check_every = 0 and -3 give the bits of x, the iterations and the status of check_every = 1."""
    with Driver(name, ops[dt], torch_cuda) as d:
        b = d.rhs()
        got = []
        for check_every in (1, 0, -3):
            x = d.vec(0.0)
            rc, states = d.solved(b, x, 0.0, 6, check_every)
            assert rc == 0
            got.append((d.bits(x), [(s.iterations, s.status) for s in states]))
        assert got[0][1] == [(6, api.CG_MAXITER)] * d.count, got[0][1]
        for bits, st in got[1:]:
            assert st == got[0][1] and np.array_equal(bits, got[0][0])


@pytest.mark.parametrize("name", SOLVERS)
def test_the_last_batch_is_clipped(torch_cuda, ops, name, dt):
    """rtol = 0, maxiter = 10, check_every = 4: MAXITER at 10 iterations (4 + 4 + 2), and x has the bits of begin and iterate(10) on a second solver from the same x0 (gmres:
    after the flush that its solve ends with, Driver.current)."""
    x0 = M.rhs(N)[::-1] / 2 if name != "cg_multi" else np.stack([M.rhs(N) / 2, M.rhs(N)[::-1] / 2], axis=1)
    with Driver(name, ops[dt], torch_cuda) as d, Driver(name, ops[dt], torch_cuda) as d2:
        b, x, x2 = d.rhs(), d.vec(x0), d2.vec(x0)
        rc, states = d.solved(b, x, 0.0, 10, 4)
        assert rc == 0 and [(s.iterations, s.status) for s in states] == [(10, api.CG_MAXITER)] * d.count
        assert d2.begin(b, x2) == 0 and d2.iterate(x2, 10) == 0 and d2.current(x2) == 0
        assert np.array_equal(d.bits(x), d2.bits(x2))


@pytest.mark.parametrize("name", SOLVERS)
def test_zero_right_hand_side(torch_cuda, ops, name, dt):
    """b = 0 with x0 = ones: CONVERGED at 0 iterations, every element of x is +0.0; rr = 0 (cgls: nn = 0 and rr = bb).  cg_multi with the zero column: that holds for column 0,
    and column 1 is solved to rtol = 1e-8 as if it were alone: CONVERGED, and against the direct solution within 10 x the numpy mirror's own error, the bound of
    tests/test_gpu_cg_multi.py::test_solves."""
    with Driver(name, ops[dt], torch_cuda) as d:
        b, x = (d.vec(0.0) if d.count == 1 else d.rhs(zero_column=True)), d.vec(1.0)
        rc, states = d.solved(b, x, 1e-8, 200, 1)
        assert rc == 0
        xb = d.bits(x)
        s = states[0]
        assert s.status == api.CG_CONVERGED and s.iterations == 0, (s.status, s.iterations)
        assert not xb[:N].reshape(N, -1)[:, 0].any()
        if name == "cgls":
            assert s.nn == 0.0 and s.rr == s.bb
        else:
            assert s.rr == 0.0
        if d.count > 1:
            errm, xs = _column_reference(dt.name)
            s1, x1 = states[1], x.cpu().numpy()[:N, 1].astype(np.float64)
            err = float(np.linalg.norm(x1 - xs) / np.linalg.norm(xs))
            print("%s column 1 beside a zero column: %d iterations, sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s1.iterations, (s1.rr / s1.bb) ** 0.5, err, errm))
            assert s1.status == api.CG_CONVERGED and s1.iterations > 0 and s1.rr <= 1e-8 * 1e-8 * s1.bb
            assert err <= 10 * errm, (err, errm)
        U.intact((x, N))
