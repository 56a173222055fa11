"""The BiCGStab solver in the library (tilespmv_bicgstab_*), as far as it can be checked without a GPU: the C ABI is there and refuses what it must without a
device, the compiler made spill-free kernels of hip_solver_bi.hip and few of them, and the numpy mirror that tests/test_gpu_bicgstab.py compares the GPU with
(tests/bicgstab_mirror.py) is itself right on the inputs of those tests — checked here so that a GPU visit is not spent finding out."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_bicgstab_create", "tilespmv_bicgstab_destroy", "tilespmv_bicgstab_begin", "tilespmv_bicgstab_iterate", "tilespmv_bicgstab_state_read",
               "tilespmv_bicgstab_solve"]
ITERATION_KERNELS = ("k_bi_dot1", "k_bi_half", "k_bi_dot2", "k_bi_update", "k_bi_direction")
MAX_SOLVER_KERNELS = 8      # the five of an iteration, k_bi_begin and its fold, and one to spare
DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_solver_symbols_are_exported_and_null_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    assert "typedef struct tilespmv_bicgstab tilespmv_bicgstab;" in header      # (the seventh name of the interface: the opaque handle)
    h = C.c_void_p(12345)
    assert lib.tilespmv_bicgstab_create(C.byref(h), None, None) == HIP_ERROR_INVALID_VALUE      # (no HIP call: this machine has no device to fail on)
    assert not h
    assert lib.tilespmv_bicgstab_create(None, None, None) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_bicgstab_destroy(None)
    st = _lib.CGState()
    assert lib.tilespmv_bicgstab_begin(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_bicgstab_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_bicgstab_state_read(None, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_bicgstab_solve(None, None, None, 1e-8, 10, 8, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE


def test_no_solver_kernel_spills_and_there_are_few_of_them(tmp_path):
    assert "hip_solver_bi.hip" in open(os.path.join(ROOT, "tilespmv_amd/csrc/Makefile")).read()
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver_bi.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert len(ITERATION_KERNELS) <= len(spills) <= MAX_SOLVER_KERNELS, (dt, names)
        for want in ITERATION_KERNELS:
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the vectors travel as 16-byte lane accesses


# ---- the mirror on the inputs of the GPU tests.  Printed by these tests on the machine they were written on (rtol = RTOL, check_every = 1):
#   convdiff67          fp64 110 it, error vs spsolve 6.1e-11      fp32 93 it, 3.2e-5
#   convdiff67_scaled   Jacobi: fp64 118 it, 1.3e-12; fp32 117 it, 1.9e-6;  plain at 4 x that many: sqrt(rr/bb) 0.34 / 0.28
#   dots in a permuted order: 110 / 93 and 119 / 117 iterations
COUNTS = {"convdiff67": (110, 93), "convdiff67_scaled": (118, 117)}
FEW = 3


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    dinv = M.inverse_diagonal(n, rp, ci, vt, dt) if name.endswith("_scaled") else None
    return M.scipy_csr(n, rp, ci, vt), b, dinv, M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def test_the_convection_diffusion_input_is_what_it_says():
    n, rp, ci, v = M.problem("convdiff67")
    A = M.scipy_csr(n, rp, ci, v)
    assert n == 4489 and n % 4 == 1 and abs(A - A.T).max() > 0.5
    i = 67 * 33 + 20      # an inner grid point
    assert (A[i, i], A[i, i - 1], A[i, i + 1], A[i, i - 67], A[i, i + 67]) == (4.0, -1.6, -0.4, -1.3, -0.7)
    assert A[66, 67] == 0 and A[67, 66] == 0      # (no coupling across the end of a grid row)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["convdiff67", "convdiff67_scaled"])
def test_the_mirror_converges_to_the_direct_solution(name, dtype):
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system(name, dt)
    x, it, status, rel = M.Mirror(A, dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    err = _relerr(x, xs)
    want = COUNTS[name][dt == np.float32]
    print("%s %s: %d iterations (recorded %d), status %d, sqrt(rr/bb) %.3g, error vs spsolve %.3g" % (name, dt, it, want, status, rel, err))
    assert status == M.CONVERGED and rel <= M.RTOL[dt]
    assert abs(it - want) <= FEW
    assert err <= 100 * M.RTOL[dt]
    # the recurrence's rr is the true one while the solve is healthy
    m = M.Mirror(A, dt, dinv); m.begin(b); m.iterate(3)
    r64 = b.astype(np.float64) - A.astype(np.float64) @ m.x.astype(np.float64)
    true_rr = float(r64 @ r64)
    assert m.iterations == 3 and m.status() == M.RUNNING and abs(m.rr - true_rr) <= 1e-3 * true_rr


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_the_scaled_input_only_jacobi_converges(dtype):
    """What makes the GPU Jacobi test mean something: with dinv the mirror converges, without it it does not inside 4 x that count."""
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system("convdiff67_scaled", dt)
    x, it, status, rel = M.Mirror(A, dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    assert status == M.CONVERGED
    x2, it2, status2, rel2 = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=4 * it, check_every=1)
    print("convdiff67_scaled %s: Jacobi %d iterations; plain %d iterations, status %d, sqrt(rr/bb) %.3g" % (dt, it, it2, status2, rel2))
    assert status2 == M.MAXITER and it2 == 4 * it and rel2 > 1e3 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["convdiff67", "convdiff67_scaled"])
def test_another_order_of_the_sums_costs_few_iterations(name, dtype):
    """The mirror with its dot products accumulated in a permuted order converges within 1.25 x the unpermuted count: the GPU (whose sums have yet another order) may be capped at
    2 x the mirror's count without the cap ever cutting off a correct solver."""
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system(name, dt)
    x, it, status, rel = M.Mirror(A, dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    order = np.random.default_rng(11).permutation(A.shape[0])
    xp, itp, statusp, relp = M.Mirror(A, dt, dinv, order=order).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    print("%s %s: %d iterations, %d with permuted sums; |x - x_permuted| / |x| = %.3g" % (name, dt, it, itp, _relerr(xp, x.astype(np.float64))))
    assert status == M.CONVERGED and statusp == M.CONVERGED
    assert itp <= 1.25 * it
    assert _relerr(xp, xs) <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mirror_guards(dtype):
    """b = 0; an exactly zero residual at the half step (A = 2 I); sigma = 0 exactly (skew); omega = 0 with a live residual; maxiter cuts the last block."""
    dt = np.dtype(dtype)
    # b = 0
    n, rp, ci, v = M.problem("2I")
    I2 = M.scipy_csr(n, rp, ci, v)
    b = M.rhs(n).astype(dt)
    m = M.Mirror(I2, dt)
    x, it, status, rel = m.solve(np.zeros(n), x0=b, rtol=M.RTOL[dt])
    assert it == 0 and status == M.CONVERGED and not x.any()
    m.begin(np.zeros(n)); m.iterate(16)
    assert m.iterations == 16 and not m.x.any() and m.rr == 0.0 and np.isfinite(m.p).all() and m.status() == M.CONVERGED
    # A = 2 I: alpha = 1/2 exactly, s = 0, t.t = 0 -> omega = 0, converged at the half step
    m.begin(b); m.iterate(1)
    assert np.array_equal(m.x, b / dt.type(2)) and m.rr == 0.0 and m.status() == M.CONVERGED
    x1, p1 = m.x.copy(), m.p.copy(); m.iterate(16)
    assert np.array_equal(m.x, x1) and np.array_equal(m.p, p1) and m.status() == M.CONVERGED and m.iterations == 17
    # skew: rhat.v = b.A b = 0 in the first iteration
    n, rp, ci, v = M.problem("skew")
    A, bs = M.scipy_csr(n, rp, ci, v), M.skew_rhs(n)
    assert n == 4098 and abs(A + A.T).max() == 0 and bs.any() and np.abs(bs).max() <= 8 and np.array_equal(bs, np.round(bs))
    x0 = np.zeros(n)
    x, it, status, rel = M.Mirror(A, dt).solve(bs, x0=x0, rtol=M.RTOL[dt], maxiter=100, check_every=8)
    assert status == M.BREAKDOWN and it == 8 and np.array_equal(x, x0)
    m = M.Mirror(A, dt); m.begin(bs); m.iterate(1)
    assert m.breakdown and np.array_equal(m.r, bs.astype(dt)) and np.array_equal(m.p, bs.astype(dt))
    # omega = 0 with a live residual.  In exact arithmetic a Krylov residual does not land there from begin, so the state is set by hand: A = diag(1, 0), r = (1, 1),
    # rhat = p = (1, 0): v = (1, 0), sigma = rho = 1, alpha = 1, s = (0, 1), t = A s = 0 -> omega = 0, x += p, r = s, rr = 1 > 0: breakdown, p as it was
    m = M.Mirror(sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 0.0]])), dt); m.begin(np.array([1.0, 1.0]))
    m.rhat, m.p, m.rho = np.array([1, 0], dtype=dt), np.array([1, 0], dtype=dt), 1.0
    m.iterate(1)
    assert m.breakdown and m.status() == M.BREAKDOWN and np.array_equal(m.x, [1, 0]) and np.array_equal(m.r, [0, 1]) and m.rr == 1.0 and np.array_equal(m.p, [1, 0])
    x1 = m.x.copy(); m.iterate(7)
    assert m.iterations == 8 and np.array_equal(m.x, x1)
    # maxiter cuts the last block of check_every
    Ac, bc, _, _ = _system("convdiff67", dt)
    x, it, status, rel = M.Mirror(Ac, dt).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=8)
    assert it == 13 and status == M.MAXITER
    x, it, status, rel = M.Mirror(Ac, dt).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=0)
    assert it == 13 and status == M.MAXITER
