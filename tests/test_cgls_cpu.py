"""The least-squares solver in the library (tilespmv_cgls_*, tilespmv_csr_row_sqnorms_device), as far as it can be checked without a GPU: the C ABI is there and
refuses what it must without a device, the compiler made spill-free kernels of hip_solver_ls.hip and few of them, and the numpy mirror that tests/test_gpu_cgls.py compares the GPU
with (tests/cgls_mirror.py) is itself right on the inputs of those tests — checked here so that a GPU visit is not spent finding out."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

import cgls_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_cgls_create", "tilespmv_cgls_destroy", "tilespmv_cgls_begin", "tilespmv_cgls_iterate", "tilespmv_cgls_state_read", "tilespmv_cgls_solve",
               "tilespmv_csr_row_sqnorms_device"]
MAX_SOLVER_KERNELS = 10
DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_solver_symbols_are_exported_and_null_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    h = C.c_void_p(12345)
    assert lib.tilespmv_cgls_create(C.byref(h), None, None, None) == HIP_ERROR_INVALID_VALUE      # (no HIP call: this machine has no device to fail on)
    assert not h
    assert lib.tilespmv_cgls_create(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_cgls_destroy(None)
    st = _lib.CGLSState()
    assert C.sizeof(st) == 48 and st.size == 48
    assert lib.tilespmv_cgls_begin(None, None, None, 0.0, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cgls_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cgls_state_read(None, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cgls_solve(None, None, None, 0.0, 1e-8, 10, 8, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_csr_row_sqnorms_device(4, None, None, None, None, 1, None) == HIP_ERROR_INVALID_VALUE


def test_the_row_norm_entry_point_fails_loudly_without_a_device():
    """No device visible: an error code comes back, the process neither aborts nor pretends."""
    code = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r)
from tilespmv_amd import _lib
for dt in (np.float64, np.float32):
    lib = _lib.load(dt)
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    for src in (a, None):
        rc = lib.tilespmv_csr_row_sqnorms_device(4, a, src, a, a, 1, None)
        print("RC", rc)
        assert rc != 0
print("DONE")
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout and r.stdout.count("RC") == 4, r.stdout


def test_no_solver_kernel_spills_and_there_are_few_of_them(tmp_path):
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver_ls.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert 5 <= len(spills) <= MAX_SOLVER_KERNELS, (dt, names)
        for want in ("k_ls_dot", "k_ls_update", "k_ls_normal", "k_ls_direction", "k_csr_row_sqnorms"):
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the vectors travel as 16-byte lane accesses


# ---- the mirror on the inputs of the GPU tests.  Counts printed by these tests on the machine they were written on (rtol = RTOL, check_every = 1):
#   tall          fp64 26 it, error vs lsqr 1.2e-10        fp32 13 it, 8.6e-6        damp 2: 24 / 12 it, 5.9e-11 / 6.4e-6
#   wide          fp64 34 it, 1.2e-10 (minimum norm)       fp32 17 it, 1.1e-5        damp 2: 20 / 10 it, 1.1e-10 / 9.6e-6
#   tall_scaled   cinv: fp64 23 it, fp32 12 it;  without cinv at 4 x that many: sqrt(nn/nn0) 0.081 / 0.115
#   square        fp64 97 it, 3.0e-10                      fp32 47 it, 2.9e-5
#   stacked       fp64 91 it, 2.4e-10                      fp32 44 it, 2.9e-5
COUNTS = {("tall", 0.0): (26, 13), ("tall", 2.0): (24, 12), ("wide", 0.0): (34, 17), ("wide", 2.0): (20, 10), ("tall_scaled", 0.0): (23, 12)}
FEW = 3


def _system(name, dtype):
    dt = np.dtype(dtype)
    rows, cols, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(rows).astype(dt)
    return M.scipy_csr(rows, cols, rp, ci, vt), b


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,damp", [("tall", 0.0), ("tall", 2.0), ("wide", 0.0), ("wide", 2.0)])
def test_the_mirror_converges_to_the_lsqr_solution(name, damp, dtype):
    dt = np.dtype(dtype)
    A, b = _system(name, dt)
    xs = M.lsqr_x(A, b, damp)
    x, it, status, rel = M.Mirror(A, dt).solve(b, damp=damp, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    err = _relerr(x, xs)
    want = COUNTS[(name, damp)][dt == np.float32]
    print("%s %s damp %g: %d iterations (recorded %d), status %d, sqrt(nn/nn0) %.3g, error vs lsqr %.3g" % (name, dt, damp, it, want, status, rel, err))
    assert status == M.CONVERGED and rel <= M.RTOL[dt]
    assert abs(it - want) <= FEW
    assert err <= 100 * M.RTOL[dt]
    # the recurrence's nn and rr are the true ones while the solve is healthy
    m = M.Mirror(A, dt); m.begin(b, damp=damp); m.iterate(3)
    A64, x64 = A.astype(np.float64), m.x.astype(np.float64)
    r64 = b.astype(np.float64) - A64 @ x64
    true_rr, true_nn = float(r64 @ r64), float(np.sum((A64.T @ r64 - damp * damp * x64) ** 2))
    assert abs(m.rr - true_rr) <= 1e-3 * true_rr and abs(m.nn - true_nn) <= 1e-3 * true_nn


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["square", "stacked"])
def test_the_chosen_square_and_stacked_inputs_qualify(name, dtype):
    """The condition on the two inputs the implementer chose: the mirror converges in fewer than 1000 iterations in both types (and to the right solution)."""
    dt = np.dtype(dtype)
    A, b = _system(name, dt)
    if name == "square":
        import scipy.sparse.linalg as spla
        xs = spla.spsolve(A.astype(np.float64).tocsc(), b.astype(np.float64))
    else:
        xs = M.lsqr_x(A, b)
    x, it, status, rel = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=1000, check_every=1)
    err = _relerr(x, xs)
    print("%s %s: %d iterations, status %d, sqrt(nn/nn0) %.3g, error %.3g" % (name, dt, it, status, rel, err))
    assert status == M.CONVERGED and 0 < it < 1000 and rel <= M.RTOL[dt]
    assert err <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_the_scaled_input_only_column_scaling_converges(dtype):
    """What makes the GPU column-scaling test mean something: with cinv = 1 / |a_j|^2 the mirror converges, without it it does not inside 4 x that count."""
    dt = np.dtype(dtype)
    A, b = _system("tall_scaled", dt)
    xs = M.lsqr_x(A, b, scale_columns=True)
    x, it, status, rel = M.Mirror(A, dt, M.column_cinv(A, dt)).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    err = _relerr(x, xs)
    want = COUNTS[("tall_scaled", 0.0)][dt == np.float32]
    print("tall_scaled %s cinv: %d iterations (recorded %d), status %d, sqrt(nn/nn0) %.3g, error vs lsqr %.3g" % (dt, it, want, status, rel, err))
    assert status == M.CONVERGED and abs(it - want) <= FEW and err <= 100 * M.RTOL[dt]
    x2, it2, status2, rel2 = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=4 * it, check_every=1)
    print("tall_scaled %s plain: %d iterations, status %d, sqrt(nn/nn0) %.3g" % (dt, it2, status2, rel2))
    assert status2 == M.MAXITER and it2 == 4 * it and rel2 > 1e3 * M.RTOL[dt]


def test_the_mirror_guards():
    """b = 0; b orthogonal to the range of A; a negative cinv; an exactly zero normal residual after one iteration (A = 2 I)."""
    n = 4099
    b = M.rhs(n)
    I2 = sp.identity(n, format="csr") * 2.0
    m = M.Mirror(I2, np.float64)
    x, it, status, rel = m.solve(np.zeros(n), rtol=1e-10)
    assert it == 0 and status == M.CONVERGED and not x.any()
    m.begin(np.zeros(n)); m.iterate(16)
    assert not m.x.any() and m.nn == 0.0 and np.isfinite(m.p).all() and m.status() == M.CONVERGED
    A, bo = M.orthogonal_case(n, np.float64)
    x, it, status, rel = M.Mirror(A, np.float64).solve(bo, x0=b, rtol=1e-10)
    assert it == 0 and status == M.CONVERGED and not x.any()
    m.begin(b); m.iterate(1)
    assert np.array_equal(m.x, b / 2) and m.nn == 0.0 and m.rr == 0.0
    x1 = m.x.copy(); m.iterate(16)
    assert np.array_equal(m.x, x1) and m.status() == M.CONVERGED and m.iterations == 17
    At, bt = _system("tall", np.float64)
    x0 = M.rhs(At.shape[1])[::-1].copy()
    x, it, status, rel = M.Mirror(At, np.float64, -M.column_cinv(At, np.float64)).solve(bt, x0=x0, rtol=1e-10, maxiter=100)
    assert status == M.BREAKDOWN and it == 8 and np.array_equal(x, x0)
