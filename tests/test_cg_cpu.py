"""The solver in the library (tilespmv_cg_*), as far as it can be checked without a GPU: the C ABI is there and refuses what it must without a device, the
compiler made spill-free kernels of hip_solver.hip and few of them, and the numpy mirror that tests/test_gpu_cg.py compares the GPU with (tests/cg_mirror.py) is itself right on
the inputs of those tests — checked here so that a GPU visit is not spent finding out."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cg_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_cg_create", "tilespmv_cg_destroy", "tilespmv_cg_begin", "tilespmv_cg_iterate", "tilespmv_cg_state_read", "tilespmv_cg_solve",
               "tilespmv_csr_diagonal_device"]
MAX_SOLVER_KERNELS = 8


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_solver_symbols_are_exported_and_null_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    h = C.c_void_p(12345)
    assert lib.tilespmv_cg_create(C.byref(h), None, None) == HIP_ERROR_INVALID_VALUE      # (no HIP call: this machine has no device to fail on)
    assert not h
    assert lib.tilespmv_cg_create(None, None, None) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_cg_destroy(None)
    st = _lib.CGState()
    assert C.sizeof(st) == 32 and st.size == 32
    assert lib.tilespmv_cg_begin(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_state_read(None, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_solve(None, None, None, 1e-8, 10, 8, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_csr_diagonal_device(4, None, None, None, None, 1, None) == HIP_ERROR_INVALID_VALUE


def test_the_diagonal_entry_point_fails_loudly_without_a_device():
    """No device visible: an error code comes back, the process neither aborts nor pretends."""
    code = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r)
from tilespmv_amd import _lib
for dt in (np.float64, np.float32):
    lib = _lib.load(dt)
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    rc = lib.tilespmv_csr_diagonal_device(4, a, a, a, a, 1, None)
    print("RC", rc)
    assert rc != 0
print("DONE")
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "DONE" in r.stdout and r.stdout.count("RC") == 2, r.stdout


def test_no_solver_kernel_spills_and_there_are_few_of_them(tmp_path):
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert 4 <= len(spills) <= MAX_SOLVER_KERNELS, (dt, names)
        for want in ("k_cg_dot", "k_cg_update", "k_cg_direction", "k_csr_diagonal"):
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the vectors travel as 16-byte lane accesses


# ---- the mirror on the inputs of the GPU tests.  Counts printed by this test on the machine it was written on (check_every = 1):
#   lap128         fp64 444 it, error vs spsolve 2.1e-10     fp32 291 it, 3.0e-5
#   tri200         fp64  35 it, 1.6e-10                      fp32  18 it, 1.1e-5
#   fem12          fp64  55 it (Jacobi 47), 2.2e-10          fp32  34 it (Jacobi 30), 3.1e-5
#   lap128_scaled  fp64 plain: not in 5000 (rel 1.04); Jacobi 495 it, 2.2e-12      fp32 plain: not in 5000; Jacobi 349 it, 8.7e-7
def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    A = M.scipy_csr(n, rp, ci, vt)
    xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))   # the solution of the system in the value type's own numbers
    return n, A, b, xs


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["lap128", "tri200", "fem12"])
def test_the_mirror_converges_to_the_direct_solution(name, dtype):
    dt = np.dtype(dtype)
    n, A, b, xs = _system(name, dt)
    for jacobi in (False, True):
        dinv = (1.0 / A.diagonal()).astype(dt) if jacobi else None
        x, it, status, rel = M.Mirror(A, dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
        err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
        print("%s %s %s: %d iterations, status %d, sqrt(rr/bb) %.3g, error vs spsolve %.3g" % (name, dt, "jacobi" if jacobi else "plain", it, status, rel, err))
        assert status == M.CONVERGED and rel <= M.RTOL[dt]
        assert 0 < it < 1000
        assert err <= 100 * M.RTOL[dt]      # (condition numbers of a few thousand at most: the error follows the residual within two decades)
    # the recurrence's |r|^2 is the true one while the solve is healthy
    m = M.Mirror(A, dt); m.begin(b); m.iterate(5)
    true_rr = float(np.sum((b.astype(np.float64) - A.astype(np.float64) @ m.x.astype(np.float64)) ** 2))
    assert abs(m.rr - true_rr) <= 1e-3 * true_rr


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_on_the_scaled_laplacian_only_jacobi_converges(dtype):
    """What makes the GPU Jacobi test mean something: with the preconditioner the mirror converges, without it it does not inside 4 x the Jacobi count."""
    dt = np.dtype(dtype)
    n, A, b, xs = _system("lap128_scaled", dt)
    dinv = (1.0 / A.diagonal()).astype(dt)
    x, it, status, rel = M.Mirror(A, dt, dinv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print("lap128_scaled %s jacobi: %d iterations, status %d, sqrt(rr/bb) %.3g, error vs spsolve %.3g" % (dt, it, status, rel, err))
    assert status == M.CONVERGED and 0 < it < 1000 and err <= 100 * M.RTOL[dt]
    x2, it2, status2, rel2 = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=4 * it, check_every=1)
    print("lap128_scaled %s plain: %d iterations, status %d, sqrt(rr/bb) %.3g" % (dt, it2, status2, rel2))
    assert status2 == M.MAXITER and it2 == 4 * it and rel2 > 1e3 * M.RTOL[dt]


def test_the_mirror_guards():
    """b = 0; an exactly zero residual after one iteration (A = 2 I); a negative definite matrix."""
    import scipy.sparse as sp
    n = 4096
    b = M.rhs(n)
    m = M.Mirror(sp.identity(n, format="csr") * 2.0, np.float64)
    x, it, status, rel = m.solve(np.zeros(n), rtol=1e-10)
    assert it == 0 and status == M.CONVERGED and not x.any()
    m.begin(np.zeros(n)); m.iterate(16)
    assert not m.x.any() and m.rr == 0.0 and np.isfinite(m.p).all()
    m.begin(b); m.iterate(1)
    assert np.array_equal(m.x, b / 2) and m.rr == 0.0
    x1 = m.x.copy(); m.iterate(16)
    assert np.array_equal(m.x, x1) and m.status() == M.CONVERGED
    nl, rp, ci, v = M.problem("lap128")
    x0 = M.rhs(nl)[::-1].copy()
    x, it, status, rel = M.Mirror(M.scipy_csr(nl, rp, ci, -v), np.float64).solve(M.rhs(nl), x0=x0, rtol=1e-10, maxiter=100)
    assert status == M.BREAKDOWN and it == 8 and np.array_equal(x, x0)
