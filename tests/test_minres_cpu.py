"""The MINRES solver in the library (tilespmv_minres_*, tilespmv_csr_abs_diagonal_device), as far as it can be checked without a GPU: the C ABI is there and
refuses what it must without a device, the compiler made spill-free kernels of hip_solver_mr.hip and few of them, and the numpy mirror that tests/test_gpu_minres.py compares the
GPU with (tests/minres_mirror.py) is itself right on the inputs of those tests — checked here so that a GPU visit is not spent finding out."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import cg_mirror as CM
import minres_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_minres_create", "tilespmv_minres_destroy", "tilespmv_minres_begin", "tilespmv_minres_iterate", "tilespmv_minres_state_read", "tilespmv_minres_solve",
               "tilespmv_csr_abs_diagonal_device"]
ITERATION_KERNELS = ("k_mr_dot", "k_mr_lanczos", "k_mr_update")
MAX_SOLVER_KERNELS = 7      # the three of an iteration, k_mr_begin and its fold, k_csr_abs_diagonal, and one to spare
DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_solver_symbols_are_exported_and_null_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    assert "typedef struct tilespmv_minres tilespmv_minres;" in header
    h = C.c_void_p(12345)
    assert lib.tilespmv_minres_create(C.byref(h), None, None) == HIP_ERROR_INVALID_VALUE      # (no HIP call: this machine has no device to fail on)
    assert not h
    assert lib.tilespmv_minres_create(None, None, None) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_minres_destroy(None)
    st = _lib.CGState()
    assert lib.tilespmv_minres_begin(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_minres_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_minres_state_read(None, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_minres_solve(None, None, None, 1e-8, 10, 8, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_csr_abs_diagonal_device(4, None, None, None, None, 1, None) == HIP_ERROR_INVALID_VALUE


def test_no_solver_kernel_spills_and_there_are_few_of_them(tmp_path):
    assert "hip_solver_mr.hip" in open(os.path.join(ROOT, "tilespmv_amd/csrc/Makefile")).read()
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver_mr.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert len(ITERATION_KERNELS) <= len(spills) <= MAX_SOLVER_KERNELS, (dt, names)
        for want in ITERATION_KERNELS:
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the vectors travel as 16-byte lane accesses


# ---- the mirror on the inputs of the GPU tests.  Recorded on the CPU (rtol = RTOL, check_every = 1):
#   saddle47            fp64 333 it, error vs spsolve 3.6e-10      fp32 201 it, 8.3e-5
#   saddlec47_scaled    minv = 1 / |diag|: fp64 247 it, 4.2e-10; fp32 148 it, 5.2e-5;  plain at 4 x that many: sqrt(rr/bb) 0.67 / 0.71
#   dots in a permuted order: the same counts
COUNTS = {"saddle47": (333, 201), "saddlec47_scaled": (247, 148)}
FEW = 3


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    minv = M.inverse_abs_diagonal(n, rp, ci, vt, dt) if name.endswith("_scaled") else None
    return M.scipy_csr(n, rp, ci, vt), b, minv, M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def test_the_saddle_point_inputs_are_what_they_say():
    n, rp, ci, v = M.problem("saddle47")
    K = M.scipy_csr(n, rp, ci, v)
    assert n == 2761 and n % 4 == 1 and len(ci) == 13065 and abs(K - K.T).max() == 0
    nh = 47 * 47
    assert K[nh:, nh:].nnz == 0 and K[nh + 5, 20] == 1.0 and K[nh + 5, 22] == -1.0 and K[20, nh + 5] == 1.0 and K[nh + 5].nnz == 2
    i = 47 * 20 + 11
    assert (K[i, i], K[i, i - 1], K[i, i + 1], K[i, i - 47], K[i, i + 47]) == (4.0, -1.0, -1.0, -1.0, -1.0)
    w = np.linalg.eigvalsh(K.toarray())
    print("saddle47 spectrum: [%.4g, %.4g] u [%.4g, %.4g], %d negative" % (w[w < 0].min(), w[w < 0].max(), w[w > 0].min(), w[w > 0].max(), (w < 0).sum()))
    assert (w < 0).sum() == 552 and abs(w[w < 0].min() + 0.710) < 1e-3 and abs(w[w < 0].max() + 0.450) < 1e-3 and abs(w[w > 0].min() - 0.0151) < 1e-4 and abs(w.max() - 7.992) < 1e-3
    nc, rpc, cic, vc = M.problem("saddlec47")
    Kc = M.scipy_csr(nc, rpc, cic, vc)
    assert nc == n and (Kc.diagonal()[nh:] == -1.0).all() and (Kc.diagonal() < 0).sum() == 552 and abs(Kc - Kc.T).max() == 0
    ns, rps, cis, vs = M.problem("saddlec47_scaled")
    assert np.array_equal(rps, rpc) and np.array_equal(cis, cic)      # (the same pattern: a value refresh leads from one to the other)
    Ks = M.scipy_csr(ns, rps, cis, vs)
    d = np.abs(Ks.diagonal())
    assert (Ks.diagonal() < 0).sum() == 552 and d.max() / d.min() > 1e4 and abs(Ks - Ks.T).max() <= 1e-12 * abs(Ks).max()
    # the tridiagonal of the size tests
    n3, rp3, ci3, v3 = M.indefinite_tridiagonal(9)
    T = M.scipy_csr(n3, rp3, ci3, v3).toarray()
    assert np.array_equal(T, T.T) and np.array_equal(np.diag(T), [3, -3, 3, -3, 3, -3, 3, -3, 3]) and (np.diag(T, 1) == -1).all()
    w3 = np.linalg.eigvalsh(T)
    assert (np.abs(w3) >= 1).all() and (np.abs(w3) <= 5).all() and (w3 < 0).any() and (w3 > 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["saddle47", "saddlec47_scaled"])
def test_the_mirror_converges_to_the_direct_solution(name, dtype):
    dt = np.dtype(dtype)
    A, b, minv, xs = _system(name, dt)
    m = M.Mirror(A, dt, minv)
    x, it, status, rel = m.solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    err = _relerr(x, xs)
    want = COUNTS[name][dt == np.float32]
    print("%s %s: %d iterations (recorded %d), status %d, sqrt(rr/bb) %.3g, error vs spsolve %.3g" % (name, dt, it, want, status, rel, err))
    assert status == M.CONVERGED and rel <= M.RTOL[dt]
    assert abs(it - want) <= FEW
    assert err <= 100 * M.RTOL[dt]
    # MINRES: rr never increases
    assert len(m.history) == it + 1 and all(a >= c for a, c in zip(m.history, m.history[1:]))
    # the recurrence's rr is the true one while the solve is healthy (unpreconditioned: rr = |r|^2)
    m = M.Mirror(A, dt); m.begin(b); m.iterate(3)
    r64 = b.astype(np.float64) - A.astype(np.float64) @ m.x.astype(np.float64)
    true_rr = float(r64 @ r64)
    assert m.iterations == 3 and m.status() == M.RUNNING and abs(m.rr - true_rr) <= 1e-3 * true_rr


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_the_scaled_input_only_the_preconditioned_run_converges(dtype):
    """What makes the GPU test of minv mean something: with minv = 1 / |diag| the mirror converges, without it it does not inside 4 x that count."""
    dt = np.dtype(dtype)
    A, b, minv, xs = _system("saddlec47_scaled", dt)
    x, it, status, rel = M.Mirror(A, dt, minv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    assert status == M.CONVERGED
    x2, it2, status2, rel2 = M.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=4 * it, check_every=1)
    print("saddlec47_scaled %s: preconditioned %d iterations; plain %d iterations, status %d, sqrt(rr/bb) %.3g" % (dt, it, it2, status2, rel2))
    assert status2 == M.MAXITER and it2 == 4 * it and rel2 > 1e3 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["saddle47", "saddlec47_scaled"])
def test_another_order_of_the_sums_costs_few_iterations(name, dtype):
    """The mirror with its dot products accumulated in a permuted order converges within 1.25 x the unpermuted count: the GPU (whose sums have yet another order) may be capped at
    2 x the mirror's count without the cap ever cutting off a correct solver."""
    dt = np.dtype(dtype)
    A, b, minv, xs = _system(name, dt)
    x, it, status, rel = M.Mirror(A, dt, minv).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    order = np.random.default_rng(11).permutation(A.shape[0])
    xp, itp, statusp, relp = M.Mirror(A, dt, minv, order=order).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    print("%s %s: %d iterations, %d with permuted sums; |x - x_permuted| / |x| = %.3g" % (name, dt, it, itp, _relerr(xp, x.astype(np.float64))))
    assert status == M.CONVERGED and statusp == M.CONVERGED
    assert itp <= 1.25 * it
    assert _relerr(xp, xs) <= 100 * M.RTOL[dt]


def test_the_mirror_agrees_with_scipy_minres():
    dt = np.dtype(np.float64)
    A, b, _, xs = _system("saddle47", dt)
    x, it, status, rel = M.Mirror(A, dt).solve(b, rtol=1e-12, maxiter=2000, check_every=1)
    try:
        xsc, info = spla.minres(A, b, rtol=1e-12, maxiter=2000)
    except TypeError:      # (older scipy names the tolerance tol)
        xsc, info = spla.minres(A, b, tol=1e-12, maxiter=2000)
    print("saddle47: mirror %d iterations; |x - scipy's| / |x| = %.3g" % (it, _relerr(x, xsc)))
    assert status == M.CONVERGED and info == 0 and _relerr(x, xsc) <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mirror_guards(dtype):
    """b = 0; the lucky termination, exact (pow2I); gamma = 0 exactly (singular); a minv that is not positive; maxiter cuts the last block."""
    dt = np.dtype(dtype)
    # b = 0
    n, rp, ci, v = M.problem("pow2I")
    I2 = M.scipy_csr(n, rp, ci, v)
    m = M.Mirror(I2, dt)
    x, it, status, rel = m.solve(np.zeros(n), x0=M.rhs(n), rtol=M.RTOL[dt])
    assert it == 0 and status == M.CONVERGED and not x.any()
    m.begin(np.zeros(n)); m.iterate(16)
    assert m.iterations == 16 and not m.x.any() and m.rr == 0.0 and np.isfinite(m.w).all() and m.status() == M.CONVERGED
    # pow2I, b = 8: every quantity is exact in both value types
    b8 = np.full(n, 8.0)
    m.begin(b8)
    assert m.bb == 262144.0 and m.rr == 262144.0 and m.beta == 512.0 and m.status() == M.RUNNING
    m.iterate(1)
    assert m.alfa == 2.0 and np.array_equal(m.x, np.full(n, 4.0)) and m.rr == 0.0 and m.status() == M.CONVERGED and m.iterations == 1
    x1 = m.x.copy(); m.iterate(16)
    assert np.array_equal(m.x, x1) and m.status() == M.CONVERGED and m.iterations == 17 and m.rr == 0.0
    # minv = -1: r2.z < 0 in begin
    x0 = M.rhs(n).astype(dt)
    x, it, status, rel = M.Mirror(I2, dt, -np.ones(n)).solve(b8, x0=x0, rtol=M.RTOL[dt], maxiter=100)
    assert status == M.BREAKDOWN and it == 0 and np.array_equal(x, x0)
    m = M.Mirror(I2, dt, -np.ones(n)); m.begin(b8, x0); m.iterate(5)
    assert m.status() == M.BREAKDOWN and m.iterations == 5 and np.array_equal(m.x, x0)
    # singular: A b = 0 exactly, so alfa = 0, y = 0, beta' = 0 and gamma = 0 in the first iteration
    n, rp, ci, v = M.problem("singular")
    A, bs = M.scipy_csr(n, rp, ci, v), M.singular_rhs(n)
    assert n == 4098 and (A.diagonal()[:2049] == 2).all() and np.diff(rp)[2049:].sum() == 0 and not (A @ bs).any() and bs.sum() == 2049
    x0 = np.zeros(n, dtype=dt)
    x, it, status, rel = M.Mirror(A, dt).solve(bs, x0=x0, rtol=M.RTOL[dt], maxiter=100, check_every=8)
    assert status == M.BREAKDOWN and it == 8 and np.array_equal(x, x0)
    m = M.Mirror(A, dt); m.begin(bs); m.iterate(1)
    assert m.breakdown and m.iterations == 1 and not m.x.any() and m.rr == 2049.0
    # maxiter cuts the last block of check_every
    Ac, bc, _, _ = _system("saddle47", dt)
    x, it, status, rel = M.Mirror(Ac, dt).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=8)
    assert it == 13 and status == M.MAXITER
    x, it, status, rel = M.Mirror(Ac, dt).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=0)
    assert it == 13 and status == M.MAXITER


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_breaks_down_where_minres_does_not(dtype):
    """saddle47 with b supported on the zero block: b.K b = 0 exactly, CG's first p.Ap — its mirror raises the breakdown flag and leaves x alone; the MINRES mirror converges."""
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem("saddle47")
    K = M.scipy_csr(n, rp, ci, v.astype(dt))
    b = M.zero_block_rhs(n).astype(dt)
    assert b[2209:].all() and not b[:2209].any() and float(b.astype(np.float64) @ (K.astype(np.float64) @ b.astype(np.float64))) == 0.0
    x, it, status, rel = CM.Mirror(K, dt).solve(b, rtol=M.RTOL[dt], maxiter=100, check_every=8)
    assert status == CM.BREAKDOWN and not x.any()
    x, it, status, rel = M.Mirror(K, dt).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=8)
    xs = M.spsolve_x(n, rp, ci, v, b.astype(np.float64))
    print("%s: MINRES %d iterations, error vs spsolve %.3g" % (dt, it, _relerr(x, xs)))
    assert status == M.CONVERGED and _relerr(x, xs) <= 100 * M.RTOL[dt]
