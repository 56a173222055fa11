"""The restarted GMRES solver in the library (tilespmv_gmres_*), as far as it can be checked without a GPU: the C ABI is there and refuses what it must without a
device, the compiler made spill-free kernels of hip_solver_gm.hip and few of them, and the numpy mirror that tests/test_gpu_gmres.py compares the GPU with (tests/gmres_mirror.py)
is itself right — it counts scipy's iterations, converges on the inputs of those tests where BiCGStab does not, and keeps its guards."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import bicgstab_mirror as B
import gmres_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_gmres_create", "tilespmv_gmres_create_block", "tilespmv_gmres_destroy", "tilespmv_gmres_begin", "tilespmv_gmres_iterate", "tilespmv_gmres_flush",
               "tilespmv_gmres_state_read", "tilespmv_gmres_solve"]
ITERATION_KERNELS = ("k_gm_dots", "k_gm_orth1", "k_gm_orth2", "k_gm_next")
MAX_SOLVER_KERNELS = 10     # the four of an iteration; the residual and the scalars of begin; the back substitution, the update of x and the block form's axpy; one to spare
DTYPES = [np.float64, np.float32]
RESTART = 16


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_solver_symbols_are_exported_and_bad_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    assert "typedef struct tilespmv_gmres tilespmv_gmres;" in header and "#define TILESPMV_GMRES_MAX_RESTART 64" in header
    plan = C.c_void_p(0x1000)      # never followed: restart is looked at first
    for args in ((None, 8, None), (plan, 0, None), (plan, 65, None)):      # (no HIP call: this machine has no device to fail on)
        h = C.c_void_p(12345)
        assert lib.tilespmv_gmres_create(C.byref(h), *args) == HIP_ERROR_INVALID_VALUE, args
        assert not h
    for args in ((None, 8, plan), (plan, 8, None), (plan, 0, plan), (plan, 65, plan)):
        h = C.c_void_p(12345)
        assert lib.tilespmv_gmres_create_block(C.byref(h), *args) == HIP_ERROR_INVALID_VALUE, args
        assert not h
    assert lib.tilespmv_gmres_create(None, None, 8, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_create_block(None, None, 8, None) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_gmres_destroy(None)
    st = _lib.CGState()
    assert lib.tilespmv_gmres_begin(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_flush(None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_state_read(None, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_solve(None, None, None, 1e-8, 10, 8, None, C.byref(st)) == HIP_ERROR_INVALID_VALUE


def test_no_solver_kernel_spills_and_there_are_few_of_them(tmp_path):
    assert "hip_solver_gm.hip" in open(os.path.join(ROOT, "tilespmv_amd/csrc/Makefile")).read()
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver_gm.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert len(ITERATION_KERNELS) <= len(spills) <= MAX_SOLVER_KERNELS, (dt, names)
        for want in ITERATION_KERNELS:
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)      # (the dot products of up to 65 basis vectors included: their accumulators are registers)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the vectors travel as 16-byte lane accesses
        assert "global_atomic" not in s and "flat_atomic" not in s


# ---- the mirror on the inputs of the GPU tests.  Printed by these tests on the machine they were written on (restart 16, rtol = RTOL, check_every = 1; fp64 / fp32):
#   convdiff67             280 / 192 it, true |b - A x| / |b| 9.3e-11 / 9.8e-6, error vs spsolve 2.9e-10 / 6.5e-5
#   convdom67              297 / 199 it, 9.4e-11 / 9.8e-6, 1.1e-10 / 1.1e-5
#   shiftskew67            383 / 188 it, 9.7e-11 / 9.9e-6, 1.7e-10 / 1.8e-5
#   convdiff67_colscaled   Jacobi: 280 / 192 it, 9.3e-11 / 9.8e-6, 2.8e-10 / 6.0e-5;  plain at 4 x that many: sqrt(rr/bb) 2.5e-3 / 1.1e-2
#   dots in a permuted order: the same counts everywhere
COUNTS = {"convdiff67": (280, 192), "convdom67": (297, 199), "shiftskew67": (383, 188), "convdiff67_colscaled": (280, 192)}
SCIPY_COUNTS = {8: 220, 16: 280, 30: 394, 64: 324}      # convdiff67 in fp64
FEW = 3
_SYSTEMS = {}


def _system(name, dtype):
    """(A, b, dinv, spsolve's x) of a named input, computed once per value type and left unchanged."""
    dt = np.dtype(dtype)
    if (name, dt) not in _SYSTEMS:
        n, rp, ci, v = M.problem(name)
        vt, b = v.astype(dt), M.rhs(n).astype(dt)
        dinv = M.inverse_diagonal(n, rp, ci, vt, dt) if name.endswith("_colscaled") else None
        _SYSTEMS[(name, dt)] = (M.scipy_csr(n, rp, ci, vt), b, dinv, M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64)))
    return _SYSTEMS[(name, dt)]


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def _true_rel(A, b, x):
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(b64 - A.astype(np.float64) @ x.astype(np.float64)) / np.linalg.norm(b64))


def test_the_inputs_are_what_they_say():
    n, rp, ci, v = M.problem("convdom67")
    A = M.scipy_csr(n, rp, ci, v)
    i = 67 * 33 + 20      # an inner grid point
    assert n == 4489 and (A[i, i], A[i, i - 1], A[i, i + 1], A[i, i - 67], A[i, i + 67]) == (4.0, -9.0, 7.0, -6.0, 4.0)
    n, rp, ci, v = M.problem("shiftskew67")
    A = M.scipy_csr(n, rp, ci, v)
    assert (A[i, i], A[i, i - 1], A[i, i + 1], A[i, i - 67], A[i, i + 67]) == (0.25, -1.0, 1.0, -1.0, 1.0)
    S = A - 0.25 * M.scipy_csr(n, np.arange(n + 1), np.arange(n), np.ones(n))
    assert abs(S + S.T).max() == 0      # (A - I/4 is skew-symmetric)
    n, rp, ci, v = M.problem("convdiff67_colscaled")
    n0, rp0, ci0, v0 = B.problem("convdiff67")
    dinv = M.inverse_diagonal(n, rp, ci, v, np.float64)
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.allclose(v * dinv[ci], v0 / 4, rtol=1e-15)      # (right Jacobi restores A / 4)
    n, rp, ci, v = M.problem("nilpotent")
    A, b = M.scipy_csr(n, rp, ci, v), M.nilpotent_rhs(n)
    assert n == 4098 and A.nnz == n // 2 and A[0, 1] == 1 and A[2, 3] == 1 and A[1].nnz == 0 and b.any() and not b[1::2].any() and not (A @ b).any() and not (A @ A).nnz


@pytest.mark.parametrize("restart", sorted(SCIPY_COUNTS))
def test_the_mirror_counts_the_iterations_of_scipy(restart):
    """convdiff67 in fp64: with check_every = 1 the mirror stops after as many inner iterations as scipy.sparse.linalg.gmres reports preconditioned residual norms."""
    A, b, _, xs = _system("convdiff67", np.float64)
    x, it, status, rel = M.Mirror(A, np.float64, restart).solve(b, rtol=1e-10, maxiter=3000, check_every=1)
    norms = []
    xsc, info = spl.gmres(A, b, rtol=1e-10, atol=0.0, restart=restart, maxiter=1000, callback=norms.append, callback_type="pr_norm")
    print("restart %d: mirror %d iterations, scipy %d (recorded %d)" % (restart, it, len(norms), SCIPY_COUNTS[restart]))
    assert status == M.CONVERGED and info == 0
    assert it == len(norms) == SCIPY_COUNTS[restart]
    assert _relerr(x, xsc) <= 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(COUNTS))
def test_the_mirror_converges_to_the_direct_solution(name, dtype):
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system(name, dt)
    x, it, status, rel = M.Mirror(A, dt, RESTART, dinv).solve(b, rtol=M.RTOL[dt], maxiter=3000, check_every=1)
    err, true = _relerr(x, xs), _true_rel(A, b, x)
    want = COUNTS[name][dt == np.float32]
    print("%s %s: %d iterations (recorded %d), status %d, sqrt(rr/bb) %.3g, true %.3g, error vs spsolve %.3g" % (name, dt, it, want, status, rel, true, err))
    assert status == M.CONVERGED
    assert true <= M.RTOL[dt] and rel <= M.RTOL[dt]
    assert abs(it - want) <= FEW
    assert err <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_gmres_fails_on_the_column_scaled_input(dtype):
    """What makes the GPU Jacobi test mean something: without dinv the mirror is still far away after 4 x the Jacobi count."""
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system("convdiff67_colscaled", dt)
    itj = COUNTS["convdiff67_colscaled"][dt == np.float32]
    x, it, status, rel = M.Mirror(A, dt, RESTART).solve(b, rtol=M.RTOL[dt], maxiter=4 * itj, check_every=1)
    print("convdiff67_colscaled %s: plain %d iterations, status %d, sqrt(rr/bb) %.3g" % (dt, it, status, rel))
    assert status == M.MAXITER and it == 4 * itj and rel >= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(COUNTS))
def test_another_order_of_the_sums_costs_few_iterations(name, dtype):
    """The mirror with its dot products accumulated in a permuted order converges within 1.25 x the unpermuted count: the GPU (whose sums have yet another order) may be capped at
    2 x the mirror's count without the cap ever cutting off a correct solver."""
    dt = np.dtype(dtype)
    A, b, dinv, xs = _system(name, dt)
    it = COUNTS[name][dt == np.float32]
    order = np.random.default_rng(11).permutation(A.shape[0])
    xp, itp, statusp, relp = M.Mirror(A, dt, RESTART, dinv, order=order).solve(b, rtol=M.RTOL[dt], maxiter=3000, check_every=1)
    print("%s %s: %d iterations recorded, %d with permuted sums" % (name, dt, it, itp))
    assert statusp == M.CONVERGED
    assert itp <= 1.25 * it
    assert _relerr(xp, xs) <= 100 * M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_motivates_the_feature(dtype):
    """shiftskew67: BiCGStab's mirror does not reach RTOL in fp64 within 3000 iterations, and in fp32 it reports CONVERGED on a recurrence residual that has drifted away from
    the true one; the GMRES mirror converges in both (test_the_mirror_converges_to_the_direct_solution).  skew: BiCGStab breaks down, GMRES needs 2 iterations."""
    dt = np.dtype(dtype)
    A, b, _, xs = _system("shiftskew67", dt)
    x, it, status, rel = B.Mirror(A, dt).solve(b, rtol=M.RTOL[dt], maxiter=3000, check_every=1)
    true = _true_rel(A, b, x)
    print("shiftskew67 %s BiCGStab: %d iterations, status %d, sqrt(rr/bb) %.3g, true %.3g" % (dt, it, status, rel, true))
    if dt == np.float64:
        assert status == M.MAXITER and it == 3000 and rel > M.RTOL[dt]
    else:
        assert status == M.CONVERGED and true > 100 * M.RTOL[dt]
    n, rp, ci, v = M.problem("skew")
    A, bs = M.scipy_csr(n, rp, ci, v), M.skew_rhs(n)
    assert B.Mirror(A, dt).solve(bs, rtol=M.RTOL[dt], maxiter=100, check_every=1)[2] == M.BREAKDOWN
    x, it, status, rel = M.Mirror(A, dt, RESTART).solve(bs, rtol=M.RTOL[dt], maxiter=100, check_every=1)
    print("skew %s GMRES: %d iterations, status %d, sqrt(rr/bb) %.3g" % (dt, it, status, rel))
    assert status == M.CONVERGED and it <= 2 and _true_rel(A, bs.astype(dt), x) <= M.RTOL[dt]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mirror_guards(dtype):
    """b = 0; rr = 0 at begin (skew from its exact solution); the lucky termination (A = 2 I, b = 4 e_k: everything exact); gamma = 0 (nilpotent); maxiter cuts the last block;
    check_every = 0 is 1; solve's final flush makes rr the recomputed residual."""
    dt = np.dtype(dtype)
    # b = 0
    n, rp, ci, v = M.problem("2I")
    I2 = M.scipy_csr(n, rp, ci, v)
    b = M.rhs(n).astype(dt)
    m = M.Mirror(I2, dt, 8)
    x, it, status, rel = m.solve(np.zeros(n), x0=b, rtol=M.RTOL[dt])
    assert it == 0 and status == M.CONVERGED and not x.any() and rel == 0.0
    m.begin(np.zeros(n)); m.iterate(16); m.flush()
    assert m.iterations == 16 and not m.x.any() and m.rr == 0.0 and m.status() == M.CONVERGED
    # skew from its exact integer solution x0 = -A b: rr = 0 at begin, nothing changes
    n, rp, ci, v = M.problem("skew")
    A, bs = M.scipy_csr(n, rp, ci, v), M.skew_rhs(n)
    x0 = -(A @ bs)
    assert np.array_equal(A @ x0, bs)
    m = M.Mirror(A, dt, 8); m.begin(bs, x0)
    assert m.rr == 0.0 and m.status() == M.CONVERGED
    m.iterate(16)
    assert m.iterations == 16 and m.rr == 0.0 and np.array_equal(m.x, x0.astype(dt)) and not m.V.any()
    # A = 2 I, b = 4 e_k: V_0 = e_k, w = 2 e_k, h = 2, w'' = 0: the lucky termination; the close gives x = 2 e_k exactly
    e = np.zeros(I2.shape[0]); e[1234] = 1.0
    m = M.Mirror(I2, dt, 8); m.begin(4 * e); m.iterate(1)
    assert m.rr == 0.0 and m.j == 1 and not m.live and m.status() == M.CONVERGED and not m.x.any()
    m.iterate(5); m.flush()
    assert m.iterations == 6 and np.array_equal(m.x, (2 * e).astype(dt)) and m.rr == 0.0 and m.status() == M.CONVERGED
    m.begin(4 * e); m.iterate(8)      # ... and the close at the end of the cycle uses the one column done
    assert np.array_equal(m.x, (2 * e).astype(dt)) and m.rr == 0.0
    # nilpotent: A V_0 = 0 exactly: gamma = 0
    n, rp, ci, v = M.problem("nilpotent")
    A, bn = M.scipy_csr(n, rp, ci, v), M.nilpotent_rhs(n)
    x0 = np.zeros(n)
    x, it, status, rel = M.Mirror(A, dt, 8).solve(bn, x0=x0, rtol=M.RTOL[dt], maxiter=100, check_every=8)
    assert status == M.BREAKDOWN and it == 8 and np.array_equal(x, x0) and rel == 1.0
    m = M.Mirror(A, dt, 8); m.begin(bn); m.iterate(1)
    assert m.breakdown and m.j == 0 and m.rr == float(bn @ bn)
    # maxiter cuts the last block of check_every; check_every = 0 is 1
    Ac, bc, _, _ = _system("convdiff67", dt)
    x, it, status, rel = M.Mirror(Ac, dt, 8).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=8)
    assert it == 13 and status == M.MAXITER
    # solve's final flush: x is the iterate of iteration 13 (5 columns into the second cycle) and rr its recomputed residual
    true = _true_rel(Ac, bc, x)
    print("%s: after 13 iterations sqrt(rr/bb) %.6g, recomputed on the host %.6g" % (dt, rel, true))
    assert abs(rel - true) <= 100 * np.finfo(dt).eps * true
    m = M.Mirror(Ac, dt, 8); m.begin(bc); m.iterate(13)
    stale = _true_rel(Ac, bc, m.x)
    assert stale > 1.01 * true and m.rel() < stale      # (before the flush x is that of the last close, and rr is ahead of it)
    x0, it0, status0, rel0 = M.Mirror(Ac, dt, 8).solve(bc, rtol=M.RTOL[dt], maxiter=13, check_every=0)
    assert it0 == 13 and status0 == M.MAXITER and np.array_equal(x0, x)
