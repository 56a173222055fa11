"""The block-Jacobi preconditioner (tilespmv_block_jacobi_*, tilespmv_cg_create_block, tilespmv_bicgstab_create_block), as far as it can be checked without a GPU:
the C ABI is there and refuses what it must without a HIP call, the compiler made scratch-free kernels of hip_precond.hip and few of them, and the numpy mirror that
tests/test_gpu_block_jacobi.py compares the GPU with (tests/block_jacobi_mirror.py) is itself right on the inputs of those tests.

Recorded on the CPU (rtol = RTOL, check_every = 1), iterations of the mirrors:
    femblk10     CG        fp64: point Jacobi 246, bs 3: 42, bs 7: 127, bs 16: 106        fp32: point Jacobi 155, bs 3: 29
    femblk10_ns  BiCGStab  fp64: point Jacobi not in 5000, bs 3: 27, bs 16: 2861          fp32: point Jacobi not in 5000, bs 3: 17"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bicgstab_mirror as BM
import block_jacobi_mirror as M
import cg_mirror as CM
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib, api, generators as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_block_jacobi_create", "tilespmv_block_jacobi_destroy", "tilespmv_block_jacobi_update", "tilespmv_block_jacobi_apply", "tilespmv_block_jacobi_apply_dot",
               "tilespmv_block_jacobi_info", "tilespmv_cg_create_block", "tilespmv_bicgstab_create_block"]
MAX_KERNELS = 8
DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_symbols_are_exported_and_bad_arguments_are_refused(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    assert "typedef struct tilespmv_block_jacobi tilespmv_block_jacobi;" in header and "TILESPMV_BJ_INFO_COUNT = %d" % len(_lib.BJ_INFO_NAMES) in header
    # (no HIP call in any of these: this machine has no device to fail on)
    for rows, bs in ((0, 3), (-5, 3), (100, 0), (100, 17), (100, -1)):
        h = C.c_void_p(12345)
        assert lib.tilespmv_block_jacobi_create(C.byref(h), rows, bs) == HIP_ERROR_INVALID_VALUE, (rows, bs)
        assert not h
        with pytest.raises(ValueError):
            api.BlockJacobi(rows, bs, dtype)
    assert lib.tilespmv_block_jacobi_create(None, 100, 3) == HIP_ERROR_INVALID_VALUE
    lib.tilespmv_block_jacobi_destroy(None)
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    info = (C.c_longlong * len(_lib.BJ_INFO_NAMES))()
    assert lib.tilespmv_block_jacobi_update(None, a, a, a, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_block_jacobi_apply(None, a, a + 256, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_block_jacobi_apply_dot(None, a, a + 256, a, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_block_jacobi_info(None, None, info) == HIP_ERROR_INVALID_VALUE
    h = C.c_void_p(12345)
    assert lib.tilespmv_cg_create_block(C.byref(h), None, None) == HIP_ERROR_INVALID_VALUE and not h
    assert lib.tilespmv_cg_create_block(None, None, None) == HIP_ERROR_INVALID_VALUE
    h = C.c_void_p(12345)
    assert lib.tilespmv_bicgstab_create_block(C.byref(h), None, None) == HIP_ERROR_INVALID_VALUE and not h
    assert lib.tilespmv_bicgstab_create_block(None, None, None) == HIP_ERROR_INVALID_VALUE


def test_no_kernel_uses_scratch_and_there_are_few_of_them(tmp_path):
    assert "hip_precond.hip" in open(os.path.join(ROOT, "tilespmv_amd/csrc/Makefile")).read()
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_precond.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        names = list(spills)
        print(dt, len(spills), "kernels:", names)
        assert 2 <= len(spills) <= MAX_KERNELS, (dt, names)
        assert sum("k_bj_build" in k for k in names) == 1 and sum("k_bj_apply" in k for k in names) == 2, (dt, names)
        assert not {k: v for k, v in spills.items() if v}, (dt, spills)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s and "ds_write_b128" in s      # planes, r and z travel as 16-byte lane accesses; the slab is staged so


def test_the_inputs_are_what_they_say():
    n, rp, ci, v = M.problem("femblk10")
    m, n0, rp0, ci0 = G.fem_hex(10, 10, 10, 3)
    assert n == n0 == 3000 and np.array_equal(rp, rp0) and np.array_equal(ci, ci0)
    A = M.scipy_csr(n, rp, ci, v)
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()
    d = A.diagonal()
    assert (d > 0).all() and d.max() / d.min() > 1e4      # the node transforms spread the diagonal over decades: point Jacobi scales, it cannot rotate
    w = np.linalg.eigvalsh(A.toarray())
    assert w.min() > 0
    ns, rps, cis, vs = M.problem("femblk10_ns")
    assert ns == n and np.array_equal(rps, rp) and np.array_equal(cis, ci)
    As = M.scipy_csr(ns, rps, cis, vs)
    assert abs(As - As.T).max() > 1e-2 * abs(As).max()
    nl, rpl, cil, vl = M.problem("lap55")
    assert nl == 3025 and nl % 2 == 1 and all(nl % bs for bs in (2, 3, 7, 16))      # a scalar tail in both builds, a short last block for these sizes
    for dt in DTYPES:
        nt, rpt, cit, vt = M.tri_capped(dt)
        assert nt == {8: 1052249, 4: 2104499}[np.dtype(dt).itemsize] and nt % 3 != 0 and len(cit) == 3 * nt - 2


def test_pivot2_has_exactly_one_singular_block():
    n, rp, ci, v = M.problem("pivot2")
    assert n == 64 and len(ci) == 2 * 64 + 2      # (the zeros of the blocks are not stored)
    B = M.blocks(n, rp, ci, v, 2)
    assert np.array_equal(B[0], [[0, 2], [3, 0]]) and np.array_equal(B[5], [[1, 2], [2, 4]]) and len(B) == 32
    inv, singular = M.invert(B)
    assert singular.sum() == 1 and singular[5] and np.array_equal(inv[5], np.eye(2))
    assert np.array_equal(inv[0], [[0, 1 / 3], [1 / 2, 0]])
    P, count = M.update(n, rp, ci, v, 2, np.float64)
    assert count == 1 and np.array_equal(P[:, :2], [[0, 1 / 2], [1 / 3, 0]]) and np.array_equal(P[:, 10:12], np.eye(2))


@pytest.mark.parametrize("bs", [1, 2, 3, 5, 7, 16])
def test_the_mirror_of_apply_is_the_block_diagonal_solve(bs):
    """planes + apply against a dense solve with the block diagonal of lap55, short last block included; bs = 1 is the inverse diagonal."""
    n, rp, ci, v = M.problem("lap55")
    P, count = M.update(n, rp, ci, v, bs, np.float64)
    assert count == 0 and P.shape == (bs, n)
    A = M.scipy_csr(n, rp, ci, v).toarray()
    keep = np.arange(n)[:, None] // bs == np.arange(n)[None, :] // bs
    r = M.rhs(n)
    want = np.linalg.solve(np.where(keep, A, 0.0), r)
    got = M.apply(P, r)
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    short = n % bs
    if short:
        assert not P[short:, n - short:].any() and P[:short, n - short:].any()
    if bs == 1:
        assert np.array_equal(P[0], M.inverse_diagonal(n, rp, ci, v, np.float64))


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    vt, b = v.astype(dt), M.rhs(n).astype(dt)
    return n, rp, ci, vt, b, M.scipy_csr(n, rp, ci, vt), M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_jacobi_cg_converges_and_point_jacobi_needs_three_times_as_long(dtype):
    dt = np.dtype(dtype)
    n, rp, ci, vt, b, A, xs = _system("femblk10", dt)
    P, count = M.update(n, rp, ci, vt, 3, dt)
    assert count == 0
    x, it, status, rel = M.CG(A, dt, P).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    xp, itp, statusp, relp = CM.Mirror(A, dt, M.inverse_diagonal(n, rp, ci, vt, dt)).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    print("femblk10 %s: block Jacobi (3) %d iterations, error vs spsolve %.3g; point Jacobi %d iterations, %.3g" % (dt, it, _relerr(x, xs), itp, _relerr(xp, xs)))
    assert status == M.CONVERGED and statusp == M.CONVERGED and rel <= M.RTOL[dt]
    assert _relerr(x, xs) <= 100 * M.RTOL[dt] and _relerr(xp, xs) <= 100 * M.RTOL[dt]
    assert itp >= 3 * it
    # bs = 1 is point Jacobi, iterate for iterate
    P1, _ = M.update(n, rp, ci, vt, 1, dt)
    x1, it1, status1, rel1 = M.CG(A, dt, P1).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    assert it1 == itp and np.array_equal(x1, xp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_jacobi_bicgstab_converges_where_point_jacobi_is_still_running(dtype):
    dt = np.dtype(dtype)
    n, rp, ci, vt, b, A, xs = _system("femblk10_ns", dt)
    P, count = M.update(n, rp, ci, vt, 3, dt)
    assert count == 0
    x, it, status, rel = M.BiCGStab(A, dt, P).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
    xp, itp, statusp, relp = BM.Mirror(A, dt, M.inverse_diagonal(n, rp, ci, vt, dt)).solve(b, rtol=M.RTOL[dt], maxiter=2 * it, check_every=1)
    print("femblk10_ns %s: block Jacobi (3) %d iterations, error vs spsolve %.3g; point Jacobi after %d: status %d, sqrt(rr/bb) %.3g" % (dt, it, _relerr(x, xs), itp, statusp, relp))
    assert status == M.CONVERGED and rel <= M.RTOL[dt] and _relerr(x, xs) <= 100 * M.RTOL[dt]
    assert statusp == M.MAXITER and itp == 2 * it and relp > 1e3 * M.RTOL[dt]
