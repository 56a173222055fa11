"""GMRES with the Krylov basis stored as floats in the fp64 library (tilespmv_gmres_create_basis; include/tilespmv.h), as far as it can be checked without a GPU:
the numerics that motivate the form and the one property its design must respect, on the numpy mirrors (tests/gmres_cb_mirror.py over tests/gmres_mirror.py); the new symbols and
their refusals without a device; spill-free kernels in both forms; the workspace formula of the header.  Values and recurrences are fp64, rtol 1e-10 and rhs(n) throughout,
unless a test says float32."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gmres_cb_mirror as CB
import gmres_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_gmres_create_basis", "tilespmv_gmres_basis_bytes", "tilespmv_gmres_workspace_bytes"]
BASIS_KERNELS = ("k_gm_dots", "k_gm_orth1", "k_gm_orth2", "k_gm_next", "k_gm_update")
F64 = np.dtype(np.float64)
RTOL = 1e-10
RESTART = 16
# Recorded on the machine these tests were written on (restart 16, check_every = 1): iterations with the fp64 basis / with the float basis, error against spsolve (both)
#   convdiff67 280 / 280, 2.9e-10;  convdom67 297 / 297, 1.1e-10;  shiftskew67 383 / 383, 1.7e-10;  convdiff67_colscaled + Jacobi 280 / 280, 2.8e-10
INPUTS = ["convdiff67", "convdom67", "shiftskew67", "convdiff67_colscaled"]
_SYSTEMS = {}


def _system(name, dtype=F64):
    """(A, b, dinv, spsolve's x) of a named input, computed once and left unchanged."""
    dt = np.dtype(dtype)
    if (name, dt) not in _SYSTEMS:
        n, rp, ci, v = CB.problem(name)
        vt, b = v.astype(dt), M.rhs(n).astype(dt)
        dinv = M.inverse_diagonal(n, rp, ci, vt, dt) if name.endswith("_colscaled") else None
        _SYSTEMS[(name, dt)] = (M.scipy_csr(n, rp, ci, vt), b, dinv, M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64)))
    return _SYSTEMS[(name, dt)]


def _relerr(x, xs):
    return float(np.linalg.norm(x.astype(np.float64) - xs) / np.linalg.norm(xs))


def _true_rel(A, b, x):
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(b64 - A.astype(np.float64) @ x.astype(np.float64)) / np.linalg.norm(b64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_new_symbols_are_exported_and_bad_basis_bytes_are_refused_without_a_device(dtype):
    lib = _lib.load(dtype)
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.DECLARED_SYMBOLS and name + "(" in header, name
    assert "#define TILESPMV_GMRES_BASIS_VALUE 0" in header and "#define TILESPMV_GMRES_BASIS_FLOAT 4" in header
    plan = C.c_void_p(0x1000)      # never followed: basis_bytes and restart are looked at first
    other = 8 if np.dtype(dtype) == np.float32 else 2
    for args in ((None, 30, None, None, 2), (plan, 30, None, None, 2), (plan, 30, None, None, 3), (plan, 30, None, None, 16), (plan, 30, None, None, -4),
                 (plan, 30, None, None, other), (plan, 0, None, None, 4), (plan, 65, None, None, 0), (plan, 30, plan, plan, 4), (None, 30, None, None, 4),
                 (None, 30, None, None, 0)):      # (no HIP call: this machine has no device to fail on)
        h = C.c_void_p(12345)
        assert lib.tilespmv_gmres_create_basis(C.byref(h), *args) == HIP_ERROR_INVALID_VALUE, args
        assert not h, args
    assert lib.tilespmv_gmres_create_basis(None, None, 30, None, None, 4) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_gmres_basis_bytes(None) == 0 and lib.tilespmv_gmres_workspace_bytes(None) == 0


def test_no_kernel_of_either_form_spills(tmp_path):
    """hip_solver_gm.hip (the value form, both builds) and hip_solver_gm_cb.hip (the float form; empty in the fp32 build): no private segment, no atomics; the float form has
    the five kernels that touch the basis once each and reads the basis with 8-byte loads beside the 16-byte loads of w."""
    jobs = [("hip_solver_gm.hip", "f64"), ("hip_solver_gm.hip", "f32"), ("hip_solver_gm_cb.hip", "f64"), ("hip_solver_gm_cb.hip", "f32")]
    with ThreadPoolExecutor(4) as ex:
        asm = dict(zip(jobs, ex.map(lambda j: device_asm(j[0], j[1], str(tmp_path / ("%s_%s.s" % j))), jobs)))
    for job, s in asm.items():
        spills = private_segments(s)
        print(job, len(spills), "kernels:", spills)
        assert not {k: v for k, v in spills.items() if v}, (job, spills)
        assert "global_atomic" not in s and "flat_atomic" not in s
    assert not private_segments(asm[("hip_solver_gm_cb.hip", "f32")])      # the float instantiations exist in the fp64 build only
    names = list(private_segments(asm[("hip_solver_gm_cb.hip", "f64")]))
    for want in BASIS_KERNELS:
        assert sum(want in k and "IfE" in k for k in names) == 1, (want, names)      # (IfE: the Itanium mangling of the template argument <float>)
    cb = asm[("hip_solver_gm_cb.hip", "f64")]
    assert "global_load_dwordx2" in cb and "global_load_dwordx4" in cb and "global_store_dwordx2" in cb and "v_cvt_f32_f64" in cb and "v_cvt_f64_f32" in cb
    assert all(sum(want in k for k in private_segments(asm[("hip_solver_gm.hip", dt)])) == 1 for want in BASIS_KERNELS for dt in ("f64", "f32"))


@pytest.mark.parametrize("name", INPUTS)
def test_the_float_basis_costs_no_iterations_at_restart_16(name):
    """CONVERGED, within one restart of the fp64 basis's count (recorded: equal counts), at an error against spsolve of at most 2 x the fp64 basis's."""
    A, b, dinv, xs = _system(name)
    x, it, status, rel = M.Mirror(A, F64, RESTART, dinv).solve(b, rtol=RTOL, maxiter=3000, check_every=1)
    xc, itc, statusc, relc = CB.Mirror(A, F64, RESTART, dinv).solve(b, rtol=RTOL, maxiter=3000, check_every=1)
    err, errc = _relerr(x, xs), _relerr(xc, xs)
    print("%s: fp64 basis %d iterations, error %.3g;  float basis %d iterations, error %.3g, sqrt(rr/bb) %.3g, true %.3g" % (name, it, err, itc, errc, relc, _true_rel(A, b, xc)))
    assert status == M.CONVERGED and statusc == M.CONVERGED
    assert abs(itc - it) <= RESTART
    assert errc <= 2 * err
    assert relc <= RTOL and not np.array_equal(x, xc)


@pytest.mark.parametrize("restart", [10, 30, 64])
def test_equal_counts_at_check_every_8(restart):
    """convdiff67 with check_every = 8 at restarts 10, 30 and 64: within one check of the fp64 basis's count (recorded: equal)."""
    A, b, dinv, xs = _system("convdiff67")
    x, it, status, rel = M.Mirror(A, F64, restart).solve(b, rtol=RTOL, maxiter=3000, check_every=8)
    xc, itc, statusc, relc = CB.Mirror(A, F64, restart).solve(b, rtol=RTOL, maxiter=3000, check_every=8)
    print("convdiff67 restart %d: fp64 basis %d, float basis %d" % (restart, it, itc))
    assert status == statusc == M.CONVERGED and abs(itc - it) <= 8 and _relerr(xc, xs) <= 2 * _relerr(x, xs)


def test_the_floor_of_one_cycle_and_the_solve_rule():
    """shiftskew67_d4 at restart 64.  After 40 inner iterations of ONE cycle the recurrence's sqrt(rr / bb) is far below rtol in both forms; after a flush the recomputed one is
    near eps32 (recorded 2.7e-8) with the float basis and below 1e-14 (recorded 6.4e-16) with the fp64 one: a solve that believed the recurrence would return that x as
    CONVERGED.  solve converges to a recomputed residual <= rtol in at most 2 x the fp64 basis's count (recorded 34 against 27; check_every = 8: 40 against 32)."""
    A, b, dinv, xs = _system("shiftskew67_d4")
    i = 67 * 33 + 20
    assert (A[i, i], A[i, i - 1], A[i, i + 1], A[i, i - 67], A[i, i + 67]) == (4.0, -1.0, 1.0, -1.0, 1.0)
    got = {}
    for label, mirror in (("fp64", M.Mirror(A, F64, 64)), ("float", CB.Mirror(A, F64, 64))):
        mirror.begin(b); mirror.iterate(40)
        recurrence = mirror.rel()
        mirror.flush()
        got[label] = (recurrence, mirror.rel(), _true_rel(A, b, mirror.x))
        print("%s basis: after 40 iterations the recurrence says %.3g, recomputed after a flush %.3g (on the host %.3g)" % ((label,) + got[label]))
    assert got["fp64"][0] <= 1e-14 and got["float"][0] <= 1e-14
    assert got["fp64"][1] <= 1e-14
    assert 1e-9 <= got["float"][1] <= 1e-6
    assert abs(got["float"][1] - got["float"][2]) <= 1e-3 * got["float"][1]
    for check_every in (1, 8):
        x, it, status, rel = M.Mirror(A, F64, 64).solve(b, rtol=RTOL, maxiter=500, check_every=check_every)
        xc, itc, statusc, relc = CB.Mirror(A, F64, 64).solve(b, rtol=RTOL, maxiter=500, check_every=check_every)
        print("check_every %d: fp64 basis %d iterations, float basis %d, recomputed sqrt(rr/bb) %.3g, on the host %.3g" % (check_every, it, itc, relc, _true_rel(A, b, xc)))
        assert status == statusc == M.CONVERGED
        assert relc <= RTOL and _true_rel(A, b, xc) <= 1.01 * RTOL
        assert itc <= 2 * it
    # restart 16: a cycle ends before the floor is reached, equal counts (recorded 27 and 27)
    x, it, status, rel = M.Mirror(A, F64, 16).solve(b, rtol=RTOL, maxiter=500, check_every=1)
    xc, itc, statusc, relc = CB.Mirror(A, F64, 16).solve(b, rtol=RTOL, maxiter=500, check_every=1)
    assert status == statusc == M.CONVERGED and abs(itc - it) <= 16 and relc <= RTOL


@pytest.mark.parametrize("name", ["convdiff67", "convdiff67_colscaled"])
def test_with_float32_values_the_compressed_mirror_is_the_plain_one(name):
    """The stored type is the value type: x, the state and the basis are the plain mirror's bit for bit, after early iterations and after a solve."""
    dt = np.dtype(np.float32)
    A, b, dinv, xs = _system(name, dt)
    p, c = M.Mirror(A, dt, 8, dinv), CB.Mirror(A, dt, 8, dinv)
    for m in (p, c):
        m.begin(b); m.iterate(11); m.flush()
    assert np.array_equal(p.x, c.x) and p.rr == c.rr and p.iterations == c.iterations and np.array_equal(p.V, c.V[:]) and p.x.any()
    x, it, status, rel = M.Mirror(A, dt, RESTART, dinv).solve(b, rtol=M.RTOL[dt], maxiter=3000, check_every=1)
    xc, itc, statusc, relc = CB.Mirror(A, dt, RESTART, dinv).solve(b, rtol=M.RTOL[dt], maxiter=3000, check_every=1)
    assert np.array_equal(x, xc) and (it, status, rel) == (itc, statusc, relc) and status == M.CONVERGED


def test_the_block_mirror_takes_the_float_basis():
    """femblk10_ns with the bs = 3 planes: the float basis converges within one restart of the fp64 one and the two iterates differ (the apply is fed the rounded vector)."""
    import block_jacobi_mirror as BJ
    n, rp, ci, v = BJ.problem("femblk10_ns")
    b = M.rhs(n)
    A = M.scipy_csr(n, rp, ci, v)
    P, _ = BJ.update(n, rp, ci, v, 3, F64)
    xs = M.spsolve_x(n, rp, ci, v, b)
    x, it, status, rel = M.BlockMirror(A, F64, RESTART, P).solve(b, rtol=RTOL, maxiter=1000, check_every=1)
    xc, itc, statusc, relc = CB.BlockMirror(A, F64, RESTART, P).solve(b, rtol=RTOL, maxiter=1000, check_every=1)
    print("femblk10_ns bs = 3: fp64 basis %d iterations, float basis %d" % (it, itc))
    assert status == statusc == M.CONVERGED and abs(itc - it) <= RESTART and _relerr(xc, xs) <= 2 * _relerr(x, xs) and not np.array_equal(x, xc)


def test_the_workspace_formula_of_the_header():
    """Restart 64 and 1 M rows in fp64: the float basis needs less than 0.56 x the workspace of the fp64 one; the value form's formula is restart + 3 (+ 1) vectors and the
    small arrays, as the GMRES block of the header has said since the solver exists."""
    header = open(os.path.join(ROOT, "include/tilespmv.h")).read()
    assert "(restart + 1) B + v D + 2 (restart + 1) Q + 2 Q + 32768 + 4 * 768 + 256" in header
    rows = 1 << 20
    value, narrow = CB.workspace_bytes(rows, 64, 8, 8), CB.workspace_bytes(rows, 64, 8, 4)
    print("restart 64, %d rows: %d bytes with the fp64 basis, %d with the float basis: %.4f" % (rows, value, narrow, narrow / value))
    assert narrow < 0.56 * value
    vec, fvec = -(-(rows + 16) * 8 // 256) * 256, -(-(rows + 16) * 4 // 256) * 256      # (rounded up to 256)
    assert value == 67 * vec + (2 * 65 + 2) * 2048 + 32768 + 4 * 768 + 256 and CB.workspace_bytes(rows, 64, 8, 8, "dinv") == value + vec
    assert narrow == 65 * fvec + 3 * vec + (2 * 65 + 2) * 2048 + 32768 + 4 * 768 + 256
    assert CB.workspace_bytes(rows, 64, 8, 4, "dinv") == narrow and CB.workspace_bytes(rows, 64, 8, 4, "block") == narrow + vec
    assert CB.workspace_bytes(rows, 64, 4, 4) == 67 * fvec + (2 * 65 + 2) * 2048 + 32768 + 4 * 768 + 256      # (the float library: 4 is the identity)
