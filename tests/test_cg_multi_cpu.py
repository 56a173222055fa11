"""The multi-right-hand-side solver (tilespmv_cg_multi_*), as far as it can be checked without a GPU: the C ABI is there and refuses what it must without a
device, the compiler made spill-free kernels of hip_solver_mv.hip with 16-byte accesses and few of them, and the numpy mirror (tests/cg_mirror.py) converges on the eight
right-hand sides that tests/test_gpu_cg_multi.py solves (tests/cg_multi_cases.py):

    j   column                        j   column
    0   M.rhs(n)                      4   A linspace(0, 1, n)
    1   A 1                           5   the unit vector e_{n//2}
    2   zeros                         6   1e-3 U(seed 5)
    3   1e3 U(seed 4)                 7   U(seed 6)                     U = uniform(-1, 1) from default_rng
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cg_mirror as M
import cg_multi_cases as MC
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NEW_SYMBOLS = ["tilespmv_cg_multi_create", "tilespmv_cg_multi_destroy", "tilespmv_cg_multi_begin", "tilespmv_cg_multi_iterate", "tilespmv_cg_multi_state_read",
               "tilespmv_cg_multi_solve"]
# 3 NVEC values x (dot, update, direction, begin) + begin_fold + freeze + zero_columns = 15 kernels; the cap is that count + 2
MAX_KERNELS = 17


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_symbols_are_exported_and_bad_arguments_are_refused_without_a_device(dtype):
    lib = _lib.load(dtype)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS, name
    h = C.c_void_p(12345)
    assert lib.tilespmv_cg_multi_create(C.byref(h), None, 2, None) == HIP_ERROR_INVALID_VALUE      # (no HIP call: this machine has no device to fail on)
    assert not h
    assert lib.tilespmv_cg_multi_create(None, None, 2, None) == HIP_ERROR_INVALID_VALUE
    dummy = (C.c_char * 65536)()                                                                   # a non-NULL plan handle that must not be looked at
    for nvec in (0, 3, 16, -1):
        h = C.c_void_p(12345)
        assert lib.tilespmv_cg_multi_create(C.byref(h), C.addressof(dummy), nvec, None) == HIP_ERROR_INVALID_VALUE, nvec
        assert not h
    lib.tilespmv_cg_multi_destroy(None)
    st = (_lib.CGState * 8)()
    st[0].size = C.sizeof(_lib.CGState)
    assert lib.tilespmv_cg_multi_begin(None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_multi_iterate(None, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_multi_state_read(None, None, st) == HIP_ERROR_INVALID_VALUE
    assert lib.tilespmv_cg_multi_solve(None, None, None, 1e-8, 10, 8, None, st) == HIP_ERROR_INVALID_VALUE


def test_no_kernel_touches_scratch_and_there_are_few_of_them(tmp_path):
    assert "hip_solver_mv.hip" in open(os.path.join(ROOT, "tilespmv_amd/csrc/Makefile")).read()
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_solver_mv.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        scratch = private_segments(s)
        names = list(scratch)
        print(dt, len(scratch), "kernels:", names)
        assert 12 <= len(scratch) <= MAX_KERNELS, (dt, names)
        for want in ("k_cgm_dot", "k_cgm_update", "k_cgm_direction", "k_cgm_begin"):
            assert sum(want + "ILi" in k for k in names) == 3, (dt, want, names)                  # one per NVEC in {2, 4, 8}
        for want in ("k_cgm_begin_fold", "k_cgm_freeze"):
            assert sum(want in k for k in names) == 1, (dt, want, names)
        assert not {k: v for k, v in scratch.items() if v}, (dt, scratch)
        assert "global_load_dwordx4" in s and "global_store_dwordx4" in s      # the arrays travel as 16-byte lane accesses


# ---- the mirror on the inputs of the GPU tests, at rtol = M.RTOL, check_every = 1.  Counts of columns 0-7 on lap128, asserted below:
#   fp64  444, 268, 0, 444, 398, 419, 444, 447          fp32  291, 186, 0, 291, 256, 242, 269, 284
LAP128_COUNTS = {np.dtype(np.float64): [444, 268, 0, 444, 398, 419, 444, 447], np.dtype(np.float32): [291, 186, 0, 291, 256, 242, 269, 284]}
WITHIN = {("tri200", np.dtype(np.float64)): 35, ("tri200", np.dtype(np.float32)): 18, ("fem12", np.dtype(np.float64)): 55, ("fem12", np.dtype(np.float32)): 35}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["lap128", "tri200", "fem12"])
def test_the_mirror_converges_on_all_eight_columns(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, vt, B = MC.system(name, dt)
    A = M.scipy_csr(n, rp, ci, vt)
    counts = []
    for j in range(8):
        x, it, status, rel = M.Mirror(A, dt).solve(B[:, j], rtol=M.RTOL[dt], maxiter=2000, check_every=1)
        counts.append(it)
        assert status == M.CONVERGED and rel <= M.RTOL[dt], (j, it, status, rel)
    print(name, dt, "mirror iterations, columns 0-7:", counts)
    assert counts[2] == 0
    if name == "lap128":
        assert len(set(counts)) >= 4                                     # the columns stop at different iterations: the freeze has work to do
        assert counts == LAP128_COUNTS[dt]
    else:
        assert max(counts) <= WITHIN[(name, dt)]
        assert np.array_equal(B[:, 1], np.ones(n, dtype=dt))             # A 1 = 1 exactly (degree + 1 on the diagonal): column 1 is at r = 0 after one iteration
        m = M.Mirror(A, dt); m.begin(B[:, 1]); m.iterate(1)
        assert m.rr == 0.0 and np.array_equal(m.x, np.ones(n, dtype=dt))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_after_three_iterations_on_tri200_every_column_still_runs(dtype):
    """What makes the GPU comparison after 1 and 3 iterations a comparison of running solves: every column but 1 and 2 sits at rr / bb of 1e-3 to 1.1e-2 (two digits;
    the largest is 0.01104), decades away from both 1 and the tolerance."""
    dt = np.dtype(dtype)
    n, rp, ci, vt, B = MC.system("tri200", dt)
    A = M.scipy_csr(n, rp, ci, vt)
    for j in (0, 3, 4, 5, 6, 7):
        m = M.Mirror(A, dt); m.begin(B[:, j]); m.iterate(3)
        assert 1e-3 <= m.rr / m.bb <= 1.15e-2, (j, m.rr / m.bb)
