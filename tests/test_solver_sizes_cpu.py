"""The ledger of tests/test_gpu_solver_sizes.py: the Python copy of the solvers' walk (tests/solver_sizes.py) agrees with tilespmv_amd/csrc/hip_solver_common.h, every case of the
table reaches the regime it is there for, in both value types, and the numpy mirrors give the closed forms the exact cases assert on the GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_mirror as BM
import cg_mirror as M
import cgls_mirror as LM
import solver_sizes as Z

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tilespmv_amd", "csrc", "hip_solver_common.h")
DTYPES = Z.DTYPES


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_constants_are_the_headers():
    text = _header()
    got = {name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1)) for name in ("SVB", "SV_U", "SV_MAX_PARTS")}
    assert got == {"SVB": Z.SVB, "SV_U": Z.SV_U, "SV_MAX_PARTS": Z.SV_MAX_PARTS}
    assert re.search(r"SV_VPL\s*=\s*16\s*/\s*\(int\)sizeof\(val_t\)", text)
    assert Z.vpl(np.float64) == 2 and Z.vpl(np.float32) == 4
    # the shape of the walk and of the fold that the copy repeats
    assert re.search(r"trips\s*=\s*\(elements / SV_VPL \+ \(long long\)SV_U \* SVB - 1\) / \(\(long long\)SV_U \* SVB\)", text)
    assert re.search(r"std::max<long long>\(1, std::min<long long>\(SV_MAX_PARTS, trips\)\)", text)
    assert re.search(r"base \+= \(long long\)\(nwg\) \* \(SV_U \* SVB\)", text)
    assert re.search(r"for \(int i = threadIdx\.x; i < np; i \+= SVB\)", text)


def test_the_cap_is_where_the_issue_says():
    """The first length with more trips than SV_MAX_PARTS: 1 048 578 in fp64, 2 097 156 in fp32."""
    for dt, first in ((np.float64, 1048578), (np.float32, 2097156)):
        v = Z.vpl(dt)
        assert Z.walk(first, v).sweeps == 2 and Z.walk(first - 1, v).sweeps == 1 and Z.walk(first - 1, v).parts == Z.SV_MAX_PARTS


@pytest.mark.parametrize("dtype", DTYPES)
def test_capped_two_sweeps_a_partial_last_trip_and_a_tail(dtype):
    v = Z.vpl(dtype)
    n = Z.capped_n(dtype)
    assert n == {2: 1052249, 4: 2104499}[v]
    w = Z.walk(n, v)
    assert w == Z.Walk(Z.SV_MAX_PARTS, 2, 300, v - 1)
    # the second sweep: 1836 lane vectors = workgroups 0-2 full, workgroup 3 with 300 (u = 0 full, u = 1 with 44 threads)
    left = n // v - Z.SV_MAX_PARTS * Z.TRIP
    assert left == 3 * Z.TRIP + 300 and 300 - Z.SVB == 44
    assert Z.fold_passes(w.parts) == 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_uncapped_fold_in_two_passes(dtype):
    v = Z.vpl(dtype)
    n = Z.fold2_n(dtype)
    assert n == {2: 307201, 4: 614403}[v]
    w = Z.walk(n, v)
    assert w == Z.Walk(300, 1, 0, v - 1) and Z.fold_passes(w.parts) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_cases(dtype):
    v = Z.vpl(dtype)
    want_rows = {(8, 2): 131531, (8, 4): 263062, (4, 2): 263062, (4, 4): 526124, (2, 2): 526124, (2, 4): 1052249}
    for case, nvec in Z.MULTI_CASES:
        rows = Z.multi_rows(case, nvec, dtype)
        w = Z.walk(rows * nvec, v)
        if case == "capped":
            assert rows == want_rows[(nvec, v)]
            tail = 2 if (nvec, v) == (2, 4) else 0          # fp32, nvec = 2, odd rows: the tail is one whole row
            assert w == Z.Walk(Z.SV_MAX_PARTS, 2, 300, tail), (nvec, w)
        else:
            assert w == Z.Walk(300, 1, 0, 0) and Z.fold_passes(w.parts, nvec) > 2
        # what hip_solver_mv.hip's "a thread meets the same columns in every trip" rests on
        lpr = max(1, nvec // v)
        assert Z.TRIP % lpr == 0 and Z.SVB % lpr == 0 and 64 % lpr == 0 and (w.parts * Z.TRIP) % lpr == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cgls_caps_one_length_and_not_the_other(dtype):
    v = Z.vpl(dtype)
    rows, cols = Z.cgls_shape("tall", dtype)
    assert (Z.parts(rows, v), Z.parts(cols, v)) == (Z.SV_MAX_PARTS, 300) and Z.walk(rows, v).sweeps == 2 and Z.walk(cols, v).sweeps == 1
    rows, cols = Z.cgls_shape("wide", dtype)
    assert (Z.parts(rows, v), Z.parts(cols, v)) == (300, Z.SV_MAX_PARTS) and Z.walk(rows, v).sweeps == 1 and Z.walk(cols, v).sweeps == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_cases_reach_a_stream_without_a_lane_vector(dtype):
    v = Z.vpl(dtype)
    none = [n for n in Z.TINY_N if Z.walk(n, v) == Z.Walk(1, 0, 0, n)]
    assert none == [n for n in Z.TINY_N if n < v] and 1 in none
    for n in Z.TINY_N:
        w = Z.walk(n, v)
        assert w.parts == 1 and w.tail == n % v and w.last_trip == n // v
    assert any(Z.walk(r, v).sweeps == 0 for r, c in Z.TINY_CGLS) and any(Z.walk(c, v).sweeps == 0 for r, c in Z.TINY_CGLS)
    # multi-RHS: the flat stream has no lane vector only in fp32 with one row of two columns
    flat_none = [(r, k) for r in Z.TINY_N for k in Z.TINY_NVEC if r * k < v]
    assert flat_none == ([(1, 2)] if v == 4 else [])


def test_the_largest_stream_of_the_older_solver_tests_stays_under_the_cap():
    """tri200 x 8 columns: 320 000 elements, 313 partials in fp64 (157 in fp32); no older case makes a second sweep."""
    assert Z.walk(320000, 2) == Z.Walk(313, 1, 256, 0) and Z.walk(320000, 4).parts == 157
    assert Z.walk(40000, 2) == Z.Walk(40, 1, 32, 0) and Z.fold_passes(40) == 1


# ---- the closed forms of the exact cases, on the mirrors
def test_exact_rhs():
    for dt in DTYPES:
        n = Z.capped_n(dt)
        b = Z.exact_rhs(n)
        assert b.min() == -30 and b.max() == 30 and not (b == 0).any() and len(np.unique(b)) == 60
        assert np.array_equal(b.astype(dt).astype(np.float64), b)
        assert Z.exact_bb(b) < 2 ** 53 and 64 * 16 * Z.exact_bb(b) < 2 ** 53      # (times the largest column factor squared, times CGLS's 16)
        B = Z.exact_columns(1000, 8)
        assert len({Z.exact_bb(B[:, c]) for c in range(8)}) == 8 and all(Z.exact_bb(B[:, c]) == (c + 1) ** 2 * Z.exact_bb(Z.exact_rhs(1000)) for c in range(8))


def _two_identity(n, dt):
    return sp.identity(n, dtype=dt, format="csr") * dt.type(2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("jacobi", [False, True])
def test_cg_mirror_on_two_identity(jacobi, dtype):
    dt = np.dtype(dtype)
    n = Z.capped_n(dt)
    b = Z.exact_rhs(n).astype(dt)
    m = M.Mirror(_two_identity(n, dt), dt, np.full(n, 0.5, dtype=dt) if jacobi else None)
    m.begin(b)
    assert m.bb == Z.exact_bb(b) and m.rr == m.bb
    m.iterate(1)
    assert np.array_equal(m.x, b / dt.type(2)) and m.rr == 0.0 and m.status() == M.CONVERGED
    m.iterate(16)
    assert np.array_equal(m.x, b / dt.type(2)) and m.rr == 0.0 and m.status() == M.CONVERGED and m.iterations == 17


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_mirror_per_column_on_two_identity(dtype):
    dt = np.dtype(dtype)
    for case, nvec in Z.MULTI_CASES[:3]:
        rows = Z.multi_rows(case, nvec, dt)
        B = Z.exact_columns(rows, nvec).astype(dt)
        A = _two_identity(rows, dt)
        for c in (0, nvec - 1):
            m = M.Mirror(A, dt)
            m.begin(B[:, c])
            assert m.bb == (c + 1) ** 2 * Z.exact_bb(Z.exact_rhs(rows))
            m.iterate(1)
            assert np.array_equal(m.x, B[:, c] / dt.type(2)) and m.rr == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bicgstab_mirror_on_two_identity(dtype):
    """alpha = 1/2 gives s = 0, t = 0, omega = 0: converged at the half step."""
    dt = np.dtype(dtype)
    n = Z.capped_n(dt)
    b = Z.exact_rhs(n).astype(dt)
    m = BM.Mirror(_two_identity(n, dt), dt)
    m.begin(b)
    assert m.bb == Z.exact_bb(b)
    m.iterate(1)
    assert np.array_equal(m.x, b / dt.type(2)) and m.rr == 0.0 and m.status() == BM.CONVERGED
    m.iterate(16)
    assert np.array_equal(m.x, b / dt.type(2)) and m.status() == BM.CONVERGED and m.iterations == 17


@pytest.mark.parametrize("dtype", DTYPES)
def test_cgls_mirror_on_two_identity(dtype):
    """s = 2 b, q = 4 b: alpha = 4 bb / 16 bb = 1/4."""
    dt = np.dtype(dtype)
    n = Z.capped_n(dt)
    b = Z.exact_rhs(n).astype(dt)
    m = LM.Mirror(_two_identity(n, dt), dt)
    m.begin(b, damp=0.0)
    bb = Z.exact_bb(b)
    assert m.bb == bb and m.rr == bb and m.nn == 4 * bb and m.nn0 == 4 * bb
    m.iterate(1)
    assert np.array_equal(m.x, b / dt.type(2)) and m.rr == 0.0 and m.nn == 0.0 and m.status() == LM.CONVERGED
    m.iterate(16)
    assert np.array_equal(m.x, b / dt.type(2)) and m.status() == LM.CONVERGED


def test_tiny_cgls_matrices_have_full_rank():
    for rows, cols in Z.TINY_CGLS:
        D = Z.tiny_cgls_matrix(rows, cols)[3]
        assert np.linalg.matrix_rank(D) == min(rows, cols)
