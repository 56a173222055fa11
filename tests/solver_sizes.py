"""The sizes at which the solvers' streaming kernels change regime (a helper, not a test): a Python copy of the walk of tilespmv_amd/csrc/hip_solver_common.h, the case table of
tests/test_gpu_solver_sizes.py, and the inputs of those cases.  tests/test_solver_sizes_cpu.py checks the copy against the header and every case against the regime it claims.

The walk: a stream of `elements` values is nv = elements // vpl lane vectors of 16 bytes (vpl = 2 in fp64, 4 in fp32) plus a scalar tail of elements % vpl values.  One workgroup
trip covers TRIP = SV_U * SVB lane vectors; parts() workgroups (= partial sums) walk the lane vectors in sweeps of parts() * TRIP, capped at SV_MAX_PARTS.  A consuming kernel folds
the partials 256 at a time (thread t adds t, t + 256, ...)."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

SVB, SV_U, SV_MAX_PARTS = 256, 2, 1024
TRIP = SV_U * SVB

DTYPES = [np.dtype(np.float64), np.dtype(np.float32)]


def vpl(dtype):
    return 16 // np.dtype(dtype).itemsize


def parts(elements, vpl):
    """solver_parts(elements): workgroups = partial sums."""
    trips = (elements // vpl + TRIP - 1) // TRIP
    return max(1, min(SV_MAX_PARTS, trips))


Walk = namedtuple("Walk", "parts sweeps last_trip tail")


def walk(elements, vpl):
    """(partials, sweeps over the workgroups, valid lane vectors of the last trip when it is a partial one (0: every trip is full), scalar tail length)."""
    nv = elements // vpl
    np_ = parts(elements, vpl)
    trips = (nv + TRIP - 1) // TRIP
    return Walk(np_, (trips + np_ - 1) // np_, nv % TRIP, elements % vpl)


def fold_passes(partials, nvec=1):
    """Iterations of the loop of fold() / fold_cols() in its busiest thread."""
    return (partials * nvec + SVB - 1) // SVB


# ---- the case table
CAPPED_NV = 526124            # 1024 full trips, then a second sweep: workgroups 0-2 full, workgroup 3 with 300 lane vectors (u = 0 full, u = 1: 44 threads)
FOLD2_NV = 300 * TRIP         # 300 partials, one sweep: the fold's second pass adds partials 256 .. 299


def capped_n(dtype):
    """1 052 249 (fp64) / 2 104 499 (fp32): CAPPED_NV lane vectors and the longest scalar tail."""
    return vpl(dtype) * CAPPED_NV + vpl(dtype) - 1


def fold2_n(dtype):
    """307 201 (fp64) / 614 403 (fp32)."""
    return vpl(dtype) * FOLD2_NV + vpl(dtype) - 1


def single_n(case, dtype):
    return {"capped": capped_n, "fold2": fold2_n}[case](dtype)


def multi_rows(case, nvec, dtype):
    """Rows of the multi-RHS cases: the flat stream rows * nvec has CAPPED_NV (FOLD2_NV) lane vectors; fp32 with nvec = 2 gets an odd row count, the tail is one whole row."""
    nv = {"capped": CAPPED_NV, "fold2": FOLD2_NV}[case]
    elements = nv * vpl(dtype)
    rows = elements // nvec
    if case == "capped" and nvec < vpl(dtype):
        rows += 1
        assert rows * nvec - elements == nvec
    return rows


MULTI_CASES = [("capped", 8), ("capped", 4), ("capped", 2), ("fold2", 8)]


def cgls_shape(case, dtype):
    """tall: capped rows, 300-partial columns; wide: the two lengths swapped."""
    long_, short = capped_n(dtype), fold2_n(dtype)
    return {"tall": (long_, short), "wide": (short, long_)}[case]


TINY_N = [1, 2, 3, 5]
TINY_NVEC = [2, 4, 8]
TINY_CGLS = [(1, 1), (3, 2), (2, 3), (5, 3)]


# ---- inputs
def tridiagonal(n, lower, diag, upper):
    """(n, rp, ci, float64 values) of the n x n tridiagonal matrix with constant diagonals, rp / ci as int32."""
    i = np.arange(n)
    r = np.concatenate([i[1:], i, i[:-1]])
    c = np.concatenate([i[:-1], i, i[1:]])
    v = np.concatenate([np.full(n - 1, float(lower)), np.full(n, float(diag)), np.full(n - 1, float(upper))])
    A = sp.csr_matrix((v, (r, c)), shape=(n, n))
    A.sort_indices()
    return n, np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64)


def spd_tridiagonal(n):
    """(-1, 3, -1): symmetric, Gershgorin puts the spectrum in [1, 5]."""
    return tridiagonal(n, -1.0, 3.0, -1.0)


def nonsymmetric_tridiagonal(n):
    """(-1.5, 3, -0.5): row sums of the magnitudes off the diagonal are 2 < 3."""
    return tridiagonal(n, -1.5, 3.0, -0.5)


def two_identity(n):
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    return n, rp, ci, np.full(n, 2.0)


def diagonal_preconditioner(n):
    """A positive diagonal that VARIES from row to row (period 7, so no lane, trip or column pattern hides a wrong index), close to 1 / 3: the dinv of the preconditioned cases."""
    return 1.0 / (3.0 + (np.arange(n) % 7) / 7.0)


def exact_rhs(n):
    """b[i] cycles through the nonzero integers of [-30, 30] (Knuth's multiplicative hash mod 61, zero remapped to 17): every product and partial sum of the solvers' first
    iteration on 2 I is an integer below 2^53, the same bits in any summation order."""
    b = (np.arange(n, dtype=np.int64) * 2654435761) % 61 - 30
    b[b == 0] = 17
    return b.astype(np.float64)


def exact_bb(b):
    """The sum of the squares as a Python int."""
    return int((b.astype(np.int64) ** 2).sum())


def exact_columns(n, nvec):
    """B[:, c] = (c + 1) x the cyclic shift of exact_rhs(n) by c + 1 rows: the columns differ element for element and bb_c = (c + 1)^2 bb differs from column to column, so a
    partial sum or a scalar that reaches the wrong column shows."""
    b = exact_rhs(n)
    return np.ascontiguousarray(np.stack([(c + 1) * np.roll(b, c + 1) for c in range(nvec)], axis=1))


def tiny_cgls_matrix(rows, cols):
    """A dense rows x cols matrix of full rank min(rows, cols), stored as a full CSR: values in [0.5, 1.5] with signs, the main diagonal raised by 2."""
    rng = np.random.default_rng(100 * rows + cols)
    D = rng.uniform(0.5, 1.5, (rows, cols)) * rng.choice([-1.0, 1.0], (rows, cols))
    k = min(rows, cols)
    D[np.arange(k), np.arange(k)] = 2.0 + np.abs(D[np.arange(k), np.arange(k)])
    A = sp.csr_matrix(D)
    A.sort_indices()
    assert A.nnz == rows * cols
    return np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64), D
