"""The reference the FSAI preconditioner is compared with (a helper, not a test): numpy restatements of tilespmv_fsai_create / _update and _apply (include/tilespmv.h,
DESIGN.md §3.15) and of the CG recurrence with that preconditioner, written for clarity and sharing nothing with the code under test.

    pattern  row i of G: the stored columns <= i of row i of A, the MAX_ROW largest where there are more.
    factor   per row, with P its m pattern columns: S = A[P, P] read from the lower triangle of A alone, in float64; numpy.linalg.cholesky(S) (a pivot that is not > 0 raises),
             S y = e_m by numpy.linalg.solve on the factor, g = y / sqrt(y_m), rounded to the value type once.  A row whose factorisation fails, or whose factor is not
             finite, FALLS BACK: zeros, 1 / sqrt(a_ii) on the diagonal where a_ii > 0 and 1 otherwise.
    apply    t = G r and z = G^T t: G in the value type, products and sums in float64, t and z each rounded to the value type once.
    CG       tests/cg_mirror.py's recurrences with z = apply(r) (the mirror there forms z once per iteration and uses it for rho and for p: a stored z).

Also the inputs of tests/test_fsai_cpu.py and tests/test_gpu_fsai.py, so that both files work on the same systems.
"""
import numpy as np
import scipy.sparse as sp

import block_jacobi_mirror as BJM
import cg_mirror as CM
from block_jacobi_mirror import tri_capped                      # noqa: F401
from cg_mirror import rhs, scipy_csr, spd_values, spsolve_x     # noqa: F401

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = CM.RTOL
MAX_ROW = 64


# ---- pattern
def pattern(n, rp, ci):
    """(gp int32 [n + 1], gci int32, src int64: the position in A's arrays of every entry of G, truncated rows)."""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    inner = np.ones(len(ci), dtype=bool)
    inner[rp[:-1]] = False                                              # (the first entry of a row has no left neighbour in it)
    assert (np.diff(ci)[inner[1:]] > 0).all(), "ascending columns"
    lower = np.bincount(rows[ci <= rows], minlength=n)                  # (ascending: the entries at or left of the diagonal lead the row)
    assert (lower >= 1).all() and (ci[rp[:-1] + lower - 1] == np.arange(n)).all(), "a stored diagonal"
    m = np.minimum(lower, MAX_ROW)
    gp = np.concatenate([[0], np.cumsum(m)])
    src = np.repeat(rp[:-1] + lower - m - gp[:-1], m) + np.arange(gp[-1])
    return gp.astype(np.int32), np.ascontiguousarray(ci[src], dtype=np.int32), src, int((lower > MAX_ROW).sum())


def local_matrices(n, rp, ci, v, gp, gci):
    """{m: (rows of G of length m, their S_i = A[P_i, P_i] as float64 [k, m, m])}, read from the lower triangle of A alone (S_ab = a_{max, min})."""
    rp64, ci64 = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp64))
    low = ci64 <= rows
    keys, vals = rows[low] * n + ci64[low], np.asarray(v, dtype=np.float64)[low]          # (ascending: CSR order is key order)
    lens, out = np.diff(gp), {}
    for m in np.unique(lens):
        idx = np.flatnonzero(lens == m)
        P = gci[gp[idx][:, None] + np.arange(m)[None, :]].astype(np.int64)                 # [k, m]
        want = np.maximum(P[:, :, None], P[:, None, :]) * n + np.minimum(P[:, :, None], P[:, None, :])
        at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
        out[int(m)] = (idx, np.where(keys[at] == want, vals[at], 0.0))
    return out


# ---- factor
def solve_rows(S):
    """(rows of G in float64 [k, m], mask of those that fell back) for a stack of local matrices [k, m, m]."""
    k, m, _ = S.shape
    e = np.zeros((m, 1))
    e[-1] = 1.0
    try:                                                                   # (all at once where every row is regular)
        L = np.linalg.cholesky(S)
        y = np.linalg.solve(L.transpose(0, 2, 1), np.linalg.solve(L, e))[:, :, 0]
        if np.isfinite(y).all() and (y[:, -1] > 0).all():
            return y / np.sqrt(y[:, -1:]), np.zeros(k, dtype=bool)
    except np.linalg.LinAlgError:
        pass
    g, fell = np.zeros((k, m)), np.zeros(k, dtype=bool)
    for i in range(k):
        try:
            L = np.linalg.cholesky(S[i])
            y = np.linalg.solve(L.T, np.linalg.solve(L, e))[:, 0]
            fell[i] = not (np.isfinite(y).all() and y[-1] > 0)
        except np.linalg.LinAlgError:
            fell[i] = True
        if fell[i]:
            g[i, -1] = 1.0 / np.sqrt(S[i, -1, -1]) if S[i, -1, -1] > 0 else 1.0
        else:
            g[i] = y / np.sqrt(y[-1])
    return g, fell


def factor64(n, rp, ci, v):
    """(gp, gci, G's values in float64, mask of the fallback rows, truncated rows, the local matrices)."""
    gp, gci, _, truncated = pattern(n, rp, ci)
    g, fell = np.zeros(gp[-1]), np.zeros(n, dtype=bool)
    local = local_matrices(n, rp, ci, v, gp, gci)
    for m, (idx, S) in local.items():
        gm, fell[idx] = solve_rows(S)
        g[gp[idx][:, None] + np.arange(m)[None, :]] = gm
    return gp, gci, g, fell, truncated, local


def factor(n, rp, ci, v, dtype):
    """(gp, gci, G's values in the value type, number of fallback rows, truncated rows); v is taken as it is (the value type's values, for a comparison with the library)."""
    gp, gci, g, fell, truncated, _ = factor64(n, rp, ci, v)
    return gp, gci, g.astype(np.dtype(dtype)), int(fell.sum()), truncated


def info(n, gp, fallback, truncated):
    """What tilespmv_fsai_info reports, device_bytes and dot_partials aside."""
    return {"rows": n, "nnz": int(gp[-1]), "longest_row": int(np.diff(gp).max()), "truncated_rows": int(truncated), "fallback_rows": int(fallback)}


# ---- apply
def g_csr(n, gp, gci, g):
    """G (values as given: the value type's) as a float64 scipy CSR."""
    return sp.csr_matrix((np.asarray(g).astype(np.float64), gci, gp), shape=(n, n))


def apply(G64, r, dtype):
    """z = G^T (G r): t and z each rounded to the value type once."""
    dt = np.dtype(dtype)
    t = (G64 @ np.asarray(r, dtype=dt).astype(np.float64)).astype(dt)
    return (G64.T @ t.astype(np.float64)).astype(dt)


class CG(CM.Mirror):
    """tests/cg_mirror.py's Mirror with z = G^T (G r); ``G64``: ``g_csr`` of the value type's G."""

    def __init__(self, A, dtype, G64):
        super().__init__(A, dtype)
        self.G64 = sp.csr_matrix(G64, dtype=np.float64)

    def _z(self, r):
        return apply(self.G64, r, self.dt)


# ---- inputs
def band(hb):
    """200 rows, half-bandwidth hb: a_ij = -1 / (1 + |i - j|), diagonal = 1 + the sum of the row's |off-diagonal| (strictly dominant: SPD).  band70: row 63 has exactly 64
    entries at or left of the diagonal and keeps all of them; rows 64 .. 199 have 65 .. 71 and are truncated: 136 rows.  band12 and band25: longest rows of 13 and 26, the
    sizes between those of the other inputs (3, 42, 64) at which the library's value kernel takes its 16- and 32-lane forms."""
    n = 200
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    D = np.where((np.abs(i - j) <= hb) & (i != j), -1.0 / (1.0 + np.abs(i - j)), 0.0)
    D[np.arange(n), np.arange(n)] = 1.0 + np.abs(D).sum(axis=1)
    A = sp.csr_matrix(D)
    A.sort_indices()
    return n, A.indptr, A.indices, A.data


def lap55_neg():
    """lap55 with a_100,100 = -1: exactly rows 100, 101 and 155 hold column 100 in their pattern, their Cholesky meets a pivot of -1 or below, they fall back."""
    n, rp, ci, v = BJM.problem("lap55")
    v = v.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[(rows == 100) & (ci == 100)] = -1.0
    return n, rp, ci, v


NEG_ROWS = (100, 101, 155)
_PROBLEMS = {}


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name not in _PROBLEMS:
        if name in ("lap55", "femblk10"):
            n, rp, ci, v = BJM.problem(name)
        elif name in ("band12", "band25", "band70"):
            n, rp, ci, v = band(int(name[4:]))
        elif name == "lap55_neg":
            n, rp, ci, v = lap55_neg()
        else:
            raise KeyError(name)
        _PROBLEMS[name] = (n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64))
    return _PROBLEMS[name]


_FACTORS = {}


def factored(name, dtype):
    """``factor`` of a named input with its values rounded to the value type, and the float64 rows and local matrices behind it, computed once:
    {"gp", "gci", "g" (value type), "g64", "fell" (mask), "truncated", "S" ({m: (rows, local matrices [k, m, m])})}."""
    dt = np.dtype(dtype)
    if (name, dt) not in _FACTORS:
        n, rp, ci, v = problem(name)
        gp, gci, g64, fell, truncated, local = factor64(n, rp, ci, v.astype(dt))
        _FACTORS[(name, dt)] = {"gp": gp, "gci": gci, "g": g64.astype(dt), "g64": g64, "fell": fell, "truncated": truncated, "S": local}
    return _FACTORS[(name, dt)]
