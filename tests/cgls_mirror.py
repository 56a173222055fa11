"""The reference the GPU least-squares solver is compared with (a helper, not a test): a numpy restatement of the recurrences of tilespmv_cgls_* (include/tilespmv.h, DESIGN.md
§3.9), written for clarity and sharing nothing with the code under test.

    min |A x - b|^2 + damp^2 |x|^2 by CGLS: r, q (rows) and x, p, s (cols) live in the build's value type; gamma = s.z, delta = q.q + damp^2 p.p, nn = s.s, rr = r.r are
    accumulated in float64; z = cinv o s (the value type); alpha, beta and damp^2 are formed in float64 and rounded to the value type once, where they multiply; the products
    A p and A^T r are scipy's CSR products in the value type.
    guards: gamma = 0 -> alpha = beta = 0;  gamma < 0, or gamma > 0 without delta > 0 -> breakdown: alpha = beta = 0 from then on.

Also the inputs of tests/test_cgls_cpu.py and tests/test_gpu_cgls.py (all from tilespmv_amd.generators), so that both files solve the same problems.
"""
import numpy as np
import scipy.sparse as sp

from tilespmv_amd import generators as G

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}


def _dot64(u, v):
    return float(np.dot(u.astype(np.float64), v.astype(np.float64)))


class Mirror:
    """begin / iterate / solve with the meaning of the C entry points.  ``A``: scipy CSR of any shape (any value type; converted), ``cinv``: None or a diagonal of ``cols``."""

    def __init__(self, A, dtype, cinv=None):
        self.dt = np.dtype(dtype)
        self.A = sp.csr_matrix(A, dtype=self.dt)
        self.AT = sp.csr_matrix(self.A.T)
        self.cinv = None if cinv is None else np.asarray(cinv, dtype=self.dt)

    def _z(self, s):
        return s if self.cinv is None else (self.cinv * s).astype(self.dt)

    def _normal(self, r, x):
        s = (self.AT @ r).astype(self.dt)
        if self.damp2 != 0.0:
            s = (s - self.dt.type(self.damp2) * x).astype(self.dt)
        return s

    def begin(self, b, x0=None, damp=0.0):
        dt = self.dt
        self.damp2 = float(damp) * float(damp)
        self.b = np.asarray(b, dtype=dt)
        self.x = np.zeros(self.A.shape[1], dtype=dt) if x0 is None else np.array(x0, dtype=dt)
        self.r = (self.b - self.A @ self.x).astype(dt)
        self.s = self._normal(self.r, self.x)
        self.p = self._z(self.s).copy()
        self.gamma = _dot64(self.s, self.p)
        self.nn = _dot64(self.s, self.s)
        self.rr = _dot64(self.r, self.r)
        self.bb = _dot64(self.b, self.b)
        atb = (self.AT @ self.b).astype(dt)
        self.nn0 = _dot64(atb, atb)
        self.iterations, self.breakdown = 0, False

    def iterate(self, count=1):
        dt = self.dt
        for _ in range(count):
            q = (self.A @ self.p).astype(dt)
            delta = _dot64(q, q)
            if self.damp2 != 0.0:
                delta += self.damp2 * _dot64(self.p, self.p)
            gamma = 0.0 if self.breakdown else self.gamma
            if gamma < 0.0 or (gamma > 0.0 and not delta > 0.0):
                self.breakdown = True
            alpha = dt.type(gamma / delta if (gamma > 0.0 and delta > 0.0) else 0.0)
            self.x = (self.x + alpha * self.p).astype(dt)
            self.r = (self.r - alpha * q).astype(dt)
            self.s = self._normal(self.r, self.x)
            z = self._z(self.s)
            gamma_new = _dot64(self.s, z)
            self.nn = _dot64(self.s, self.s)
            self.rr = _dot64(self.r, self.r)
            beta = dt.type(gamma_new / gamma if (gamma > 0.0 and not self.breakdown) else 0.0)
            self.p = (z + beta * self.p).astype(dt)
            self.gamma = gamma_new
            self.iterations += 1

    def status(self):
        return BREAKDOWN if self.breakdown else CONVERGED if self.nn == 0.0 else RUNNING

    def solve(self, b, x0=None, damp=0.0, rtol=1e-10, maxiter=1000, check_every=8):
        """Returns (x, iterations, status, sqrt(nn / nn0))."""
        if check_every < 1:
            check_every = 1
        self.begin(b, x0, damp)
        while True:
            if self.breakdown:
                return self.x, self.iterations, BREAKDOWN, self.rel()
            if self.nn0 == 0.0:
                self.x[:] = 0
                self.nn = 0.0
                return self.x, self.iterations, CONVERGED, 0.0
            if self.nn <= rtol * rtol * self.nn0:
                return self.x, self.iterations, CONVERGED, self.rel()
            if self.iterations >= maxiter:
                return self.x, self.iterations, MAXITER, self.rel()
            self.iterate(min(check_every, maxiter - self.iterations))

    def rel(self):
        return (self.nn / self.nn0) ** 0.5 if self.nn0 > 0 else 0.0


# ---- inputs
def rhs(n):
    return np.random.default_rng(3).uniform(-1, 1, n)


def _scattered(rows, cols):
    """Six random columns per row plus the entries (j, j), values uniform(0.5, 1.5) with a random sign."""
    rng = np.random.default_rng(13)
    r, c = np.repeat(np.arange(rows), 6), rng.integers(0, cols, rows * 6)
    k = min(rows, cols)
    r = np.concatenate([r, np.arange(k)]); c = np.concatenate([c, np.arange(k)])
    _, _, rp, ci = G.from_coo(rows, cols, r, c)
    nnz = int(rp[rows])
    v = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    return rp, ci, v


def problem(name):
    """(rows, cols, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name in ("tall", "tall_scaled"):
        rows, cols = 40000, 6000
        rp, ci, v = _scattered(rows, cols)
        if name == "tall_scaled":   # column j times 10^U(-1.5, 1.5): the column norms span three decades, the column-scaled normal matrix is tall's again
            v = v * (10.0 ** np.random.default_rng(5).uniform(-1.5, 1.5, cols))[ci]
    elif name == "wide":            # underdetermined, with empty columns
        rows, cols = 6000, 40000
        rp, ci, v = _scattered(rows, cols)
    elif name == "square":          # non-symmetric and row-diagonally dominant: off-diagonal values in (-1, 1), the diagonal 1 + 2 x the sum of their magnitudes
        rows = cols = 20000
        _, _, rp, ci = G.band_plus_random(rows, 2, 3, seed=17)
        rowid = np.repeat(np.arange(rows), np.diff(rp))
        v = np.random.default_rng(19).uniform(-1, 1, len(ci))
        off = np.bincount(rowid, weights=np.where(ci == rowid, 0.0, np.abs(v)), minlength=rows)
        v[ci == rowid] = 1.0 + 2.0 * off[rowid[ci == rowid]]
    elif name == "stacked":         # [L; I] on the 5-point Laplacian of a 128 x 128 grid: A^T A = L^2 + I
        _, n, lrp, lci = G.laplacian5pt(128)
        rowid = np.repeat(np.arange(n), np.diff(lrp))
        L = sp.csr_matrix((np.where(lci == rowid, 4.0, -1.0), lci, lrp), shape=(n, n))
        A = sp.vstack([L, sp.identity(n, format="csr")], format="csr")
        A.sort_indices()
        rows, cols, rp, ci, v = 2 * n, n, A.indptr, A.indices, A.data
    else:
        raise KeyError(name)
    return rows, cols, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


def orthogonal_case(n, dtype):
    """A = [2 I; 0] (2n x n) and a b that lives in the empty rows: A^T b = 0 exactly."""
    A = sp.vstack([sp.identity(n, format="csr") * 2.0, sp.csr_matrix((n, n))], format="csr").astype(dtype)
    b = np.concatenate([np.zeros(n), rhs(n)]).astype(dtype)
    return A, b


def scipy_csr(rows, cols, rp, ci, v):
    return sp.csr_matrix((v, ci, rp), shape=(rows, cols))


def column_cinv(A, dtype):
    """1 / |a_j|^2 in the value type, 1 for an empty column: sums in float64 in row order of A^T, as tilespmv_csr_row_sqnorms_device makes them."""
    dt = np.dtype(dtype)
    A = sp.csr_matrix(A, dtype=dt)
    sq = np.asarray(A.astype(np.float64).multiply(A.astype(np.float64)).sum(axis=0)).ravel().astype(dt)
    return np.where(sq == 0, dt.type(1), dt.type(1) / np.where(sq == 0, dt.type(1), sq)).astype(dt)


def lsqr_x(A, b, damp=0.0, scale_columns=False):
    """The (damped, minimum-norm) least-squares solution in float64 by scipy's LSQR, run to its limits.  ``scale_columns`` (full column rank, damp = 0): LSQR on A D with
    D = diag(1 / |a_j|), x = D y — the same solution, reached where LSQR on the badly scaled A itself stalls early."""
    import scipy.sparse.linalg as spla
    A = sp.csr_matrix(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if scale_columns:
        assert damp == 0.0
        d = 1.0 / np.sqrt(np.asarray(A.multiply(A).sum(axis=0)).ravel())
        return d * spla.lsqr(A @ sp.diags(d), b, atol=1e-14, btol=1e-14, conlim=0, iter_lim=20000)[0]
    return spla.lsqr(A, b, damp=damp, atol=1e-14, btol=1e-14, conlim=0, iter_lim=20000)[0]
