"""The reference the GPU solver is compared with (a helper, not a test): a numpy restatement of the recurrences of tilespmv_cg_* (include/tilespmv.h),
written for clarity and sharing nothing with the code under test.

    x, r, p live in the build's value type; rho = r.z, p.Ap, r.r are accumulated in float64; z = dinv o r (the value type); alpha, beta are formed in float64 and rounded to the
    value type once, where they multiply; the product A p is scipy's CSR product in the value type.
    guards: rho = 0 -> alpha = beta = 0;  rho > 0 and not p.Ap > 0, or rho < 0 -> breakdown: alpha = beta = 0 from then on.

Also the inputs of tests/test_cg_cpu.py and tests/test_gpu_cg.py (all from tilespmv_amd.generators), so that both files solve the same systems.
"""
import numpy as np
import scipy.sparse as sp

from tilespmv_amd import generators as G

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}


def _dot64(u, v):
    return float(np.dot(u.astype(np.float64), v.astype(np.float64)))


class Mirror:
    """begin / iterate / solve with the meaning of the C entry points.  ``A``: scipy CSR (any value type; converted), ``dinv``: None or the inverse diagonal."""

    def __init__(self, A, dtype, dinv=None):
        self.dt = np.dtype(dtype)
        self.A = sp.csr_matrix(A, dtype=self.dt)
        self.dinv = None if dinv is None else np.asarray(dinv, dtype=self.dt)

    def _z(self, r):
        return r if self.dinv is None else (self.dinv * r).astype(self.dt)

    def begin(self, b, x0=None):
        dt = self.dt
        self.b = np.asarray(b, dtype=dt)
        self.x = np.zeros(self.A.shape[0], dtype=dt) if x0 is None else np.array(x0, dtype=dt)
        self.r = (self.b - self.A @ self.x).astype(dt)
        self.p = self._z(self.r).copy()
        self.rho = _dot64(self.r, self.p)
        self.rr = _dot64(self.r, self.r)
        self.bb = _dot64(self.b, self.b)
        self.iterations, self.breakdown = 0, False

    def iterate(self, count=1):
        dt = self.dt
        for _ in range(count):
            Ap = (self.A @ self.p).astype(dt)
            pap = _dot64(self.p, Ap)
            rho = 0.0 if self.breakdown else self.rho
            if rho < 0.0 or (rho > 0.0 and not pap > 0.0):
                self.breakdown = True
            alpha = dt.type(rho / pap if (rho > 0.0 and pap > 0.0) else 0.0)
            self.x = (self.x + alpha * self.p).astype(dt)
            self.r = (self.r - alpha * Ap).astype(dt)
            z = self._z(self.r)
            rho_new = _dot64(self.r, z)
            self.rr = _dot64(self.r, self.r)
            beta = dt.type(rho_new / rho if (rho > 0.0 and not self.breakdown) else 0.0)
            self.p = (z + beta * self.p).astype(dt)
            self.rho = rho_new
            self.iterations += 1

    def status(self):
        return BREAKDOWN if self.breakdown else CONVERGED if self.rr == 0.0 else RUNNING

    def solve(self, b, x0=None, rtol=1e-10, maxiter=1000, check_every=8):
        """Returns (x, iterations, status, sqrt(rr / bb))."""
        self.begin(b, x0)
        while True:
            if self.breakdown:
                return self.x, self.iterations, BREAKDOWN, self.rel()
            if self.bb == 0.0:
                self.x[:] = 0
                self.rr = 0.0
                return self.x, self.iterations, CONVERGED, 0.0
            if self.rr <= rtol * rtol * self.bb:
                return self.x, self.iterations, CONVERGED, self.rel()
            if self.iterations >= maxiter:
                return self.x, self.iterations, MAXITER, self.rel()
            self.iterate(min(check_every, maxiter - self.iterations))

    def rel(self):
        return (self.rr / self.bb) ** 0.5 if self.bb > 0 else 0.0


# ---- inputs
def spd_values(n, rp, ci):
    """Diagonally dominant symmetric values on a symmetric pattern: -1 off the diagonal, degree + 1 on it (as tests/test_halo_gloo.py::_spd_values)."""
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = np.where(ci == rows, 0.0, -1.0)
    deg = np.bincount(rows, weights=(ci != rows).astype(np.float64), minlength=n)
    v[ci == rows] = deg[rows[ci == rows]] + 1.0
    return v


def laplacian_values(n, rp, ci):
    """The 5-point Laplacian itself: 4 on the diagonal, -1 beside it."""
    rows = np.repeat(np.arange(n), np.diff(rp))
    return np.where(ci == rows, 4.0, -1.0)


def rhs(n):
    return np.random.default_rng(3).uniform(-1, 1, n)


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name in ("lap128", "lap128_scaled"):
        m, n, rp, ci = G.laplacian5pt(128)
        v = laplacian_values(n, rp, ci)
        if name == "lap128_scaled":   # S A S with s = 10^U(-1.5, 1.5): the diagonal spans six decades, the Jacobi-scaled matrix is the Laplacian again
            s = 10.0 ** np.random.default_rng(5).uniform(-1.5, 1.5, n)
            rows = np.repeat(np.arange(n), np.diff(rp))
            v = s[rows] * v * s[ci]
    elif name == "tri200":
        m, n, rp, ci = G.tri_mesh(200, 200, shuffle=1024)
        v = spd_values(n, rp, ci)
    elif name == "fem12":
        m, n, rp, ci = G.fem_hex(12, 12, 12, 3)
        v = spd_values(n, rp, ci)
    else:
        raise KeyError(name)
    assert m == n
    return n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


def scipy_csr(n, rp, ci, v):
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def spsolve_x(n, rp, ci, v, b):
    import scipy.sparse.linalg as spla
    return spla.spsolve(scipy_csr(n, rp, ci, v).tocsc(), b)
