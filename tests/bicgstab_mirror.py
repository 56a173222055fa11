"""The reference the GPU BiCGStab solver is compared with (a helper, not a test): a numpy restatement of the recurrences of tilespmv_bicgstab_* (include/tilespmv.h, DESIGN.md
§3.10), written for clarity and sharing nothing with the code under test.

    Right-preconditioned BiCGStab, M^-1 = diag(dinv) (dinv = None: phat = p, shat = s).  x, r, rhat, p, v, s, t, phat, shat live in the build's value type; rho = rhat.r,
    sigma = rhat.v, t.s, t.t and rr = r.r are accumulated in float64; alpha, omega, beta are formed in float64 and rounded to the value type once, where they multiply; the
    products A phat and A shat are scipy's CSR products in the value type.
    guards (exact-zero tests):
      rr = 0 at the start of an iteration, or the breakdown flag   nothing changes: x, r, p keep their bits
      rr > 0, and rho = 0 or sigma = 0                             breakdown: nothing changes in this or any later iteration
      t.t = 0 (or t.s = 0)                                         omega = 0: x += alpha phat, r = s, p stays; rr = 0 then: converged at the half step; rr > 0: breakdown
      the iteration counter advances whatever the guards did.

``order``: None, or a permutation of the rows in which every dot product is accumulated (another summation order: tests/test_bicgstab_cpu.py uses it to bound what the order
of the GPU's sums may cost in iterations).

Also the inputs of tests/test_bicgstab_cpu.py and tests/test_gpu_bicgstab.py, so that both files solve the same systems.
"""
import numpy as np
import scipy.sparse as sp

from cg_mirror import rhs, scipy_csr, spsolve_x   # noqa: F401  (the inputs' right-hand side and the direct solution are those of the CG tests)
from tilespmv_amd import generators as G

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}


class Mirror:
    """begin / iterate / solve with the meaning of the C entry points.  ``A``: scipy CSR (any value type; converted), ``dinv``: None or the inverse diagonal."""

    def __init__(self, A, dtype, dinv=None, order=None):
        self.dt = np.dtype(dtype)
        self.A = sp.csr_matrix(A, dtype=self.dt)
        self.dinv = None if dinv is None else np.asarray(dinv, dtype=self.dt)
        self.order = order

    def _dot(self, u, v):
        u, v = u.astype(np.float64), v.astype(np.float64)
        if self.order is not None:
            u, v = u[self.order], v[self.order]
        return float(np.dot(u, v))

    def _hat(self, p):
        return p if self.dinv is None else (self.dinv * p).astype(self.dt)

    def begin(self, b, x0=None):
        dt = self.dt
        self.b = np.asarray(b, dtype=dt)
        self.x = np.zeros(self.A.shape[0], dtype=dt) if x0 is None else np.array(x0, dtype=dt)
        self.r = (self.b - self.A @ self.x).astype(dt)
        self.rhat = self.r.copy()
        self.p = self.r.copy()
        self.rr = self._dot(self.r, self.r)
        self.rho = self.rr
        self.bb = self._dot(self.b, self.b)
        self.iterations, self.breakdown = 0, False

    def _one(self):
        dt = self.dt
        if self.breakdown or self.rr == 0.0:
            return
        phat = self._hat(self.p)
        v = (self.A @ phat).astype(dt)
        sigma = self._dot(self.rhat, v)
        if self.rho == 0.0 or sigma == 0.0:
            self.breakdown = True
            return
        alpha64 = self.rho / sigma
        alpha = dt.type(alpha64)
        s = (self.r - alpha * v).astype(dt)
        shat = self._hat(s)
        t = (self.A @ shat).astype(dt)
        ts, tt = self._dot(t, s), self._dot(t, t)
        omega64 = 0.0 if (tt == 0.0 or ts == 0.0) else ts / tt
        omega = dt.type(omega64)
        self.x = (self.x + alpha * phat + omega * shat).astype(dt)
        self.r = (s - omega * t).astype(dt)
        rho_new = self._dot(self.rhat, self.r)
        self.rr = self._dot(self.r, self.r)
        if omega64 == 0.0:
            if self.rr != 0.0:
                self.breakdown = True
        else:
            beta = dt.type((rho_new / self.rho) * (alpha64 / omega64))
            self.p = (self.r + beta * (self.p - omega * v)).astype(dt)
        self.rho = rho_new

    def iterate(self, count=1):
        for _ in range(count):
            self._one()
            self.iterations += 1

    def status(self):
        return BREAKDOWN if self.breakdown else CONVERGED if self.rr == 0.0 else RUNNING

    def solve(self, b, x0=None, rtol=1e-10, maxiter=1000, check_every=8):
        """Returns (x, iterations, status, sqrt(rr / bb))."""
        if check_every < 1:
            check_every = 1
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
GRID = 67


def convdiff_values(k, n, rp, ci):
    """Convection-diffusion on the pattern of the 5-point Laplacian of a k x k grid (row i = grid point (i // k, i % k)): 4 on the diagonal, -1 - 0.6 / -1 + 0.6 on the west / east
    neighbour (columns i - 1 / i + 1), -1 - 0.3 / -1 + 0.3 on the south / north neighbour (columns i - k / i + k).  Nonsymmetric."""
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = ci.astype(np.int64) - rows
    v = np.zeros(len(ci))
    v[d == 0] = 4.0
    v[d == -1] = -1.6
    v[d == 1] = -0.4
    v[d == -k] = -1.3
    v[d == k] = -0.7
    assert np.all(v != 0)
    return v


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name in ("convdiff67", "convdiff67_scaled"):
        m, n, rp, ci = G.laplacian5pt(GRID)
        v = convdiff_values(GRID, n, rp, ci)
        if name == "convdiff67_scaled":   # S A S with s = 10^U(-1.5, 1.5) (the lap128_scaled construction of cg_mirror): the diagonal spans six decades
            s = 10.0 ** np.random.default_rng(5).uniform(-1.5, 1.5, n)
            rows = np.repeat(np.arange(n), np.diff(rp))
            v = s[rows] * v * s[ci]
    elif name == "skew":                  # 2049 blocks [[0, 1], [-1, 0]]: x.A x = 0 for every x
        m = n = 4098
        rp = np.arange(n + 1)
        ci = np.arange(n) ^ 1
        v = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    elif name == "2I":
        m = n = 4099
        rp, ci, v = np.arange(n + 1), np.arange(n), np.full(n, 2.0)
    else:
        raise KeyError(name)
    assert m == n
    return n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


def skew_rhs(n):
    """Integers in [-8, 8]: every product and sum of the first iteration on `skew` is exact in both value types, so rhat.v = b.A b = 0 exactly."""
    return np.random.default_rng(7).integers(-8, 9, n).astype(np.float64)


def inverse_diagonal(n, rp, ci, v, dtype):
    """1 / a_ii in the value type (every input here stores a nonzero diagonal), as tilespmv_csr_diagonal_device(invert = 1) makes it."""
    dt = np.dtype(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n, dtype=dt)
    d[rows[ci == rows]] = np.asarray(v, dtype=dt)[ci == rows]
    return (dt.type(1) / d).astype(dt)
