"""The reference the GPU MINRES solver is compared with (a helper, not a test): a numpy restatement of the recurrences of tilespmv_minres_* (include/tilespmv.h),
written for clarity and sharing nothing with the code under test.

    Preconditioned Paige-Saunders MINRES for a symmetric A that may be indefinite, M^-1 = diag(minv) with minv > 0 (minv = None: z = r2).  x, r1, r2, y, z, v, w, w1, w2 live in
    the build's value type; r2.z, v.y, y.z' and b.(minv o b) are accumulated in float64; every scalar of the recurrence is float64; 1/beta, alfa/beta, beta/oldb, oldeps, delta,
    1/gamma and phi are rounded to the value type once, where they multiply; the product A v is scipy's CSR product in the value type.
    begin:   r2 = b - A x;  r1 = 0;  z = minv o r2;  beta = sqrt(r2.z);  bb = b.(minv o b);  oldb = dbar = epsln = 0;  phibar = beta;  cs = -1;  sn = 0;  w = w2 = 0;
             rr = r2.z (= phibar^2, kept as the sum itself: no square root in between);  iteration count and breakdown flag cleared
    iterate: v = z / beta;  y = A v;  if oldb != 0: y -= (beta/oldb) r1;  alfa = v.y;  y -= (alfa/beta) r2;  z' = minv o y;  beta' = sqrt(y.z');
             oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  gamma = hypot(gbar, beta');
             r1 = r2;  r2 = y;  z = z';  oldb = beta;  beta = beta';  epsln = sn beta;  dbar = -cs beta;  cs = gbar/gamma;  sn = beta/gamma;  phi = cs phibar;  phibar = sn phibar;
             w1 = w2;  w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  x += phi w;  rr = phibar^2
    guards (exact tests):
      phibar = 0 at the start of an iteration, or the breakdown flag   nothing changes: x keeps its bits (b = 0; beta' = 0, the lucky termination)
      r2.z < 0 (begin) or y.z' < 0                                     M is not positive definite: breakdown, nothing changes in this or any later iteration
      gamma = 0                                                        A is singular on this Krylov space and the system incompatible: breakdown, the same way
      the iteration counter advances whatever the guards did.

``order``: None, or a permutation of the rows in which every dot product is accumulated (another summation order: tests/test_minres_cpu.py uses it to bound what the order of the
GPU's sums may cost in iterations).

Also the inputs of tests/test_minres_cpu.py and tests/test_gpu_minres.py, so that both files solve the same systems.
"""
import math

import numpy as np
import scipy.sparse as sp

from cg_mirror import rhs, scipy_csr, spsolve_x   # noqa: F401  (the inputs' right-hand side and the direct solution are those of the CG tests)
from tilespmv_amd import generators as G

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}


class Mirror:
    """begin / iterate / solve with the meaning of the C entry points.  ``A``: scipy CSR (any value type; converted), ``minv``: None or the positive diagonal M^-1."""

    def __init__(self, A, dtype, minv=None, order=None):
        self.dt = np.dtype(dtype)
        self.A = sp.csr_matrix(A, dtype=self.dt)
        self.minv = None if minv is None else np.asarray(minv, dtype=self.dt)
        self.order = order

    def _dot(self, u, v):
        u, v = u.astype(np.float64), v.astype(np.float64)
        if self.order is not None:
            u, v = u[self.order], v[self.order]
        return float(np.dot(u, v))

    def _m(self, r):
        return r if self.minv is None else (self.minv * r).astype(self.dt)

    def begin(self, b, x0=None):
        dt, n = self.dt, self.A.shape[0]
        self.b = np.asarray(b, dtype=dt)
        self.x = np.zeros(n, dtype=dt) if x0 is None else np.array(x0, dtype=dt)
        self.r2 = (self.b - self.A @ self.x).astype(dt)
        self.r1 = np.zeros(n, dtype=dt)
        self.z = self._m(self.r2)
        self.w, self.w2 = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
        rz = self._dot(self.r2, self.z)
        self.bb = self._dot(self.b, self._m(self.b))
        self.iterations, self.breakdown = 0, rz < 0.0
        self.beta = 0.0 if self.breakdown else math.sqrt(rz)
        self.oldb = self.dbar = self.epsln = 0.0
        self.phibar, self.cs, self.sn = self.beta, -1.0, 0.0
        self.rr = rz
        self.history = [self.rr]

    def _one(self):
        dt = self.dt
        if self.breakdown or self.phibar == 0.0:
            return
        v = (self.z * dt.type(1.0 / self.beta)).astype(dt)
        y = (self.A @ v).astype(dt)
        if self.oldb != 0.0:
            y = (y - dt.type(self.beta / self.oldb) * self.r1).astype(dt)
        alfa = self._dot(v, y)
        y = (y - dt.type(alfa / self.beta) * self.r2).astype(dt)
        zn = self._m(y)
        yz = self._dot(y, zn)
        if yz < 0.0:
            self.breakdown = True
            return
        betan = math.sqrt(yz)
        oldeps = self.epsln
        delta = self.cs * self.dbar + self.sn * alfa
        gbar = self.sn * self.dbar - self.cs * alfa
        gamma = math.hypot(gbar, betan)
        if gamma == 0.0:
            self.breakdown = True
            return
        self.r1, self.r2, self.z = self.r2, y, zn
        self.oldb, self.beta = self.beta, betan
        self.epsln, self.dbar = self.sn * betan, -self.cs * betan
        self.cs, self.sn = gbar / gamma, betan / gamma
        phi = self.cs * self.phibar
        self.phibar = self.sn * self.phibar
        w1, self.w2 = self.w2, self.w
        self.w = ((v - dt.type(oldeps) * w1 - dt.type(delta) * self.w2) * dt.type(1.0 / gamma)).astype(dt)
        self.x = (self.x + dt.type(phi) * self.w).astype(dt)
        self.rr = self.phibar * self.phibar
        self.alfa = alfa

    def iterate(self, count=1):
        for _ in range(count):
            self._one()
            self.iterations += 1
            self.history.append(self.rr)

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
GRID = 47


def _saddle(c):
    """[[H, B^T], [B, -c I]]: H the 5-point Laplacian of a GRID x GRID grid (4 / -1), B with n // 4 rows, row j = +1 at column 4 j, -1 at column 4 j + 2; c = 0 stores no (2,2)
    block at all."""
    m, n, rp, ci = G.laplacian5pt(GRID)
    rows = np.repeat(np.arange(n), np.diff(rp))
    H = sp.csr_matrix((np.where(ci == rows, 4.0, -1.0), ci, rp), shape=(n, n))
    k = n // 4
    j = np.arange(k)
    B = sp.csr_matrix((np.concatenate([np.ones(k), -np.ones(k)]), (np.concatenate([j, j]), np.concatenate([4 * j, 4 * j + 2]))), shape=(k, n))
    C = None if c == 0 else sp.identity(k, format="csr") * (-float(c))
    K = sp.bmat([[H, B.T], [B, C]], format="csr")
    K.sort_indices()
    return K


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name == "saddle47":
        K = _saddle(0)
    elif name in ("saddlec47", "saddlec47_scaled"):
        K = _saddle(1)
        if name == "saddlec47_scaled":   # S K S with s = 10^U(-1.5, 1.5) (the lap128_scaled construction of cg_mirror): |diag| spans six decades
            s = 10.0 ** np.random.default_rng(5).uniform(-1.5, 1.5, K.shape[0])
            rows = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
            K = sp.csr_matrix((s[rows] * K.data * s[K.indices], K.indices, K.indptr), shape=K.shape)
    elif name == "singular":             # 2 on the diagonal of rows 0 .. 2048; rows 2049 .. are empty
        n = 4098
        K = sp.csr_matrix((np.full(2049, 2.0), np.arange(2049), np.minimum(np.arange(n + 1), 2049)), shape=(n, n))
    elif name == "pow2I":
        n = 4096
        K = sp.csr_matrix((np.full(n, 2.0), np.arange(n), np.arange(n + 1)), shape=(n, n))
    else:
        raise KeyError(name)
    n = K.shape[0]
    return n, np.ascontiguousarray(K.indptr, dtype=np.int32), np.ascontiguousarray(K.indices, dtype=np.int32), np.ascontiguousarray(K.data, dtype=np.float64)


def singular_rhs(n):
    """1 on the rows whose diagonal is 0, 0 elsewhere: A b = 0 exactly."""
    return np.where(np.arange(n) > 2048, 1.0, 0.0)


def zero_block_rhs(n):
    """saddle47: rhs on the rows of the zero block, 0 on the first 2209: b.K b = 0 exactly, which is CG's first p.Ap."""
    b = rhs(n).copy()
    b[: GRID * GRID] = 0.0
    return b


def indefinite_tridiagonal(n):
    """Off-diagonals -1, diagonal 3 (-1)^i: symmetric, Gershgorin puts the spectrum in +-[1, 5].  (n, rp, ci, float64 values)."""
    i = np.arange(n)
    r = np.concatenate([i[1:], i, i[:-1]])
    c = np.concatenate([i[:-1], i, i[1:]])
    v = np.concatenate([np.full(n - 1, -1.0), np.where(i % 2 == 0, 3.0, -3.0), np.full(n - 1, -1.0)])
    A = sp.csr_matrix((v, (r, c)), shape=(n, n))
    A.sort_indices()
    return n, np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float64)


def inverse_abs_diagonal(n, rp, ci, v, dtype):
    """1 / |a_ii| in the value type, 1 where a_ii is 0 or not stored, as tilespmv_csr_abs_diagonal_device(invert = 1) makes it (no input here stores an entry twice)."""
    dt = np.dtype(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n, dtype=dt)
    d[rows[ci == rows]] = np.abs(np.asarray(v, dtype=dt)[ci == rows])
    out = np.ones(n, dtype=dt)
    out[d != 0] = (dt.type(1) / d[d != 0]).astype(dt)
    return out
