"""The reference the GPU GMRES solver is compared with (a helper, not a test): a numpy restatement of the recurrences of tilespmv_gmres_* (include/tilespmv.h),
written for clarity and sharing nothing with the code under test.

    Right-preconditioned GMRES(restart), M^-1 = diag(dinv) (dinv = None: M = I).  x, b, the basis V and w live in the build's value type; every dot product is accumulated in
    float64; the Hessenberg column, the Givens rotations, g, y and every scalar are float64; h1_i, h2_i, 1 / h_{j+1,j}, 1 / beta and y_i are rounded to the value type once, where
    they multiply a vector; the products are scipy's CSR products in the value type.
      open     r = b - A x;  rr = r.r;  beta = sqrt(rr);  V_0 = r / beta;  g = beta e_0;  j = 0  (rr = 0: nothing is formed, the cycle is dead)
      inner    w = A (dinv o V_j);  h1 = V^T w;  w -= V h1;  h2 = V^T w;  w -= V h2;  hh = |w|;  column (h1 + h2, hh), the stored rotations, the new one;  g_{j+1} = -sn g_j,
               g_j = cs g_j;  rr = g_{j+1}^2;  V_{j+1} = w / hh;  after `restart` inner iterations of a cycle: close and open
      close    R y = g over the k columns done (column-oriented back substitution);  x += dinv o (sum_i y_i V_i)
    guards (exact tests):
      rr = 0 at an open, or the breakdown flag   inner iterations and closes change nothing
      hh = 0 with gamma != 0                      the lucky termination: rr = 0, V_{j+1} is not formed, the cycle is closed early; the close uses the columns done
      gamma = 0                                   breakdown: nothing changes in this or any later iteration or close
      the iteration counter advances whatever the guards did.
    x is current only after a close; rr after an open is the recomputed |b - A x|^2.  solve ends with a flush: the rr it returns is that of the returned x.

``order``: None, or a permutation of the rows in which every dot product is accumulated (another summation order: tests/test_gmres_cpu.py uses it to bound what the order of the
GPU's sums may cost in iterations).

Also the inputs of tests/test_gmres_cpu.py and tests/test_gpu_gmres.py, so that both files solve the same systems.
"""
import numpy as np
import scipy.sparse as sp

import bicgstab_mirror as B
from bicgstab_mirror import BREAKDOWN, CONVERGED, GRID, MAXITER, RTOL, RUNNING, inverse_diagonal, rhs, scipy_csr, skew_rhs, spsolve_x   # noqa: F401
from tilespmv_amd import generators as G

MAX_RESTART = 64


class Mirror:
    """begin / iterate / flush / solve with the meaning of the C entry points.  ``A``: scipy CSR (any value type; converted), ``dinv``: None or the inverse diagonal."""

    def __init__(self, A, dtype, restart=30, dinv=None, order=None):
        assert 1 <= restart <= MAX_RESTART
        self.dt = np.dtype(dtype)
        self.A = sp.csr_matrix(A, dtype=self.dt)
        self.m = int(restart)
        self.dinv = None if dinv is None else np.asarray(dinv, dtype=self.dt)
        self.order = order

    def _dots(self, V, w):
        """V^T w for the rows of V, in float64."""
        V, w = V.astype(np.float64), w.astype(np.float64)
        if self.order is not None:
            V, w = V[:, self.order], w[self.order]
        return V @ w

    def _hat(self, v):
        return v if self.dinv is None else (self.dinv * v).astype(self.dt)

    def _open(self):
        dt = self.dt
        r = (self.b - self.A @ self.x).astype(dt)
        self.rr = float(self._dots(r[None, :], r)[0])
        self.j = 0
        self.live = self.rr != 0.0 and not self.breakdown
        if self.live:
            beta = self.rr ** 0.5
            self.V[0] = (dt.type(1.0 / beta) * r).astype(dt)
            self.g[0] = beta
        self.pos = 0

    def _close(self):
        dt = self.dt
        k = 0 if self.breakdown else self.j
        if k == 0:
            return
        g = self.g[:k].copy()
        for i in range(k - 1, -1, -1):
            g[i] = g[i] / self.R[i, i]
            g[:i] -= self.R[:i, i] * g[i]
        u = np.zeros(self.A.shape[0], dtype=dt)
        for i in range(k):
            u = (u + dt.type(g[i]) * self.V[i]).astype(dt)
        self.x = (self.x + self._hat(u)).astype(dt)

    def begin(self, b, x0=None):
        dt, n = self.dt, self.A.shape[0]
        self.b = np.array(b, dtype=dt)
        self.x = np.zeros(n, dtype=dt) if x0 is None else np.array(x0, dtype=dt)
        self.bb = float(self._dots(self.b[None, :], self.b)[0])
        self.iterations, self.breakdown = 0, False
        self.V = np.zeros((self.m + 1, n), dtype=dt)
        self.R = np.zeros((self.m, self.m))
        self.cs, self.sn, self.g = np.zeros(self.m), np.zeros(self.m), np.zeros(self.m + 1)
        self._open()

    def _orthogonalise(self, w, k):
        h = self._dots(self.V[:k], w)
        for i in range(k):
            w = (w - self.dt.type(h[i]) * self.V[i]).astype(self.dt)
        return w, h

    def _inner(self):
        dt, j = self.dt, self.j
        if not self.live or self.breakdown or j >= self.m:
            return
        w = (self.A @ self._hat(self.V[j])).astype(dt)
        w, h1 = self._orthogonalise(w, j + 1)
        w, h2 = self._orthogonalise(w, j + 1)
        hh = float(self._dots(w[None, :], w)[0]) ** 0.5
        col = h1 + h2
        for i in range(j):
            col[i], col[i + 1] = self.cs[i] * col[i] + self.sn[i] * col[i + 1], -self.sn[i] * col[i] + self.cs[i] * col[i + 1]
        gamma = float(np.hypot(col[j], hh))
        if gamma == 0.0:
            self.breakdown, self.live = True, False
            return
        self.cs[j], self.sn[j] = col[j] / gamma, hh / gamma
        self.R[:j, j], self.R[j, j] = col[:j], gamma
        self.g[j + 1], self.g[j] = -self.sn[j] * self.g[j], self.cs[j] * self.g[j]
        self.rr = self.g[j + 1] ** 2
        self.j = j + 1
        if hh == 0.0:
            self.live = False      # closed early
        else:
            self.V[j + 1] = (dt.type(1.0 / hh) * w).astype(dt)

    def iterate(self, count=1):
        for _ in range(count):
            self._inner()
            self.iterations += 1
            self.pos += 1
            if self.pos == self.m:
                self._close()
                self._open()

    def flush(self):
        self._close()
        self._open()

    def status(self):
        return BREAKDOWN if self.breakdown else CONVERGED if self.rr == 0.0 else RUNNING

    def solve(self, b, x0=None, rtol=1e-10, maxiter=1000, check_every=8):
        """Returns (x, iterations, status, sqrt(rr / bb)); rr is the recomputed one of the returned x."""
        if check_every < 1:
            check_every = 1
        self.begin(b, x0)
        while True:
            if self.breakdown:
                status = BREAKDOWN
            elif self.bb == 0.0:
                self.x[:] = 0
                self.rr = 0.0
                return self.x, self.iterations, CONVERGED, 0.0
            elif self.rr <= rtol * rtol * self.bb:
                status = CONVERGED
            elif self.iterations >= maxiter:
                status = MAXITER
            else:
                self.iterate(min(check_every, maxiter - self.iterations))
                continue
            self.flush()
            return self.x, self.iterations, status, self.rel()

    def rel(self):
        return (self.rr / self.bb) ** 0.5 if self.bb > 0 else 0.0


# ---- inputs
STENCILS = {"convdom67": (4.0, -9.0, 7.0, -6.0, 4.0), "shiftskew67": (0.25, -1.0, 1.0, -1.0, 1.0)}      # diagonal; west, east; south, north


def stencil_values(k, n, rp, ci, diag, west, east, south, north):
    """Values on the pattern of the 5-point Laplacian of a k x k grid, as bicgstab_mirror.convdiff_values lays them out."""
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = ci.astype(np.int64) - rows
    v = np.zeros(len(ci))
    for off, val in ((0, diag), (-1, west), (1, east), (-k, south), (k, north)):
        v[d == off] = val
    assert np.all(v != 0)
    return v


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32: those of bicgstab_mirror, and
      convdom67, shiftskew67     convection-dominated and shifted skew-symmetric stencils on the pattern of the 67 x 67 grid (STENCILS)
      convdiff67_colscaled       convdiff67's values times s[column], s = 10^U(-1.5, 1.5): right Jacobi restores A / 4
      nilpotent                  4098 rows, row 2k holds a single 1 at column 2k + 1, odd rows are empty: with nilpotent_rhs, A V_0 = 0 exactly."""
    if name in STENCILS:
        m, n, rp, ci = G.laplacian5pt(GRID)
        v = stencil_values(GRID, n, rp, ci, *STENCILS[name])
    elif name == "convdiff67_colscaled":
        n, rp, ci, v = B.problem("convdiff67")
        s = 10.0 ** np.random.default_rng(5).uniform(-1.5, 1.5, n)
        v = v * s[ci]
    elif name == "nilpotent":
        n = 4098
        rp = np.repeat(np.arange(n // 2 + 1), 2)[1:]      # 0, 1, 1, 2, 2, ...
        ci = np.arange(1, n, 2)
        v = np.ones(n // 2)
    else:
        return B.problem(name)
    return n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


def nilpotent_rhs(n):
    """skew_rhs with the odd entries set to 0."""
    b = skew_rhs(n)
    b[1::2] = 0
    return b


class BlockMirror(Mirror):
    """Mirror with M^-1 the block-Jacobi planes ``P`` of tests/block_jacobi_mirror.py (``update``), applied as the library applies them."""

    def __init__(self, A, dtype, restart, P, order=None):
        super().__init__(A, dtype, restart, order=order)
        self.P = np.asarray(P, dtype=self.dt)

    def _hat(self, v):
        import block_jacobi_mirror as BJ
        return BJ.apply(self.P, v)
