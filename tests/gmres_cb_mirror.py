"""The reference for GMRES with a compressed basis (tilespmv_gmres_create_basis(..., TILESPMV_GMRES_BASIS_FLOAT); include/tilespmv.h) — a helper, not a test:
the numpy mirror of tests/gmres_mirror.py (imported, not edited) with three things changed, and nothing else:

    the basis array is float32: a vector stored into it is rounded to nearest, and EVERY read of it — the dots, the subtraction, the close, and the vector that the product and
    the preconditioner (``_hat``) are fed — sees the stored vector widened back to the value type, never the unrounded one;
    ``solve`` accepts the stopping test only on a recomputed rr: when rr <= rtol^2 bb and the cycle position is not 0 it flushes and tests again, and carries on if that fails;
    no second flush at the end when the decision was taken on a flushed state.

With dtype float32 the stored type is the value type, and the mirrors here equal the plain ones bit for bit.

Also the input ``shiftskew67_d4``: the 67 x 67 skew stencil with diagonal 4, which converges fast enough for the floor of one cycle (about eps32 x the residual the cycle began
with) to show before a restart."""
import numpy as np

import gmres_mirror as M
from gmres_mirror import BREAKDOWN, CONVERGED, GRID, MAXITER, RTOL, RUNNING, inverse_diagonal, nilpotent_rhs, rhs, scipy_csr, skew_rhs, spsolve_x   # noqa: F401
from tilespmv_amd import generators as G

BASIS = np.dtype(np.float32)
STENCILS = {"shiftskew67_d4": (4.0, -1.0, 1.0, -1.0, 1.0)}      # diagonal; west, east; south, north


class NarrowBasis:
    """restart + 1 vectors stored as float32 behind the indexing the mirror uses: a store rounds to nearest, a read widens the stored vector(s) back to ``dt``."""

    def __init__(self, count, n, dt):
        self.store, self.dt = np.zeros((count, n), dtype=BASIS), dt

    def __getitem__(self, i):
        return self.store[i].astype(self.dt)

    def __setitem__(self, i, v):
        self.store[i] = v

    def any(self):
        return bool(self.store.any())


class _Compressed:
    """What the two mirrors below share; in front of gmres_mirror.Mirror (or BlockMirror) in the order of the bases."""

    def _open(self):
        if not isinstance(self.V, NarrowBasis):      # (begin has just made a value-type array)
            self.V = NarrowBasis(self.m + 1, self.A.shape[0], self.dt)
        super()._open()

    def solve(self, b, x0=None, rtol=1e-10, maxiter=1000, check_every=8):
        """Returns (x, iterations, status, sqrt(rr / bb)); rr is the recomputed one of the returned x, and CONVERGED was decided on a recomputed rr."""
        if check_every < 1:
            check_every = 1
        self.begin(b, x0)
        while True:
            if self.breakdown:
                status = BREAKDOWN
                break
            if self.bb == 0.0:
                self.x[:] = 0
                self.rr = 0.0
                return self.x, self.iterations, CONVERGED, 0.0
            if self.rr <= rtol * rtol * self.bb:
                if self.pos != 0:
                    self.flush()
                if self.rr <= rtol * rtol * self.bb:
                    status = CONVERGED
                    break
            if self.iterations >= maxiter:
                status = MAXITER
                break
            self.iterate(min(check_every, maxiter - self.iterations))
        if self.pos != 0:
            self.flush()
        return self.x, self.iterations, status, self.rel()


class Mirror(_Compressed, M.Mirror):
    """gmres_mirror.Mirror with the basis stored as float32."""


class BlockMirror(_Compressed, M.BlockMirror):
    """gmres_mirror.BlockMirror with the basis stored as float32."""


def workspace_bytes(rows, restart, value_bytes, basis_bytes, precond=None):
    """The workspace formula of include/tilespmv.h ("WORKSPACE, one hipMalloc of ..."), restated.  ``precond``: None, "dinv" or "block"."""
    def up(b):
        return (b + 255) // 256 * 256
    B, D = up((rows + 16) * basis_bytes), up((rows + 16) * value_bytes)
    v = 2 + ({None: 0, "dinv": 1, "block": 1}[precond] if basis_bytes == value_bytes else {None: 1, "dinv": 1, "block": 2}[precond])
    lane = 16 // value_bytes
    cap = 1024 if rows * value_bytes >= 128 << 20 else 512 if rows * value_bytes >= 32 << 20 else 256
    P = min(cap, max(1, min(1024, -(-(rows // lane) // 512))))
    Q = up(8 * P)
    return (restart + 1) * B + v * D + 2 * (restart + 1) * Q + 2 * Q + 32768 + 4 * 768 + 256


def problem(name):
    """gmres_mirror.problem, and shiftskew67_d4."""
    if name in STENCILS:
        m, n, rp, ci = G.laplacian5pt(GRID)
        v = M.stencil_values(GRID, n, rp, ci, *STENCILS[name])
        return n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    return M.problem(name)
