"""The reference the block-Jacobi preconditioner is compared with (a helper, not a test): numpy restatements of tilespmv_block_jacobi_update and _apply (include/tilespmv.h,
DESIGN.md §3.12) and of the CG and BiCGStab recurrences with that preconditioner, written for clarity and sharing nothing with the code under test.

    update   block k = rows and columns [k bs, min((k + 1) bs, rows)) of the CSR, duplicates added, in float64; its inverse by numpy.linalg.inv in float64; the IDENTITY for a
             singular block (inv raises, or returns something that is not finite).
    apply    z_i = sum_j (M^-1)[i][blockstart(i) + j] r[blockstart(i) + j]: M^-1 rounded to the value type, the products and the sum in float64, z rounded to the value type once.
    CG       tests/cg_mirror.py's recurrences with z = apply(r) in place of dinv o r (the mirror there forms z once per iteration and uses it for rho and for p: a stored z).
    BiCGStab tests/bicgstab_mirror.py's with phat = apply(p), shat = apply(s).

Also the inputs of tests/test_block_jacobi_cpu.py and tests/test_gpu_block_jacobi.py, so that both files work on the same systems.
"""
import numpy as np
import scipy.sparse as sp

import bicgstab_mirror as BM
import cg_mirror as CM
import solver_sizes as SS
from cg_mirror import rhs, scipy_csr, spsolve_x   # noqa: F401
from tilespmv_amd import generators as G

RUNNING, CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2, 3
RTOL = CM.RTOL


# ---- update
def blocks(n, rp, ci, v, bs):
    """The diagonal blocks as float64 [ceil(n / bs), bs, bs]; a short last block is padded by the identity (its inverse is then padded by the identity too)."""
    nb = (n + bs - 1) // bs
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci, dtype=np.int64)
    inside = rows // bs == cols // bs
    B = np.zeros((nb, bs, bs))
    np.add.at(B, (rows[inside] // bs, rows[inside] % bs, cols[inside] % bs), np.asarray(v, dtype=np.float64)[inside])
    for l in range(n - (nb - 1) * bs, bs):
        B[nb - 1, l, l] = 1.0
    return B


def invert(B):
    """(float64 inverses [nb, bs, bs], mask of the singular blocks: theirs is the identity)."""
    singular = np.zeros(len(B), dtype=bool)
    try:                                   # (all at once where every block is regular: the large inputs)
        inv = np.linalg.inv(B)
        if np.isfinite(inv).all():
            return inv, singular
    except np.linalg.LinAlgError:
        pass
    inv = np.empty_like(B)
    for k, b in enumerate(B):
        try:
            inv[k] = np.linalg.inv(b)
            singular[k] = not np.isfinite(inv[k]).all()
        except np.linalg.LinAlgError:
            singular[k] = True
        if singular[k]:
            inv[k] = np.eye(B.shape[1])
    return inv, singular


def planes(inv, n):
    """The library's layout: [bs, n], planes[j, i] = (M^-1)[i][blockstart(i) + j]; 0 where the last block is short."""
    nb, bs, _ = inv.shape
    P = inv.transpose(2, 0, 1).reshape(bs, nb * bs)[:, :n].copy()
    short = n - (nb - 1) * bs
    P[short:, (nb - 1) * bs:] = 0.0
    return P


def update(n, rp, ci, v, bs, dtype):
    """(planes in the value type, number of singular blocks)."""
    inv, singular = invert(blocks(n, rp, ci, v, bs))
    return planes(inv, n).astype(np.dtype(dtype)), int(singular.sum())


# ---- apply
def apply(P, r):
    """z = M^-1 r for planes P [bs, n] (the value type) and r (the value type)."""
    bs, n = P.shape
    dt = P.dtype
    start = np.arange(n) // bs * bs
    r64 = np.concatenate([np.asarray(r, dtype=np.float64), np.zeros(bs)])
    z = np.zeros(n)
    for j in range(bs):
        z += P[j].astype(np.float64) * r64[start + j]
    return z.astype(dt)


class CG(CM.Mirror):
    """tests/cg_mirror.py's Mirror with z = M^-1 r; ``P``: the planes of ``update``."""

    def __init__(self, A, dtype, P):
        super().__init__(A, dtype)
        self.P = np.asarray(P, dtype=self.dt)

    def _z(self, r):
        return apply(self.P, r)


class BiCGStab(BM.Mirror):
    """tests/bicgstab_mirror.py's Mirror with phat = M^-1 p, shat = M^-1 s."""

    def __init__(self, A, dtype, P, order=None):
        super().__init__(A, dtype, order=order)
        self.P = np.asarray(P, dtype=self.dt)

    def _hat(self, p):
        return apply(self.P, p)


# ---- inputs
FEM = (10, 10, 10, 3)
COUPLING = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.9, 0.9, 1.0]])


def _node_transform(rng, nodes):
    """blockdiag(Q_a diag(10^U(-1.5, 1.5))), Q_a the Q factor of a 3 x 3 standard normal matrix; nodes in order, the normal draw before the uniform one."""
    out = []
    for _ in range(nodes):
        q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        out.append(q @ np.diag(10.0 ** rng.uniform(-1.5, 1.5, 3)))
    return sp.block_diag(out, format="csr")


def femblk(nonsymmetric, mesh=FEM):
    """(n, rp, ci, values) on the pattern of generators.fem_hex(*mesh), 3 unknowns per node: A = T^T (G x C) T, G the node graph's Laplacian with degree + 1 on the diagonal and -1
    off it, C = COUPLING, T = blockdiag(Q_a diag(10^U(-1.5, 1.5))) drawn with seed 21 — symmetric positive definite, its 3 x 3 node blocks full and badly scaled in rotated
    coordinates, which a point diagonal cannot undo.  nonsymmetric: -1.4 above / -0.6 below the diagonal of G, and independent left and right transforms (seed 22, the left one
    drawn first): A = L^T (G x C) R."""
    m, n, rp, ci = G.fem_hex(*mesh)
    dof = mesh[3]
    assert dof == 3
    nodes = n // dof
    pattern = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    node_graph = sp.csr_matrix(pattern[::dof, ::dof])       # (a full dof x dof block per pair of coupled nodes: any one entry of it shows the pair)
    node_graph.setdiag(0)
    node_graph.eliminate_zeros()
    adj = sp.coo_matrix(node_graph)
    deg = np.bincount(adj.row, minlength=nodes)
    if nonsymmetric:
        w = np.where(adj.col > adj.row, -1.4, -0.6)
    else:
        w = np.full(len(adj.row), -1.0)
    Gm = sp.coo_matrix((w, (adj.row, adj.col)), shape=(nodes, nodes)).tocsr() + sp.diags(deg + 1.0)
    K = sp.kron(Gm, COUPLING, format="csr")
    if nonsymmetric:
        rng = np.random.default_rng(22)
        L = _node_transform(rng, nodes)
        R = _node_transform(rng, nodes)
        A = (L.T @ K @ R).tocsr()
    else:
        T = _node_transform(np.random.default_rng(21), nodes)
        A = (T.T @ K @ T).tocsr()
    A.sort_indices()
    assert A.nnz == len(ci) and np.array_equal(A.indptr, rp) and np.array_equal(A.indices, ci) and (A.data != 0).all(), "the pattern is the generator's"
    return n, rp, ci, A.data


def pivot2():
    """64 rows, bs = 2: every diagonal block is [[0, 2], [3, 0]] (a zero pivot without the row exchange) except block 5, [[1, 2], [2, 4]] (singular); -0.5 couples every row to
    the row two further on (cyclically), outside its block."""
    n = 64
    D = np.zeros((n, n))
    for k in range(n // 2):
        D[2 * k:2 * k + 2, 2 * k:2 * k + 2] = [[1.0, 2.0], [2.0, 4.0]] if k == 5 else [[0.0, 2.0], [3.0, 0.0]]
    for i in range(n):
        D[i, (i + 2) % n] = -0.5
    A = sp.csr_matrix(D)
    A.sort_indices()
    return n, A.indptr, A.indices, A.data


_PROBLEMS = {}


def problem(name):
    """(n, rp, ci, float64 values) of the named input, rp / ci as int32."""
    if name not in _PROBLEMS:
        if name == "femblk10":
            n, rp, ci, v = femblk(False)
        elif name == "femblk10_ns":
            n, rp, ci, v = femblk(True)
        elif name == "lap55":
            m, n, rp, ci = G.laplacian5pt(55)
            v = CM.laplacian_values(n, rp, ci)
        elif name == "pivot2":
            n, rp, ci, v = pivot2()
        else:
            raise KeyError(name)
        _PROBLEMS[name] = (n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64))
    return _PROBLEMS[name]


def tri_capped(dtype):
    """The tridiagonal (-1, 2, -1) of solver_sizes.capped_n(dtype) rows: 1024 partial sums, a second sweep over the workgroups, the longest scalar tail."""
    return SS.tridiagonal(SS.capped_n(dtype), -1.0, 2.0, -1.0)


def inverse_diagonal(n, rp, ci, v, dtype):
    return BM.inverse_diagonal(n, rp, ci, v, dtype)
