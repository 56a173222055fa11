"""A structural-FEM-like system by CG with a block-Jacobi preconditioner, one 3 x 3 block per node, on one GPU (api.BlockJacobi + SparseOperator.cg(precond=...) over
tilespmv_block_jacobi_* and tilespmv_cg_create_block) — against point Jacobi on the same operator.

    python examples/block_jacobi_solve.py --mesh 24 [--dtype f32] [--nonsymmetric] [--block-size 3]

The pattern is generators.fem_hex(mesh, mesh, mesh, 3): 3 unknowns per node, every node coupled to its 27 neighbours by a full 3 x 3 block.  The values are
A = T^T (G x C) T: G the node graph's Laplacian (degree + 1 on the diagonal, -1 off it), C = [[1, .9, .9], [.9, 1, .9], [.9, .9, 1]] couples a node's unknowns, and
T = blockdiag(Q_a diag(10^U(-1.5, 1.5))) gives every node its own rotated, badly scaled coordinates — what shells, beams and mixed units do to a stiffness matrix.  A point
diagonal can rescale an unknown; it cannot rotate a node's block back, the block inverse can.  --nonsymmetric: weights -1.4 / -0.6 above / below the diagonal of G and independent
left and right transforms, solved by BiCGStab.  Prints one JSON line per solve: iterations, residuals, seconds.  After new values on the same pattern (a Newton step):
op.update_values(d_vals) and bj.update(d_rp, d_ci, d_vals) again, into the same objects.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def node_transform(rng, nodes):
    return sp.block_diag([np.linalg.qr(rng.standard_normal((3, 3)))[0] @ np.diag(10.0 ** rng.uniform(-1.5, 1.5, 3)) for _ in range(nodes)], format="csr")


def system(mesh, nonsymmetric):
    from tilespmv_amd import generators as G
    m, n, rp, ci = G.fem_hex(mesh, mesh, mesh, 3)
    nodes = n // 3
    adj = sp.coo_matrix(sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))[::3, ::3])
    off = adj.row != adj.col
    r, c = adj.row[off], adj.col[off]
    w = np.where(c > r, -1.4, -0.6) if nonsymmetric else np.full(len(r), -1.0)
    Gm = sp.coo_matrix((w, (r, c)), shape=(nodes, nodes)).tocsr() + sp.diags(np.bincount(r, minlength=nodes) + 1.0)
    K = sp.kron(Gm, np.array([[1.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.9, 0.9, 1.0]]), format="csr")
    rng = np.random.default_rng(22 if nonsymmetric else 21)
    L = node_transform(rng, nodes)
    R = node_transform(rng, nodes) if nonsymmetric else L
    A = (L.T @ K @ R).tocsr()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=24)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--nonsymmetric", action="store_true")
    ap.add_argument("--block-size", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=20000)
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("block_jacobi_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    A = system(a.mesh, a.nonsymmetric)
    n = A.shape[0]
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    # the CSR on the device: the operator is built from it, and both preconditioners are taken from it by kernels
    rpd, cid = torch.from_numpy(np.ascontiguousarray(A.indptr, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(A.indices, dtype=np.int32)).cuda()
    vd = torch.from_numpy(A.data.astype(dtype)).cuda()
    op = SparseOperator(n, n, rpd, cid, vd)
    dinv = torch.empty(n, dtype=b.dtype, device="cuda")
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=st, dtype=dtype)
    bj = api.BlockJacobi(n, a.block_size, dtype)
    bj.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st)
    print(json.dumps({"preconditioner": bj.info(st)}))
    solve = op.bicgstab if a.nonsymmetric else op.cg
    runs = (("point Jacobi", lambda: solve(b, rtol=rtol, maxiter=a.maxiter, dinv=dinv)), ("block Jacobi, bs = %d" % a.block_size, lambda: solve(b, rtol=rtol, maxiter=a.maxiter, precond=bj)))
    for label, run in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info.update({"solver": ("bicgstab, " if a.nonsymmetric else "cg, ") + label, "n": n, "dtype": a.dtype, "seconds": round(dt, 4),
                     "ms_per_iteration": round(dt * 1e3 / max(info["iterations"], 1), 4),
                     "true_relative_residual": float(torch.linalg.vector_norm(b - op.matvec(x)) / torch.linalg.vector_norm(b))})
        print(json.dumps(info))
    bj.close()
    op.close()


if __name__ == "__main__":
    main()
