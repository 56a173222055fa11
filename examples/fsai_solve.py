"""A symmetric positive definite system by CG with the FSAI preconditioner on one GPU (api.FSAI + SparseOperator.cg(precond=...) over tilespmv_fsai_* and
tilespmv_cg_create_fsai) — against point Jacobi on the same operator.

    python examples/fsai_solve.py --problem aniso --grid 256 [--eps 0.01] [--dtype f32]
    python examples/fsai_solve.py --problem jump --grid 48
    python examples/fsai_solve.py --problem laplacian --grid 512

Three systems without node blocks, where the inverse diagonal does little or nothing:
    laplacian  the 5-point Laplacian of a grid x grid mesh: a constant diagonal, point Jacobi is plain CG.
    aniso      -eps u_xx - u_yy on a grid x grid mesh (a stretched grid): 2 + 2 eps on the diagonal, -eps / -1 beside it.
    jump       the 7-point operator of a grid^3 mesh with a coefficient 10^U(-2, 2) per cell face (a diffusion problem with jumping coefficients).
FSAI builds a sparse lower-triangular G on the pattern of A's lower triangle with G A G^T ~ I and applies z = G^T (G r) by two products.  Prints one JSON line for the object and
one per solve: iterations, residuals, seconds.  After new values on the same pattern (a Newton step, a new coefficient field): op.update_values(d_vals) and
f.update(d_rp, d_ci, d_vals) again, into the same objects.
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


def second_difference(n, w):
    """The 1-D operator with weight w[k] between nodes k and k + 1 (Dirichlet ends: one more unit weight at either end)."""
    d = np.concatenate([[1.0], w]) + np.concatenate([w, [1.0]])
    return sp.diags([-w, d, -w], [-1, 0, 1], format="csr")


def system(problem, grid, eps):
    one, eye = np.ones(grid - 1), sp.identity(grid, format="csr")
    if problem in ("laplacian", "aniso"):
        T = second_difference(grid, one)
        A = sp.kron(eye, (1.0 if problem == "laplacian" else eps) * T) + sp.kron(T, eye)
    else:                                                    # weights per face, direction by direction
        rng = np.random.default_rng(7)
        n = grid ** 3
        idx = np.arange(n).reshape(grid, grid, grid)
        A = sp.csr_matrix((n, n))
        for axis in range(3):
            lo, hi = np.take(idx, range(grid - 1), axis=axis).ravel(), np.take(idx, range(1, grid), axis=axis).ravel()
            w = 10.0 ** rng.uniform(-2, 2, len(lo))
            A = A + sp.coo_matrix((np.concatenate([-w, -w, w, w]), (np.concatenate([lo, hi, lo, hi]), np.concatenate([hi, lo, lo, hi]))), shape=(n, n)).tocsr()
        A = A + 1e-2 * sp.identity(n, format="csr")          # (definite without boundary conditions)
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="aniso", choices=["laplacian", "aniso", "jump"])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=50000)
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("fsai_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    A = system(a.problem, a.grid, a.eps)
    n = A.shape[0]
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    # the CSR on the device: the operator is built from it, and both preconditioners are taken from it by kernels
    rpd, cid = torch.from_numpy(np.ascontiguousarray(A.indptr, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(A.indices, dtype=np.int32)).cuda()
    vd = torch.from_numpy(A.data.astype(dtype)).cuda()
    op = SparseOperator(n, n, rpd, cid, vd)
    dinv = torch.empty(n, dtype=b.dtype, device="cuda")
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=st, dtype=dtype)
    f = api.FSAI(n, A.nnz, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dtype, stream=st)
    print(json.dumps({"preconditioner": f.info(st)}))
    runs = (("point Jacobi", lambda: op.cg(b, rtol=rtol, maxiter=a.maxiter, dinv=dinv)), ("FSAI", lambda: op.cg(b, rtol=rtol, maxiter=a.maxiter, precond=f)))
    for label, run in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info.update({"solver": "cg, " + label, "problem": a.problem, "n": n, "dtype": a.dtype, "seconds": round(dt, 4),
                     "ms_per_iteration": round(dt * 1e3 / max(info["iterations"], 1), 4),
                     "true_relative_residual": float(torch.linalg.vector_norm(b - op.matvec(x)) / torch.linalg.vector_norm(b))})
        print(json.dumps(info))
    f.close()
    op.close()


if __name__ == "__main__":
    main()
