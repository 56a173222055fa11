"""Least squares  min ||A x - b||  with CGLS on one GPU: the plans of A and of A^T from one CSR (SparseOperator; A^T built on the device from A's CSR).

    python examples/least_squares.py --rows 2000000 --cols 500000 --per-row 8 [--solver library|torch] [--damp 0.1]

--solver library (the default): SparseOperator.cgls, the solver in the library (tilespmv_cgls_*: two products and four fused kernels per iteration, every scalar on the device);
--solver torch: the module-level cgls, the same recurrences as a loop of torch operations (no damping).

A is a tall random sparse matrix with a scaled identity stacked into its first rows (well conditioned); b = A x_true + noise.  Prints one JSON line: iterations, residuals, the
error against x_true, and the time per iteration (one A p and one A^T r).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400000)
    ap.add_argument("--cols", type=int, default=100000)
    ap.add_argument("--per-row", type=int, default=8)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--solver", default="library", choices=["library", "torch"])
    ap.add_argument("--damp", type=float, default=0.0, help="Tikhonov damping (library solver only)")
    a = ap.parse_args()
    import torch
    from tilespmv_amd import generators as G
    from tilespmv_amd.operator import SparseOperator, cgls
    if not torch.cuda.is_available():
        raise SystemExit("least_squares.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.float64 if a.dtype == "f64" else np.float32
    rng = np.random.default_rng(1)
    r = np.concatenate([np.repeat(np.arange(a.rows), a.per_row), np.arange(a.cols)])
    c = np.concatenate([rng.integers(0, a.cols, a.rows * a.per_row), np.arange(a.cols)])
    rows, cols, rp, ci = G.from_coo(a.rows, a.cols, r, c)
    nnz = int(rp[rows])
    v = (rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(dtype)
    x_true = rng.standard_normal(cols).astype(dtype)
    op = SparseOperator(rows, cols, rp, ci, v)
    xt = torch.from_numpy(x_true).cuda()
    b = op.matvec(xt).clone()
    b += 1e-3 * torch.randn(rows, dtype=b.dtype, device=b.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.solver == "library":
        x, info = op.cgls(b, rtol=a.tol, maxiter=a.maxiter, check_every=4, damp=a.damp)
    else:
        if a.damp != 0.0:
            raise SystemExit("--damp needs --solver library")
        x, info = cgls(op, b, tol=a.tol, maxiter=a.maxiter, check_every=4)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    info.update({"solver": a.solver, "rows": rows, "cols": cols, "nnz": nnz, "dtype": a.dtype, "seconds": round(dt, 4),
                 "ms_per_iteration": round(dt * 1e3 / max(info["iterations"], 1), 4),
                 "relative_error_vs_x_true": float(torch.linalg.vector_norm(x - xt) / torch.linalg.vector_norm(xt))})
    op.close()
    print(json.dumps(info))


if __name__ == "__main__":
    main()
