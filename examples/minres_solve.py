"""A saddle-point system K [u; p] = b by MINRES in the library, on one GPU (SparseOperator.minres over tilespmv_minres_*: one product and three fused kernels per iteration, every
scalar on the device) — and what CG makes of the same system.

    python examples/minres_solve.py --grid 256 [--dtype f32] [--c 0.0] [--scale 1.5] [--compare]

K = [[H, B^T], [B, -c I]]: H is the 5-point Laplacian of a grid x grid mesh (4 / -1), B has grid^2 // 4 rows with +1 at column 4 j and -1 at column 4 j + 2 (differences of the
unknowns as constraints), c >= 0 regularises the constraint block.  K is symmetric and INDEFINITE: one negative eigenvalue per constraint.  The right-hand side is supported on the
constraint rows, so b.K b = 0 exactly when c = 0 and CG breaks down in its first iteration (p.Ap = 0); MINRES solves the system.  --scale S > 0 solves S K S instead,
s = 10^U(-S, S): a diagonal spread over 2 S decades, with negative (or, at c = 0, zero) entries in the constraint block, which MINRES preconditioned by 1 / |diag|
(tilespmv_csr_abs_diagonal_device) gets through and plain MINRES does not.  Prints one JSON line per solve: iterations, residuals, seconds.  --compare also times this solver
against the loop of torch operations tilespmv_amd.operator.minres on a shifted Laplacian of the same grid (what scripts/minres_time.py records at full size).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def saddle(k, c):
    from tilespmv_amd import generators as G
    m, n, rp, ci = G.laplacian5pt(k)
    H = sp.csr_matrix((np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 4.0, -1.0), ci, rp), shape=(n, n))
    nc = n // 4
    j = np.arange(nc)
    B = sp.csr_matrix((np.concatenate([np.ones(nc), -np.ones(nc)]), (np.concatenate([j, j]), np.concatenate([4 * j, 4 * j + 2]))), shape=(nc, n))
    K = sp.bmat([[H, B.T], [B, None if c == 0 else -c * sp.identity(nc, format="csr")]], format="csr")
    K.sort_indices()
    return K, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--c", type=float, default=0.0)
    ap.add_argument("--scale", type=float, default=0.0)
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("minres_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    K, nh = saddle(a.grid, a.c)
    n = K.shape[0]
    if a.scale > 0:
        s = 10.0 ** np.random.default_rng(5).uniform(-a.scale, a.scale, n)
        K = sp.csr_matrix((s[np.repeat(np.arange(n), np.diff(K.indptr))] * K.data * s[K.indices], K.indices, K.indptr), shape=K.shape)
    bh = np.random.default_rng(3).uniform(-1, 1, n)
    bh[:nh] = 0.0
    b = torch.from_numpy(bh.astype(dtype)).cuda()
    # the CSR on the device: the operator is built from it, and 1 / |diagonal| is taken from it by a kernel
    rpd, cid = torch.from_numpy(np.ascontiguousarray(K.indptr, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(K.indices, dtype=np.int32)).cuda()
    vd = torch.from_numpy(K.data.astype(dtype)).cuda()
    op = SparseOperator(n, n, rpd, cid, vd)
    minv = torch.empty(n, dtype=b.dtype, device="cuda")
    api.csr_abs_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), minv.data_ptr(), invert=True, stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    runs = (("cg", lambda: op.cg(b, rtol=rtol, maxiter=a.maxiter)), ("minres", lambda: op.minres(b, rtol=rtol, maxiter=a.maxiter)),
            ("minres, minv = 1 / |diag|", lambda: op.minres(b, rtol=rtol, maxiter=a.maxiter, minv=minv)))
    for label, run in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info.update({"solver": label, "n": n, "constraints": n - nh, "dtype": a.dtype, "seconds": round(dt, 4), "ms_per_iteration": round(dt * 1e3 / max(info["iterations"], 1), 4),
                     "true_relative_residual": float(torch.linalg.vector_norm(b - op.matvec(x)) / torch.linalg.vector_norm(b))})
        print(json.dumps(info))
    op.close()
    if a.compare:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "minres_time.py"), "--workloads", "lap%d:%s" % (a.grid, a.dtype), "--rounds", "2"])


if __name__ == "__main__":
    main()
