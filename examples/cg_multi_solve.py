"""A X = B for several right-hand sides at once by conjugate gradients in the library (SparseOperator.cg with a 2-D b over tilespmv_cg_multi_*: the multi-vector product and
three fused kernels per iteration for all columns, one set of device scalars per column).

    python examples/cg_multi_solve.py --grid 512 --k 8 [--dtype f32] [--compare]

A is the 5-point Laplacian of a grid x grid mesh; the k right-hand sides are load cases of different smoothness and scale (a random field, A 1, a point load, a zero column,
scaled random fields), so the columns stop at different iterations: a column that has reached the tolerance is frozen on the device while the others run on.  Prints one JSON
line per column, then the seconds of the batched solve and of k single solves.  --compare also runs scripts/cg_multi_time.py on the same grid.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=5000)
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    import torch
    from tilespmv_amd import generators as G
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("cg_multi_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    m, n, rp, ci = G.laplacian5pt(a.grid)
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = np.where(ci == rows, 4.0, -1.0)
    rng = np.random.default_rng(3)
    point = np.zeros(n)
    point[n // 2] = 1.0
    cases = [rng.uniform(-1, 1, n), np.bincount(rows, weights=v, minlength=n), point, np.zeros(n)]      # (A 1 = the row sums)
    B = np.stack([cases[j] if j < len(cases) else 10.0 ** (j - 6) * rng.uniform(-1, 1, n) for j in range(a.k)], axis=1)
    Bd = torch.from_numpy(np.ascontiguousarray(B.astype(dtype))).cuda()
    with SparseOperator(n, n, rp, ci, v.astype(dtype)) as op:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, infos = op.cg(Bd, rtol=rtol, maxiter=a.maxiter)
        torch.cuda.synchronize()
        t_multi = time.perf_counter() - t0
        R = Bd - op.spmm(X.contiguous()) if a.k in (1, 2, 4, 8) else None
        for j, info in enumerate(infos):
            info.update({"column": j, "n": n, "dtype": a.dtype})
            if R is not None and float(torch.linalg.vector_norm(Bd[:, j])) > 0:
                info["true_relative_residual"] = float(torch.linalg.vector_norm(R[:, j]) / torch.linalg.vector_norm(Bd[:, j]))
            print(json.dumps(info))
        t0 = time.perf_counter()
        for j in range(a.k):
            op.cg(Bd[:, j].contiguous(), rtol=rtol, maxiter=a.maxiter)
        torch.cuda.synchronize()
        t_single = time.perf_counter() - t0
        print(json.dumps({"k": a.k, "groups": SparseOperator.cg_groups(a.k), "seconds_batched": round(t_multi, 4), "seconds_one_by_one": round(t_single, 4)}))
    if a.compare:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "cg_multi_time.py"), "--workloads", "lap%d:%s" % (a.grid, a.dtype), "--rounds", "2"])


if __name__ == "__main__":
    main()
