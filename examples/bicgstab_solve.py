"""A x = b for a nonsymmetric A by BiCGStab in the library, plain and Jacobi-preconditioned, on one GPU (SparseOperator.bicgstab over tilespmv_bicgstab_*: the two products and five
fused kernels per iteration, every scalar on the device).

    python examples/bicgstab_solve.py --grid 512 [--dtype f32] [--wind 0.6,0.3] [--scale 1.5] [--compare]

A is a convection-diffusion operator on a grid x grid mesh: 4 on the diagonal, -1 -/+ wx on the west / east neighbour, -1 -/+ wy on the south / north neighbour (--wind wx,wy; 0,0 is
the symmetric Laplacian).  --scale S > 0 solves S A S instead, s = 10^U(-S, S): a diagonal spread over 2 S decades, which the plain solver does not get through and the inverse
diagonal undoes.  Prints one JSON line per solve: iterations, residuals, seconds.  --compare also times this solver against the loop of torch operations
tilespmv_amd.operator.bicgstab on the same plan (what scripts/bicgstab_time.py records at full size; there the wind is the default one).
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
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--wind", default="0.6,0.3")
    ap.add_argument("--scale", type=float, default=0.0)
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=5000)
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api, generators as G
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("bicgstab_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    wx, wy = (float(w) for w in a.wind.split(","))
    k = a.grid
    m, n, rp, ci = G.laplacian5pt(k)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = ci.astype(np.int64) - rows
    v = np.select([d == 0, d == -1, d == 1, d == -k, d == k], [4.0, -1.0 - wx, -1.0 + wx, -1.0 - wy, -1.0 + wy])
    if a.scale > 0:
        s = 10.0 ** np.random.default_rng(5).uniform(-a.scale, a.scale, n)
        v = s[rows] * v * s[ci]
    v = v.astype(dtype)
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)).cuda()
    # the CSR on the device: the operator is built from it, and the inverse diagonal is taken from it by a kernel
    rpd, cid, vd = torch.from_numpy(np.ascontiguousarray(rp, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).cuda(), torch.from_numpy(v).cuda()
    op = SparseOperator(n, n, rpd, cid, vd)
    dinv = torch.empty(n, dtype=b.dtype, device="cuda")
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=torch.cuda.current_stream().cuda_stream, dtype=dtype)
    for label, dd in (("plain", None), ("jacobi", dinv)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = op.bicgstab(b, rtol=rtol, maxiter=a.maxiter, dinv=dd)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info.update({"solver": label, "n": n, "dtype": a.dtype, "seconds": round(dt, 4), "ms_per_iteration": round(dt * 1e3 / max(info["iterations"], 1), 4),
                     "true_relative_residual": float(torch.linalg.vector_norm(b - op.matvec(x)) / torch.linalg.vector_norm(b))})
        print(json.dumps(info))
    op.close()
    if a.compare:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "bicgstab_time.py"), "--workloads", "cd%d:%s" % (a.grid, a.dtype), "--rounds", "2"])


if __name__ == "__main__":
    main()
