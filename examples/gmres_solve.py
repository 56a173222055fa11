"""A x = b for nonsymmetric systems that BiCGStab does not solve, by restarted GMRES in the library, next to BiCGStab on the same plan, on one GPU (SparseOperator.gmres over
tilespmv_gmres_*: one product and four fused kernels per inner iteration, every scalar on the device).

    python examples/gmres_solve.py --grid 67 [--dtype f32] [--restart 30] [--stencil shiftskew|convdom|D,W,E,S,N] [--basis float32]

A lives on the pattern of the 5-point Laplacian of a grid x grid mesh: D on the diagonal, W / E on the west / east neighbour, S / N on the south / north neighbour.
  shiftskew   0.25; -1, 1; -1, 1      a skew-symmetric operator shifted by I / 4: BiCGStab stagnates, or reports a recurrence residual far below the true one
  convdom     4; -9, 7; -6, 4         convection-dominated: BiCGStab needs several times the products of GMRES
--basis float32 stores GMRES's Krylov basis as 4-byte floats (fp64: all arithmetic stays double, about half the bytes per iteration and half the workspace; inside
one cycle the true residual stops near 6e-8 x the residual the cycle began with, so the solve accepts convergence only on a recomputed residual; f32: the same solver).
Prints one JSON line per solver and stencil: status, iterations, products, the residual the solver reports and the true one, seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STENCILS = {"shiftskew": (0.25, -1.0, 1.0, -1.0, 1.0), "convdom": (4.0, -9.0, 7.0, -6.0, 4.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=67)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--stencil", default="shiftskew,convdom".split(","), nargs="*")
    ap.add_argument("--rtol", type=float, default=None)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--basis", default=None, choices=["value", "float32"], help="how GMRES stores its Krylov basis (default: the value type)")
    a = ap.parse_args()
    import torch
    from tilespmv_amd import generators as G
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("gmres_solve.py needs a HIP device (there is no CPU path in the product)")
    dtype = np.dtype(np.float64 if a.dtype == "f64" else np.float32)
    rtol = a.rtol if a.rtol is not None else (1e-10 if a.dtype == "f64" else 1e-5)
    k = a.grid
    m, n, rp, ci = G.laplacian5pt(k)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = ci.astype(np.int64) - rows
    b = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)).cuda()
    for name in a.stencil:
        dg, w, e, s, nn = STENCILS[name] if name in STENCILS else (float(t) for t in name.split(","))
        v = np.select([d == 0, d == -1, d == 1, d == -k, d == k], [dg, w, e, s, nn]).astype(dtype)
        with SparseOperator(n, n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), v) as op:
            for solver, products in (("bicgstab", 2), ("gmres", 1)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if solver == "gmres":
                    x, info = op.gmres(b, rtol=rtol, maxiter=a.maxiter, restart=a.restart, basis=a.basis)
                else:
                    x, info = op.bicgstab(b, rtol=rtol, maxiter=a.maxiter)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                info.update({"solver": solver if solver != "gmres" or not a.basis else "gmres(basis=%s)" % a.basis, "stencil": name, "n": n, "dtype": a.dtype, "products": products * info["iterations"], "seconds": round(dt, 4),
                             "true_relative_residual": float(torch.linalg.vector_norm(b - op.matvec(x)) / torch.linalg.vector_norm(b))})
                print(json.dumps(info))


if __name__ == "__main__":
    main()
