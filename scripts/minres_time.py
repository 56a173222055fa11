"""Seconds per MINRES iteration: the solver in the library (tilespmv_minres_iterate: the product + three fused kernels, scalars on the device) against the loop of torch
operations (tilespmv_amd.operator.minres) — the SAME deterministic plan, matrix and right-hand side, one process per workload, alternating a, b, a, b.

    python scripts/minres_time.py [--workloads lap4096:f64,lap4096:f32,lap512:f64] [--rounds 3] [--iters 100] [--warmup 10] [--step-timeout 600] [--out profiles/minres_fused_ab.txt]

lapN: the 5-point Laplacian of an N x N grid shifted by -1 I (3 on the diagonal, -1 beside it): symmetric, spectrum in (-1, 7), indefinite; lap512 is launch-bound.
Every workload is one GPU step: a child process of its own under its own time limit (--step-timeout seconds); after a step that fails or runs out of time no further step starts.
A window = device events around one call that starts a solve and runs `iters` iterations without a convergence check inside (a: minres(tol=0, maxiter=iters,
check_every=iters); b: begin + iterate(iters)); each side's set-up is inside its window, divided by `iters` like the rest.  Before every window the same call runs `warmup`
iterations untimed.  Beside the times: the product alone on the same plan (Plan.time) and the vector elements either loop moves per iteration by count (23 n against 14 n) — a
count, not a measurement.  No ratio is fixed in advance: the table is the result."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(name):
    from tilespmv_amd import generators as G
    if not name.startswith("lap"):
        raise SystemExit("unknown workload %r (lapN)" % name)
    k = int(name[3:])
    m, n, rp, ci = G.laplacian5pt(k)
    v = np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 3.0, -1.0)
    return n, rp, ci, v


def one(wl, a):
    """One workload in this process; prints its lines."""
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator, minres
    if not torch.cuda.is_available():
        raise SystemExit("minres_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    name, ty = wl.split(":")
    dt = np.dtype(np.float64 if ty == "f64" else np.float32)
    tdt = torch.float64 if ty == "f64" else torch.float32
    t0 = time.time()
    n, rp, ci, v = build(name)
    op = SparseOperator(n, n, rp, ci, v.astype(dt), dtype=dt, deterministic=1, placement_tries=1)
    b = torch.zeros(n + 16, dtype=tdt, device="cuda")[:n]
    b.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dt)))
    x = torch.zeros(n + 16, dtype=tdt, device="cuda")[:n]
    y = torch.zeros(n + 16, dtype=tdt, device="cuda")[:n]
    st = torch.cuda.current_stream().cuda_stream
    solver = api.MINRES(op.A)
    a_ms = min(op.A.time(x.data_ptr(), y.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
    info = op.A.info()

    def window(side, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if side == "a":
            out, _ = minres(op, b, tol=0.0, maxiter=iters, check_every=iters)
        else:
            x.zero_()
            solver.begin(b.data_ptr(), x.data_ptr(), st)
            solver.iterate(x.data_ptr(), iters, st)
            out = x
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters, out

    t = {"a": [], "b": []}
    xs = {}
    for r in range(a.rounds):
        for side in ("a", "b"):
            window(side, a.warmup)
            sec, xs[side] = window(side, a.iters)
            t[side].append(sec)
    state = solver.state(st)
    diff = float(torch.linalg.vector_norm(xs["a"] - xs["b"]) / torch.linalg.vector_norm(xs["a"]))
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    spread_a, spread_b = max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"])
    prod = a_ms * 1e-3
    isz = dt.itemsize
    print("# %s" % torch.cuda.get_device_name(0))
    print("%s %s: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), entry_ordered %d, set-up %.0f s" % (name, ty, n, len(ci), info["stream_bytes"] / 1e6, info["entry_ordered"],
                                                                                                          time.time() - t0))
    print("  product alone (Plan.time)             %.4f ms   one per iteration" % a_ms)
    print("  vector bytes per iteration, by count  a: 23 n = %.1f MB   b: 14 n = %.1f MB" % (23 * n * isz / 1e6, 14 * n * isz / 1e6))
    print("  a  torch loop    ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["a"]) + "   median %.4f  spread %.4f" % (ma * 1e3, spread_a * 1e3))
    print("  b  fused solver  ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["b"]) + "   median %.4f  spread %.4f" % (mb * 1e3, spread_b * 1e3))
    print("  ratio a / b (medians) %.3f;  the product's share of an iteration  a: %.2f  b: %.2f" % (ma / mb, prod / ma, prod / mb))
    print("  after %d iterations: |x_a - x_b| / |x_a| = %.3g, sqrt(rr / bb) of b = %.3g, status %s" % (a.iters, diff, state["relative_residual"], state["status_name"]), flush=True)
    solver.close()
    op.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="lap4096:f64,lap4096:f32,lap512:f64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this one workload in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    lines = ["# seconds per MINRES iteration, fused solver (b: tilespmv_minres_iterate) vs torch loop (a: tilespmv_amd.operator.minres), same deterministic plan, alternating a b a b",
             "# %d rounds, %d iterations per window after %d warm-up iterations, device events around each window; one process per workload" % (a.rounds, a.iters, a.warmup)]
    print("\n".join(lines), flush=True)
    rc = 0
    for wl in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", wl, "--rounds", str(a.rounds), "--iters", str(a.iters),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, flush=True)
        lines += ["", r.stdout.rstrip()]
        if r.returncode != 0:      # nothing more is started on the device after a step that failed or ran out of time
            lines.append("# %s ended with status %d: stopped here" % (wl, r.returncode))
            print(lines[-1], flush=True)
            rc = 1
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
