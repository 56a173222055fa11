"""Seconds per CGLS iteration: the solver in the library (tilespmv_cgls_iterate: the two products + four fused kernels, scalars on the device) against the loop of torch operations
(tilespmv_amd.operator.cgls) — the SAME SparseOperator, matrix and right-hand side, one process, alternating a, b, a, b.

    python scripts/cgls_time.py [--workloads lapI4096:f64,lapI4096:f32,femI3_68:f64,lapI512:f64,tall4M:f64] [--rounds 3] [--iters 100] [--warmup 10] [--out profiles/cgls_fused_ab.txt]

A window = device events around one call that starts a solve and runs `iters` iterations without a convergence check inside (a: cgls(tol=0, maxiter=iters, check_every=iters);
b: begin + iterate(iters)); each side's set-up (a: clones, two products, a norm and two host reads, and the residual it reports at the end; b: three products and three kernels) is
inside its window, divided by `iters` like the rest.  Before every window the same call runs `warmup` iterations untimed.  Beside the times: both products alone on the same plans
(Plan.time) and the vector elements either loop moves per iteration by count (7 rows + 12 cols against 4 rows + 7 cols) — a count, not a measurement.  The condition printed per
workload: the slowest b window is faster than the fastest a window by more than the spread between a's own windows.  No speed-up is fixed in advance: workloads where the
condition is not met are reported as such."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stack_identity(n, rp, ci, v):
    """[S; I] for a square CSR S: the identity's rows behind S's (2n x n)."""
    rp = np.asarray(rp, dtype=np.int64)
    return 2 * n, n, np.concatenate([rp, rp[-1] + np.arange(1, n + 1)]).astype(np.int32), np.concatenate([ci, np.arange(n)]).astype(np.int32), np.concatenate([v, np.ones(n)])


def build(name):
    from tilespmv_amd import generators as G
    if name.startswith("lapI"):
        m, n, rp, ci = G.laplacian5pt(int(name[4:]))
        rows = np.repeat(np.arange(n), np.diff(rp))
        return stack_identity(n, rp, ci, np.where(ci == rows, 4.0, -1.0))
    if name.startswith("femI3_"):
        g = int(name[6:])
        m, n, rp, ci = G.fem_hex(g, g, g, 3)
        rows = np.repeat(np.arange(n), np.diff(rp))
        deg = np.bincount(rows, weights=(ci != rows).astype(np.float64), minlength=n)
        return stack_identity(n, rp, ci, np.where(ci == rows, deg[rows] + 1.0, -1.0))      # diagonally dominant: -1 beside the diagonal, degree + 1 on it
    if name.startswith("tall") and name.endswith("M"):      # tallNM: N M rows, N / 4 M columns, 8 uniformly random columns per row
        rows = int(name[4:-1]) * 1000000
        cols = rows // 4
        m, n, rp, ci = G.uniform_per_row(rows, cols, 8, seed=21)
        rng = np.random.default_rng(22)
        return rows, cols, rp, ci, rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    raise SystemExit("unknown workload %r (lapIN, femI3_N, tallNM)" % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="lapI4096:f64,lapI4096:f32,femI3_68:f64,lapI512:f64,tall4M:f64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator, cgls
    if not torch.cuda.is_available():
        raise SystemExit("cgls_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# seconds per CGLS iteration, fused solver (b: tilespmv_cgls_iterate) vs torch loop (a: tilespmv_amd.operator.cgls), same operator, one process, alternating a b a b")
    say("# %s, %d rounds, %d iterations per window after %d warm-up iterations, device events around each window" % (torch.cuda.get_device_name(0), a.rounds, a.iters, a.warmup))
    failed = []
    for wl in a.workloads.split(","):
        name, ty = wl.split(":")
        dt = np.dtype(np.float64 if ty == "f64" else np.float32)
        tdt = torch.float64 if ty == "f64" else torch.float32
        t0 = time.time()
        rows, cols, rp, ci, v = build(name)
        op = SparseOperator(rows, cols, rp, ci, v.astype(dt), dtype=dt)
        b = torch.zeros(rows + 16, dtype=tdt, device="cuda")[:rows]
        b.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, rows).astype(dt)))
        x = torch.zeros(cols + 16, dtype=tdt, device="cuda")[:cols]
        yr = torch.zeros(rows + 16, dtype=tdt, device="cuda")[:rows]
        st = torch.cuda.current_stream().cuda_stream
        solver = api.CGLS(op.A, op.AT)
        a_ms = min(op.A.time(x.data_ptr(), yr.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
        at_ms = min(op.AT.time(b.data_ptr(), x.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
        x.zero_()
        info_a, info_at = op.A.info(), op.AT.info()

        def window(side, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if side == "a":
                out, _ = cgls(op, b, tol=0.0, maxiter=iters, check_every=iters)
            else:
                x.zero_()
                solver.begin(b.data_ptr(), x.data_ptr(), 0.0, st)
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
        ok = min(t["a"]) - max(t["b"]) > spread_a
        isz = dt.itemsize
        prod = (a_ms + at_ms) * 1e-3
        say()
        say("%s %s: %d x %d, nnz = %d, plan stream bytes A %.1f MB, A^T %.1f MB (plan model), set-up %.0f s" % (name, ty, rows, cols, len(ci), info_a["stream_bytes"] / 1e6,
                                                                                                            info_at["stream_bytes"] / 1e6, time.time() - t0))
        say("  products alone (Plan.time)            A %.4f ms   A^T %.4f ms   both %.4f ms" % (a_ms, at_ms, a_ms + at_ms))
        say("  vector bytes per iteration, by count  a: 7 rows + 12 cols = %.1f MB   b: 4 rows + 7 cols = %.1f MB" % ((7 * rows + 12 * cols) * isz / 1e6, (4 * rows + 7 * cols) * isz / 1e6))
        say("  a  torch loop    ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["a"]) + "   median %.4f  spread %.4f" % (ma * 1e3, spread_a * 1e3))
        say("  b  fused solver  ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["b"]) + "   median %.4f  spread %.4f" % (mb * 1e3, spread_b * 1e3))
        say("  ratio a / b (medians) %.3f;  the products' share of an iteration  a: %.2f  b: %.2f" % (ma / mb, prod / ma, prod / mb))
        say("  b faster than a by more than a's spread (slowest b %.4f < fastest a %.4f - %.4f): %s" % (max(t["b"]) * 1e3, min(t["a"]) * 1e3, spread_a * 1e3, "yes" if ok else "NO"))
        say("  after %d iterations: |x_a - x_b| / |x_a| = %.3g, sqrt(nn / nn0) of b = %.3g, status %s" % (a.iters, diff, state["relative_normal_residual"], state["status_name"]))
        if not ok:
            failed.append(wl)
        solver.close()
        op.close()
        del op, b, x, yr, xs
        torch.cuda.empty_cache()
    say()
    say("# condition met on every workload: %s" % ("yes" if not failed else "NO (%s)" % ", ".join(failed)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
