"""Seconds per CG iteration: the solver in the library (tilespmv_cg_iterate: the product + three fused kernels, scalars on the device) against the loop of torch operations
(tilespmv_amd.halo.cg on a one-rank HaloSpMV) — the SAME plan object, matrix and right-hand side, one process, alternating a, b, a, b.

    python scripts/cg_time.py [--workloads lap4096:f64,lap4096:f32,fem3_68:f64,lap512:f64] [--rounds 3] [--iters 200] [--warmup 20] [--out profiles/cg_fused_ab.txt]

A window = device events around one call that starts a solve and runs `iters` iterations without a convergence check inside (a: cg(tol=0, maxiter=iters, check_every=iters);
b: begin + iterate(iters)); each side's set-up (a: two clones, three dots and two host reads; b: one product and two kernels) is inside its window, divided by `iters` like the
rest.  Before every window the same call runs `warmup` iterations untimed.  Beside the times: the product alone on the same plan (Plan.time) and the vector bytes either loop
moves per iteration by count (14 n against 11 n elements) — a byte count, not a measurement.  The condition printed per workload: b is faster than a by more than the spread
between a's own windows."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(name):
    from tilespmv_amd import generators as G
    if name.startswith("lap"):
        m, n, rp, ci = G.laplacian5pt(int(name[3:]))
        rows = np.repeat(np.arange(n), np.diff(rp))
        v = np.where(ci == rows, 4.0, -1.0)
    elif name.startswith("fem3_"):
        g = int(name[5:])
        m, n, rp, ci = G.fem_hex(g, g, g, 3)
        rows = np.repeat(np.arange(n), np.diff(rp))
        deg = np.bincount(rows, weights=(ci != rows).astype(np.float64), minlength=n)
        v = np.where(ci == rows, deg[rows] + 1.0, -1.0)      # diagonally dominant: -1 beside the diagonal, degree + 1 on it
    else:
        raise SystemExit("unknown workload %r (lapN, fem3_N)" % name)
    assert m == n and n % 16 == 0
    return n, rp, ci, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="lap4096:f64,lap4096:f32,fem3_68:f64,lap512:f64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.halo import HaloSpMV, cg
    if not torch.cuda.is_available():
        raise SystemExit("cg_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# seconds per CG iteration, fused solver (b: tilespmv_cg_iterate) vs torch loop (a: tilespmv_amd.halo.cg), same plan, one process, alternating a b a b")
    say("# %s, %d rounds, %d iterations per window after %d warm-up iterations, device events around each window" % (torch.cuda.get_device_name(0), a.rounds, a.iters, a.warmup))
    failed = []
    for wl in a.workloads.split(","):
        name, ty = wl.split(":")
        dt = np.dtype(np.float64 if ty == "f64" else np.float32)
        t0 = time.time()
        n, rp, ci, v = build(name)
        A = HaloSpMV(0, 1, n, rp, ci, v.astype(dt), dtype=dt)
        assert len(A.blocks) == 1 and A.nhalo == 0
        plan = A.blocks[0][2]
        b = A.new_vector()
        b[:n].copy_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dt)))
        x = A.new_vector()
        st = torch.cuda.current_stream().cuda_stream
        solver = api.CG(plan)
        spmv_ms = min(plan.time(b.data_ptr(), x.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
        info = plan.info()

        def window(side, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if side == "a":
                xa, it, rel = cg(A, b, tol=0.0, maxiter=iters, check_every=iters)
                out = xa
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
        diff = float(torch.linalg.vector_norm(xs["a"][:n] - xs["b"][:n]) / torch.linalg.vector_norm(xs["a"][:n]))
        ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
        spread_a, spread_b = max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"])
        ok = min(t["a"]) - max(t["b"]) > spread_a
        isz = dt.itemsize
        say()
        say("%s %s: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), set-up %.0f s" % (name, ty, n, len(ci), info["stream_bytes"] / 1e6, time.time() - t0))
        say("  product alone (Plan.time)            %.4f ms" % spmv_ms)
        say("  vector bytes per iteration, by count  a: 14 n = %.1f MB   b: 11 n = %.1f MB" % (14 * n * isz / 1e6, 11 * n * isz / 1e6))
        say("  a  torch loop    ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["a"]) + "   median %.4f  spread %.4f" % (ma * 1e3, spread_a * 1e3))
        say("  b  fused solver  ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["b"]) + "   median %.4f  spread %.4f" % (mb * 1e3, spread_b * 1e3))
        say("  ratio a / b (medians) %.3f;  product's share of an iteration  a: %.2f  b: %.2f" % (ma / mb, spmv_ms * 1e-3 / ma, spmv_ms * 1e-3 / mb))
        say("  b faster than a by more than a's spread (slowest b %.4f < fastest a %.4f - %.4f): %s" % (max(t["b"]) * 1e3, min(t["a"]) * 1e3, spread_a * 1e3, "yes" if ok else "NO"))
        say("  after %d iterations: |x_a - x_b| / |x_a| = %.3g, sqrt(rr / bb) of b = %.3g, status %s" % (a.iters, diff, state["relative_residual"], state["status_name"]))
        if not ok:
            failed.append(wl)
        solver.close()
        A.close()
        del A, b, x, xs
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
