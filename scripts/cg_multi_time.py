"""Milliseconds per system-iteration of CG on nvec right-hand sides: the multi-right-hand-side solver (b: one tilespmv_cg_multi begin + iterate around the multi-vector
product) against nvec successive single solves (a: tilespmv_cg begin + iterate on contiguous copies of the columns) — the SAME plan object and data, one process,
alternating a, b, a, b (the protocol of scripts/cg_time.py).

    python scripts/cg_multi_time.py [--workloads lap4096:f64,lap4096:f32,fem3_68:f64,lap512:f64] [--nvec 2,4,8] [--rounds 3] [--iters 200] [--warmup 20]
                                    [--out profiles/cg_multi_ab.txt]

A window = device events around one side's whole work for nvec systems: a: for every column, x = 0, begin, iterate(iters); b: X = 0, begin, iterate(iters).  No convergence
check inside; each side's set-up is inside its window.  The window's time is divided by iters * nvec: ms per system-iteration.  Before every window the same work runs with
`warmup` iterations untimed.  Beside the times: the products alone on the same plan (Plan.time, Plan.time_spmm) and the ratio predicted before the solver existed, from figures
committed earlier (README.md) — a prediction, not a measurement.  The condition printed per row: b is faster than a by more than the spread between a's
own windows; it is asked of nvec >= 4."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cg_time import build  # noqa: E402  (the workloads of scripts/cg_time.py)

# a / b predicted from the single solver's measured iteration and the products' measured times; "several" = launch-bound, no figure was predicted
PREDICTED = {("lap4096", "f64", 8): "1.2", ("fem3_68", "f64", 8): "1.4", ("lap512", "f64", 2): "several-fold", ("lap512", "f64", 4): "several-fold", ("lap512", "f64", 8): "several-fold"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="lap4096:f64,lap4096:f32,fem3_68:f64,lap512:f64")
    ap.add_argument("--nvec", default="2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tilespmv_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("cg_multi_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# ms per system-iteration of CG on nvec right-hand sides: b = one tilespmv_cg_multi solve, a = nvec successive tilespmv_cg solves; same plan, one process, alternating a b a b")
    say("# %s, %d rounds, %d iterations per window after %d warm-up iterations, device events around each window" % (torch.cuda.get_device_name(0), a.rounds, a.iters, a.warmup))
    failed = []
    for wl in a.workloads.split(","):
        name, ty = wl.split(":")
        dt = np.dtype(np.float64 if ty == "f64" else np.float32)
        tdt = torch.float64 if ty == "f64" else torch.float32
        t0 = time.time()
        n, rp, ci, v = build(name)
        plan = api.Plan.from_csr(n, n, len(ci), np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), v.astype(dt), dtype=dt)
        st = torch.cuda.current_stream().cuda_stream
        x1, y1 = torch.ones(n + 16, dtype=tdt, device="cuda"), torch.zeros(n + 16, dtype=tdt, device="cuda")
        spmv_ms = min(plan.time(x1.data_ptr(), y1.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
        del x1, y1
        info = plan.info()
        say()
        say("%s %s: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), set-up %.0f s;  product alone (Plan.time) %.4f ms" % (name, ty, n, len(ci), info["stream_bytes"] / 1e6,
                                                                                                                                   time.time() - t0, spmv_ms))
        single = api.CG(plan)
        for nvec in [int(k) for k in a.nvec.split(",")]:
            B = torch.empty((n + 16, nvec), dtype=tdt, device="cuda")
            for j in range(nvec):
                B[:n, j].copy_(torch.from_numpy(np.random.default_rng(3 + j).uniform(-1, 1, n).astype(dt)))
            X = torch.zeros((n + 16, nvec), dtype=tdt, device="cuda")
            bs = [B[:, j].contiguous() for j in range(nvec)]
            xs = [torch.zeros(n + 16, dtype=tdt, device="cuda") for _ in range(nvec)]
            multi = api.CGMulti(plan, nvec)
            Y = torch.zeros((n + 16, nvec), dtype=tdt, device="cuda")
            spmm_ms = min(plan.time_spmm(B.data_ptr(), Y.data_ptr(), nvec, st, warmup=20, reps=100) for _ in range(3))
            del Y

            def window(side, iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if side == "a":
                    for b, x in zip(bs, xs):
                        x.zero_()
                        single.begin(b.data_ptr(), x.data_ptr(), st)
                        single.iterate(x.data_ptr(), iters, st)
                else:
                    X.zero_()
                    multi.begin(B.data_ptr(), X.data_ptr(), st)
                    multi.iterate(X.data_ptr(), iters, st)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / (iters * nvec)

            t = {"a": [], "b": []}
            for r in range(a.rounds):
                for side in ("a", "b"):
                    window(side, a.warmup)
                    t[side].append(window(side, a.iters))
            states = multi.state(st)
            diffs = [float(torch.linalg.vector_norm(xs[j][:n] - X[:n, j]) / torch.linalg.vector_norm(xs[j][:n])) for j in range(nvec)]
            ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
            spread_a, spread_b = max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"])
            ok = min(t["a"]) - max(t["b"]) > spread_a
            asked = nvec >= 4
            say("  nvec %d: products alone: Plan.time_spmm %.4f ms = %.4f per right-hand side, against Plan.time %.4f" % (nvec, spmm_ms, spmm_ms / nvec, spmv_ms))
            say("    a  %d single solves  ms per system-iteration   " % nvec + "  ".join("%.4f" % s for s in t["a"]) + "   median %.4f  spread %.4f" % (ma, spread_a))
            say("    b  one multi solve   ms per system-iteration   " + "  ".join("%.4f" % s for s in t["b"]) + "   median %.4f  spread %.4f" % (mb, spread_b))
            say("    ratio a / b (medians) %.3f;  predicted before the solver existed: %s" % (ma / mb, PREDICTED.get((name, ty, nvec), "no prediction")))
            say("    b faster than a by more than a's spread (slowest b %.4f < fastest a %.4f - %.4f): %s%s" % (max(t["b"]), min(t["a"]), spread_a, "yes" if ok else "NO",
                                                                                                               "" if asked else "   (not asked of nvec 2)"))
            say("    after %d iterations, per column: |x_a - x_b| / |x_a| = %s;  sqrt(rr / bb) of b = %s" % (a.iters, " ".join("%.2g" % d for d in diffs),
                                                                                                            " ".join("%.2g" % s["relative_residual"] for s in states)))
            if asked and not ok:
                failed.append("%s nvec %d" % (wl, nvec))
            multi.close()
            del B, X, bs, xs
            torch.cuda.empty_cache()
        single.close()
        plan.close()
        torch.cuda.empty_cache()
    say()
    say("# condition met on every row with nvec >= 4: %s" % ("yes" if not failed else "NO (%s)" % ", ".join(failed)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
