"""Seconds per CG iteration and iterations to the tolerance: point Jacobi (a: tilespmv_cg with d_dinv, unchanged from before the block preconditioner existed — the baseline)
against block Jacobi with one 3 x 3 block per node (b: tilespmv_cg_create_block) — the SAME deterministic plan, matrix and right-hand side, one process per workload, alternating
a, b, a, b.

    python scripts/block_jacobi_time.py [--workloads femblk68:f64,femblk68:f32] [--rounds 3] [--iters 100] [--warmup 10] [--step-timeout 900] [--out profiles/block_jacobi_ab.txt]

femblkN: the pattern of generators.fem_hex(N, N, N, 3) with the symmetric positive definite values of tests/block_jacobi_mirror.py::femblk (A = T^T (G x C) T: full, badly scaled,
rotated 3 x 3 node blocks).  Every workload is one GPU step: a child process of its own under its own time limit (--step-timeout seconds); after a step that fails or runs out of
time no further step starts.  A window = device events around begin + iterate(iters), no convergence check inside; before every window the same call runs `warmup` iterations
untimed.  Then each arm solves to rtol (1e-10 in fp64, 1e-5 in fp32; check_every 8) for its iteration count, and the apply kernel runs alone (device events around `iters`
applies) for its time and its bytes per second BY COUNT ((bs + 2) n elements).  Beside the times: the product alone on the same plan (Plan.time) and the vector elements per
iteration by count (13 n against (13 + bs) n).  No figure is fixed in advance: the table is the result."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BS = 3
RTOL = {"f64": 1e-10, "f32": 1e-5}


def one(wl, a):
    """One workload in this process; prints its lines."""
    import torch
    import block_jacobi_mirror as M
    from tilespmv_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("block_jacobi_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    name, ty = wl.split(":")
    if not name.startswith("femblk"):
        raise SystemExit("unknown workload %r (femblkN)" % name)
    k = int(name[6:])
    dt = np.dtype(np.float64 if ty == "f64" else np.float32)
    tdt = torch.float64 if ty == "f64" else torch.float32
    t0 = time.time()
    n, rp, ci, v = M.femblk(False, (k, k, k, 3))
    rp, ci, v = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=dt)
    plan = api.Plan.from_csr(n, n, len(ci), rp, ci, v, dtype=dt, deterministic=1, placement_tries=1)
    rpd, cid, vd = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def vec():
        return torch.zeros(n + 16, dtype=tdt, device="cuda")[:n]

    b, x, y, dinv = vec(), vec(), vec(), vec()
    b.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dt)))
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=st, dtype=dt)
    bj = api.BlockJacobi(n, BS, dt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bj.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st)      # (warm-up)
    torch.cuda.synchronize()
    e0.record(); bj.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st); e1.record()
    torch.cuda.synchronize()
    update_ms = e0.elapsed_time(e1)
    bji = bj.info(st)
    solvers = {"a": api.CG(plan, dinv.data_ptr()), "b": api.CG(plan, block=bj)}
    a_ms = min(plan.time(x.data_ptr(), y.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
    info = plan.info()

    def window(side, iters):
        torch.cuda.synchronize()
        x.zero_()
        e0.record()
        solvers[side].begin(b.data_ptr(), x.data_ptr(), st)
        solvers[side].iterate(x.data_ptr(), iters, st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters

    t = {"a": [], "b": []}
    for r in range(a.rounds):
        for side in ("a", "b"):
            window(side, a.warmup)
            t[side].append(window(side, a.iters))
    solved = {}
    for side in ("a", "b"):
        x.zero_()
        solved[side] = solvers[side].solve(b.data_ptr(), x.data_ptr(), rtol=RTOL[ty], maxiter=a.maxiter, check_every=8, stream=st)
    # the apply alone
    for _ in range(a.warmup):
        bj.apply(b.data_ptr(), y.data_ptr(), st)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        bj.apply(b.data_ptr(), y.data_ptr(), st)
    e1.record()
    torch.cuda.synchronize()
    apply_s = e0.elapsed_time(e1) * 1e-3 / a.iters
    isz = dt.itemsize
    apply_bytes = (BS + 2) * n * isz
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    spread_a, spread_b = max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"])
    prod = a_ms * 1e-3
    print("# %s" % torch.cuda.get_device_name(0))
    print("%s %s: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), set-up %.0f s" % (name, ty, n, len(ci), info["stream_bytes"] / 1e6, time.time() - t0))
    print("  block Jacobi, bs = %d: %d blocks, %d singular, %.1f MB on the device; update %.3f ms" % (BS, bji["blocks"], bji["singular_blocks"], bji["device_bytes"] / 1e6, update_ms))
    print("  product alone (Plan.time)              %.4f ms   one per iteration" % a_ms)
    print("  vector bytes per iteration, by count   a: 13 n = %.1f MB   b: (13 + bs) n = %.1f MB" % (13 * n * isz / 1e6, (13 + BS) * n * isz / 1e6))
    print("  a  point Jacobi  ms per iteration      " + "  ".join("%.4f" % (s * 1e3) for s in t["a"]) + "   median %.4f  spread %.4f" % (ma * 1e3, spread_a * 1e3))
    print("  b  block Jacobi  ms per iteration      " + "  ".join("%.4f" % (s * 1e3) for s in t["b"]) + "   median %.4f  spread %.4f" % (mb * 1e3, spread_b * 1e3))
    print("  ratio b / a per iteration (medians) %.3f;  the product's share of an iteration  a: %.2f  b: %.2f" % (mb / ma, prod / ma, prod / mb))
    print("  the apply alone                        %.4f ms   (bs + 2) n = %.1f MB by count: %.0f GB/s" % (apply_s * 1e3, apply_bytes / 1e6, apply_bytes / apply_s / 1e9))
    for side, label in (("a", "point Jacobi"), ("b", "block Jacobi")):
        s = solved[side]
        print("  %s  %s  to rtol %.0e: %d iterations, status %s, sqrt(rr / bb) %.3g" % (side, label, RTOL[ty], s["iterations"], s["status_name"], s["relative_residual"]))
    ia, ib = solved["a"]["iterations"], solved["b"]["iterations"]
    print("  iterations a / b %.2f;  time to rtol by the medians  a: %.1f ms  b: %.1f ms  (a / b %.2f)" % (ia / max(ib, 1), ia * ma * 1e3, ib * mb * 1e3, (ia * ma) / max(ib * mb, 1e-30)),
          flush=True)
    for s in solvers.values():
        s.close()
    bj.close()
    plan.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="femblk68:f64,femblk68:f32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this one workload in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    lines = ["# CG with point Jacobi (a: tilespmv_cg_create with d_dinv) vs block Jacobi, bs = %d (b: tilespmv_cg_create_block), same deterministic plan, alternating a b a b" % BS,
             "# %d rounds, %d iterations per window after %d warm-up iterations, device events around each window; one process per workload" % (a.rounds, a.iters, a.warmup)]
    print("\n".join(lines), flush=True)
    rc = 0
    for wl in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", wl, "--rounds", str(a.rounds), "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--maxiter", str(a.maxiter)]
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
