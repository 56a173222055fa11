"""Seconds per CG iteration, iterations to the tolerance and time to the tolerance: point Jacobi (a: tilespmv_cg with d_dinv), block Jacobi with one 3 x 3 block per node (b:
tilespmv_cg_create_block; on the mesh only) and FSAI (c: tilespmv_cg_create_fsai) — the SAME deterministic plan, matrix and right-hand side, one process per workload, the arms
alternating a, b, c, a, b, c.  The arms a and b are code the FSAI change does not touch: they are the baseline.

    python scripts/fsai_time.py [--workloads femblk68:f64,femblk68:f32,lap4096:f64,lap4096:f32,lap512:f64,lap512:f32] [--rounds 3] [--iters 100] [--warmup 10]
                                [--step-timeout 900] [--out profiles/fsai_ab.txt]

femblkN: the pattern of generators.fem_hex(N, N, N, 3) with the symmetric positive definite values of tests/block_jacobi_mirror.py::femblk.  lapN: the 5-point Laplacian of an
N x N grid (4096: bound by the memory; 512: bound by the launches).  Every workload is one GPU step: a child process of its own under its own time limit (--step-timeout seconds);
after a step that fails or runs out of time no further step starts.  A window = device events around begin + iterate(iters), no convergence check inside; before every window
the same call runs `warmup` iterations untimed.  Then each arm solves to rtol (1e-10 in fp64, 1e-5 in fp32; check_every 8) for its iteration count; time to the tolerance is
that count times the arm's median time per iteration.  Beside them: the product alone on the same plan (Plan.time), the FSAI apply alone, the wall-clock time of the FSAI create
(pattern, values and both plans; synchronised) and the device time of one update (values and both plans' refresh).  No figure is fixed in advance: the table is the result."""
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
LABEL = {"a": "point Jacobi", "b": "block Jacobi", "c": "FSAI        "}


def matrix(name, dt):
    import block_jacobi_mirror as M
    import cg_mirror as CM
    from tilespmv_amd import generators as G
    if name.startswith("femblk"):
        k = int(name[6:])
        n, rp, ci, v = M.femblk(False, (k, k, k, 3))
        mesh = True
    elif name.startswith("lap"):
        m, n, rp, ci = G.laplacian5pt(int(name[3:]))
        v = CM.laplacian_values(n, rp, ci)
        mesh = False
    else:
        raise SystemExit("unknown workload %r (femblkN, lapN)" % name)
    return n, np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(v, dtype=dt), mesh


def one(wl, a):
    """One workload in this process; prints its lines."""
    import torch
    from tilespmv_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("fsai_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
    name, ty = wl.split(":")
    dt = np.dtype(np.float64 if ty == "f64" else np.float32)
    tdt = torch.float64 if ty == "f64" else torch.float32
    t0 = time.time()
    n, rp, ci, v, mesh = matrix(name, dt)
    plan = api.Plan.from_csr(n, n, len(ci), rp, ci, v, dtype=dt, deterministic=1, placement_tries=1)
    rpd, cid, vd = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def vec():
        return torch.zeros(n + 16, dtype=tdt, device="cuda")[:n]

    b, x, y, dinv = vec(), vec(), vec(), vec()
    b.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, n).astype(dt)))
    api.csr_diagonal_device(n, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dinv.data_ptr(), invert=True, stream=st, dtype=dt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    fs = api.FSAI(n, len(ci), rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), dt, stream=st, deterministic=1, placement_tries=1)
    torch.cuda.synchronize()
    create_ms = (time.perf_counter() - c0) * 1e3
    updates = []
    for r in range(4):                                                  # (the first one is the warm-up)
        torch.cuda.synchronize()
        e0.record(); fs.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st); e1.record()
        torch.cuda.synchronize()
        updates.append(e0.elapsed_time(e1))
    update_ms = float(np.median(updates[1:]))
    fi = fs.info(st)
    solvers = {"a": api.CG(plan, dinv.data_ptr()), "c": api.CG(plan, fsai=fs)}
    bj = None
    if mesh:
        bj = api.BlockJacobi(n, BS, dt)
        bj.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st)
        solvers["b"] = api.CG(plan, block=bj)
    arms = sorted(solvers)
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

    t = {side: [] for side in arms}
    for r in range(a.rounds):
        for side in arms:
            window(side, a.warmup)
            t[side].append(window(side, a.iters))
    solved = {}
    for side in arms:
        x.zero_()
        solved[side] = solvers[side].solve(b.data_ptr(), x.data_ptr(), rtol=RTOL[ty], maxiter=a.maxiter, check_every=8, stream=st)
    # the apply alone
    for _ in range(a.warmup):
        fs.apply(b.data_ptr(), y.data_ptr(), st)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        fs.apply(b.data_ptr(), y.data_ptr(), st)
    e1.record()
    torch.cuda.synchronize()
    apply_ms = e0.elapsed_time(e1) / a.iters
    med = {side: float(np.median(t[side])) for side in arms}
    print("# %s" % torch.cuda.get_device_name(0))
    print("%s %s: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), set-up %.0f s" % (name, ty, n, len(ci), info["stream_bytes"] / 1e6, time.time() - t0))
    print("  FSAI: nnz of G %d, longest row %d, %d truncated, %d fallback rows, %.1f MB on the device (both plans included); create %.1f ms (wall clock), update %.3f ms" % (
        fi["nnz"], fi["longest_row"], fi["truncated_rows"], fi["fallback_rows"], fi["device_bytes"] / 1e6, create_ms, update_ms))
    print("  product alone (Plan.time)              %.4f ms   one per iteration" % a_ms)
    print("  the FSAI apply alone (two products)    %.4f ms" % apply_ms)
    for side in arms:
        print("  %s  %s  ms per iteration      " % (side, LABEL[side]) + "  ".join("%.4f" % (s * 1e3) for s in t[side]) +
              "   median %.4f  spread %.4f" % (med[side] * 1e3, (max(t[side]) - min(t[side])) * 1e3))
    for side in arms:
        s = solved[side]
        print("  %s  %s  to rtol %.0e: %d iterations, status %s, sqrt(rr / bb) %.3g;  time to rtol by the median %.2f ms" % (
            side, LABEL[side], RTOL[ty], s["iterations"], s["status_name"], s["relative_residual"], s["iterations"] * med[side] * 1e3))
    tc = solved["c"]["iterations"] * med["c"]
    for side in arms[:-1]:
        print("  c against %s: per iteration %.3f x, iterations %.2f x fewer, time to rtol %.2f x (above 1: FSAI is faster)" % (
            side, med["c"] / med[side], solved[side]["iterations"] / max(solved["c"]["iterations"], 1), solved[side]["iterations"] * med[side] / max(tc, 1e-30)), flush=True)
    for s in solvers.values():
        s.close()
    if bj is not None:
        bj.close()
    fs.close()
    plan.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="femblk68:f64,femblk68:f32,lap4096:f64,lap4096:f32,lap512:f64,lap512:f32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--maxiter", type=int, default=50000)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this one workload in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    lines = ["# CG with point Jacobi (a: tilespmv_cg_create with d_dinv), block Jacobi bs = %d (b: tilespmv_cg_create_block, the mesh only) and FSAI (c: tilespmv_cg_create_fsai)," % BS,
             "# same deterministic plan, alternating a b c; %d rounds, %d iterations per window after %d warm-up iterations, device events around each window; one process per workload" % (
                 a.rounds, a.iters, a.warmup)]
    print("\n".join(lines), flush=True)
    rc = 0
    for wl in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", wl, "--rounds", str(a.rounds), "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--maxiter", str(a.maxiter)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)      # (the child's stderr passes through: the table holds its lines alone)
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
