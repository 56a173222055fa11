"""Seconds per GMRES inner iteration: the solver in the library (tilespmv_gmres_iterate: the product + four fused kernels, the Hessenberg column and the rotations on the device)
against the loop of torch operations (tilespmv_amd.operator.gmres: the basis a 2-D tensor, V @ w for the dot products, the rotations on the host) — the SAME deterministic plan,
matrix and right-hand side, one process per workload, alternating a, b, a, b.

    python scripts/gmres_time.py [--workloads cd4096:f64,cd4096:f32,cd512:f64] [--restart 30] [--cycles 3] [--rounds 3] [--step-timeout 600] [--out profiles/gmres_fused_ab.txt]

cdN: the convection-dominated values of tests/gmres_mirror.py's convdom67 (4 on the diagonal, -9 / 7 west / east, -6 / 4 south / north) on an N x N grid; cd512 is launch-bound.
Every workload is one GPU step: a child process of its own under its own time limit (--step-timeout seconds); after a step that fails or runs out of time no further step starts.
A window = device events around one call that starts a solve and runs `cycles` full cycles of `restart` inner iterations without a convergence check inside (a: gmres(tol=0,
maxiter=cycles * restart, check_every=maxiter); b: begin + iterate(cycles * restart)); each side's set-up, closes and opens are inside its window, divided by the inner iterations
like the rest.  Before every window the same call runs one cycle untimed.  Beside the times: the product alone on the same plan (Plan.time) and the vector elements the fused
solver moves per inner iteration by count, averaged over a cycle — a count, not a measurement.  No ratio is fixed in advance: the table is the result.

    python scripts/gmres_time.py --basis value,float32 [--workloads cd4096:f64,cd2048:f64,cd512:f64] [--solve-rtol 1e-10] [--out profiles/gmres_cb_ab.txt]

times the fused solver against ITSELF instead, with its Krylov basis stored in each of the named forms (api.GMRES(basis=...)), on the same plan in the same
process, alternating windows as above.  Beside each form's times: its bytes per row and inner iteration by count with the re-reads — the 4 k + 1 basis elements at the basis's own
size, the other 2 ceil(k / 8) + 5 (+ 1 with a narrow basis) at the value type's — the rate on that count, what the first form's rate would give on the other's count, and one solve
to --solve-rtol in each form (iterations and wall-clock ms, one host read per 8 iterations)."""
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
    if not name.startswith("cd"):
        raise SystemExit("unknown workload %r (cdN)" % name)
    k = int(name[2:])
    m, n, rp, ci = G.laplacian5pt(k)
    d = ci.astype(np.int64) - np.repeat(np.arange(n), np.diff(rp))
    v = np.select([d == 0, d == -1, d == 1, d == -k, d == k], [4.0, -9.0, 7.0, -6.0, 4.0])
    return n, rp, ci, v


def one(wl, a):
    """One workload in this process; prints its lines."""
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator, gmres
    if not torch.cuda.is_available():
        raise SystemExit("gmres_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
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
    m = a.restart
    solver = api.GMRES(op.A, m)
    a_ms = min(op.A.time(x.data_ptr(), y.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
    info = op.A.info()

    def window(side, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if side == "a":
            out, _ = gmres(op, b, tol=0.0, maxiter=iters, restart=m, check_every=iters)
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
            window(side, m)
            sec, xs[side] = window(side, a.cycles * m)
            t[side].append(sec)
    state = solver.state(st)
    diff = float(torch.linalg.vector_norm(xs["a"] - xs["b"]) / torch.linalg.vector_norm(xs["a"]))
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    spread_a, spread_b = max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"])
    prod = a_ms * 1e-3
    isz = dt.itemsize
    ks = np.arange(1, m + 1)
    once, reread = float(np.mean(3 * ks + 7)), float(np.mean(4 * ks + 2 * ((ks + 7) // 8) + 6))
    print("# %s" % torch.cuda.get_device_name(0))
    print("%s %s restart %d: n = %d, nnz = %d, plan stream bytes %.1f MB (plan model), entry_ordered %d, set-up %.0f s" % (name, ty, m, n, len(ci), info["stream_bytes"] / 1e6,
                                                                                                                     info["entry_ordered"], time.time() - t0))
    print("  product alone (Plan.time)             %.4f ms" % a_ms)
    print("  b's vector bytes per inner iteration, by count, mean over a cycle   3 k + 7: %.1f n = %.1f MB   with the re-reads, 4 k + 2 ceil(k / 8) + 6: %.1f n = %.1f MB"
          % (once, once * n * isz / 1e6, reread, reread * n * isz / 1e6))
    print("  a  torch loop    ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["a"]) + "   median %.4f  spread %.4f" % (ma * 1e3, spread_a * 1e3))
    print("  b  fused solver  ms per iteration     " + "  ".join("%.4f" % (s * 1e3) for s in t["b"]) + "   median %.4f  spread %.4f" % (mb * 1e3, spread_b * 1e3))
    print("  ratio a / b (medians) %.3f;  the product's share of an iteration  a: %.2f  b: %.2f;  b's rate on the count with re-reads %.2f TB/s"
          % (ma / mb, prod / ma, prod / mb, reread * n * isz / max(mb - prod, 1e-12) / 1e12))
    print("  after %d iterations: |x_a - x_b| / |x_a| = %.3g, sqrt(rr / bb) of b = %.3g, status %s" % (a.cycles * m, diff, state["relative_residual"], state["status_name"]), flush=True)
    solver.close()
    op.close()
    return 0


def one_basis(wl, a):
    """One workload in this process with --basis: the fused solver in each of the named forms of its stored basis on the same plan, alternating windows; prints its lines."""
    import torch
    from tilespmv_amd import api
    from tilespmv_amd.operator import SparseOperator
    if not torch.cuda.is_available():
        raise SystemExit("gmres_time.py needs a HIP device: a time taken anywhere else says nothing about the MI355X")
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
    m = a.restart
    forms = a.basis.split(",")
    solvers = {f: api.GMRES(op.A, m, basis=f) for f in forms}
    a_ms = min(op.A.time(x.data_ptr(), y.data_ptr(), st, warmup=20, reps=100) for _ in range(3))
    prod = a_ms * 1e-3

    def window(form, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        x.zero_()
        solvers[form].begin(b.data_ptr(), x.data_ptr(), st)
        solvers[form].iterate(x.data_ptr(), iters, st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters, x.clone()

    t = {f: [] for f in forms}
    xs = {}
    for r in range(a.rounds):
        for f in forms:
            window(f, m)
            sec, xs[f] = window(f, a.cycles * m)
            t[f].append(sec)
    ks = np.arange(1, m + 1)
    groups = (ks + 7) // 8
    # bytes per row and inner iteration with the re-reads, mean over a cycle: every element of the value type, or the 4 k + 1 basis elements at the basis's own size
    # (a narrow basis: one more, the value-type copy that k_gm_next writes beside the stored vector)
    count = {f: float(np.mean((4 * ks + 1) * solvers[f].basis_bytes + (2 * groups + 5 + (solvers[f].basis_bytes != dt.itemsize)) * dt.itemsize)) for f in forms}
    print("# %s" % torch.cuda.get_device_name(0))
    print("%s %s restart %d: n = %d, nnz = %d, entry_ordered %d, set-up %.0f s" % (name, ty, m, n, len(ci), op.A.info()["entry_ordered"], time.time() - t0))
    print("  product alone (Plan.time)             %.4f ms" % a_ms)
    med = {}
    for f in forms:
        med[f] = float(np.median(t[f]))
        print("  basis %-8s %d bytes per element, workspace %.1f MB, %.1f bytes per row and iteration by count (%.1f MB)   ms per iteration  %s   median %.4f  spread %.4f   rate on that count %.2f TB/s"
              % (f, solvers[f].basis_bytes, solvers[f].workspace_bytes / 1e6, count[f], count[f] * n / 1e6, "  ".join("%.4f" % (s * 1e3) for s in t[f]), med[f] * 1e3,
                 (max(t[f]) - min(t[f])) * 1e3, count[f] * n / max(med[f] - prod, 1e-12) / 1e12))
    for f in forms[1:]:
        f0 = forms[0]
        predicted = (count[f0] * n / max(med[f0] - prod, 1e-12))      # the first form's achieved rate, applied to this form's count
        print("  %s / %s (medians) %.3f;  by the byte counts at %s's rate, with the product: %.3f;  |x_%s - x_%s| / |x_%s| after %d iterations = %.3g"
              % (f0, f, med[f0] / med[f], f0, med[f0] / (count[f] * n / predicted + prod), f, f0, f0, a.cycles * m,
                 float(torch.linalg.vector_norm(xs[f] - xs[f0]) / torch.linalg.vector_norm(xs[f0]))))
    if a.solve_rtol > 0:
        for f in forms:
            x.zero_()
            solvers[f].solve(b.data_ptr(), x.data_ptr(), rtol=a.solve_rtol, maxiter=m, check_every=m, stream=st)      # (untimed: the first call)
            x.zero_()
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            s = solvers[f].solve(b.data_ptr(), x.data_ptr(), rtol=a.solve_rtol, maxiter=a.solve_maxiter, check_every=8, stream=st)
            torch.cuda.synchronize()
            print("  solve to rtol %.0e, basis %-8s %d iterations, %s, sqrt(rr / bb) %.3g, %.1f ms" % (a.solve_rtol, f, s["iterations"], s["status_name"], s["relative_residual"],
                                                                                                     (time.perf_counter() - w0) * 1e3), flush=True)
    for s in solvers.values():
        s.close()
    op.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cd4096:f64,cd4096:f32,cd512:f64")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--basis", default=None, help="e.g. value,float32: time the fused solver in these forms of its stored basis against each other instead of a against b")
    ap.add_argument("--solve-rtol", type=float, default=1e-10, help="with --basis: also one solve to this tolerance in each form (0: none)")
    ap.add_argument("--solve-maxiter", type=int, default=3000)
    ap.add_argument("--one", default=None, help="(internal) run this one workload in this process")
    a = ap.parse_args()
    if a.one:
        return one_basis(a.one, a) if a.basis else one(a.one, a)
    if a.basis:
        if a.workloads == ap.get_default("workloads"):
            a.workloads = "cd4096:f64,cd2048:f64,cd512:f64"
        lines = ["# seconds per GMRES(%d) inner iteration of the fused solver (tilespmv_gmres_iterate) with its basis stored as: %s — same deterministic plan, same process, alternating windows"
                 % (a.restart, a.basis)]
    else:
        lines = ["# seconds per GMRES(%d) inner iteration, fused solver (b: tilespmv_gmres_iterate) vs torch loop (a: tilespmv_amd.operator.gmres), same deterministic plan, alternating a b a b" % a.restart]
    lines.append("# %d rounds, %d full cycles per window after one warm-up cycle, device events around each window; one process per workload" % (a.rounds, a.cycles))
    print("\n".join(lines), flush=True)
    rc = 0
    for wl in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", wl, "--restart", str(a.restart), "--cycles", str(a.cycles),
               "--rounds", str(a.rounds)]
        if a.basis:
            cmd += ["--basis", a.basis, "--solve-rtol", str(a.solve_rtol), "--solve-maxiter", str(a.solve_maxiter)]
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
