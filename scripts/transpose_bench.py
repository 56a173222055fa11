#!/usr/bin/env python3
"""What a transposed plan costs and how fast it runs (TILESPMV_CREATE_TRANSPOSE).

Per workload, in one process, the CSR arrays already on the device:
  - device creation (from_device_csr, deterministic=1) of the plan of A and of the plan of A^T (the flag), median of 3, and the transposer alone (tilespmv_csr_transpose_device)
  - the peak of device memory in use during each creation (hipMemGetInfo sampled every millisecond by a second thread, above what was in use before the call)
  - A x and A^T x (hipEvents, 5 x 50 timed launches each, alternated), and the rate each implies over B_alg (x and y swap sizes for A^T)
  - the paired refresh: SparseOperator(value_map=True).update_values (both plans from A's one value array) against the refresh of the plan of A alone
Every GPU step runs under a time limit of its own: past it the process reports and exits 124.

    python scripts/transpose_bench.py [--out profiles/r07_transpose.json] [--workloads laplacian4096,powerlaw8m,bandrand2m,rmat20x16,nlpkkt160,rect3m]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class limit:
    """Time limit of one GPU step: past it the process exits 124 (nothing is retried)."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def _expire(self):
        sys.stderr.write("transpose_bench: step '%s' exceeded %d s — giving up (exit 124)\n" % (self.name, self.seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expire)
        self.timer.daemon = True
        self.timer.start()
        return self

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


class peak_memory:
    """Peak of device memory in use (hipMemGetInfo, every ~1 ms) during the block, minus what was in use at its start."""

    def __init__(self, torch):
        self.torch, self.peak, self.stop = torch, 0, threading.Event()

    def _used(self):
        free, total = self.torch.cuda.mem_get_info()
        return total - free

    def _poll(self):
        while not self.stop.is_set():
            self.peak = max(self.peak, self._used() - self.base)
            time.sleep(0.001)

    def __enter__(self):
        self.base = self._used()
        self.thread = threading.Thread(target=self._poll, daemon=True)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak = max(self.peak, self._used() - self.base)
        return False


def matrix(name):
    from tilespmv_amd import generators as G
    if name == "laplacian4096":
        return G.laplacian5pt(4096) + (np.float64, "config 4: 5-pt Laplacian 4096^2 (symmetric)")
    if name == "powerlaw8m":
        return G.powerlaw(8000000, seed=2) + (np.float64, "power-law 8 M rows")
    if name == "bandrand2m":
        return G.band_plus_random(2000000, 4, 3, 5) + (np.float64, "band hbw=4 + 3 random per row, 2 M rows")
    if name == "rmat20x16":
        return G.rmat(20, 16, 3) + (np.float64, "R-MAT scale 20, 16 edges per vertex")
    if name == "nlpkkt160":
        return G.nlpkkt_like(160) + (np.float32, "KKT stand-in for nlpkkt160")
    if name == "rect3m":
        return G.uniform_per_row(3000000, 1000003, 6, 21) + (np.float64, "rectangular 3 M x 1 M, 6 uniform random per row")
    raise SystemExit("unknown workload " + name)


def events_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed_build(torch, fn):
    torch.cuda.synchronize()
    with peak_memory(torch) as pm:
        t0 = time.perf_counter()
        p = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return p, ms, pm.peak


def one(torch, name):
    from tilespmv_amd import api, generators as G
    from tilespmv_amd.operator import SparseOperator
    m, n, rp, ci, dtype, what = matrix(name)
    rp = np.ascontiguousarray(rp, np.int32)
    nnz = int(rp[m])
    ci = np.ascontiguousarray(ci[:nnz], np.int32)
    sv = np.dtype(dtype).itemsize
    v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
    rec = {"workload": name, "what": what, "dtype": np.dtype(dtype).name, "rows": m, "cols": n, "nnz": nnz}
    with limit(name + ": upload", 300):
        drp, dci, dv1, dv2 = (torch.from_numpy(a).cuda() for a in (rp, ci, v1, v2))
        x = torch.from_numpy(G.real_x(n, nnz, dtype)).cuda()
        u = torch.from_numpy(G.real_x(m, nnz, dtype)).cuda()
        y = torch.zeros(m + 16, dtype=x.dtype, device="cuda")
        z = torch.zeros(n + 16, dtype=x.dtype, device="cuda")
        torch.cuda.synchronize()
    opts = dict(deterministic=1)
    create = lambda transpose: api.Plan.from_device_csr(m, n, nnz, drp.data_ptr(), dci.data_ptr(), dv1.data_ptr(), dtype, transpose=transpose, **opts)  # noqa: E731
    for key, transpose in (("plain", False), ("transposed", True)):
        ms, peaks = [], []
        for k in range(3):
            with limit("%s: create %s %d" % (name, key, k), 600):
                p, t, pk = timed_build(torch, lambda: create(transpose))
            ms.append(t); peaks.append(pk)
            if k < 2:
                p.close()
        rec["create_ms_" + key] = float(np.median(ms))
        rec["create_peak_bytes_" + key] = int(max(peaks))
        rec["device_bytes_" + key] = p.info()["device_bytes"]
        if transpose:
            pT = p
        else:
            pA = p
    rec["flag_cost_ms"] = rec["create_ms_transposed"] - rec["create_ms_plain"]
    rec["flag_cost_over_plain_create"] = rec["flag_cost_ms"] / rec["create_ms_plain"]
    with limit(name + ": transposer alone", 300):
        drpT = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        dciT = torch.empty(max(nnz, 1), dtype=torch.int32, device="cuda")
        dvT = torch.empty(max(nnz, 1), dtype=dv1.dtype, device="cuda")
        tt = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.csr_transpose_device(m, n, drp.data_ptr(), dci.data_ptr(), dv1.data_ptr(), drpT.data_ptr(), dciT.data_ptr(), dvT.data_ptr(), dtype=dtype)
            tt.append((time.perf_counter() - t0) * 1e3)
        rec["transposer_ms"] = float(np.median(tt))
        del drpT, dciT, dvT
    stream = torch.cuda.current_stream().cuda_stream
    with limit(name + ": A x / A^T x", 300):
        ta, tt = [], []
        for _ in range(5):
            ta.append(pA.time(x.data_ptr(), y.data_ptr(), stream, warmup=10, reps=50))
            tt.append(pT.time(u.data_ptr(), z.data_ptr(), stream, warmup=10, reps=50))
    rec["spmv_ms_A"], rec["spmv_ms_AT"] = float(np.median(ta)), float(np.median(tt))
    rec["AT_over_A"] = rec["spmv_ms_AT"] / rec["spmv_ms_A"]
    rec["B_alg_A"], rec["B_alg_AT"] = api.algorithmic_bytes(nnz, m, n, sv), api.algorithmic_bytes(nnz, n, m, sv)
    rec["rate_TBps_A"] = rec["B_alg_A"] / (rec["spmv_ms_A"] * 1e-3) / 1e12
    rec["rate_TBps_AT"] = rec["B_alg_AT"] / (rec["spmv_ms_AT"] * 1e-3) / 1e12
    info_A, info_T = pA.info(), pT.info()
    for k in ("entry_mode", "csr_form", "num_split_rows", "dense_mode", "x_panels"):
        rec["facts_A_" + k], rec["facts_AT_" + k] = info_A[k], info_T[k]
    pA.close(); pT.close()
    with limit(name + ": paired refresh", 900):
        op = SparseOperator.from_device_csr(m, n, nnz, drp.data_ptr(), dci.data_ptr(), dv1.data_ptr(), dtype, value_map=True, **opts)
        flip, state = [dv2, dv1], {"i": 0}

        def both():
            state["i"] ^= 1
            op.update_values(flip[state["i"]], stream)

        def a_only():
            state["i"] ^= 1
            op.A.update_values(flip[state["i"]].data_ptr(), stream)
        rec["refresh_ms_both"] = events_ms(torch, both, 10, 100)
        rec["refresh_ms_A_only"] = events_ms(torch, a_only, 10, 100)
        rec["value_map_bytes_A"], rec["value_map_bytes_AT"] = op.A.info()["value_map_bytes"], op.AT.info()["value_map_bytes"]
        op.close()
        torch.cuda.synchronize()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_transpose.json"))
    ap.add_argument("--workloads", default="laplacian4096,powerlaw8m,bandrand2m,rmat20x16,nlpkkt160,rect3m")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {"what": "plans of A^T built on the device from A's CSR (TILESPMV_CREATE_TRANSPOSE): creation cost, transposer alone, A^T x against A x, peak device memory during "
                   "creation, the paired value refresh", "runs": []}
    for name in args.workloads.split(","):
        r = one(torch, name)
        print(json.dumps(r), flush=True)
        out["runs"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
