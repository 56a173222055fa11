#!/usr/bin/env python3
"""What a value refresh costs against a rebuild (TILESPMV_CREATE_VALUE_MAP, Plan.update_values), on config 4 (fp64), fem3_68 (fp64) and the nlpkkt160 stand-in (fp32).

Per workload, in one process: the refresh time (hipEvents, warmed, 100 back-to-back refreshes), the bytes one refresh must move (index map + new stream values + one read of the CSR
values) and the rate they imply; the rebuild a solver would otherwise pay (from_device_csr with deterministic=1, values already on the device, median of 3); the SpMV time of the flagged
and the unflagged plan (same options: deterministic=1), alternated in the same process.  Every GPU step runs under a time limit of its own: past it the process reports and exits 124.

    python scripts/update_values_bench.py [--out profiles/r07_update_values.json] [--workloads laplacian4096,fem3_68,nlpkkt160]
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
        sys.stderr.write("update_values_bench: step '%s' exceeded %d s — giving up (exit 124)\n" % (self.name, self.seconds))
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


def matrix(name):
    from tilespmv_amd import generators as G
    if name == "laplacian4096":
        return G.laplacian5pt(4096) + (np.float64,)
    if name == "fem3_68":
        return G.fem_hex(68, 68, 68, 3) + (np.float64,)
    if name == "nlpkkt160":
        return G.nlpkkt_like(160) + (np.float32,)
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


def one(torch, name):
    from tilespmv_amd import api, generators as G
    m, n, rp, ci, dtype = matrix(name)
    rows = (m // 16) * 16
    rp = np.ascontiguousarray(rp[:rows + 1], np.int32)
    nnz = int(rp[rows])
    ci = np.ascontiguousarray(ci[:nnz], np.int32)
    sv = np.dtype(dtype).itemsize
    v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
    x = G.real_x(n, nnz, dtype)
    rec = {"workload": name, "dtype": np.dtype(dtype).name, "rows": rows, "cols": n, "nnz": nnz}
    with limit(name + ": upload", 300):
        drp, dci, dv1, dv2 = (torch.from_numpy(a).cuda() for a in (rp, ci, v1, v2))
        xd = torch.from_numpy(x).cuda()
        yd = torch.zeros(rows + 16, dtype=xd.dtype, device="cuda")
        torch.cuda.synchronize()
    opts = dict(deterministic=1)
    with limit(name + ": flagged plan", 600):
        f = api.Plan.from_device_csr(rows, n, nnz, drp.data_ptr(), dci.data_ptr(), dv1.data_ptr(), dtype, value_map=True, **opts)
        torch.cuda.synchronize()
    info = f.info()
    vmb = info["value_map_bytes"]
    slots = vmb // 4
    rec["value_map_bytes"] = vmb
    rec["device_bytes"] = info["device_bytes"]
    rec["refresh_bytes"] = vmb + slots * sv + nnz * sv   # map + new stream values + one read of the CSR values (entry records: value words only, counted whole)
    stream = torch.cuda.current_stream().cuda_stream
    with limit(name + ": refresh", 300):
        flip = [dv2, dv1]
        state = {"i": 0}

        def refresh():
            state["i"] ^= 1
            f.update_values(flip[state["i"]].data_ptr(), stream)
        rec["refresh_ms"] = events_ms(torch, refresh, 10, 100)
        if state["i"] == 1:   # (leave the plan holding v1 for the SpMV timings)
            refresh()
        torch.cuda.synchronize()
    rec["refresh_TBps"] = rec["refresh_bytes"] / (rec["refresh_ms"] * 1e-3) / 1e12
    builds = []
    for k in range(3):
        with limit(name + ": rebuild %d" % k, 600):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = api.Plan.from_device_csr(rows, n, nnz, drp.data_ptr(), dci.data_ptr(), dv2.data_ptr(), dtype, **opts)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
            if k < 2:
                p.close()
    rec["rebuild_ms"] = float(np.median(builds))
    rec["rebuild_over_refresh"] = rec["rebuild_ms"] / rec["refresh_ms"]
    with limit(name + ": spmv flagged / unflagged", 300):
        tf, tu = [], []
        for _ in range(5):
            tf.append(f.time(xd.data_ptr(), yd.data_ptr(), stream, warmup=10, reps=50))
            tu.append(p.time(xd.data_ptr(), yd.data_ptr(), stream, warmup=10, reps=50))
    rec["spmv_ms_flagged"], rec["spmv_ms_unflagged"] = float(np.median(tf)), float(np.median(tu))
    rec["spmv_flagged_over_unflagged"] = rec["spmv_ms_flagged"] / rec["spmv_ms_unflagged"]
    f.close(); p.close()
    rec["targets"] = {"refresh_le_0.5ms (config 4)": rec["refresh_ms"] <= 0.5 if name == "laplacian4096" else None, "rebuild_ge_100x": rec["rebuild_over_refresh"] >= 100,
                      "rate_ge_4TBps": rec["refresh_TBps"] >= 4.0, "flagged_spmv_within_2pct": rec["spmv_flagged_over_unflagged"] <= 1.02}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_update_values.json"))
    ap.add_argument("--workloads", default="laplacian4096,fem3_68,nlpkkt160")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {"what": "value refresh (Plan.update_values) against a rebuild (from_device_csr, deterministic=1) and the SpMV of flagged / unflagged plans", "runs": []}
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
