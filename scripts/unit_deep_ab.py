"""A/B of the deep unit kernel (TILESPMV_UNIT_DEEP, csrc/hip_kernels_deep.hip) against the lean launch of the same library and the parent commit's library in ONE process (the
protocol of profiles/strip_sweep_ab.txt; record: profiles/unit_deep_ab.txt):
    python scripts/unit_deep_ab.py <workload> [f64|f32] [real] [knob=value ...]
The matrix is tiled once; plans of the parent commit's library ("parent": tilespmv_amd/lib/*_old.so, scripts/ab_prev.sh build), of this library with the knob at 0 ("off") and
at 1 ("deep") are created from it, each at TWO positions of the sequence (where a plan's streams land in memory moves a workload by a few per cent).  knob=value pairs — value_narrow=1 — go to every plan; `real`: U(-1, 1) values and x instead of the compat data.  Every plan runs once and its
whole y is compared bit for bit with the first plan's; then 5 rounds, each timing every plan once with tilespmv_plan_time (events around 200 launches after 20 warm-up
launches).  Printed per plan: median of the rounds and max - min of rounds 2-5 (the first round of the first plan carries the clock ramp); then, per pairing of positions, the
difference deep - parent and deep - off, which counts where it holds for both pairings and exceeds three times the larger spread."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (opens the device before the library does)

from tilespmv_amd import _lib, api, generators as G  # noqa: E402


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "laplacian4096"
    dtype = np.float32 if (sys.argv[2] if len(sys.argv) > 2 else "f64") == "f32" else np.float64
    real = "real" in sys.argv[3:]
    knobs = {k: int(v) for k, v in (a.split("=") for a in sys.argv[3:] if "=" in a)}
    argv, sys.argv = sys.argv, sys.argv[:1]
    import bench
    sys.argv = argv
    m, n, rp, ci, src = bench.build_matrix(wl)
    rows = (m // 16) * 16; nnz = int(rp[rows])
    vals, x = (G.real_values(len(ci), dtype), G.real_x(n, len(ci), dtype)) if real else (G.compat_values(len(ci), dtype), G.compat_x(n, dtype))
    tm = api.Tile_create(rows, n, nnz, rp, ci, vals, dtype=dtype)
    xd = torch.from_numpy(x).cuda(); yd = torch.zeros(rows + 16, dtype=xd.dtype, device="cuda")
    order = ["parent", "off", "deep"] * 2
    base_lib = tm._lib
    plans, y0 = [], None
    for pos, v in enumerate(order):
        if v == "parent":
            os.environ["TILESPMV_LIB_VARIANT"] = "_old"; _lib._CACHE.pop(np.dtype(dtype), None)
            tm._lib = _lib.load(dtype)
            os.environ.pop("TILESPMV_LIB_VARIANT"); _lib._CACHE[np.dtype(dtype)] = base_lib
        else:
            os.environ["TILESPMV_UNIT_DEEP"] = "0" if v == "off" else "1"
        p = api.Plan(tm, rows, n, nnz, **knobs)
        os.environ.pop("TILESPMV_UNIT_DEEP", None)
        tm._lib = base_lib
        yd.fill_(-1); p.spmv(xd.data_ptr(), yd.data_ptr()); torch.cuda.synchronize()
        y = yd.cpu().numpy()[:rows].copy()
        y0 = y if y0 is None else y0
        plans.append((v, pos, p, bool(np.array_equal(y, y0))))
    t = {pos: [] for _, pos, _, _ in plans}
    for _ in range(5):
        for v, pos, p, _ in plans:
            t[pos].append(p.time(xd.data_ptr(), yd.data_ptr(), warmup=20, reps=200))
    print("== %s %s %s %s(%s): %d rows, %d nnz" % (wl, np.dtype(dtype).name, "real" if real else "compat", "".join("%s=%d " % kv for kv in knobs.items()), src, rows, nnz))
    med, spread = {}, {}
    for v, pos, p, same in plans:
        a = np.array(t[pos]); i = p.info()
        med[pos], spread[pos] = float(np.median(a)), float(a[1:].max() - a[1:].min())
        print("  #%d %-12s y==#0 %-5s median %.5f ms  spread %.5f  rounds %s  deep %s  stride %s  form %s  value bytes %d  desc bytes %d  list entries %d  stream_bytes %d" % (
            pos, v, same, med[pos], spread[pos], " ".join("%.5f" % q for q in a), "-" if v == "parent" else p.unit_deep(), "-" if v == "parent" else p.strip_stride(),
            i["unit_lean"], i["unit_value_bytes"], i["desc_bytes"], i["list_entries"], i["stream_bytes"]), flush=True)
    for ref in ("parent", "off"):
        gs = [pos for v, pos, _, _ in plans if v == ref]
        ls = [pos for v, pos, _, _ in plans if v == "deep"]
        for g, l in zip(gs, ls):
            d, s3 = med[l] - med[g], 3 * max(spread[g], spread[l])
            print("  deep #%d - %s #%d: %+.5f ms (%+.2f %%), 3 x larger spread %.5f -> %s" % (l, ref, g, d, 100 * d / med[g], s3, "counts" if abs(d) > s3 else "inside the noise"))


main()
