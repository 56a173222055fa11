"""Layout digests of the plans that reach every outcome of the builder's ENCODE stage (csrc/hip_plan_stream.hip): per case the layout digest, the eight stage
digests and the plan facts, from host-only builds (api.plan_layout_digest / plan_layout_stages: no GPU).  Run it with two libraries and diff the outputs to show that
a change of the builder kept every stream of every plan:

    python scripts/encode_digests.py > new.txt;  TILESPMV_LIB_VARIANT=_old python scripts/encode_digests.py > old.txt;  diff old.txt new.txt

(TILESPMV_LIB_VARIANT: scripts/ab_prev.sh build <commit>.)  The last lines say which descriptor forms the list reached; the script fails if one is missing.
--device: the plans of tests/test_gpu_device_build.py::test_device_built_plan_classes_and_shards created on the GPU in host and in device mode with placement_tries=1;
their streams in upload order (member offset, bytes, digest) and their facts — the same text from two libraries = the same streams at the same places in the arena.
--brief FILE: a saved output condensed to one short line per case (what profiles/encode_once_digests.txt keeps)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from tilespmv_amd import api, generators as G  # noqa: E402

FACTS = ["desc_bytes", "csr_form", "unit_value_bytes", "unit_lean", "device_bytes", "stream_bytes", "num_tasks", "num_split_rows", "list_entries", "derived_units", "entry_mode", "wg_strips",
         "brick_order", "nt_stream", "x_panels"]
# The smallest cases found at which a dictionary is tried and given up because the shard has more than 2^DICT_MAX_BITS = 1024 patterns:
#   pooled:  fem_hex(5, 5, 5, 3, shuffle=16) (368 rows; 5 x 5 x 4 nodes keep their dictionary and get 4-byte words)
#   classic: random_uniform(736, 736, 0.08, seed 3) under desc_dict=1 (45 tile-rows of units with random nibbles; 704 x 704 gets 4-byte words)
OVER_POOLED = ("fem_hex(5,5,5,3,shuffle=16)", lambda: G.fem_hex(5, 5, 5, 3, shuffle=16))
OVER_CLASSIC = ("random_uniform(736,736,0.08)", lambda: G.random_uniform(736, 736, 0.08, 3))


def shuffled(gen, window=64, seed=21):
    """The matrix under a symmetric permutation that moves rows at random inside windows of `window` consecutive rows."""
    m, n, rp, ci = gen
    new = G._fem_node_order(m, window, seed)
    ri = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    return G.from_coo(m, n, new[ri], new[np.asarray(ci, dtype=np.int64)])


def matrices():
    yield "laplacian7pt(48)", G.laplacian7pt(48), False
    yield "powerlaw(60000)", G.powerlaw(60000, seed=2), False
    yield "all_formats(12,7)+hyb", G.all_formats(12, 7), True
    yield "band_plus_random(40000,4,3,5)", G.band_plus_random(40000, 4, 3, 5), False
    yield "band(30000,40)", G.band(30000, 40), False
    yield "kkt_like(12)", G.kkt_like(12), False
    yield "kkt_like(12) shuffled", shuffled(G.kkt_like(12)), False
    yield "fem_hex(12,12,12,3)", G.fem_hex(12, 12, 12, 3), False
    yield "fem_hex(12,12,12,3,shuffle=16)", G.fem_hex(12, 12, 12, 3, shuffle=16), False
    yield "fem_hex(16,16,16,3,shuffle=64)", G.fem_hex(16, 16, 16, 3, shuffle=64), False
    yield OVER_POOLED[0], OVER_POOLED[1](), False
    yield OVER_CLASSIC[0], OVER_CLASSIC[1](), False


KNOBS = ([dict()] + [dict(desc_dict=d) for d in (0, 1, 2)] + [dict(csr_split=c) for c in (2, 3)] + [dict(csr_split=2, desc_dict=d) for d in (0, 1, 2)] + [dict(csr_split=3, desc_dict=0)] +
         [dict(entry_mode=e) for e in (0, 1, 2)] + [dict(entry_mode=e, csr_split=2) for e in (0, 1, 2)] + [dict(x_window=2), dict(x_window=2, desc_dict=0)])


def line(name, dtype, kw, tm, rows, n, nnz, seen):
    d, _ = api.plan_layout_digest(tm, rows, n, nnz, **kw)
    st, i = api.plan_layout_stages(tm, rows, n, nnz, **kw)
    form = "%d%s" % (i["desc_bytes"], {4: " classic" if i["csr_form"] < 2 else " pooled"}.get(i["desc_bytes"], ""))
    dd = kw.get("desc_dict", -1)
    if i["csr_form"] == 2 and dd != 0 and i["desc_bytes"] == 20:
        form += " (pooled dictionary over)"
    if i["csr_form"] < 2 and dd == 1 and i["desc_bytes"] == 12:
        form += " (classic dictionary over)"
    seen.setdefault(form, "%s %s %s" % (name, np.dtype(dtype).name, kw))
    if i["unit_value_bytes"] < np.dtype(dtype).itemsize:
        seen.setdefault("values in %d bytes" % i["unit_value_bytes"], "%s %s" % (name, kw))
    print("%s | %s | %s | %016x | %s | %s" % (name, np.dtype(dtype).name, " ".join("%s=%d" % kv for kv in sorted(kw.items())) or "-", d, " ".join("%016x" % st[k] for k in api.STAGE_NAMES),
                                           " ".join("%s=%d" % (k, i[k]) for k in FACTS)))


def host_cases():
    seen = {}
    print("# matrix | dtype | knobs | layout digest | stage digests (%s) | facts" % " ".join(api.STAGE_NAMES))
    for name, gen, hyb in matrices():
        m, n, rp, ci = gen
        rows = cases.truncated_rows(m); nnz = int(rp[rows])
        for dtype in (np.float64, np.float32):
            tm = api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci), dtype), dtype=dtype, hyb=hyb)
            for kw in KNOBS:
                line(name, dtype, kw, tm, rows, n, nnz, seen)
            api.Tile_destroy(tm)
        if name in ("laplacian7pt(48)", "band_plus_random(40000,4,3,5)", "kkt_like(12)"):   # fp64, values that are all floats (not halves: 1 + 2^-20 among them) / all halves
            for what, vals in (("floats", G.compat_values(len(ci)) + 2.0 ** -20), ("halves", G.compat_values(len(ci)))):
                tm = api.Tile_create(rows, n, nnz, rp, ci, vals)
                for kw in (dict(value_narrow=1), dict(value_narrow=2), dict(value_narrow=2, desc_dict=0), dict(value_narrow=2, entry_mode=2)):
                    line("%s %s" % (name, what), np.float64, kw, tm, rows, n, nnz, seen)
                api.Tile_destroy(tm)
    print("# forms reached (first case of each):")
    for k in sorted(seen):
        print("#   %-40s %s" % (k, seen[k]))
    want = ["4 classic", "12", "20", "8", "4 pooled", "28", "20 (pooled dictionary over)", "12 (classic dictionary over)", "values in 4 bytes", "values in 2 bytes"]
    missing = [k for k in want if k not in seen]
    assert not missing, "no case reaches: %s" % missing


def device_cases():
    mats = {"fem3": G.fem_hex(14, 14, 14, 3), "fem6s": G.fem_hex(10, 10, 10, 6, shuffle=16), "fem3s64": G.fem_hex(16, 16, 16, 3, shuffle=64), "circuit": G.circuit_like(120000), "lap3d": G.laplacian7pt(48),
            "kkt24": G.kkt_like(24), "powerlaw": G.powerlaw(300000), "band40": G.band(60000, 40), "rmat16": G.rmat(16, 8, 3), "lap2d": G.laplacian5pt(500)}
    for name, (rows, cols, rp, ci) in mats.items():
        rows = cases.truncated_rows(rows); nnz = int(rp[rows]); tilem = rows // 16
        for dtype in (np.float64, np.float32):
            v = G.real_values(nnz, dtype)
            for kw in (dict(placement_tries=1), dict(placement_tries=1, deterministic=1, tilerow_begin=tilem // 3, tilerow_end=2 * tilem // 3)):
                tm = api.Tile_create(rows, cols, nnz, rp, ci, v, dtype=dtype)
                for mode, plan in (("host", api.Plan(tm, rows, cols, nnz, **kw)), ("device", api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, **kw))):
                    i = plan.info()
                    print("%s | %s | %s | %s | %s | %s" % (name, np.dtype(dtype).name, "shard" if "tilerow_end" in kw else "whole", mode,
                                                         " ".join("%d:%d:%016x" % (off, b, h) for off, (b, h) in plan.stream_digests().items()),
                                                         " ".join("%s=%d" % (k, i[k]) for k in sorted(i) if not k.endswith("_us"))))
                    plan.close()
                api.Tile_destroy(tm)


def brief(path):
    """A saved output condensed for a file that is kept: the SHA-256 of the whole output, then one line per matrix and dtype with an entry per case —
    knobs (or whole / shard, host / device), desc_bytes/csr_form/unit_value_bytes, and the first 8 hex digits of the SHA-256 of the rest of the case's line."""
    import hashlib
    text = open(path).read()
    print("# sha256 of the full output (%d lines): %s" % (text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    groups = {}
    for ln in text.splitlines():
        if ln.startswith("#"):
            if not ln.startswith("# matrix"):
                print(ln)
            continue
        f = ln.split(" | ")
        n = 4 if f[3] in ("host", "device") else 3
        facts = dict(kv.split("=") for kv in f[-1].split())
        groups.setdefault(" ".join(f[:2]), []).append("%s %s/%s/%s %s" % (" ".join(f[2:n]).replace(" ", ","), facts["desc_bytes"], facts["csr_form"], facts["unit_value_bytes"], hashlib.sha256(" | ".join(f[n:]).encode()).hexdigest()[:8]))
    for k, v in groups.items():
        print("%s: %s" % (k, "; ".join(v)))


if __name__ == "__main__":
    if "--brief" in sys.argv:
        brief(sys.argv[sys.argv.index("--brief") + 1])
    else:
        device_cases() if "--device" in sys.argv else host_cases()
