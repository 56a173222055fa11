"""bench.py keeps the driver's contract: one JSON line with the required keys; the N>1 path runs end to end
(rehearsed with two ranks sharing the one GPU over gloo — RCCL needs one GPU per rank)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


LINE_LIMIT = 4096   # the driver parses the LAST stdout line; round 5's 30 KB line was not parsed (BENCH_r05.parsed = null)


def _last_json(out):
    """What the driver does: the last stdout line is the record.  It must be the only `{` line, short, and valid JSON."""
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    assert out.rstrip("\n").splitlines()[-1] == lines[0]
    assert len(lines[0]) < LINE_LIMIT, len(lines[0])
    return json.loads(lines[0])


def _full(line):
    """The complete record the line points to (`full`): plan parameters, preparation seconds, per-workload detail."""
    path = line["full"] if os.path.isabs(line["full"]) else os.path.join(ROOT, line["full"])
    with open(path) as f:
        return json.load(f)


def test_headline_command_line_is_short_and_complete(tmp_path):
    """The driver's own command with --full (`python bench.py --gpus 1 --steps 20 --warmup 5 --full`: headline workload, every extra, population, CPU baseline) prints ONE line under 4 KB
    that carries the contract keys, `roofline` and `cpu_baseline`; everything else sits in the sidecar."""
    full = str(tmp_path / "full.json")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--full-json", full], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in d, k
    assert d["config"]["workload"] == "laplacian4096" and d["steps"] == 20 and d["warmup"] == 5 and d["check"].startswith("pass")
    assert abs(d["value"] - 2 * d["config"]["nnz"] / (d["ms_per_step"] * 1e-3) * 1e-9) / d["value"] < 0.02          # value IS the asked protocol
    rf, cb = d["roofline"], d["cpu_baseline"]
    assert rf["bound"] == "hbm" and rf["kernel_ms"] <= d["ms_per_step"] * 1.02 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert cb["kind"] == "reference" and cb["cores"] == 1 and cb["value"] > 0 and cb["all_host_cores"]["cores"] >= 1
    assert d["steady_state"]["setup_launches"] == 200 and d["steady_state"]["value"] > 0
    assert len(d["other_workloads"]) >= 10 and all(v != "error" and v[2] == "pass" for v in d["other_workloads"].values()), d["other_workloads"]
    assert d["population"]["this_run"]["count"] >= 10
    f = _full(d)
    assert f["value"] == d["value"] and set(f["other_workloads"]) == set(d["other_workloads"]) and "prep_seconds_per_rank" in f


def test_single_gpu_line():
    r = subprocess.run([sys.executable, "bench.py", "--workload", "laplacian512", "--steps", "10", "--warmup", "3", "--full"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in line, k
    assert line["roofline"]["bound"] == "hbm" and line["cpu_baseline"]["cores"] == 1 and line["value"] > 0
    d = _full(line)
    assert d["value"] == line["value"] and d["ms_per_step"] == line["ms_per_step"]
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3 and d["check"].startswith("pass: whole row block")
    assert d["config"]["workload"] == "laplacian512" and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] == 1 and cb["value"] > 0
    assert cb["sample"].startswith("the full workload") and cb["format_loop_only"]["serial_1_core"]["errcount"] == 0
    assert d["ranks"] == 1 and d["devices"] == [0] and d["reference_style_timing"]["ms_per_spmv"] > 0 and d["steady_state"]["setup_launches"] == 200
    assert {"tile_create", "plan_build", "plan_upload"} <= set(d["prep_seconds"]) and len(d["prep_seconds_per_rank"]) == 1
    assert d["steady_state"]["value"] > 0 and d["steady_state"]["ms_per_step"] > 0      # beside the headline (which is the plain W + K protocol)
    assert len(d["rank_devices"]) == 1 and d["rank_devices"][0]["device"] == 0 and "timed steps" in d["phase_seconds"]
    assert d["config"]["generated"] == "own row block only"
    allc = cb["format_loop_only"]["all_host_cores"]
    assert allc["threads"] == allc["usable_cores"] >= 1 and allc["y_equals_csr_golden"] is True
    assert "C loop" in d["reference_style_timing"]["protocol"]
    fp = rf["plan_fingerprint"]
    assert fp["num_tasks"] == d["config"]["tasks"] and (rf["traffic"] is None or rf["traffic_source"]["plan_fingerprint_matches"])
    assert abs(d["value"] - 2 * d["config"]["nnz"] / (d["ms_per_step"] * 1e-3) * 1e-9) / d["value"] < 0.02


def test_single_gpu_line_real_valued_data(tmp_path):
    """--data real: U(-1, 1) values and x (seed 12345), whole-y tolerance check; --cache: the second run reads the Tile_matrix cache."""
    cmd = [sys.executable, "bench.py", "--workload", "laplacian512", "--steps", "10", "--warmup", "3", "--data", "real", "--full", "--no-cpu-baseline",
           "--no-extras", "--cache", str(tmp_path)]
    lines = []
    for _ in range(2):
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_full(_last_json(r.stdout)))
    assert "U(-1,1)" in lines[0]["data"] and "<=" in lines[0]["check"] and lines[0]["check"].startswith("pass")
    assert lines[0]["prep_seconds"]["tile_cache"] == "miss" and lines[1]["prep_seconds"]["tile_cache"] == "hit"
    assert lines[1]["check"].startswith("pass")
    # the cache is tied to its input: with another digest beside it (= same shape, other values / flags / generator) it is not used
    keys = [f for f in os.listdir(tmp_path) if f.endswith(".key")]
    assert len(keys) == 1
    with open(os.path.join(tmp_path, keys[0]), "w") as f:
        f.write("0" * 32 + "\n")
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    third = _full(_last_json(r.stdout))
    assert third["prep_seconds"]["tile_cache"] == "miss" and third["check"].startswith("pass")


def test_two_rank_rehearsal_over_gloo():
    # the driver's command shape, bare: bench.py starts its own ranks (child torch.distributed.run) and relays the line
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "10", "--warmup", "3", "--backend", "gloo", "--workload", "laplacian512", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and len(line["rank_devices"]) == 2 and len(line["per_rank_kernel_ms"]) == 2
    assert set(line["with_y_combine"]) == {"allgather", "allreduce", "halo"} and all(v["check"] == "pass" for v in line["with_y_combine"].values()), line
    d = _full(line)
    assert d["n_gpus"] == 2 and d["check"].startswith("pass") and d["scaling"] == "strong"
    assert d["ranks"] == 2 and len(d["devices"]) == 2 and d["backend"] == "gloo" and d["launched_by"].startswith("self")
    assert len(d["per_rank_ms_per_step"]["wall"]) == 2 and d["per_rank_ms_per_step"]["max"] >= d["per_rank_ms_per_step"]["min"] > 0
    assert set(d["with_y_combine"]) == {"allgather", "allreduce", "halo"} and d["cpu_baseline"] is None
    assert all(v["check_full_y_on_every_rank"] == "pass" for k, v in d["with_y_combine"].items() if k != "halo"), d["with_y_combine"]
    assert d["with_y_combine"]["halo"]["check_own_rows_on_every_rank"] == "pass" and d["with_y_combine"]["halo"]["halo_bytes_per_rank"] > 0
    assert len(d["prep_seconds_per_rank"]) == 2 and d["config"]["generated"] == "own row block only"      # each rank built only its rows


def test_two_rank_halo_mode_over_gloo():
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2", "--backend", "gloo", "--workload", "laplacian512", "--combine", "halo",
           "--data", "real", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _full(_last_json(r.stdout))
    assert d["config"]["y_combine"] == "halo" and d["halo_bytes_per_rank"] > 0 and d["check"].startswith("pass") and d["value"] > 0


def test_one_rank_through_the_launcher_equals_the_bare_run(tmp_path):
    """The SCALE N = 1 point (driver: `python -m torch.distributed.run --nproc-per-node 1 ... bench.py --gpus 1`) must agree with BENCH (`python bench.py`):
    same code path (no process group at world size 1), same line, same value within run-to-run noise."""
    args = ["--gpus", "1", "--steps", "100", "--warmup", "10", "--workload", "laplacian2048", "--full", "--no-cpu-baseline", "--no-extras"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    bare = subprocess.run([sys.executable, "bench.py"] + args + ["--full-json", str(tmp_path / "bare.json")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert bare.returncode == 0, bare.stderr[-2000:]
    import socket
    with socket.socket() as so:      # a free port for the rendezvous (a fixed one may still be in TIME_WAIT from an earlier run)
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    launched = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
                               "bench.py"] + args + ["--full-json", str(tmp_path / "launched.json")], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert launched.returncode == 0, launched.stderr[-2000:]
    a, b = _full(_last_json(bare.stdout)), _full(_last_json(launched.stdout))
    assert a["n_gpus"] == b["n_gpus"] == 1 and a["ranks"] == b["ranks"] == 1 and a["config"] == b["config"]
    assert a["launched_by"] == "direct" and b["launched_by"] == "direct" and b["backend"] is None      # world size 1: no process group either way
    assert a["check"] == b["check"] and a["check"].startswith("pass")
    # the kernel's own time (HIP events on the launch stream) agrees closely; `value` is wall clock around a region of a few milliseconds and may catch a host hiccup
    ka, kb = a["roofline"]["kernel_ms"], b["roofline"]["kernel_ms"]
    assert abs(ka - kb) / ka < 0.15, (ka, kb)
    assert 0.5 < a["value"] / b["value"] < 2.0, (a["value"], b["value"])
    assert a["roofline"]["plan_fingerprint"] == b["roofline"]["plan_fingerprint"]


def test_four_rank_rehearsal_over_gloo():
    """More than two ranks through the driver's command shape, all on device 0 over gloo (the GPU box lets 6 processes of one job use its card at once: this test process +
    4 ranks stay below that; scripts/archive/rounds/r4_rehearsal.sh runs 6 ranks bare): the plumbing of an 8-rank run — per-rank generation and preprocessing with a share of the host cores
    each, the three y combines with the neighbours' rows checked, max-over-ranks timing — before there is an 8-GPU node."""
    cmd = [sys.executable, "bench.py", "--gpus", "4", "--steps", "10", "--warmup", "3", "--backend", "gloo", "--workload", "laplacian1024", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _last_json(r.stdout)          # (< 4 KB with four ranks' devices, kernel times and the three combines in it)
    assert line["ranks"] == 4 and [r_["device"] for r_ in line["rank_devices"]] == [0] * 4 and len({r_["uuid"] for r_ in line["rank_devices"]}) == 1
    assert len(line["per_rank_kernel_ms"]) == 4 and all(v["check"] == "pass" for v in line["with_y_combine"].values()), line
    d = _full(line)
    assert d["n_gpus"] == 4 and d["ranks"] == 4 and d["devices"] == [0] * 4 and d["check"].startswith("pass")
    assert len(d["prep_seconds_per_rank"]) == 4 and len(d["per_rank_ms_per_step"]["wall"]) == 4
    assert all(v["check_full_y_on_every_rank"] == "pass" for k, v in d["with_y_combine"].items() if k != "halo"), d["with_y_combine"]
    assert d["with_y_combine"]["halo"]["check_own_rows_on_every_rank"] == "pass"
    assert 1 <= d["host_threads_per_rank"] <= 16


def _csr_rows_compat(rp, ci, pick):
    """y at rows `pick` of A x on the reference driver's data (val[k] = k % 10, x[j] = j % 10), from the CSR arrays alone: exact in float64."""
    import numpy as np
    lens = (rp[pick + 1] - rp[pick]).astype(np.int64)
    first = np.cumsum(lens) - lens
    k = np.repeat(rp[pick].astype(np.int64), lens) + np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(first, lens)
    return np.add.reduceat(((k % 10) * (ci[k].astype(np.int64) % 10)).astype(np.float64), first)


def test_plain_run_is_the_headline_alone_and_dumps_y(tmp_path):
    """A plain run (no --full): set-up, W warm-ups, K timed steps, the line — no parity check, no side measurement.  --dump-outputs writes y of the
    last timed step; the same arguments give the same inputs, so two runs write the same y, and on the reference driver's data it is the CSR product exactly."""
    import numpy as np
    from tilespmv_amd import generators as G
    ys = []
    for rep in range(2):
        out = tmp_path / ("out%d" % rep)
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", "laplacian512", "--dump-outputs", str(out),
                            "--full-json", str(tmp_path / "full.json")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = _last_json(r.stdout)
        for k in REQUIRED:
            assert k in line, k
        assert line["steps"] == 7 and line["warmup"] == 2 and line["run"] == "plain" and line["check"] == "skipped"
        assert line["cpu_baseline"] is None and line["reference_style_ms"] is None and "steady_state" not in line and "other_workloads" not in line
        assert abs(line["value"] - 2 * line["config"]["nnz"] / (line["ms_per_step"] * 1e-3) * 1e-9) / line["value"] < 0.02
        f = _full(line)
        assert f["device_state_under_load"] is None and "measured_ceilings_gbps" not in f["roofline"] and "other_path" not in f["prep_seconds"]
        assert f["prep_seconds"]["process_warm_up_seconds"] is None and set(f["phase_seconds"]) == {"prepare (Tile_create + plan)", "parity check", "timed steps", "dump outputs"}
        assert os.listdir(out) == ["y.npy"]
        ys.append(np.load(out / "y.npy"))
    m, n, rp, ci = G.laplacian5pt(512)
    rows = (m // 16) * 16
    assert ys[0].dtype == np.float64 and ys[0].shape == (rows,)
    assert np.array_equal(ys[0], _csr_rows_compat(rp, ci, np.arange(rows))) and np.array_equal(ys[0], ys[1])


def test_plain_headline_run_is_lean_and_dumps_a_fixed_sample(tmp_path):
    """The benchmark's own command, plain, with --dump-outputs: at most 30 s outside its W + K steps, from start to exit; y of the headline (134 MB)
    is written as the fixed seeded sample of bench.dump_rows (< 64 MB), equal to the CSR product at those rows."""
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from tilespmv_amd import generators as G
    out = tmp_path / "out"
    t0 = time.time()
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out), "--full-json", str(tmp_path / "full.json")],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    line = _last_json(r.stdout)
    assert line["config"]["workload"] == "laplacian4096" and line["steps"] == 20 and line["run"] == "plain"
    assert wall - 25 * line["ms_per_step"] * 1e-3 <= 30.0, wall
    assert os.listdir(out) == ["y_sample.npy"] and os.path.getsize(out / "y_sample.npy") <= 64 << 20
    y = np.load(out / "y_sample.npy")
    m, n, rp, ci = G.laplacian5pt(4096)
    pick = bench.dump_rows(line["config"]["rows"], 8)
    assert y.dtype == np.float64 and y.shape == pick.shape
    assert np.array_equal(y, _csr_rows_compat(rp, ci, pick))


def test_two_rank_dump_holds_every_ranks_rows(tmp_path):
    """--dump-outputs with two ranks (over gloo on the one GPU): rank 0 writes the whole y, every rank's block in row order — with y left sharded and with the halo form."""
    import numpy as np
    from tilespmv_amd import generators as G
    m, n, rp, ci = G.laplacian5pt(512)
    want = _csr_rows_compat(rp, ci, np.arange((m // 16) * 16))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for combine in ("none", "halo"):
        out = tmp_path / combine
        cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "4", "--warmup", "1", "--backend", "gloo", "--workload", "laplacian512", "--combine", combine,
               "--dump-outputs", str(out), "--full-json", str(tmp_path / "full.json")]
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        line = _last_json(r.stdout)
        assert line["ranks"] == 2 and line["steps"] == 4 and "with_y_combine" not in line
        assert np.array_equal(np.load(out / "y.npy"), want), combine
