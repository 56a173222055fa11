"""The deep unit kernel (csrc/hip_kernels_deep.hip, environment knob TILESPMV_UNIT_DEEP), checked without a GPU.  From the device assembly of both builds: the 12 / 4
instantiations exist by name, none uses scratch, and the unit loop of the one the headline runs (dictionary descriptors, halves, derived units) — the loop around the
nontemporal value load — holds no `s_waitcnt vmcnt(0)`, and its first wait behind the loop's loads leaves at least one batch of loads (4 gathers + 1 value load) outstanding;
its VGPR count is printed and held to the bound its `__launch_bounds__` asks for (7 waves per SIMD: 72).  From the host layout builder: the 5-point 4096^2 compat plan
satisfies the predicate and keeps every plan fact and stage digest it has with the knob at 0; plans with list entries, split tile-rows, pooled units or the workgroup entry
mode do not satisfy it; the knob is the environment's, read in a child process."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases
from kernel_asm import ROOT, device_asm, private_segments
from tilespmv_amd import api, generators as G

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from loop_waits import NT_VALUE_LOAD, _blocks, unit_loops  # noqa: E402

UB, DEPTH = 4, 2                                     # hip_plan.h UNIT_DEEP_UB, UNIT_DEEP_DEPTH
HOT = "k_units_deep<4, 2, true, 2, true>"            # dictionary descriptors, halves, derived units: what the 5-point 4096^2 headline runs
HOT_MAX_VGPR = 72                                    # 7 waves per SIMD (512 / 7, in allocation units of 8), what the halves forms ask of the register allocator
BATCH_LOADS = UB + 1                                 # halves: 4 gathers and one 8-byte value load


@pytest.fixture(scope="module")
def deep_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("deep_asm")
    with ThreadPoolExecutor(2) as ex:
        return dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_kernels_deep.hip", dt, str(d / (dt + ".s"))), ("f64", "f32"))))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_kernels_exist_by_name_and_use_no_scratch(deep_asm, dt):
    asm = deep_asm[dt]
    spills = private_segments(asm)
    assert not any(spills.values()), {k: v for k, v in spills.items() if v}
    names = subprocess.run(["c++filt"] + list(spills), capture_output=True, text=True, check=True).stdout.split("\n")[:len(spills)]
    got = sorted(n.split("(")[0].replace("void tilespmv::", "") for n in names)
    forms = (0, 1, 2) if dt == "f64" else (0,)
    want = sorted("k_units_deep<%d, %d, %s, %d, %s>" % (UB, DEPTH, cd, vf, dv) for cd in ("true", "false") for vf in forms for dv in ("true", "false"))
    assert got == want, got
    assert len(want) == (12 if dt == "f64" else 4)


def test_unit_loop_of_the_hot_kernel_never_drains(deep_asm):
    rec = unit_loops(deep_asm["f64"], ("k_units_deep",), NT_VALUE_LOAD)[HOT]
    print(HOT, rec)
    assert rec["insns"] > 0 and rec["vmcnt"], rec                            # the loop around the nontemporal value load was found, and it waits for loads
    assert 0 not in rec["vmcnt"], rec["vmcnt"]
    assert rec["scratch"] == 0 and rec["vgpr"] <= HOT_MAX_VGPR, rec
    # ... and the first wait behind the first loads of the loop: everything issued in this iteration stays outstanding
    funcs = re.findall(r"^(_Z\w+):\s*; @\1\n(.*?)^\s+s_endpgm", deep_asm["f64"], re.S | re.M)
    dem = subprocess.run(["c++filt"] + [n for n, _ in funcs], capture_output=True, text=True, check=True).stdout.split("\n")
    body = [b for (_, b), d in zip(funcs, dem) if d.split("(")[0].replace("void tilespmv::", "") == HOT][0]
    value_load = re.compile(NT_VALUE_LOAD)
    loops = [h for _, h, insns in _blocks(body) if h is not None and any(value_load.match(op + a) for op, a in insns)]
    insns = [i for _, h, ins in _blocks(body) if h == loops[-1] for i in ins]
    first_load = next(k for k, (op, _) in enumerate(insns) if op.startswith("global_load"))
    waits = [int(v) for op, a in insns[first_load:] if op == "s_waitcnt" for v in re.findall(r"vmcnt\((\d+)\)", a)]
    print("first wait behind the loop's loads: vmcnt(%d)" % waits[0])
    assert waits[0] >= BATCH_LOADS, waits


def _headline():
    m, n, rp, ci = G.laplacian5pt(4096)
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    return api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci))), rows, n, nnz


def test_headline_plan_satisfies_the_predicate_and_stays_the_same_plan(monkeypatch):
    tm, rows, n, nnz = _headline()
    got = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("TILESPMV_UNIT_DEEP", knob)
        st, info = api.plan_layout_stages(tm, rows, n, nnz)
        got[knob] = (st, {k: v for k, v in info.items() if not k.endswith("_us")}, api.plan_layout_unit_deep(tm, rows, n, nnz))
    monkeypatch.delenv("TILESPMV_UNIT_DEEP")
    assert api.plan_layout_unit_deep(tm, rows, n, nnz) == DEPTH               # knob unset: nontemporal by size -> taken by rule
    assert api.plan_layout_unit_deep(tm, rows, n, nnz, value_narrow=1) == DEPTH   # ... as floats too
    assert got["0"][2] == 0 and got["1"][2] == DEPTH, (got["0"][2], got["1"][2])
    assert got["1"][0] == got["0"][0]                                         # every stage digest
    assert got["1"][1] == got["0"][1]                                         # every plan fact
    i = got["1"][1]
    assert (i["unit_lean"], i["unit_value_bytes"], i["desc_bytes"], i["nt_stream"], i["entry_mode"], i["wg_strips"], i["list_entries"], i["num_split_rows"]) == (1, 2, 4, 1, 0, 16, 0, 0), i
    api.Tile_destroy(tm)


def _tm(gen, dtype=np.float64):
    m, n, rp, ci = gen
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    return api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci), dtype), dtype=dtype), rows, n, nnz


def _grid5(nx, ny):
    idx = np.arange(nx * ny, dtype=np.int64)
    i, j = idx // nx, idx % nx
    cand = np.stack([idx - nx, idx - 1, idx, idx + 1, idx + nx], axis=1)
    mask = np.stack([i > 0, j > 0, np.ones(idx.size, bool), j < nx - 1, i < ny - 1], axis=1)
    rp, ci = G._from_mask(cand, mask)
    return nx * ny, nx * ny, rp, ci


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_which_plans_satisfy_the_predicate(dtype, monkeypatch):
    """Knob at 1, nontemporal streams forced: units only -> the depth; list entries, split tile-rows, pooled units, the workgroup entry mode, unit_lean = 0 -> 0."""
    monkeypatch.setenv("TILESPMV_UNIT_DEEP", "1")
    for gen, kw, want, fact in ((G.laplacian5pt(48), {}, DEPTH, None), (G.laplacian7pt(16), {}, DEPTH, None), (G.band(1024, 1), dict(entry_mode=0, strip_even=0, strip_cost=100), DEPTH, None),
                                (_grid5(47, 48), {}, 0, "list_entries"), (G.kkt_like(4), dict(entry_mode=0), 0, "list_entries"),
                                (G.band(3000, 40), dict(dense_mode=api.DENSE_VALU, entry_mode=0, split_above=200, strip_cost=32), 0, "num_split_rows"),
                                (G.fem_hex(6, 6, 6, 3), {}, 0, "csr_form"), (G.laplacian5pt(48), dict(entry_mode=2), 0, "entry_mode"), (G.laplacian5pt(48), dict(unit_lean=0), 0, None),
                                (G.laplacian5pt(48), dict(nt_stream=0), 0, None)):
        tm, rows, n, nnz = _tm(gen, dtype)
        kw = dict(dict(nt_stream=1), **kw)
        info = api.plan_layout_digest(tm, rows, n, nnz, **kw)[1]
        assert api.plan_layout_unit_deep(tm, rows, n, nnz, **kw) == want, (kw, info)
        if fact:
            assert info[fact] > 0, (kw, fact, info)                          # what keeps the plan out (pooled plans: csr_form 2)
        api.Tile_destroy(tm)


def test_small_plans_keep_the_lean_kernels_by_rule(monkeypatch):
    monkeypatch.delenv("TILESPMV_UNIT_DEEP", raising=False)
    tm, rows, n, nnz = _tm(G.laplacian5pt(48))
    assert api.plan_layout_unit_deep(tm, rows, n, nnz, nt_stream=1) == 0      # not nontemporal by size
    api.Tile_destroy(tm)


def test_the_knob_is_the_environments():
    """TILESPMV_UNIT_DEEP as a child process finds it: 0 = never, 1 = wherever the predicate holds, unset = by rule (a small plan: not taken)."""
    code = ("import numpy as np; from tilespmv_amd import api, generators as G\n"
            "m, n, rp, ci = G.laplacian5pt(48); nnz = len(ci)\n"
            "tm = api.Tile_create(m, n, nnz, rp, ci, G.compat_values(nnz))\n"
            "print(api.plan_layout_unit_deep(tm, m, n, nnz, nt_stream=1))\n")
    for env, want in ((None, "0"), ("0", "0"), ("1", str(DEPTH)), ("-1", "0")):
        e = dict(os.environ, PYTHONPATH=ROOT)
        e.pop("TILESPMV_UNIT_DEEP", None)
        if env is not None:
            e["TILESPMV_UNIT_DEEP"] = env
        res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, cwd=ROOT)
        assert res.returncode == 0 and res.stdout.split("\n")[-2].strip() == want, (env, res.stdout[-500:], res.stderr[-2000:])
