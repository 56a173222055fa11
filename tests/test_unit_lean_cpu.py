"""The lean forms of the unit kernel (csrc/hip_kernels_lean.hip, tilespmv_plan_options.unit_lean), checked without a GPU.  From the device assembly of both builds: the
instantiation budget (24 kernels in the fp64 library, 8 in the fp32 one), no scratch, at most 64 VGPRs (8 waves per SIMD), no 16-lane all-reduce (`row_ror:8`) in any lean
kernel and no `row_ror:15` (the derived unit's x one lane up) in those compiled without derived units; and the length of the unit loop of the lean halves kernel that the
headline runs (dictionary descriptors, entry mode 0, derived units): at most 280 instructions per batch of 4 units — the general kernel's 385, less the four all-reduce blocks
(104), their and / cmp / saveexec / branch / s_or (16) and the three gather-side instructions of a row unit x 4 (12) = 253, plus 27 of slack for scheduling — and shorter still
without derived units.  From the host layout builder (tilespmv_plan_layout_digest / _stages): which plans report which form, that knob value 0 reports the general kernel,
that the environment variable is the knob's default, and that the lean form changes no stage of the layout."""
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
from loop_waits import HALF_VALUE_LOAD, unit_loops  # noqa: E402

BUDGET = {"f64": 24, "f32": 8}
HOT = "k_units_lean<4, 0, 16, true, true, 2, %s>"   # halves, dictionary descriptors, entry mode 0: what the 5-point 4096^2 headline runs (derived units: true)
HOT_MAX_INSNS = 280


@pytest.fixture(scope="module")
def lean_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_asm")
    with ThreadPoolExecutor(2) as ex:
        return dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_kernels_lean.hip", dt, str(d / (dt + ".s"))), ("f64", "f32"))))


def _kernels(asm):
    """{demangled kernel name: (text of the function, its descriptor)} of an assembly text."""
    funcs = re.findall(r"^(_Z\w+):\s*; @\1\n(.*?)^\s+s_endpgm", asm, re.S | re.M)
    meta = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S))
    dem = subprocess.run(["c++filt"] + [n for n, _ in funcs], capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.split("(")[0].replace("void tilespmv::", ""): (body, meta[n]) for (n, body), d in zip(funcs, dem) if n in meta}


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_budget_and_resources_of_the_lean_kernels(lean_asm, dt):
    asm = lean_asm[dt]
    spills = private_segments(asm)
    assert len(spills) == BUDGET[dt], (dt, len(spills))
    assert not any(spills.values()), {k: v for k, v in spills.items() if v}
    kernels = _kernels(asm)
    forms = (0, 1, 2) if dt == "f64" else (0,)
    want = sorted("k_units_lean<4, %d, 16, %s, true, %d, %s>" % (w, cd, vf, dv) for w in (0, 2) for cd in ("true", "false") for vf in forms for dv in ("true", "false"))
    assert sorted(kernels) == want, sorted(kernels)
    for name, (body, desc) in kernels.items():
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        assert vgpr <= 64, (dt, name, vgpr)                                   # 8 waves per SIMD
        assert "row_ror:8" not in body, (dt, name)                            # the all-reduce of a row unit is gone
        if name.endswith(", false>"):
            assert "row_ror:15" not in body, (dt, name)                       # ... and without derived units, unit_x_use
        else:
            assert "row_ror:15" in body, (dt, name)


def test_unit_loop_of_the_lean_halves_kernel(lean_asm):
    loops = unit_loops(lean_asm["f64"], ("k_units_lean",), HALF_VALUE_LOAD)
    on, off = loops[HOT % "true"], loops[HOT % "false"]
    print(on, off)
    assert on["vmcnt"] and off["vmcnt"]                                       # the loop around the nontemporal 8-byte value load was found, and waits for loads
    assert 0 < on["insns"] <= HOT_MAX_INSNS, on
    assert 0 < off["insns"] < on["insns"], (off, on)


def _tm(gen, dtype=np.float64, hyb=False):
    m, n, rp, ci = gen
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    return api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci), dtype), dtype=dtype, hyb=hyb), rows, n, nnz


LEAN_ON = dict(nt_stream=1)   # (small plans are not nontemporal by rule; the lean forms are nontemporal ones)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_which_plans_report_which_form(dtype):
    """5-point grid: derived units, no row unit -> 1 (and 2 with absorb = 2, which derives nothing); KKT-like: no derived unit -> 2; all-formats: dense-row tiles -> 0."""
    for gen, hyb, kw, want in ((G.laplacian5pt(48), False, {}, 1), (G.laplacian5pt(48), False, dict(absorb=2), 2), (G.laplacian5pt(48), False, dict(entry_mode=2), 1),
                               (G.kkt_like(4), False, dict(entry_mode=0), 2), (G.kkt_like(4), False, dict(entry_mode=2), 2),
                               (G.all_formats(12, 7), True, dict(csr_split=1, entry_mode=0), 0)):
        tm, rows, n, nnz = _tm(gen, dtype, hyb)
        d1, i1 = api.plan_layout_digest(tm, rows, n, nnz, **LEAN_ON, **kw)
        d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, unit_lean=0, **LEAN_ON, **kw)
        assert i1["unit_lean"] == want, (kw, i1["unit_lean"])
        assert (i1["derived_units"] > 0) == (want == 1) or want == 0, (kw, i1["derived_units"])
        assert i0["unit_lean"] == 0, kw                                       # knob value 0: the general kernel
        assert d1 == d0 and {k: v for k, v in i1.items() if k != "unit_lean" and not k.endswith("_us")} == {k: v for k, v in i0.items() if k != "unit_lean" and not k.endswith("_us")}
        s1, _ = api.plan_layout_stages(tm, rows, n, nnz, **LEAN_ON, **kw)
        s0, _ = api.plan_layout_stages(tm, rows, n, nnz, unit_lean=0, **LEAN_ON, **kw)
        assert s1 == s0, kw                                                   # no stage of the layout knows about the form
        api.Tile_destroy(tm)


def test_forms_without_a_lean_kernel_keep_the_general_one():
    """Default cache policy, the wavefront entry mode, 32 strips per workgroup, pooled units and the first-generation kernel have no lean form."""
    tm, rows, n, nnz = _tm(G.laplacian5pt(48))
    for kw in (dict(nt_stream=0), dict(entry_mode=1), dict(nt_stream=1, entry_mode=2, wg_strips=32), dict(nt_stream=1, kernel=api.KERNEL_DIRECT)):
        assert api.plan_layout_digest(tm, rows, n, nnz, **kw)[1]["unit_lean"] == 0, kw
    assert api.plan_layout_digest(tm, rows, n, nnz)[1]["unit_lean"] == 0      # (a small plan: not nontemporal by rule)
    api.Tile_destroy(tm)
    tm, rows, n, nnz = _tm(G.fem_hex(6, 6, 6, 3))
    i = api.plan_layout_digest(tm, rows, n, nnz, nt_stream=1)[1]
    assert (i["csr_form"], i["unit_lean"]) == (2, 0), i                       # pooled
    api.Tile_destroy(tm)


def test_headline_plan_takes_the_lean_halves_form():
    """5-point 4096^2 on compat data with every knob unset: halves, dictionary descriptors, nontemporal, per-strip entries, derived units -> form 1."""
    m, n, rp, ci = G.laplacian5pt(4096)
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    tm = api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci)))
    i = api.plan_layout_digest(tm, rows, n, nnz)[1]
    assert (i["unit_lean"], i["unit_value_bytes"], i["desc_bytes"], i["nt_stream"], i["entry_mode"], i["wg_strips"]) == (1, 2, 4, 1, 0, 16), i
    assert i["derived_units"] > 0
    api.Tile_destroy(tm)


def test_environment_variable_is_the_knobs_default():
    """TILESPMV_UNIT_LEAN is read once per process: a child process each."""
    code = ("import numpy as np; from tilespmv_amd import api, generators as G\n"
            "m, n, rp, ci = G.laplacian5pt(48); nnz = len(ci)\n"
            "tm = api.Tile_create(m, n, nnz, rp, ci, G.compat_values(nnz))\n"
            "print(api.plan_layout_digest(tm, m, n, nnz, nt_stream=1)[1]['unit_lean'], api.plan_layout_digest(tm, m, n, nnz, nt_stream=1, unit_lean=1)[1]['unit_lean'])\n")
    for env, want in ((None, "1 1"), ("0", "0 1"), ("1", "1 1")):
        e = dict(os.environ, PYTHONPATH=ROOT)
        e.pop("TILESPMV_UNIT_LEAN", None)
        if env is not None:
            e["TILESPMV_UNIT_LEAN"] = env
        res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, cwd=ROOT)
        assert res.returncode == 0 and res.stdout.split("\n")[-2].strip() == want, (env, res.stdout[-500:], res.stderr[-2000:])   # an option beats the environment
