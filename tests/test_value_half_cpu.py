"""Unit values stored as halves (tilespmv_plan_options.value_narrow = 2, or unset on large plans; fp64 build): a plan whose unit values are all +-0 or normal IEEE binary16
numbers stores them in 2 bytes, the kernels widen half -> float -> double (both exact).  Host layout builder only (tilespmv_plan_layout_digest / _stages): the predicate's
boundaries through whole plans, what knob values 1 and 2 mean, the size rule tried narrowest first, which stages the 2-byte form may change, the forms without a narrow
kernel, the fp32 library; then the predicate and the conversion over all 65,536 half patterns in a stand-alone C++ program under AddressSanitizer and UBSan (on the CPU;
nothing is loaded into python), and the resources of the four kernels of hip_kernels_half.hip from their device assembly.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from kernel_asm import ROOT, device_asm, private_segments
from tilespmv_amd import api, generators as G

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from loop_waits import HALF_VALUE_LOAD, unit_loops  # noqa: E402

# tilespmv_plan_layout_digest of the 5-point 64^2 grid on compat data with value_narrow=1 at the commit before the 2-byte form existed (4-byte values): knob value 1 keeps its meaning
PARENT_FLOAT_PLAN_DIGEST = 0xb7a42f6836b21110
PARENT_FLOAT_PLAN_FACTS = dict(unit_value_bytes=4, stream_bytes=154352, device_bytes=88928, num_tasks=64)


def _tm(gen, vals=None, dtype=np.float64, hyb=False):
    m, n, rp, ci = gen
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    v = G.compat_values(len(ci), dtype) if vals is None else vals
    return api.Tile_create(rows, n, nnz, rp, ci, v, dtype=dtype, hyb=hyb), rows, n, nnz


def _grid_with(value):
    """5-point 64^2 grid (classic units, per-strip entries: eligible), the diagonal entry of a middle row replaced by `value`."""
    m, n, rp, ci = G.laplacian5pt(64)
    vals = G.compat_values(len(ci))
    row = 64 * 31 + 17
    k = int(rp[row]) + int(np.nonzero(ci[rp[row]:rp[row + 1]] == row)[0][0])
    vals[k] = value
    return _tm((m, n, rp, ci), vals)


def _facts(i):
    return {k: v for k, v in i.items() if not k.endswith("_us")}


@pytest.mark.parametrize("value", [2.0 ** -14, 1.0 + 2.0 ** -10, 65504.0, -0.0, -65504.0, -(2.0 ** -14)])
def test_values_a_half_holds_exactly_keep_the_plan_at_two_bytes(value):
    tm, rows, n, nnz = _grid_with(value)
    d2, i2 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)
    d4, i4 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    assert (i2["unit_value_bytes"], i4["unit_value_bytes"]) == (2, 4) and d2 != d4
    assert i2["nt_stream"] == 1 and i2["stream_bytes"] < i4["stream_bytes"]
    api.Tile_destroy(tm)


@pytest.mark.parametrize("value", [2.0 ** -15, 2.0 ** -24, 1.0 + 2.0 ** -11, 65536.0, float(np.nextafter(65504.0, np.inf, dtype=np.float32))])
def test_one_exact_float_that_is_no_normal_half_gives_four_bytes(value):
    """fp16 denormals (2^-15, 2^-24), an 11th mantissa bit, 2^16 and the float behind 65504: all exact floats, none a normal half."""
    assert float(np.float32(value)) == value
    tm, rows, n, nnz = _grid_with(value)
    d2, i2 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)
    d4, i4 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    assert i2["unit_value_bytes"] == 4 and d2 == d4 and _facts(i2) == _facts(i4)
    api.Tile_destroy(tm)


def test_one_value_that_is_no_float_gives_the_wide_plan():
    tm, rows, n, nnz = _grid_with(0.1)
    d2, i2 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)
    d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    assert i2["unit_value_bytes"] == 8 and d2 == d0 and _facts(i2) == _facts(i0)
    api.Tile_destroy(tm)


def test_knob_value_one_still_means_floats():
    """Halvable data, value_narrow=1: 4 bytes, and the plan the parent commit built for this knob value (digest and facts recorded there)."""
    tm, rows, n, nnz = _tm(G.laplacian5pt(64))
    d1, i1 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    assert d1 == PARENT_FLOAT_PLAN_DIGEST and {k: i1[k] for k in PARENT_FLOAT_PLAN_FACTS} == PARENT_FLOAT_PLAN_FACTS
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)[1]["unit_value_bytes"] == 2
    api.Tile_destroy(tm)


@pytest.mark.parametrize("gen,kw", [(lambda: G.laplacian7pt(48), {}), (lambda: G.band_plus_random(40000, 4, 3, 5), {"entry_mode": 2}), (lambda: G.laplacian5pt(50), {"csr_split": 1})])
def test_two_byte_form_differs_from_the_float_form_in_the_value_array_only(gen, kw):
    """Same unit numbering (groups of 4 units, task tails padded to 4): of the stages only encode / entries / finish may change, the task count stays, and the streams lose
    exactly 16 x 2 bytes per padded unit — in the byte model (stream_bytes) and in what is uploaded (device_bytes)."""
    tm, rows, n, nnz = _tm(gen())
    half, i2 = api.plan_layout_stages(tm, rows, n, nnz, value_narrow=2, **kw)
    flt, i4 = api.plan_layout_stages(tm, rows, n, nnz, value_narrow=1, **kw)
    assert (i2["unit_value_bytes"], i4["unit_value_bytes"]) == (2, 4)
    changed = {k for k in api.STAGE_NAMES if half[k] != flt[k]}
    assert "encode" in changed and changed <= {"encode", "entries", "finish"}, changed
    assert i2["num_tasks"] == i4["num_tasks"]
    # The padded unit count, from plans that hold no halves: the float plan with 12-byte descriptors against the float plan with 4-byte ones differs by 8 bytes per padded
    # unit in the byte model (the dictionary itself is not part of it) and by nothing else.
    _, i12 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1, **{**kw, "desc_dict": 0})
    _, i04 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1, **{**kw, "desc_dict": 1})
    assert (i12["desc_bytes"], i04["desc_bytes"], i12["unit_value_bytes"], i04["unit_value_bytes"]) == (12, 4, 4, 4)
    assert (i12["stream_bytes"] - i04["stream_bytes"]) % 8 == 0
    padded_units = (i12["stream_bytes"] - i04["stream_bytes"]) // 8
    assert padded_units % 4 == 0 and padded_units > 0                                  # whole groups of 4
    assert i4["stream_bytes"] - i2["stream_bytes"] == 32 * padded_units                # 16 values x 2 bytes per padded unit, exactly: the byte model ...
    assert i4["device_bytes"] - i2["device_bytes"] == 32 * padded_units                # ... and what is uploaded
    for k in ("num_split_rows", "list_entries", "derived_units", "desc_bytes", "entry_mode", "nt_stream", "csr_form"):
        assert i2[k] == i4[k], k
    api.Tile_destroy(tm)


def test_size_rule_is_tried_narrowest_first():
    """Unset knob.  5-point 4096^2: the 2-byte launch still moves more than the 400 MB of the nontemporal rule -> halves.  5-point 3456^2: the 2-byte launch would fall
    under it (about 328 MB), the 4-byte launch does not -> floats, as before.  (Layout digests only: nothing is uploaded.)"""
    for side, want in ((3456, 4), (4096, 2)):
        m, n, rp, ci = G.laplacian5pt(side)
        rows = cases.truncated_rows(m); nnz = int(rp[rows])
        tm = api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci)))
        d, i = api.plan_layout_digest(tm, rows, n, nnz)
        assert (i["unit_value_bytes"], i["nt_stream"]) == (want, 1), side
        assert i["stream_bytes"] > (400 << 20), side
        dk, ik = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2 if want == 2 else 1)   # the knob value that asks for this width
        assert dk == d and _facts(ik) == _facts(i), side
        api.Tile_destroy(tm)


def test_small_plans_stay_wide_by_default():
    for gen, hyb in ((G.laplacian7pt(48), False), (G.powerlaw(60000, seed=2), False), (G.all_formats(12, 7), True), (G.band_plus_random(40000, 4, 3, 5), False), (G.band(30000, 40), False)):
        tm, rows, n, nnz = _tm(gen, hyb=hyb)
        d, i = api.plan_layout_digest(tm, rows, n, nnz)
        d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
        assert i["unit_value_bytes"] == 8 and d == d0
        api.Tile_destroy(tm)


def test_forms_without_a_narrow_kernel_stay_wide():
    """Pooled units, the wavefront entry mode, 32 strips per workgroup and the first-generation kernel have no narrow form, of either width."""
    tm, rows, n, nnz = _tm(G.fem_hex(12, 12, 12, 3))
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)[1]["unit_value_bytes"] == 8          # pooled
    api.Tile_destroy(tm)
    tm, rows, n, nnz = _tm(G.powerlaw(60000, seed=2))
    for kw, want in ((dict(entry_mode=1), 8), (dict(entry_mode=2, wg_strips=32), 8), (dict(kernel=api.KERNEL_DIRECT), 8), (dict(entry_mode=2), 2), (dict(entry_mode=0), 2)):
        assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2, **kw)[1]["unit_value_bytes"] == want, kw
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2, nt_stream=0)[1]["unit_value_bytes"] == 8      # the caller refused nontemporal streams
    api.Tile_destroy(tm)


def test_environment_variable_is_the_knobs_default(monkeypatch):
    tm, rows, n, nnz = _tm(G.laplacian5pt(64))
    monkeypatch.setenv("TILESPMV_VALUE_NARROW", "2")
    assert api.plan_layout_digest(tm, rows, n, nnz)[1]["unit_value_bytes"] == 2
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)[1]["unit_value_bytes"] == 4     # an option beats the environment
    api.Tile_destroy(tm)


def test_fp32_library_takes_the_value_and_changes_nothing():
    tm, rows, n, nnz = _tm(G.laplacian5pt(64), dtype=np.float32)
    d2, i2 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=2)
    d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    dd, idf = api.plan_layout_digest(tm, rows, n, nnz)
    assert d2 == d0 == dd and i2["unit_value_bytes"] == i0["unit_value_bytes"] == idf["unit_value_bytes"] == 4
    api.Tile_destroy(tm)


def test_predicate_and_conversion_over_all_half_patterns(tmp_path):
    """tests/value_half_check.cpp: value_halvable is true exactly for +-0 and the 61,440 normal halves, value_half_bits returns the pattern, the neighbouring doubles of every
    accepted value are refused.  Host code with AddressSanitizer + UBSan, run as a program of its own."""
    exe = str(tmp_path / "value_half_check")
    csrc = os.path.join(ROOT, "tilespmv_amd", "csrc")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-DMAT_VAL_TYPE=double",
                    os.path.join(ROOT, "tests", "value_half_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "61442 patterns accepted, 0 failures" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr


def test_resources_of_the_half_kernels(tmp_path):
    """hip_kernels_half.hip as the gfx950 compiler built it: exactly the four kernels (entry mode 0 / 2 x 12-byte / dictionary descriptors), no scratch, at most 64 VGPRs
    (8 waves per SIMD), and the unit loop — the loop around the nontemporal 8-byte value load — is found in each."""
    asm = device_asm("hip_kernels_half.hip", "f64", str(tmp_path / "half.s"))
    spills = private_segments(asm)
    assert len(spills) == 4 and not any(spills.values()), spills
    loops = unit_loops(asm, ("k_units_half",), HALF_VALUE_LOAD)
    assert sorted(loops) == sorted("k_units_half<4, %d, 16, %s, true, false, false, true>" % (w, cd) for w in (0, 2) for cd in ("true", "false")), sorted(loops)
    for k, rec in loops.items():
        print(k, rec)
        assert rec["scratch"] == 0 and rec["vgpr"] <= 64, (k, rec)
        assert rec["insns"] > 0 and rec["vmcnt"], (k, rec)
    assert "v_cvt_f32_f16" in asm and "v_cvt_f64_f32" in asm          # widened in registers, half -> float -> double
