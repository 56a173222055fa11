"""Narrow unit values (tilespmv_plan_options.value_narrow; fp64 build): a plan whose unit values all survive double -> float -> double stores them in 4 bytes.
Host layout builder only (tilespmv_plan_layout_digest / _stages): the predicate's boundaries, the default (size) rule, which stages the narrow form may change,
and the fp32 library, which takes the knob and changes nothing.  No GPU needed.
(A value-map plan stays wide too; value maps exist on the device path only, so that case lives in tests/test_gpu_value_narrow.py.)"""
import numpy as np
import pytest

import cases
from tilespmv_amd import api, generators as G

FLT_MAX = float(np.finfo(np.float32).max)


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


@pytest.mark.parametrize("value", [2.0 ** -126, 1.0 + 2.0 ** -23, FLT_MAX, -0.0, -FLT_MAX, -(2.0 ** -126)])
def test_values_a_float_holds_exactly_keep_the_plan_narrow(value):
    tm, rows, n, nnz = _grid_with(value)
    dn, i_n = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    dw, i_w = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    assert (i_n["unit_value_bytes"], i_w["unit_value_bytes"]) == (4, 8) and dn != dw
    assert i_n["nt_stream"] == 1                      # a narrow plan reads its streams nontemporally, whatever its size
    assert i_n["stream_bytes"] < i_w["stream_bytes"]
    api.Tile_destroy(tm)


@pytest.mark.parametrize("value", [2.0 ** -127, 1.0 + 2.0 ** -24, 2.0 ** 128, 0.1, 2.0 ** -149, float(np.nextafter(FLT_MAX, np.inf))])
def test_one_value_a_float_cannot_hold_keeps_the_plan_wide(value):
    tm, rows, n, nnz = _grid_with(value)
    dn, i_n = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    dw, i_w = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    assert i_n["unit_value_bytes"] == 8 and dn == dw
    assert {k: v for k, v in i_n.items() if not k.endswith("_us")} == {k: v for k, v in i_w.items() if not k.endswith("_us")}
    api.Tile_destroy(tm)


def test_default_rule_narrows_large_narrowable_plans_only():
    """Unset knob: narrow iff eligible, narrowable and the narrowed launch still moves more than the 400 MB above which the streams are read nontemporally."""
    m, n, rp, ci = G.laplacian5pt(3456)
    rows = cases.truncated_rows(m); nnz = int(rp[rows])
    tm = api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci)))
    d_def, i_def = api.plan_layout_digest(tm, rows, n, nnz)
    d_w, i_w = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    assert (i_def["unit_value_bytes"], i_def["nt_stream"]) == (4, 1) and i_w["unit_value_bytes"] == 8
    # 64 bytes less per padded unit (16 values of 4 instead of 8 bytes); the plan's device bytes lose exactly the same, which names the padded unit count
    saved = i_w["stream_bytes"] - i_def["stream_bytes"]
    assert saved == i_w["device_bytes"] - i_def["device_bytes"] and saved % 64 == 0
    padded_units = saved // 64
    assert nnz / 16 <= padded_units <= 1.05 * nnz / 16 + 3 * i_def["num_tasks"]     # 16 slots per unit, at most 3 padding units per task
    assert i_def["stream_bytes"] > (400 << 20)
    assert api.plan_layout_digest(tm, rows, n, nnz, nt_stream=0)[1]["unit_value_bytes"] == 8          # the caller refused nontemporal streams: wide
    d_off, i_off = api.plan_layout_digest(tm, rows, n, nnz, nt_stream=0, value_narrow=1)
    assert (i_off["unit_value_bytes"], i_off["nt_stream"]) == (8, 0)
    api.Tile_destroy(tm)
    tm = api.Tile_create(rows, n, nnz, rp, ci, G.real_values(len(ci)))                                 # real-valued data: the plan of before, byte for byte
    d_r, i_r = api.plan_layout_digest(tm, rows, n, nnz)
    d_r0, i_r0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    assert i_r["unit_value_bytes"] == 8 and d_r == d_r0
    api.Tile_destroy(tm)


def test_small_plans_stay_wide_by_default():
    for gen, hyb in ((G.laplacian7pt(48), False), (G.powerlaw(60000, seed=2), False), (G.all_formats(12, 7), True), (G.band_plus_random(40000, 4, 3, 5), False), (G.band(30000, 40), False)):
        tm, rows, n, nnz = _tm(gen, hyb=hyb)
        d, i = api.plan_layout_digest(tm, rows, n, nnz)
        d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
        assert i["unit_value_bytes"] == 8 and d == d0
        api.Tile_destroy(tm)


def test_forms_without_a_narrow_kernel_stay_wide():
    """Pooled units, the wavefront entry mode, 32 strips per workgroup and the first-generation kernel have no narrow form."""
    tm, rows, n, nnz = _tm(G.fem_hex(12, 12, 12, 3))
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)[1]["unit_value_bytes"] == 8          # pooled
    api.Tile_destroy(tm)
    tm, rows, n, nnz = _tm(G.powerlaw(60000, seed=2))
    for kw, want in ((dict(entry_mode=1), 8), (dict(entry_mode=2, wg_strips=32), 8), (dict(kernel=api.KERNEL_DIRECT), 8), (dict(entry_mode=2), 4), (dict(entry_mode=0), 4)):
        assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1, **kw)[1]["unit_value_bytes"] == want, kw
    api.Tile_destroy(tm)


@pytest.mark.parametrize("gen,kw", [(lambda: G.laplacian7pt(48), {}), (lambda: G.band_plus_random(40000, 4, 3, 5), {"entry_mode": 2}), (lambda: G.laplacian5pt(50), {"csr_split": 1})])
def test_narrow_form_changes_the_encoding_stages_only(gen, kw):
    tm, rows, n, nnz = _tm(gen())
    narrow, i_n = api.plan_layout_stages(tm, rows, n, nnz, value_narrow=1, **kw)
    wide, i_w = api.plan_layout_stages(tm, rows, n, nnz, value_narrow=0, **kw)
    assert (i_n["unit_value_bytes"], i_w["unit_value_bytes"]) == (4, 8)
    changed = {k for k in api.STAGE_NAMES if narrow[k] != wide[k]}
    assert "encode" in changed and changed <= {"encode", "entries", "finish"}, changed
    api.Tile_destroy(tm)


def test_environment_variable_is_the_knobs_default(monkeypatch):
    tm, rows, n, nnz = _tm(G.laplacian5pt(64))
    monkeypatch.setenv("TILESPMV_VALUE_NARROW", "1")
    assert api.plan_layout_digest(tm, rows, n, nnz)[1]["unit_value_bytes"] == 4
    assert api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)[1]["unit_value_bytes"] == 8     # an option beats the environment
    api.Tile_destroy(tm)


def test_fp32_library_takes_the_knob_and_changes_nothing():
    tm, rows, n, nnz = _tm(G.laplacian5pt(64), dtype=np.float32)
    d1, i1 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=1)
    d0, i0 = api.plan_layout_digest(tm, rows, n, nnz, value_narrow=0)
    dd, idf = api.plan_layout_digest(tm, rows, n, nnz)
    assert d1 == d0 == dd and i1["unit_value_bytes"] == i0["unit_value_bytes"] == idf["unit_value_bytes"] == 4
    api.Tile_destroy(tm)
