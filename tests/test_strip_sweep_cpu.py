"""Strided strips (environment knob TILESPMV_STRIP_SWEEP; csrc/hip_plan_stream.hip strip_sweep_stride, cut, renumber_units), checked without a GPU through the stage digests of
the host layout builder (tilespmv_plan_layout_stages).  tests/golden/strip_sweep_parent_stages.json holds the eight stage digests of every case below as the commit BEFORE the
strided strips built them (both libraries, dictionary and 12-byte descriptors, nt_stream = 1, placement_tries = 1, deterministic = 1, compat values), so:
  - with the knob at 0 every stage of every case is the parent's, digest for digest;
  - with the knob unset these small plans are the parent's too (the rule asks for a launch the size rule makes nontemporal; a forced nt_stream does not count);
  - with the knob at 1 the cases whose grid lines are whole tile-rows long (5-point 64^2, 48^2, a row block of 64^2 numbered from its own origin) change from CHOOSE on and keep
    COUNT and ENTRIES, and the others (7-point 16^3: lines one tile-row long; 5-point 40^2: lines of 2.5 tile-rows; power-law 4096) stay the parent's plan in every stage;
  - knob 1 without nontemporal streams, with the wavefront entry mode or with 32 strips per workgroup changes nothing."""
import json
import os

import numpy as np
import pytest

from kernel_asm import ROOT
from tilespmv_amd import api, generators as G

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "strip_sweep_parent_stages.json")))
OPTS = dict(nt_stream=1, placement_tries=1, deterministic=1)
STRIDED = {"lap64": True, "lap48": True, "lap64_shard": True, "lap7pt16": False, "lap40": False, "powerlaw4096": False}


def _gen(name):
    return {"lap64": lambda: G.laplacian5pt(64), "lap48": lambda: G.laplacian5pt(48), "lap64_shard": lambda: G.laplacian5pt(64, rows=(16 * 37, 16 * 211)),
            "lap7pt16": lambda: G.laplacian7pt(16), "lap40": lambda: G.laplacian5pt(40), "powerlaw4096": lambda: G.powerlaw(4096)}[name]()


def _stages(name, dtype, knob, monkeypatch, **kw):
    """{desc_dict: {stage: digest}} of a case under TILESPMV_STRIP_SWEEP = knob (None: unset)"""
    m, n, rp, ci = _gen(name)
    rows = (min(m, len(rp) - 1) // 16) * 16; nnz = int(rp[rows])
    if knob is None:
        monkeypatch.delenv("TILESPMV_STRIP_SWEEP", raising=False)
    else:
        monkeypatch.setenv("TILESPMV_STRIP_SWEEP", str(knob))
    tm = api.Tile_create(rows, n, nnz, rp, ci, G.compat_values(len(ci), dtype), dtype=dtype)
    out = {dd: {k: int(v) for k, v in api.plan_layout_stages(tm, rows, n, nnz, desc_dict=dd, **dict(OPTS, **kw))[0].items()} for dd in (1, 0)}
    api.Tile_destroy(tm)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(STRIDED))
def test_stage_digests_against_the_parent_commit(name, dtype, monkeypatch):
    off, auto, on = (_stages(name, dtype, knob, monkeypatch) for knob in (0, None, 1))
    for dd in (1, 0):
        parent = GOLDEN["%s/%s/dict%d" % (name, np.dtype(dtype).name, dd)]
        assert off[dd] == parent, (name, dd, [k for k in parent if off[dd][k] != parent[k]])          # knob 0: the parent's plan
        assert auto[dd] == parent, (name, dd, [k for k in parent if auto[dd][k] != parent[k]])        # by rule: small plans never change
        changed = sorted(k for k in parent if on[dd][k] != parent[k])
        if STRIDED[name]:
            assert changed == sorted(["choose", "cut", "emit", "order", "encode", "finish"]), (name, dd, changed)   # (COUNT and ENTRIES — there are no list entries — know nothing of the strips)
        else:
            assert changed == [], (name, dd, changed)


def test_knob_one_needs_the_forms_the_rule_names(monkeypatch):
    for kw in (dict(nt_stream=0), dict(entry_mode=1), dict(entry_mode=2, wg_strips=32), dict(csr_split=2)):
        assert _stages("lap64", np.float64, 1, monkeypatch, **kw) == _stages("lap64", np.float64, 0, monkeypatch, **kw), kw


def test_headline_plan_is_strided_by_rule(monkeypatch):
    """5-point 4096^2 on compat data with every knob unset (a 461 MB launch, one stride): the rule's plan is knob 1's, not knob 0's, from CHOOSE on."""
    m, n, rp, ci = G.laplacian5pt(4096)
    nnz = len(ci)
    tm = api.Tile_create(m, n, nnz, rp, ci, G.compat_values(nnz))
    st = {}
    for knob in (None, 0, 1):
        if knob is None:
            monkeypatch.delenv("TILESPMV_STRIP_SWEEP", raising=False)
        else:
            monkeypatch.setenv("TILESPMV_STRIP_SWEEP", str(knob))
        st[knob] = api.plan_layout_stages(tm, m, n, nnz)[0]
    api.Tile_destroy(tm)
    assert st[None] == st[1]
    assert st[None]["count"] == st[0]["count"] and st[None]["choose"] != st[0]["choose"] and st[None]["cut"] != st[0]["cut"]
