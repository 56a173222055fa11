"""The deep unit kernel on the GPU (environment knob TILESPMV_UNIT_DEEP, tilespmv_plan_unit_deep; csrc/hip_kernels_deep.hip).  A lean plan with per-strip entries that holds
nothing but units — no list entry, no split tile-row, no fallback launch — runs k_units_deep, which keeps the x gathers of two unit batches in flight per wavefront.  Same
plan, same streams, same multiply-then-add in unit order, so y must keep EVERY bit: each case compares the whole y of the deep launch (knob 1) with the lean launch (knob 0) and
the general launch (unit_lean = 0) of the same plan by np.array_equal, checks the 777 sentinel behind y, and compares with the oracle inside the parity tests' tolerance
(TOL x sum |a_ij x_j|).  Host- and device-built plans, 12-byte and dictionary descriptors, compat values and U(-1, 1) values rounded to the form, every value form.  Small plans
reach the kernel through nt_stream = 1 and the knob at 1; with the knob unset they keep the lean kernels (the rule asks for a launch that is nontemporal by size).

Shapes, the smallest where each thing can go wrong: 5-point 48^2 (40 units per task: two whole descriptor chunks and a rest of two batches, with derived units); the same with
strided strips (TILESPMV_STRIP_SWEEP = 1: S = 3, the strided y store); 7-point 16^3; the tridiagonal band of tests/test_gpu_unit_lean.py cut into tasks of 3, 6, 9 and 12 units
(shorter than the pipeline, every residue mod 4); one tile-row of 3 units (a one-task grid).  5-point 47 x 48 and the KKT-like generator at g = 4 have list entries: the query
reports 0 and the launch is the lean one."""
import numpy as np
import pytest

from cases import truncated_rows
from test_gpu_unit_lean import COMMON, FORMS, TOL, _abs_bound, _grid5, _run, _value_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_unit_lean.py)."""
    import torch
    torch.zeros(1, device="cuda")
    yield


def _cases():
    from tilespmv_amd import generators as G
    band = lambda sc, tasks: dict(gen=lambda: G.band(1024, 1), kw=dict(entry_mode=0, strip_even=0, strip_cost=sc), deep=True, facts=dict(num_tasks=tasks, list_entries=0))
    return {
        "lap48": dict(gen=lambda: G.laplacian5pt(48), kw={}, deep=True, facts=dict(list_entries=0, derived_units=239)),
        "lap48_strided": dict(gen=lambda: G.laplacian5pt(48), kw={}, deep=True, sweep=1, facts=dict(list_entries=0)),
        "lap7pt16": dict(gen=lambda: G.laplacian7pt(16), kw={}, deep=True, facts=dict(list_entries=0)),
        "band_3_units": band(100, 64), "band_6_units": band(128, 32), "band_9_units": band(200, 22), "band_12_units": band(256, 16),
        "one_tile_row": dict(gen=lambda: G.band(16, 1, 64), kw=dict(entry_mode=0), deep=True, facts=dict(num_tasks=1, rows=16, list_entries=0)),
        "lap47x48": dict(gen=lambda: _grid5(47, 48), kw={}, deep=False, facts=dict(rows=2256)),
        "kkt4": dict(gen=lambda: G.kkt_like(4), kw=dict(entry_mode=0), deep=False, facts=dict(list_entries=120)),
    }


CASE_NAMES = ["lap48", "lap48_strided", "lap7pt16", "band_3_units", "band_6_units", "band_9_units", "band_12_units", "one_tile_row", "lap47x48", "kkt4"]


def _plans(monkeypatch, c, dtype, tm, rowA, n, nnz, rp, ci, vals, kw):
    """{(builder, launch): plan}: deep = knob 1, lean = knob 0, general = knob 1 with unit_lean = 0; the strided case sets TILESPMV_STRIP_SWEEP for all of them."""
    from tilespmv_amd import api
    if "sweep" in c:
        monkeypatch.setenv("TILESPMV_STRIP_SWEEP", str(c["sweep"]))
    plans = {}
    for launch, knob, extra in (("deep", 1, {}), ("lean", 0, {}), ("general", 1, dict(unit_lean=0))):
        monkeypatch.setenv("TILESPMV_UNIT_DEEP", str(knob))
        plans[("host", launch)] = api.Plan(tm, rowA, n, nnz, **kw, **extra)
        plans[("device", launch)] = api.Plan.from_csr(rowA, n, nnz, rp, ci, vals, dtype=dtype, **kw, **extra)
    monkeypatch.delenv("TILESPMV_UNIT_DEEP")
    monkeypatch.delenv("TILESPMV_STRIP_SWEEP", raising=False)
    return plans


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_deep_launch_equals_lean_and_general_launch(name, form, monkeypatch):
    from oracle.oracle import CpuImpl
    from tilespmv_amd import api
    c = _cases()[name]
    dtype, narrow, vbytes = FORMS[form]
    m, n, rp, ci = c["gen"]()
    nnz, rowA = len(ci), truncated_rows(m)
    O = CpuImpl("oracle", dtype)
    for vals, x, what in _value_sets(form, nnz, n):
        want = O.spmv(O.tile_create(rowA, n, nnz, rp, ci, vals), rowA, n, nnz, rp, ci, vals, x)["y"].astype(np.float64)
        bound = TOL[np.dtype(dtype)] * _abs_bound(rowA, rp, ci, vals, x) + 1e-300
        tm = api.Tile_create(rowA, n, nnz, rp, ci, vals, dtype=dtype)
        for desc_dict in (0, 1):
            kw = dict(COMMON, value_narrow=narrow, desc_dict=desc_dict, **c["kw"])
            tag = (name, form, what, desc_dict)
            plans = _plans(monkeypatch, c, dtype, tm, rowA, n, nnz, rp, ci, vals, kw)
            info = {k: p.info() for k, p in plans.items()}
            deep = {k: p.unit_deep() for k, p in plans.items()}
            ih = info[("host", "deep")]
            print(tag, deep, plans[("host", "deep")].strip_stride(), {k: ih[k] for k in ("unit_lean", "entry_mode", "num_tasks", "list_entries", "derived_units", "desc_bytes", "unit_value_bytes", "nt_stream")})
            assert (ih["unit_value_bytes"], ih["nt_stream"], ih["desc_bytes"], ih["entry_mode"]) == (vbytes, 1, 4 if desc_dict else 12, 0), (tag, ih)
            for k, v in c["facts"].items():
                assert ih[k] == v, (tag, k, ih[k])
            for b in ("host", "device"):
                assert deep[(b, "deep")] == (2 if c["deep"] else 0), (tag, deep)              # the depth, or 0: list entries keep today's kernels
                assert deep[(b, "lean")] == deep[(b, "general")] == 0, (tag, deep)            # knob 0: never; unit_lean = 0: no lean form, no deep one
                assert info[(b, "deep")]["unit_lean"] == info[(b, "lean")]["unit_lean"] > 0 and info[(b, "general")]["unit_lean"] == 0, tag
                assert {k: v for k, v in info[(b, "deep")].items() if not k.endswith("_us")} == {k: v for k, v in info[(b, "lean")].items() if not k.endswith("_us")}, (tag, b)
            if "sweep" in c:
                assert all(p.strip_stride() == 3 for p in plans.values()), tag
            assert len({tuple(sorted(p.stream_digests().items())) for p in plans.values()}) == 1, tag    # one plan, byte for byte, whatever launches it
            y = {k: _run(p, x, rowA) for k, p in plans.items()}                               # (_run checks the sentinel behind y)
            for p in plans.values():
                p.close()
            ref = y[("host", "lean")]
            for k, got in y.items():
                assert np.array_equal(got, ref), (tag, k, int(np.count_nonzero(got != ref)))  # whole y, every bit
            err = np.abs(ref.astype(np.float64) - want)
            assert (err <= bound).all(), (tag, float((err / bound).max()))
        api.Tile_destroy(tm)


def test_small_plans_keep_the_lean_kernels_with_the_knob_unset(monkeypatch):
    """The rule: a launch that is not nontemporal by size does not take the deep kernel, so the plans of the other GPU tests run the kernels those tests name."""
    from tilespmv_amd import api, generators as G
    monkeypatch.delenv("TILESPMV_UNIT_DEEP", raising=False)
    m, n, rp, ci = G.laplacian5pt(48)
    nnz = len(ci)
    tm = api.Tile_create(m, n, nnz, rp, ci, G.compat_values(nnz))
    p = api.Plan(tm, m, n, nnz, **COMMON)
    assert p.info()["unit_lean"] == 1 and p.info()["list_entries"] == 0 and p.unit_deep() == 0
    p.close()
    api.Tile_destroy(tm)
