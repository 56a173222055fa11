"""New values for a plan whose pattern stays (TILESPMV_CREATE_VALUE_MAP, ``Plan.update_values``; include/tilespmv.h tilespmv_plan_update_values).

The contract: a plan created with the flag from values v1 and updated to v2 holds exactly the bytes of a plan created with the flag from v2 — the same stream digests, the same facts,
bit-identical y where the sums have a fixed order — in every form a device-built plan can take; and the flag changes nothing else."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
from tilespmv_amd import api, generators as G  # noqa: E402

pytestmark = pytest.mark.gpu

FACTS = ["device_bytes", "stream_bytes", "nnz", "rows", "tiles", "coo_mode", "dense_mode", "kernel", "num_tasks", "num_split_rows", "entry_mode", "entry_ordered", "strip_cost", "wg_strips",
         "list_entries", "derived_units", "brick_order", "desc_bytes", "nt_stream", "x_panels", "x_panel_merge", "scattered_entries", "x_slice_passes", "csr_form", "value_map_bytes"]
# every form of a device-built plan: classic units (12-B and dictionary descriptors, derived units, absorbed entries 0 / 1 / 2), pooled / pooled-dictionary / wide pooled units,
# entry modes 0 / 1 / 2, column panels, XCD column slices, split tile-rows (inline and by k_fixup_split), dense tiles on the matrix cores, brick order, reproducible sums
KNOBS = [dict(), dict(csr_split=1), dict(csr_split=1, absorb=0), dict(csr_split=1, absorb=2), dict(csr_split=1, desc_dict=0), dict(csr_split=1, desc_dict=1),
         dict(csr_split=2), dict(csr_split=2, desc_dict=0), dict(csr_split=2, desc_dict=2), dict(csr_split=3), dict(entry_mode=0), dict(entry_mode=1), dict(entry_mode=2),
         dict(entry_mode=2, x_panel_kb=1, x_panel_merge=1), dict(entry_mode=2, x_panel_kb=1, x_panel_merge=0, x_slice_passes=1), dict(strip_cost=64, split_above=200, fix_inline=1),
         dict(strip_cost=64, split_above=200, fix_inline=0), dict(csr_split=2, strip_cost=64, split_above=128, dense_mode=1), dict(dense_mode=1), dict(x_window=2), dict(deterministic=1)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spmv(torch, plan, rows, x, stream=None):
    xd = _dev(torch, x)
    yd = torch.full((rows + 16,), 12345.0, dtype=xd.dtype, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), stream or torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[rows:] == 12345.0).all()
    return y[:rows]


def _csr_product(rows, cols, rp, ci, v, x):
    import scipy.sparse as sp
    nnz = int(rp[rows])
    A = sp.csr_matrix((np.asarray(v[:nnz], np.float64), np.asarray(ci[:nnz]), np.asarray(rp[:rows + 1])), shape=(rows, cols))
    absA = sp.csr_matrix((np.abs(np.asarray(v[:nnz], np.float64)), np.asarray(ci[:nnz]), np.asarray(rp[:rows + 1])), shape=(rows, cols))
    return A @ np.asarray(x, np.float64), absA @ np.abs(np.asarray(x, np.float64))


def _close_to_csr(y, want, scale, dtype):
    eps = 2e-4 if dtype == np.float32 else 1e-12
    return np.abs(y.astype(np.float64) - want) <= eps * (scale + 1.0)


def refreshed_equals_fresh(torch, rows, cols, rp, ci, dtype, knobs, v1, v2, shard=None, cdna4=False, hyb=False):
    """Flagged plan from v1, updated to v2  ==  flagged plan from v2 (digests, facts, y); y is A(v2) x; rows outside the shard keep their sentinel."""
    nnz = int(rp[rows])
    x = G.real_x(cols, nnz, dtype)
    kw = dict(knobs)
    kw.setdefault("placement_tries", 1)
    if shard:
        kw["tilerow_begin"], kw["tilerow_end"] = shard
    a = api.Plan.from_csr(rows, cols, nnz, rp, ci, v1, dtype=dtype, cdna4=cdna4, hyb=hyb, value_map=True, **kw)
    b = api.Plan.from_csr(rows, cols, nnz, rp, ci, v2, dtype=dtype, cdna4=cdna4, hyb=hyb, value_map=True, **kw)
    try:
        d_v2 = _dev(torch, np.asarray(v2, dtype))
        a.update_values(d_v2.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ai, bi = a.info(), b.info()
        assert ai["value_map_bytes"] > 0 or ai["nnz"] == 0
        bad = [(k, ai[k], bi[k]) for k in FACTS if ai[k] != bi[k]]
        assert bad == [], bad
        ad, bd = a.stream_digests(), b.stream_digests()
        assert sorted(ad) == sorted(bd)
        assert [k for k in ad if ad[k] != bd[k]] == [], {k: (ad[k], bd[k]) for k in ad if ad[k] != bd[k]}
        r0, r1 = (shard[0] * 16, min(rows, shard[1] * 16)) if shard else (0, rows)
        ya, yb = _spmv(torch, a, rows, x), _spmv(torch, b, rows, x)
        if ai["entry_ordered"]:
            assert np.array_equal(ya[r0:r1], yb[r0:r1])
        else:
            assert np.allclose(ya[r0:r1], yb[r0:r1], rtol=1e-4 if dtype == np.float32 else 1e-11, atol=1e-4 if dtype == np.float32 else 1e-11)
        want, scale = _csr_product(rows, cols, rp, ci, np.asarray(v2, dtype), x)
        assert _close_to_csr(ya[r0:r1], want[r0:r1], scale[r0:r1], dtype).all()
        assert (ya[:r0] == 12345.0).all() and (ya[r1:] == 12345.0).all()
        return ai
    finally:
        a.close(); b.close()


def test_contract_on_the_small_and_medium_cases(torch_cuda):
    for i, name in enumerate(sorted(cases.SMALL) + sorted(cases.MEDIUM)):
        rows, cols, rp, ci = (cases.SMALL.get(name) or cases.MEDIUM[name])()
        rows = cases.truncated_rows(rows)
        nnz = int(rp[rows])
        for j in range(4):
            knobs = KNOBS[(3 * i + 5 * j) % len(KNOBS)]
            dtype = np.float64 if (i + j) % 2 == 0 else np.float32
            shard = (rows // 48, max(rows // 48 + 1, 2 * rows // 48)) if j == 3 and rows >= 64 else None
            refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz), shard=shard, hyb=j == 2)


def test_contract_across_forms_on_the_class_set(torch_cuda):
    """The class set of the device-build tests (pooled FEM, shuffled FEM, circuit, 3-D stencil, KKT, power-law, band with dense tiles, R-MAT, 2-D stencil); every knob set once per
    matrix, fp64 and fp32, whole matrix and a shard of tile-rows in turn; CDNA4 selection and HYB tiles on some."""
    mats = {"fem3": G.fem_hex(14, 14, 14, 3), "fem6s": G.fem_hex(10, 10, 10, 6, shuffle=16), "fem3s64": G.fem_hex(16, 16, 16, 3, shuffle=64), "circuit": G.circuit_like(120000), "lap3d": G.laplacian7pt(48), "kkt24": G.kkt_like(24), "powerlaw": G.powerlaw(300000),
            "band40": G.band(60000, 40), "rmat16": G.rmat(16, 8, 3), "lap2d": G.laplacian5pt(500)}
    seen = set()
    for m, (name, (rows, cols, rp, ci)) in enumerate(mats.items()):
        rows = cases.truncated_rows(rows)
        tilem, nnz = rows // 16, int(rp[rows])
        for k, knobs in enumerate(KNOBS):
            dtype = np.float64 if (k + m) % 2 == 0 else np.float32
            shard = (tilem // 3, 2 * tilem // 3) if (k // 2 + m) % 2 else None
            info = refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz), shard=shard,
                                          cdna4=(k + m) % 7 == 3, hyb=(k + m) % 5 == 1)
            seen.add(("csr_form", info["csr_form"])); seen.add(("entry_mode", info["entry_mode"])); seen.add(("dense", info["dense_mode"])); seen.add(("brick", info["brick_order"]))
            seen.add(("derived", info["derived_units"] > 0)); seen.add(("split", info["num_split_rows"] > 0)); seen.add(("slices", info["x_slice_passes"] > 0)); seen.add(("panels", info["x_panels"] > 1))
            seen.add(("dict", info["desc_bytes"]))
    # the forms really occurred
    for want in [("csr_form", 1), ("csr_form", 2), ("csr_form", 3), ("entry_mode", 0), ("entry_mode", 1), ("entry_mode", 2), ("dense", api.DENSE_MFMA), ("brick", 1), ("derived", True),
                 ("split", True), ("slices", True), ("panels", True), ("dict", 4), ("dict", 12)]:
        assert want in seen, (want, sorted(seen))


def hand_matrix():
    """An ELL tile of width 1 whose row 5 holds one entry, at column nibble 0, beside a COO tile with an entry one column to its left: when that entry's value is 0 the unflagged
    builder takes row 5's slot for padding and moves the COO entry into it (plan_tile_ops.h absorb planning); a flagged plan must not."""
    r, c = [], []
    for row in range(16):
        r.append(row); c.append(16 if row == 5 else 16 + row % 8)
    for row, col in ((5, 15), (2, 3), (9, 10)):
        r.append(row); c.append(col)
    for row in range(16, 32):
        r.append(row); c.append(row)
    rows, cols, rp, ci = G.from_coo(32, 32, r, c)
    zero_at = [k for k in range(int(rp[5]), int(rp[6])) if ci[k] == 16][0]
    return rows, cols, rp, ci, zero_at


def test_explicit_zeros_both_ways(torch_cuda):
    for name in ("allfmt", "circuit8k", "band4096_8", "lap64"):
        rows, cols, rp, ci = cases.SMALL[name]()
        rows = cases.truncated_rows(rows)
        nnz = int(rp[rows])
        for dtype, knobs in ((np.float64, dict()), (np.float32, dict(csr_split=1)), (np.float64, dict(entry_mode=2, x_panel_kb=1, x_panel_merge=1)), (np.float32, dict(csr_split=2, entry_mode=1))):
            compat, real = G.compat_values(nnz, dtype), G.real_values(nnz, dtype)
            refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, compat, real)
            refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, real, compat)
    rows, cols, rp, ci, z = hand_matrix()
    nnz = int(rp[rows])
    for dtype in (np.float64, np.float32):
        v = np.arange(1, nnz + 1).astype(dtype)
        vz = v.copy(); vz[z] = 0
        for knobs in (dict(csr_split=1), dict(csr_split=1, absorb=2), dict()):
            iz = refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, v, vz)
            inz = refreshed_equals_fresh(torch_cuda, rows, cols, rp, ci, dtype, knobs, vz, v)
            assert iz["list_entries"] == inz["list_entries"]
        # the hazard is real: unflagged plans of the two value sets differ in where the COO entry went
        p0 = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, csr_split=1, placement_tries=1)
        p1 = api.Plan.from_csr(rows, cols, nnz, rp, ci, vz, dtype=dtype, csr_split=1, placement_tries=1)
        f = api.Plan.from_csr(rows, cols, nnz, rp, ci, vz, dtype=dtype, csr_split=1, placement_tries=1, value_map=True)
        assert p0.info()["list_entries"] == 3 and p1.info()["list_entries"] == 2 and f.info()["list_entries"] == 3
        p0.close(); p1.close(); f.close()


def test_the_flag_changes_nothing_else(torch_cuda):
    mats = [cases.SMALL["allfmt"](), cases.MEDIUM["kkt12"](), G.fem_hex(12, 12, 12, 3), G.powerlaw(100000), G.band(20000, 40)]
    for i, (rows, cols, rp, ci) in enumerate(mats):
        rows = cases.truncated_rows(rows)
        nnz = int(rp[rows])
        for j, knobs in enumerate((dict(), dict(csr_split=1), dict(csr_split=2, entry_mode=2), dict(deterministic=1), dict(dense_mode=1, csr_split=3))):
            dtype = np.float64 if (i + j) % 2 == 0 else np.float32
            v = G.real_values(nnz, dtype)
            p = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, placement_tries=1, **knobs)
            f = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, placement_tries=1, value_map=True, **knobs)
            try:
                pi, fi = p.info(), f.info()
                assert pi["value_map_bytes"] == 0 and fi["value_map_bytes"] > 0
                assert pi["device_bytes"] == fi["device_bytes"]
                assert [(k, pi[k], fi[k]) for k in FACTS if k != "value_map_bytes" and pi[k] != fi[k]] == []
                assert p.stream_digests() == f.stream_digests()
            finally:
                p.close(); f.close()


def test_round_trip_restores_the_first_plan(torch_cuda):
    rows, cols, rp, ci = G.fem_hex(12, 12, 12, 3)
    rows = cases.truncated_rows(rows)
    nnz = int(rp[rows])
    for dtype, knobs in ((np.float64, dict()), (np.float32, dict(csr_split=1, entry_mode=2)), (np.float64, dict(deterministic=1, x_window=2))):
        vs = [G.real_values(nnz, dtype, first=k * nnz) for k in range(3)]
        p = api.Plan.from_csr(rows, cols, nnz, rp, ci, vs[0], dtype=dtype, value_map=True, placement_tries=1, **knobs)
        d0 = p.stream_digests()
        for v in (vs[1], vs[2], vs[0]):
            dv = _dev(torch_cuda, v)
            p.update_values(dv.data_ptr())
            torch_cuda.cuda.synchronize()
        assert p.stream_digests() == d0
        p.close()


def test_stream_order_on_one_stream(torch_cuda):
    """spmv, update_values, spmv on one non-default stream, one synchronisation at the end: the first y has the old values, the second the new."""
    torch = torch_cuda
    rows, cols, rp, ci = G.kkt_like(16)
    rows = cases.truncated_rows(rows)
    nnz = int(rp[rows])
    for dtype in (np.float64, np.float32):
        v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
        x = G.real_x(cols, nnz, dtype)
        p = api.Plan.from_csr(rows, cols, nnz, rp, ci, v1, dtype=dtype, value_map=True, placement_tries=1)
        s = torch.cuda.Stream()
        xd, dv2 = _dev(torch, x), _dev(torch, v2)
        y1 = torch.zeros(rows + 16, dtype=xd.dtype, device="cuda"); y2 = torch.zeros_like(y1)
        torch.cuda.synchronize()
        p.spmv(xd.data_ptr(), y1.data_ptr(), s.cuda_stream)
        p.update_values(dv2.data_ptr(), s.cuda_stream)
        p.spmv(xd.data_ptr(), y2.data_ptr(), s.cuda_stream)
        s.synchronize()
        for y, v in ((y1, v1), (y2, v2)):
            want, scale = _csr_product(rows, cols, rp, ci, v, x)
            assert _close_to_csr(y.cpu().numpy()[:rows], want, scale, dtype).all()
        p.close()


def test_refusals(torch_cuda):
    rows, cols, rp, ci = cases.SMALL["allfmt"]()
    rows = cases.truncated_rows(rows)
    nnz = int(rp[rows])
    v = G.real_values(nnz, np.float64)
    dv = _dev(torch_cuda, G.real_values(nnz, np.float64, first=nnz))
    tm = api.Tile_create(rows, cols, nnz, rp, ci, v)
    for p in (api.Plan.from_csr(rows, cols, nnz, rp, ci, v, placement_tries=1), api.Plan(tm, rows, cols, nnz, placement_tries=1)):
        d0 = p.stream_digests()
        assert p.lib.tilespmv_plan_update_values(p.h, C.c_void_p(dv.data_ptr()), None) == api.ERR_NO_VALUE_MAP
        with pytest.raises(RuntimeError):
            p.update_values(dv.data_ptr())
        torch_cuda.cuda.synchronize()
        assert p.stream_digests() == d0 and p.info()["value_map_bytes"] == 0
        p.close()
    api.Tile_destroy(tm)
    for knobs in (dict(csr_split=0), dict(kernel=api.KERNEL_DIRECT), dict(coo_mode=api.COO_FALLBACK)):
        with pytest.raises(NotImplementedError):
            api.Plan.from_csr(rows, cols, nnz, rp, ci, v, value_map=True, **knobs)


def test_device_csr_autotune_and_sharded(torch_cuda):
    """from_device_csr with the flag (the map indexes the caller's device array); autotune builds the map for the plan it keeps; ShardedSpMV hands each rank its block."""
    torch = torch_cuda
    from tilespmv_amd.dist import ShardedSpMV
    rows, cols, rp, ci = G.fem_hex(10, 10, 10, 3)
    rows = cases.truncated_rows(rows)
    rp = np.ascontiguousarray(rp[:rows + 1], np.int32)
    nnz = int(rp[rows])
    ci = np.ascontiguousarray(ci[:nnz], np.int32)
    for dtype in (np.float64, np.float32):
        v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
        x = G.real_x(cols, nnz, dtype)
        want, scale = _csr_product(rows, cols, rp, ci, v2, x)
        drp, dci, dv1, dv2 = _dev(torch, rp), _dev(torch, ci), _dev(torch, v1), _dev(torch, v2)
        p = api.Plan.from_device_csr(rows, cols, nnz, drp.data_ptr(), dci.data_ptr(), dv1.data_ptr(), dtype, value_map=True, placement_tries=1)
        q = api.Plan.from_csr(rows, cols, nnz, rp, ci, v2, dtype=dtype, value_map=True, placement_tries=1)
        p.update_values(dv2.data_ptr())
        torch.cuda.synchronize()
        assert p.stream_digests() == q.stream_digests()
        assert _close_to_csr(_spmv(torch, p, rows, x), want, scale, dtype).all()
        p.close(); q.close()
        t = api.Plan.from_csr(rows, cols, nnz, rp, ci, v1, dtype=dtype, value_map=True, autotune=True)
        t.update_values(dv2.data_ptr())
        assert t.info()["value_map_bytes"] > 0
        assert _close_to_csr(_spmv(torch, t, rows, x), want, scale, dtype).all()
        t.close()
        for rank in range(2):
            sh = ShardedSpMV(rank, 2, rows, cols, rp, ci, v1, dtype=dtype, device_build=True, value_map=True, placement_tries=1)
            sh.update_values(dv2)
            xd = _dev(torch, x)
            y = torch.full((rows + 16,), 12345.0, dtype=xd.dtype, device="cuda")
            sh.spmv(xd, y)
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert _close_to_csr(yh[sh.r0:sh.r1], want[sh.r0:sh.r1], scale[sh.r0:sh.r1], dtype).all()
            assert (yh[:sh.r0] == 12345.0).all() and (yh[sh.r1:] == 12345.0).all()
            sh.close()


@pytest.mark.parametrize("workload", ["laplacian4096", "nlpkkt160"])
def test_full_size(torch_cuda, workload):
    """Config 4 (fp64) and the config 5 / nlpkkt160 stand-in (fp32): update to new values, then the whole y against the CSR product with them."""
    torch = torch_cuda
    if workload == "laplacian4096":
        rows, cols, rp, ci = G.laplacian5pt(4096); dtype = np.float64
    else:
        rows, cols, rp, ci = G.nlpkkt_like(160); dtype = np.float32
    rows = cases.truncated_rows(rows)
    nnz = int(rp[rows])
    v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
    x = G.real_x(cols, nnz, dtype)
    p = api.Plan.from_csr(rows, cols, nnz, rp, ci, v1, dtype=dtype, value_map=True, placement_tries=1)
    del v1
    dv2 = _dev(torch, v2)
    p.update_values(dv2.data_ptr())
    y = _spmv(torch, p, rows, x)
    p.close()
    del dv2
    want, scale = _csr_product(rows, cols, rp, ci, v2, x)
    ok = _close_to_csr(y, want, scale, dtype)
    assert ok.all(), (int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
