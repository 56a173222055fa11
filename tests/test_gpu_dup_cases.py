"""CSR input with repeated (i, j) entries on the GPU (tests/dup_cases.py has the cases, tests/test_dup_cases_cpu.py what they reach and the host half).  The contract
(include/tilespmv.h "Repeated entries"): y is the sum over ALL stored entries on every path; a tile that stores a position twice is never DNS / DNSROW / DNSCOL; a tile with
a repeated position and more than 255 entries is refused with -2 before anything is packed.  Every served case is built by both builders — the host Tile_matrix and
Plan.from_csr — which must make the same streams; SpMV and SpMM are compared with an integer golden (tests/witness.py: exact in any order, so np.array_equal and no
tolerance anywhere); a sentinel behind y must survive; every third case also runs its middle third as a shard.  Transposed and value-mapped plans, Tile_create_device
against the host's bytes, and the two refusals have tests of their own."""
import ctypes as C

import numpy as np
import pytest

import dup_cases as D
from witness import golden

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e30
CREATE = [dict(), dict(hyb=True), dict(cdna4=True), dict(transpose=True)]


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_cross_forms.py)"""
    import torch
    torch.zeros(1, device="cuda")
    yield


@pytest.fixture(scope="module")
def served():
    cs = D.served_cases()
    assert len(cs) == len(D.PLANTED) - 2 + len(D.SWEEP_SEEDS) >= 50        # every planted matrix but the two refused ones, and the sweep
    return cs


def _run(torch, plan, Xh, rows, dtype, nvec, shard=None):
    """[y of SpMV on column 0, Y of SpMM when nvec > 1] over the rows the plan must write, after the sentinel checks; and those rows"""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    room = 16 * ((rows + 15) // 16)
    b, e = (16 * shard[0], 16 * shard[1]) if shard else (0, room)             # what the header lets the plan write
    lo, hi = b, min(e, rows)
    out = []
    for nv in ([1] if nvec == 1 else [1, nvec]):
        xh = np.ascontiguousarray(Xh if Xh.ndim == 1 else (Xh[:, 0] if nv == 1 else Xh))
        xd = torch.from_numpy(xh).cuda()
        yd = torch.full((room + 16,) if nv == 1 else (room + 16, nv), SENTINEL, dtype=tdt, device="cuda")
        if nv == 1:
            plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
        else:
            plan.spmm(xd.data_ptr(), yd.data_ptr(), nv, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        s = np.asarray(SENTINEL, dtype=dtype)
        assert (y[:b] == s).all() and (y[e:] == s).all(), "wrote outside y[%d .. %d)" % (b, e)
        out.append(y[lo:hi])
    return out, (lo, hi)


def _check(c, what, got, want, win):
    lo, hi = win
    w = want if want.ndim == 2 else want[:, None]
    assert np.array_equal(got[0], w[lo:hi, 0]), (c, what, "SpMV", int(np.count_nonzero(got[0] != w[lo:hi, 0])))
    if len(got) > 1:
        bad = [j for j in range(w.shape[1]) if not np.array_equal(got[1][:, j], w[lo:hi, j])]
        assert bad == [], (c, what, "SpMM columns", bad)


def _same_streams(a, b, c, what):
    da, db = a.stream_digests(), b.stream_digests()
    assert sorted(da) == sorted(db) and [k for k in da if da[k] != db[k]] == [], (c, what, "host-built and device-built streams differ")


def _windows(c):
    return [None] + ([c.shard] if c.shard else [])


@pytest.mark.parametrize("opt", sorted(D.OPTIONS))
def test_both_builders_make_the_same_plan_and_the_exact_product(served, opt):
    import torch
    from tilespmv_amd import api
    narrow = "value_narrow" in D.OPTIONS[opt]
    for c in served:
        kind, dtype = ("half", np.float64) if narrow else (c.kind, c.dtype)       # value_narrow = 2 gets halves
        vals, Xh = c.data(kind=kind)
        want = golden(c.rowA, c.rp, c.ci, vals, Xh)
        kw = dict(D.OPTIONS[opt], **D.COMMON)
        if c.nvec > 1:
            kw["mv_native"] = c.mv_native
        tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, hyb=c.hyb)
        for w in _windows(c):
            k = dict(kw, tilerow_begin=w[0], tilerow_end=w[1]) if w else kw
            host = api.Plan(tm, c.rowA, c.colA, c.nnz, **k)
            dev = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, hyb=c.hyb, **k)
            assert dev.info()["device_build"] == 1 and host.info()["device_build"] == 0
            _same_streams(host, dev, c, (opt, w))
            got, win = _run(torch, dev, Xh, c.rowA, dtype, c.nvec, w)
            _check(c, (opt, w), got, want, win)
            if narrow:                                                           # the value_narrow = 0 twin: the same y in every bit
                wide = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, hyb=c.hyb, **dict(k, value_narrow=0))
                assert wide.info()["unit_value_bytes"] == 8
                gw, _ = _run(torch, wide, Xh, c.rowA, dtype, c.nvec, w)
                assert all(g.tobytes() == x.tobytes() for g, x in zip(got, gw)), (c, opt, "narrow and wide plan differ")
                wide.close()
            host.close(); dev.close()
        api.Tile_destroy(tm)


@pytest.mark.parametrize("opt", sorted(D.HOST_ONLY))
def test_forms_without_a_device_builder(served, opt):
    """the first-generation kernel, the CSR fallback for the extracted entries and whole CSR tiles: host-built plans only, SpMV only (they have no multi-vector kernel)"""
    import torch
    from tilespmv_amd import api
    for c in served:
        vals, Xh = c.data()
        x = Xh if Xh.ndim == 1 else np.ascontiguousarray(Xh[:, 0])
        want = golden(c.rowA, c.rp, c.ci, vals, x)
        tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb)
        for w in _windows(c):
            k = dict(D.HOST_ONLY[opt], **D.COMMON)
            if w:
                k.update(tilerow_begin=w[0], tilerow_end=w[1])
            plan = api.Plan(tm, c.rowA, c.colA, c.nnz, **k)
            got, win = _run(torch, plan, x, c.rowA, c.dtype, 1, w)
            _check(c, (opt, w), got, want, win)
            plan.close()
        api.Tile_destroy(tm)


def test_transposed_plans(served):
    import torch
    from tilespmv_amd import api
    for c in served:
        vals, Xh = c.data(cols=c.rowA)
        want = golden(c.rowA, c.rp, c.ci, vals, Xh, transpose_cols=c.colA)
        kw = dict(D.COMMON, **({"mv_native": c.mv_native} if c.nvec > 1 else {}))
        dev = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb, transpose=True, **kw)
        tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb, transpose=True)
        host = api.Plan(tm, c.colA, c.rowA, c.nnz, **kw)
        _same_streams(host, dev, c, "transpose")
        got, win = _run(torch, dev, Xh, c.colA, c.dtype, c.nvec)
        _check(c, "transpose", got, want, win)
        host.close(); dev.close(); api.Tile_destroy(tm)


@pytest.mark.parametrize("transpose", [False, True])
def test_value_mapped_plans_before_and_after_update_values(served, transpose):
    """update_values to a second witness gives the streams and the y of a plan created from the second values: every stored entry, repeats included, has a slot of its own"""
    import torch
    from tilespmv_amd import api
    for c in served:
        rows, cols = (c.colA, c.rowA) if transpose else (c.rowA, c.colA)
        vals, Xh = c.data(cols=cols)
        vals2, _ = c.data(second=True, cols=cols)
        assert not np.array_equal(vals, vals2)
        tc = c.colA if transpose else None
        kw = dict(D.COMMON, **({"mv_native": c.mv_native} if c.nvec > 1 else {}))
        plan = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb, transpose=transpose, value_map=True, **kw)
        assert plan.info()["value_map_bytes"] > 0
        got, win = _run(torch, plan, Xh, rows, c.dtype, c.nvec)
        _check(c, "value map", got, golden(c.rowA, c.rp, c.ci, vals, Xh, transpose_cols=tc), win)
        d2 = torch.from_numpy(np.ascontiguousarray(vals2)).cuda()
        plan.update_values(d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fresh = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals2, dtype=c.dtype, hyb=c.hyb, transpose=transpose, value_map=True, **kw)
        _same_streams(fresh, plan, c, "after update_values")
        got2, _ = _run(torch, plan, Xh, rows, c.dtype, c.nvec)
        _check(c, "after update_values", got2, golden(c.rowA, c.rp, c.ci, vals2, Xh, transpose_cols=tc), win)
        plan.close(); fresh.close()


@pytest.mark.parametrize("kw", CREATE, ids=["plain", "hyb", "cdna4", "transpose"])
def test_device_tile_create_gives_the_hosts_bytes(served, kw):
    from tilespmv_amd import api
    for c in served:
        vals, _ = c.data()
        k = dict(kw, hyb=c.hyb or kw.get("hyb", False))
        host = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, **k)
        dev = api.Tile_create_device(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, **k)
        rows = c.colA if kw.get("transpose") else c.rowA
        h, d = api.to_dict(host, rows), api.to_dict(dev, rows)
        bad = [key for key in h if (h[key].tobytes() != d[key].tobytes() if isinstance(h[key], np.ndarray) else h[key] != d[key])]
        assert bad == [], (c, kw, bad)
        api.Tile_destroy(host); api.Tile_destroy(dev)


@pytest.mark.parametrize("name", ["csr_256", "row_of_256"])
def test_refused_matrices_return_minus_two_and_build_nothing(name):
    """the selection kernel decides, the status comes back with the scans' totals, and the packing kernel is not launched: no Tile_matrix, no plan handle"""
    from tilespmv_amd import _lib, api
    c = D.Case(name)
    assert c.outcome == D.REFUSED
    vals, _ = c.data(kind="half")
    lib = _lib.load(np.float64)
    rp, ci, v = api._csr(lib, c.rp, c.ci, vals)
    for flags in (api.CREATE_QUIET, api.CREATE_QUIET | api.CREATE_HYB, api.CREATE_QUIET | api.CREATE_CDNA4, api.CREATE_QUIET | api.CREATE_TRANSPOSE):
        tm = lib._TM()
        blank = bytes(tm)
        rc = lib.Tile_create_device(C.byref(tm), c.rowA, c.colA, c.nnz, api._p(rp, C.c_int), api._p(ci, C.c_int), api._p(v, lib._vt), flags)
        assert rc == -2 and bytes(tm) == blank, (name, flags, rc)
        for extra in (0, api.CREATE_VALUE_MAP):
            opts = _lib.PlanOptions(**D.COMMON)
            h = C.c_void_p()
            rc = lib.tilespmv_plan_create_from_csr(C.byref(h), c.rowA, c.colA, c.nnz, api._p(rp, C.c_int), api._p(ci, C.c_int), api._p(v, lib._vt), flags | extra, C.byref(opts))
            assert rc == -2 and not h, (name, flags, extra, rc)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals)
