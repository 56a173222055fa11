"""Cross-feature parity sweep on random matrices (tests/cross_forms.py has the cases, tests/test_cross_forms_cpu.py what they reach): device-built, transposed, value-mapped,
absorbed / derived, narrow-valued and sharded plans, SpMV and SpMM, on matrices with partial last tile-rows and tile-columns, HYB on for odd seeds.  The data
(tests/witness.py) is exact in any summation order, so every y — fp64 and fp32, every SpMM column — is compared with np.array_equal against an integer golden:
there is no tolerance in this file.  Behind y a sentinel must survive from the next tile-row boundary on (y[16 * tilerow_begin .. 16 * tilerow_end) is what
include/tilespmv.h lets a plan write), and a shard leaves every row outside its window alone."""
import time

import numpy as np
import pytest

import cross_forms as X
from witness import golden

pytestmark = pytest.mark.gpu

FACTS = ("nnz", "rows", "tiles", "num_tasks", "num_split_rows", "entry_mode", "desc_bytes", "unit_value_bytes", "list_entries", "derived_units", "csr_form")


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_value_half.py): the other way round PyTorch finds no GPU in this process."""
    import torch
    torch.zeros(1, device="cuda")
    yield


def _build(api, c, vals, device, **over):
    """The case's plan from one of the two builders; (plan, host Tile_matrix or None)."""
    kw = dict(c.plan_kw, **over)
    if device:
        return api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb, transpose=c.transpose, value_map=c.value_map, **kw), None
    tm = X.host_tile_matrix(api, c, vals)
    return api.Plan(tm, c.rows, c.cols, c.nnz, **kw), tm


def _run(torch, c, plan, Xh):
    """y of the plan's window (SpMV on column 0, then SpMM on all columns when the case has several), after the sentinel checks."""
    tdt = torch.float64 if c.dtype == np.float64 else torch.float32
    sentinel = -7.5e30
    room = 16 * ((c.rows + 15) // 16)
    b, e = (16 * c.shard[0], 16 * c.shard[1]) if c.shard else (0, room)          # what the header lets the plan write
    lo, hi = b, min(e, c.rows)                                                   # the rows it must write
    out = []
    for nv in ([1] if c.nvec == 1 else [1, c.nvec]):
        xh = np.ascontiguousarray(Xh if Xh.ndim == 1 else (Xh[:, 0] if nv == 1 else Xh))
        xd = torch.from_numpy(xh).cuda()
        yd = torch.full((room + 16,) if nv == 1 else (room + 16, nv), sentinel, dtype=tdt, device="cuda")
        if nv == 1:
            plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
        else:
            plan.spmm(xd.data_ptr(), yd.data_ptr(), nv, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        s = np.asarray(sentinel, dtype=c.dtype)
        assert (y[:b] == s).all() and (y[e:] == s).all(), (c, nv, "wrote outside y[%d .. %d)" % (b, e))
        out.append(y[lo:hi])
    return out, (lo, hi)


def _check(c, got, want, win, what):
    lo, hi = win
    w = want if want.ndim == 2 else want[:, None]
    assert np.array_equal(got[0], w[lo:hi, 0]), (c, what, "SpMV", int(np.count_nonzero(got[0] != w[lo:hi, 0])))
    if c.nvec > 1:
        bad = [j for j in range(c.nvec) if not np.array_equal(got[1][:, j], w[lo:hi, j])]
        assert bad == [], (c, what, "SpMM columns", bad)


@pytest.mark.parametrize("group", range(len(X.GROUPS)))
def test_every_form_gives_the_exact_product(group):
    import torch
    from tilespmv_amd import api
    for seed in X.GROUPS[group]:
        t0 = time.time()
        c = X.Case(seed)
        vals, Xh = c.data()
        want = golden(c.rowA, c.rp, c.ci, vals, Xh, transpose_cols=c.colA if c.transpose else None)
        predicted = X.layout_facts(api, c)                                    # host layout builder: what the CPU ledger counted
        plan, tm = _build(api, c, vals, c.device_build)
        info = plan.info()
        assert info["device_build"] == int(c.device_build)
        if c.value_map:
            assert info["unit_value_bytes"] == 8 and info["value_map_bytes"] > 0, (c, info)       # a flagged plan's layout follows the pattern alone
        else:
            assert [(k, info[k], predicted[k]) for k in FACTS if info[k] != predicted[k]] == [], c
            if c.wants_two_bytes():
                assert info["unit_value_bytes"] == predicted["unit_value_bytes"], c
            # the other builder makes the same streams
            other, tm2 = _build(api, c, vals, not c.device_build)
            a, b = plan.stream_digests(), other.stream_digests()
            assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == [], (c, "host-built and device-built streams differ")
            other.close()
            if tm2 is not None:
                api.Tile_destroy(tm2)
        got, win = _run(torch, c, plan, Xh)
        _check(c, got, want, win, "plan")
        if c.narrow:                                                          # the value_narrow = 0 plan of the same options: the same y in every bit
            wide, tm3 = _build(api, c, vals, c.device_build, value_narrow=0)
            assert wide.info()["unit_value_bytes"] == 8
            gw, _ = _run(torch, c, wide, Xh)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, gw)), (c, "narrow and wide plan differ")
            wide.close()
            if tm3 is not None:
                api.Tile_destroy(tm3)
        if c.value_map:                                                       # new values of the same pattern, written in place
            vals2, _ = c.data(second=True)
            assert not np.array_equal(vals2, vals)
            d2 = torch.from_numpy(np.ascontiguousarray(vals2)).cuda()
            plan.update_values(d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            want2 = golden(c.rowA, c.rp, c.ci, vals2, Xh, transpose_cols=c.colA if c.transpose else None)
            got2, _ = _run(torch, c, plan, Xh)
            _check(c, got2, want2, win, "after update_values")
            assert plan.info()["unit_value_bytes"] == 8
        plan.close()
        if tm is not None:
            api.Tile_destroy(tm)
        print("seed %d: %.2f s" % (seed, time.time() - t0))
