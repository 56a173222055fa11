"""The lean forms of the unit kernel (tilespmv_plan_options.unit_lean, csrc/hip_kernels_lean.hip): a classic plan with nontemporal streams in which no unit is a row unit runs
k_units_lean — nothing a row unit needs, with no derived unit in the plan nothing a derived unit needs either, and a unit loop that tests the task's end once per task.  Same
plan, same streams, same multiply-then-add in unit order, so y must keep EVERY bit: each case compares the whole y of the lean launch with the y of the general launch of the
same plan options (unit_lean = 0) by np.array_equal, checks the sentinel behind y, and compares with the oracle inside the parity tests' tolerance (TOL x sum |a_ij x_j|).
x is U(-1, 1) throughout; the values are the compat data and U(-1, 1) rounded to what the value form stores.  Every case runs host-built and device-built plans, which must
report the same TILESPMV_INFO_UNIT_LEAN and give bit-equal y, with 12-byte and dictionary descriptors.  Small plans reach the lean kernels through nt_stream = 1.

Shapes, the smallest where each thing can go wrong: 5-point 48^2 (derived units, absorbed corners, no entries; strips of 8 tile-rows = 40 units cross two descriptor chunks);
5-point 47 columns x 48 lines (2256 rows = 141 tile-rows: the last strip is a partial one, five corners stay on the lists); 7-point 16^3; the KKT-like generator at g = 4, its
smallest size with units AND list entries and no derived unit, in entry modes 0 and 2; a tridiagonal band of 64 tile-rows with 3 units per tile-row cut into strips of 1, 2, 3
and 4 tile-rows — 3, 6, 9 and 12 units per task, every residue mod 4 of the peeled loop (the strip counts pin the cut); one tile-row of 16 rows and 3 units (the peeled batch
alone); the all-formats matrix (dense-row tiles: general kernel, info 0); a band of half-width 40 with split tile-rows (the in-kernel piece sum)."""
import numpy as np
import pytest

from cases import truncated_rows

pytestmark = pytest.mark.gpu

COMMON = dict(placement_tries=1, deterministic=1, nt_stream=1)
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # (tests/test_gpu_parity.py)
# value form -> (library, value_narrow, bytes per stored unit value)
FORMS = {"wide": (np.float64, 0, 8), "floats": (np.float64, 1, 4), "halves": (np.float64, 2, 2), "f32": (np.float32, 0, 4)}


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_unit_loop.py): the other way round PyTorch finds no GPU in this process."""
    import torch
    torch.zeros(1, device="cuda")
    yield


def _grid5(nx, ny):
    """5-point stencil on a grid of ny lines of nx points (row-major)."""
    from tilespmv_amd import generators as G
    idx = np.arange(nx * ny, dtype=np.int64)
    i, j = idx // nx, idx % nx
    cand = np.stack([idx - nx, idx - 1, idx, idx + 1, idx + nx], axis=1)
    mask = np.stack([i > 0, j > 0, np.ones(idx.size, bool), j < nx - 1, i < ny - 1], axis=1)
    rp, ci = G._from_mask(cand, mask)
    return nx * ny, nx * ny, rp, ci


def _cases():
    from tilespmv_amd import api, generators as G
    band = lambda sc, tasks: dict(gen=lambda: G.band(1024, 1), kw=[dict(entry_mode=0, strip_even=0, strip_cost=sc)], lean=None, facts=dict(num_tasks=tasks))
    return {
        "lap48": dict(gen=lambda: G.laplacian5pt(48), kw=[{}], lean=1, facts=dict(list_entries=0, derived_units=239)),
        "lap47x48": dict(gen=lambda: _grid5(47, 48), kw=[{}], lean=None, facts=dict(rows=2256)),
        "lap7pt16": dict(gen=lambda: G.laplacian7pt(16), kw=[{}], lean=None, facts={}),
        "kkt4": dict(gen=lambda: G.kkt_like(4), kw=[dict(entry_mode=0), dict(entry_mode=2)], lean=2, facts=dict(derived_units=0, list_entries=120, csr_form=1)),
        "band_3_units": band(100, 64), "band_6_units": band(128, 32), "band_9_units": band(200, 22), "band_12_units": band(256, 16),
        "one_tile_row": dict(gen=lambda: G.band(16, 1, 64), kw=[dict(entry_mode=0)], lean=None, facts=dict(num_tasks=1, rows=16)),
        "all_formats": dict(gen=lambda: G.all_formats(12, 7), hyb=True, kw=[dict(csr_split=1, entry_mode=0), dict(csr_split=1, entry_mode=2)], lean=0, facts={}),
        "split_rows": dict(gen=lambda: G.band(3000, 40), kw=[dict(dense_mode=api.DENSE_VALU, entry_mode=0, split_above=200, strip_cost=32)], lean=None, facts=dict(num_split_rows=187)),
    }


CASE_NAMES = ["lap48", "lap47x48", "lap7pt16", "kkt4", "band_3_units", "band_6_units", "band_9_units", "band_12_units", "one_tile_row", "all_formats", "split_rows"]


def _value_sets(form, nnz, n):
    """[(values, x, what)]: compat values and U(-1, 1) values as the form stores them exactly (floats: rounded to float32; halves: rounded to a NORMAL binary16), x = U(-1, 1)."""
    from tilespmv_amd import generators as G
    dtype = FORMS[form][0]
    rng = np.random.default_rng(20261019)
    x = rng.uniform(-1, 1, n).astype(dtype)
    u = rng.uniform(-1, 1, nnz)
    if form == "floats":
        u = u.astype(np.float32).astype(np.float64)
    elif form == "halves":
        u = u.astype(np.float16).astype(np.float64)
        u[np.abs(u) < 2.0 ** -14] = 2.0 ** -14                       # (a denormal half is no value the 2-byte form takes)
    return [(G.compat_values(nnz, dtype), x, "compat"), (u.astype(dtype), x, "uniform")]


def _run(plan, x, rows):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((rows + 16,), 777.0, dtype=xd.dtype, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[rows:] == 777.0).all(), "wrote past the end of y"
    return y[:rows]


def _abs_bound(rowA, rp, ci, vals, x):
    nz = int(rp[rowA])
    ri = np.repeat(np.arange(rowA), np.diff(rp[:rowA + 1]))
    out = np.zeros(rowA)
    np.add.at(out, ri, np.abs(vals[:nz].astype(np.float64) * x[ci[:nz]].astype(np.float64)))
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_lean_launch_equals_general_launch(name, form):
    from oracle.oracle import CpuImpl
    from tilespmv_amd import api
    c = _cases()[name]
    dtype, narrow, vbytes = FORMS[form]
    hyb = c.get("hyb", False)
    m, n, rp, ci = c["gen"]()
    nnz, rowA = len(ci), truncated_rows(m)
    O = CpuImpl("oracle", dtype)
    for vals, x, what in _value_sets(form, nnz, n):
        want = O.spmv(O.tile_create(rowA, n, nnz, rp, ci, vals, hyb=hyb), rowA, n, nnz, rp, ci, vals, x)["y"].astype(np.float64)
        bound = TOL[np.dtype(dtype)] * _abs_bound(rowA, rp, ci, vals, x) + 1e-300
        tm = api.Tile_create(rowA, n, nnz, rp, ci, vals, dtype=dtype, hyb=hyb)
        for kw0 in c["kw"]:
            for desc_dict in (0, 1):
                kw = dict(COMMON, value_narrow=narrow, desc_dict=desc_dict, **kw0)
                tag = (name, form, what, kw0, desc_dict)
                plans = {("host", lean): api.Plan(tm, rowA, n, nnz, unit_lean=lean, **kw) for lean in (1, 0)}
                plans.update({("device", lean): api.Plan.from_csr(rowA, n, nnz, rp, ci, vals, dtype=dtype, hyb=hyb, unit_lean=lean, **kw) for lean in (1, 0)})
                info = {k: p.info() for k, p in plans.items()}
                ih = info[("host", 1)]
                print(tag, {k: ih[k] for k in ("unit_lean", "entry_mode", "num_tasks", "list_entries", "derived_units", "desc_bytes", "unit_value_bytes", "nt_stream")})
                assert (ih["unit_value_bytes"], ih["nt_stream"], ih["desc_bytes"]) == (vbytes, 1, 4 if desc_dict else 12), (tag, ih)
                for k, v in c["facts"].items():
                    assert ih[k] == v, (tag, k, ih[k])
                if "entry_mode" in kw0:
                    assert ih["entry_mode"] == kw0["entry_mode"], tag
                assert info[("host", 0)]["unit_lean"] == info[("device", 0)]["unit_lean"] == 0, tag               # knob value 0: the general kernel
                assert ih["unit_lean"] == info[("device", 1)]["unit_lean"], tag                                   # both builders find the same facts
                if c["lean"] is None:
                    assert ih["unit_lean"] > 0, (tag, ih["unit_lean"])                                            # (no dense-row tile in the matrix: a lean form)
                else:
                    assert ih["unit_lean"] == c["lean"], (tag, ih["unit_lean"])
                for k in ("num_tasks", "num_split_rows", "list_entries", "derived_units", "desc_bytes", "entry_mode", "csr_form", "stream_bytes"):
                    assert len({i[k] for i in info.values()}) == 1, (tag, k)
                assert plans[("host", 1)].stream_digests() == plans[("host", 0)].stream_digests() == plans[("device", 1)].stream_digests(), tag   # the same plan, byte for byte
                y = {k: _run(p, x, rowA) for k, p in plans.items()}
                for p in plans.values():
                    p.close()
                ref = y[("host", 0)]
                for k, got in y.items():
                    assert np.array_equal(got, ref), (tag, k, int(np.count_nonzero(got != ref)))                  # whole y, every bit
                err = np.abs(ref.astype(np.float64) - want)
                assert (err <= bound).all(), (tag, float((err / bound).max()))
        api.Tile_destroy(tm)
