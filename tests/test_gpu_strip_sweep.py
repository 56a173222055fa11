"""Strided strips on the GPU (environment knob TILESPMV_STRIP_SWEEP, tilespmv_plan_strip_stride; csrc/hip_plan_stream.hip strip_sweep_stride).  A strided plan holds the units,
values and task records of the unstrided plan in another order and every kernel turns (strip, tile-row in strip) into rows through the stride, so y must keep EVERY bit: each
case builds the plan with the knob at 0 and at 1, on the host and on the device, with 12-byte and dictionary descriptors, and compares the whole y of every plan with the
host-built knob-0 plan's by np.array_equal, checks the sentinel behind y, and compares with the oracle inside the parity tests' tolerance (TOL x sum |a_ij x_j|,
tests/test_gpu_parity.py).  The two builders must agree stream for stream under either knob value.  x is U(-1, 1); the values are the compat data and U(-1, 1) rounded to what
the value form stores.  Small plans reach the rule through nt_stream = 1 (and run the lean kernels).

Shapes: 5-point 64^2 (256 tile-rows, lines of 4: S = 4, blocks of 32 tile-rows); 5-point 48^2 (S = 3; 144 tile-rows = 6 blocks); rows 592 .. 3376 of the 64^2 grid (174 tile-rows
numbered from an origin that is not the columns': the first line has no "up", the last block is a partial one of 14 tile-rows); 7-point 16^3 (lines one tile-row long), 5-point
40^2 (lines of 2.5 tile-rows) and a power-law matrix of 4096 rows: S = 1 and the knob-1 plan IS the knob-0 plan, stream for stream.  On the S = 4 case also: the multi-vector
product with 4 vectors, values refreshed in place followed by a product, the transposed plan, and unit_lean = 0 (the general kernel on a strided plan)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMMON = dict(placement_tries=1, deterministic=1, nt_stream=1)
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # (tests/test_gpu_parity.py)
FORMS = {"wide": (np.float64, 0, 8), "floats": (np.float64, 1, 4), "halves": (np.float64, 2, 2), "f32": (np.float32, 0, 4)}   # value form -> (library, value_narrow, bytes per stored unit value)
CASES = {"lap64": 4, "lap48": 3, "lap64_rows_592_3376": 4, "lap7pt16": 1, "lap40": 1, "powerlaw4096": 1}   # case -> the stride S the knob at 1 must give


def _gen(name):
    from tilespmv_amd import generators as G
    return {"lap64": lambda: G.laplacian5pt(64), "lap48": lambda: G.laplacian5pt(48), "lap64_rows_592_3376": lambda: G.laplacian5pt(64, rows=(16 * 37, 16 * 211)),
            "lap7pt16": lambda: G.laplacian7pt(16), "lap40": lambda: G.laplacian5pt(40), "powerlaw4096": lambda: G.powerlaw(4096)}[name]()


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_unit_lean.py)."""
    import torch
    torch.zeros(1, device="cuda")
    yield


_MATRIX = {}


def _matrix(name):
    """(rows, n, nnz, rp, ci) of a case, generated once."""
    if name not in _MATRIX:
        m, n, rp, ci = _gen(name)
        rows = (min(m, len(rp) - 1) // 16) * 16
        _MATRIX[name] = (rows, n, int(rp[rows]), rp, ci)
    return _MATRIX[name]


def _value_sets(form, nnz_all, n):
    """[(values, x, what)]: compat values and U(-1, 1) values as the form stores them exactly, x = U(-1, 1) (tests/test_gpu_unit_lean.py)."""
    from tilespmv_amd import generators as G
    dtype = FORMS[form][0]
    rng = np.random.default_rng(20261021)
    x = rng.uniform(-1, 1, n).astype(dtype)
    u = rng.uniform(-1, 1, nnz_all)
    if form == "floats":
        u = u.astype(np.float32).astype(np.float64)
    elif form == "halves":
        u = u.astype(np.float16).astype(np.float64)
        u[np.abs(u) < 2.0 ** -14] = 2.0 ** -14                       # (a denormal half is no value the 2-byte form takes)
    return [(G.compat_values(nnz_all, dtype), x, "compat"), (u.astype(dtype), x, "real")]


def _run(plan, x, rows):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((rows + 16,), 777.0, dtype=xd.dtype, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[rows:] == 777.0).all(), "wrote past the end of y"
    return y[:rows]


def _abs_bound(rows, rp, ci, vals, x):
    nz = int(rp[rows])
    ri = np.repeat(np.arange(rows), np.diff(rp[:rows + 1]))
    out = np.zeros(rows)
    np.add.at(out, ri, np.abs(vals[:nz].astype(np.float64) * x[ci[:nz]].astype(np.float64)))
    return out


def _reference(form, rows, n, nnz, rp, ci, vals, x):
    """(oracle y in float64, the bound on |y - oracle y|)"""
    from oracle.oracle import CpuImpl
    dtype = FORMS[form][0]
    O = CpuImpl("oracle", dtype)
    want = O.spmv(O.tile_create(rows, n, nnz, rp, ci, vals), rows, n, nnz, rp, ci, vals, x)["y"].astype(np.float64)
    return want, TOL[np.dtype(dtype)] * _abs_bound(rows, rp, ci, vals, x) + 1e-300


def _plans(monkeypatch, form, rows, n, nnz, rp, ci, vals, tm, **kw):
    """{(builder, knob): plan}: host- and device-built, TILESPMV_STRIP_SWEEP at 0 and at 1."""
    from tilespmv_amd import api
    dtype, narrow, _ = FORMS[form]
    plans = {}
    for knob in (0, 1):
        monkeypatch.setenv("TILESPMV_STRIP_SWEEP", str(knob))
        plans[("host", knob)] = api.Plan(tm, rows, n, nnz, value_narrow=narrow, **COMMON, **kw)
        plans[("device", knob)] = api.Plan.from_csr(rows, n, nnz, rp, ci, vals, dtype=dtype, value_narrow=narrow, **COMMON, **kw)
    monkeypatch.delenv("TILESPMV_STRIP_SWEEP")
    return plans


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_strided_plan_gives_the_unstrided_plans_y(name, form, monkeypatch):
    from tilespmv_amd import api
    rows, n, nnz, rp, ci = _matrix(name)
    dtype, narrow, vbytes = FORMS[form]
    for vals, x, what in _value_sets(form, len(ci), n):
        tag = (name, form, what)
        want, bound = _reference(form, rows, n, nnz, rp, ci, vals, x)
        tm = api.Tile_create(rows, n, nnz, rp, ci, vals, dtype=dtype)
        for desc_dict in (1, 0):
            tag = (name, form, what, desc_dict)
            plans = _plans(monkeypatch, form, rows, n, nnz, rp, ci, vals, tm, desc_dict=desc_dict)
            stride = {k: p.strip_stride() for k, p in plans.items()}
            info = {k: p.info() for k, p in plans.items()}
            digests = {k: p.stream_digests() for k, p in plans.items()}
            print(tag, stride, {k: info[("host", 1)][k] for k in ("unit_lean", "num_tasks", "list_entries", "derived_units", "desc_bytes", "unit_value_bytes", "nt_stream", "csr_form")})
            assert stride[("host", 0)] == stride[("device", 0)] == 1, (tag, stride)                                   # knob 0: never
            assert stride[("host", 1)] == stride[("device", 1)] == CASES[name], (tag, stride)
            if CASES[name] > 1:
                assert info[("host", 1)]["unit_value_bytes"] == vbytes and info[("host", 1)]["unit_lean"] == 1, (tag, info[("host", 1)])
            else:
                assert digests[("host", 1)] == digests[("host", 0)], tag                                              # no stride: the knob-0 plan, stream for stream
            for knob in (0, 1):
                assert digests[("host", knob)] == digests[("device", knob)], (tag, knob)                              # the two builders agree
                for k in ("num_tasks", "num_split_rows", "list_entries", "derived_units", "desc_bytes", "entry_mode", "csr_form", "stream_bytes", "unit_lean"):
                    assert info[("host", knob)][k] == info[("device", knob)][k], (tag, knob, k)
            y = {k: _run(p, x, rows) for k, p in plans.items()}
            for p in plans.values():
                p.close()
            ref = y[("host", 0)]
            for k, got in y.items():
                assert np.array_equal(got, ref), (tag, k, int(np.count_nonzero(got != ref)))                          # whole y, every bit
            err = np.abs(ref.astype(np.float64) - want)
            assert (err <= bound).all(), (tag, float((err / bound).max()))
        api.Tile_destroy(tm)


@pytest.mark.parametrize("form", ["halves", "f32", "wide"])
def test_other_consumers_of_a_strided_plan(form, monkeypatch):
    """5-point 64^2, S = 4: the multi-vector kernel, the general unit kernel (unit_lean = 0), values refreshed in place and the transposed plan all honour the stride."""
    import torch
    from tilespmv_amd import api
    rows, n, nnz, rp, ci = _matrix("lap64")
    dtype, narrow, _ = FORMS[form]
    (vals, x, _), (vals2, _, _) = _value_sets(form, len(ci), n)
    want, bound = _reference(form, rows, n, nnz, rp, ci, vals, x)
    tm = api.Tile_create(rows, n, nnz, rp, ci, vals, dtype=dtype)
    plans = _plans(monkeypatch, form, rows, n, nnz, rp, ci, vals, tm)
    general = _plans(monkeypatch, form, rows, n, nnz, rp, ci, vals, tm, unit_lean=0)
    assert plans[("host", 1)].strip_stride() == general[("host", 1)].strip_stride() == general[("device", 1)].strip_stride() == 4 and general[("host", 0)].strip_stride() == 1
    assert general[("host", 1)].info()["unit_lean"] == 0
    ref = _run(plans[("host", 0)], x, rows)
    assert (np.abs(ref.astype(np.float64) - want) <= bound).all()
    for k, p in list(plans.items()) + list(general.items()):
        assert np.array_equal(_run(p, x, rows), ref), (form, k)
    # 4 vectors.  The multi-vector kernel's sums are fused multiply-adds whose rounding follows a unit's place in its batch, so two cuts of one matrix into strips agree to rounding
    # on real data, not bit for bit (an unstrided plan cut into strips of 8 tile-rows differs from one cut into 4 in the same way): every plan's Y inside the oracle's bound
    # column by column, and — integer X on the compat values, exact in any order — bit-equal among the plans
    rng = np.random.default_rng(7)
    X = np.ascontiguousarray(np.stack([x] + [rng.uniform(-1, 1, n).astype(dtype) for _ in range(3)], axis=1))
    refs = [(want, bound)] + [_reference(form, rows, n, nnz, rp, ci, vals, np.ascontiguousarray(X[:, j])) for j in range(1, 4)]
    Xi = (np.arange(n * 4, dtype=np.int64) % 5).astype(dtype).reshape(n, 4)
    Yi = {}
    for k, p in plans.items():
        for Xh, exact in ((X, False), (Xi, True)):
            Xd = torch.from_numpy(Xh).cuda()
            Yd = torch.full((rows + 16, 4), 777.0, dtype=Xd.dtype, device="cuda")
            p.spmm(Xd.data_ptr(), Yd.data_ptr(), 4); torch.cuda.synchronize()
            Y = Yd.cpu().numpy()
            assert (Y[rows:] == 777.0).all(), (form, k)
            if exact:
                Yi[k] = Y
            else:
                for j in range(4):
                    err = np.abs(Y[:rows, j].astype(np.float64) - refs[j][0])
                    assert (err <= refs[j][1]).all(), (form, "spmm", k, j, float((err / refs[j][1]).max()))
    for k in Yi:
        assert np.array_equal(Yi[k], Yi[("host", 0)]), (form, "spmm", k, int(np.count_nonzero(Yi[k] != Yi[("host", 0)])))
    for p in list(plans.values()) + list(general.values()):
        p.close()
    api.Tile_destroy(tm)
    # values refreshed in place (a flagged plan's layout follows the pattern alone: wide values in the fp64 library), then a product; and the transposed plan
    y2 = {}
    for knob in (0, 1):
        monkeypatch.setenv("TILESPMV_STRIP_SWEEP", str(knob))
        p = api.Plan.from_csr(rows, n, nnz, rp, ci, vals, dtype=dtype, value_map=True, **COMMON)
        pt = api.Plan.from_csr(rows, n, nnz, rp, ci, vals, dtype=dtype, transpose=True, value_narrow=narrow, **COMMON)
        assert p.strip_stride() == pt.strip_stride() == (4 if knob else 1), (form, knob)
        v2d = torch.from_numpy(np.ascontiguousarray(vals2[:nnz])).cuda()
        p.update_values(v2d.data_ptr()); torch.cuda.synchronize()
        y2[knob] = (_run(p, x, rows), _run(pt, x[:rows], n))
        p.close(); pt.close()
    monkeypatch.delenv("TILESPMV_STRIP_SWEEP")
    assert np.array_equal(y2[0][0], y2[1][0]) and np.array_equal(y2[0][1], y2[1][1]), form
    want2, bound2 = _reference(form, rows, n, nnz, rp, ci, vals2, x)
    assert (np.abs(y2[1][0].astype(np.float64) - want2) <= bound2).all(), form
    rpT, ciT, vT, _ = api.csr_transpose(rows, n, rp, ci, vals[:nnz], dtype=dtype)
    wantT, boundT = _reference(form, n, rows, nnz, rpT, ciT, vT, x[:rows])
    assert (np.abs(y2[1][1].astype(np.float64) - wantT) <= boundT).all(), form
