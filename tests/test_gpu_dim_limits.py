"""Products at the dimension limits (tests/dim_cases.py has the matrices, tests/test_dim_cases_cpu.py what they reach): 2^21 .. 2^28 columns on the stream kernel — the
limit itself, 2^28, included — 2^30 + 11 and 2^31 - 1 columns on the first-generation kernel and the CSR fallback, 2^26 + 5 rows, through every descriptor form, entry
mode, panelled and sliced launch, SpMM path, transposer, value map and the device Tile_create.  Everything a kernel decides from a DIMENSION is met where it flips.

x lives on the device only (dim_cases.x_at, filled in chunks of 2^26 elements); the expected y is the integer golden of the compacted pattern, so every comparison is
exact: the rows that hold entries are gathered and compared with torch.equal, every other row of the window the header lets the plan write must be exactly 0 (one
reduction over y), and the sentinel must survive in front of the window and behind it.  No tolerance, nothing read back but a few thousand numbers."""
import time

import numpy as np
import pytest

import dim_cases as D
from witness import KINDS

pytestmark = pytest.mark.gpu

SENTINEL = -7.5e30
CHUNK = 2 ** 26
FACTS = ("nnz", "rows", "tiles", "kernel", "num_tasks", "num_split_rows", "entry_mode", "wg_strips", "desc_bytes", "unit_value_bytes", "list_entries", "derived_units", "csr_form",
         "x_panels", "x_panel_merge", "x_slice_passes", "fallback_nnz", "entry_ordered")
_EXPECTED = {}


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_value_half.py): the other way round PyTorch finds no GPU in this process."""
    import torch
    torch.zeros(1, device="cuda")
    yield
    _EXPECTED.clear()
    torch.cuda.empty_cache()


def _tdt(torch, kind):
    return torch.float64 if KINDS[kind][3] == np.float64 else torch.float32


def _fill_x(torch, n, kind, nvec=1):
    """x (n, or n x nvec row-major) on the device: x_at of every index, 2^26 indices at a time."""
    xd = torch.empty((n,) if nvec == 1 else (n, nvec), dtype=_tdt(torch, kind), device="cuda")
    for s in range(0, n, CHUNK):
        j = torch.arange(s, min(n, s + CHUNK), dtype=torch.int64, device="cuda")
        for v in range(nvec):
            (xd[s:s + len(j)] if nvec == 1 else xd[s:s + len(j), v]).copy_(D.x_at(j, kind, v))
        del j
    return xd


def _expected(torch, c, kind, second=False, transpose=False, nvec=1):
    """(values, row indices on the device, their exact y on the device); computed once per case and shared."""
    key = (c.name, c.seed, c.repeat, kind, second, transpose, nvec)
    if key not in _EXPECTED:
        vals = c.vals(kind, second)
        idx, y = c.expected(kind, vals, transpose=transpose, nvec=nvec)
        _EXPECTED[key] = (vals, torch.from_numpy(idx).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda())
    return _EXPECTED[key]


def _run(torch, plan, xd, rows, idx_d, want_d, nvec=1, window=None, what=""):
    """One product into a sentinel-filled y; the touched rows of the window exact, every other row of it 0, the sentinel everywhere else.  Returns the touched rows' values."""
    room = 16 * ((rows + 15) // 16)
    b, e = window or (0, room)                       # y[b .. e) is what the header lets the plan write
    hi = min(e, rows)                                # ... and [b, hi) what it must write
    yd = torch.full((room + 16,) if nvec == 1 else (room + 16, nvec), SENTINEL, dtype=xd.dtype, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if nvec == 1:
        plan.spmv(xd.data_ptr(), yd.data_ptr(), stream)
    else:
        plan.spmm(xd.data_ptr(), yd.data_ptr(), nvec, stream)
    torch.cuda.synchronize()
    inside = (idx_d >= b) & (idx_d < hi)
    sel = idx_d[inside]
    got = yd[sel]
    assert torch.equal(got, want_d[inside]), (what, "rows that differ: %d of %d" % (int((got != want_d[inside]).sum()), len(sel)))
    yd[sel] = 0
    assert int(torch.count_nonzero(yd[b:hi])) == 0, (what, "a row without entries is not 0")
    s = torch.tensor(SENTINEL, dtype=xd.dtype, device="cuda")
    assert bool((yd[:b] == s).all()) and bool((yd[e:] == s).all()), (what, "wrote outside y[%d .. %d)" % (b, e))
    return got


def _same_facts(info, predicted, what):
    assert [(k, info[k], predicted[k]) for k in FACTS if info[k] != predicted[k]] == [], what


def _both_builders(torch, api, c, kind, tm, xd, opts, what, device=True, check=None):
    """The option set's plan from the host Tile_matrix and (where it has a device path) from the CSR on the device: the facts the host layout builder predicts, the same
    streams, the exact y from both."""
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind)
    kw = D.plan_kw(opts)
    predicted = api.plan_layout_digest(tm, c.rowA, c.colA, c.nnz, **kw)[1]
    if check:
        check(predicted)
    host = api.Plan(tm, c.rowA, c.colA, c.nnz, **kw)
    _same_facts(host.info(), predicted, (what, "host-built"))
    got = _run(torch, host, xd, c.rowA, idx_d, want_d, what=(what, "host-built"))
    if device:
        dev = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, **kw)
        assert dev.info()["device_build"] == 1
        _same_facts(dev.info(), predicted, (what, "device-built"))
        a, b = host.stream_digests(), dev.stream_digests()
        assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == [], (what, "host-built and device-built streams differ")
        _run(torch, dev, xd, c.rowA, idx_d, want_d, what=(what, "device-built"))
        dev.close()
    host.close()
    return got, predicted


def _bits(torch, t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- 1. SpMV through every option set, 2^21 .. 2^28 columns
@pytest.mark.parametrize("kind", ["half", "f32"])
@pytest.mark.parametrize("name", ["W21", "W24", "W28", "W28m"])
def test_spmv_every_option_set_up_to_2_28_columns(name, kind):
    import torch
    from tilespmv_amd import api
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype)
    xd = _fill_x(torch, c.colA, kind)
    for key, opts in D.SPMV_SETS.items():
        t0 = time.time()
        got, predicted = _both_builders(torch, api, c, kind, tm, xd, opts, (name, kind, key))
        assert predicted["kernel"] == api.KERNEL_STREAM
        if kind == "half" and key in D.NARROWABLE:      # halves and doubles of the same plan: the same y in every bit
            ys = []
            for narrow, nbytes in ((2, 2), (0, 8)):
                p = api.Plan(tm, c.rowA, c.colA, c.nnz, **D.plan_kw(dict(opts, value_narrow=narrow)))
                assert p.info()["unit_value_bytes"] == nbytes, (name, key, narrow)
                ys.append(_run(torch, p, xd, c.rowA, idx_d, want_d, what=(name, key, "value_narrow=%d" % narrow)))
                p.close()
            assert torch.equal(_bits(torch, ys[0]), _bits(torch, ys[1])), (name, key, "narrow and wide plan differ")
        print("%s %s %s: %.2f s" % (name, kind, key, time.time() - t0))
    if name == "W28":                                   # the stream kernel at its limit beside the CSR fallback (host builder only: no device path)
        t0 = time.time()

        def stream_with_fallback(f):
            assert f["kernel"] == api.KERNEL_STREAM and f["fallback_nnz"] > 0, f
        _both_builders(torch, api, c, kind, tm, xd, dict(coo_mode=api.COO_FALLBACK), (name, kind, "COO_FALLBACK"), device=False, check=stream_with_fallback)
        print("%s %s COO_FALLBACK: %.2f s" % (name, kind, time.time() - t0))
    api.Tile_destroy(tm)
    del xd


@pytest.mark.parametrize("kind", ["half", "f32"])
def test_pooled_four_byte_words_at_2_21_columns(kind):
    """The 4-byte pooled word needs window base + pattern id + tile-row in 32 bits: at 2^21 columns that is a matrix of at most 256 patterns (the generator's repeat form)."""
    import torch
    from tilespmv_amd import api
    c = D.case("W21", repeat=True)
    vals, _, _ = _expected(torch, c, kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=KINDS[kind][3])
    xd = _fill_x(torch, c.colA, kind)

    def is_word(f):
        assert (f["desc_bytes"], f["csr_form"]) == (4, 2), f
    for em in (0, 2):
        _both_builders(torch, api, c, kind, tm, xd, dict(D.SPMV_SETS["pool"], entry_mode=em), ("W21 repeat", kind, "pool", em), check=is_word)
    api.Tile_destroy(tm)


# ---- 2. column panels and XCD slices
@pytest.mark.parametrize("kind", ["half", "f32"])
@pytest.mark.parametrize("name", ["W24", "W28"])
def test_panels_and_slices(name, kind):
    import torch
    from tilespmv_amd import api
    c = D.case(name)
    vals, _, _ = _expected(torch, c, kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=KINDS[kind][3])
    xd = _fill_x(torch, c.colA, kind)
    plain, _ = _both_builders(torch, api, c, kind, tm, xd, D.SPMV_SETS["em2"], (name, kind, "unpanelled"), device=False)
    for kb in (16, 2048):
        t0 = time.time()

        def panelled(f):
            assert f["x_panels"] > 32 and f["x_panel_merge"] == 1, f
        got, _ = _both_builders(torch, api, c, kind, tm, xd, D.panel_set(kb), (name, kind, "panels", kb), check=panelled)
        assert torch.equal(_bits(torch, got), _bits(torch, plain)), (name, kb, "panelled and plain launch differ")
        for passes in (1, 3):
            def sliced(f):
                assert f["x_slice_passes"] == passes and f["entry_ordered"] == 0, f
            got, _ = _both_builders(torch, api, c, kind, tm, xd, D.slice_set(kb, passes), (name, kind, "slices", kb, passes), check=sliced)
        print("%s %s panels of %d KB: %.2f s" % (name, kind, kb, time.time() - t0))
    api.Tile_destroy(tm)


# ---- 3. beyond the stream kernel: first-generation kernel and the CSR fallback, x past 2^32 bytes
@pytest.mark.parametrize("name, kind", [("X30", "half"), ("X30", "f32"), ("XMAX", "f32")])
def test_first_generation_kernel_and_fallback_beyond_2_28_columns(name, kind):
    import torch
    from tilespmv_amd import api
    t0 = time.time()
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype)
    assert tm.tilen == c.colA // 16 + 1 > 2 ** 24
    xd = _fill_x(torch, c.colA, kind)
    assert xd.numel() * xd.element_size() > 2 ** 32
    print("%s %s: matrix and x in %.2f s" % (name, kind, time.time() - t0))
    for coo in (api.COO_IN_TILE, api.COO_FALLBACK):
        for dense in (api.DENSE_MFMA, api.DENSE_VALU):
            t0 = time.time()

            def first_generation(f):
                assert f["kernel"] == api.KERNEL_DIRECT and (f["fallback_nnz"] > 0) == (coo == api.COO_FALLBACK), f
            _both_builders(torch, api, c, kind, tm, xd, dict(coo_mode=coo, dense_mode=dense), (name, kind, coo, dense), device=False, check=first_generation)
            print("%s %s coo_mode %d dense_mode %d: %.2f s" % (name, kind, coo, dense, time.time() - t0))
    with pytest.raises(NotImplementedError):              # no device path beyond 2^24 column blocks: a status, nothing built
        api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, **D.plan_kw({}))
    with pytest.raises(RuntimeError):                     # ... and the stream kernel refuses
        api.Plan(tm, c.rowA, c.colA, c.nnz, kernel=api.KERNEL_STREAM, **D.plan_kw({}))
    api.Tile_destroy(tm)
    del xd


# ---- 4. SpMM
@pytest.mark.parametrize("kind", ["float", "f32"])
@pytest.mark.parametrize("name, nvec", [("W28", 2), ("W24", 8)])
def test_spmm_every_path(name, nvec, kind):
    """mv_native 0 = one right-hand side at a time over transposed copies of X (leading dimension colA + 16 rounded up: j * ldx crosses 2^32 bytes at 2^28 columns),
    1 = the multi-vector kernel (X[col * nvec + n]), 2 = the multi-vector kernel + the entry pass over the merged lists (classic, workgroup entry mode)."""
    import torch
    from tilespmv_amd import api
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind, nvec=nvec)
    _, idx1, want1 = _expected(torch, c, kind)
    assert torch.equal(want_d[:, 0], want1)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype)
    Xd = _fill_x(torch, c.colA, kind, nvec)
    for form, natives in (("em2", (0, 1, 2)), ("pool", (0, 1)), ("wide", (1,))):
        for mv in natives:
            for device in (False, True):
                if device and mv != 1:
                    continue
                t0 = time.time()
                kw = D.plan_kw(dict(D.SPMV_SETS[form], mv_native=mv))
                if device:
                    plan = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, **kw)
                else:
                    plan = api.Plan(tm, c.rowA, c.colA, c.nnz, **kw)
                assert plan.info()["csr_form"] == {"em2": 1, "pool": 2, "wide": 3}[form]
                _run(torch, plan, Xd, c.rowA, idx_d, want_d, nvec=nvec, what=(name, kind, form, "mv_native", mv, "device" if device else "host"))
                plan.close()
                print("%s %s nvec %d %s mv_native %d %s: %.2f s" % (name, kind, nvec, form, mv, "device-built" if device else "host-built", time.time() - t0))
    api.Tile_destroy(tm)
    del Xd


# ---- 5. 2^26 + 5 rows
@pytest.mark.parametrize("kind", ["half", "f32"])
@pytest.mark.parametrize("name", ["T26", "SQ26"])
def test_tall_and_square_plans_and_their_shards(name, kind):
    import torch
    from tilespmv_amd import api
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype)
    xd = _fill_x(torch, c.colA, kind)
    tilem = (c.rowA + 15) // 16
    assert tm.tilem == tilem == 2 ** 22 + 1
    for label, opts in (("default knobs", {}), ("classic entry_mode 2", D.SPMV_SETS["em2"])):
        kw = D.plan_kw(opts)
        t0 = time.time()
        host = api.Plan(tm, c.rowA, c.colA, c.nnz, **kw)
        t1 = time.time()
        dev = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, **kw)
        t2 = time.time()
        print("%s %s %s: host build %.2f s, device build (CSR upload included) %.2f s" % (name, kind, label, t1 - t0, t2 - t1))
        hi, di = host.info(), dev.info()
        assert [(k, hi[k], di[k]) for k in FACTS if hi[k] != di[k]] == [] and di["device_build"] == 1 and hi["rows"] == c.rowA
        a, b = host.stream_digests(), dev.stream_digests()
        assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == [], (name, label, "host-built and device-built streams differ")
        _run(torch, host, xd, c.rowA, idx_d, want_d, what=(name, kind, label, "host-built"))
        _run(torch, dev, xd, c.rowA, idx_d, want_d, what=(name, kind, label, "device-built"))
        host.close(); dev.close()
    # shards: the middle third of the tile-rows (device-built), and the last tile-row alone (host-built: 5 rows)
    b, e = tilem // 3, 2 * tilem // 3
    t0 = time.time()
    mid = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, tilerow_begin=b, tilerow_end=e, **D.plan_kw({}))
    assert mid.info()["rows"] == 16 * (e - b)
    _run(torch, mid, xd, c.rowA, idx_d, want_d, window=(16 * b, 16 * e), what=(name, kind, "middle third"))
    mid.close()
    t1 = time.time()
    last = api.Plan(tm, c.rowA, c.colA, c.nnz, tilerow_begin=tilem - 1, tilerow_end=tilem, **D.plan_kw({}))
    print("%s %s shards: middle third (device build) %.2f s, last tile-row host build %.2f s" % (name, kind, t1 - t0, time.time() - t1))
    assert last.info()["rows"] == c.rowA - 16 * (tilem - 1) == 5
    _run(torch, last, xd, c.rowA, idx_d, want_d, window=(16 * (tilem - 1), 16 * tilem), what=(name, kind, "last tile-row"))
    last.close()
    api.Tile_destroy(tm)


# ---- 6. transposed plans: a wide one from a tall matrix (the transposer scans 4100 counters), a tall one from a wide matrix (2^26 + 10 counters: three scan levels)
@pytest.mark.parametrize("kind", ["half", "f32"])
@pytest.mark.parametrize("name", ["T26", "WIDE26"])
def test_transposed_plans(name, kind):
    import torch
    from tilespmv_amd import api
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind, transpose=True)
    xd = _fill_x(torch, c.rowA, kind)                     # A^T x: x has A's rows
    kw = D.plan_kw({})
    t0 = time.time()
    dev = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, transpose=True, **kw)
    assert dev.shape == (c.colA, c.rowA) and dev.info()["rows"] == c.colA and dev.info()["nnz"] == c.nnz
    _run(torch, dev, xd, c.colA, idx_d, want_d, what=(name, kind, "transposed on the device"))
    t1 = time.time()
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, transpose=True)       # the host transposer, the host builders
    host = api.Plan(tm, c.colA, c.rowA, c.nnz, **kw)
    a, b = host.stream_digests(), dev.stream_digests()
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == [], (name, "host-transposed and device-transposed streams differ")
    _run(torch, host, xd, c.colA, idx_d, want_d, what=(name, kind, "transposed on the host"))
    print("%s %s transposed: device %.2f s, host %.2f s" % (name, kind, t1 - t0, time.time() - t1))
    host.close(); dev.close()
    api.Tile_destroy(tm)


@pytest.mark.parametrize("kind", ["half", "f32"])
def test_device_transposer_equals_the_host_transposer_at_2_26_columns(kind):
    import torch
    from tilespmv_amd import api
    c = D.case("WIDE26")
    dtype = KINDS[kind][3]
    vals = c.vals(kind)
    rpT, ciT, vT, srcT = api.csr_transpose(c.rowA, c.colA, c.rp, c.ci, vals, dtype=dtype)
    assert len(rpT) == 2 ** 26 + 10 and rpT[-1] == c.nnz
    d_rp, d_ci, d_v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.rp, c.ci, vals))
    d_rpT = torch.full((c.colA + 1 + 16,), -7, dtype=torch.int32, device="cuda")
    d_ciT, d_srcT = (torch.full((c.nnz + 16,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    d_vT = torch.full((c.nnz + 16,), SENTINEL, dtype=_tdt(torch, kind), device="cuda")
    api.csr_transpose_device(c.rowA, c.colA, d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), d_rpT.data_ptr(), d_ciT.data_ptr(), d_vT.data_ptr(), d_srcT.data_ptr(), dtype=dtype,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(d_rpT[:c.colA + 1], torch.from_numpy(rpT).cuda()) and bool((d_rpT[c.colA + 1:] == -7).all())
    for d, h in ((d_ciT, ciT), (d_srcT, srcT)):
        assert torch.equal(d[:c.nnz], torch.from_numpy(h).cuda()) and bool((d[c.nnz:] == -7).all())
    assert torch.equal(_bits(torch, d_vT[:c.nnz]), _bits(torch, torch.from_numpy(vT).cuda()))
    assert bool((d_vT[c.nnz:] == torch.tensor(SENTINEL, dtype=d_vT.dtype, device="cuda")).all())


# ---- 7. value maps
@pytest.mark.parametrize("kind", ["half", "f32"])
@pytest.mark.parametrize("name", ["W28m", "SQ26"])
def test_value_map_update_at_the_limits(name, kind):
    import torch
    from tilespmv_amd import api
    t0 = time.time()
    c = D.case(name)
    dtype = KINDS[kind][3]
    vals, idx_d, want_d = _expected(torch, c, kind)
    vals2, idx2, want2 = _expected(torch, c, kind, second=True)
    assert not np.array_equal(vals, vals2) and torch.equal(idx_d, idx2)
    xd = _fill_x(torch, c.colA, kind)
    kw = D.plan_kw({})
    plan = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, value_map=True, **kw)
    assert plan.info()["value_map_bytes"] > 0
    _run(torch, plan, xd, c.rowA, idx_d, want_d, what=(name, kind, "value map, first values"))
    d2 = torch.from_numpy(np.ascontiguousarray(vals2)).cuda()
    plan.update_values(d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _run(torch, plan, xd, c.rowA, idx_d, want2, what=(name, kind, "after update_values"))
    fresh = api.Plan.from_csr(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals2, dtype=dtype, value_map=True, **kw)
    a, b = plan.stream_digests(), fresh.stream_digests()
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == [], (name, kind, "updated plan and fresh plan of the new values differ")
    fi, pi = fresh.info(), plan.info()
    assert [(k, pi[k], fi[k]) for k in FACTS if pi[k] != fi[k]] == []
    plan.close(); fresh.close()
    print("%s %s value map: %.2f s" % (name, kind, time.time() - t0))


# ---- 8. the device Tile_create: tile keys of 2^24 column blocks and 2^22 + 1 tile-rows
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["W28", "SQ26", "T26"])
def test_device_tile_create_equals_host_at_the_limits(name, dtype):
    from test_gpu_device_build import same_tile_matrix
    t0 = time.time()
    c = D.case(name)
    assert same_tile_matrix(c.rowA, c.colA, c.rp, c.ci, dtype) == []
    print("%s %s device Tile_create == host: %.2f s" % (name, np.dtype(dtype).name, time.time() - t0))
