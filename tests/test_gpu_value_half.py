"""Unit values stored as halves on the device (tilespmv_plan_options.value_narrow = 2; fp64): a plan whose unit values are all +-0 or normal IEEE binary16 numbers stores them
in 2 bytes, four units per 8-byte lane load, and k_units_half / k_units_mv widen them in registers, half -> float -> double.  Both conversions are exact and the arithmetic is
the wide plan's, so y must keep EVERY bit: each case compares the whole y of the 2-byte plan with the y of the value_narrow=0 plan of the same options (np.array_equal),
checks the sentinel behind y, and compares with a CSR golden — exact on the integer-valued compat data, inside the usual 1e-12 x sum |a_ij x_j| on real-valued x (fp64
sums in another order).  The shapes are those of tests/test_gpu_value_narrow.py: the smallest that reach each path of the narrow layout."""
import numpy as np
import pytest

from cases import truncated_rows

pytestmark = pytest.mark.gpu

COMMON = dict(placement_tries=1, deterministic=1)


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_unit_loop.py): the other way round PyTorch finds no GPU in this process."""
    import torch
    torch.zeros(1, device="cuda")
    yield
TOL = 1e-12


def _value_sets(nnz, n):
    """(values, x, exact): the reference's integer-valued compat data, and signed multiples of 2^-4 below 2^6 (mantissa and exponent bits of a half in use) with real x —
    the largest half, the smallest normal half and a negative zero in a few slots."""
    from tilespmv_amd import generators as G
    rng = np.random.default_rng(2024)
    v = rng.integers(-2 ** 10 + 1, 2 ** 10, nnz).astype(np.float64) / 16.0
    for k, special in zip(rng.choice(nnz, 12, replace=False), [65504.0, 2.0 ** -14, -0.0, -65504.0] * 3):
        v[k] = special
    return [(G.compat_values(nnz), G.compat_x(n), True), (v, G.real_x(n, nnz), False)]


def _golden(rowA, rp, ci, vals, x, transpose_cols=None):
    """y = A x (or A^T x) from the CSR in float64, and sum |a_ij x_j| per row for the tolerance."""
    k = int(rp[rowA])
    ri = np.repeat(np.arange(rowA), np.diff(rp[:rowA + 1]))
    if transpose_cols is None:
        prod = vals[:k] * x[ci[:k]]
        y = np.zeros(rowA); b = np.zeros(rowA)
        np.add.at(y, ri, prod); np.add.at(b, ri, np.abs(prod))
    else:
        prod = vals[:k] * x[ri]
        y = np.zeros(transpose_cols); b = np.zeros(transpose_cols)
        np.add.at(y, ci[:k], prod); np.add.at(b, ci[:k], np.abs(prod))
    return y, b


def _run(plan, x, rows):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((rows + 16,), 777.0, dtype=torch.float64, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[rows:] == 777.0).all(), "wrote past the end of y"      # the rows behind the plan keep their sentinel
    return y[:rows]


def _check(y, want, bound, exact, what):
    if exact:
        assert np.array_equal(y, want), (what, int(np.count_nonzero(y != want)))
    else:
        assert (np.abs(y - want) <= TOL * bound + 1e-300).all(), what


def _half_vs_wide(gen, kw, hyb=False, want_facts=None):
    """Host-built plans of one matrix and one option set with value_narrow 2 and 0, both value sets: 2-byte y == wide y in every bit, y against the golden."""
    from tilespmv_amd import api
    m, n, rp, ci = gen
    nnz, rowA = len(ci), truncated_rows(m)
    for vals, x, exact in _value_sets(nnz, n):
        want, bound = _golden(rowA, rp, ci, vals, x)
        tm = api.Tile_create(rowA, n, nnz, rp, ci, vals, hyb=hyb)
        pn = api.Plan(tm, rowA, n, nnz, value_narrow=2, **COMMON, **kw)
        pw = api.Plan(tm, rowA, n, nnz, value_narrow=0, **COMMON, **kw)
        i_n, i_w = pn.info(), pw.info()
        assert (i_n["unit_value_bytes"], i_w["unit_value_bytes"], i_n["nt_stream"]) == (2, 8, 1), (kw, i_n)
        for k in ("num_tasks", "num_split_rows", "list_entries", "derived_units", "desc_bytes", "entry_mode", "csr_form"):
            assert i_n[k] == i_w[k], (kw, k)
        for k, v in (want_facts or {}).items():
            assert v(i_n[k]), (kw, k, i_n[k])
        yn, yw = _run(pn, x, rowA), _run(pw, x, rowA)
        pn.close(); pw.close(); api.Tile_destroy(tm)
        assert np.array_equal(yn, yw), (kw, exact, int(np.count_nonzero(yn != yw)))
        _check(yn, want, bound, exact, (kw, exact))


def test_dictionary_descriptors_absorbed_entries_derived_units():
    from tilespmv_amd import generators as G
    _half_vs_wide(G.laplacian5pt(64), {}, want_facts={"desc_bytes": lambda v: v == 4, "derived_units": lambda v: v > 0, "list_entries": lambda v: v == 0})
    _half_vs_wide(G.laplacian5pt(64), dict(desc_dict=0), want_facts={"desc_bytes": lambda v: v == 12})


@pytest.mark.parametrize("entry_mode", [0, 2])
def test_unaligned_grid_split_csr_tiles_and_list_entries(entry_mode):
    """5-point 50^2: 2500 rows, truncated to 2496 (the last tile-row's padding rows keep their sentinel); CSR tiles split into units + list entries."""
    from tilespmv_amd import generators as G
    _half_vs_wide(G.laplacian5pt(50), dict(csr_split=1, entry_mode=entry_mode), want_facts={"list_entries": lambda v: v > 0, "entry_mode": lambda v: v == entry_mode})


@pytest.mark.parametrize("strip_cost", [100, 200, 300])
def test_task_tails_of_one_two_and_three_units(strip_cost):
    """7-point 32^3: 7 units per tile-row, so strips of 1, 2 and 3 tile-rows end with 3, 2 and 1 units in their last group of 4 (the clamp on the last group's load)."""
    from tilespmv_amd import generators as G
    _half_vs_wide(G.laplacian7pt(32), dict(strip_even=0, strip_cost=strip_cost))


SPLIT = dict(split_above=200, strip_cost=32)   # (rows are cut above max(6 x strip cost, split_above): 200 with strips of 32)


@pytest.mark.parametrize("kw", [dict(), SPLIT, dict(fix_inline=0, **SPLIT), dict(fix_inline=1, **SPLIT), dict(entry_mode=2, **SPLIT)],
                         ids=["long_tasks", "split_rows", "split_rows_fixup_kernel", "split_rows_inline", "split_rows_workgroup_entries"])
def test_long_tasks_and_split_tile_rows(kw):
    """Band of half-width 40 with its dense tiles as units: tasks longer than one 16-unit descriptor chunk; split tile-rows summed in the unit kernel or by k_fixup_split.
    3000 rows are truncated to 2992.  (By rule this small, entry-heavy grid gets the wavefront entry mode, which has no narrow form: the per-strip mode is asked for.)"""
    from tilespmv_amd import api, generators as G
    facts = {"num_split_rows": (lambda v: v > 0)} if kw else {"num_split_rows": (lambda v: v == 0), "num_tasks": (lambda v: v <= 2992 // 16)}
    _half_vs_wide(G.band(3000, 40), dict(dense_mode=api.DENSE_VALU, **{"entry_mode": 0, **kw}), want_facts=facts)


@pytest.mark.parametrize("desc_dict", [0, 1])
def test_all_seven_tile_formats(desc_dict):
    """(The rule gives this small matrix the wavefront entry mode, which has no narrow form: the per-strip and the workgroup mode are asked for.)"""
    from tilespmv_amd import generators as G
    _half_vs_wide(G.all_formats(12, 7), dict(desc_dict=desc_dict, csr_split=1, entry_mode=2 * desc_dict), hyb=True, want_facts={"desc_bytes": lambda v: v == (4 if desc_dict else 12)})


@pytest.mark.parametrize("name", ["lap64", "allfmt"])
def test_host_and_device_builders_make_the_same_two_byte_plan(name):
    from tilespmv_amd import api, generators as G
    gen, hyb, kw = (G.laplacian5pt(64), False, {}) if name == "lap64" else (G.all_formats(12, 7), True, dict(csr_split=1, entry_mode=0))
    m, n, rp, ci = gen
    nnz, rowA = len(ci), truncated_rows(m)
    vals, x, _ = _value_sets(nnz, n)[1]
    tm = api.Tile_create(rowA, n, nnz, rp, ci, vals, hyb=hyb)
    host = api.Plan(tm, rowA, n, nnz, value_narrow=2, **COMMON, **kw)
    dev = api.Plan.from_csr(rowA, n, nnz, rp, ci, vals, hyb=hyb, value_narrow=2, **COMMON, **kw)
    ih, idv = host.info(), dev.info()
    assert ih["unit_value_bytes"] == idv["unit_value_bytes"] == 2
    facts = ("device_bytes", "stream_bytes", "nnz", "rows", "tiles", "coo_mode", "dense_mode", "kernel", "num_tasks", "num_split_rows", "entry_mode", "entry_ordered", "strip_cost", "wg_strips",
             "brick_order", "desc_bytes", "nt_stream", "unit_value_bytes", "list_entries", "derived_units", "x_panels", "scattered_entries", "csr_form")   # (what does not depend on where the plan was built)
    assert [(k, ih[k], idv[k]) for k in facts if ih[k] != idv[k]] == []
    assert host.stream_digests() == dev.stream_digests()
    wide = api.Plan(tm, rowA, n, nnz, value_narrow=0, **COMMON, **kw)
    assert wide.info()["unit_value_bytes"] == 8
    yw = _run(wide, x, rowA)
    assert np.array_equal(_run(host, x, rowA), yw) and np.array_equal(_run(dev, x, rowA), yw)       # whole y of both 2-byte plans against the wide plan's
    want, bound = _golden(rowA, rp, ci, vals, x)
    _check(yw, want, bound, False, name)
    host.close(); dev.close(); wide.close(); api.Tile_destroy(tm)


@pytest.mark.parametrize("name", ["lap64", "lap50_entries"])
def test_multi_vector_product_reads_two_byte_plans_natively(name):
    """tilespmv_plan_spmm with nvec 2 / 4 / 8, the multi-vector kernel alone (mv_native 1) and with the entry pass (2): every column bit-equal to the wide plan's (the third arm of k_units_mv's value load)."""
    import torch
    from tilespmv_amd import api, generators as G
    gen, kw = (G.laplacian5pt(64), {}) if name == "lap64" else (G.laplacian5pt(50), dict(csr_split=1, entry_mode=2))
    m, n, rp, ci = gen
    nnz, rowA = len(ci), truncated_rows(m)
    vals, _, _ = _value_sets(nnz, n)[1]
    X = np.random.default_rng(5).uniform(-1, 1, (n, 8))
    tm = api.Tile_create(rowA, n, nnz, rp, ci, vals)
    for mv in (1, 2):
        pn = api.Plan(tm, rowA, n, nnz, value_narrow=2, mv_native=mv, **COMMON, **kw)
        pw = api.Plan(tm, rowA, n, nnz, value_narrow=0, mv_native=mv, **COMMON, **kw)
        assert (pn.info()["unit_value_bytes"], pw.info()["unit_value_bytes"]) == (2, 8)
        for nv in (2, 4, 8):
            got = []
            for p in (pn, pw):
                Xd = torch.from_numpy(np.ascontiguousarray(X[:, :nv])).cuda()
                Yd = torch.full((rowA + 16, nv), -4.0, dtype=torch.float64, device="cuda")
                p.spmm(Xd.data_ptr(), Yd.data_ptr(), nv); torch.cuda.synchronize()
                Y = Yd.cpu().numpy()
                assert (Y[rowA:] == -4.0).all()
                got.append(Y[:rowA])
            assert np.array_equal(got[0], got[1]), (name, mv, nv)
            for j in range(nv):
                want, bound = _golden(rowA, rp, ci, vals, np.ascontiguousarray(X[:, j]))
                _check(got[0][:, j], want, bound, False, (name, mv, nv, j))
        pn.close(); pw.close()
    api.Tile_destroy(tm)


def test_transposed_plan_gets_halves_too():
    from tilespmv_amd import api, generators as G
    m, n, rp, ci = G.laplacian5pt(50)
    nnz = len(ci)
    for vals, _, exact in _value_sets(nnz, n):
        x = G.compat_x(m) if exact else G.real_x(m, nnz)
        want, bound = _golden(m, rp, ci, vals, x, transpose_cols=n)
        rows_t = truncated_rows(n)                                   # (the plan of A^T drops the last n % 16 rows of A^T like every plan)
        p = api.Plan.from_csr(m, n, nnz, rp, ci, vals, transpose=True, value_narrow=2, csr_split=1, **COMMON)
        w = api.Plan.from_csr(m, n, nnz, rp, ci, vals, transpose=True, value_narrow=0, csr_split=1, **COMMON)
        assert (p.info()["unit_value_bytes"], w.info()["unit_value_bytes"]) == (2, 8) and p.info()["rows"] == w.info()["rows"]
        rows_p = p.info()["rows"]
        y, yw = _run(p, x, rows_p), _run(w, x, rows_p)
        p.close(); w.close()
        assert np.array_equal(y, yw), ("transpose", exact, int(np.count_nonzero(y != yw)))            # whole y against the wide plan of A^T
        _check(y, want[:rows_p], bound[:rows_p], exact, ("transpose", exact))
        assert rows_p in (n, rows_t)


def test_value_map_plans_stay_wide_and_update():
    """A flagged plan's layout follows the pattern alone: value_narrow=2 changes nothing, and update_values still writes 8-byte values."""
    import torch
    from tilespmv_amd import api, generators as G
    m, n, rp, ci = G.laplacian5pt(64)
    nnz, rowA = len(ci), truncated_rows(m)
    (v1, x, _), (v2, _, _) = _value_sets(nnz, n)
    p = api.Plan.from_csr(rowA, n, nnz, rp, ci, v1, value_map=True, value_narrow=2, **COMMON)
    q = api.Plan.from_csr(rowA, n, nnz, rp, ci, v1, value_map=True, value_narrow=0, **COMMON)
    assert p.info()["unit_value_bytes"] == 8 and p.stream_digests() == q.stream_digests()
    q.close()
    want1, _ = _golden(rowA, rp, ci, v1, x)
    assert np.array_equal(_run(p, x, rowA), want1)
    dv2 = torch.from_numpy(v2).cuda()
    p.update_values(dv2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want2, _ = _golden(rowA, rp, ci, v2, x)
    assert np.array_equal(_run(p, x, rowA), want2)                  # (compat x: small integers times multiples of 2^-14 below 2^16, exact in any order)
    p.close()
