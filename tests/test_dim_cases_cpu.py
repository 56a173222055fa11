"""Ledger of the dimension-limit cases (tests/dim_cases.py; the GPU half is tests/test_gpu_dim_limits.py), no GPU: the generator keeps its promises (pinned and straddling
clusters, the long last row, the dense tile; an x that tells j from j + 2^k), the host layout builder (tilespmv_plan_layout_digest) says which plan forms the case list
reaches — a shape or generator change that stops reaching the 4 / 8 / 12 / 20 / 28-byte descriptors, an entry mode, a panelled or sliced plan, the CSR fallback or the
first-generation kernel where the GPU file expects them fails here, not silently there — and the host half of the limits themselves: Tile_create, tilespmv_cpu and the
matrix cache at 2^31 - 1 columns, where (colA + 15) / 16 in int used to overflow.

The ROW side near 2^31 is not tested anywhere: the row pointer of such a matrix alone is 8 GB (16 GB with the int64 counts behind it).  It is covered by the same
tiles_of() fix and by reading (the summary of the change that added this file lists the index arithmetic)."""
import hashlib
import os

import numpy as np
import pytest

import dim_cases as D
from witness import KINDS
from tilespmv_amd import api


def _facts_of(tm, c, **kw):
    return api.plan_layout_digest(tm, c.rowA, c.colA, c.nnz, **D.plan_kw(kw))[1]


def _facts(c, kind="half", dtype=np.float64, **kw):
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, c.vals(kind), dtype=dtype)
    try:
        return _facts_of(tm, c, **kw)
    finally:
        api.Tile_destroy(tm)


def _first_generation_facts(tm, c):
    """More than 2^24 column blocks: the builder itself takes the first-generation kernel, with in-tile entries and with the CSR fallback."""
    f = _facts_of(tm, c)
    assert f["kernel"] == api.KERNEL_DIRECT and f["nnz"] == c.nnz and f["fallback_nnz"] == 0, c.name
    f = _facts_of(tm, c, coo_mode=api.COO_FALLBACK)
    assert f["kernel"] == api.KERNEL_DIRECT and f["fallback_nnz"] > 0, c.name


# ---- x
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_x_is_nonzero_sign_mixed_and_the_same_in_numpy_and_torch(kind):
    import torch
    for lo in (0, 2 ** 20 - 5000, 2 ** 28 - 5000, 2 ** 31 - 10001):
        j = np.arange(lo, lo + 10000, dtype=np.int64)
        for col in (0, 1, 7):
            a = D.x_at(j, kind, col)
            b = D.x_at(torch.from_numpy(j), kind, col)
            assert a.dtype == np.int64 and b.dtype == torch.int64 and np.array_equal(a, b.numpy())
            assert np.abs(a).min() >= 1 and np.abs(a).max() <= KINDS[kind][2]
            assert 0.4 < np.mean(a > 0) < 0.6
            assert np.array_equal(a.astype(KINDS[kind][3]).astype(np.int64), a)          # a machine number of the kind's type
    assert not np.array_equal(D.x_at(j, kind, 0), D.x_at(j, kind, 1))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_x_tells_j_from_j_plus_every_power_of_two(kind):
    """A gather that drops or wraps one index bit reads x[j +- 2^k]: for every k that must be another number for most j (a 63-valued x cannot do better than 62 / 63)."""
    rng = np.random.default_rng(1)
    for k in range(4, 31):
        j = rng.integers(0, 2 ** 31 - 2 ** k, 20000)
        differ = np.mean(D.x_at(j, kind) != D.x_at(j + 2 ** k, kind))
        assert differ > 0.95, (kind, k, differ)
        assert np.mean(D.x_at(j, kind) != D.x_at(j ^ 2 ** k, kind)) > 0.95, (kind, k)


# ---- the generator
@pytest.mark.parametrize("name", sorted(D.SHAPES) + ["WIDE26"])
def test_generator_places_what_it_promises(name):
    c = D.case(name)
    rows, cols = D.WIDE26 if name == "WIDE26" else D.SHAPES[name]
    assert (c.rowA, c.colA) == (rows, cols) and 15000 <= c.nnz <= 25000
    assert c.rp[0] == 0 and c.rp[rows] == c.nnz and len(c.rp) == rows + 1 and np.all(np.diff(c.rp[:4097]) >= 0)
    key = c.ri * cols + c.ci
    assert np.all(np.diff(key) > 0)                                                           # CSR order, no duplicates
    ri, ci = c.ri, c.ci.astype(np.int64)
    assert np.count_nonzero((ri < 64) & (ci >= cols - 64)) >= 64                              # first rows, last columns (the partial last tile-column with them)
    assert np.count_nonzero((ri >= rows - 64) & (ci < 64)) >= 64                              # last rows, first columns
    if cols % 16:
        assert np.count_nonzero(ci >= cols // 16 * 16) >= cols % 16
    for p in c.straddled:                                                                     # a cluster on both sides of every power of two the code branches on
        assert np.count_nonzero((ci >= 2 ** p - 32) & (ci < 2 ** p)) >= 20 and np.count_nonzero((ci >= 2 ** p) & (ci < min(cols, 2 ** p + 32))) >= 1, p
    assert c.straddled == [p for p in D.BRANCH_POWERS if 2 ** p < cols]
    assert c.last_row_len >= 400
    last = ci[c.rp[rows - 1]:]
    assert last[0] == 0 and last[-1] == cols - 1 and np.diff(last).max() <= (cols + 399) // 400 + 64     # spread over all columns
    rb, cb = c.dense_tile
    assert cb == cols // 16 - 1 and np.count_nonzero((ri // 16 == rb) & (ci // 16 == cb)) == 256
    assert np.count_nonzero(np.diff(c.rp) == 0) > rows - 8000                                 # hypersparse


def test_expected_is_the_golden_of_the_compacted_pattern():
    """On a shape small enough to write out, the compacted expectation is witness.golden of the matrix itself with x_at as x — both products."""
    from witness import golden
    c = D.DimCase("small", 700, 4099, 3)
    for kind in ("half", "f32"):
        v = c.vals(kind)
        x = D.x_at(np.arange(c.colA), kind).astype(KINDS[kind][3])
        idx, y = c.expected(kind, v)
        full = golden(c.rowA, c.rp, c.ci, v, x)
        assert np.array_equal(full[idx], y) and np.count_nonzero(np.delete(full, idx)) == 0
        xt = D.x_at(np.arange(c.rowA), kind).astype(KINDS[kind][3])
        idx, y = c.expected(kind, v, transpose=True)
        full = golden(c.rowA, c.rp, c.ci, v, xt, transpose_cols=c.colA)
        assert np.array_equal(full[idx], y) and np.count_nonzero(np.delete(full, idx)) == 0
        X = np.stack([D.x_at(np.arange(c.colA), kind, j) for j in range(4)], axis=1).astype(KINDS[kind][3])
        idx, Y = c.expected(kind, v, nvec=4)
        assert np.array_equal(golden(c.rowA, c.rp, c.ci, v, X)[idx], Y)
        assert np.array_equal(D.host_x(c, kind)[np.unique(c.ci)], x[np.unique(c.ci)])


# ---- the ledger: what the GPU file's cases reach
def test_classic_dictionary_words_at_2_21_and_the_12_byte_form_beyond():
    assert _facts(D.case("W21"), **D.SPMV_SETS["dict1"])["desc_bytes"] == 4
    for name in ("W24", "W28", "W28m"):
        f = _facts(D.case(name), **D.SPMV_SETS["dict1"])
        assert (f["desc_bytes"], f["csr_form"], f["kernel"]) == (12, 1, api.KERNEL_STREAM), name


@pytest.mark.parametrize("form, want", [("pool", 4), ("pool_pairs", 8), ("pool20", 20), ("wide", 28)])
def test_every_pooled_descriptor_form_on_a_tall_and_on_a_wide_case(form, want):
    csr_form = 3 if form == "wide" else 2
    tall, wide = D.POOLED_CASES[form]
    for which in (tall, wide):
        c = D.case(*which)
        f = _facts(c, **D.SPMV_SETS[form])
        assert (f["desc_bytes"], f["csr_form"]) == (want, csr_form), (form, which, f["desc_bytes"], f["csr_form"])
    assert D.case(*tall).rowA > 2 ** 26 and D.case(*wide).colA > 2 ** 21 and D.case(*wide).rowA < 5000


def test_pooled_words_widen_to_pairs_with_the_dimension():
    """4 bytes while the window base fits beside the pattern id (pool_word_base_bits), pairs beyond: the flip the GPU cases sit on both sides of."""
    assert _facts(D.case("W21", repeat=True), **D.SPMV_SETS["pool"])["desc_bytes"] == 4
    for name in ("W24", "W28", "SQ26"):
        assert _facts(D.case(name), **D.SPMV_SETS["pool"])["desc_bytes"] == 8, name


def test_entry_modes_and_chunk_closing():
    for name in ("W21", "W24", "W28", "W28m"):
        c = D.case(name)
        for key, (em, strips) in {"em0": (0, 16), "em1": (1, 16), "em2": (2, 16), "em2x32": (2, 32)}.items():
            f = _facts(c, **D.SPMV_SETS[key])
            assert (f["entry_mode"], f["wg_strips"], f["csr_form"]) == (em, strips, 1), (name, key)
            assert f["list_entries"] >= c.last_row_len                                       # the long row is on the lists (mode 0 keeps them per strip: no chunks there)


def test_panelled_and_sliced_plans():
    want = {("W24", 2048): 33, ("W28", 2048): 64}
    for name in ("W24", "W28"):
        for kb in (16, 2048):
            f = _facts(D.case(name), **D.panel_set(kb))
            assert f["x_panels"] > 32 and f["x_panel_merge"] == 1 and f["entry_mode"] == 2, (name, kb, f["x_panels"])
            if (name, kb) in want:
                assert f["x_panels"] == want[(name, kb)]
            for passes in (1, 3):
                f = _facts(D.case(name), **D.slice_set(kb, passes))
                assert f["x_slice_passes"] == passes and f["entry_ordered"] == 0 and f["x_panels"] >= 1, (name, kb, passes)
    assert _facts(D.case("W21"), **D.panel_set(2048))["x_panels"] == 9


def test_fallback_and_first_generation_kernel():
    f = _facts(D.case("W28"), coo_mode=api.COO_FALLBACK)
    assert f["kernel"] == api.KERNEL_STREAM and f["fallback_nnz"] > 0
    c = D.case("X30")                                                                         # (XMAX: with its host products below)
    for dtype, kind in ((np.float64, "half"), (np.float32, "f32")):
        tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, c.vals(kind), dtype=dtype)
        _first_generation_facts(tm, c)
        api.Tile_destroy(tm)


def test_stream_kernel_is_refused_with_its_status_beyond_2_28_columns(capfd):
    c = D.case("X30")
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, c.vals("half"))
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        api.plan_layout_digest(tm, c.rowA, c.colA, c.nnz, kernel=api.KERNEL_STREAM)
    assert "2^24 column blocks" in capfd.readouterr().err
    api.Tile_destroy(tm)


def test_option_sets_cover_what_the_gpu_file_promises():
    S = D.SPMV_SETS
    assert {S[k].get("entry_mode") for k in S} >= {0, 1, 2} and S["em2x32"]["wg_strips"] == 32
    assert {S[k].get("desc_dict") for k in S} >= {0, 1} and {S[k].get("csr_split") for k in S} >= {1, 2, 3}
    assert {S[k].get("absorb") for k in S} >= {0, 1} and {S[k].get("dense_mode") for k in S} >= {api.DENSE_MFMA, api.DENSE_VALU}
    assert D.plan_kw({})["deterministic"] == 1 and D.plan_kw({})["placement_tries"] == 1
    assert "deterministic" not in D.plan_kw(D.slice_set(16, 1))                                # the one row without it


# ---- the host at the largest column count an int can name
def _digest(tm, rows):
    d = api.to_dict(tm, rows)
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(k.encode())
        h.update(d[k].tobytes() if isinstance(d[k], np.ndarray) else str(d[k]).encode())
    return h.hexdigest()


# Tile_matrix of DimCase(4099 x (2^31 - 16), seed 7) as the library built it BEFORE the tile counts were computed without overflow (the largest column count the old
# expression could serve): the fix changes nothing below the limit
PINNED_2_31_MINUS_16 = {
    "half": "4432deda3182b20595558c2ededdf3a40e3e459405d42d4c9027e939d9a61c57",
    "f32": "daec47ae64f84b783dae094ab2ed363999bdf70f2b59e2fa6033a7e94b5db767",
}


@pytest.mark.parametrize("kind", ["half", "f32"])
def test_tile_matrix_at_2_31_minus_16_columns_is_what_it_was(kind):
    c = D.DimCase("P", 4099, 2 ** 31 - 16, 7)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, c.vals(kind), dtype=KINDS[kind][3])
    assert (tm.tilem, tm.tilen) == (257, 2 ** 27 - 1)
    assert _digest(tm, c.rowA) == PINNED_2_31_MINUS_16[kind]
    api.Tile_destroy(tm)


@pytest.mark.parametrize("cols", [2 ** 31 - 15, 2 ** 31 - 1])
def test_tile_create_and_cpu_product_at_the_last_column_counts(cols, tmp_path):
    """(colA + 15) / 16 overflowed from 2^31 - 15 columns on and Tile_create took the process down with std::length_error.  Now: 2^27 column blocks, the product of
    tilespmv_cpu equal to the integer golden (x: zeros with the referenced columns set, never touched elsewhere), and the matrix cache takes the matrix back."""
    c = D.case("XMAX") if cols == 2 ** 31 - 1 else D.DimCase("P", 4099, cols, 7)
    kind, dtype = "f32", np.float32
    v = c.vals(kind)
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, v, dtype=dtype)
    assert (tm.tilem, tm.tilen) == (257, 2 ** 27)
    d = api.to_dict(tm, c.rowA)
    assert d["tile_columnidx"].max() == 2 ** 27 - 1 and d["tile_nnz"][-1] == c.nnz
    idx, want = c.expected(kind, v)
    full = np.zeros(c.rowA, dtype=dtype)
    full[idx] = want
    out = api.tilespmv_cpu(tm, c.rowA, c.colA, c.nnz, c.rp, c.ci, v, D.host_x(c, kind), full)
    assert out["errcount"] == 0 and np.array_equal(out["y"], full)
    if cols == 2 ** 31 - 1:
        _first_generation_facts(tm, c)
        path = os.path.join(str(tmp_path), "xmax.tile")
        api.matrix_save(tm, c.rowA, c.colA, c.nnz, path)
        tm2, r, k, z = api.matrix_load(path, dtype=dtype)
        assert (r, k, z) == (c.rowA, c.colA, c.nnz) and _digest(tm2, c.rowA) == _digest(tm, c.rowA)
        api.Tile_destroy(tm2)
    api.Tile_destroy(tm)


def test_fp64_product_at_2_31_minus_1_columns():
    c = D.case("XMAX")
    v = c.vals("half")
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, v)
    _first_generation_facts(tm, c)
    idx, want = c.expected("half", v)
    full = np.zeros(c.rowA)
    full[idx] = want
    out = api.tilespmv_cpu(tm, c.rowA, c.colA, c.nnz, c.rp, c.ci, v, D.host_x(c, "half"), full)
    assert out["errcount"] == 0 and np.array_equal(out["y"], full)
    api.Tile_destroy(tm)
