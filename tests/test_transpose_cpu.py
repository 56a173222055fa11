"""Transposed products where no GPU is needed (TILESPMV_CREATE_TRANSPOSE, tilespmv_csr_transpose): the host transposer against the definition — A's entries in
CSR order, stably sorted by column — the host Tile_create of A^T, the ABI, the compiled device transposer, and the loud failure without a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
from tilespmv_amd import _lib, api, generators as G  # noqa: E402
from tilespmv_amd.tile_matrix import to_dict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tilespmv.h")


def definition(rows, cols, rp, ci, v):
    """The transpose by its definition: order = stable argsort of the block's columns."""
    lo, hi = int(rp[0]), int(rp[rows])
    c = np.asarray(ci[lo:hi], np.int64)
    order = np.argsort(c, kind="stable")
    row_of = np.repeat(np.arange(rows), np.diff(np.asarray(rp[:rows + 1], np.int64)))
    rpT = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=cols))]).astype(np.int32)
    vT = None if v is None else np.asarray(v)[lo:hi][order]
    return rpT, row_of[order].astype(np.int32), vT, (order + lo).astype(np.int32)


def check(rows, cols, rp, ci, v, dtype=None):
    got = api.csr_transpose(rows, cols, rp, ci, v, dtype=dtype)
    want = definition(rows, cols, rp, ci, v)
    for name, g, w in zip(("rpT", "ciT", "vT", "srcT"), got, want):
        if w is None:
            assert g is None, name
            continue
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, rows, cols)
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_small_and_medium_cases_match_the_definition(dtype):
    for name in sorted(cases.SMALL) + sorted(cases.MEDIUM):
        rows, cols, rp, ci = (cases.SMALL.get(name) or cases.MEDIUM[name])()
        nnz = int(rp[rows])
        check(rows, cols, rp, ci, G.real_values(nnz, dtype), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rectangular_empty_and_degenerate(dtype):
    mats = [G.random_uniform(3000, 197, 0.03, 1),      # tall, cols % 16 != 0
            G.random_uniform(83, 5011, 0.02, 2),       # wide
            G.from_coo(200, 300, [0, 5, 5, 199], [299, 0, 17, 150]),   # empty rows and columns
            (50, 70, np.zeros(51, np.int32), np.zeros(0, np.int32)),   # nnz 0
            (0, 9, np.zeros(1, np.int32), np.zeros(0, np.int32)),      # no rows
            (5, 1, np.array([0, 1, 1, 3, 3, 4], np.int32), np.zeros(4, np.int32))]   # one column
    for rows, cols, rp, ci in mats:
        nnz = int(rp[rows])
        rpT, ciT, vT, srcT = check(rows, cols, rp, ci, G.real_values(nnz, dtype), dtype)
        assert len(rpT) == cols + 1 and rpT[-1] == nnz
    # big enough for the threaded passes (several chunks)
    rows, cols, rp, ci = G.powerlaw(400000)
    check(rows, cols, rp, ci, G.real_values(int(rp[rows]), dtype), dtype)


def test_duplicates_unsorted_rows_and_a_row_block():
    rng = np.random.default_rng(3)
    rows, cols = 700, 333
    lens = rng.integers(0, 12, rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, 40, int(rp[-1])).astype(np.int32) * 8 % cols   # unsorted rows with many duplicates
    v = rng.standard_normal(int(rp[-1]))
    rpT, ciT, vT, srcT = check(rows, cols, rp, ci, v)
    assert np.array_equal(vT, v[srcT])
    # rp[0] != 0: rows 100 .. 400 of the matrix, positions stay the caller's
    r0, r1 = 100, 400
    blk = rp[r0:r1 + 1]
    assert blk[0] != 0
    bT = check(r1 - r0, cols, blk, ci, v)
    assert bT[3].min() >= blk[0] and bT[3].max() < blk[-1]
    assert np.array_equal(bT[2], v[bT[3]])
    # without values
    rpT2, ciT2, vT2, srcT2 = check(rows, cols, rp, ci, None)
    assert vT2 is None and np.array_equal(srcT2, srcT)


def test_transposing_twice_sorts_every_row_stably():
    rng = np.random.default_rng(4)
    rows, cols = 300, 211
    lens = rng.integers(0, 20, rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, cols, int(rp[-1])).astype(np.int32)
    v = rng.standard_normal(int(rp[-1]))
    rpT, ciT, vT, _ = api.csr_transpose(rows, cols, rp, ci, v)
    rpTT, ciTT, vTT, _ = api.csr_transpose(cols, rows, rpT, ciT, vT)
    assert np.array_equal(rpTT, rp)
    for r in range(rows):
        a, b = rp[r], rp[r + 1]
        order = np.argsort(ci[a:b], kind="stable")
        assert np.array_equal(ciTT[a:b], ci[a:b][order]) and np.array_equal(vTT[a:b], v[a:b][order])


def test_bad_input_is_refused():
    rp = np.array([0, 2, 3], np.int32)
    with pytest.raises(ValueError):
        api.csr_transpose(2, 4, rp, np.array([0, 4, 1], np.int32), np.ones(3))       # column outside [0, cols)
    with pytest.raises(ValueError):
        api.csr_transpose(2, 4, np.array([0, 3, 2], np.int32), np.array([0, 1, 1], np.int32), np.ones(3))   # decreasing row pointer
    lib = _lib.load(np.float64)
    import ctypes as C
    out = np.zeros(5, np.int32)
    bad = np.array([0, -1, 1], np.int32)
    assert lib.tilespmv_csr_transpose(2, 4, rp.ctypes.data_as(C.POINTER(C.c_int)), bad.ctypes.data_as(C.POINTER(C.c_int)), None,
                                      out.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_int)), None, None) == -1


def _same_tiles(a, b, rows):
    da, db = to_dict(a, rows), to_dict(b, rows)
    bad = []
    for k in da:
        if isinstance(da[k], np.ndarray):
            if da[k].shape != db[k].shape or da[k].tobytes() != db[k].tobytes():
                bad.append(k)
        elif da[k] != db[k]:
            bad.append(k)
    return bad


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tile_create_transpose_is_tile_create_of_the_transpose(dtype):
    for i, (rows, cols, rp, ci) in enumerate([cases.SMALL["allfmt_pad5"](), cases.SMALL["one_long_row"](), cases.SMALL["rand500x700"](), cases.MEDIUM["kkt12"](),
                                              G.random_uniform(2000, 345, 0.02, 5)]):
        nnz = int(rp[rows])
        v = G.real_values(nnz, dtype)
        rpT, ciT, vT, _ = api.csr_transpose(rows, cols, rp, ci, v)
        for kw in (dict(), dict(hyb=True), dict(cdna4=True)):
            a = api.Tile_create(rows, cols, nnz, rp, ci, v, dtype=dtype, transpose=True, **kw)
            b = api.Tile_create(cols, rows, nnz, rpT, ciT, vT, dtype=dtype, **kw)
            try:
                assert a.tilem == (cols + 15) // 16 and a.tilen == (rows + 15) // 16
                assert _same_tiles(a, b, cols) == [], (i, kw)
            finally:
                api.Tile_destroy(a); api.Tile_destroy(b)


def test_tile_create_transpose_serves_the_host_plan_layout():
    """The host-built plan of A^T (Tile_create(transpose=True) + the plan builder, here its host-only layout) is the plan of the transposed arrays."""
    rows, cols, rp, ci = G.random_uniform(1000, 403, 0.02, 6)
    nnz = int(rp[rows])
    v = G.real_values(nnz)
    rpT, ciT, vT, _ = api.csr_transpose(rows, cols, rp, ci, v)
    a = api.Tile_create(rows, cols, nnz, rp, ci, v, transpose=True)
    b = api.Tile_create(cols, rows, nnz, rpT, ciT, vT)
    (da, fa), (db, fb) = api.plan_layout_digest(a, cols, rows, nnz), api.plan_layout_digest(b, cols, rows, nnz)
    assert da == db
    assert [k for k in fa if not k.endswith("_us") and fa[k] != fb[k]] == []
    assert fa["rows"] == cols
    api.Tile_destroy(a); api.Tile_destroy(b)


def test_symbols_and_constants():
    h = open(HEADER).read()
    for name in ("tilespmv_csr_transpose", "tilespmv_csr_transpose_device"):
        assert name in _lib.DECLARED_SYMBOLS
        assert re.search(r"int\s+%s\s*\(" % name, h)
        for dt in (np.float64, np.float32):
            assert hasattr(_lib.load(dt), name)
    assert int(re.search(r"#define\s+TILESPMV_CREATE_TRANSPOSE\s+(\d+)u", h).group(1)) == api.CREATE_TRANSPOSE == 16
    assert int(re.search(r"TILESPMV_INFO_COUNT\s*=\s*(\d+)", h).group(1)) == len(_lib.INFO_NAMES) == 35   # no new plan fact


def _device_asm(dt, out):
    defs = ["-DMAT_VAL_TYPE=double"] if dt == "f64" else ["-DMAT_VAL_TYPE=float", "-DTILESPMV_F32"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950", "-munsafe-fp-atomics", "-w"] + defs +
                   ["-S", "--cuda-device-only", os.path.join(ROOT, "tilespmv_amd/csrc/hip_transpose.hip"), "-o", out], check=True)
    return open(out).read()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_device_transposer_compiles_without_scratch(tmp_path, dt):
    s = _device_asm(dt, str(tmp_path / (dt + ".s")))
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S)
    names = [k for k, _ in kernels]
    for want in ("k_tr_hist", "k_tr_rowid", "k_tr_gather"):
        assert any(want in n for n in names), (want, names)
    assert not any("radix" in n or "rocprim" in n for n in names), names   # the sort is hip_prims.hip's instantiation, not a new one
    spills = {name: int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) for name, body in kernels}
    assert not {k: v for k, v in spills.items() if v}, spills


def test_transposed_plan_fails_loudly_without_a_device():
    if _lib.load(np.float64).tilespmv_device_count() > 0:   # (asked here, not at collection time: the question initialises HIP in the test runner's process)
        pytest.skip("a GPU is visible: tests/test_gpu_transpose.py covers the device path")
    rows, cols, rp, ci = G.random_uniform(200, 90, 0.05, 7)
    v = G.real_values(len(ci), np.float64)
    for kw in (dict(), dict(value_map=True)):
        with pytest.raises(RuntimeError):
            api.Plan.from_csr(rows, cols, len(ci), rp, ci, v, transpose=True, **kw)
    with pytest.raises(RuntimeError):
        api.Tile_create_device(rows, cols, len(ci), rp, ci, v, transpose=True)
