"""The value-map feature (TILESPMV_CREATE_VALUE_MAP, tilespmv_plan_update_values) where no GPU is needed: the ABI, the constants the Python side mirrors, the loud failure without a
device, and how ShardedSpMV hands every rank's multiplier its block of a new value array."""
import os
import re

import numpy as np
import pytest

from tilespmv_amd import _lib, api, generators as G
from tilespmv_amd.dist import ShardedSpMV, partition_rows

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tilespmv.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_new_symbol_is_exported():
    assert "tilespmv_plan_update_values" in _lib.DECLARED_SYMBOLS
    assert re.search(r"int\s+tilespmv_plan_update_values\s*\(\s*tilespmv_plan\s*\*\s*plan\s*,\s*const\s+MAT_VAL_TYPE\s*\*\s*d_csrVal\s*,\s*void\s*\*\s*stream\s*\)", _header())
    for dt in (np.float64, np.float32):
        assert hasattr(_lib.load(dt), "tilespmv_plan_update_values")


def test_header_constants_match_python():
    h = _header()
    assert int(re.search(r"#define\s+TILESPMV_CREATE_VALUE_MAP\s+(\d+)u", h).group(1)) == api.CREATE_VALUE_MAP == 8
    flags = [int(re.search(r"#define\s+TILESPMV_CREATE_%s\s+(\d+)u" % n, h).group(1)) for n in ("HYB", "QUIET", "CDNA4", "VALUE_MAP")]
    assert flags == [1, 2, 4, 8]
    assert int(re.search(r"TILESPMV_INFO_COUNT\s*=\s*(\d+)", h).group(1)) == len(_lib.INFO_NAMES) == 35
    assert int(re.search(r"TILESPMV_INFO_VALUE_MAP_BYTES\s*=\s*(\d+)", h).group(1)) == _lib.INFO_NAMES.index("value_map_bytes") == 34
    assert int(re.search(r"#define\s+TILESPMV_ERR_NO_VALUE_MAP\s+\((-?\d+)\)", h).group(1)) == api.ERR_NO_VALUE_MAP


def test_value_map_plan_fails_loudly_without_a_device():
    if _lib.load(np.float64).tilespmv_device_count() > 0:   # (asked here, not at collection time: the question initialises HIP in the test runner's process)
        pytest.skip("a GPU is visible: tests/test_gpu_update_values.py covers the device path")
    rows, cols, rp, ci = G.laplacian5pt(32)
    v = G.real_values(len(ci), np.float64)
    with pytest.raises(RuntimeError):
        api.Plan.from_csr(rows, cols, len(ci), rp, ci, v, value_map=True)


def test_value_map_options_without_a_device_path_are_refused():
    rows, cols, rp, ci = G.laplacian5pt(32)
    for dtype in (np.float64, np.float32):
        v = G.real_values(len(ci), dtype)
        for knobs in (dict(csr_split=0), dict(kernel=api.KERNEL_DIRECT), dict(coo_mode=api.COO_FALLBACK)):
            with pytest.raises(NotImplementedError):
                api.Plan.from_csr(rows, cols, len(ci), rp, ci, v, dtype=dtype, value_map=True, **knobs)


class _Recorder:
    """Stand-in local multiplier: remembers the block it was built from and every value block it is handed."""

    def __init__(self, rows, cols, rp, ci, v):
        self.built_from, self.updates = np.array(v), []

    def update_values(self, vals):
        self.updates.append(np.array(vals))


def test_sharded_update_hands_each_rank_its_slice():
    rows, cols, rp, ci = G.kkt_like(12)
    rows = (rows // 16) * 16
    nnz = int(rp[rows])
    v1, v2 = G.real_values(nnz, np.float64), G.real_values(nnz, np.float64, first=nnz)
    world = 3
    bounds = partition_rows(rp, rows, world)
    for rank in range(world):
        r0, r1 = int(bounds[rank]), int(bounds[rank + 1])
        lo, hi = int(rp[r0]), int(rp[r1])
        # the whole matrix on every rank: the full value array in, the rank's slice out
        s = ShardedSpMV(rank, world, rows, cols, rp, ci, v1, make_local=_Recorder, value_map=True)
        assert np.array_equal(s.local.built_from, v1[lo:hi])
        s.update_values(v2)
        assert len(s.local.updates) == 1 and np.array_equal(s.local.updates[0], v2[lo:hi])
        # bounds given: the rank holds its block only and is handed its block's values
        brp = (np.asarray(rp[r0:r1 + 1], np.int64) - lo).astype(np.int32)
        b = ShardedSpMV(rank, world, rows, cols, brp, ci[lo:hi], v1[lo:hi], make_local=_Recorder, bounds=bounds, value_map=True)
        b.update_values(v2[lo:hi])
        assert np.array_equal(b.local.updates[0], v2[lo:hi])


def test_sharded_value_map_needs_the_device_build():
    rows, cols, rp, ci = G.laplacian5pt(32)
    with pytest.raises(ValueError):
        ShardedSpMV(0, 1, 1024, cols, rp, ci, G.real_values(len(ci)), value_map=True)
