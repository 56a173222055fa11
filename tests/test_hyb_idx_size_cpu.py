"""hybIdx holds exactly the bytes the tile packer writes (csrc/tile_pack.h: whole bytes per HYB tile), also where that is more than (hybellsize + 1) / 2 + hybcoosize:
HYB tiles of odd width in a partial last tile-row of odd height.  Host side: Tile_create, tilespmv_cpu, the cache file, the Python mirror of the lengths; the same in a
stand-alone C++ program under AddressSanitizer and UBSan (nothing is loaded into python).  Matrices without such tiles keep the Tile_matrix and the cache file they had."""
import os
import subprocess

import numpy as np
import pytest

import cases
from hyb_cases import HYB_CASES, hyb_case
from tilespmv_amd import api, generators as G
from tilespmv_amd.tile_matrix import SCALARS, hyb_idx_bytes
from witness import golden, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [(np.float64, "half"), (np.float32, "f32")]


def _built(name, dtype, kind):
    m, n, rp, ci, hyb_tiles, idx_bytes = hyb_case(name)
    vals, x = witness(kind, len(ci), n, seed=40, colidx=ci)
    tm = api.Tile_create(m, n, len(ci), rp, ci, vals, dtype=dtype, hyb=True)
    return tm, (m, n, rp, ci, vals, x), hyb_tiles, idx_bytes


@pytest.mark.parametrize("dtype,kind", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(HYB_CASES))
def test_hybidx_has_the_packers_length_and_the_product_is_exact(name, dtype, kind):
    tm, (m, n, rp, ci, vals, x), hyb_tiles, idx_bytes = _built(name, dtype, kind)
    d = api.to_dict(tm, m)
    assert int(np.count_nonzero(d["Format"] == 3)) == hyb_tiles
    assert len(d["hybIdx"]) == idx_bytes == hyb_idx_bytes(tm, m)
    if hyb_tiles:
        assert set(d["tilewidth"][d["Format"] == 3].tolist()) == {1} and d["hybcoosize"] == 4 * hyb_tiles and d["hybellsize"] == m * hyb_tiles
        assert idx_bytes == (d["hybellsize"] + 1) // 2 + d["hybcoosize"] + hyb_tiles // 2           # half a byte per tile more than the old formula
        last = d["hybIdx"][-12 if m == 15 else -10:]
        assert (last[-4:] >> 4).tolist() == [0, 0, 0, 0] and (last[-4:] & 15).tolist() == [1, 2, 3, 4]   # the last tile's remainder: row 0, columns 1 .. 4 — inside the array
    want = golden(m, rp, ci, vals, x)
    got = api.tilespmv_cpu(tm, m, n, len(ci), rp, ci, vals, x, want)
    assert np.array_equal(got["y"], want), int(np.count_nonzero(got["y"] != want))
    api.Tile_destroy(tm)


@pytest.mark.parametrize("dtype,kind", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(HYB_CASES))
def test_cache_round_trip_keeps_every_byte_of_hybidx(name, dtype, kind, tmp_path):
    tm, (m, n, rp, ci, vals, x), hyb_tiles, idx_bytes = _built(name, dtype, kind)
    path = str(tmp_path / "m.tile")
    api.matrix_save(tm, m, n, len(ci), path)
    back, m2, n2, nnz2 = api.matrix_load(path, dtype)
    assert (m2, n2, nnz2) == (m, n, len(ci))
    a, b = api.to_dict(tm, m), api.to_dict(back, m)
    assert len(b["hybIdx"]) == idx_bytes
    assert [k for k in a if (a[k].tobytes() != b[k].tobytes() if isinstance(a[k], np.ndarray) else a[k] != b[k])] == []
    want = golden(m, rp, ci, vals, x)
    got = api.tilespmv_cpu(back, m, n, len(ci), rp, ci, vals, x, want)
    assert np.array_equal(got["y"], want), int(np.count_nonzero(got["y"] != want))
    # a file that ends where the old length ended is refused
    raw = open(path, "rb").read()
    if hyb_tiles:
        open(path, "wb").write(raw[:-(hyb_tiles // 2)])
        with pytest.raises(OSError):
            api.matrix_load(path, dtype)
    api.Tile_destroy(tm); api.Tile_destroy(back)


# Tile_create(hyb=True) on compat values at the commit before hybIdx's length changed: FNV-1a-64 of (the 14 scalars as int64, then every member array in declaration
# order) and of the cache file.  Neither matrix has a partial last tile-row, so both lengths coincide and nothing may move.
PARENT = {
    ("allfmt", "float64"): ("e0b6918b652f9797", "fdfc2c3e1ac59afc", 67496, 110),
    ("allfmt", "float32"): ("8d9fa4f46b29b2b1", "27a93835c10e8604", 37876, 110),
    ("circuit8k", "float64"): ("b654c52bbe6eccd8", "e635314fe0e2f403", 1534912, 474),
    ("circuit8k", "float32"): ("cdb21359b89e0cab", "4cd6a95ae4d4a57e", 1176036, 474),
}


@pytest.mark.parametrize("name,dtype", sorted(PARENT))
def test_matrices_without_a_partial_last_tile_row_keep_their_bytes(name, dtype, tmp_path):
    m, n, rp, ci = cases.SMALL[name]()
    nnz = len(ci)
    tm = api.Tile_create(m, n, nnz, rp, ci, G.compat_values(nnz, np.dtype(dtype)), dtype=np.dtype(dtype), hyb=True)
    d = api.to_dict(tm, m)
    assert int(np.count_nonzero(d["Format"] == 3)) > 0
    assert len(d["hybIdx"]) == (d["hybellsize"] + 1) // 2 + d["hybcoosize"]
    blob = np.array([d[k] for k in SCALARS], np.int64).tobytes() + b"".join(np.ascontiguousarray(d[k]).tobytes() for k in d if k not in SCALARS)
    path = str(tmp_path / "m.tile")
    api.matrix_save(tm, m, n, nnz, path)
    raw = np.fromfile(path, np.uint8)
    assert (cases.fnv1a64(np.frombuffer(blob, np.uint8)), cases.fnv1a64(raw), len(raw), len(d["hybIdx"])) == PARENT[(name, dtype)]
    api.Tile_destroy(tm)


@pytest.mark.parametrize("flags", ["-DMAT_VAL_TYPE=double", "-DMAT_VAL_TYPE=float -DTILESPMV_F32"], ids=["f64", "f32"])
def test_host_builder_and_product_under_address_and_ub_sanitizers(flags, tmp_path):
    """tests/hyb_idx_check.cpp with the host sources it needs, AddressSanitizer + UBSan, run as a program of its own: Tile_create_ex, tilespmv_cpu, the cache round trip
    and tilespmv_cpu again on the three matrices, with x, y and the CSR arrays exactly as long as the header says."""
    exe = str(tmp_path / "hyb_idx_check")
    csrc = os.path.join(ROOT, "tilespmv_amd", "csrc")
    src = [os.path.join(csrc, f) for f in ("host_tile_create.cpp", "host_tilespmv_cpu.cpp", "host_matrix_io.cpp", "host_transpose.cpp", "host_mmio.cpp")]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + flags.split() +
                   [os.path.join(ROOT, "tests", "hyb_idx_check.cpp")] + src + ["-lpthread", "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "3 cases, 0 failures" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
