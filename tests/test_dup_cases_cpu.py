"""CSR input with repeated (i, j) entries, host side (tests/dup_cases.py has the cases; the GPU half is tests/test_gpu_dup_cases.py).  The contract (include/tilespmv.h
"Repeated entries"): y is the sum over ALL stored entries; a tile that stores a position twice is never DNS, DNSROW or DNSCOL — those hold one value per position, and chosen
from entry counts they lost values or were written past their slots —; a tile with a repeated position and more than 255 entries is refused (exit status 2 from the void
Tile_create_ex).  A ledger keeps the cases from going vacuous; Tile_create + tilespmv_cpu are compared with an integer golden (np.array_equal: the data of tests/witness.py is
exact in any order); every plan layout of the GPU file's option table is built by the host layout builder, which re-decodes its packed entry lists; tests/dup_check.cpp runs
the planted tiles through the host builder under AddressSanitizer and UBSan, as a program of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dup_cases as D
from tilespmv_amd import api
from witness import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSITIONAL = (4, 5, 6)                                  # TILESPMV_FMT_DNS, _DNSROW, _DNSCOL
FMT = {0: "CSR", 1: "COO", 2: "ELL", 3: "HYB", 4: "DNS", 5: "DNSROW", 6: "DNSCOL"}
CREATE = [dict(), dict(hyb=True), dict(cdna4=True), dict(transpose=True)]


@pytest.fixture(scope="module")
def cases():
    return D.all_cases()


def _formats(c, m=None, **kw):
    """Format of every tile of the case's matrix (or of matrix m), beside the census of its tiles"""
    rows, cols, rp, ci = m or (c.rowA, c.colA, c.rp, c.ci)
    nnz = int(rp[rows])
    vals, _ = D.witness("half", nnz, cols, seed=1)
    tm = api.Tile_create(rows, cols, nnz, rp, ci, vals, **kw)
    if kw.get("transpose"):                            # the tiles are those of A^T
        r = np.repeat(np.arange(rows), np.diff(rp[:rows + 1]))
        rows, cols, rp, ci = D.csr_keeping_repeats(cols, rows, ci[:nnz], r)
    d = api.to_dict(tm, rows)
    api.Tile_destroy(tm)
    bi, bj, n, distinct = D.tile_census(rows, cols, rp, ci)
    assert np.array_equal(bj, d["tile_columnidx"]) and np.array_equal(np.diff(d["tile_nnz"]), n) and np.array_equal(np.repeat(np.arange(len(d["tile_ptr"]) - 1), np.diff(d["tile_ptr"])), bi)
    return d["Format"], n, distinct, d


@pytest.fixture(scope="module")
def ledger(cases):
    return [(c, _formats(c, hyb=c.hyb)) for c in cases if c.outcome != D.REFUSED]


def test_sizes_and_exact_data(cases):
    assert len(D.SWEEP_SEEDS) >= 24 and len(set(D.PLANTED)) == len(D.PLANTED)
    for c in cases:
        assert c.rowA <= 640 and c.colA <= 960 and c.nnz == len(c.ci) > 0, c
        for kind in ("half", "float", "f32"):           # golden() asserts that every sum is exact in any order, for A and for A^T
            vals, X = c.data(kind=kind)
            golden(c.rowA, c.rp, c.ci, vals, X)
            valsT, XT = c.data(kind=kind, cols=c.rowA)
            golden(c.rowA, c.rp, c.ci, valsT, XT, transpose_cols=c.colA)
        rows = np.repeat(np.arange(c.rowA), np.diff(c.rp))
        if c.nnz > 40:                                   # the entries of a row are not in column order: repeats are not adjacent
            assert np.any((np.diff(c.ci) < 0) & (np.diff(rows) == 0)), c


def test_planted_tiles_get_a_format_that_keeps_entries_apart(ledger):
    seen = {}
    for c, (fmt, n, distinct, _) in ledger:
        if not isinstance(c.name, str):
            continue
        for kw in CREATE:
            f, n, distinct, _ = _formats(c, **dict(kw, hyb=c.hyb or kw.get("hyb", False)))
            rep = n != distinct
            if c.outcome == D.DENSE:
                assert not rep.any() and (f == 4).sum() == 1, (c, kw)
            else:
                assert rep.sum() == 1 and not np.isin(f[rep], POSITIONAL).any(), (c, kw, f.tolist())
                if not kw:
                    seen[c.name] = FMT[int(f[rep][0])]
    print(seen)
    assert seen["ell_twice"] == "ELL" and seen["csr_255"] == "CSR" and seen["A"] in ("CSR", "ELL")
    c = D.Case("hyb_remainder")
    f, n, distinct, d = _formats(c, hyb=True)
    t = int(np.flatnonzero(n != distinct)[0])
    assert f[t] == 3 and d["tilewidth"][t] == 1 and np.diff(d["hyb_coocount"])[t] == 4        # HYB of width 1, four remainder entries: two of them the same position
    c = D.Case("ell_twice")
    f, n, distinct, d = _formats(c)
    t = int(np.flatnonzero(n != distinct)[0])
    assert d["tilewidth"][t] == 10 and n[t] == 160 and distinct[t] == 80                           # width 2 w
    assert D.Case("csr_255").nnz == 255 + 3 and D.Case("csr_256").nnz == 256 + 3


def test_sweep_reaches_every_served_format_with_repeats(ledger):
    count, beside = dict.fromkeys(FMT.values(), 0), dict.fromkeys(FMT.values(), 0)
    partial_row = partial_col = shards = 0
    hyb = set()
    for c, (fmt, n, distinct, d) in ledger:
        if isinstance(c.name, str):
            continue
        rep = n != distinct
        assert not np.isin(fmt[rep], POSITIONAL).any(), c
        assert n[rep].max(initial=0) <= D.TILE_REPEAT_MAX, c
        for f in fmt[rep]:
            count[FMT[int(f)]] += 1
        for f in fmt[~rep]:
            beside[FMT[int(f)]] += 1
        partial_row += c.rowA % 16 != 0; partial_col += c.colA % 16 != 0; shards += c.shard is not None
        hyb.add(c.hyb)
        assert len(c.planted) == 2 or min(c.rowA, c.colA) < 16, c
    print(count, beside)
    assert all(count[k] >= 5 for k in ("COO", "ELL", "HYB", "CSR")), count
    assert all(beside[k] >= 5 for k in ("DNS", "DNSROW", "DNSCOL")), beside          # the duplicate-free tiles beside them keep the positional formats
    assert partial_row >= 5 and partial_col >= 5 and shards >= 5 and hyb == {False, True}
    assert {c.rowA % 16 for c, _ in ledger if not isinstance(c.name, str)} >= {0, 15, 11, 1}


def test_without_the_repeats_the_sweep_holds_the_positional_formats(ledger):
    """... in the very tiles that hold repeats: selecting by entry counts would have met all three wrong rules"""
    hit = dict.fromkeys(POSITIONAL, 0)
    for c, (fmt, n, distinct, _) in ledger:
        if isinstance(c.name, str):
            continue
        f1, n1, d1, _ = _formats(c, m=D.without_repeats(c.rowA, c.colA, c.rp, c.ci), hyb=c.hyb)
        assert np.array_equal(n1, distinct) and np.array_equal(n1, d1)
        for f in f1[n != distinct]:
            if int(f) in hit:
                hit[int(f)] += 1
    print(hit)
    assert all(v >= 3 for v in hit.values()), hit


@pytest.mark.parametrize("kw", CREATE, ids=["plain", "hyb", "cdna4", "transpose"])
def test_host_product_is_the_sum_over_all_stored_entries(cases, kw):
    for c in cases:
        if c.outcome == D.REFUSED:
            continue
        tr = bool(kw.get("transpose"))
        rows, cols = (c.colA, c.rowA) if tr else (c.rowA, c.colA)
        for kind, dtype in (("half", np.float64), ("float", np.float64), ("f32", np.float32)):
            vals, X = c.data(kind=kind, cols=cols)
            x = X if X.ndim == 1 else np.ascontiguousarray(X[:, 0])
            want = golden(c.rowA, c.rp, c.ci, vals, x, transpose_cols=c.colA if tr else None)
            tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=dtype, **dict(kw, hyb=c.hyb or kw.get("hyb", False)))
            got = api.tilespmv_cpu(tm, rows, cols, c.nnz, c.rp, c.ci, vals, x, want)      # (the CSR arguments are the reference's signature: the product reads the tiles)
            assert np.array_equal(got["y"], want), (c, kw, kind, int(np.count_nonzero(got["y"] != want)))
            api.Tile_destroy(tm)


@pytest.mark.parametrize("opt", sorted(D.OPTIONS) + sorted(D.HOST_ONLY))
def test_every_plan_layout_builds_and_its_entry_lists_decode(cases, opt):
    """the host layout builder re-decodes every packed entry list in a digest build and fails on a mismatch"""
    kw = dict(D.OPTIONS[opt] if opt in D.OPTIONS else D.HOST_ONLY[opt], **D.COMMON)
    for c in cases:
        if c.outcome == D.REFUSED:
            continue
        vals, _ = c.data(kind="half" if "value_narrow" in kw else None)
        tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, hyb=c.hyb)
        windows = [None] + ([c.shard] if c.shard else [])
        for w in windows:
            k = dict(kw, tilerow_begin=w[0], tilerow_end=w[1]) if w else kw
            digest, facts = api.plan_layout_digest(tm, c.rowA, c.colA, c.nnz, **k)
            assert facts["nnz"] > 0 and api.plan_layout_digest(tm, c.rowA, c.colA, c.nnz, **k)[0] == digest, (c, opt)
        api.Tile_destroy(tm)


def test_cache_round_trip_of_a_planted_matrix(tmp_path):
    c = D.Case("A")
    vals, x = c.data(kind="half")
    x = x if x.ndim == 1 else np.ascontiguousarray(x[:, 0])
    tm = api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals)
    path = str(tmp_path / "a.tile")
    api.matrix_save(tm, c.rowA, c.colA, c.nnz, path)
    back, m2, n2, nnz2 = api.matrix_load(path, np.float64)
    assert (m2, n2, nnz2) == (c.rowA, c.colA, c.nnz)
    a, b = api.to_dict(tm, c.rowA), api.to_dict(back, c.rowA)
    assert [k for k in a if (a[k].tobytes() != b[k].tobytes() if isinstance(a[k], np.ndarray) else a[k] != b[k])] == []
    want = golden(c.rowA, c.rp, c.ci, vals, x)
    assert np.array_equal(api.tilespmv_cpu(back, c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, x, want)["y"], want)
    api.Tile_destroy(tm); api.Tile_destroy(back)


REFUSAL_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import dup_cases as D
from tilespmv_amd import api
c = D.Case(sys.argv[1])
vals, _ = c.data(kind="half")
api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, hyb=(sys.argv[2] == "hyb"), cdna4=(sys.argv[2] == "cdna4"), transpose=(sys.argv[2] == "transpose"))
print("built")
"""


@pytest.mark.parametrize("how", ["plain", "hyb", "cdna4", "transpose"])
@pytest.mark.parametrize("name", ["csr_256", "row_of_256"])
def test_a_tile_with_repeats_and_more_than_255_entries_is_refused(name, how, tmp_path):
    """Tile_create_ex is void: it prints the tile and exits with status 2, as for an int32 offset overflow — in a child process, so that this one lives on"""
    assert D.Case(name).outcome == D.REFUSED
    script = tmp_path / "child.py"
    script.write_text(REFUSAL_CHILD % (ROOT, os.path.join(ROOT, "tests")))
    res = subprocess.run([sys.executable, str(script), name, how], capture_output=True, text=True)
    assert res.returncode == 2 and "built" not in res.stdout, (res.returncode, res.stdout[-500:], res.stderr[-2000:])
    assert "tile-row 1, column block 1: 256 entries with a repeated position" in res.stderr, res.stderr[-2000:]


@pytest.mark.parametrize("flags", ["-DMAT_VAL_TYPE=double", "-DMAT_VAL_TYPE=float -DTILESPMV_F32"], ids=["f64", "f32"])
def test_planted_tiles_under_address_and_ub_sanitizers(flags, tmp_path):
    """tests/dup_check.cpp with the host sources it needs, AddressSanitizer + UBSan, run as a program of its own (nothing is loaded into python): a row of 16 columns stored
    twice beside a whole row used to put 48 values into the 16 slots of a DNSROW tile, a column of 8 rows stored twice 16 column ids into the one of a DNSCOL tile."""
    exe = str(tmp_path / "dup_check")
    csrc = os.path.join(ROOT, "tilespmv_amd", "csrc")
    src = [os.path.join(csrc, f) for f in ("host_tile_create.cpp", "host_tilespmv_cpu.cpp", "host_transpose.cpp")]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + flags.split() +
                   [os.path.join(ROOT, "tests", "dup_check.cpp")] + src + ["-lpthread", "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout[-3000:], res.stderr[-3000:])
    assert res.returncode == 0 and "48 cases, 0 failures" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
