"""The unit loop of k_units on the device after its x index went to 32 bits (column block * 16 + window shift + nibble, one signed min against colA - 1, one 64-bit
scale-and-add for the address; pooled and wide pooled windows alike) and the value prefetch of a task's last iteration reads the plan's first word instead of the
task's last group (nobody uses it: a task's own last group, whole or partial, must still arrive through the regular prefetch).  The sums and their order are unchanged, so every y is compared with the CSR golden in float64 —
bit for bit on the integer-valued compat data, inside the project's 1e-12 (fp32 build: 1e-5) x sum |a_ij x_j| on real-valued data — and the 16 elements behind the
plan's rows keep their sentinel.  Shapes are the smallest that reach every path of the loop: tasks of every length mod 8 (odd and even batch counts, ends inside the
first 16-unit descriptor chunk and chunks later), ragged tasks at the grid's boundary, shifted windows and derived units, a column count that is no multiple of 16 (the
clamp), tasks without units, list entries in front of the loop in all three entry modes, split tile-rows behind it, narrow and wide values, 4- and 12-byte
descriptors, pooled and wide pooled plans."""
import numpy as np
import pytest

from cases import truncated_rows

pytestmark = pytest.mark.gpu

COMMON = dict(placement_tries=1, deterministic=1)
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # the project's per-product tolerances on real-valued data
SENTINEL = 777.0
_CACHE = {}


def _matrix(name):
    """(rows, n, rowptr, colidx) of a named matrix, truncated to whole tile-rows as every plan is; built once."""
    if name not in _CACHE:
        from tilespmv_amd import api, generators as G
        if name == "lap5_holes":   # 5-point 64^2 with rows 1024 .. 1535 emptied: 32 tile-rows without a nonzero, more than any strip holds (8): strips without a unit
            m, n, rp, ci = G.laplacian5pt(64)
            rp, ci = np.asarray(rp).copy(), np.asarray(ci)
            lo, hi = int(rp[1024]), int(rp[1536])
            ci = np.ascontiguousarray(np.concatenate([ci[:lo], ci[hi:]]))
            rp[1024:1536] = lo; rp[1536:] -= hi - lo
        else:
            m, n, rp, ci = {"lap5_64": lambda: G.laplacian5pt(64), "lap7_16": lambda: G.laplacian7pt(16), "lap5_50": lambda: G.laplacian5pt(50),
                            "fem_hex": lambda: G.fem_hex(6, 6, 6, 3), "fem_hex_shuffled": lambda: G.fem_hex(8, 8, 8, 3, shuffle=64), "band": lambda: G.band(3000, 40)}[name]()
        _CACHE[name] = (truncated_rows(m), n, rp, ci)
    return _CACHE[name]


def _data(name, dtype):
    """[(values, x, exact, golden y, sum |a_ij x_j| per row)]: the compat data, and real-valued data whose values are exact floats (multiples of 2^-12 below 2^8: a narrow
    plan can hold them) with x ~ U(-1, 1); goldens in float64 from the CSR, computed once per matrix and build."""
    key = (name, np.dtype(dtype))
    if key not in _CACHE:
        from tilespmv_amd import generators as G
        rows, n, rp, ci = _matrix(name)
        nnz = len(ci)
        rng = np.random.default_rng(2024)
        sets = [(G.compat_values(nnz, dtype), G.compat_x(n, dtype), True),
                ((rng.integers(-2 ** 20, 2 ** 20, nnz).astype(np.float64) / 4096.0).astype(dtype), G.real_x(n, nnz, dtype), False)]
        k = int(rp[rows])
        ri = np.repeat(np.arange(rows), np.diff(rp[:rows + 1]))
        out = []
        for vals, x, exact in sets:
            prod = vals[:k].astype(np.float64) * x.astype(np.float64)[ci[:k]]
            y = np.zeros(rows); b = np.zeros(rows)
            np.add.at(y, ri, prod); np.add.at(b, ri, np.abs(prod))
            out.append((vals, x, exact, y, b))
        _CACHE[key] = out
    return _CACHE[key]


def _run(plan, x, rows):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((rows + 16,), SENTINEL, dtype=xd.dtype, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert (y[rows:] == SENTINEL).all(), "wrote past the end of y"
    return y[:rows]


def _check(y, want, bound, exact, dtype, what):
    err = np.abs(y.astype(np.float64) - want)
    print(what, "max |y - y_ref| / sum|a x| = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    if exact:
        assert np.array_equal(y.astype(np.float64), want), (what, int(np.count_nonzero(y != want)))
    else:
        assert (err <= TOL[np.dtype(dtype)] * bound + 1e-300).all(), what


def _plans(name, dtype, option_sets, facts=None, hyb=False):
    """Every option set on both value sets of one matrix; fp64 option sets with ``narrow`` run with value_narrow 1 and 0 and their y must be the same in every bit.
    Returns the plan facts per option set (of the compat data)."""
    import torch
    from tilespmv_amd import api
    torch.zeros(1, device="cuda")   # (PyTorch opens the device before the library does)
    rows, n, rp, ci = _matrix(name)
    nnz = len(ci)
    infos = []
    for si, (vals, x, exact, want, bound) in enumerate(_data(name, dtype)):
        tm = api.Tile_create(rows, n, nnz, rp, ci, vals, dtype=dtype, hyb=hyb)
        for kw in option_sets:
            kw = dict(kw)
            narrow = kw.pop("narrow", False) and np.dtype(dtype) == np.float64
            ys = []
            for vn in ((1, 0) if narrow else (0,)):
                p = api.Plan(tm, rows, n, nnz, value_narrow=vn, **COMMON, **kw)
                info = p.info()
                assert info["unit_value_bytes"] == (4 if vn or np.dtype(dtype) == np.float32 else 8), (name, kw, vn, info)
                for k, f in (facts or {}).items():
                    assert f(info[k]), (name, kw, k, info[k])
                ys.append(_run(p, x, rows))
                p.close()
                _check(ys[-1], want, bound, exact, dtype, (name, np.dtype(dtype).name, kw, "narrow" if vn else "wide", "compat" if exact else "real"))
                if si == 0 and vn == (1 if narrow else 0):
                    infos.append(info)
            if narrow:
                assert np.array_equal(ys[0], ys[1]), (name, kw, exact, int(np.count_nonzero(ys[0] != ys[1])))
        api.Tile_destroy(tm)
    return infos


STRIP_COSTS = list(range(100, 900, 100))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("desc_dict", [1, 0])
@pytest.mark.parametrize("name", ["lap5_64", "lap7_16"])
def test_task_lengths_of_every_residue(name, desc_dict, dtype):
    """5-point 64^2 and 7-point 16^3 (4096 rows each): 5 and 7 units per interior tile-row, strips of 1 .. 8 tile-rows as strip_cost goes from 100 to 800 — 5 k and 7 k units per
    task: every residue mod 8, so odd and even batch counts and tasks that end on either step of a trip, in the first descriptor chunk (up to 16 units) and behind it; the
    tile-rows at the grid's boundary give ragged tasks.  The strips must really differ: the number of tasks never grows with strip_cost, falls from the first to the last and
    takes at least five values (the planner gives 300 and 400, and 700 and 800, the same strips on these grids).  Dictionary (4-byte) and 12-byte descriptors; fp64 narrow == wide."""
    infos = _plans(name, dtype, [dict(strip_cost=sc, desc_dict=desc_dict, narrow=True) for sc in STRIP_COSTS],
                   facts={"desc_bytes": lambda v: v == (4 if desc_dict else 12), "entry_mode": lambda v: v == 0, "csr_form": lambda v: v == 1})
    tasks = [i["num_tasks"] for i in infos]
    print(name, "tasks per strip_cost", tasks)
    assert all(a >= b for a, b in zip(tasks, tasks[1:])) and tasks[0] > tasks[-1] and len(set(tasks)) >= 5, tasks


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("entry_mode", [0, 1, 2])
def test_list_entries_in_front_of_the_units(entry_mode, dtype):
    """5-point 50^2 with its CSR tiles split into units and list entries (2500 rows and columns, truncated to 2496 rows; 2500 is no multiple of 16: the last column block is
    partial): per-strip entries (0) and workgroup entries (2) run the loop behind their entry phase, the wavefront mode (1) fetches its first batch before it (and has no narrow form)."""
    _plans("lap5_50", dtype, [dict(csr_split=1, entry_mode=entry_mode, narrow=entry_mode != 1)],
           facts={"list_entries": lambda v: v > 0, "entry_mode": lambda v: v == entry_mode})


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_strips_without_units(dtype):
    """32 consecutive empty tile-rows, more than any strip holds (8): tasks without a unit skip the loop and store zeros."""
    rows, n, rp, ci = _matrix("lap5_holes")
    assert (np.diff(rp[1024:1537]) == 0).all()
    _plans("lap5_holes", dtype, [dict(narrow=True), dict(strip_cost=300, desc_dict=0, narrow=True)], facts={"entry_mode": lambda v: v == 0})
    for _, _, _, want, _ in _data("lap5_holes", dtype):
        assert (want[1024:1536] == 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("entry_mode", [0, 2])
def test_split_tile_rows_behind_the_loop(entry_mode, dtype):
    """Band of half-width 40 (3000 columns: a partial last column block) with its dense tiles as units, strips of cost 32 and rows cut above 200: tasks of several chunks
    whose sums meet in the split-row slots."""
    from tilespmv_amd import api
    _plans("band", dtype, [dict(dense_mode=api.DENSE_VALU, entry_mode=entry_mode, split_above=200, strip_cost=32, narrow=True)],
           facts={"num_split_rows": lambda v: v > 0, "entry_mode": lambda v: v == entry_mode})


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_pooled_windows(dtype):
    """fem_hex(6, 6, 6, 3): pooled units (csr_form 2: window base + column nibble) — as the rule picks the plan (wavefront entries on this small grid), with per-strip and
    with workgroup entries, with the pattern dictionary and without."""
    _plans("fem_hex", dtype, [dict(), dict(entry_mode=0), dict(entry_mode=2), dict(entry_mode=0, desc_dict=0)], facts={"csr_form": lambda v: v == 2})


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_wide_pooled_windows(dtype):
    """fem_hex(8, 8, 8, 3) shuffled inside windows of 64 nodes, wide pooled units asked for (csr_form 3: window base + a byte of column offset, up to 255)."""
    _plans("fem_hex_shuffled", dtype, [dict(csr_split=3), dict(csr_split=3, entry_mode=0), dict(csr_split=3, entry_mode=2)], facts={"csr_form": lambda v: v == 3})
