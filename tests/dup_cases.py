"""CSR input that stores the same (i, j) more than once (tests/test_dup_cases_cpu.py: what the cases reach, and the host product; tests/test_gpu_dup_cases.py: every plan
form on the GPU; tests/dup_check.cpp: the planted tiles under the host sanitizers), numpy only.  The library takes such input by contract (include/tilespmv.h "Repeated
entries"): y is the sum over all stored entries, a tile with a repeated position is never DNS / DNSROW / DNSCOL, and a tile with a repeated position and more than 255 entries
is refused.

PLANTED: one small matrix per rule that used to go wrong — the tile sits at block (1, 1) behind a tile-row of three single entries, so partial heights and widths are those
of a last tile-row / tile-column.  SWEEP: random matrices (tests/random_matrices.py) whose entries are stored 1, 2 or 3 times, tile by tile, with two planted tiles on top.
The entries of a planted matrix's rows are shuffled, and so are those of every sweep tile that holds repeats: repeats are not adjacent.  Data comes from tests/witness.py: every product is exact in any order and compared with np.array_equal."""
import numpy as np

from random_matrices import random_matrix
from witness import witness

SERVED, REFUSED, DENSE = "served", "refused", "dense"      # what the builders do with the planted tile
TILE_REPEAT_MAX = 255                                      # csrc/tile_select.h


def csr_keeping_repeats(rows, cols, r, c, rng=None):
    """(rows, cols, rowptr, colidx) of the entries as given — nothing summed, nothing removed; with ``rng`` the entries of every row in shuffled order."""
    r = np.asarray(r, dtype=np.int64); c = np.asarray(c, dtype=np.int64)
    assert len(r) == len(c) and (len(r) == 0 or (r.min() >= 0 and r.max() < rows and c.min() >= 0 and c.max() < cols))
    if rng is not None:
        p = rng.permutation(len(r)); r, c = r[p], c[p]
    o = np.argsort(r, kind="stable")
    rp = np.zeros(rows + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(r, minlength=rows))
    return rows, cols, rp, c[o].astype(np.int32)


def _times(pos, times):
    """positions (row, column) stored `times` times (one count for all, or one per position)"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 2)
    out = np.repeat(pos, times, axis=0)
    return out[:, 0], out[:, 1]


# ---- the tiles: local (rows, columns) of every stored entry of a tile rowlen high and collen wide
def tile_near_dense(rowlen=16, collen=16):
    """A: enough positions stored twice that the entry COUNT reaches the 75 % of the dense rule (100 of 256 in a full tile)."""
    area = rowlen * collen
    p = 100 if area == 256 else max(1, min(area, (int(area * 0.75) + 1) // 2))
    step = next(s for s in (37, 12, 11, 7, 5, 3, 2, 1) if np.gcd(s, area) == 1)
    k = (np.arange(p) * step) % area
    return _times(np.stack([k // collen, k % collen], 1), 2)


def tile_rows_of_repeats(rowlen=16, collen=16):
    """B: rows that hold exactly collen entries — as a whole row does — on half as many columns (more than 12 entries when the tile has room: not a COO tile)."""
    nrows = min(rowlen, 12 // collen + 1)
    cols = 2 * np.arange((collen + 1) // 2) if collen > 1 else np.zeros(1, dtype=np.int64)
    times = np.full(len(cols), 2); times[-1] = collen - 2 * (len(cols) - 1)
    rows = (np.arange(nrows) * 3 + 1) % rowlen if nrows * 3 <= rowlen else np.arange(nrows)
    pos = [(r, c) for r in rows for c in cols]
    times = np.tile(times, nrows)
    times[-1] = max(times[-1], 2)          # (a tile one column wide: its last row stores that column twice)
    return _times(pos, times)


def tile_columns_of_repeats(rowlen=16, collen=16):
    """B's column twin: columns that hold exactly rowlen entries on half as many rows."""
    c, r = tile_rows_of_repeats(collen, rowlen)
    return r, c


def tile_row_twice_and_full_row():
    """D: 48 entries in two rows (a multiple of 16, like three whole rows): one row of 16 columns stored twice, one whole row."""
    return _times([(2, j) for j in range(16)] + [(9, j) for j in range(16)], [2] * 16 + [1] * 16)


def tile_column_twice_and_full_column():
    r, c = tile_row_twice_and_full_row()
    return c, r


def tile_one_column_half():
    """G: one column, rows 0 .. 7 stored twice (16 entries: what a whole column holds)."""
    return _times([(i, 6) for i in range(8)], 2)


def tile_one_row_half():
    """G's row twin"""
    return _times([(0, j) for j in range(8)], 2)


def tile_ell_twice(w=5):
    """every row holds the same w columns' worth of entries, every position twice: an ELL tile of width 2 w"""
    return _times([(i, (3 * i + 2 * k) % 16) for i in range(16) for k in range(w)], 2)


def tile_hyb_repeat_in_remainder():
    """rows of 5, 1 x 8, 0 x 7 entries: the HYB rule (hyb=True) takes width 1 and four remainder entries; row 0 stores two of its columns twice, so whichever entry comes
    first, the remainder holds a repeated position"""
    return _times([(0, 1), (0, 7), (0, 12)] + [(i, (5 * i) % 16) for i in range(1, 9)], [1, 2, 2] + [1] * 8)


RAGGED = [45, 5, 40, 5, 35, 5, 30, 5, 25, 5, 20, 5, 15, 5, 5, 5]      # 255 entries


def tile_ragged(total=255):
    """a CSR-format tile with repeats: row r holds RAGGED[r] entries on columns (5 k + r) % 16; total = 256 adds one entry to the last row"""
    counts = list(RAGGED); counts[15] += total - sum(RAGGED)
    pos = [(r, (5 * k + r) % 16) for r in range(16) for k in range(counts[r])]
    return _times(pos, 1)


def tile_one_long_row():
    """one local row of 256 entries: where 8-bit row counters wrap"""
    return _times([(4, j) for j in range(16)], 16)


def tile_full():
    """256 distinct positions: stays dense"""
    return _times([(i, j) for i in range(16) for j in range(16)], 1)


def _planted(tile, rowlen=16, collen=16, alone=False):
    """the tile at block (1, 1) of a (16 + rowlen) x (16 + collen) matrix, three single entries in tile-row 0; alone: the tile is the whole matrix"""
    lr, lc = tile
    assert lr.max() < rowlen and lc.max() < collen
    if alone:
        return rowlen, collen, lr, lc
    return 16 + rowlen, 16 + collen, np.concatenate([[0, 3, 15], 16 + lr]), np.concatenate([[2, 0, min(15 + collen, 20)], 16 + lc])


PARTIAL = [(rl, cl) for rl in (1, 5, 15) for cl in (1, 7, 15)] + [(16, 7), (5, 16)]

# name: (builder of (rows, cols, r, c), hyb, outcome)
_PLANTED = {
    "A": (lambda: _planted(tile_near_dense()), False, SERVED),
    "B": (lambda: _planted(tile_rows_of_repeats()), False, SERVED),
    "B_columns": (lambda: _planted(tile_columns_of_repeats()), False, SERVED),
    "D": (lambda: _planted(tile_row_twice_and_full_row()), False, SERVED),
    "D_columns": (lambda: _planted(tile_column_twice_and_full_column()), False, SERVED),
    "F": (lambda: _planted(tile_near_dense(5, 7), 5, 7, alone=True), False, SERVED),
    "G": (lambda: _planted(tile_one_column_half()), False, SERVED),
    "G_rows": (lambda: _planted(tile_one_row_half()), False, SERVED),
    "ell_twice": (lambda: _planted(tile_ell_twice()), False, SERVED),
    "hyb_remainder": (lambda: _planted(tile_hyb_repeat_in_remainder()), True, SERVED),
    "csr_255": (lambda: _planted(tile_ragged(255)), False, SERVED),
    "csr_256": (lambda: _planted(tile_ragged(256)), False, REFUSED),
    "row_of_256": (lambda: _planted(tile_one_long_row()), False, REFUSED),
    "full_no_repeats": (lambda: _planted(tile_full()), False, DENSE),
}
for _rl, _cl in PARTIAL:
    _PLANTED["A_%dx%d" % (_rl, _cl)] = (lambda rl=_rl, cl=_cl: _planted(tile_near_dense(rl, cl), rl, cl), False, SERVED)
    _PLANTED["B_%dx%d" % (_rl, _cl)] = (lambda rl=_rl, cl=_cl: _planted(tile_rows_of_repeats(rl, cl), rl, cl), False, SERVED)
PLANTED = sorted(_PLANTED)
# the tiles the sweep plants (full 16 x 16 ones that are served)
SWEEP_TILES = [tile_near_dense, tile_rows_of_repeats, tile_columns_of_repeats, tile_row_twice_and_full_row, tile_column_twice_and_full_column, tile_one_column_half,
               tile_one_row_half, tile_ell_twice, tile_hyb_repeat_in_remainder, tile_ragged]
SWEEP_SEEDS = list(range(5000, 5024))


def tile_census(rows, cols, rp, ci):
    """per tile (tile-row, column block) in tile order: entries, distinct positions"""
    nz = int(rp[rows])
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp[:rows + 1])); c = np.asarray(ci[:nz], dtype=np.int64)
    tn = (cols + 15) // 16
    t = (r // 16) * tn + c // 16
    pos = t * 256 + (r % 16) * 16 + c % 16
    tiles, n = np.unique(t, return_counts=True)
    distinct = np.bincount(np.searchsorted(tiles, np.unique(pos) // 256), minlength=len(tiles))
    return tiles // tn, tiles % tn, n, distinct


def without_repeats(rows, cols, rp, ci):
    """the same pattern with every position stored once (columns sorted)"""
    nz = int(rp[rows])
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp[:rows + 1]))
    key = np.unique(r * cols + np.asarray(ci[:nz], dtype=np.int64))
    return csr_keeping_repeats(rows, cols, key // cols, key % cols)


def sweep_matrix(seed):
    """random_matrix(seed) with rows_off cycling through 0 / 1 / 5 / 15; then, tile by tile: three tiles in ten stay as they are, in the others every entry is stored once or
    twice more with seeded probabilities (a tile that would pass 255 entries stays as it is: it could not be served); then two planted tiles replace what two seeded blocks held (odd seeds, HYB on: the first of them is the HYB tile)."""
    rows, cols, rp, ci = random_matrix(seed, rows_off=[0, 1, 5, 15][seed % 4])
    rng = np.random.default_rng([seed, 77])
    nz = int(rp[rows])
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp[:rows + 1])); c = np.asarray(ci[:nz], dtype=np.int64)
    tn = (cols + 15) // 16
    t = (r // 16) * tn + c // 16
    p1, p2 = rng.uniform(0.1, 0.6), rng.uniform(0.0, 0.25)
    u = rng.random(nz)
    extra = (u < p1).astype(np.int64) + (u < p1 * p2)
    tiles, inv = np.unique(t, return_inverse=True)
    extra[(rng.random(len(tiles)) < 0.3)[inv]] = 0
    total = np.bincount(inv, weights=1 + extra, minlength=len(tiles))
    extra[(total > TILE_REPEAT_MAX)[inv]] = 0
    r, c = np.repeat(r, 1 + extra), np.repeat(c, 1 + extra)
    planted = []
    for i in range(2):
        if rows < 16 or cols < 16:
            break
        k = int(rng.integers(0, len(SWEEP_TILES))); bi = int(rng.integers(0, rows // 16)); bj = int(rng.integers(0, cols // 16))
        if i == 0 and seed & 1:   # (the HYB rule is on for odd seeds and almost never fires on random ingredients: the first planted tile is the one it takes)
            k = SWEEP_TILES.index(tile_hyb_repeat_in_remainder)
        lr, lc = SWEEP_TILES[k]()
        keep = ~((r // 16 == bi) & (c // 16 == bj))
        r, c = np.concatenate([r[keep], 16 * bi + lr]), np.concatenate([c[keep], 16 * bj + lc])
        planted.append((SWEEP_TILES[k].__name__, bi, bj))
    # order inside a row: by column block; inside a tile with repeats shuffled, inside a tile without them by column (dense-row / dense-column tiles assume ascending
    # columns, DESIGN.md: "restated, not repaired" — those tiles keep the bytes they had)
    t = (r // 16) * tn + c // 16
    pos, inv = np.unique(t * 256 + (r % 16) * 16 + c % 16, return_inverse=True)
    _, n_t = np.unique(t, return_counts=True); _, d_t = np.unique(pos // 256, return_counts=True)
    repeats = (n_t != d_t)[np.searchsorted(np.unique(t), t)]
    key = np.where(repeats, rng.permutation(len(r)), c % 16)
    o = np.lexsort((key, c // 16, r))
    return csr_keeping_repeats(rows, cols, r[o], c[o]) + (planted,)


# ---- plan options (tests/test_gpu_dup_cases.py; the CPU file builds every layout)
COMMON = dict(placement_tries=1, deterministic=1)
DENSE_MFMA, DENSE_VALU = 1, 2
KERNEL_DIRECT, COO_FALLBACK = 1, 2
OPTIONS = {
    "default": {},
    "csr_split=1": dict(csr_split=1), "csr_split=2": dict(csr_split=2), "csr_split=3": dict(csr_split=3),
    "entry_mode=0": dict(entry_mode=0), "entry_mode=1": dict(entry_mode=1), "entry_mode=2": dict(entry_mode=2),
    "absorb=0": dict(absorb=0), "absorb=1": dict(absorb=1),
    "desc_dict=0": dict(desc_dict=0), "desc_dict=1": dict(desc_dict=1),
    "dense=MFMA": dict(dense_mode=DENSE_MFMA), "dense=VALU": dict(dense_mode=DENSE_VALU),
    "value_narrow=2": dict(value_narrow=2, csr_split=1, entry_mode=0),      # (the narrow forms exist for classic units with per-strip or per-workgroup entry lists)
    "nt_stream=1": dict(nt_stream=1),
    "small strips": dict(strip_cost=64, split_above=150),
}
HOST_ONLY = {"kernel=DIRECT": dict(kernel=KERNEL_DIRECT), "coo=FALLBACK": dict(coo_mode=COO_FALLBACK), "csr_split=0": dict(csr_split=0)}


class Case:
    """One matrix with repeated entries and what to do with it: name = a key of the planted table, or a sweep seed."""

    def __init__(self, name, index=0):
        self.name, self.index = name, index
        if isinstance(name, str):
            build, self.hyb, self.outcome = _PLANTED[name]
            rows, cols, r, c = build()
            self.rowA, self.colA, self.rp, self.ci = csr_keeping_repeats(rows, cols, r, c, np.random.default_rng([len(r), 5]))
            self.planted, seed = [], 900 + PLANTED.index(name)
        else:
            self.hyb, self.outcome, seed = bool(name & 1), SERVED, name
            self.rowA, self.colA, self.rp, self.ci, self.planted = sweep_matrix(name)
        self.seed = seed
        self.nnz = int(self.rp[self.rowA])
        self.kind = ["half", "float", "f32"][index % 3]
        self.dtype = np.float32 if self.kind == "f32" else np.float64
        self.nvec = [1, 2, 4, 8][index % 4]
        self.mv_native = 1 + (index // 4) % 2
        tilem = (self.rowA + 15) // 16
        self.shard = (tilem // 3, 2 * tilem // 3) if index % 3 == 0 and tilem >= 3 else None

    def data(self, second=False, kind=None, cols=None):
        return witness(kind or self.kind, self.nnz, self.colA if cols is None else cols, seed=2 * self.seed + (1 if second else 0), nvec=self.nvec, colidx=self.ci)

    def __repr__(self):
        return "%s: %d x %d, %d entries, hyb=%d, %s, nvec %d (mv_native %d), shard %s, planted %s" % (
            self.name, self.rowA, self.colA, self.nnz, self.hyb, self.kind, self.nvec, self.mv_native, self.shard, self.planted)


def all_cases():
    return [Case(n, i) for i, n in enumerate(PLANTED + SWEEP_SEEDS)]


def served_cases():
    return [c for c in all_cases() if c.outcome != REFUSED]
