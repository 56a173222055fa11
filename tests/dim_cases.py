"""Hypersparse matrices at the dimension limits (tests/test_dim_cases_cpu.py: which plan forms they reach; tests/test_gpu_dim_limits.py: their products), numpy only.

About 20 k nonzeros in up to 2^31 - 1 columns or 2^26 + 5 rows: what the builders and kernels decide from the DIMENSIONS alone (24-bit column blocks of the unit stream, the
32-bit x index of k_units, 4 / 8 / 12 / 20 / 28-byte descriptors, the span of a 64-record chunk, panel counts, the transposer's scan levels, the tile keys of the device
Tile_create) is met at its limit by matrices that build in a fraction of a second.

x is never materialised on the host: it is a pure integer function ``x_at`` of the column number that numpy int64 and torch int64 evaluate alike (no product leaves 63 bits),
nonzero, sign-mixed and as large as the x of tests/witness.py's kinds; the values come from ``witness`` with the case's column indices, so the expected y is
``witness.golden`` on the pattern with its columns (and rows) compacted through ``np.unique`` — integer arithmetic, exact in any summation order, no tolerance."""
import functools

import numpy as np

from witness import KINDS, golden, witness

SHAPES = {   # name: (rows, cols); no count is a multiple of 16 except W28's (the stream kernel's limit itself) and the 4096 rows beside it
    "W21": (4096, 2 ** 21 + 3),
    "W24": (4099, 2 ** 24 + 3),
    "W28": (4096, 2 ** 28),
    "W28m": (4099, 2 ** 28 - 7),
    "SQ26": (2 ** 26 + 5, 2 ** 26 + 9),
    "T26": (2 ** 26 + 5, 4099),
    "X30": (4099, 2 ** 30 + 11),
    "XMAX": (4099, 2 ** 31 - 1),
}
WIDE26 = (4099, 2 ** 26 + 9)              # only ever transposed: its A^T is a tall plan whose transposer scans 2^26 + 10 counters
BRANCH_POWERS = (20, 21, 23, 24, 28, 30)  # powers of two the code branches on (4-byte word bases, chunk spans 2^20 .. 2^23, 24-bit column blocks, the stream limit)
N_CLUSTERS, CLUSTER, CLUSTER_NNZ, N_SCATTER, LAST_ROW = 40, 64, 300, 3000, 448

# ---- plan options (names of include/tilespmv.h; the numbers are TILESPMV_DENSE_MFMA / _VALU)
COMMON = dict(deterministic=1, placement_tries=1)
DENSE_MFMA, DENSE_VALU = 1, 2
CLASSIC = dict(csr_split=1)
SPMV_SETS = {   # every one runs on W21, W24, W28 and W28m in both value types
    "em0": dict(entry_mode=0, **CLASSIC),
    "em1": dict(entry_mode=1, **CLASSIC),
    "em2": dict(entry_mode=2, **CLASSIC),
    "em2x32": dict(entry_mode=2, wg_strips=32, **CLASSIC),
    "dict0": dict(desc_dict=0, **CLASSIC),
    "dict1": dict(desc_dict=1, **CLASSIC),
    "pool": dict(csr_split=2),
    "pool_pairs": dict(csr_split=2, desc_dict=2),
    "pool20": dict(csr_split=2, desc_dict=0),
    "wide": dict(csr_split=3),
    "absorb0": dict(absorb=0, entry_mode=2, **CLASSIC),
    "absorb1": dict(absorb=1, entry_mode=0, **CLASSIC),
    "mfma": dict(dense_mode=DENSE_MFMA),
    "valu": dict(dense_mode=DENSE_VALU, entry_mode=2),
}
NARROWABLE = ("em0", "em2", "absorb0", "absorb1")      # classic, entry mode 0 / 2, 16 strips: value_narrow = 2 stores halves there
# (arguments of case()) of the tall-or-square and of the wide case on which each pooled descriptor form is asserted
POOLED_CASES = {"pool": (("T26",), ("W21", 7, True)), "pool_pairs": (("SQ26",), ("W28",)), "pool20": (("SQ26",), ("W28m",)), "wide": (("T26",), ("W24",))}


def panel_set(kb):
    return dict(entry_mode=2, x_panel_kb=kb, x_panel_merge=1, **CLASSIC)


def slice_set(kb, passes):
    """Column slices add into y atomically in no fixed order: never with deterministic = 1 (exact data: still one right y)."""
    return dict(entry_mode=2, x_panel_kb=kb, x_panel_merge=0, x_slice_passes=passes, **CLASSIC)


def plan_kw(opts):
    kw = dict(opts)
    kw.setdefault("placement_tries", 1)
    if "x_slice_passes" not in kw:
        kw.setdefault("deterministic", 1)
    return kw


def x_at(j, kind, col=0):
    """x[j] (column ``col`` of a multi-vector X) as int64: a nonzero integer of magnitude <= KINDS[kind]'s largest |x|.  ``j``: a numpy or torch int64 array of indices
    below 2^31.  Only *, +, ^, >>, & and % on non-negative numbers below 2^63: both libraries give the same bits."""
    xmax = KINDS[kind][2]
    h = (j * 2654435761 + (col * 974711 + 12345)) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 40503) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 60493) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return (1 + (h >> 8) % xmax) * (1 - 2 * (h & 1))


class DimCase:
    """rows x cols CSR (sorted, duplicate-free) from a seed; built once per (shape, seed)."""

    def __init__(self, name, rows, cols, seed, repeat=False):
        """``repeat``: every cluster repeats ONE drawn pattern, and the freely placed ones sit on tile boundaries — a matrix whose pooled units share a few dozen patterns, so
        that the 4-byte pooled descriptor word (window base | pattern id | tile-row: base below 2^(30 - id bits)) is reachable at 2^21 columns."""
        self.name, self.rowA, self.colA, self.seed, self.repeat = name, rows, cols, seed, repeat
        rng = np.random.default_rng([seed, rows % 9973, cols % 9973])
        align = 16 if repeat else 1
        assert rows >= CLUSTER and cols >= CLUSTER
        corners = [(0, cols - CLUSTER), (rows - CLUSTER, 0)]                                   # first rows / last columns (its partial tile-column included), last rows / first columns
        for p in BRANCH_POWERS:                                                               # one cluster across every such column (and row) the shape has
            if 2 ** p < cols:
                corners.append((int(rng.integers(0, (rows - CLUSTER) // align + 1)) * align, min(2 ** p - CLUSTER // 2, cols - CLUSTER)))
            if 2 ** p < rows:
                corners.append((min(2 ** p - CLUSTER // 2, rows - CLUSTER), int(rng.integers(0, (cols - CLUSTER) // align + 1)) * align))
        self.straddled = [p for p in BRANCH_POWERS if 2 ** p < cols]
        while len(corners) < N_CLUSTERS:
            corners.append((int(rng.integers(0, (rows - CLUSTER) // align + 1)) * align, int(rng.integers(0, (cols - CLUSTER) // align + 1)) * align))
        r, c = [], []
        one = np.random.default_rng([seed, 4242]).integers(0, CLUSTER * CLUSTER, CLUSTER_NNZ)   # (a generator of its own: the other draws do not move)
        for r0, c0 in corners:
            k = one if repeat else rng.integers(0, CLUSTER * CLUSTER, CLUSTER_NNZ)
            d = np.arange(CLUSTER)
            r += [r0 + k // CLUSTER, r0 + d]; c += [c0 + k % CLUSTER, c0 + d]
        r.append(rng.integers(0, rows, N_SCATTER)); c.append(rng.integers(0, cols, N_SCATTER))
        last = np.unique(np.linspace(0, cols - 1, LAST_ROW).astype(np.int64))                 # one long last row over all columns: every merged list has to close chunks
        r.append(np.full(len(last), rows - 1)); c.append(last)
        cb = cols // 16 - 1                                                                   # a dense tile in the last FULL tile-column
        rb = int(rng.integers(0, rows // 16))
        d = np.arange(256)
        r.append(16 * rb + d // 16); c.append(16 * cb + d % 16)
        self.dense_tile = (rb, cb)
        key = np.unique(np.concatenate(r).astype(np.int64) * cols + np.concatenate(c).astype(np.int64))
        self.ri, cj = key // cols, key % cols
        assert self.ri.min() >= 0 and self.ri.max() == rows - 1 and cj.min() == 0 and cj.max() == cols - 1
        self.ci = cj.astype(np.int32)
        self.nnz = len(self.ci)
        rp = np.zeros(rows + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.ri, minlength=rows), out=rp[1:])
        self.rp = rp
        self.last_row_len = int(rp[rows] - rp[rows - 1])

    def vals(self, kind, second=False):
        """The case's values of a witness kind (``second``: another set for update_values)."""
        return witness(kind, self.nnz, 1, seed=2 * self.seed + (1 if second else 0), colidx=self.ci)[0]

    def expected(self, kind, vals, transpose=False, nvec=1):
        """(idx, y): the rows of the product that hold an entry (columns of A for A^T x) in ascending order, and their exact y (len(idx), or len(idx) x nvec); every other row is 0."""
        ur, rinv = np.unique(self.ri, return_inverse=True)
        uc, cinv = np.unique(self.ci.astype(np.int64), return_inverse=True)
        rp = np.zeros(len(ur) + 1, dtype=np.int64)
        np.cumsum(np.bincount(rinv, minlength=len(ur)), out=rp[1:])
        src = ur if transpose else uc                                                        # x is indexed by A's rows for the transposed product
        X = np.stack([x_at(src, kind, v) for v in range(nvec)], axis=1).astype(KINDS[kind][3])
        y = golden(len(ur), rp, cinv, vals, X[:, 0] if nvec == 1 else X, transpose_cols=len(uc) if transpose else None)
        return (uc if transpose else ur), y


@functools.lru_cache(maxsize=None)
def case(name, seed=7, repeat=False):
    rows, cols = WIDE26 if name == "WIDE26" else SHAPES[name]
    return DimCase(name, rows, cols, seed, repeat)


def host_x(c, kind, transpose=False):
    """x on the host for the CPU checks: zeros with only the referenced elements set (np.zeros maps untouched pages lazily)."""
    n, used = (c.rowA, np.unique(c.ri)) if transpose else (c.colA, np.unique(c.ci.astype(np.int64)))
    x = np.zeros(n, dtype=KINDS[kind][3])
    x[used] = x_at(used, kind)
    return x
