"""The cases of the cross-feature sweep (tests/test_cross_forms_cpu.py: which plan forms they reach; tests/test_gpu_cross_forms.py: their y), numpy only.
Seed s gives a random matrix (tests/random_matrices.py) with its last 0 / 1 / 5 / 15 rows cut off (s % 4), HYB on for odd s, and — from s alone — one row of TABLE, a data
kind (tests/witness.py), a builder, a shard window and a multi-vector count.  The table has 13 rows so that every row meets every rows_off, both HYB settings, both builders
and the shard over the seeds."""
import numpy as np

from random_matrices import random_matrix
from witness import witness

# 3000 .. 3047, and six more: the HYB rule almost never fires on these ingredients (none of the 24 odd seeds below 3048 has a HYB tile), so the odd seeds after them whose
# matrix holds one — and whose table row and data kind give a 2-byte plan — are appended (tests/test_cross_forms_cpu.py checks that they do hold one)
HYB_SEEDS = [3121, 3235, 3287, 3341, 3351, 3393]
SEEDS = list(range(3000, 3048)) + HYB_SEEDS
GROUPS = [SEEDS[k:k + 8] for k in range(0, len(SEEDS), 8)]
COMMON = dict(placement_tries=1, deterministic=1)
DENSE_MFMA, DENSE_VALU = 1, 2
SMALL_STRIPS = dict(strip_cost=64, split_above=150)          # strips of a few tile-rows, tile-rows cut above 6 x 64 entries: split rows on matrices this small
NARROW = dict(csr_split=1)                                   # the narrow value forms exist for classic units with per-strip (0) or per-workgroup (2) entry lists only

# (plan options, transpose, value_map); value_narrow = 2 rows ask for halves, and get them on "half" data
TABLE = [
    (dict(value_narrow=2, entry_mode=0, **NARROW), False, False),
    (dict(value_narrow=2, entry_mode=2, desc_dict=0, **NARROW), False, False),
    (dict(csr_split=2, entry_mode=1), False, False),
    (dict(value_narrow=2, entry_mode=0, **NARROW, **SMALL_STRIPS), False, False),
    (dict(value_narrow=2, entry_mode=2, desc_dict=1, dense_mode=DENSE_VALU, **NARROW), False, False),
    (dict(csr_split=3, entry_mode=2, absorb=0, dense_mode=DENSE_MFMA), False, False),
    (dict(value_narrow=2, entry_mode=2, absorb=1, **NARROW, **SMALL_STRIPS), False, False),
    (dict(value_narrow=1, entry_mode=0, dense_mode=DENSE_MFMA, **NARROW), False, False),
    (dict(value_narrow=2, entry_mode=0, absorb=0, desc_dict=0, dense_mode=DENSE_VALU, **NARROW), False, False),
    (dict(value_narrow=2, entry_mode=0, **NARROW, **SMALL_STRIPS), True, False),
    (dict(value_narrow=2, entry_mode=2, **NARROW), False, True),
    (dict(csr_split=1, entry_mode=1, **SMALL_STRIPS), False, False),
    (dict(csr_split=3, entry_mode=0, desc_dict=1), True, False),
]


class Case:
    """Everything the two halves need to know about seed s, and nothing they computed."""

    def __init__(self, seed):
        i = seed - SEEDS[0]
        self.seed, self.hyb = seed, bool(seed & 1)
        self.rowA, self.colA, self.rp, self.ci = random_matrix(seed, rows_off=[0, 1, 5, 15][seed % 4])
        self.nnz = int(self.rp[self.rowA])
        self.row = i % len(TABLE)
        opts, self.transpose, self.value_map = TABLE[self.row]
        self.opts = dict(opts)
        self.narrow = self.opts.get("value_narrow", 0)
        # data: fp32 on every other visit of a wide row; narrow rows get halves, every fifth seed floats that are no halves
        if not self.narrow and (i // len(TABLE)) % 2 == 0:
            self.kind, self.dtype = "f32", np.float32
        else:
            self.kind, self.dtype = ("float" if i % 5 == 4 or self.narrow == 1 else "half"), np.float64
        self.device_build = self.transpose or self.value_map or (i // 2) % 2 == 1      # Plan.from_csr; otherwise api.Plan on the host's Tile_matrix
        self.rows, self.cols = (self.colA, self.rowA) if self.transpose else (self.rowA, self.colA)   # of the plan
        tilem = (self.rows + 15) // 16
        self.shard = (tilem // 3, 2 * tilem // 3) if i % 3 == 2 and tilem >= 3 else None   # the middle third of the tile-rows
        self.nvec = [1, 2, 4, 8][(i // 3) % 4]
        if self.nvec > 1:
            self.opts["mv_native"] = 1 + (i // 5) % 2
        self.plan_kw = dict(self.opts, **COMMON)
        if self.shard:
            self.plan_kw.update(tilerow_begin=self.shard[0], tilerow_end=self.shard[1])

    def data(self, second=False):
        """(vals, X): X has `cols of A^T`-many rows for a transposed plan; the second set is what update_values brings."""
        return witness(self.kind, self.nnz, self.cols, seed=2 * self.seed + (1 if second else 0), nvec=self.nvec, colidx=self.ci)

    def wants_two_bytes(self):
        """value_narrow = 2 on half data, no value map (a flagged plan's layout follows the pattern alone: 8 bytes)."""
        return self.narrow == 2 and self.kind == "half" and not self.value_map

    def __repr__(self):
        return "seed %d: %d x %d, %d nnz, hyb=%d, table row %d %s%s%s, %s %s, %s, shard %s, nvec %d" % (
            self.seed, self.rowA, self.colA, self.nnz, self.hyb, self.row, self.opts, " transpose" if self.transpose else "", " value_map" if self.value_map else "",
            self.kind, np.dtype(self.dtype).name, "from_csr" if self.device_build else "host Tile_matrix", self.shard, self.nvec)


def host_tile_matrix(api, c, vals):
    """The host Tile_matrix of the case's plan (of A^T for a transposed case)."""
    return api.Tile_create(c.rowA, c.colA, c.nnz, c.rp, c.ci, vals, dtype=c.dtype, hyb=c.hyb, transpose=c.transpose)


def layout_facts(api, c, value_narrow=None):
    """Facts of the case's plan from the host layout builder (no GPU): what the device must report too."""
    vals, _ = c.data()
    tm = host_tile_matrix(api, c, vals)
    kw = dict(c.plan_kw)
    if value_narrow is not None:
        kw["value_narrow"] = value_narrow
    _, facts = api.plan_layout_digest(tm, c.rows, c.cols, c.nnz, **kw)
    d = api.to_dict(tm, c.rows)
    facts["hyb_tiles"] = int(np.count_nonzero(d["Format"] == 3))
    api.Tile_destroy(tm)
    return facts
