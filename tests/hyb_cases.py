"""Short, wide matrices whose HYB tiles sit in a partial last tile-row (numpy only; tests/hyb_idx_check.cpp builds the same ones).  Every block column holds one tile whose
row r has counts[r] entries in local columns 0 .. counts[r] - 1.  With the HYB rule on, [5, 1 x 8, 0 ...] gives a HYB tile of width 1 with 4 remainder entries: ELL part
of `rows` nibbles — an odd number, rounded up to whole bytes per tile — then 4 bytes.  (hybellsize + 1) / 2 + hybcoosize is half a byte per tile short of that."""
import numpy as np

from tilespmv_amd import generators as G

# name: (rows, block columns, counts, HYB tiles, bytes of hybIdx the packer writes)
HYB_CASES = {
    "15x640": (15, 40, [5, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], 40, 40 * (8 + 4)),
    # a HYB tile in every block column of 4000: 11 rows is the lowest odd height at which the rule can choose HYB at all (it wants more than 12 entries, a row-length
    # variation of 1 and at most 4 entries outside the equal-width part; every tile of 5, 7 or 9 rows fails one of the three)
    "11x4000": (11, 250, [5, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], 250, 250 * (6 + 4)),
    # ... so on 5 x 4000 the same rule selects no HYB tile, whatever the counts: the case is kept for the product and for hybIdx's length of 0
    "5x4000": (5, 250, [5, 1, 1, 1, 1], 0, 0),
}


def hyb_case(name):
    """(rows, cols, rowptr, colidx, HYB tiles, hybIdx bytes)"""
    rows, blocks, counts, hyb_tiles, idx_bytes = HYB_CASES[name]
    assert len(counts) == rows
    r = np.concatenate([np.full(k * blocks, i) for i, k in enumerate(counts)])
    c = np.concatenate([(16 * np.arange(blocks)[:, None] + np.arange(k)[None, :]).ravel() for k in counts])
    m, n, rp, ci = G.from_coo(rows, 16 * blocks, r, c)
    return m, n, rp, ci, hyb_tiles, idx_bytes
