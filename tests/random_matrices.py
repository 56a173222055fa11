"""Random test matrices from ingredients (numpy only: CPU tests use them too).  ``random_matrix``: blocks of every tile format, bands, long rows, empty tile-rows, single
entries, duplicate-free scatter, odd column counts, half of them with unsorted columns inside rows.  ``stencil_matrix``: a 3-D stencil plus random extras.  A seed always
gives the same matrix (tests/test_random_matrices_cpu.py pins the hashes): tests/gpu_fuzz.py and the GPU test files draw their cases from here."""
import numpy as np

from tilespmv_amd import generators as G


def random_matrix(seed, rows_off=0):
    """``rows_off`` (0, 1, 5 or 15; applied when the matrix has more than 16 rows): the matrix loses its last rows_off rows, so that the last tile-row is partial —
    rowA = rows - rows_off, the row pointer and the column indices end there.  The structure above those rows and every rng draw are those of rows_off = 0."""
    assert rows_off in (0, 1, 5, 15)
    rng = np.random.default_rng(seed)
    tm = int(rng.integers(1, 40)); tn = int(rng.integers(1, 60))
    rows = 16 * tm
    cols = 16 * tn - int(rng.integers(0, 16)) if rng.random() < 0.5 else 16 * tn
    cols = max(cols, 1)
    R, Cc = [], []
    def add(r, c):
        r = np.asarray(r).ravel(); c = np.asarray(c).ravel()
        k = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
        R.append(r[k]); Cc.append(c[k])
    for _ in range(int(rng.integers(1, 4 * tm + 2))):
        kind = rng.integers(0, 9)
        br, bc = 16 * int(rng.integers(0, tm)), 16 * int(rng.integers(0, tn))
        if kind == 0:      # dense block
            rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij"); keep = rng.random((16, 16)) < rng.uniform(0.75, 1.0)
            add(br + rr[keep], bc + cc[keep])
        elif kind == 1:    # full rows
            for q in rng.choice(16, int(rng.integers(1, 5)), replace=False): add(np.full(16, br + q), bc + np.arange(16))
        elif kind == 2:    # full columns
            for q in rng.choice(16, int(rng.integers(1, 5)), replace=False): add(br + np.arange(16), np.full(16, bc + q))
        elif kind == 3:    # uniform width (ELL)
            w = int(rng.integers(1, 8))
            for q in range(16): add(np.full(w, br + q), bc + rng.choice(16, w, replace=False))
        elif kind == 4:    # ragged (CSR / HYB)
            for q in range(16):
                w = int(rng.integers(0, 14)); add(np.full(w, br + q), bc + rng.choice(16, w, replace=False))
        elif kind == 5:    # a few entries (COO)
            k = int(rng.integers(1, 12)); p = rng.choice(256, k, replace=False); add(br + p // 16, bc + p % 16)
        elif kind == 6:    # band segment
            hb = int(rng.integers(1, 30)); r0 = int(rng.integers(0, rows)); n = int(rng.integers(1, 200))
            for r in range(r0, min(rows, r0 + n)): add(np.full(2 * hb + 1, r), np.arange(r - hb, r + hb + 1))
        elif kind == 7:    # one long row
            r = int(rng.integers(0, rows)); k = int(rng.integers(1, cols + 1)); add(np.full(k, r), rng.choice(cols, k, replace=False))
        else:              # scattered singles
            k = int(rng.integers(1, 300)); add(rng.integers(0, rows, k), rng.integers(0, cols, k))
    r = np.concatenate(R); c = np.concatenate(Cc)
    key = np.unique(r.astype(np.int64) * cols + c)          # no duplicates (uchar per-tile counters, SURVEY S8c hazards)
    r, c = key // cols, key % cols
    if rng.random() < 0.5:                                   # unsorted columns within rows, like a symmetric .mtx
        perm = rng.permutation(len(r)); r, c = r[perm], c[perm]
    rows, cols, rp, ci = G.from_coo(rows, cols, r, c)
    if rows_off and rows > 16:
        rows -= rows_off
        rp = rp[:rows + 1].copy(); ci = ci[:int(rp[rows])].copy()
    return rows, cols, rp, ci


def stencil_matrix(seed):
    """Round 3: a 3-D stencil (7- or 27-point on g x g x gz cells, g a multiple of 16 so that grid lines are whole tile-rows) plus
    random scatter, a few dense blocks and long rows: grid strides exist, so the brick task order and the LDS x windows engage."""
    rng = np.random.default_rng(seed)
    g = 16 * int(rng.integers(1, 4)); gy = int(rng.integers(4, 11)); gz = int(rng.integers(4, 11))
    N = g * gy * gz
    idx = np.arange(N, dtype=np.int64); k, j, i = idx // (g * gy), (idx // g) % gy, idx % g
    R, Cc = [], []
    full = rng.random() < 0.5
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not full and abs(dz) + abs(dy) + abs(dx) > 1: continue
                ok = (k + dz >= 0) & (k + dz < gz) & (j + dy >= 0) & (j + dy < gy) & (i + dx >= 0) & (i + dx < g)
                R.append(idx[ok]); Cc.append(idx[ok] + (dz * gy + dy) * g + dx)
    ns = int(rng.integers(0, 400)); R.append(rng.integers(0, N, ns)); Cc.append(rng.integers(0, N, ns))
    for _ in range(int(rng.integers(0, 4))):
        br, bc = 16 * int(rng.integers(0, N // 16)), 16 * int(rng.integers(0, N // 16))
        rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij"); R.append((br + rr).ravel()); Cc.append((bc + cc).ravel())
    if rng.random() < 0.3:
        r = int(rng.integers(0, N)); kk = int(rng.integers(1, N)); R.append(np.full(kk, r)); Cc.append(rng.choice(N, kk, replace=False))
    r = np.concatenate(R); c = np.concatenate(Cc)
    key = np.unique(r.astype(np.int64) * N + c)
    return G.from_coo(N, N, key // N, key % N)
