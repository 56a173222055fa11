"""Test data whose product is exact in ANY summation order, and still tells entries apart (numpy only).

The reference's compat data (values and x are i % 10) makes y exact, but a tenth of it is zero and every index that is off by a multiple of 10 goes unseen — 80 columns, five
tiles, among them.  The data here is aperiodic (drawn from a seeded generator), zero-free, sign-mixed, and made of integers over a power of two that are small enough for every
partial sum of a row to be a machine number: whatever order a kernel adds in, and whichever of fp64 / fp32 it adds in, one y is right and it is compared with ``np.array_equal``.

    kind      values                                                       x                                   bits of a row sum (960 entries)
    "half"    +-k/16, 1 <= k <= 1023: normal halves, 10 mantissa bits      nonzero integers, |x| <= 2^20       40 of 53
    "float"   +-k/4096, 1 <= k < 2^20: exact floats; one of them           nonzero integers, |x| <= 2^12       42 of 53
              (4097/4096) is planted, so at least one is no half
    "f32"     +-k, 1 <= k <= 15                                            nonzero integers, |x| <= 63         20 of 24

A few values are then replaced by explicit +0.0 / -0.0 (stored entries that happen to be zero: the layout rules that look at a value, plan_tile_ops.h ell_absorb_plan, meet
them) — with ``colidx`` given, one of them at local column 0 of a tile, the slot an ELL unit takes for padding."""
import numpy as np

KINDS = {   # kind: (denominator of the values, largest numerator, largest |x|, dtype, mantissa bits)
    "half": (16, 1023, 2 ** 20, np.float64, 53),
    "float": (4096, 2 ** 20 - 1, 2 ** 12, np.float64, 53),
    "f32": (1, 15, 63, np.float32, 24),
}
N_ZEROS = 4


def witness(kind, nnz, n, seed, nvec=1, colidx=None):
    """(vals[nnz], X): X has n elements (nvec = 1) or n x nvec."""
    den, kmax, xmax, dtype, _ = KINDS[kind]
    rng = np.random.default_rng([seed, sorted(KINDS).index(kind)])
    k = rng.integers(1, kmax + 1, nnz) * rng.choice([-1, 1], nnz)
    x = rng.integers(1, xmax + 1, (n, nvec)) * rng.choice([-1, 1], (n, nvec))
    vals = (k / den).astype(dtype)
    assert np.array_equal(vals.astype(np.float64) * den, k)
    if nnz > 2 * N_ZEROS:
        spots = rng.choice(nnz, N_ZEROS + 1, replace=False)
        if colidx is not None and (np.asarray(colidx[:nnz]) % 16 == 0).any():
            spots[0] = rng.choice(np.flatnonzero(np.asarray(colidx[:nnz]) % 16 == 0))
        vals[spots[:N_ZEROS]] = [0.0, -0.0] * (N_ZEROS // 2)
        if kind == "float":
            far = spots[N_ZEROS] if spots[N_ZEROS] != spots[0] else spots[1]
            vals[far] = 4097.0 / 4096.0                      # 13 significant bits: an exact float, no half
    X = x.astype(dtype)
    return vals, (np.ascontiguousarray(X[:, 0]) if nvec == 1 else X)


def _numerators(a, what):
    """(integers, denominator): a = integers / denominator with the smallest power of two that does it."""
    a = np.asarray(a, dtype=np.float64)
    den = 1
    while not np.array_equal(a * den, np.rint(a * den)):
        den *= 2
        assert den <= 2 ** 30, "%s are not small dyadic numbers" % what
    return np.rint(a * den).astype(np.int64), den


def golden(rowA, rp, ci, vals, x, transpose_cols=None):
    """y = A x (x: n or n x nvec) — or A^T x with ``transpose_cols`` = columns of A — in int64 on the numerators, converted once to the dtype of vals.  No floating-point sum.
    Asserts what makes the data exact in any order: (longest row, or column) x max |numerator of a value| x max |numerator of x| fits the mantissa."""
    vals = np.asarray(vals); x = np.asarray(x)
    nz = int(rp[rowA])
    ri = np.repeat(np.arange(rowA), np.diff(rp[:rowA + 1]))
    cj = np.asarray(ci[:nz], dtype=np.int64)
    kv, dv = _numerators(vals[:nz], "values")
    kx, dx = _numerators(x, "x")
    src, dst, nout = (cj, ri, rowA) if transpose_cols is None else (ri, cj, transpose_cols)
    longest = int(np.bincount(dst, minlength=1).max()) if nz else 0
    bits = 24 if vals.dtype == np.float32 else 53
    worst = longest * int(np.abs(kv).max(initial=0)) * int(np.abs(kx).max(initial=0))
    assert worst < 2 ** bits, "not exact in every order: a sum can need %d bits of %d" % (worst.bit_length(), bits)
    X = kx.reshape(len(kx), -1)
    y = np.zeros((nout, X.shape[1]), dtype=np.int64)
    np.add.at(y, dst, kv[:, None] * X[src])
    out = (y.astype(np.float64) / (dv * dx)).astype(vals.dtype)
    assert np.array_equal(out.astype(np.float64) * (dv * dx), y)
    return out[:, 0] if x.ndim == 1 else out
