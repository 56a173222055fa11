"""Why tests/witness.py exists: three ways a kernel can be wrong that the reference's compat data (values and x are i % 10) cannot see and witness data can.  A plain CSR
product in numpy stands in for the kernel; the mutants are applied to its inputs.  numpy only."""
import numpy as np
import pytest

import cases
from tilespmv_amd import generators as G
from witness import KINDS, golden, witness

MATRICES = ["allfmt_pad5", "rand500x700"]


def _mutants(m, rp, ci, vals):
    """name -> (rp, ci, vals) of the mutated product."""
    ri = np.repeat(np.arange(m), np.diff(rp[:m + 1]))
    n = int(ci.max()) + 1
    out = {}
    moved = ci.copy()                                           # 1: every column index of tile column 1 lands five tiles to the right
    sel = (ci // 16 == 1) & (ci + 80 < n)
    assert sel.any()
    moved[sel] += 80
    out["tile_column_moved_by_80"] = (rp, moved, vals)
    row = int(np.flatnonzero(np.diff(rp[:m + 1]) >= 2)[0])      # 2: two values of one row change places (the first one and the next that differs from it)
    a = int(rp[row])
    b = a + 1 + int(np.flatnonzero(vals[a + 1:rp[row + 1]] != vals[a])[0])
    swapped = vals.copy(); swapped[[a, b]] = vals[[b, a]]
    out["two_values_of_a_row_swapped"] = (rp, ci, swapped)
    keep = ci % 10 != 0                                         # 3: every entry that meets a zero of compat_x is lost
    assert not keep.all()
    rp3 = np.zeros(m + 1, dtype=rp.dtype); np.add.at(rp3, ri[keep] + 1, 1)
    out["entries_at_compat_zeros_dropped"] = (np.cumsum(rp3).astype(rp.dtype), ci[keep], vals[keep])
    return out


def _compat_y(m, rp, ci, vals, x):
    y = np.zeros(m)
    np.add.at(y, np.repeat(np.arange(m), np.diff(rp[:m + 1])), vals * x[ci])      # (small integers: exact)
    return y


@pytest.mark.parametrize("name", MATRICES)
def test_compat_data_is_blind_to_two_of_the_mutants(name):
    m, n, rp, ci = cases.SMALL[name]()
    vals, x = G.compat_values(len(ci)), G.compat_x(n)
    want = _compat_y(m, rp, ci, vals, x)
    mut = _mutants(m, rp, ci, vals)
    for k in ("tile_column_moved_by_80", "entries_at_compat_zeros_dropped"):
        assert _compat_y(m, *mut[k], x).tobytes() == want.tobytes(), k


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", MATRICES)
def test_witness_data_sees_all_three(name, kind):
    m, n, rp, ci = cases.SMALL[name]()
    vals, x = witness(kind, len(ci), n, seed=1, colidx=ci)
    want = golden(m, rp, ci, vals, x)
    for k, (rp2, ci2, v2) in _mutants(m, rp, ci, vals).items():
        assert not np.array_equal(golden(m, rp2, ci2, v2, x), want), k


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_witness_data_is_what_its_table_says(kind):
    den, kmax, xmax, dtype, bits = KINDS[kind]
    m, n, rp, ci = cases.SMALL["rand500x700"]()
    vals, X = witness(kind, len(ci), n, seed=7, nvec=4, colidx=ci)
    assert vals.dtype == dtype and X.dtype == dtype and X.shape == (n, 4)
    k = vals.astype(np.float64) * den
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= max(kmax, 4097) and (np.abs(X) >= 1).all() and np.abs(X).max() <= xmax and np.array_equal(X, np.rint(X))
    zeros = np.flatnonzero(vals == 0)
    assert 2 <= len(zeros) <= 4 and np.signbit(vals[zeros]).any() and not np.signbit(vals[zeros]).all()      # +0.0 and -0.0, nowhere else a zero
    assert (ci[zeros] % 16 == 0).any()                                                                       # one of them at local column 0 of a tile
    assert (vals > 0).sum() > len(vals) // 3 and (vals < 0).sum() > len(vals) // 3
    as_half = vals.astype(np.float16).astype(np.float64)
    nz = vals != 0
    if kind == "half":
        assert np.array_equal(as_half, vals) and (np.abs(vals[nz]) >= 2.0 ** -14).all()                     # normal halves
    if kind == "float":
        assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals) and not np.array_equal(as_half, vals)
    assert len(np.unique(np.abs(vals))) > min(kmax, 200) // 2                                                # not a handful of values, no period
    # the same seed gives the same data; golden is a column-by-column product
    v2, X2 = witness(kind, len(ci), n, seed=7, nvec=4, colidx=ci)
    assert vals.tobytes() == v2.tobytes() and X.tobytes() == X2.tobytes()
    Y = golden(m, rp, ci, vals, X)
    for j in range(4):
        assert np.array_equal(Y[:, j], golden(m, rp, ci, vals, np.ascontiguousarray(X[:, j])))
    YT = golden(m, rp, ci, vals, np.ascontiguousarray(witness(kind, len(ci), m, seed=8)[1]), transpose_cols=n)
    assert YT.shape == (n,)


def test_golden_refuses_data_that_is_not_exact_in_every_order():
    m, n, rp, ci = cases.SMALL["rand500x700"]()
    vals, x = witness("f32", len(ci), n, seed=3)
    with pytest.raises(AssertionError):
        golden(m, rp, ci, vals * np.float32(4096), x)          # 32 bits for a row sum: more than a float's 24
    with pytest.raises(AssertionError):
        golden(m, rp, ci, np.full(len(ci), 0.1), np.ones(n))   # not dyadic
