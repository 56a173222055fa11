"""tests/random_matrices.py gives the matrices the generators of tests/gpu_fuzz.py gave before they moved (same rng call sequence): the hashes below were recorded from
gpu_fuzz.py at the commit before the move.  rows_off only cuts rows off the end."""
import numpy as np
import pytest

import cases
from random_matrices import random_matrix, stencil_matrix

# seed: (rows, cols, FNV-1a-64 of rowptr, of colidx) — int32 arrays
RANDOM = {
    1000: (128, 496, "e20820ee4c4f3eaa", "7ae7fbb1f84ca8e4"),
    1001: (576, 584, "807f1cd822a435f0", "2871a63d7a7e35cc"),
    1002: (384, 354, "3e769e22c28c558f", "b1d7f4cf67690cc4"),
    1003: (192, 188, "ddd5609ce3419cbc", "20f753f7396e7af9"),
    2000: (160, 544, "7f5dcb4576246997", "d5e80be1c16fb92c"),
    2001: (16, 393, "882e2c8316643da6", "9416e005df83e626"),
    2002: (528, 848, "a668de3e945d8f8f", "8f675034d3d0af88"),
    2003: (512, 288, "b793c8b4929a2111", "d699994ca0a2c443"),
}
STENCIL = {   # (the seeds of these two ranges that gpu_fuzz.check gives to stencil_matrix: seed % 4 == 1)
    1001: (3456, 3456, "c77106ddfcc4b1cd", "e5d1e1ab2bb808c3"),
    2001: (480, 480, "36ea3580cf56af39", "63e45ced4eebe8b0"),
}


def _pin(gen, seed):
    m, n, rp, ci = gen(seed)
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    return m, n, cases.fnv1a64(rp), cases.fnv1a64(ci)


@pytest.mark.parametrize("seed", sorted(RANDOM))
def test_random_matrix_is_the_matrix_of_the_parent_commit(seed):
    assert _pin(random_matrix, seed) == RANDOM[seed]


@pytest.mark.parametrize("seed", sorted(STENCIL))
def test_stencil_matrix_is_the_matrix_of_the_parent_commit(seed):
    assert _pin(stencil_matrix, seed) == STENCIL[seed]


@pytest.mark.parametrize("rows_off", [0, 1, 5, 15])
def test_rows_off_cuts_rows_off_the_end_and_changes_nothing_else(rows_off):
    for seed in (1000, 1002, 2001, 2003):                   # (2001 has 16 rows: left alone)
        m, n, rp, ci = random_matrix(seed)
        m2, n2, rp2, ci2 = random_matrix(seed, rows_off=rows_off)
        want = m - rows_off if m > 16 else m
        assert (m2, n2) == (want, n) and len(rp2) == want + 1 and len(ci2) == rp2[want]
        assert np.array_equal(rp2, rp[:want + 1]) and np.array_equal(ci2, ci[:rp[want]])
    with pytest.raises(AssertionError):
        random_matrix(1000, rows_off=3)
