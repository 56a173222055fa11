"""prims::scan_int (tilespmv_amd/csrc/hip_prims.hip) at the boundaries of its levels, in place, through tilespmv_csr_transpose_device: the transposer scans its colA + 1 column
counts in place.  A tile is 2048 elements: up to 2048 elements take one launch, up to 2048^2 two levels, more three.  The row pointer of A^T must be the exact prefix of the
column histogram; the column indices and source positions must be the host transposer's (tilespmv_csr_transpose)."""
import numpy as np
import pytest

from tilespmv_amd import api

pytestmark = pytest.mark.gpu

TILE = 2048
COUNTS = [2, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, TILE * TILE + TILE + 1]   # colA + 1
ROWS, PER_ROW = 1000, 200


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """PyTorch opens the device before the library does (as in tests/test_gpu_cross_forms.py)."""
    import torch
    torch.zeros(1, device="cuda")
    yield


def _matrix(cols):
    """1000 rows x 200 random columns each (unsorted, duplicates allowed), with column 0, column cols - 1 and columns m - 1, m, m + 1 of every multiple m of 2048 below 10 000
    forced to occur."""
    rng = np.random.default_rng(cols)
    ci = rng.integers(0, cols, ROWS * PER_ROW).astype(np.int32)
    forced = [0, cols - 1] + [m + d for m in range(TILE, 10000, TILE) for d in (-1, 0, 1)]
    forced = np.array(sorted({c for c in forced if 0 <= c < cols}), dtype=np.int32)
    at = rng.choice(len(ci), len(forced), replace=False)
    ci[at] = forced
    return np.arange(0, ROWS * PER_ROW + 1, PER_ROW, dtype=np.int32), ci, forced


@pytest.mark.parametrize("count", COUNTS)
def test_in_place_scan_at_the_level_boundaries(count):
    import torch
    cols = count - 1
    rp, ci, forced = _matrix(cols)
    nnz = len(ci)
    hist = np.bincount(ci, minlength=cols)
    assert (hist[forced] > 0).all()
    want_rpT = np.concatenate([[0], np.cumsum(hist)]).astype(np.int32)
    _, want_ciT, _, want_srcT = api.csr_transpose(ROWS, cols, rp, ci)
    drp, dci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    drpT = torch.full((cols + 2,), -7, dtype=torch.int32, device="cuda")
    dciT = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
    dsrcT = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
    api.csr_transpose_device(ROWS, cols, drp.data_ptr(), dci.data_ptr(), 0, drpT.data_ptr(), dciT.data_ptr(), None, dsrcT.data_ptr())
    rpT, ciT, srcT = drpT.cpu().numpy(), dciT.cpu().numpy(), dsrcT.cpu().numpy()
    wrong = np.flatnonzero(rpT[:cols + 1] != want_rpT)
    assert wrong.size == 0, "colA + 1 = %d: %d entries of rpT differ from the prefix of the histogram, the first at %d" % (count, wrong.size, wrong[0])
    assert np.array_equal(ciT[:nnz], want_ciT) and np.array_equal(srcT[:nnz], want_srcT)
    assert rpT[cols + 1] == -7 and ciT[nnz] == -7 and srcT[nnz] == -7   # nothing written past the end
