"""hybIdx on the device (tests/test_hyb_idx_size_cpu.py has the host side): Tile_create_device allocates, packs and downloads the packer's exact byte total, so short, wide
matrices whose HYB tiles sit in a partial last tile-row come back byte for byte the host's Tile_matrix, and plans of them — from the host matrix and built on the
device — give the exact y."""
import numpy as np
import pytest

from hyb_cases import HYB_CASES, hyb_case
from tilespmv_amd import api
from tilespmv_amd.tile_matrix import to_dict
from witness import golden, witness

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    import torch
    torch.zeros(1, device="cuda")
    yield


@pytest.mark.parametrize("dtype,kind", [(np.float64, "half"), (np.float32, "f32")], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(HYB_CASES))
def test_device_builder_and_plans_on_hyb_tiles_in_a_partial_last_tile_row(name, dtype, kind):
    import torch
    m, n, rp, ci, hyb_tiles, idx_bytes = hyb_case(name)
    nnz = len(ci)
    vals, x = witness(kind, nnz, n, seed=41, colidx=ci)
    host = api.Tile_create(m, n, nnz, rp, ci, vals, dtype=dtype, hyb=True)
    dev = api.Tile_create_device(m, n, nnz, rp, ci, vals, dtype=dtype, hyb=True)
    h, d = to_dict(host, m), to_dict(dev, m)
    assert int(np.count_nonzero(d["Format"] == 3)) == hyb_tiles and len(d["hybIdx"]) == idx_bytes
    assert [k for k in h if (h[k].tobytes() != d[k].tobytes() if isinstance(h[k], np.ndarray) else h[k] != d[k])] == []
    api.Tile_destroy(dev)
    want = golden(m, rp, ci, vals, x)
    xd = torch.from_numpy(x).cuda()
    for plan in (api.Plan(host, m, n, nnz, deterministic=1), api.Plan.from_csr(m, n, nnz, rp, ci, vals, dtype=dtype, hyb=True, deterministic=1)):
        yd = torch.full((32,), -7.5e30, dtype=xd.dtype, device="cuda")
        plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        assert np.array_equal(y[:m], want), (name, plan.info()["device_build"], int(np.count_nonzero(y[:m] != want)))
        assert (y[16:] == np.asarray(-7.5e30, dtype=dtype)).all()
        plan.close()
    api.Tile_destroy(host)
