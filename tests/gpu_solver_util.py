"""What the GPU tests of the device-resident solvers share (tests/test_gpu_{cg,cg_multi,cgls,bicgstab,minres,gmres,block_jacobi,solver_sizes,solver_driver}.py, tests/solver_contract.py):
the fixture that hands out torch, the value types and the project's tolerances, plans and operators with deterministic=1 and placement_tries=1, and device vectors with sixteen
sentinel elements behind them.  A plain module beside tests/solver_sizes.py, imported the same way; the fixture is taken with ``from gpu_solver_util import torch_cuda``."""
import numpy as np
import pytest

from tilespmv_amd import api
from tilespmv_amd.operator import SparseOperator

DTYPES = [np.float64, np.float32]
PRODUCT_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}   # README: the project's per-product tolerance on real-valued data
SENTINEL = 777.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _deterministic(kw):
    kw.setdefault("deterministic", 1)
    kw.setdefault("placement_tries", 1)
    return kw


def square_plan(n, rp, ci, v, dtype, **kw):
    """A plan of an n x n matrix through Plan.from_csr."""
    return api.Plan.from_csr(n, n, len(ci), rp, ci, np.ascontiguousarray(v, dtype=dtype), dtype=dtype, **_deterministic(kw))


def rect_op(rows, cols, rp, ci, v, dtype, **kw):
    """A SparseOperator of a rows x cols matrix: the plans of A and of A^T."""
    return SparseOperator(rows, cols, rp, ci, np.ascontiguousarray(v, dtype=dtype), dtype=dtype, **_deterministic(kw))


def square_op(n, rp, ci, v, dtype, **kw):
    return rect_op(n, n, rp, ci, v, dtype, **kw)


def tdt(torch, dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def vec(torch, a, n, dtype, nvec=None):
    """A device vector of n elements (with nvec: a row-major (n, nvec) array) with 16 sentinel elements (rows) behind it: the whole tensor.  a = None: zeros."""
    t = torch.full((n + 16,) if nvec is None else (n + 16, nvec), SENTINEL, dtype=tdt(torch, dtype), device="cuda")
    if a is None:
        t[:n].zero_()
    else:
        a = np.ascontiguousarray(a, dtype=dtype)
        t[:n].copy_(torch.from_numpy(a if nvec is None else a.reshape(n, nvec)))
    return t


def host(t, n):
    return t.cpu().numpy()[:n].copy()


def intact(*tensors_and_lengths):
    for t, n in tensors_and_lengths:
        assert (t.cpu().numpy()[n:] == SENTINEL).all(), "a sentinel behind a caller vector was overwritten"


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def device_csr(torch, rp, ci, v):
    return torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()


def transpose_pattern(torch, rows, cols, rpd, cid, dt):
    """rpT and srcT of the pattern, by tilespmv_csr_transpose_device (no values gathered): what a caller keeps for the column scaling."""
    nnz = cid.numel()
    rpT = torch.zeros(cols + 1, dtype=torch.int32, device="cuda")
    ciT = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    srcT = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    api.csr_transpose_device(rows, cols, rpd.data_ptr(), cid.data_ptr(), None, rpT.data_ptr(), ciT.data_ptr(), None, srcT.data_ptr(), dtype=dt, stream=stream(torch))
    return rpT, srcT


def relerr(x, xs):
    xs = np.asarray(xs, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(x, dtype=np.float64) - xs) / np.linalg.norm(xs))


def dist(a, b):
    """|a - b| / |b|; against b = 0 the absolute |a|, so that an exact zero is held to the same bound."""
    return abs(a - b) / abs(b) if b != 0 else abs(a)
