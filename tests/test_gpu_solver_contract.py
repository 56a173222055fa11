"""The promises of tests/solver_contract.py that run for every row of its table SOLVERS, over both value types: graph capture, and nothing touched past the end.  A solver added
to the table is tested here without another line.  (Fixed order, value refresh and the refusals of create are still called from tests/test_gpu_{cg,cgls,bicgstab,minres,gmres}.py.)"""
import numpy as np
import pytest

import gmres_mirror
import gpu_solver_util as U
import solver_contract as K
import test_gpu_bicgstab
import test_gpu_gmres
from gpu_solver_util import DTYPES, torch_cuda  # noqa: F401
from tilespmv_amd import api

pytestmark = pytest.mark.gpu

EVERY_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)


def _bicgstab_early(torch, dt, op, A, b, dinv, dims, label):
    """One and three Jacobi iterations against the mirror: the ``_early`` of tests/test_gpu_bicgstab.py, which closes its solver."""
    return test_gpu_bicgstab._early(torch, dt, A, b, op.A, dinv, dims[0], label) + (None,)


def _gmres_early(torch, dt, op, A, b, dinv, dims, label):
    """Three and five iterations of restart 8 and a flush against the mirror: the ``_early`` of tests/test_gpu_gmres.py, which closes its solver."""
    dd = U.vec(torch, dinv, dims[0], dt)
    return test_gpu_gmres._early(torch, dt, gmres_mirror.Mirror(A, dt, 8, dinv), b, lambda: api.GMRES(op.A, 8, dd.data_ptr()), dims[0], label) + (dd, None)


EARLY = {"bicgstab": _bicgstab_early, "gmres": _gmres_early}      # where the table has ``past_early=None``: these two helpers stay with the other tests that use them


@EVERY_DTYPE
@pytest.mark.parametrize("name", list(K.SOLVERS))
def test_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, name, dtype):
    K.begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, name, dtype)


PAST = [pytest.param(name, case, id="%s-%s" % (name, case["id"])) for name, spec in K.SOLVERS.items() for case in spec.past or ()]      # (``past=None``: MINRES has none)


@EVERY_DTYPE
@pytest.mark.parametrize("name,case", PAST)
def test_nothing_is_touched_past_the_end(torch_cuda, name, case, dtype):
    K.nothing_is_touched_past_the_end(torch_cuda, name, dtype, early=EARLY.get(name), **{k: v for k, v in case.items() if k != "id"})
