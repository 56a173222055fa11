"""The FSAI preconditioner without a GPU (tilespmv_fsai_*, tilespmv_cg_create_fsai; include/tilespmv.h): the facts of its numpy mirror (tests/fsai_mirror.py) that
the GPU tests lean on, the iteration counts the mirror gives beside the point-Jacobi and block-Jacobi mirrors, and the interface: the exports of both libraries, api.FSAI, and the
fsai argument of api.CG."""
import inspect
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

import block_jacobi_mirror as BJM
import cg_mirror as CM
import fsai_mirror as M
from kernel_asm import device_asm, private_segments
from tilespmv_amd import _lib, api

DTYPES = [np.float64, np.float32]
INPUTS = ["lap55", "femblk10", "band70", "lap55_neg", "band12", "band25"]
FSAI_SYMBOLS = ["tilespmv_fsai_create", "tilespmv_fsai_destroy", "tilespmv_fsai_update", "tilespmv_fsai_apply", "tilespmv_fsai_apply_dot", "tilespmv_fsai_factor_csr",
                "tilespmv_fsai_info", "tilespmv_cg_create_fsai"]


# ---- the interface (fails before the feature)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_libraries_export_the_fsai_entry_points(dtype):
    lib = _lib.load(dtype)
    for name in FSAI_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.DECLARED_SYMBOLS
    assert len(_lib.FSAI_INFO_NAMES) == 7


def test_the_python_interface():
    assert issubclass(api.FSAI, api._Solver)
    for method in ("update", "apply", "factor", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(api.FSAI, method)), method
    assert "d_partials" in inspect.signature(api.FSAI.apply).parameters
    params = inspect.signature(api.CG.__init__).parameters
    assert list(params)[:5] == ["self", "plan", "d_dinv", "block", "fsai"] and params["fsai"].default is None


def test_no_fsai_kernel_uses_scratch(tmp_path):
    """The device assembly of hip_fsai.hip in both value types: the count, fill and dot kernels and the five forms of the value kernel, none with a private segment."""
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_fsai.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        segments = private_segments(s)
        assert len(segments) == 8 and sum("k_fsai_values" in k for k in segments) == 5, (dt, list(segments))
        assert not any(segments.values()), (dt, segments)


# ---- the mirror
@pytest.mark.parametrize("name", INPUTS)
def test_the_pattern_is_the_stated_one(name):
    n, rp, ci, v = M.problem(name)
    gp, gci, src, truncated = M.pattern(n, rp, ci)
    for i in range(n):                                       # (the definition, row by row)
        lower = [c for c in ci[rp[i]:rp[i + 1]] if c <= i]
        want = lower[-M.MAX_ROW:]
        assert list(gci[gp[i]:gp[i + 1]]) == want and want[-1] == i
    assert np.array_equal(ci[src], gci)
    assert truncated == (136 if name == "band70" else 0)
    longest = int(np.diff(gp).max())
    assert longest == {"lap55": 3, "lap55_neg": 3, "femblk10": 42, "band70": 64, "band12": 13, "band25": 26}[name]
    if name == "band70":
        lens = np.diff(gp)
        lower = np.array([(ci[rp[i]:rp[i + 1]] <= i).sum() for i in range(n)])
        assert lower[63] == 64 and lens[63] == 64 and (lower[64:] >= 65).all() and (lower[64:] <= 71).all() and (lens[64:] == 64).all()
        assert gci[gp[199]] == 199 - 63                      # (the 64 columns nearest the diagonal)


@pytest.mark.parametrize("name", INPUTS)
def test_g_a_gt_has_a_unit_diagonal(name):
    """diag(G A G^T) = 1 within 1e-12 on the rows that did not fall back (float64 G; A = the symmetric matrix of the input's lower triangle)."""
    n, rp, ci, v = M.problem(name)
    gp, gci, g, fell, truncated, _ = M.factor64(n, rp, ci, v)
    L = sp.tril(M.scipy_csr(n, rp, ci, v), format="csr")
    A = (L + sp.tril(L, -1).T).tocsr()
    G = M.g_csr(n, gp, gci, g)
    d = np.asarray((G @ A).multiply(G).sum(axis=1)).ravel()
    worst = float(np.abs(d[~fell] - 1.0).max())
    print("%s: largest |diag(G A G^T) - 1| = %.3g over %d rows, %d fell back" % (name, worst, int((~fell).sum()), int(fell.sum())))
    assert worst <= 1e-12
    assert (g[gp[1:] - 1] > 0).all()                         # (a positive diagonal: G is nonsingular, G^T G positive definite)
    if name == "lap55_neg":
        assert tuple(np.flatnonzero(fell)) == M.NEG_ROWS and int(fell.sum()) == 3
        for i in M.NEG_ROWS:
            row = g[gp[i]:gp[i + 1]]
            assert not row[:-1].any() and row[-1] == (1.0 if i == 100 else 0.5)
    else:
        assert not fell.any()


def test_the_fallback_rows_of_lap55_neg_hold_column_100():
    n, rp, ci, v = M.problem("lap55_neg")
    gp, gci, _, _ = M.pattern(n, rp, ci)
    assert tuple(i for i in range(n) if 100 in gci[gp[i]:gp[i + 1]]) == M.NEG_ROWS


def test_the_mirror_scales_to_the_capped_tridiagonal():
    """tri_capped (about a million rows) is factored by the stacked path.  Every row of G of (-1, 2, -1) but the first has the local matrix [[2, -1], [-1, 2]]:
    y = (1, 2) / 3, g = y / sqrt(2 / 3); the first row is 1 / sqrt(2)."""
    dt = np.dtype(np.float64)
    n, rp, ci, v = M.tri_capped(dt)
    gp, gci, g, fallback, truncated = M.factor(n, rp, ci, v, dt)
    assert fallback == 0 and truncated == 0 and gp[-1] == 2 * n - 1
    assert np.allclose(g[0], 0.5 ** 0.5, rtol=1e-14, atol=0)
    assert np.allclose(g[1::2], (1.0 / 3.0) / (2.0 / 3.0) ** 0.5, rtol=1e-14, atol=0) and np.allclose(g[2::2], (2.0 / 3.0) ** 0.5, rtol=1e-14, atol=0)


# ---- iteration counts
_COUNTS = {}


def _counts(name, dtype):
    """CG iterations to RTOL at check_every = 1 of the mirrors: {"jacobi", "block3" (femblk10 only), "fsai"}."""
    dt = np.dtype(dtype)
    if (name, dt) not in _COUNTS:
        n, rp, ci, v = M.problem(name)
        vt, b = v.astype(dt), M.rhs(n).astype(dt)
        A = M.scipy_csr(n, rp, ci, vt)
        f = M.factored(name, dt)
        solvers = {"jacobi": CM.Mirror(A, dt, BJM.inverse_diagonal(n, rp, ci, vt, dt)), "fsai": M.CG(A, dt, M.g_csr(n, f["gp"], f["gci"], f["g"]))}
        if name == "femblk10":
            solvers["block3"] = BJM.CG(A, dt, BJM.update(n, rp, ci, vt, 3, dt)[0])
        out = {}
        for k, s in solvers.items():
            x, it, status, rel = s.solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
            assert status == M.CONVERGED, (name, dt, k)
            out[k] = it
        _COUNTS[(name, dt)] = out
    return _COUNTS[(name, dt)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["femblk10", "lap55"])
def test_fsai_takes_fewer_iterations_than_the_jacobi_mirrors(name, dtype):
    c = _counts(name, dtype)
    print("%s %s: CG iterations to rtol %g: %s" % (name, np.dtype(dtype), M.RTOL[np.dtype(dtype)], ", ".join("%s %d" % kv for kv in c.items())))
    assert c["fsai"] < c["jacobi"]
    if name == "femblk10":
        assert c["fsai"] < c["block3"]
