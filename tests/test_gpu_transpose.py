"""Transposed products on the MI355X (TILESPMV_CREATE_TRANSPOSE, tilespmv_csr_transpose_device, SparseOperator, cgls).

The contract: the device transposer writes what the host one writes, bit for bit; a plan (or tiled matrix) created with the flag from A's CSR is the plan (tiled matrix) created
without it from A^T's CSR — same stream digests, same facts; its value map indexes A's value array."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
from test_gpu_update_values import FACTS, KNOBS, _close_to_csr  # noqa: E402
from test_transpose_cpu import _same_tiles  # noqa: E402
from tilespmv_amd import api, generators as G  # noqa: E402
from tilespmv_amd.operator import SparseOperator, cgls  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spmv(torch, plan, x):
    m, n = plan.shape
    assert len(x) == n
    xd = _dev(torch, x)
    yd = torch.full((m + 16,), SENTINEL, dtype=xd.dtype, device="cuda")
    plan.spmv(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _at_product(rows, cols, rp, ci, v, u):
    """A^T u and |A|^T |u| in fp64 (scipy)."""
    import scipy.sparse as sp
    lo, hi = int(rp[0]), int(rp[rows])
    rpz = np.asarray(rp[:rows + 1], np.int64) - lo
    A = sp.csr_matrix((np.asarray(v[lo:hi], np.float64), np.asarray(ci[lo:hi]), rpz), shape=(rows, cols))
    absA = sp.csr_matrix((np.abs(np.asarray(v[lo:hi], np.float64)), np.asarray(ci[lo:hi]), rpz), shape=(rows, cols))
    return A.T @ np.asarray(u, np.float64), absA.T @ np.abs(np.asarray(u, np.float64))


def _matrices():
    mats = [(n, (cases.SMALL.get(n) or cases.MEDIUM[n])()) for n in sorted(cases.SMALL) + sorted(cases.MEDIUM)]
    mats += [("tall", G.random_uniform(3000, 197, 0.03, 1)), ("wide", G.random_uniform(83, 5011, 0.02, 2)),
             ("holes", G.from_coo(200, 300, [0, 5, 5, 199], [299, 0, 17, 150])), ("empty", (50, 70, np.zeros(51, np.int32), np.zeros(0, np.int32)))]
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 12, 700)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    mats.append(("dups_unsorted", (700, 333, rp, (rng.integers(0, 40, int(rp[-1])) * 8 % 333).astype(np.int32))))
    return mats


def test_device_transposer_equals_the_host_one(torch_cuda):
    torch = torch_cuda
    for i, (name, (rows, cols, rp, ci)) in enumerate(_matrices()):
        dtype = np.float64 if i % 2 == 0 else np.float32
        blocks = [(0, rows)] + ([(rows // 5, rows - rows // 7)] if rows >= 20 else [])   # whole matrix, and a row block (rp[0] != 0)
        for r0, r1 in blocks:
            brp = np.ascontiguousarray(rp[r0:r1 + 1], np.int32)
            nr = r1 - r0
            v = G.real_values(max(int(rp[rows]), 1), dtype)
            want = api.csr_transpose(nr, cols, brp, ci, v[:int(rp[rows])], dtype=dtype)
            nnz = len(want[1])
            drp, dci, dv = _dev(torch, brp), _dev(torch, np.asarray(ci, np.int32) if len(ci) else np.zeros(1, np.int32)), _dev(torch, v)
            drpT = torch.full((cols + 1,), -7, dtype=torch.int32, device="cuda")
            dciT = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
            dsrcT = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
            dvT = torch.full((nnz + 1,), -7, dtype=dv.dtype, device="cuda")
            api.csr_transpose_device(nr, cols, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), drpT.data_ptr(), dciT.data_ptr(), dvT.data_ptr(), dsrcT.data_ptr(), dtype=dtype)
            got = [drpT.cpu().numpy(), dciT.cpu().numpy(), dvT.cpu().numpy(), dsrcT.cpu().numpy()]
            for k, (g, w) in enumerate(zip(got, want)):
                assert g[:len(w)].tobytes() == w.tobytes(), (name, r0, r1, k)
            assert got[1][nnz] == -7 and got[3][nnz] == -7   # nothing written past the end
            # no values, no positions
            dciT2 = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
            api.csr_transpose_device(nr, cols, drp.data_ptr(), dci.data_ptr(), 0, drpT.data_ptr(), dciT2.data_ptr(), dtype=dtype)
            assert dciT2.cpu().numpy()[:nnz].tobytes() == want[1].tobytes()


def test_device_transposer_refuses_bad_columns(torch_cuda):
    torch = torch_cuda
    rp, ci = np.array([0, 2, 3], np.int32), np.array([0, 9, 1], np.int32)
    d = [_dev(torch, a) for a in (rp, ci)]
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        api.csr_transpose_device(2, 4, d[0].data_ptr(), d[1].data_ptr(), 0, out.data_ptr(), out.data_ptr(), dtype=np.float64)


def test_tile_create_device_transpose_equals_the_host_one(torch_cuda):
    for i, (name, (rows, cols, rp, ci)) in enumerate(_matrices()):
        dtype = np.float64 if i % 2 == 0 else np.float32
        nnz = int(rp[rows])
        v = G.real_values(nnz, dtype)
        for kw in (dict(), dict(hyb=True), dict(cdna4=True)) if i % 3 == 0 else (dict(),):
            host = api.Tile_create(rows, cols, nnz, rp, ci, v, dtype=dtype, transpose=True, **kw)
            dev = api.Tile_create_device(rows, cols, nnz, rp, ci, v, dtype=dtype, transpose=True, **kw)
            try:
                assert _same_tiles(host, dev, cols) == [], (name, kw)
            finally:
                api.Tile_destroy(host); api.Tile_destroy(dev)


def flag_equals_pretransposed(torch, rows, cols, rp, ci, dtype, knobs, v, shard=None, cdna4=False, hyb=False):
    """Plan with the flag from A == plan without it from A^T (digests, facts); y = A^T u within the CSR tolerance; rows of y outside the shard keep their sentinel."""
    nnz = int(rp[rows])
    kw = dict(knobs)
    kw.setdefault("placement_tries", 1)
    if shard:
        kw["tilerow_begin"], kw["tilerow_end"] = shard
    rpT, ciT, vT, _ = api.csr_transpose(rows, cols, rp, ci, v)
    a = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, cdna4=cdna4, hyb=hyb, transpose=True, **kw)
    b = api.Plan.from_csr(cols, rows, nnz, rpT, ciT, vT, dtype=dtype, cdna4=cdna4, hyb=hyb, **kw)
    try:
        assert a.shape == b.shape == (cols, rows)
        ai, bi = a.info(), b.info()
        assert shard or ai["rows"] == cols   # (a shard's fact counts its own rows)
        bad = [(k, ai[k], bi[k]) for k in FACTS if ai[k] != bi[k]]
        assert bad == [], bad
        assert a.stream_digests() == b.stream_digests()
        u = G.real_x(rows, nnz, dtype)
        y = _spmv(torch, a, u)
        r0, r1 = (shard[0] * 16, min(cols, shard[1] * 16)) if shard else (0, cols)
        want, scale = _at_product(rows, cols, rp, ci, v, u)
        assert _close_to_csr(y[r0:r1], want[r0:r1], scale[r0:r1], dtype).all()
        assert (y[:r0] == SENTINEL).all() and (y[r1:] == SENTINEL).all()
        if ai["entry_ordered"]:
            assert np.array_equal(y, _spmv(torch, b, u))
        return ai
    finally:
        a.close(); b.close()


def test_plan_contract_on_the_cases(torch_cuda):
    for i, (name, (rows, cols, rp, ci)) in enumerate(_matrices()):
        nnz = int(rp[rows])
        if nnz == 0:
            continue
        for j in range(2):
            knobs = KNOBS[(3 * i + 5 * j) % len(KNOBS)]
            dtype = np.float64 if (i + j) % 2 == 0 else np.float32
            tilem_T = (cols + 15) // 16
            shard = (tilem_T // 4, max(tilem_T // 4 + 1, 3 * tilem_T // 4)) if j == 1 and tilem_T >= 4 else None
            flag_equals_pretransposed(torch_cuda, rows, cols, rp, ci, dtype, knobs, G.real_values(nnz, dtype), shard=shard, hyb=(i + j) % 4 == 1, cdna4=(i + j) % 5 == 2)


def test_plan_contract_across_forms(torch_cuda):
    """Every knob set of the value-map tests on nonsymmetric matrices (power-law, R-MAT, circuit, KKT, a wide and a tall rectangular one), fp64 and fp32, whole and sharded."""
    mats = {"powerlaw": G.powerlaw(300000), "rmat16": G.rmat(16, 8, 3), "circuit": G.circuit_like(120000), "kkt24": G.kkt_like(24),
            "wide": G.random_uniform(4000, 90001, 0.0004, 8), "tall": G.random_uniform(200000, 7001, 0.0005, 14)}
    seen = set()
    for m, (name, (rows, cols, rp, ci)) in enumerate(mats.items()):
        nnz = int(rp[rows])
        tilem_T = (cols + 15) // 16
        for k, knobs in enumerate(KNOBS):
            dtype = np.float64 if (k + m) % 2 == 0 else np.float32
            shard = (tilem_T // 3, 2 * tilem_T // 3) if (k // 2 + m) % 2 else None
            info = flag_equals_pretransposed(torch_cuda, rows, cols, rp, ci, dtype, knobs, G.real_values(nnz, dtype), shard=shard, cdna4=(k + m) % 7 == 3, hyb=(k + m) % 5 == 1)
            seen.add(("csr_form", info["csr_form"])); seen.add(("entry_mode", info["entry_mode"])); seen.add(("split", info["num_split_rows"] > 0))
    for want in [("entry_mode", 0), ("entry_mode", 1), ("entry_mode", 2), ("split", True)]:
        assert want in seen, (want, sorted(seen))


def test_symmetric_laplacian_transposed_plan_is_the_plan(torch_cuda):
    rows, cols, rp, ci = G.laplacian5pt(300)
    rows = cases.truncated_rows(rows)
    nnz = int(rp[rows])
    r = np.repeat(np.arange(rows), np.diff(rp[:rows + 1]))
    c = np.asarray(ci[:nnz], np.int64)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    for dtype in (np.float64, np.float32):
        v = (np.sin(lo * 0.37 + hi * 1.11) + 2.5 * (lo == hi)).astype(dtype)   # symmetric: a function of the unordered pair
        for knobs in (dict(), dict(csr_split=2, entry_mode=2), dict(deterministic=1)):
            p = api.Plan.from_csr(rows, rows, nnz, rp[:rows + 1], ci[:nnz], v, dtype=dtype, placement_tries=1, **knobs)
            t = api.Plan.from_csr(rows, rows, nnz, rp[:rows + 1], ci[:nnz], v, dtype=dtype, placement_tries=1, transpose=True, **knobs)
            try:
                assert p.stream_digests() == t.stream_digests()
                x = G.real_x(rows, nnz, dtype)
                assert np.array_equal(_spmv(torch_cuda, p, x), _spmv(torch_cuda, t, x))
            finally:
                p.close(); t.close()


def test_value_map_indexes_the_values_of_a(torch_cuda):
    torch = torch_cuda
    mats = [cases.SMALL["allfmt_pad5"](), cases.SMALL["rand500x700"](), G.powerlaw(100000), G.random_uniform(3000, 197, 0.03, 1), cases.MEDIUM["kkt12"]()]
    for i, (rows, cols, rp, ci) in enumerate(mats):
        nnz = int(rp[rows])
        for j, knobs in enumerate((dict(), dict(csr_split=1, absorb=2), dict(entry_mode=2, csr_split=2), dict(deterministic=1))):
            dtype = np.float64 if (i + j) % 2 == 0 else np.float32
            v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
            a = api.Plan.from_csr(rows, cols, nnz, rp, ci, v1, dtype=dtype, value_map=True, transpose=True, placement_tries=1, **knobs)
            b = api.Plan.from_csr(rows, cols, nnz, rp, ci, v2, dtype=dtype, value_map=True, transpose=True, placement_tries=1, **knobs)
            try:
                dv2 = _dev(torch, v2)
                a.update_values(dv2.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                ai, bi = a.info(), b.info()
                assert ai["value_map_bytes"] > 0
                assert [(k, ai[k], bi[k]) for k in FACTS if ai[k] != bi[k]] == []
                assert a.stream_digests() == b.stream_digests()
                u = G.real_x(rows, nnz, dtype)
                ya, yb = _spmv(torch, a, u), _spmv(torch, b, u)
                if ai["entry_ordered"]:
                    assert np.array_equal(ya, yb)
                want, scale = _at_product(rows, cols, rp, ci, v2, u)
                assert _close_to_csr(ya[:cols], want, scale, dtype).all()
            finally:
                a.close(); b.close()
    # a row block of a larger CSR (rp[0] != 0): the map names positions of the caller's whole value array
    rows, cols, rp, ci = G.random_uniform(2000, 900, 0.01, 9)
    nnz = int(rp[rows])
    v1, v2 = G.real_values(nnz), G.real_values(nnz, first=nnz)
    r0, r1 = 320, 1440
    brp = rp[r0:r1 + 1]
    a = api.Plan.from_csr(r1 - r0, cols, int(brp[-1] - brp[0]), brp, ci, v1, value_map=True, transpose=True, placement_tries=1)
    dv2 = _dev(torch, v2)
    a.update_values(dv2.data_ptr())
    u = G.real_x(r1 - r0, nnz, np.float64)
    want, scale = _at_product(r1 - r0, cols, brp, ci, v2, u)
    assert _close_to_csr(_spmv(torch, a, u)[:cols], want, scale, np.float64).all()
    a.close()


def test_operator_refreshes_both_plans_and_captures(torch_cuda):
    torch = torch_cuda
    rows, cols, rp, ci = G.random_uniform(5000, 1700, 0.004, 10)
    nnz = int(rp[rows])
    for dtype in (np.float64, np.float32):
        v1, v2 = G.real_values(nnz, dtype), G.real_values(nnz, dtype, first=nnz)
        op = SparseOperator(rows, cols, rp, ci, v1, value_map=True, placement_tries=1, deterministic=1)
        ref = SparseOperator(rows, cols, rp, ci, v2, value_map=True, placement_tries=1, deterministic=1)
        dv2 = _dev(torch, v2)
        x, u = _dev(torch, G.real_x(cols, nnz, dtype)), _dev(torch, G.real_x(rows, nnz, dtype))
        y, z = torch.empty(rows + 16, dtype=x.dtype, device="cuda"), torch.empty(cols + 16, dtype=x.dtype, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):   # warm-up outside the capture
            op.update_values(dv2); op.matvec(x, y[:rows]); op.rmatvec(u, z[:cols])
        s.synchronize()
        op.update_values(_dev(torch, v1))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            op.update_values(dv2)
            op.matvec(x, y[:rows])
            op.rmatvec(u, z[:cols])
        g.replay()
        torch.cuda.synchronize()
        assert op.A.stream_digests() == ref.A.stream_digests() and op.AT.stream_digests() == ref.AT.stream_digests()
        assert torch.equal(y[:rows], ref.matvec(x)) and torch.equal(z[:cols], ref.rmatvec(u))
        op.close(); ref.close()


def test_spmm_on_a_transposed_plan(torch_cuda):
    torch = torch_cuda
    rows, cols, rp, ci = G.random_uniform(3000, 1100, 0.005, 11)
    nnz = int(rp[rows])
    for dtype in (np.float64, np.float32):
        op = SparseOperator(rows, cols, rp, ci, G.real_values(nnz, dtype), placement_tries=1, deterministic=1)
        for nvec in (2, 4, 8):
            U = torch.from_numpy(np.random.default_rng(nvec).uniform(-1, 1, (rows, nvec)).astype(dtype)).cuda()
            V = op.rspmm(U)
            torch.cuda.synchronize()
            for k in range(nvec):
                col = op.rmatvec(U[:, k].contiguous())
                torch.cuda.synchronize()
                if dtype == np.float64:
                    assert torch.allclose(V[:, k], col, rtol=1e-12, atol=1e-12)
                else:
                    assert torch.allclose(V[:, k], col, rtol=1e-5, atol=1e-5)
            Y = op.spmm(torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (cols, nvec)).astype(dtype)).cuda())
            assert Y.shape == (rows, nvec)
        op.close()


def test_from_device_csr_with_a_torch_csr_tensor(torch_cuda):
    torch = torch_cuda
    rows, cols, rp, ci = G.random_uniform(4000, 2500, 0.003, 12)
    nnz = int(rp[rows])
    v = G.real_values(nnz)
    t = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v), size=(rows, cols)).cuda()
    crow, col, vals = t.crow_indices().to(torch.int32), t.col_indices().to(torch.int32), t.values()
    p = api.Plan.from_device_csr(rows, cols, nnz, crow.data_ptr(), col.data_ptr(), vals.data_ptr(), np.float64, transpose=True, placement_tries=1)
    q = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, transpose=True, placement_tries=1)
    assert p.shape == (cols, rows) and p.stream_digests() == q.stream_digests()
    u = G.real_x(rows, nnz, np.float64)
    y = _spmv(torch, p, u)
    want, scale = _at_product(rows, cols, rp, ci, v, u)
    assert _close_to_csr(y[:cols], want, scale, np.float64).all() and (y[cols:] == SENTINEL).all()
    p.close(); q.close()
    op = SparseOperator(rows, cols, crow, col, vals)   # device CSR through the operator
    assert torch.allclose(op.rmatvec(_dev(torch, u)).cpu(), torch.from_numpy(y[:cols]), rtol=1e-12, atol=1e-12)
    op.close()


@pytest.mark.parametrize("workload", ["laplacian4096", "powerlaw8m"])
def test_full_size(torch_cuda, workload):
    """Config 4 (symmetric pattern, fp64) and the power-law 8 M (nonsymmetric, >= 10 M nonzeros, fp64): A^T u against scipy over the whole of y."""
    torch = torch_cuda
    if workload == "laplacian4096":
        rows, cols, rp, ci = G.laplacian5pt(4096)
    else:
        rows, cols, rp, ci = G.powerlaw(8000000, seed=2)
    nnz = int(rp[rows])
    assert nnz >= 10_000_000
    v = G.real_values(nnz)
    p = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, transpose=True, placement_tries=1)
    u = G.real_x(rows, nnz, np.float64)
    y = _spmv(torch, p, u)
    p.close()
    want, scale = _at_product(rows, cols, rp, ci, v, u)
    ok = _close_to_csr(y[:cols], want, scale, np.float64)
    assert ok.all(), (int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
    assert (y[cols:] == SENTINEL).all()


def test_cgls_reaches_the_least_squares_solution(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(13)
    rows, cols = 4000, 300
    r, c = np.repeat(np.arange(rows), 6), rng.integers(0, cols, rows * 6)
    r = np.concatenate([r, np.arange(cols)]); c = np.concatenate([c, np.arange(cols)])   # every column held
    _, _, rp, ci = G.from_coo(rows, cols, r, c)
    nnz = int(rp[rows])
    v = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    dense = np.zeros((rows, cols)); np.add.at(dense, (np.repeat(np.arange(rows), np.diff(rp)), ci), v)
    assert np.linalg.cond(dense) < 100
    b = rng.standard_normal(rows)
    want = np.linalg.lstsq(dense, b, rcond=None)[0]
    op = SparseOperator(rows, cols, rp, ci, v, placement_tries=1)
    x, info = cgls(op, _dev(torch, b), tol=1e-13, maxiter=500)
    op.close()
    assert info["converged"], info
    got = x.cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-8 * np.linalg.norm(want), (np.linalg.norm(got - want), info)
