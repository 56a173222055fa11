"""The FSAI preconditioner on the GPU (tilespmv_fsai_*, tilespmv_cg_create_fsai; include/tilespmv.h) against its numpy mirror (tests/fsai_mirror.py, itself
checked by tests/test_fsai_cpu.py) and scipy's direct solutions.  Plans — the operators' and the two inside every object — are deterministic=1, placement_tries=1.  G is read
back through ``FSAI.factor()``."""
import ctypes as C

import numpy as np
import pytest

import cg_mirror as CM
import fsai_mirror as M
import gpu_solver_util as U
import solver_sizes as SS
from gpu_solver_util import DTYPES, PRODUCT_TOL, SENTINEL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api

pytestmark = pytest.mark.gpu

_CACHE = {}


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _fsai(torch, n, csr, dt):
    """An object from a device CSR (rp, ci, v tensors)."""
    return api.FSAI(n, csr[1].numel(), csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dt, stream=U.stream(torch), deterministic=1, placement_tries=1)


def _solved(name, dtype):
    """The FSAI mirror's solve of a named input and the direct solution, once per value type: (xs, mirror iterations, mirror error, G of the mirror as float64 CSR)."""
    dt = np.dtype(dtype)
    if (name, dt) not in _CACHE:
        n, rp, ci, vt, b = _system(name, dt)
        f = M.factored(name, dt)
        G64 = M.g_csr(n, f["gp"], f["gci"], f["g"])
        xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
        xm, itm, stm, relm = M.CG(M.scipy_csr(n, rp, ci, vt), dt, G64).solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[(name, dt)] = (xs, itm, U.relerr(xm, xs), G64)
    return _CACHE[(name, dt)]


# ---- 1. G
def _row_ratio(got, f, dt):
    """The largest |GPU - g64| / (16 m eps cond_2(S_i) max|g64_i|) over the rows that did not fall back."""
    gp, g64, worst = f["gp"], f["g64"], 0.0
    for m, (idx, S) in f["S"].items():
        keep = ~f["fell"][idx]
        if not keep.any():
            continue
        idx, S = idx[keep], S[keep]
        pos = gp[idx][:, None] + np.arange(m)[None, :]
        diff, big = np.abs(got[pos].astype(np.float64) - g64[pos]).max(axis=1), np.abs(g64[pos]).max(axis=1)
        worst = max(worst, float((diff / (16 * m * np.finfo(dt).eps * np.linalg.cond(S) * big)).max()))
    return worst


def _check_pattern_and_info(info, gp_g, gci_g, f, n, dt, fallback):
    assert gp_g.dtype == np.int32 and gci_g.dtype == np.int32
    assert np.array_equal(gp_g, f["gp"]) and np.array_equal(gci_g, f["gci"])
    want = M.info(n, f["gp"], fallback, f["truncated"])
    assert {k: info[k] for k in want} == want, (info, want)
    assert info["dot_partials"] == SS.parts(n, SS.vpl(dt))
    assert info["device_bytes"] > int(f["gp"][-1]) * (4 + dt.itemsize) + (2 * n + 1) * 4 + n * dt.itemsize      # (G's CSR, the pattern's start per row and t; then the two plans)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["lap55", "femblk10", "band70", "band12", "band25"])
def test_g_equals_the_mirror(torch_cuda, name, dtype):
    """Row pointer and columns exactly; per row |GPU - g64| <= 16 m eps cond_2(S_i) max|g64_i| — the bound of the block inverse's test with m in place of bs: the forward error of
    a Cholesky solve of an m x m system (the rounding of the row to the value type is inside it).  The arithmetic is double in both builds.  The longest rows, 3, 42, 64, 13
    and 26, take the value kernel through each of its forms (8, 48, 64, 16 and 32 lanes per row)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    f = M.factored(name, dt)
    with _fsai(torch, n, U.device_csr(torch, rp, ci, vt), dt) as fs:
        info = fs.info(U.stream(torch))
        gp_g, gci_g, g_g = fs.factor(U.stream(torch))
    _check_pattern_and_info(info, gp_g, gci_g, f, n, dt, 0)
    assert g_g.dtype == dt
    ratio = _row_ratio(g_g, f, dt)
    print("%s %s: longest row %d, %d truncated; largest |GPU - g64| / bound over the rows = %.3g" % (name, dt, info["longest_row"], info["truncated_rows"], ratio))
    assert ratio <= 1.0


# ---- 2. fallback rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_rows(torch_cuda, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("lap55_neg", dt)
    f = M.factored("lap55_neg", dt)
    assert int(f["fell"].sum()) == 3 and tuple(np.flatnonzero(f["fell"])) == M.NEG_ROWS
    good = M.problem("lap55")[3].astype(dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    goodd = torch.from_numpy(good).cuda()
    st = U.stream(torch)
    with _fsai(torch, n, (rpd, cid, vd), dt) as fs:
        info = fs.info(st)
        gp_g, gci_g, g_g = fs.factor(st)
        _check_pattern_and_info(info, gp_g, gci_g, f, n, dt, 3)
        for i in M.NEG_ROWS:                                     # (the Jacobi rows: a_100,100 = -1 -> 1, the others 1 / sqrt(4))
            row = g_g[gp_g[i]:gp_g[i + 1]]
            assert not row[:-1].any() and row[-1] == dt.type(1.0 if i == 100 else 0.5), (i, row)
            assert np.array_equal(row, f["g"][gp_g[i]:gp_g[i + 1]])
        ratio = _row_ratio(g_g, f, dt)
        print("lap55_neg %s: 3 fallback rows; largest |GPU - g64| / bound over the other rows = %.3g" % (dt, ratio))
        assert ratio <= 1.0
        # lap55's own values on the same pattern: the counter is rewritten, G has the bytes of a fresh object's
        fs.update(rpd.data_ptr(), cid.data_ptr(), goodd.data_ptr(), st)
        assert fs.info(st)["fallback_rows"] == 0
        g_u = fs.factor(st)[2]
    with _fsai(torch, n, (rpd, cid, goodd), dt) as fresh:
        assert fresh.info(st)["fallback_rows"] == 0
        g_f = fresh.factor(st)[2]
    assert g_u.tobytes() == g_f.tobytes() and not np.array_equal(g_u, g_g)


# ---- 3. apply
def _check_apply(torch, dt, n, fs, label):
    """apply and apply_dot on a random r against numpy with the GPU's own G; the sentinels behind z and the partials; r untouched."""
    gp_g, gci_g, g_g = fs.factor(U.stream(torch))
    r = np.random.default_rng(41).uniform(-1, 1, n).astype(dt)
    want = M.apply(M.g_csr(n, gp_g, gci_g, g_g), r, dt)
    bound = 100 * PRODUCT_TOL[dt]
    rd, zd, z2 = U.vec(torch, r, n, dt), U.vec(torch, None, n, dt), U.vec(torch, None, n, dt)
    parts = torch.full((1024 + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    fs.apply(rd.data_ptr(), zd.data_ptr(), U.stream(torch))
    fs.apply(rd.data_ptr(), z2.data_ptr(), U.stream(torch), d_partials=parts.data_ptr())
    torch.cuda.synchronize()
    z = U.host(zd, n)
    np_ = SS.parts(n, SS.vpl(dt))
    p = parts.cpu().numpy()
    dot = float(np.dot(r.astype(np.float64), want.astype(np.float64)))
    err, derr = U.relerr(z, want.astype(np.float64)), U.dist(float(p[:np_].sum()), dot)
    print("%s %s: |z - numpy| / |numpy| = %.3g, r.z from %d partials %.3g (bound %.3g)" % (label, dt, err, np_, derr, bound))
    assert err <= bound and derr <= bound
    assert np.array_equal(z, U.host(z2, n))
    U.intact((parts, np_), (zd, n), (z2, n), (rd, n))
    assert np.array_equal(U.host(rd, n), r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["lap55", "femblk10", "band70"])
def test_apply_equals_numpy(torch_cuda, name, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    with _fsai(torch, n, U.device_csr(torch, rp, ci, vt), dt) as fs:
        _check_apply(torch, dt, n, fs, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_past_the_partial_sum_cap(torch_cuda, dtype):
    """tri_capped: 1024 partials and a second sweep over the workgroups, the longest scalar tail.  Then one CG iteration on its plan against the mirror: k_cg_zstep folds the 1024
    partials in four passes."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, v = M.tri_capped(dt)
    vt = v.astype(dt)
    assert SS.walk(n, SS.vpl(dt)).parts == 1024 and SS.walk(n, SS.vpl(dt)).sweeps == 2
    gp, gci, g, fallback, truncated = M.factor(n, rp, ci, vt, dt)
    with _fsai(torch, n, U.device_csr(torch, rp, ci, vt), dt) as fs:
        assert fs.info(U.stream(torch))["dot_partials"] == 1024
        _check_apply(torch, dt, n, fs, "tri_capped")
        b = M.rhs(n).astype(dt)
        m = M.CG(M.scipy_csr(n, rp, ci, vt), dt, M.g_csr(n, gp, gci, g))
        m.begin(b); m.iterate(1)
        plan = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1)
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.CG(plan, fsai=fs) as cg:
            cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
            cg.iterate(xd.data_ptr(), 1, U.stream(torch))
            s = cg.state(U.stream(torch))
        plan.close()
        dx, drr = U.relerr(U.host(xd, n), m.x.astype(np.float64)), U.dist(s["rr"], m.rr)
        print("tri_capped %s: after 1 iteration |x - mirror| / |mirror| = %.3g, rr %.3g" % (dt, dx, drr))
        assert s["iterations"] == 1 and max(dx, drr, U.dist(s["bb"], m.bb)) <= 100 * PRODUCT_TOL[dt]


# ---- 4. CG
def _early(torch, dt, make_solver, mirror, b, n, label):
    """x and rr after 1 and after 3 iterations against the mirror, within 100 x the per-product tolerance (the bound of the solvers' own tests)."""
    mirror.begin(b)
    bound = 100 * PRODUCT_TOL[dt]
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with make_solver() as sv:
        sv.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
        s0 = sv.state(U.stream(torch))
        assert s0["iterations"] == 0 and s0["status"] == api.CG_RUNNING
        assert max(U.dist(s0["rr"], mirror.rr), U.dist(s0["bb"], mirror.bb)) <= bound
        done = 0
        for step in (1, 2):
            sv.iterate(xd.data_ptr(), step, U.stream(torch)); mirror.iterate(step); done += step
            s = sv.state(U.stream(torch))
            dx, drr = U.relerr(U.host(xd, n), mirror.x.astype(np.float64)), U.dist(s["rr"], mirror.rr)
            print("%s %s after %d iterations: |x - mirror| / |mirror| = %.3g, rr %.3g (bound %.3g)" % (label, dt, done, dx, drr, bound))
            assert s["iterations"] == done == mirror.iterations and s["status"] == api.CG_RUNNING == mirror.status()
            assert dx <= bound and drr <= bound
    U.intact((xd, n))
    assert np.array_equal(U.host(bd, n), b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_with_the_preconditioner(torch_cuda, dtype):
    """Early iterations equal the mirror; solve with maxiter = 2 x the mirror's count: CONVERGED, error against spsolve within 10 x the mirror's; the point-Jacobi solver on the
    same plan at that cap: MAXITER (its mirror needs 246 / 155 iterations against a cap of about 56 / 34)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system("femblk10", dt)
    xs, itm, errm, G64 = _solved("femblk10", dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op, _fsai(torch, n, csr, dt) as fs:
        _early(torch, dt, lambda: api.CG(op.A, fsai=fs), M.CG(M.scipy_csr(n, rp, ci, vt), dt, G64), b, n, "femblk10")
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.CG(op.A, fsai=fs) as sv:
            s = sv.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("femblk10 %s: FSAI %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        dinv = U.vec(torch, None, n, dt)
        api.csr_diagonal_device(n, csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
        xd[:n].zero_()
        with api.CG(op.A, dinv.data_ptr()) as sv:
            sp = sv.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        print("femblk10 %s: point Jacobi on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (dt, sp["iterations"], sp["status_name"], sp["relative_residual"]))
        assert sp["status"] == api.CG_MAXITER and sp["iterations"] == 2 * itm


def test_sparse_operator_takes_the_preconditioner(torch_cuda):
    torch = torch_cuda
    dt = np.dtype(np.float64)
    n, rp, ci, vt, b = _system("femblk10", dt)
    xs, itm, errm, G64 = _solved("femblk10", dt)
    bd = torch.from_numpy(b).cuda()
    with U.square_op(n, rp, ci, vt, dt) as op, _fsai(torch, n, U.device_csr(torch, rp, ci, vt), dt) as fs:
        x, info = op.cg(bd, rtol=M.RTOL[dt], maxiter=2 * itm, precond=fs)
        assert info["converged"] and info["iterations"] <= 2 * itm and U.relerr(x.cpu().numpy(), xs) <= 10 * errm
        with pytest.raises(ValueError):
            op.cg(torch.stack([bd, bd], dim=1).contiguous(), precond=fs)
        with pytest.raises(ValueError):
            op.cg(bd, dinv=torch.ones(n, dtype=bd.dtype, device="cuda"), precond=fs)


# ---- 5. value refresh
@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """A plan with a value map and an object made from spd_values on femblk10's pattern; update_values and fs.update from femblk10's values: G has the bytes of a fresh object's
    and the solve the bits of a fresh solver's."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, v2, b = _system("femblk10", dt)
    v1 = CM.spd_values(n, rp, ci).astype(dt)
    xs, itm, errm, G64 = _solved("femblk10", dt)
    rpd, cid, v1d = U.device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with U.square_op(n, rp, ci, v1, dt, value_map=True) as op, _fsai(torch, n, (rpd, cid, v1d), dt) as fs:
        with api.CG(op.A, fsai=fs) as cg:
            s1 = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
            assert s1["status"] == api.CG_CONVERGED
            g1 = fs.factor(stream)[2]
            op.update_values(v2d.data_ptr(), stream)
            fs.update(rpd.data_ptr(), cid.data_ptr(), v2d.data_ptr(), stream)
            xd[:n].zero_()
            s2 = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
            x2 = U.host(xd, n)
        g2 = fs.factor(stream)[2]
    with U.square_op(n, rp, ci, v2, dt, value_map=True) as fresh, _fsai(torch, n, (rpd, cid, v2d), dt) as ff:
        gf = ff.factor(stream)[2]
        xf = U.vec(torch, None, n, dt)
        with api.CG(fresh.A, fsai=ff) as cg:
            sf = cg.solve(bd.data_ptr(), xf.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
    print("%s: refreshed %d iterations, fresh %d; error vs spsolve %.3g" % (dt, s2["iterations"], sf["iterations"], U.relerr(x2, xs)))
    assert not np.array_equal(g1, g2) and g2.tobytes() == gf.tobytes()
    assert s2["status"] == api.CG_CONVERGED and sf["status"] == api.CG_CONVERGED
    assert s2["iterations"] == sf["iterations"] and s2["rr"] == sf["rr"] and np.array_equal(x2, U.host(xf, n))
    assert U.relerr(x2, xs) <= 10 * errm


# ---- 6. fixed order
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_factor_and_the_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two runs of create + 10 CG iterations on separately created objects and operators: bit-identical G, x and rr."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("femblk10", dt)
    bd = U.vec(torch, b, n, dt)
    results = []
    for _ in range(2):
        with U.square_op(n, rp, ci, vt, dt) as op, _fsai(torch, n, U.device_csr(torch, rp, ci, vt), dt) as fs:
            xd = U.vec(torch, None, n, dt)
            with api.CG(op.A, fsai=fs) as cg:
                cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
                cg.iterate(xd.data_ptr(), 10, U.stream(torch))
                s = cg.state(U.stream(torch))
            results.append((fs.factor(U.stream(torch))[2], U.host(xd, n), s))
    (ga, xa, sa), (gb, xb, sb) = results
    assert sa["iterations"] == 10 and sa["status"] == api.CG_RUNNING and xa.any()
    assert ga.tobytes() == gb.tobytes() and np.array_equal(xa, xb) and sa["rr"] == sb["rr"]


# ---- 7. hipGraph
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, dtype):
    """update + begin + iterate(5) captured with torch's graph API on a side stream (one linear chain, as the solvers' capture tests do) and replayed twice from the same x0: each
    replay equals the eager run bit for bit.  Between the replays G is overwritten through an update with another matrix's values: the replayed update restores it."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("femblk10", dt)
    x0 = (0.01 * M.rhs(n)[::-1]).astype(dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    other = torch.from_numpy(CM.spd_values(n, rp, ci).astype(dt)).cuda()
    with U.square_op(n, rp, ci, vt, dt) as op, _fsai(torch, n, (rpd, cid, vd), dt) as fs:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        cg = api.CG(op.A, fsai=fs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()

        def chain(st):
            fs.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st)
            cg.begin(bd.data_ptr(), xd.data_ptr(), st)
            cg.iterate(xd.data_ptr(), 5, st)

        with torch.cuda.stream(side):
            st = side.cuda_stream
            chain(st)                                             # (uncaptured: the comparison, and the warm-up)
            s5 = cg.state(st); x5 = U.host(xd, n)
            xd[:n].copy_(torch.from_numpy(x0))
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                chain(st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert np.array_equal(U.host(xd, n), x0)                   # (captured, not run)
        for _ in range(2):
            xd[:n].copy_(torch.from_numpy(x0))
            fs.update(rpd.data_ptr(), cid.data_ptr(), other.data_ptr(), U.stream(torch))
            torch.cuda.synchronize()
            graph.replay(); torch.cuda.synchronize()
            s = cg.state(U.stream(torch))
            assert np.array_equal(U.host(xd, n), x5) and not np.array_equal(x5, x0)
            assert s["iterations"] == 5 and s["rr"] == s5["rr"] and s["status"] == api.CG_RUNNING
        del graph
        cg.close()


# ---- 8. refusals
def _broken(rp, ci, v):
    """lap55 with one row's promise broken, by name: unsorted columns, a repeated entry, a missing diagonal (row 5 holds columns 4, 5, 6, 60; row 0 holds 0, 1, 55)."""
    out = {}
    c, w = ci.copy(), v.copy()
    c[rp[5]], c[rp[5] + 1] = ci[rp[5] + 1], ci[rp[5]]
    w[rp[5]], w[rp[5] + 1] = v[rp[5] + 1], v[rp[5]]
    out["unsorted columns"] = (c, w)
    c = ci.copy()
    c[rp[6] - 1] = c[rp[6] - 2]
    out["a repeated entry"] = (c, v)
    c = ci.copy()
    c[rp[0]], c[rp[0] + 1] = 1, 2
    out["a missing diagonal"] = (c, v)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(torch_cuda, dtype):
    """A CSR that breaks the input's promise, mismatched rows, fsai together with d_dinv or block, misaligned, aliased or NULL vectors: hipErrorInvalidValue, no handle, nothing
    launched; the wrappers raise ValueError."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    st = U.stream(torch)
    n, rp, ci, vt, b = _system("lap55", dt)
    assert list(ci[rp[5]:rp[6]]) == [4, 5, 6, 60] and list(ci[rp[0]:rp[1]]) == [0, 1, 55]
    for what, (c, w) in _broken(rp, ci, vt).items():
        rpd, cid, vd = U.device_csr(torch, rp, np.ascontiguousarray(c), np.ascontiguousarray(w))
        h = C.c_void_p(1)
        rc = lib.tilespmv_fsai_create(C.byref(h), n, len(c), C.c_void_p(rpd.data_ptr()), C.c_void_p(cid.data_ptr()), C.c_void_p(vd.data_ptr()), None, C.c_void_p(st))
        assert rc == api.HIP_ERROR_INVALID_VALUE and not h, what
        with pytest.raises(ValueError):
            _fsai(torch, n, (rpd, cid, vd), dt)
    nb, rpb, cib, vb, _ = _system("band70", dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op, _fsai(torch, n, csr, dt) as fs, _fsai(torch, nb, U.device_csr(torch, rpb, cib, vb), dt) as other, api.BlockJacobi(n, 3, dt) as bj:
        for handle in (other.h, None):
            h = C.c_void_p(1)
            assert lib.tilespmv_cg_create_fsai(C.byref(h), op.A.h, handle) == api.HIP_ERROR_INVALID_VALUE and not h
        with pytest.raises(ValueError):
            api.CG(op.A, fsai=other)
        dinv = U.vec(torch, np.ones(n), n, dt)
        with pytest.raises(ValueError):
            api.CG(op.A, dinv.data_ptr(), fsai=fs)
        with pytest.raises(ValueError):
            api.CG(op.A, block=bj, fsai=fs)
        with api.CG(op.A, fsai=fs) as sv:
            assert sv.h
        rd, zd = U.vec(torch, np.ones(n + 1), n + 1, dt), U.vec(torch, None, n + 1, dt)
        item = dt.itemsize
        for r_, z_ in ((rd.data_ptr() + item, zd.data_ptr()), (rd.data_ptr(), zd.data_ptr() + item), (rd.data_ptr(), rd.data_ptr()), (0, zd.data_ptr()), (rd.data_ptr(), 0)):
            assert lib.tilespmv_fsai_apply(fs.h, C.c_void_p(r_), C.c_void_p(z_), C.c_void_p(st)) == api.HIP_ERROR_INVALID_VALUE
            with pytest.raises(ValueError):
                fs.apply(r_, z_, st)
        assert lib.tilespmv_fsai_apply_dot(fs.h, C.c_void_p(rd.data_ptr()), C.c_void_p(zd.data_ptr()), None, C.c_void_p(st)) == api.HIP_ERROR_INVALID_VALUE
        torch.cuda.synchronize()
        assert not U.host(zd, n + 1).any()                         # (nothing was launched)
        fs.apply(rd.data_ptr(), zd.data_ptr(), st)                # (aligned and distinct: accepted)
        torch.cuda.synchronize()
        assert U.host(zd, n).any()
