"""The block-Jacobi preconditioner on the GPU (tilespmv_block_jacobi_*, tilespmv_cg_create_block, tilespmv_bicgstab_create_block; include/tilespmv.h) against its
numpy mirror (tests/block_jacobi_mirror.py, itself checked by tests/test_block_jacobi_cpu.py) and scipy's direct solutions.  Plans are deterministic=1, placement_tries=1.

M^-1 is read back through the public interface: applying the object to the indicator vector of the rows i with i % bs = j returns plane j exactly (every other product is a
zero)."""
import ctypes as C

import numpy as np
import pytest

import block_jacobi_mirror as M
import cg_mirror as CM
import gpu_solver_util as U
import solver_sizes as SS
from gpu_solver_util import DTYPES, PRODUCT_TOL, SENTINEL, torch_cuda  # noqa: F401
from tilespmv_amd import _lib, api

pytestmark = pytest.mark.gpu

CASES = [("lap55", bs) for bs in (1, 2, 3, 5, 7, 16)] + [("femblk10", bs) for bs in (3, 6, 16)]
_CACHE = {}


def _system(name, dtype):
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    return n, rp, ci, v.astype(dt), M.rhs(n).astype(dt)


def _updated(torch, n, bs, dt, csr):
    bj = api.BlockJacobi(n, bs, dt)
    bj.update(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), U.stream(torch))
    return bj


def _planes(torch, bj, n, bs, dt):
    """M^-1 as the library holds it, [bs, n], read by bs applies to indicator vectors."""
    P = np.zeros((bs, n), dtype=dt)
    zd = U.vec(torch, None, n, dt)
    for j in range(bs):
        e = np.zeros(n, dtype=dt)
        e[j::bs] = 1
        bj.apply(U.vec(torch, e, n, dt).data_ptr(), zd.data_ptr(), U.stream(torch))
        torch.cuda.synchronize()
        P[j] = U.host(zd, n)
    return P


def _solved(name, dtype):
    """The block-Jacobi (bs = 3) mirror's solve of a named input and the direct solution, once per value type: (xs, mirror iterations, mirror error, planes)."""
    dt = np.dtype(dtype)
    if (name, dt) not in _CACHE:
        n, rp, ci, vt, b = _system(name, dt)
        P, _ = M.update(n, rp, ci, vt, 3, dt)
        xs = M.spsolve_x(n, rp, ci, vt.astype(np.float64), b.astype(np.float64))
        mirror = (M.BiCGStab if name.endswith("_ns") else M.CG)(M.scipy_csr(n, rp, ci, vt), dt, P)
        xm, itm, stm, relm = mirror.solve(b, rtol=M.RTOL[dt], maxiter=2000, check_every=1)
        assert stm == M.CONVERGED
        _CACHE[(name, dt)] = (xs, itm, U.relerr(xm, xs), P)
    return _CACHE[(name, dt)]


# ---- 1. the inverse
def _inverse_ratio(got, n, rp, ci, vt, bs, dt):
    """The largest |GPU - inv64| / (16 bs eps cond_2(B) max|inv64|) over the blocks (none of them singular); a short last block is judged as the block it is."""
    nb, short = (n + bs - 1) // bs, n % bs
    B = M.blocks(n, rp, ci, vt, bs)
    inv64, singular = M.invert(B)
    assert not singular.any()
    pad = np.zeros((bs, nb * bs - n))
    diff = np.abs(np.concatenate([got.astype(np.float64) - M.planes(inv64, n), pad], axis=1)).reshape(bs, nb, bs).max(axis=(0, 2))
    cond, big = np.linalg.cond(B), np.abs(inv64).max(axis=(1, 2))
    if short:
        cond[-1], big[-1] = np.linalg.cond(B[-1][:short, :short]), np.abs(inv64[-1][:short, :short]).max()
    return float((diff / (16 * bs * np.finfo(dt).eps * cond * big)).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,bs", CASES)
def test_the_inverse_equals_the_mirror(torch_cuda, name, bs, dtype):
    """Per block |GPU - inv64| <= 16 bs eps cond_2(B) max|inv64|: the forward error of elimination with partial pivoting at a growth factor of 1 (the rounding of the result to
    the value type, eps max|inv64| / 2, is inside it).  bs = 1 in fp64: the bits of tilespmv_csr_diagonal_device(invert = 1)."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with _updated(torch, n, bs, dt, csr) as bj:
        info = bj.info(U.stream(torch))
        got = _planes(torch, bj, n, bs, dt)
    nb = (n + bs - 1) // bs
    assert info == {"rows": n, "block_size": bs, "blocks": nb, "singular_blocks": 0, "device_bytes": info["device_bytes"], "dot_partials": SS.parts(n, SS.vpl(dt))}
    assert bs * n * dt.itemsize <= info["device_bytes"] <= bs * (n * dt.itemsize + 255) + 256
    ratio = _inverse_ratio(got, n, rp, ci, vt, bs, dt)
    print("%s bs %d %s: largest |GPU - inv64| / bound over the blocks = %.3g" % (name, bs, dt, ratio))
    assert ratio <= 1.0
    short = n % bs
    if short:
        assert not got[short:, n - short:].any()
    if bs == 1 and dt == np.float64:
        dinv = U.vec(torch, None, n, dt)
        api.csr_diagonal_device(n, csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dinv.data_ptr(), invert=True, stream=U.stream(torch), dtype=dt)
        torch.cuda.synchronize()
        assert np.array_equal(got[0], U.host(dinv, n))


# ---- 2. pivoting, singular blocks
@pytest.mark.parametrize("dtype", DTYPES)
def test_pivoting_and_singular_blocks(torch_cuda, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, v = M.problem("pivot2")
    csr = U.device_csr(torch, rp, ci, v.astype(dt))
    with _updated(torch, n, 2, dt, csr) as bj:
        assert bj.info(U.stream(torch))["singular_blocks"] == 1
        P = _planes(torch, bj, n, 2, dt)
        third, half = dt.type(1.0 / 3.0), dt.type(0.5)
        for k in range(n // 2):
            block = np.array([[P[0, 2 * k], P[1, 2 * k]], [P[0, 2 * k + 1], P[1, 2 * k + 1]]])
            assert np.array_equal(block, np.eye(2) if k == 5 else np.array([[0, third], [half, 0]], dtype=dt)), (k, block)
        # nonsingular values on the same pattern: the counter is cleared
        v2 = v.copy()
        rows = np.repeat(np.arange(n), np.diff(rp))
        v2[(rows == 10) & (ci == 10)] = 3.0
        v2d = torch.from_numpy(v2.astype(dt)).cuda()
        bj.update(csr[0].data_ptr(), csr[1].data_ptr(), v2d.data_ptr(), U.stream(torch))
        assert bj.info(U.stream(torch))["singular_blocks"] == 0
        P2 = _planes(torch, bj, n, 2, dt)
        assert _inverse_ratio(P2, n, rp, ci, v2.astype(dt), 2, dt) <= 1.0 and np.array_equal(P2[:, :10], P[:, :10]) and np.array_equal(P2[:, 12:], P[:, 12:])


# ---- 3. apply
def _check_apply(torch, dt, n, bs, bj, P, label):
    """apply and apply_dot on a random r against numpy with the planes P; the sentinels behind z; r untouched."""
    r = np.random.default_rng(41).uniform(-1, 1, n).astype(dt)
    want = M.apply(P, r)
    bound = 100 * PRODUCT_TOL[dt]
    rd, zd, z2 = U.vec(torch, r, n, dt), U.vec(torch, None, n, dt), U.vec(torch, None, n, dt)
    parts = torch.full((1024 + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    bj.apply(rd.data_ptr(), zd.data_ptr(), U.stream(torch))
    bj.apply(rd.data_ptr(), z2.data_ptr(), U.stream(torch), d_partials=parts.data_ptr())
    torch.cuda.synchronize()
    z = U.host(zd, n)
    np_ = SS.parts(n, SS.vpl(dt))
    p = parts.cpu().numpy()
    dot = float(np.dot(r.astype(np.float64), want.astype(np.float64)))
    err, derr = U.relerr(z, want.astype(np.float64)), U.dist(float(p[:np_].sum()), dot)
    print("%s bs %d %s: |z - numpy| / |numpy| = %.3g, r.z from %d partials %.3g (bound %.3g)" % (label, bs, dt, err, np_, derr, bound))
    assert err <= bound and derr <= bound
    assert np.array_equal(z, U.host(z2, n))
    U.intact((parts, np_), (zd, n), (z2, n), (rd, n))
    assert np.array_equal(U.host(rd, n), r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,bs", CASES)
def test_apply_equals_numpy(torch_cuda, name, bs, dtype):
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system(name, dt)
    with _updated(torch, n, bs, dt, U.device_csr(torch, rp, ci, vt)) as bj:
        _check_apply(torch, dt, n, bs, bj, _planes(torch, bj, n, bs, dt), name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_past_the_partial_sum_cap(torch_cuda, dtype):
    """tri_capped, bs = 3: 1024 partials and a second sweep over the workgroups, the longest scalar tail, a short last block.  Then one CG iteration on its plan against the mirror:
    k_cg_zstep folds the 1024 partials in four passes."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, v = M.tri_capped(dt)
    vt = v.astype(dt)
    assert SS.walk(n, SS.vpl(dt)).parts == 1024 and SS.walk(n, SS.vpl(dt)).sweeps == 2
    P, count = M.update(n, rp, ci, vt, 3, dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with _updated(torch, n, 3, dt, csr) as bj:
        _check_apply(torch, dt, n, 3, bj, P, "tri_capped")
        b = M.rhs(n).astype(dt)
        m = M.CG(M.scipy_csr(n, rp, ci, vt), dt, P)
        m.begin(b); m.iterate(1)
        plan = api.Plan.from_csr(n, n, len(ci), rp, ci, vt, dtype=dt, deterministic=1, placement_tries=1)
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with api.CG(plan, block=bj) as cg:
            cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
            cg.iterate(xd.data_ptr(), 1, U.stream(torch))
            s = cg.state(U.stream(torch))
        plan.close()
        dx, drr = U.relerr(U.host(xd, n), m.x.astype(np.float64)), U.dist(s["rr"], m.rr)
        print("tri_capped %s: after 1 iteration |x - mirror| / |mirror| = %.3g, rr %.3g" % (dt, dx, drr))
        assert s["iterations"] == 1 and max(dx, drr, U.dist(s["bb"], m.bb)) <= 100 * PRODUCT_TOL[dt]


# ---- 4 / 5. the solvers
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
@pytest.mark.parametrize("name,Solver", [("femblk10", "CG"), ("femblk10_ns", "BiCGStab")])
def test_the_solvers_with_a_block_preconditioner(torch_cuda, name, Solver, dtype):
    """Early iterations equal the mirror; solve with maxiter = 2 x the mirror's count: CONVERGED, error against spsolve within 10 x the mirror's; the point-Jacobi solver on the
    same plan at that cap: MAXITER."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, vt, b = _system(name, dt)
    xs, itm, errm, P = _solved(name, dt)
    Api, Mirror = getattr(api, Solver), getattr(M, Solver)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op, _updated(torch, n, 3, dt, csr) as bj:
        _early(torch, dt, lambda: Api(op.A, block=bj), Mirror(M.scipy_csr(n, rp, ci, vt), dt, P), b, n, name)
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
        with Api(op.A, block=bj) as sv:
            s = sv.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        err = U.relerr(U.host(xd, n), xs)
        print("%s %s: block Jacobi %d iterations (mirror %d), sqrt(rr/bb) %.3g, error vs spsolve %.3g (mirror %.3g)" % (name, dt, s["iterations"], itm, s["relative_residual"], err, errm))
        assert s["status"] == api.CG_CONVERGED and s["relative_residual"] <= M.RTOL[dt] and s["iterations"] <= 2 * itm
        assert err <= 10 * errm
        dinv = U.vec(torch, None, n, dt)
        api.csr_diagonal_device(n, csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), dinv.data_ptr(), invert=True, stream=stream, dtype=dt)
        xd[:n].zero_()
        with Api(op.A, dinv.data_ptr()) as sv:
            sp = sv.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, check_every=8, stream=stream)
        print("%s %s: point Jacobi on the same plan: %d iterations, status %s, sqrt(rr/bb) %.3g" % (name, dt, sp["iterations"], sp["status_name"], sp["relative_residual"]))
        assert sp["status"] == api.CG_MAXITER and sp["iterations"] == 2 * itm


def test_sparse_operator_takes_the_preconditioner(torch_cuda):
    torch = torch_cuda
    dt = np.dtype(np.float64)
    for name, method in (("femblk10", "cg"), ("femblk10_ns", "bicgstab")):
        n, rp, ci, vt, b = _system(name, dt)
        xs, itm, errm, P = _solved(name, dt)
        bd = torch.from_numpy(b).cuda()
        with U.square_op(n, rp, ci, vt, dt) as op, _updated(torch, n, 3, dt, U.device_csr(torch, rp, ci, vt)) as bj:
            x, info = getattr(op, method)(bd, rtol=M.RTOL[dt], maxiter=2 * itm, precond=bj)
            assert info["converged"] and info["iterations"] <= 2 * itm and U.relerr(x.cpu().numpy(), xs) <= 10 * errm
            with pytest.raises(ValueError):
                getattr(op, method)(torch.stack([bd, bd], dim=1).contiguous(), precond=bj)
            with pytest.raises(ValueError):
                getattr(op, method)(bd, dinv=torch.ones(n, dtype=bd.dtype, device="cuda"), precond=bj)


# ---- 6. value refresh
@pytest.mark.parametrize("dtype", DTYPES)
def test_value_refresh(torch_cuda, dtype):
    """A plan with a value map and an object updated from lap55-like values on femblk10's pattern; update_values and bj.update from femblk10's values: the inverse has the bytes of
    a fresh object's and the solve the bits of a fresh solver's."""
    torch, dt = torch_cuda, np.dtype(dtype)
    stream = U.stream(torch)
    n, rp, ci, v2, b = _system("femblk10", dt)
    v1 = CM.spd_values(n, rp, ci).astype(dt)
    xs, itm, errm, P = _solved("femblk10", dt)
    rpd, cid, v1d = U.device_csr(torch, rp, ci, v1)
    v2d = torch.from_numpy(v2).cuda()
    bd, xd = U.vec(torch, b, n, dt), U.vec(torch, None, n, dt)
    with U.square_op(n, rp, ci, v1, dt, value_map=True) as op, _updated(torch, n, 3, dt, (rpd, cid, v1d)) as bj:
        with api.CG(op.A, block=bj) as cg:
            s1 = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=500, stream=stream)
            assert s1["status"] == api.CG_CONVERGED
            P1 = _planes(torch, bj, n, 3, dt)
            op.update_values(v2d.data_ptr(), stream)
            bj.update(rpd.data_ptr(), cid.data_ptr(), v2d.data_ptr(), stream)
            xd[:n].zero_()
            s2 = cg.solve(bd.data_ptr(), xd.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
            x2 = U.host(xd, n)
        P2 = _planes(torch, bj, n, 3, dt)
    with U.square_op(n, rp, ci, v2, dt, value_map=True) as fresh, _updated(torch, n, 3, dt, (rpd, cid, v2d)) as bjf:
        Pf = _planes(torch, bjf, n, 3, dt)
        xf = U.vec(torch, None, n, dt)
        with api.CG(fresh.A, block=bjf) as cg:
            sf = cg.solve(bd.data_ptr(), xf.data_ptr(), rtol=M.RTOL[dt], maxiter=2 * itm, stream=stream)
    print("%s: refreshed %d iterations, fresh %d; error vs spsolve %.3g" % (dt, s2["iterations"], sf["iterations"], U.relerr(x2, xs)))
    assert not np.array_equal(P1, P2) and P2.tobytes() == Pf.tobytes()
    assert s2["status"] == api.CG_CONVERGED and sf["status"] == api.CG_CONVERGED
    assert s2["iterations"] == sf["iterations"] and s2["rr"] == sf["rr"] and np.array_equal(x2, U.host(xf, n))
    assert U.relerr(x2, xs) <= 10 * errm


# ---- 7. fixed order
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_and_the_sums_have_a_fixed_order(torch_cuda, dtype):
    """Two runs of update + 10 CG iterations on separately created objects and operators: bit-identical M^-1, x and rr."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("femblk10", dt)
    bd = U.vec(torch, b, n, dt)
    results = []
    for _ in range(2):
        with U.square_op(n, rp, ci, vt, dt) as op, _updated(torch, n, 3, dt, U.device_csr(torch, rp, ci, vt)) as bj:
            xd = U.vec(torch, None, n, dt)
            with api.CG(op.A, block=bj) as cg:
                cg.begin(bd.data_ptr(), xd.data_ptr(), U.stream(torch))
                cg.iterate(xd.data_ptr(), 10, U.stream(torch))
                s = cg.state(U.stream(torch))
            results.append((_planes(torch, bj, n, 3, dt), U.host(xd, n), s))
    (Pa, xa, sa), (Pb, xb, sb) = results
    assert sa["iterations"] == 10 and sa["status"] == api.CG_RUNNING and xa.any()
    assert Pa.tobytes() == Pb.tobytes() and np.array_equal(xa, xb) and sa["rr"] == sb["rr"]


# ---- 8. hipGraph
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_begin_and_iterate_are_capturable_into_a_hip_graph(torch_cuda, dtype):
    """update + begin + iterate(5) captured with torch's graph API on a side stream (one linear chain, as the solvers' capture tests do) and replayed twice from the same x0: each
    replay equals the eager run bit for bit.  Between the replays M^-1 is overwritten with another matrix's: the replayed update restores it."""
    torch, dt = torch_cuda, np.dtype(dtype)
    n, rp, ci, vt, b = _system("femblk10", dt)
    x0 = (0.01 * M.rhs(n)[::-1]).astype(dt)
    rpd, cid, vd = U.device_csr(torch, rp, ci, vt)
    other = torch.from_numpy(CM.spd_values(n, rp, ci).astype(dt)).cuda()
    with U.square_op(n, rp, ci, vt, dt) as op, api.BlockJacobi(n, 3, dt) as bj:
        bd, xd = U.vec(torch, b, n, dt), U.vec(torch, x0, n, dt)
        cg = api.CG(op.A, block=bj)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()

        def chain(st):
            bj.update(rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), st)
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
            bj.update(rpd.data_ptr(), cid.data_ptr(), other.data_ptr(), U.stream(torch))
            torch.cuda.synchronize()
            graph.replay(); torch.cuda.synchronize()
            s = cg.state(U.stream(torch))
            assert np.array_equal(U.host(xd, n), x5) and not np.array_equal(x5, x0)
            assert s["iterations"] == 5 and s["rr"] == s5["rr"] and s["status"] == api.CG_RUNNING
        del graph
        cg.close()


# ---- 9. refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(torch_cuda, dtype):
    """Mismatched rows, block sizes 0 and 17, misaligned or aliased vectors, block together with d_dinv: hipErrorInvalidValue and no handle; the wrappers raise ValueError."""
    torch, dt = torch_cuda, np.dtype(dtype)
    lib = _lib.load(dt)
    n, rp, ci, vt, b = _system("lap55", dt)
    for bs in (0, 17):
        h = C.c_void_p(1)
        assert lib.tilespmv_block_jacobi_create(C.byref(h), n, bs) == api.HIP_ERROR_INVALID_VALUE and not h
        with pytest.raises(ValueError):
            api.BlockJacobi(n, bs, dt)
    csr = U.device_csr(torch, rp, ci, vt)
    with U.square_op(n, rp, ci, vt, dt) as op, _updated(torch, n, 3, dt, csr) as bj, api.BlockJacobi(n + 1, 3, dt) as longer:
        for create, Api in ((lib.tilespmv_cg_create_block, api.CG), (lib.tilespmv_bicgstab_create_block, api.BiCGStab)):
            h = C.c_void_p(1)
            assert create(C.byref(h), op.A.h, longer.h) == api.HIP_ERROR_INVALID_VALUE and not h
            with pytest.raises(ValueError):
                Api(op.A, block=longer)
            dinv = U.vec(torch, np.ones(n), n, dt)
            with pytest.raises(ValueError):
                Api(op.A, dinv.data_ptr(), block=bj)
            with Api(op.A, block=bj) as sv:
                assert sv.h
        rd, zd = U.vec(torch, np.ones(n + 1), n + 1, dt), U.vec(torch, None, n + 1, dt)
        st = U.stream(torch)
        item = dt.itemsize
        for r_, z_ in ((rd.data_ptr() + item, zd.data_ptr()), (rd.data_ptr(), zd.data_ptr() + item), (rd.data_ptr(), rd.data_ptr()), (0, zd.data_ptr()), (rd.data_ptr(), 0)):
            assert lib.tilespmv_block_jacobi_apply(bj.h, C.c_void_p(r_), C.c_void_p(z_), C.c_void_p(st)) == api.HIP_ERROR_INVALID_VALUE
            with pytest.raises(ValueError):
                bj.apply(r_, z_, st)
        assert lib.tilespmv_block_jacobi_apply_dot(bj.h, C.c_void_p(rd.data_ptr()), C.c_void_p(zd.data_ptr()), None, C.c_void_p(st)) == api.HIP_ERROR_INVALID_VALUE
        torch.cuda.synchronize()
        assert not U.host(zd, n + 1).any()                         # (nothing was launched)
        bj.apply(rd.data_ptr(), zd.data_ptr(), st)                # (aligned and distinct: accepted)
        torch.cuda.synchronize()
        assert U.host(zd, n).any()
