"""A sparse operator with both products, ``A x`` and ``A^T x``, from one CSR.

    op = SparseOperator(rows, cols, rp, ci, v)                     # host CSR (numpy); or CUDA tensors / from_device_csr(...) for a device CSR
    y = op.matvec(x)                                                 # A x      (plan of A)
    z = op.rmatvec(u)                                                # A^T u    (plan of A^T, built on the device from A's CSR: TILESPMV_CREATE_TRANSPOSE)
    op = SparseOperator(..., value_map=True); op.update_values(v2)   # new values of the same pattern: both plans refreshed from A's one value array
    x, info = op.cgls(b)                                             # least squares  min ||A x - b|| (+ damp, column scaling): the solver in the library
    x, info = cgls(op, b)                                            # ... the same as a loop of torch operations (the A/B baseline of scripts/cgls_time.py)
    x, info = op.cg(b)                                               # A x = b, A symmetric positive definite: the solver in the library
    X, infos = op.cg(B)                                              # B of shape (rows, k): k systems in lock-step around the multi-vector product
    x, info = op.bicgstab(b)                                         # A x = b, A square and not symmetric: the solver in the library
    x, info = bicgstab(op, b)                                        # ... the same as a loop of torch operations (the A/B baseline of scripts/bicgstab_time.py)
    x, info = op.gmres(b)                                            # A x = b where BiCGStab breaks down or stagnates: restarted GMRES in the library
    x, info = gmres(op, b)                                           # ... the same as a loop of torch operations
    x, info = op.minres(b)                                 # A x = b, A symmetric and indefinite (saddle point, KKT): the solver in the library
    x, info = minres(op, b)                                          # ... the same as a loop of torch operations (the A/B baseline of scripts/minres_time.py)

The plan of A^T is a plan like any other (tuned kernels, form choice, ordered sums); there is no scatter form of A^T x.
"""
import numpy as np

from . import api


def _is_tensor(a):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(a, torch.Tensor)


def _stream(stream):
    if stream is not None:
        return stream
    import torch
    return torch.cuda.current_stream().cuda_stream


def _info(s):
    """The info dict of ``cg``, ``bicgstab`` and ``minres`` from the solver's state dict (the rr of MINRES is r.M^-1 r, below 0 at a breakdown under a ``minv`` that is not positive: the residual is 0 then)."""
    return {"iterations": s["iterations"], "residual": max(s["rr"], 0.0) ** 0.5, "relative_residual": s["relative_residual"], "converged": s["status"] == api.CG_CONVERGED,
            "status": s["status_name"]}


class SparseOperator:
    """The plans of A (``rows x cols``) and of A^T from one CSR.

    ``rp`` / ``ci`` / ``v``: numpy arrays (host CSR: ``Plan.from_csr``) or CUDA tensors (device CSR: ``Plan.from_device_csr``; the row pointer starts at 0).  ``value_map=True``
    gives both plans a value map that indexes A's value array, so that ``update_values`` refreshes both from it.  Every other keyword goes to both plan creations
    (``cdna4``, ``hyb`` (host CSR only), ``coo_mode``, knobs such as ``placement_tries=1``)."""

    def __init__(self, rows, cols, rp, ci, v, dtype=None, value_map=False, **opts):
        self.shape = (rows, cols)
        self.value_map = value_map
        if _is_tensor(v):
            import torch
            dtype = np.dtype(dtype or str(v.dtype).replace("torch.", ""))
            rp32 = rp.to(device=v.device, dtype=torch.int32).contiguous()
            ci32 = ci.to(device=v.device, dtype=torch.int32).contiguous()
            vc = v.contiguous()
            nnz = int(rp32[rows].item())
            self._init_device(rows, cols, nnz, rp32.data_ptr(), ci32.data_ptr(), vc.data_ptr(), dtype, value_map, opts)
        else:
            dtype = np.dtype(dtype or np.asarray(v).dtype)
            rp = np.ascontiguousarray(rp, dtype=np.int32)
            nnz = int(rp[rows]) - int(rp[0])
            self.dtype, self.nnz = dtype, nnz
            self.A = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, value_map=value_map, **opts)
            try:
                self.AT = api.Plan.from_csr(rows, cols, nnz, rp, ci, v, dtype=dtype, value_map=value_map, transpose=True, **opts)
            except Exception:
                self.A.close()
                raise

    @classmethod
    def from_device_csr(cls, rows, cols, nnz, d_rp, d_ci, d_v, dtype, value_map=False, **opts):
        """Device ADDRESSES of an int32 row pointer (starting at 0), int32 column indices and values, as ``Plan.from_device_csr`` takes them; borrowed for the call."""
        self = cls.__new__(cls)
        self.shape = (rows, cols)
        self.value_map = value_map
        self._init_device(rows, cols, nnz, d_rp, d_ci, d_v, np.dtype(dtype), value_map, opts)
        return self

    def _init_device(self, rows, cols, nnz, d_rp, d_ci, d_v, dtype, value_map, opts):
        self.dtype, self.nnz = dtype, nnz
        self.A = api.Plan.from_device_csr(rows, cols, nnz, d_rp, d_ci, d_v, dtype, value_map=value_map, **opts)
        try:
            self.AT = api.Plan.from_device_csr(rows, cols, nnz, d_rp, d_ci, d_v, dtype, value_map=value_map, transpose=True, **opts)
        except Exception:
            self.A.close()
            raise

    # ---- products
    def _apply(self, plan, x, y, stream):
        m, n = plan.shape
        if not _is_tensor(x):   # device addresses: the caller owns both vectors
            if y is None:
                raise ValueError("with a device address for x, y must be a device address too")
            plan.spmv(x, y, stream or 0)
            return y
        import torch
        if x.dim() != 1 or x.numel() != n or not x.is_contiguous():
            raise ValueError("x must be a contiguous vector of %d elements" % n)
        if y is None:
            y = torch.empty(m + 16, dtype=x.dtype, device=x.device)[:m]   # (room behind the vector, as every y of this project has)
        elif y.numel() < m or not y.is_contiguous():
            raise ValueError("y must be a contiguous vector of at least %d elements" % m)
        plan.spmv(x.data_ptr(), y.data_ptr(), _stream(stream))
        return y

    def matvec(self, x, y=None, stream=None):
        """y = A x (x: cols, y: rows).  Torch CUDA vectors (y allocated when None, returned) or device addresses; asynchronous on ``stream`` (default: torch's current)."""
        return self._apply(self.A, x, y, stream)

    def rmatvec(self, u, v=None, stream=None):
        """v = A^T u (u: rows, v: cols), as ``matvec``."""
        return self._apply(self.AT, u, v, stream)

    def _apply_mm(self, plan, X, Y, nvec, stream):
        m, n = plan.shape
        if not _is_tensor(X):
            if Y is None or nvec is None:
                raise ValueError("with a device address for X, Y and nvec must be given")
            plan.spmm(X, Y, nvec, stream or 0)
            return Y
        import torch
        if X.dim() != 2 or X.shape[0] != n or not X.is_contiguous():
            raise ValueError("X must be a contiguous (%d, nvec) matrix" % n)
        nvec = X.shape[1]
        if Y is None:
            Y = torch.empty((m + 16, nvec), dtype=X.dtype, device=X.device)[:m]
        elif Y.dim() != 2 or Y.shape[0] < m or Y.shape[1] != nvec or not Y.is_contiguous():
            raise ValueError("Y must be a contiguous (%d, %d) matrix" % (m, nvec))
        plan.spmm(X.data_ptr(), Y.data_ptr(), nvec, _stream(stream))
        return Y

    def spmm(self, X, Y=None, nvec=None, stream=None):
        """Y = A X, X row-major (cols, nvec), nvec in {1, 2, 4, 8}."""
        return self._apply_mm(self.A, X, Y, nvec, stream)

    def rspmm(self, U, V=None, nvec=None, stream=None):
        """V = A^T U, U row-major (rows, nvec)."""
        return self._apply_mm(self.AT, U, V, nvec, stream)

    def update_values(self, d_vals, stream=None):
        """New values of A, same pattern (``value_map=True``): both plans rewritten from A's one value array (a CUDA tensor, or its device address), asynchronously and in order
        on one stream — capturable into a graph."""
        if not self.value_map:
            raise RuntimeError("SparseOperator.update_values: create the operator with value_map=True")
        if _is_tensor(d_vals):
            if d_vals.numel() < self.nnz or not d_vals.is_contiguous():
                raise ValueError("update_values: a contiguous array of at least %d values" % self.nnz)
            st = _stream(stream)
            d_vals = d_vals.data_ptr()
        else:
            st = stream or 0
        self.A.update_values(d_vals, st)
        self.AT.update_values(d_vals, st)

    def _square(self, what):
        rows, cols = self.shape
        if rows != cols:
            raise ValueError("%s needs a square operator; this one is %d x %d (least squares: cgls)" % (what, rows, cols))

    def _solve(self, make, b, x0, n, scaling_name, scaling, stream, maxiter=None, **solve_args):
        """What ``cg`` (1-D ``b``), ``bicgstab``, ``minres`` and ``cgls`` share: ``b`` is a contiguous CUDA vector of ``rows`` elements of the operator's type; the diagonal
        ``scaling`` (or None) and ``x0`` (or None: zeros) have the ``n`` elements of x and b's type; ``maxiter`` defaults to ``2 * n``.  ``make(address of the diagonal or None)``
        creates the ``api`` solver, which lives for the one ``solve``.  Returns ``(x, the solver's final state dict)``."""
        import torch
        rows = self.shape[0]
        if not _is_tensor(b) or b.dim() != 1 or b.numel() != rows or not b.is_contiguous() or np.dtype(str(b.dtype).replace("torch.", "")) != self.dtype:
            raise ValueError("b must be a contiguous %s vector of %d elements" % (self.dtype, rows))
        if scaling is not None and (not _is_tensor(scaling) or scaling.numel() != n or not scaling.is_contiguous() or scaling.dtype != b.dtype):
            raise ValueError("%s must be a contiguous vector of %d elements of b's type" % (scaling_name, n))
        if x0 is not None and (not _is_tensor(x0) or x0.dim() != 1 or x0.numel() != n or x0.dtype != b.dtype):
            raise ValueError("x0 must be a vector of %d elements of b's type" % n)
        x = torch.zeros(n + 16, dtype=b.dtype, device=b.device)[:n]
        if x0 is not None:
            x.copy_(x0)
        st = _stream(stream)
        solver = make(None if scaling is None else scaling.data_ptr())
        try:
            s = solver.solve(b.data_ptr(), x.data_ptr(), maxiter=2 * n if maxiter is None else maxiter, stream=st, **solve_args)
        finally:
            solver.close()
        return x, s

    def cg(self, b, x0=None, rtol=1e-10, maxiter=None, check_every=8, dinv=None, stream=None, precond=None):
        """A x = b by conjugate gradients in the library (``api.CG`` over the plan of A: symmetric positive definite A) — the product and three fused kernels per
        iteration, every scalar on the device, one host synchronisation per ``check_every`` iterations.  ``b``: a torch CUDA vector of ``rows`` elements; ``dinv``: the inverse
        diagonal as a CUDA vector (Jacobi; ``api.csr_diagonal_device(..., invert=True)`` makes it), None = plain CG.  Stops at ``sqrt(rr / bb) <= rtol`` or after ``maxiter``
        iterations (default ``2 * rows``).  Returns ``(x, info)`` with ``info = {"iterations", "residual", "relative_residual", "converged", "status"}``.
        A contiguous 2-D ``b`` of shape (rows, k) solves k systems at once (``_cg_multi``): ``(X, [info] * k)``.
        ``precond``: an updated ``api.BlockJacobi`` (block Jacobi) or an ``api.FSAI`` of ``rows`` rows instead of ``dinv``; a 1-D ``b`` only."""
        self._square("cg")
        if _is_tensor(b) and b.dim() == 2:
            if precond is not None:
                raise ValueError("precond (block Jacobi, FSAI) applies to a 1-D b only")
            return self._cg_multi(b, x0, rtol, maxiter, check_every, dinv, stream)
        which = "fsai" if isinstance(precond, api.FSAI) else "block"
        x, s = self._solve(lambda d: api.CG(self.A, d, **{which: precond}), b, x0, self.shape[0], "dinv", dinv, stream, rtol=rtol, maxiter=maxiter, check_every=check_every)
        return x, _info(s)

    @staticmethod
    def cg_groups(k):
        """How ``cg`` splits ``k`` right-hand sides: ``[(first column, columns, nvec), ...]`` — groups of at most 8 columns, each solved by ``api.CGMulti`` with nvec = the next
        of 2, 4, 8 (a lone last column: nvec = 1, the single solver)."""
        out = []
        for g in range(0, k, 8):
            w = min(8, k - g)
            out.append((g, w, 1 if w == 1 else 2 if w == 2 else 4 if w <= 4 else 8))
        return out

    def _cg_multi(self, b, x0, rtol, maxiter, check_every, dinv, stream):
        """``cg`` for a contiguous ``b`` of shape (rows, k), k >= 1: the columns are solved in lock-step around the multi-vector product (``api.CGMulti``) in the
        groups of ``cg_groups(k)``; a group narrower than its nvec is padded with zero columns, which the library returns as x = 0 after 0 iterations without touching the others.
        Returns ``(X, infos)``: ``X`` of shape (rows, k) and a list of k info dicts as the 1-D form returns."""
        import torch
        rows = self.shape[0]
        k = b.shape[1]
        if b.shape[0] != rows or k < 1 or not b.is_contiguous():
            raise ValueError("b must be a contiguous (%d, k) matrix, k >= 1" % rows)
        if x0 is not None and (tuple(x0.shape) != (rows, k)):
            raise ValueError("x0 must have b's shape")
        if dinv is not None and (dinv.numel() != rows or not dinv.is_contiguous() or dinv.dtype != b.dtype):
            raise ValueError("dinv must be a contiguous vector of %d elements of b's type" % rows)
        maxiter = 2 * rows if maxiter is None else maxiter
        st = _stream(stream)
        X = torch.zeros((rows + 16, k), dtype=b.dtype, device=b.device)[:rows]
        if x0 is not None:
            X.copy_(x0)
        infos = []
        for g, w, nvec in self.cg_groups(k):
            whole = w == k and nvec == k and b.data_ptr() % 16 == 0   # the group is b itself: no copies
            if whole:
                Bg, Xg = b, X
            else:
                Bg = torch.zeros((rows + 16, nvec), dtype=b.dtype, device=b.device)[:rows]
                Xg = torch.zeros((rows + 16, nvec), dtype=b.dtype, device=b.device)[:rows]
                Bg[:, :w].copy_(b[:, g:g + w])
                Xg[:, :w].copy_(X[:, g:g + w])
            solver = api.CGMulti(self.A, nvec, None if dinv is None else dinv.data_ptr())
            try:
                states = solver.solve(Bg.data_ptr(), Xg.data_ptr(), rtol=rtol, maxiter=maxiter, check_every=check_every, stream=st)
            finally:
                solver.close()
            if not whole:
                X[:, g:g + w].copy_(Xg[:, :w])
            for s in states[:w]:
                infos.append({"iterations": s["iterations"], "residual": s["rr"] ** 0.5, "relative_residual": s["relative_residual"],
                              "converged": s["status"] == api.CG_CONVERGED, "status": s["status_name"]})
        return X, infos

    def cgls(self, b, x0=None, rtol=1e-10, maxiter=None, check_every=8, cinv=None, damp=0.0, stream=None):
        """Least squares ``min |A x - b|^2 + damp^2 |x|^2`` by CGLS in the library (``api.CGLS`` over both plans) — the two products and four fused kernels per
        iteration, every scalar on the device, one host synchronisation per ``check_every`` iterations.  ``b``: a contiguous torch CUDA vector of ``rows`` elements; ``cinv``: a
        positive diagonal of ``cols`` elements as a CUDA vector (column scaling; ``api.csr_row_sqnorms_device(..., invert=True)`` makes it), None = unpreconditioned.  Stops at
        ``|A^T r - damp^2 x| <= rtol |A^T b|`` or after ``maxiter`` iterations (default ``2 * cols``).  Returns ``(x, info)`` with ``info = {"iterations", "normal_residual",
        "relative_normal_residual", "residual", "converged", "status"}`` (``residual``: the recurrence's ``|r|``)."""
        x, s = self._solve(lambda d: api.CGLS(self.A, self.AT, d), b, x0, self.shape[1], "cinv", cinv, stream, damp=damp, rtol=rtol, maxiter=maxiter, check_every=check_every)
        info = {"iterations": s["iterations"], "normal_residual": s["nn"] ** 0.5, "relative_normal_residual": s["relative_normal_residual"], "residual": s["rr"] ** 0.5,
                "converged": s["status"] == api.CG_CONVERGED, "status": s["status_name"]}
        return x, info

    def bicgstab(self, b, x0=None, rtol=1e-10, maxiter=None, check_every=8, dinv=None, stream=None, precond=None):
        """A x = b for a square A that need not be symmetric, by BiCGStab in the library (``api.BiCGStab`` over the plan of A) — the two products and five fused
        kernels per iteration, every scalar on the device, one host synchronisation per ``check_every`` iterations.  ``b``: a contiguous torch CUDA vector of ``rows`` elements;
        ``dinv``: the inverse diagonal as a CUDA vector (Jacobi, applied from the right; ``api.csr_diagonal_device(..., invert=True)`` makes it), None = unpreconditioned.  Stops at
        ``sqrt(rr / bb) <= rtol``, after ``maxiter`` iterations (default ``2 * rows``) or at a breakdown.  Returns ``(x, info)`` with ``info = {"iterations", "residual",
        "relative_residual", "converged", "status"}`` (``residual``: the recurrence's ``|r|``).  ``precond``: an updated ``api.BlockJacobi`` of ``rows`` rows instead of ``dinv``
        (block Jacobi, applied from the right)."""
        self._square("bicgstab")
        if precond is not None and _is_tensor(b) and b.dim() == 2:
            raise ValueError("precond (block Jacobi) applies to a 1-D b only")
        x, s = self._solve(lambda d: api.BiCGStab(self.A, d, block=precond), b, x0, self.shape[0], "dinv", dinv, stream, rtol=rtol, maxiter=maxiter, check_every=check_every)
        return x, _info(s)

    def gmres(self, b, x0=None, rtol=1e-10, maxiter=None, check_every=8, restart=30, dinv=None, stream=None, precond=None, basis=None):
        """A x = b for a square A that need not be symmetric, by restarted GMRES in the library (``api.GMRES`` over the plan of A) — one product and four fused
        kernels per iteration, every scalar on the device, one host synchronisation per ``check_every`` iterations; the solver for what ``bicgstab`` breaks down or stagnates on
        (convection-dominated, nearly skew-symmetric).  ``b``: a contiguous torch CUDA vector of ``rows`` elements; ``restart``: 1 .. 64 iterations per cycle; ``dinv``: the inverse
        diagonal as a CUDA vector (Jacobi, applied from the right), None = unpreconditioned; ``precond``: an updated ``api.BlockJacobi`` of ``rows`` rows instead of ``dinv``.
        Stops at ``sqrt(rr / bb) <= rtol``, after ``maxiter`` iterations (default ``2 * rows``) or at a breakdown.  Returns ``(x, info)`` with ``info = {"iterations", "residual",
        "relative_residual", "converged", "status"}`` (``residual``: ``|b - A x|`` recomputed for the returned x).  ``basis``: None, ``"value"``, ``"float32"``, 4 or 0 — how the
        Krylov basis is stored (``api.GMRES``): ``"float32"`` on an fp64 operator halves the bytes of the basis, all arithmetic stays double and convergence is
        accepted on a recomputed residual only."""
        self._square("gmres")
        if precond is not None and _is_tensor(b) and b.dim() == 2:
            raise ValueError("precond (block Jacobi) applies to a 1-D b only")
        x, s = self._solve(lambda d: api.GMRES(self.A, restart, d, block=precond, basis=basis), b, x0, self.shape[0], "dinv", dinv, stream, rtol=rtol, maxiter=maxiter, check_every=check_every)
        return x, _info(s)

    def minres(self, b, x0=None, rtol=1e-10, maxiter=None, check_every=8, minv=None, stream=None):
        """A x = b for a square SYMMETRIC A that may be indefinite (saddle-point, KKT), by MINRES in the library (``api.MINRES`` over the plan of A) — one product
        and three fused kernels per iteration, every scalar on the device, one host synchronisation per ``check_every`` iterations; the residual norm never increases.  ``b``: a
        contiguous torch CUDA vector of ``rows`` elements; ``minv``: a POSITIVE diagonal M^-1 as a CUDA vector (``api.csr_abs_diagonal_device(..., invert=True)`` makes one),
        None = unpreconditioned.  Stops at ``sqrt(rr / bb) <= rtol`` (with ``minv``: in the M^-1 norm), after ``maxiter`` iterations (default ``2 * rows``) or at a breakdown.
        Returns ``(x, info)`` with ``info = {"iterations", "residual", "relative_residual", "converged", "status"}`` (``residual``: the recurrence's ``sqrt(rr)``)."""
        self._square("minres")
        x, s = self._solve(lambda d: api.MINRES(self.A, d), b, x0, self.shape[0], "minv", minv, stream, rtol=rtol, maxiter=maxiter, check_every=check_every)
        return x, _info(s)

    def close(self):
        for p in (getattr(self, "A", None), getattr(self, "AT", None)):
            if p is not None:
                p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def bicgstab(op, b, x0=None, tol=1e-10, maxiter=None, dinv=None, check_every=1):
    """``A x = b`` for a square operator by right-preconditioned BiCGStab as a loop of torch operations: the recurrences of ``SparseOperator.bicgstab``, without
    its guards — the baseline of scripts/bicgstab_time.py and a second opinion in tests.  ``b``: a torch CUDA vector of ``rows`` elements; ``dinv``: None or the inverse diagonal.
    Stops when ``|r| <= tol * |b|`` for the recurrence's r (checked every ``check_every`` iterations: each check is one host sync) or after ``maxiter`` iterations (default
    ``2 * rows``).  Returns ``(x, info)`` with ``info = {"iterations", "residual", "relative_residual", "converged"}`` (``residual``: a recomputed ``|b - A x|``)."""
    import torch
    rows, cols = op.shape
    if rows != cols:
        raise ValueError("bicgstab needs a square operator; this one is %d x %d" % (rows, cols))
    if b.numel() != rows:
        raise ValueError("b must have %d elements" % rows)
    maxiter = 2 * rows if maxiter is None else maxiter
    x = torch.zeros(rows, dtype=b.dtype, device=b.device) if x0 is None else x0.clone()
    r = b.clone()
    if x0 is not None:
        r -= op.matvec(x)
    rhat, p = r.clone(), r.clone()
    rho = torch.dot(rhat, r)
    rr = rho.clone()
    norm_b = float(torch.linalg.vector_norm(b))
    v = torch.empty(rows + 16, dtype=b.dtype, device=b.device)[:rows]
    t = torch.empty(rows + 16, dtype=b.dtype, device=b.device)[:rows]
    it, converged = 0, float(rr.sqrt()) <= tol * norm_b
    while not converged and it < maxiter:
        phat = p if dinv is None else dinv * p
        op.matvec(phat, v)
        alpha = rho / torch.dot(rhat, v)
        r.addcmul_(v, -alpha)                       # s, over r
        shat = r if dinv is None else dinv * r
        op.matvec(shat, t)
        omega = torch.dot(t, r) / torch.dot(t, t)
        x.addcmul_(phat, alpha).addcmul_(shat, omega)
        r.addcmul_(t, -omega)
        rho_new = torch.dot(rhat, r)
        rr = torch.dot(r, r)
        beta = (rho_new / rho) * (alpha / omega)
        p.addcmul_(v, -omega).mul_(beta).add_(r)
        rho = rho_new
        it += 1
        if it % check_every == 0 or it == maxiter:
            converged = float(rr.sqrt()) <= tol * norm_b
    res = float(torch.linalg.vector_norm(b - op.matvec(x)))
    info = {"iterations": it, "residual": res, "relative_residual": res / norm_b if norm_b > 0 else 0.0, "converged": bool(converged)}
    return x, info


def gmres(op, b, x0=None, tol=1e-10, maxiter=None, restart=30, dinv=None, check_every=1, basis=None):
    """``A x = b`` for a square operator by right-preconditioned restarted GMRES as a loop of torch operations: the recurrences of ``SparseOperator.gmres`` (DESIGN.md §3.13:
    classical Gram-Schmidt applied twice, the basis a 2-D tensor, ``V @ w`` for the dot products, Givens rotations on the host), without its guards — what the fused solver is
    measured against and a second opinion in tests.  ``b``: a torch CUDA vector of ``rows`` elements; ``dinv``: None or the inverse diagonal.  Stops when the recurrence's residual
    estimate is ``<= tol * |b|`` (checked every ``check_every`` iterations and at the end of a cycle) or after ``maxiter`` iterations (default ``2 * rows``).  Returns ``(x, info)``
    with ``info = {"iterations", "residual", "relative_residual", "converged"}`` (``residual``: a recomputed ``|b - A x|``).  ``basis``: as for ``SparseOperator.gmres``;
    with ``"float32"`` (or 4) the basis is a float32 tensor, a store rounds to nearest and every use — the product, the dots, the subtraction, the close — reads it widened back
    to ``b``'s type.  Convergence is declared at the top of a cycle, on a recomputed residual, in either form."""
    import torch
    rows, cols = op.shape
    if rows != cols:
        raise ValueError("gmres needs a square operator; this one is %d x %d" % (rows, cols))
    if basis not in (None, "value", "float32", 0, 4):
        raise ValueError("basis must be None, 'value', 'float32', 0 or 4, not %r" % (basis,))
    narrow = basis in ("float32", 4) and b.dtype != torch.float32

    def wide(t):
        return t.to(b.dtype) if narrow else t
    if b.numel() != rows:
        raise ValueError("b must have %d elements" % rows)
    maxiter = 2 * rows if maxiter is None else maxiter
    m = int(restart)
    x = torch.zeros(rows, dtype=b.dtype, device=b.device) if x0 is None else x0.clone()
    norm_b = float(torch.linalg.vector_norm(b))
    V = torch.zeros((m + 1, rows), dtype=torch.float32 if narrow else b.dtype, device=b.device)
    w = torch.empty(rows + 16, dtype=b.dtype, device=b.device)[:rows]
    it, converged = 0, norm_b == 0.0
    if converged:
        x.zero_()
    while not converged and it < maxiter:
        r = b - op.matvec(x)
        beta = float(torch.linalg.vector_norm(r))
        if beta <= tol * norm_b:
            converged = True
            break
        V[0] = r / beta
        R = np.zeros((m, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = beta
        k = 0
        while k < m and it < maxiter:
            Vk = wide(V[:k + 1])
            op.matvec(Vk[k] if dinv is None else dinv * Vk[k], w)
            h1 = Vk @ w
            w -= h1 @ Vk
            h2 = Vk @ w
            w -= h2 @ Vk
            hh = float(torch.linalg.vector_norm(w))
            col = (h1 + h2).double().cpu().numpy()
            for i in range(k):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], -sn[i] * col[i] + cs[i] * col[i + 1]
            gamma = float(np.hypot(col[k], hh))
            cs[k], sn[k] = col[k] / gamma, hh / gamma
            R[:k, k], R[k, k] = col[:k], gamma
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            k += 1
            it += 1
            if hh == 0.0:
                break
            V[k] = w / hh
            if (it % check_every == 0 or it == maxiter) and abs(g[k]) <= tol * norm_b:
                break
        y = np.linalg.solve(np.triu(R[:k, :k]), g[:k])
        u = torch.from_numpy(y).to(device=b.device, dtype=b.dtype) @ wide(V[:k])
        x += u if dinv is None else dinv * u
    res = float(torch.linalg.vector_norm(b - op.matvec(x)))
    converged = converged or res <= tol * norm_b
    info = {"iterations": it, "residual": res, "relative_residual": res / norm_b if norm_b > 0 else 0.0, "converged": bool(converged)}
    return x, info


def minres(op, b, x0=None, tol=1e-10, maxiter=None, minv=None, check_every=1):
    """``A x = b`` for a square symmetric operator by preconditioned MINRES as a loop of torch operations: the recurrences of ``SparseOperator.minres``, without
    its guards — the baseline of scripts/minres_time.py and a second opinion in tests.  ``b``: a torch CUDA vector of ``rows`` elements; ``minv``: None or a positive diagonal.
    The scalars of the recurrence are 0-d tensors on the device: nothing is read on the host between checks.  Stops when ``phibar <= tol * sqrt(b.M^-1 b)`` (checked every
    ``check_every`` iterations: each check is one host sync) or after ``maxiter`` iterations (default ``2 * rows``).  Returns ``(x, info)`` with ``info = {"iterations",
    "residual", "relative_residual", "converged"}`` (``residual``: a recomputed ``|b - A x|``, relative to ``|b|``)."""
    import torch
    rows, cols = op.shape
    if rows != cols:
        raise ValueError("minres needs a square operator; this one is %d x %d" % (rows, cols))
    if b.numel() != rows:
        raise ValueError("b must have %d elements" % rows)
    maxiter = 2 * rows if maxiter is None else maxiter

    def vector():
        return torch.zeros(rows + 16, dtype=b.dtype, device=b.device)[:rows]

    x = vector()
    r1, r2, y, v, w, w2 = vector(), vector(), vector(), vector(), vector(), vector()
    r2.copy_(b)
    if x0 is not None:
        x.copy_(x0)
        r2 -= op.matvec(x)
    z = r2 if minv is None else minv * r2
    beta = torch.dot(r2, z).sqrt()
    bnorm = float(torch.dot(b, b if minv is None else minv * b).sqrt())
    zero = torch.zeros((), dtype=b.dtype, device=b.device)
    oldb, dbar, epsln, phibar, cs, sn = zero, zero, zero, beta, zero - 1, zero
    it, converged = 0, float(phibar) <= tol * bnorm
    while not converged and it < maxiter:
        torch.div(z, beta, out=v)
        op.matvec(v, y)
        if it > 0:
            y.addcmul_(r1, -(beta / oldb))
        alfa = torch.dot(v, y)
        y.addcmul_(r2, -(alfa / beta))
        r1, r2, y = r2, y, r1
        z = r2 if minv is None else minv * r2
        betan = torch.dot(r2, z).sqrt()
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        gamma = torch.hypot(gbar, betan)
        oldb, beta = beta, betan
        epsln, dbar = sn * beta, -cs * beta
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w, w2 = w2, w                               # w' over the older of the two
        w.mul_(-oldeps / gamma).addcmul_(w2, -delta / gamma).addcmul_(v, 1 / gamma)
        x.addcmul_(w, phi)
        it += 1
        if it % check_every == 0 or it == maxiter:
            converged = float(phibar) <= tol * bnorm
    res, norm_b = float(torch.linalg.vector_norm(b - op.matvec(x))), float(torch.linalg.vector_norm(b))
    info = {"iterations": it, "residual": res, "relative_residual": res / norm_b if norm_b > 0 else 0.0, "converged": bool(converged)}
    return x, info


def cgls(op, b, x0=None, tol=1e-12, maxiter=None, check_every=1):
    """Least squares ``min ||A x - b||_2`` by CGLS (conjugate gradients on the normal equations, never forming A^T A): one ``A p`` and one ``A^T r`` per iteration.
    ``b``: a torch CUDA vector of ``rows`` elements.  Stops when ``||A^T r|| <= tol * ||A^T b||`` (checked every ``check_every`` iterations: each check is one host sync) or after
    ``maxiter`` iterations (default ``2 * cols``).  Returns ``(x, info)`` with ``info = {"iterations", "normal_residual", "residual", "converged"}``."""
    import torch
    rows, cols = op.shape
    if b.numel() != rows:
        raise ValueError("b must have %d elements" % rows)
    maxiter = 2 * cols if maxiter is None else maxiter
    x = torch.zeros(cols, dtype=b.dtype, device=b.device) if x0 is None else x0.clone()
    r = b.clone()
    if x0 is not None:
        r -= op.matvec(x)
    s = op.rmatvec(r)
    norm_atb = float(torch.linalg.vector_norm(op.rmatvec(b)))
    p = s.clone()
    gamma = torch.dot(s, s)
    q = torch.empty(rows + 16, dtype=b.dtype, device=b.device)[:rows]
    it, converged = 0, float(gamma.sqrt()) <= tol * norm_atb
    while not converged and it < maxiter:
        op.matvec(p, q)
        alpha = gamma / torch.dot(q, q)
        x.add_(alpha * p)
        r.sub_(alpha * q)
        op.rmatvec(r, s)
        gamma_new = torch.dot(s, s)
        p.mul_(gamma_new / gamma).add_(s)
        gamma = gamma_new
        it += 1
        if it % check_every == 0 or it == maxiter:
            converged = float(gamma.sqrt()) <= tol * norm_atb
    info = {"iterations": it, "normal_residual": float(gamma.sqrt()), "residual": float(torch.linalg.vector_norm(b - op.matvec(x))), "converged": bool(converged)}
    return x, info
