"""The right-hand sides of tests/test_cg_multi_cpu.py and tests/test_gpu_cg_multi.py (a helper, not a test): eight columns that stop at different iterations, one of them zero,
one the unit vector, two scaled by 1e3 and 1e-3 (the scalars are per column: a scale must not leak)."""
import numpy as np

import cg_mirror as M


def columns(n, A):
    """B of shape (n, 8), float64: column j as the table in tests/test_cg_multi_cpu.py lists it.  ``A``: scipy CSR in float64."""
    def U(seed):
        return np.random.default_rng(seed).uniform(-1, 1, n)

    e = np.zeros(n)
    e[n // 2] = 1.0
    cols = [M.rhs(n), A @ np.ones(n), np.zeros(n), 1e3 * U(4), A @ np.linspace(0, 1, n), e, 1e-3 * U(5), U(6)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def system(name, dtype):
    """(n, rp, ci, values in dtype, B (n, 8) in dtype) of a named input of cg_mirror.problem."""
    dt = np.dtype(dtype)
    n, rp, ci, v = M.problem(name)
    B = columns(n, M.scipy_csr(n, rp, ci, v))
    return n, rp, ci, v.astype(dt), np.ascontiguousarray(B.astype(dt))
