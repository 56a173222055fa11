"""Host-side mirror of the reference's driver interface (same names and argument meaning as
reference src/main.cu calls them), over the C ABI of ``include/tilespmv.h``.

    tm = Tile_create(rowA, colA, nnzA, rowptr, colidx, vals)        # src/csr2tile.h:629
    sched = tilespmv_cpu(tm, rowA, colA, nnzA, rowptr, colidx, vals, x, y_golden)   # src/tilespmv_cpu.h:3
    y = call_tilespmv_hip("A.mtx", tm, sched, rowA, colA, nnzA, rowptr, colidx, vals, x)  # src/tilespmv_cuda.h:794
    plan = Plan(tm, rowA, colA, nnzA); plan.spmv(x_dev_ptr, y_dev_ptr)            # resident-plan API (new)
"""
import ctypes as C

import numpy as np

from . import _lib
from .tile_matrix import to_dict  # noqa: F401  (re-export)

_I, _U = _lib._I, _lib._U

COO_AUTO, COO_IN_TILE, COO_FALLBACK = 0, 1, 2
DENSE_AUTO, DENSE_MFMA, DENSE_VALU = 0, 1, 2
KERNEL_AUTO, KERNEL_DIRECT, KERNEL_STREAM = 0, 1, 2
CREATE_HYB, CREATE_QUIET, CREATE_CDNA4, CREATE_VALUE_MAP = 1, 2, 4, 8
CREATE_TRANSPOSE = 16   # the tiled matrix / plan of A^T, built from A's CSR (include/tilespmv.h)
ERR_NO_VALUE_MAP = -4   # tilespmv_plan_update_values on a plan without a value map


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _take(lib, ptr, n, dtype):
    if not ptr:
        return np.zeros(0, dtype=dtype)
    addr = C.cast(ptr, C.c_void_p).value
    out = np.frombuffer((C.c_char * (max(n, 0) * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype, count=max(n, 0)).copy()
    lib._free(C.cast(ptr, C.c_void_p))
    return out


def _csr(lib, rowptr, colidx, vals):
    return (np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(colidx, dtype=np.int32),
            np.ascontiguousarray(vals, dtype=lib._dtype))


def Tile_create(rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, dtype=None, hyb=False, quiet=True, cdna4=False, transpose=False):
    """``transpose=True`` (TILESPMV_CREATE_TRANSPOSE): the tiled matrix of A^T (colA x rowA), transposed on the host; the arguments still describe A."""
    dtype = np.dtype(dtype or np.asarray(csrValA).dtype)
    lib = _lib.load(dtype)
    rp, ci, v = _csr(lib, csrRowPtrA, csrColIdxA, csrValA)
    if transpose:
        _check_csr(rowA, colA, rp, ci)
    tm = lib._TM()
    flags = (CREATE_HYB if hyb else 0) | (CREATE_QUIET if quiet else 0) | (CREATE_CDNA4 if cdna4 else 0) | (CREATE_TRANSPOSE if transpose else 0)
    lib.Tile_create_ex(C.byref(tm), rowA, colA, nnzA, _p(rp, C.c_int), _p(ci, C.c_int), _p(v, lib._vt), flags)
    tm._keep = (rp, ci, v)
    tm._lib = lib
    return tm


def Tile_create_device(rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, dtype=None, quiet=True, cdna4=False, hyb=False, transpose=False):
    """``Tile_create`` computed on the GPU (hip_tile_create.hip): the CSR arrays go up, the tiled matrix comes back, byte for byte what ``Tile_create`` builds
    (``hyb=True``: with the reference's dormant HYB rule switched on, as ``Tile_create(hyb=True)``).  No CPU fallback: raises when no device is visible (rc -1).
    ``transpose=True``: the tiled matrix of A^T, transposed on the device — byte for byte ``Tile_create(transpose=True)``."""
    dtype = np.dtype(dtype or np.asarray(csrValA).dtype)
    lib = _lib.load(dtype)
    rp, ci, v = _csr(lib, csrRowPtrA, csrColIdxA, csrValA)
    tm = lib._TM()
    flags = (CREATE_QUIET if quiet else 0) | (CREATE_CDNA4 if cdna4 else 0) | (CREATE_HYB if hyb else 0) | (CREATE_TRANSPOSE if transpose else 0)
    rc = lib.Tile_create_device(C.byref(tm), rowA, colA, nnzA, _p(rp, C.c_int), _p(ci, C.c_int), _p(v, lib._vt), flags)
    if rc != 0:
        raise RuntimeError("Tile_create_device failed (%d): no usable HIP device / extension, or offsets beyond int32" % rc)
    tm._keep = (rp, ci, v)
    tm._lib = lib
    return tm


def _check_csr(rows, cols, rp, ci):
    if rows < 0 or cols < 0 or len(rp) < rows + 1:
        raise ValueError("not a %d x %d CSR: the row pointer needs %d entries" % (rows, cols, rows + 1))
    lo, hi = int(rp[0]), int(rp[rows])
    if lo < 0 or hi < lo or len(ci) < hi or (rows and np.any(np.diff(rp[:rows + 1]) < 0)):
        raise ValueError("not a %d x %d CSR: the row pointer decreases or points past the column indices" % (rows, cols))
    if hi > lo and (int(ci[lo:hi].min()) < 0 or int(ci[lo:hi].max()) >= cols):
        raise ValueError("not a %d x %d CSR: a column index outside [0, %d)" % (rows, cols, cols))


def csr_transpose(rows, cols, rp, ci, v=None, dtype=None):
    """A^T of a ``rows x cols`` CSR (``tilespmv_csr_transpose``, host, threaded): ``(rpT, ciT, vT, srcT)``, the entries of A in CSR order stably sorted by column —
    ``srcT[k]`` is the position of entry k of A^T in the caller's arrays (``rp[0] != 0`` allowed: a row block of a larger CSR).  ``vT`` is ``None`` when ``v`` is."""
    dtype = np.dtype(dtype if dtype is not None else (np.asarray(v).dtype if v is not None else np.float64))
    lib = _lib.load(dtype)
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    _check_csr(rows, cols, rp, ci)
    nnz = int(rp[rows]) - int(rp[0])
    vv = None if v is None else np.ascontiguousarray(v, dtype=lib._dtype)
    if vv is not None and len(vv) < int(rp[rows]):
        raise ValueError("csr_transpose: %d values for %d positions" % (len(vv), int(rp[rows])))
    rpT, ciT, srcT = np.zeros(cols + 1, np.int32), np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.int32)
    vT = None if vv is None else np.zeros(max(nnz, 1), lib._dtype)
    rc = lib.tilespmv_csr_transpose(rows, cols, _p(rp, C.c_int), _p(ci, C.c_int), None if vv is None else _p(vv, lib._vt), _p(rpT, C.c_int), _p(ciT, C.c_int),
                                    None if vT is None else _p(vT, lib._vt), _p(srcT, C.c_int))
    if rc != 0:
        raise ValueError("tilespmv_csr_transpose failed (%d): not a valid CSR" % rc)
    return rpT, ciT[:nnz], None if vT is None else vT[:nnz], srcT[:nnz]


def csr_transpose_device(rows, cols, d_rp, d_ci, d_v, d_rpT, d_ciT, d_vT=None, d_srcT=None, dtype=np.float64, stream=0):
    """``tilespmv_csr_transpose_device``: the same on DEVICE arrays (addresses, as ``Plan.from_device_csr`` takes them; ``d_rpT`` has cols + 1 int32 elements, ``d_ciT`` /
    ``d_vT`` / ``d_srcT`` one per nonzero; ``d_v`` / ``d_vT`` / ``d_srcT`` may be 0 / None).  Allocates scratch and synchronises ``stream``: not for graph capture."""
    lib = _lib.load(dtype)
    rc = lib.tilespmv_csr_transpose_device(rows, cols, C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v or None), C.c_void_p(d_rpT), C.c_void_p(d_ciT),
                                           C.c_void_p(d_vT or None), C.c_void_p(d_srcT or None), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("tilespmv_csr_transpose_device failed (hipError %d): bad argument, a column index outside [0, cols), or no usable device" % rc)


def Tile_destroy(tm):
    tm._lib.Tile_destroy(C.byref(tm))


def tilespmv_cpu(tm, rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, x, y_golden):
    lib = tm._lib
    rp, ci, v = _csr(lib, csrRowPtrA, csrColIdxA, csrValA)
    x = np.ascontiguousarray(x, dtype=lib._dtype)
    yg = np.ascontiguousarray(y_golden, dtype=lib._dtype)
    n = tm.tilenum
    p1 = np.zeros(max(n, 1), dtype=np.int32); p2 = np.zeros(max(n, 1), dtype=np.int32)
    y = np.zeros(rowA + 16, dtype=lib._dtype)
    nb = C.c_int(0); a, b, c = _U(), _I(), _I()
    lib.tilespmv_cpu(C.byref(tm), _p(p1, C.c_int), _p(p2, C.c_int), C.byref(nb), C.byref(a), C.byref(b), C.byref(c),
                     rowA, colA, nnzA, _p(rp, C.c_int), _p(ci, C.c_int), _p(v, lib._vt), _p(x, lib._vt), _p(y, lib._vt), _p(yg, lib._vt))
    k = nb.value
    return {"y": y[:rowA].copy(), "ptroffset1": p1[:n].copy(), "ptroffset2": p2[:n].copy(), "rowblkblock": k,
            "blkcoostylerowidx": _take(lib, a, k, np.uint32), "blkcoostylerowidx_colstart": _take(lib, b, k, np.int32),
            "blkcoostylerowidx_colstop": _take(lib, c, k, np.int32),
            "errcount": int(np.count_nonzero(y[:rowA] != yg[:rowA]))}


def mmio_allinone(filename, dtype=np.float64, cache=None):
    """``cache``: path of the binary CSR cache kept beside the text (``mmio_allinone_cached``): read when it is fresh for
    ``filename`` (size and mtime), otherwise the text is parsed and the cache (re)written.  The result then carries
    ``from_cache`` (1 read, 0 parsed and saved, -1 parsed, cache not writable)."""
    lib = _lib.load(dtype)
    VP = C.POINTER(lib._vt)
    m, n, nnz, sym, hit = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(0)
    rp, ci, cv = _I(), _I(), VP()
    if cache is None:
        rc = lib.mmio_allinone(C.byref(m), C.byref(n), C.byref(nnz), C.byref(sym), C.byref(rp), C.byref(ci), C.byref(cv), filename.encode())
    else:
        rc = lib.mmio_allinone_cached(C.byref(m), C.byref(n), C.byref(nnz), C.byref(sym), C.byref(rp), C.byref(ci), C.byref(cv), filename.encode(),
                                      cache.encode(), C.byref(hit))
    if rc != 0:
        return {"rc": rc}
    out = {"rc": 0, "m": m.value, "n": n.value, "nnz": nnz.value, "sym": sym.value,
           "rowptr": _take(lib, rp, m.value + 1, np.int32), "colidx": _take(lib, ci, nnz.value, np.int32),
           "val": _take(lib, cv, nnz.value, lib._dtype)}
    if cache is not None:
        out["from_cache"] = hit.value
    return out


def mtx_write(path, rows, cols, rowptr, colidx, vals=None, dtype=np.float64):
    """General coordinate Matrix Market file in CSR order, written by the library's threaded writer (GBs in seconds);
    ``vals=None`` writes a pattern file."""
    lib = _lib.load(dtype)
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colidx, dtype=np.int32)
    v = None if vals is None else np.ascontiguousarray(vals, dtype=lib._dtype)
    rc = lib.tilespmv_mtx_write(path.encode(), rows, cols, len(ci), _p(rp, C.c_int), _p(ci, C.c_int), None if v is None else _p(v, lib._vt))
    if rc != 0:
        raise OSError("tilespmv_mtx_write(%s) failed: %d" % (path, rc))


Y_SHARDED, Y_ALLGATHER, Y_ALLREDUCE = 0, 1, 2


def call_tilespmv_hip(filename, tm, sched, rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, x, alpha=1.0,
                      device_ids=None, y_combine_mode=Y_ALLGATHER):
    """Host pointers in, y (host) out — the reference's one-shot GPU entry (timing + results.csv included).
    With ``device_ids`` (a list, ids may repeat) the multi-device form ``call_tilespmv_hip_multi`` runs instead."""
    lib = tm._lib
    rp, ci, v = _csr(lib, csrRowPtrA, csrColIdxA, csrValA)
    x = np.ascontiguousarray(x, dtype=lib._dtype)
    y = np.zeros(rowA + 16, dtype=lib._dtype)
    yg = np.zeros(rowA + 16, dtype=lib._dtype)
    p1 = np.ascontiguousarray(sched["ptroffset1"], dtype=np.int32) if sched else np.zeros(max(tm.tilenum, 1), np.int32)
    p2 = np.ascontiguousarray(sched["ptroffset2"], dtype=np.int32) if sched else np.zeros(max(tm.tilenum, 1), np.int32)
    ri = np.ascontiguousarray(sched["blkcoostylerowidx"], dtype=np.uint32) if sched else np.zeros(1, np.uint32)
    c0 = np.ascontiguousarray(sched["blkcoostylerowidx_colstart"], dtype=np.int32) if sched else np.zeros(1, np.int32)
    c1 = np.ascontiguousarray(sched["blkcoostylerowidx_colstop"], dtype=np.int32) if sched else np.zeros(1, np.int32)
    args = (filename.encode(), C.byref(tm), _p(p1, C.c_int), _p(p2, C.c_int), int(sched["rowblkblock"]) if sched else 0,
            _p(ri, C.c_uint), _p(c0, C.c_int), _p(c1, C.c_int), rowA, colA, nnzA, _p(rp, C.c_int), _p(ci, C.c_int),
            _p(v, lib._vt), alpha, _p(x, lib._vt), _p(y, lib._vt), _p(yg, lib._vt))
    if device_ids is None:
        lib.call_tilespmv_hip(*args)
    else:
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        rc = lib.call_tilespmv_hip_multi(*args, len(ids), _p(ids, C.c_int), int(y_combine_mode))
        if rc != 0:
            raise RuntimeError("call_tilespmv_hip_multi failed (%d): see stderr" % rc)
    return y[:rowA].copy()


def matrix_save(tm, rowA, colA, nnzA, path):
    rc = tm._lib.tilespmv_matrix_save(C.byref(tm), rowA, colA, nnzA, path.encode())
    if rc != 0:
        raise OSError("tilespmv_matrix_save(%s) failed: %d" % (path, rc))


def matrix_load(path, dtype=np.float64):
    """Returns (Tile_matrix, rowA, colA, nnzA) read from a cache file written by matrix_save."""
    lib = _lib.load(dtype)
    tm = lib._TM()
    r, c, z = C.c_int(), C.c_int(), C.c_int()
    rc = lib.tilespmv_matrix_load(C.byref(tm), C.byref(r), C.byref(c), C.byref(z), path.encode())
    if rc != 0:
        raise OSError("tilespmv_matrix_load(%s) failed: %d" % (path, rc))
    tm._lib = lib
    return tm, r.value, c.value, z.value


def partition_tilerows(tm, nparts):
    b = np.zeros(nparts + 1, dtype=np.int32)
    tm._lib.tilespmv_partition_tilerows(C.byref(tm), nparts, _p(b, C.c_int))
    return b


def reorder_rcm(n, rowptr, colidx, dtype=np.float64):
    """Reverse Cuthill-McKee on the symmetrised pattern of the leading n x n block (host; tilespmv_reorder_rcm): ``perm[new] = old``."""
    lib = _lib.load(dtype)
    rp, ci = np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(colidx, dtype=np.int32)
    perm = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib.tilespmv_reorder_rcm(n, _p(rp, C.c_int), _p(ci, C.c_int), _p(perm, C.c_int))
    if rc != 0:
        raise RuntimeError("tilespmv_reorder_rcm failed (%d)" % rc)
    return perm[:n]


def csr_permute(n, rowptr, colidx, vals, perm, dtype=None):
    """``B = P A P^T`` for ``perm[new] = old`` (tilespmv_csr_permute): rows and the columns < n are renumbered, columns >= n (halo) stay, every row comes out in ascending column order."""
    dtype = np.dtype(dtype if dtype is not None else np.asarray(vals).dtype)
    lib = _lib.load(dtype)
    rp, ci, v = _csr(lib, rowptr, colidx, vals)
    pm = np.ascontiguousarray(perm, dtype=np.int32)
    nnz = int(rp[n])
    orp, oci, ov = np.zeros(n + 1, dtype=np.int32), np.zeros(max(nnz, 1), dtype=np.int32), np.zeros(max(nnz, 1), dtype=dtype)
    rc = lib.tilespmv_csr_permute(n, _p(rp, C.c_int), _p(ci, C.c_int), _p(v, lib._vt), _p(pm, C.c_int), _p(orp, C.c_int), _p(oci, C.c_int), _p(ov, lib._vt))
    if rc != 0:
        raise ValueError("tilespmv_csr_permute: perm is not a permutation of 0 .. n - 1 (%d)" % rc)
    return orp, oci[:nnz], ov[:nnz]


def csr_bandwidth(n, rowptr, colidx, dtype=np.float64):
    lib = _lib.load(dtype)
    rp, ci = np.ascontiguousarray(rowptr, dtype=np.int32), np.ascontiguousarray(colidx, dtype=np.int32)
    return int(lib.tilespmv_csr_bandwidth(n, _p(rp, C.c_int), _p(ci, C.c_int)))


def permute_vector(d_in, d_out, d_perm, n, scatter=False, stream=0, dtype=np.float64):
    """Device vectors between the caller's numbering and a reordered plan's: gather ``out[i] = in[perm[i]]`` (into plan order) or scatter ``out[perm[i]] = in[i]`` (back)."""
    rc = _lib.load(dtype).tilespmv_permute_vector(d_in, d_out, d_perm, n, 1 if scatter else 0, stream)
    if rc != 0:
        raise RuntimeError("tilespmv_permute_vector failed (hipError %d)" % rc)


def plan_layout_digest(tm, rowA, colA, nnzA, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, **knobs):
    """Host-only build of the plan layout (no GPU needed): returns (FNV-1a-64 digest of every stream, plan facts)."""
    opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, False, **knobs)
    d = C.c_ulonglong(0)
    out = (C.c_longlong * len(_lib.INFO_NAMES))()
    rc = tm._lib.tilespmv_plan_layout_digest(C.byref(tm), rowA, colA, nnzA, C.byref(opts), C.byref(d), out)
    if rc != 0:
        raise RuntimeError("tilespmv_plan_layout_digest failed (%d)" % rc)
    return d.value, {k: int(out[i]) for i, k in enumerate(_lib.INFO_NAMES)}


def plan_layout_unit_deep(tm, rowA, colA, nnzA, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, **knobs):
    """Host-only: what ``Plan.unit_deep()`` of the plan of this matrix and these options would report (tilespmv_plan_layout_unit_deep)."""
    opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, False, **knobs)
    rc = tm._lib.tilespmv_plan_layout_unit_deep(C.byref(tm), rowA, colA, nnzA, C.byref(opts))
    if rc < 0:
        raise RuntimeError("tilespmv_plan_layout_unit_deep failed (%d)" % rc)
    return int(rc)


STAGE_NAMES = ["count", "choose", "cut", "emit", "order", "encode", "entries", "finish"]


def plan_layout_stages(tm, rowA, colA, nnzA, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, **knobs):
    """Host-only build of the unit-stream layout, one digest per builder stage (``STAGE_NAMES``) + the plan facts."""
    opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, False, **knobs)
    st = (C.c_ulonglong * len(STAGE_NAMES))()
    out = (C.c_longlong * len(_lib.INFO_NAMES))()
    rc = tm._lib.tilespmv_plan_layout_stages(C.byref(tm), rowA, colA, nnzA, C.byref(opts), st, out)
    if rc != 0:
        raise RuntimeError("tilespmv_plan_layout_stages failed (%d)" % rc)
    return {k: int(st[i]) for i, k in enumerate(STAGE_NAMES)}, {k: int(out[i]) for i, k in enumerate(_lib.INFO_NAMES)}


class Plan:
    """Device-resident tiled matrix (or one tile-row shard of it)."""

    def __init__(self, tm, rowA, colA, nnzA, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, autotune=False, **knobs):
        """``knobs``: the tuning fields of ``tilespmv_plan_options`` (``entry_mode=2, strip_cost=800, xcd_chunk=8, ...``;
        ``_lib.KNOB_NAMES``).  An unset knob falls back to its TILESPMV_* environment variable, then to the built-in default."""
        self.lib = tm._lib
        self.rowA, self.colA, self.nnzA = rowA, colA, nnzA
        self.shape = (rowA, colA)
        opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, autotune, **knobs)
        h = C.c_void_p()
        rc = self.lib.tilespmv_plan_create(C.byref(h), C.byref(tm), rowA, colA, nnzA, C.byref(opts))
        if rc != 0 or not h:
            raise RuntimeError("tilespmv_plan_create failed (%d): no usable HIP device / extension" % rc)
        self.h = h

    @classmethod
    def from_csr(cls, rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, dtype=None, cdna4=False, hyb=False, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, autotune=False,
                 value_map=False, transpose=False, **knobs):
        """``tilespmv_plan_create_from_csr``: the tiled matrix and the plan's streams are built on the device; only the CSR arrays cross the bus.
        Raises ``NotImplementedError`` for the options that have no device path (rc -4: first-generation kernel, CSR fallback, csr_split=0).  ``autotune=True``: every candidate is built from the one device-resident tiled matrix.
        ``value_map=True`` (TILESPMV_CREATE_VALUE_MAP): the plan keeps a value map, so that ``update_values`` can give it new values of the same pattern.
        ``transpose=True`` (TILESPMV_CREATE_TRANSPOSE): the plan of A^T, transposed on the device — ``spmv`` computes y[0 .. colA) = A^T x with x of rowA elements
        (``shape`` = (colA, rowA)); tilerow_begin / tilerow_end count tile-rows of A^T; with ``value_map`` the map indexes A's value array."""
        dtype = np.dtype(dtype or np.asarray(csrValA).dtype)
        lib = _lib.load(dtype)
        rp, ci, v = _csr(lib, csrRowPtrA, csrColIdxA, csrValA)
        if transpose:
            _check_csr(rowA, colA, rp, ci)
        self = cls.__new__(cls)
        self.lib = lib
        self.rowA, self.colA, self.nnzA = rowA, colA, nnzA
        self.shape = (colA, rowA) if transpose else (rowA, colA)
        opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, autotune, **knobs)
        h = C.c_void_p()
        rc = lib.tilespmv_plan_create_from_csr(C.byref(h), rowA, colA, nnzA, _p(rp, C.c_int), _p(ci, C.c_int), _p(v, lib._vt), CREATE_QUIET | (CREATE_CDNA4 if cdna4 else 0) | (CREATE_HYB if hyb else 0) | (CREATE_VALUE_MAP if value_map else 0) | (CREATE_TRANSPOSE if transpose else 0), C.byref(opts))
        if rc == -4:
            raise NotImplementedError("tilespmv_plan_create_from_csr: these options have no device path")
        if rc != 0 or not h:
            raise RuntimeError("tilespmv_plan_create_from_csr failed (%d)" % rc)
        self.h = h
        return self

    @classmethod
    def from_device_csr(cls, rowA, colA, nnzA, d_rowptr, d_colidx, d_vals, dtype, cdna4=False, coo_mode=COO_AUTO, dense_mode=DENSE_AUTO, kernel=0, tilerow_begin=0, tilerow_end=0, value_map=False, transpose=False, **knobs):
        """``tilespmv_plan_create_from_device_csr``: like ``from_csr`` with the CSR arrays already in device memory — ``d_rowptr`` / ``d_colidx`` (int32) and ``d_vals`` are device
        ADDRESSES (e.g. ``tensor.data_ptr()`` of the crow / col / values tensors of a torch CSR tensor cast to int32); borrowed for the call.  ``transpose=True``: the plan of A^T
        (as in ``from_csr``)."""
        dtype = np.dtype(dtype)
        lib = _lib.load(dtype)
        self = cls.__new__(cls)
        self.lib = lib
        self.rowA, self.colA, self.nnzA = rowA, colA, nnzA
        self.shape = (colA, rowA) if transpose else (rowA, colA)
        opts = _lib.PlanOptions(coo_mode, dense_mode, kernel, tilerow_begin, tilerow_end, False, **knobs)
        h = C.c_void_p()
        rc = lib.tilespmv_plan_create_from_device_csr(C.byref(h), rowA, colA, nnzA, C.c_void_p(d_rowptr), C.c_void_p(d_colidx), C.c_void_p(d_vals), CREATE_QUIET | (CREATE_CDNA4 if cdna4 else 0) | (CREATE_VALUE_MAP if value_map else 0) | (CREATE_TRANSPOSE if transpose else 0), C.byref(opts))
        if rc == -4:
            raise NotImplementedError("tilespmv_plan_create_from_device_csr: these options have no device path")
        if rc != 0 or not h:
            raise RuntimeError("tilespmv_plan_create_from_device_csr failed (%d)" % rc)
        self.h = h
        return self

    def update_values(self, d_vals, stream=0):
        """``tilespmv_plan_update_values``: every value of the plan rewritten from ``d_vals`` (device ADDRESS of the CSR value array the plan was created from, same pattern,
        new values), asynchronously on ``stream``.  The plan must have been created with ``value_map=True``."""
        rc = self.lib.tilespmv_plan_update_values(self.h, C.c_void_p(d_vals), C.c_void_p(stream))
        if rc == ERR_NO_VALUE_MAP:
            raise RuntimeError("tilespmv_plan_update_values: the plan has no value map (create it with value_map=True)")
        if rc != 0:
            raise RuntimeError("tilespmv_plan_update_values: HIP error %d" % rc)

    def spmv(self, d_x, d_y, stream=0):
        rc = self.lib.tilespmv_plan_spmv(self.h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("tilespmv_plan_spmv: HIP error %d" % rc)

    def spmv_n(self, d_x, d_y, stream=0, count=1):
        rc = self.lib.tilespmv_plan_spmv_n(self.h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(stream), count)
        if rc != 0:
            raise RuntimeError("tilespmv_plan_spmv_n: HIP error %d" % rc)

    def spmm(self, d_X, d_Y, nvec, stream=0):
        """Y[rows][nvec] = A X[cols][nvec], row-major device arrays (16-B aligned), nvec in {1, 2, 4, 8}."""
        rc = self.lib.tilespmv_plan_spmm(self.h, C.c_void_p(d_X), C.c_void_p(d_Y), nvec, C.c_void_p(stream))
        if rc == 801:
            raise NotImplementedError("tilespmv_plan_spmm: this plan uses the CSR fallback / whole-tile passes (no multi-vector kernel)")
        if rc != 0:
            raise RuntimeError("tilespmv_plan_spmm: HIP error %d" % rc)

    def time_spmm(self, d_X, d_Y, nvec, stream=0, warmup=10, reps=50):
        ms = self.lib.tilespmv_plan_time_spmm(self.h, C.c_void_p(d_X), C.c_void_p(d_Y), nvec, C.c_void_p(stream), warmup, reps)
        if ms < 0:
            raise RuntimeError("tilespmv_plan_time_spmm failed")
        return ms

    def time(self, d_x, d_y, stream=0, warmup=10, reps=50):
        ms = self.lib.tilespmv_plan_time(self.h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(stream), warmup, reps)
        if ms < 0:
            raise RuntimeError("tilespmv_plan_time failed")
        return ms

    def time_reference_style(self, d_x, d_y, stream=0, reps=100):
        """Mean ms per SpMV by the reference's protocol: wall clock around one launch + synchronize (a C loop)."""
        ms = self.lib.tilespmv_plan_time_reference_style(self.h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(stream), reps)
        if ms < 0:
            raise RuntimeError("tilespmv_plan_time_reference_style failed")
        return ms

    def reserve_spmm(self, nvec):
        rc = self.lib.tilespmv_plan_reserve_spmm(self.h, nvec)
        if rc != 0:
            raise RuntimeError("tilespmv_plan_reserve_spmm: HIP error %d" % rc)

    def info(self):
        out = (C.c_longlong * len(_lib.INFO_NAMES))()
        self.lib.tilespmv_plan_info(self.h, out)
        return {k: int(out[i]) for i, k in enumerate(_lib.INFO_NAMES)}

    def strip_stride(self):
        """S: tile-rows between the consecutive tile-rows of one strip of the unit stream, 1 = consecutive (tilespmv_plan_strip_stride; TILESPMV_STRIP_SWEEP)."""
        return int(self.lib.tilespmv_plan_strip_stride(self.h))

    def unit_deep(self):
        """0, or the batches of x gathers the plan's unit launch keeps in flight per wavefront: the deep unit kernel (tilespmv_plan_unit_deep; TILESPMV_UNIT_DEEP)."""
        return int(self.lib.tilespmv_plan_unit_deep(self.h))

    def stream_digests(self):
        """{member offset: (bytes, FNV-1a-64)} of every stream of the plan, read back from the device (test / audit aid)."""
        out = (C.c_ulonglong * (3 * 64))()
        n = self.lib.tilespmv_plan_stream_digests(self.h, out, 64)
        if n < 0 or n > 64:
            raise RuntimeError("tilespmv_plan_stream_digests failed (%d)" % n)
        return {int(out[3 * i]): (int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(n)}

    def close(self):
        if getattr(self, "h", None):
            self.lib.tilespmv_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CG_RUNNING, CG_CONVERGED, CG_MAXITER, CG_BREAKDOWN = 0, 1, 2, 3
CG_STATUS_NAMES = ["running", "converged", "maxiter", "breakdown"]
HIP_ERROR_INVALID_VALUE = 1


class _Solver:
    """What the solver wrappers share: the handle ``h`` of library ``lib``, the translation of return codes, and the end of the handle's life.  A subclass names its destroy
    entry point (``_destroy``) and says what hipErrorInvalidValue means for it (``_hint``)."""

    @classmethod
    def _check(cls, rc, what):
        if rc == HIP_ERROR_INVALID_VALUE:
            raise ValueError("%s: hipErrorInvalidValue (%s)" % (what, cls._hint))
        if rc != 0:
            raise RuntimeError("%s: HIP error %d" % (what, rc))

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self._destroy)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_diagonal_device(rows, d_rp, d_ci, d_v, d_out, invert=False, stream=0, dtype=np.float64):
    """``tilespmv_csr_diagonal_device``: ``d_out[i]`` = the sum of the stored entries (i, i) of a device CSR (addresses, as ``Plan.from_device_csr`` takes them); ``invert=True``: its
    inverse, 1 where it is 0 — the ``d_dinv`` of ``CG``.  Asynchronous on ``stream``."""
    lib = _lib.load(dtype)
    rc = lib.tilespmv_csr_diagonal_device(rows, C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v), C.c_void_p(d_out), 1 if invert else 0, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("tilespmv_csr_diagonal_device failed (hipError %d): bad argument, or no usable device" % rc)


class BlockJacobi(_Solver):
    """``tilespmv_block_jacobi``: M^-1 for M = the block diagonal of A in consecutive blocks of ``block_size`` rows (1 .. 16; the last block may be short), held on the device and
    applied by one streaming kernel (include/tilespmv.h) — the ``block`` of ``CG`` and ``BiCGStab``, one block per node of an FEM matrix with ``block_size``
    unknowns per node.  All arguments of the methods are device ADDRESSES; vectors have ``rows`` elements and are 16-byte aligned.  Raises ``ValueError`` where the library returns
    hipErrorInvalidValue."""

    _destroy = "tilespmv_block_jacobi_destroy"
    _hint = "rows > 0, 1 <= block_size <= 16; vectors distinct and 16-byte aligned"

    def __init__(self, rows, block_size, dtype=np.float64):
        self.lib = _lib.load(dtype)
        self.rows, self.block_size, self.dtype = int(rows), int(block_size), np.dtype(dtype)
        h = C.c_void_p()
        self._check(self.lib.tilespmv_block_jacobi_create(C.byref(h), self.rows, self.block_size), "tilespmv_block_jacobi_create")
        self.h = h

    def update(self, d_rp, d_ci, d_v, stream=0):
        """Extract the blocks from a device CSR and invert them; asynchronous, capturable.  After ``Plan.update_values``: the same call again."""
        self._check(self.lib.tilespmv_block_jacobi_update(self.h, C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v), C.c_void_p(stream)), "tilespmv_block_jacobi_update")

    def apply(self, d_r, d_z, stream=0, d_partials=None):
        """z = M^-1 r (z and r distinct); asynchronous, capturable.  ``d_partials``: also the ``info()["dot_partials"]`` partial sums of r.z, doubles."""
        if d_partials is None:
            rc = self.lib.tilespmv_block_jacobi_apply(self.h, C.c_void_p(d_r), C.c_void_p(d_z), C.c_void_p(stream))
        else:
            rc = self.lib.tilespmv_block_jacobi_apply_dot(self.h, C.c_void_p(d_r), C.c_void_p(d_z), C.c_void_p(d_partials), C.c_void_p(stream))
        self._check(rc, "tilespmv_block_jacobi_apply")

    def info(self, stream=0):
        """Synchronises ``stream``; ``{"rows", "block_size", "blocks", "singular_blocks", "device_bytes", "dot_partials"}`` (singular_blocks: blocks the last update replaced by
        the identity)."""
        out = (C.c_longlong * len(_lib.BJ_INFO_NAMES))()
        self._check(self.lib.tilespmv_block_jacobi_info(self.h, C.c_void_p(stream), out), "tilespmv_block_jacobi_info")
        return dict(zip(_lib.BJ_INFO_NAMES, [int(v) for v in out]))


class FSAI(_Solver):
    """``tilespmv_fsai``: a factorised sparse approximate inverse of a symmetric positive definite A — a sparse lower-triangular G on the pattern of A's lower triangle with
    G A G^T ~ I, applied as z = G^T (G r) by two plans the object holds (include/tilespmv.h) — the ``fsai`` of ``CG``.  ``d_rp`` / ``d_ci`` (int32) / ``d_v`` are
    device ADDRESSES of a square CSR with strictly ascending columns in every row and a stored diagonal; only its lower triangle is read.  ``knobs``: the plan options handed to
    both plans (``deterministic=1, placement_tries=1, ...``; none: the defaults).  Vectors have ``rows`` elements and are 16-byte aligned.  Raises ``ValueError`` where the library
    returns hipErrorInvalidValue."""

    _destroy = "tilespmv_fsai_destroy"
    _hint = "a square CSR with strictly ascending columns and a stored diagonal in every row; vectors distinct and 16-byte aligned"

    def __init__(self, rows, nnz, d_rp, d_ci, d_v, dtype=np.float64, stream=0, **knobs):
        self.lib = _lib.load(dtype)
        self.rows, self.dtype = int(rows), np.dtype(dtype)
        opts = _lib.PlanOptions(**knobs) if knobs else None
        h = C.c_void_p()
        self._check(self.lib.tilespmv_fsai_create(C.byref(h), self.rows, int(nnz), C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v), C.byref(opts) if opts is not None else None,
                                                  C.c_void_p(stream)), "tilespmv_fsai_create")
        self.h = h

    def update(self, d_rp, d_ci, d_v, stream=0):
        """New values of A on the same pattern: G's values and both plans rewritten in place; asynchronous, capturable.  After ``Plan.update_values``: this call."""
        self._check(self.lib.tilespmv_fsai_update(self.h, C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v), C.c_void_p(stream)), "tilespmv_fsai_update")

    def apply(self, d_r, d_z, stream=0, d_partials=None):
        """z = G^T (G r) (z and r distinct); asynchronous, capturable.  ``d_partials``: also the ``info()["dot_partials"]`` partial sums of r.z, doubles."""
        if d_partials is None:
            rc = self.lib.tilespmv_fsai_apply(self.h, C.c_void_p(d_r), C.c_void_p(d_z), C.c_void_p(stream))
        else:
            rc = self.lib.tilespmv_fsai_apply_dot(self.h, C.c_void_p(d_r), C.c_void_p(d_z), C.c_void_p(d_partials), C.c_void_p(stream))
        self._check(rc, "tilespmv_fsai_apply")

    def factor(self, stream=0):
        """Synchronises ``stream``; G as host copies ``(rowptr int32 [rows + 1], colidx int32 [nnz], values [nnz] of the value type)``, numpy arrays."""
        rp, ci, v, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        self._check(self.lib.tilespmv_fsai_factor_csr(self.h, C.byref(rp), C.byref(ci), C.byref(v), C.byref(nnz)), "tilespmv_fsai_factor_csr")
        out = (np.empty(self.rows + 1, dtype=np.int32), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value, dtype=self.dtype))
        sync, copy = self.lib.hipStreamSynchronize, self.lib.hipMemcpy           # (the HIP runtime the library is linked against)
        sync.argtypes, sync.restype = [C.c_void_p], C.c_int
        copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        rc = sync(C.c_void_p(stream))
        for a, src in zip(out, (rp, ci, v)):
            rc = rc or copy(a.ctypes.data_as(C.c_void_p), src, a.nbytes, 2)      # hipMemcpyDeviceToHost
        self._check(rc, "FSAI.factor: hipMemcpy")
        return out

    def info(self, stream=0):
        """Synchronises ``stream``; ``{"rows", "nnz", "longest_row", "truncated_rows", "fallback_rows", "device_bytes", "dot_partials"}`` (nnz, longest_row: of G; truncated_rows:
        rows of A with more than 64 entries at or left of the diagonal; fallback_rows: rows the last create or update replaced by point Jacobi)."""
        out = (C.c_longlong * len(_lib.FSAI_INFO_NAMES))()
        self._check(self.lib.tilespmv_fsai_info(self.h, C.c_void_p(stream), out), "tilespmv_fsai_info")
        return dict(zip(_lib.FSAI_INFO_NAMES, [int(v) for v in out]))


def _fsai_handle(fsai, d_dinv, block, lib):
    """The handle of the ``fsai`` argument of ``CG`` (None: none given)."""
    if fsai is None:
        return None
    if d_dinv or block is not None:
        raise ValueError("fsai, block and d_dinv are mutually exclusive: one preconditioner")
    if not isinstance(fsai, FSAI) or not fsai.h or fsai.lib is not lib:
        raise ValueError("fsai must be an open api.FSAI of the plan's value type")
    return fsai.h


def _block_handle(block, d_dinv, lib):
    """The handle of the ``block`` argument of ``CG`` / ``BiCGStab`` (None: none given)."""
    if block is None:
        return None
    if d_dinv:
        raise ValueError("block and d_dinv are mutually exclusive: one preconditioner")
    if not isinstance(block, BlockJacobi) or not block.h or block.lib is not lib:
        raise ValueError("block must be an open api.BlockJacobi of the plan's value type")
    return block.h


class _IterativeSolver(_Solver):
    """``begin`` / ``iterate`` / ``state`` / ``solve`` of a device-resident solver over the entry points ``<_prefix>_{begin,iterate,state_read,solve,destroy}``.  A subclass names
    the prefix, where it differs the state struct (``_State``) with its dict form (``_state``), and creates the handle; ``_begin`` and ``_solve`` take the arguments an entry point
    has between ``d_x`` and the common ones (``extra``: the ``damp`` of ``CGLS``)."""

    _State = _lib.CGState

    @property
    def _destroy(self):
        return self._prefix + "_destroy"

    @staticmethod
    def _state(st):
        rel = (st.rr / st.bb) ** 0.5 if st.bb > 0 else 0.0
        return {"iterations": st.iterations, "status": st.status, "status_name": CG_STATUS_NAMES[st.status], "rr": st.rr, "bb": st.bb, "relative_residual": rel}

    def _buffer(self):
        """What ``state_read`` and ``solve`` fill."""
        return self._State()

    def _result(self, buf):
        return self._state(buf)

    def _call(self, what, *args):
        name = "%s_%s" % (self._prefix, what)
        self._check(getattr(self.lib, name)(self.h, *args), name)

    def _begin(self, d_b, d_x, extra, stream):
        self._call("begin", C.c_void_p(d_b), C.c_void_p(d_x), *extra, C.c_void_p(stream))

    def _solve(self, d_b, d_x, extra, rtol, maxiter, check_every, stream):
        buf = self._buffer()
        self._call("solve", C.c_void_p(d_b), C.c_void_p(d_x), *extra, rtol, maxiter, check_every, C.c_void_p(stream), buf)
        return self._result(buf)

    def begin(self, d_b, d_x, stream=0):
        """The start of a solve from the x that ``d_x`` holds: the residual and what the recurrence keeps beside it; asynchronous."""
        self._begin(d_b, d_x, (), stream)

    def iterate(self, d_x, count=1, stream=0):
        """``count`` iterations; asynchronous, capturable into a graph."""
        self._call("iterate", C.c_void_p(d_x), count, C.c_void_p(stream))

    def state(self, stream=0):
        """Synchronises ``stream``; the state as a dict (the class says which keys)."""
        buf = self._buffer()
        self._call("state_read", C.c_void_p(stream), buf)
        return self._result(buf)

    def solve(self, d_b, d_x, rtol=1e-10, maxiter=1000, check_every=8, stream=0):
        """``<prefix>_solve``; returns the final state (as ``state``)."""
        return self._solve(d_b, d_x, (), rtol, maxiter, check_every, stream)


class CG(_IterativeSolver):
    """``tilespmv_cg``: conjugate gradients around a resident plan, every scalar on the device (include/tilespmv.h).

    ``plan``: square and whole; it must stay open while the solver is.  ``d_dinv``: device ADDRESS of the inverse diagonal (Jacobi; borrowed), or None for plain CG.  ``block``: a
    ``BlockJacobi`` of the plan's rows instead of ``d_dinv`` (borrowed: keep it open while the solver is).  ``fsai``: an ``FSAI`` of the plan's rows instead of
    either (borrowed likewise).  ``b`` / ``x``
    are device addresses of ``rows`` elements, 16-byte aligned.  The solver and its plan run on one stream at a time.  Raises ``ValueError`` where the library returns
    hipErrorInvalidValue (a shard, a non-square plan, a misaligned vector, a preconditioner object of another row count) and for two of ``d_dinv``, ``block`` and ``fsai`` together.
    ``begin``: r = b - A x, p = z.  ``state``: ``{"iterations", "status", "status_name", "rr", "bb", "relative_residual"}``."""

    _prefix = "tilespmv_cg"
    _hint = "the plan must be square and whole; vectors 16-byte aligned; a block preconditioner has the plan's rows"

    def __init__(self, plan, d_dinv=None, block=None, fsai=None):
        self.lib, self.plan, self.block, self.fsai = plan.lib, plan, block, fsai
        h = C.c_void_p()
        fh = _fsai_handle(fsai, d_dinv, block, plan.lib)
        bh = _block_handle(block, d_dinv, plan.lib)
        if fh is not None:
            self._check(self.lib.tilespmv_cg_create_fsai(C.byref(h), plan.h, fh), "tilespmv_cg_create_fsai")
        elif bh is not None:
            self._check(self.lib.tilespmv_cg_create_block(C.byref(h), plan.h, bh), "tilespmv_cg_create_block")
        else:
            self._check(self.lib.tilespmv_cg_create(C.byref(h), plan.h, C.c_void_p(d_dinv or None)), "tilespmv_cg_create")
        self.h = h


class CGMulti(_IterativeSolver):
    """``tilespmv_cg_multi``: conjugate gradients on ``nvec`` systems in lock-step around the multi-vector product, one set of device scalars per column (include/tilespmv.h,
    DESIGN.md §3.8).

    ``plan``: square and whole; it must stay open while the solver is.  ``nvec``: 1, 2, 4 or 8.  ``d_dinv``: device ADDRESS of the inverse diagonal (``rows`` elements, shared by
    the columns; borrowed), or None.  ``B`` / ``X`` are device addresses of row-major ``(rows, nvec)`` arrays, 16-byte aligned.  ``state`` and ``solve`` return a list of ``nvec``
    dicts in the shape of ``CG.state``.  Raises ``ValueError`` where the library returns hipErrorInvalidValue (another nvec, a shard, a non-square plan, a misaligned array).
    ``begin``: R = B - A X, P = Z; ``iterate`` advances every column."""

    _prefix = "tilespmv_cg_multi"
    _hint = "nvec in {1, 2, 4, 8}; the plan must be square and whole; arrays 16-byte aligned"

    def __init__(self, plan, nvec, d_dinv=None):
        self.lib, self.plan, self.nvec = plan.lib, plan, int(nvec)
        h = C.c_void_p()
        rc = self.lib.tilespmv_cg_multi_create(C.byref(h), plan.h, self.nvec, C.c_void_p(d_dinv or None))
        self._check(rc, "tilespmv_cg_multi_create")
        self.h = h

    def _buffer(self):
        arr = (_lib.CGState * self.nvec)()
        arr[0].size = C.sizeof(_lib.CGState)
        return arr

    def _result(self, buf):
        return [self._state(st) for st in buf]


def csr_row_sqnorms_device(rows, d_rp, d_src, d_v, d_out, invert=False, stream=0, dtype=np.float64):
    """``tilespmv_csr_row_sqnorms_device``: ``d_out[i]`` = the sum of the squares of the values of row ``i`` of a device CSR (addresses), read through ``d_src`` when it is not None
    (``v[src[k]]``: with the ``rpT`` / ``srcT`` of ``csr_transpose_device`` and A's own value array, the squared column norms of A); ``invert=True``: its inverse, 1 where it is
    0 — the ``d_cinv`` of ``CGLS``.  Asynchronous on ``stream``."""
    lib = _lib.load(dtype)
    rc = lib.tilespmv_csr_row_sqnorms_device(rows, C.c_void_p(d_rp), C.c_void_p(d_src or None), C.c_void_p(d_v), C.c_void_p(d_out), 1 if invert else 0, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("tilespmv_csr_row_sqnorms_device failed (hipError %d): bad argument, or no usable device" % rc)


class CGLS(_IterativeSolver):
    """``tilespmv_cgls``: least squares ``min |A x - b|^2 + damp^2 |x|^2`` by CGLS around the resident plans of A and A^T, every scalar on the device (include/tilespmv.h,
    DESIGN.md §3.9).  It mirrors ``CG``.

    ``plan_A`` (rows x cols) and ``plan_AT`` (cols x rows; ``transpose=True``, or any plan of the transposed CSR): whole plans; they must stay open while the solver is.
    ``d_cinv``: device ADDRESS of a positive diagonal of ``cols`` elements (column scaling: ``csr_row_sqnorms_device(..., invert=True)``; borrowed), or None.  ``b`` (rows) / ``x``
    (cols) are device addresses, 16-byte aligned.  The solver and its plans run on one stream at a time.  Raises ``ValueError`` where the library returns hipErrorInvalidValue
    (swapped or mismatched plans, a shard, a misaligned vector).
    ``state``: ``{"iterations", "status", "status_name", "nn", "nn0", "rr", "bb", "relative_normal_residual"}``."""

    _prefix = "tilespmv_cgls"
    _State = _lib.CGLSState
    _hint = "whole plans of a rows x cols matrix and of its transpose; vectors 16-byte aligned"

    def __init__(self, plan_A, plan_AT, d_cinv=None):
        if plan_A.lib is not plan_AT.lib:
            raise ValueError("CGLS: both plans must have the same value type")
        self.lib, self.plan_A, self.plan_AT = plan_A.lib, plan_A, plan_AT
        h = C.c_void_p()
        rc = self.lib.tilespmv_cgls_create(C.byref(h), plan_A.h, plan_AT.h, C.c_void_p(d_cinv or None))
        self._check(rc, "tilespmv_cgls_create")
        self.h = h

    @staticmethod
    def _state(st):
        rel = (st.nn / st.nn0) ** 0.5 if st.nn0 > 0 else 0.0
        return {"iterations": st.iterations, "status": st.status, "status_name": CG_STATUS_NAMES[st.status], "nn": st.nn, "nn0": st.nn0, "rr": st.rr, "bb": st.bb,
                "relative_normal_residual": rel}

    def begin(self, d_b, d_x, damp=0.0, stream=0):
        """r = b - A x, s = A^T r - damp^2 x, p = z; asynchronous.  ``damp`` holds for the ``iterate`` calls that follow."""
        self._begin(d_b, d_x, (damp,), stream)

    def solve(self, d_b, d_x, damp=0.0, rtol=1e-10, maxiter=1000, check_every=8, stream=0):
        """``tilespmv_cgls_solve``; returns the final state (as ``state``)."""
        return self._solve(d_b, d_x, (damp,), rtol, maxiter, check_every, stream)


class BiCGStab(_IterativeSolver):
    """``tilespmv_bicgstab``: BiCGStab for a square, nonsymmetric A around a resident plan, right-preconditioned by a diagonal, every scalar on the device (include/tilespmv.h,
    DESIGN.md §3.10).  It mirrors ``CG``: the same state dict, the same statuses.

    ``plan``: square and whole (a square ``transpose=True`` plan solves ``A^T x = b``); it must stay open while the solver is.  ``d_dinv``: device ADDRESS of the inverse diagonal
    (Jacobi: ``csr_diagonal_device(..., invert=True)``; borrowed), or None.  ``block``: a ``BlockJacobi`` of the plan's rows instead of ``d_dinv`` (borrowed).
    ``b`` / ``x`` are device addresses of ``rows`` elements, 16-byte aligned.  The solver and its plan run on one stream at a time.  Raises ``ValueError`` where the library
    returns hipErrorInvalidValue (a shard, a non-square plan, a misaligned vector, a block preconditioner of another row count) and for ``block`` together with ``d_dinv``.
    ``begin``: r = b - A x, rhat = p = r."""

    _prefix = "tilespmv_bicgstab"
    _hint = "the plan must be square and whole; vectors 16-byte aligned; a block preconditioner has the plan's rows"

    def __init__(self, plan, d_dinv=None, block=None):
        self.lib, self.plan, self.block = plan.lib, plan, block
        h = C.c_void_p()
        bh = _block_handle(block, d_dinv, plan.lib)
        if bh is not None:
            self._check(self.lib.tilespmv_bicgstab_create_block(C.byref(h), plan.h, bh), "tilespmv_bicgstab_create_block")
        else:
            self._check(self.lib.tilespmv_bicgstab_create(C.byref(h), plan.h, C.c_void_p(d_dinv or None)), "tilespmv_bicgstab_create")
        self.h = h


class GMRES(_IterativeSolver):
    """``tilespmv_gmres``: restarted GMRES(``restart``) for a square, nonsymmetric A around a resident plan, right-preconditioned by a diagonal or a block-Jacobi object, every
    scalar on the device (include/tilespmv.h) — the solver for the systems ``BiCGStab`` breaks down or stagnates on.  It mirrors ``BiCGStab``: the same state
    dict, the same statuses.  One product per iteration.

    ``plan``: square and whole (a square ``transpose=True`` plan solves ``A^T x = b``); it must stay open while the solver is.  ``restart``: 1 .. 64 inner iterations per cycle
    (the workspace holds ``restart + 1`` basis vectors).  ``d_dinv`` / ``block``: as for ``BiCGStab``.  ``b`` / ``x`` are device addresses of ``rows`` elements, 16-byte aligned.
    ``x`` HOLDS THE ITERATE ONLY AFTER A CLOSE: at the end of every ``restart``-th iteration of a cycle, after ``flush`` and after ``solve``; ``rr`` is then a recomputed
    ``|b - A x|^2``, inside a cycle the recurrence's estimate of it.  A captured ``iterate(count)`` replays correctly when captured at a cycle boundary with ``count`` a multiple of
    ``restart``.  Raises ``ValueError`` where the library returns hipErrorInvalidValue (``restart`` out of range, a shard, a non-square plan, a misaligned vector, a block
    preconditioner of another row count, ``basis`` bytes the library does not store) and for ``block`` together with ``d_dinv``.

    ``basis``: how the Krylov basis is stored (``tilespmv_gmres_create_basis``).  ``None``: the plain creates.  ``"value"`` or ``0``: the value type, the same
    solver.  ``"float32"`` or ``4``: 4-byte floats — in the fp64 library the compressed basis (all arithmetic stays double; about half the bytes per iteration and half the
    workspace), in the fp32 library the identity.  With the compressed basis the true residual cannot fall below about 6e-8 x the residual a cycle began with INSIDE that cycle
    while ``rr`` keeps falling: ``solve`` accepts convergence only on a recomputed ``rr`` (it flushes and tests again); a caller of ``iterate`` who stops on ``rr`` flushes first.
    ``basis_bytes``: bytes per stored basis element; ``workspace_bytes``: the size of the solver's one allocation."""

    _prefix = "tilespmv_gmres"
    _hint = "1 <= restart <= 64; the plan must be square and whole; vectors 16-byte aligned; a block preconditioner has the plan's rows; basis bytes 0, 4 or the value type's"
    _BASIS = {"value": 0, "float32": 4}

    def __init__(self, plan, restart=30, d_dinv=None, block=None, basis=None):
        self.lib, self.plan, self.block, self.restart = plan.lib, plan, block, int(restart)
        h = C.c_void_p()
        bh = _block_handle(block, d_dinv, plan.lib)
        if basis is not None:
            if isinstance(basis, str) and basis not in self._BASIS:
                raise ValueError("basis must be None, 'value', 'float32' or a number of bytes, not %r" % (basis,))
            nbytes = self._BASIS[basis] if isinstance(basis, str) else int(basis)
            self._check(self.lib.tilespmv_gmres_create_basis(C.byref(h), plan.h, self.restart, C.c_void_p(d_dinv or None), bh, nbytes), "tilespmv_gmres_create_basis")
        elif bh is not None:
            self._check(self.lib.tilespmv_gmres_create_block(C.byref(h), plan.h, self.restart, bh), "tilespmv_gmres_create_block")
        else:
            self._check(self.lib.tilespmv_gmres_create(C.byref(h), plan.h, self.restart, C.c_void_p(d_dinv or None)), "tilespmv_gmres_create")
        self.h = h
        self.basis_bytes = self.lib.tilespmv_gmres_basis_bytes(h)
        self.workspace_bytes = self.lib.tilespmv_gmres_workspace_bytes(h)

    def flush(self, d_x, stream=0):
        """Close the cycle early and open the next: ``d_x`` is the current iterate and ``rr`` its recomputed residual; asynchronous, capturable."""
        self._call("flush", C.c_void_p(d_x), C.c_void_p(stream))


def csr_abs_diagonal_device(rows, d_rp, d_ci, d_v, d_out, invert=False, stream=0, dtype=np.float64):
    """``tilespmv_csr_abs_diagonal_device``: ``csr_diagonal_device`` with the absolute value of the summed entries (i, i); ``invert=True``: ``1 / |d|``, 1 where d is 0 — a positive
    ``d_minv`` for ``MINRES`` whatever the signs on the diagonal (a KKT matrix with a negative or zero (2,2) block).  Asynchronous on ``stream``."""
    lib = _lib.load(dtype)
    rc = lib.tilespmv_csr_abs_diagonal_device(rows, C.c_void_p(d_rp), C.c_void_p(d_ci), C.c_void_p(d_v), C.c_void_p(d_out), 1 if invert else 0, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("tilespmv_csr_abs_diagonal_device failed (hipError %d): bad argument, or no usable device" % rc)


class MINRES(_IterativeSolver):
    """``tilespmv_minres``: MINRES for a square, symmetric A that may be indefinite (saddle-point and KKT systems) around a resident plan, preconditioned by a positive diagonal,
    every scalar on the device (include/tilespmv.h).  It mirrors ``CG``: the same state dict, the same statuses.  One product per iteration; ``rr`` never increases.

    ``plan``: square and whole; it must stay open while the solver is.  ``d_minv``: device ADDRESS of a POSITIVE diagonal M^-1 (``csr_abs_diagonal_device(..., invert=True)``;
    borrowed), or None.  With it ``rr`` is ``r.M^-1 r`` and ``bb`` is ``b.M^-1 b``.  ``b`` / ``x`` are device addresses of ``rows`` elements, 16-byte aligned.  The solver and its
    plan run on one stream at a time.  Raises ``ValueError`` where the library returns hipErrorInvalidValue (a shard, a non-square plan, a misaligned vector).
    ``begin``: r2 = b - A x, z = minv o r2, beta = sqrt(r2.z)."""

    _prefix = "tilespmv_minres"
    _hint = "the plan must be square and whole; vectors 16-byte aligned"

    def __init__(self, plan, d_minv=None):
        self.lib, self.plan = plan.lib, plan
        h = C.c_void_p()
        rc = self.lib.tilespmv_minres_create(C.byref(h), plan.h, C.c_void_p(d_minv or None))
        self._check(rc, "tilespmv_minres_create")
        self.h = h


def algorithmic_bytes(nnz, rows, cols, itemsize):
    """B_alg = nnz*(s_v+4) + 4*(m+1) + s_v*(n+m)."""
    return nnz * (itemsize + 4) + 4 * (rows + 1) + itemsize * (cols + rows)
