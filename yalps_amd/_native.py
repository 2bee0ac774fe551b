"""ctypes binding of libyalps_hip.so (include/yalps_hip.h), libyalps_lpbatch.so (include/yalps_lpbatch.h),
libyalps_milpbatch.so (include/yalps_milpbatch.h), libyalps_lpvar.so (include/yalps_lpvar.h), libyalps_lpsens.so
(include/yalps_lpsens.h), libyalps_milptree.so (include/yalps_milptree.h) and libyalps_lpdense.so (include/yalps_lpdense.h).

There is no CPU path: if the library is missing, or no gfx950 device is usable,
every call raises.  Nothing here imports the oracle.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YALPS_HIP_LIB") or os.path.join(HERE, "libyalps_hip.so")  # (same switch as the N-API addon)

STATUS = ("optimal", "infeasible", "unbounded", "cycled", "timedout")
COPYBACK_FULL, COPYBACK_SOLUTION = 0, 1

# every symbol include/yalps_hip.h declares
SYMBOLS = (
    "yalps_last_error", "yalps_device_count", "yalps_simplex_f64", "yalps_simplex_f64_ex", "yalps_ctx_create",
    "yalps_ctx_destroy", "yalps_tableau_create", "yalps_tableau_destroy", "yalps_tableau_upload",
    "yalps_tableau_download", "yalps_tableau_download_rhs", "yalps_tableau_copy", "yalps_tableau_height",
    "yalps_tableau_solve", "yalps_tableau_pivot", "yalps_tableau_bench_sweep", "yalps_ctx_exchange_floor", "yalps_dense_lp_f64", "yalps_dense_lp_rows_f64",
    "yalps_round_to_precision", "yalps_ctx_create_on_stream", "yalps_tableau_set_shard", "yalps_shard_slot_doubles",
    "yalps_shard_begin", "yalps_shard_select", "yalps_shard_apply", "yalps_shard_poll", "yalps_tableau_info",
    "yalps_tableau_assemble", "yalps_simplex_sparse_f64", "yalps_tableau_apply_cuts", "yalps_tableau_node_solve", "yalps_tableau_download_solution", "yalps_milp_f64", "yalps_batch_create", "yalps_batch_destroy", "yalps_batch_set_root", "yalps_batch_solve", "yalps_batch_download",
    "yalps_tableau_debug_stamps", "yalps_tableau_padding_check", "yalps_comm_unique_id", "yalps_comm_create", "yalps_comm_create_host", "yalps_comm_destroy",
    "yalps_comm_info", "yalps_shard_run",
)
# every symbol include/yalps_lpbatch.h declares (a library of its own, loaded on first use)
LPBATCH_LIB_PATH = os.environ.get("YALPS_LPBATCH_LIB") or os.path.join(HERE, "libyalps_lpbatch.so")
SYMBOLS_LPBATCH = (
    "yalps_lpbatch_last_error", "yalps_lpbatch_create", "yalps_lpbatch_destroy", "yalps_lpbatch_class", "yalps_lpbatch_lds_bytes", "yalps_lpbatch_aux_hbm",
    "yalps_lpbatch_validate", "yalps_lpbatch_solve", "yalps_lpbatch_solution", "yalps_lpbatch_tableau", "yalps_lpbatch_info",
)
LPBATCH_MAX_BYTES = 4 << 20  # YALPS_LPBATCH_MAX_BYTES
# every symbol include/yalps_milpbatch.h declares (a third library, loaded on first use)
MILPBATCH_LIB_PATH = os.environ.get("YALPS_MILPBATCH_LIB") or os.path.join(HERE, "libyalps_milpbatch.so")
SYMBOLS_MILPBATCH = (
    "yalps_milpbatch_last_error", "yalps_milpbatch_create", "yalps_milpbatch_destroy", "yalps_milpbatch_roots", "yalps_milpbatch_root",
    "yalps_milpbatch_nodes", "yalps_milpbatch_validate_nodes", "yalps_milpbatch_node", "yalps_milpbatch_node_tableau",
    "yalps_milpbatch_solve", "yalps_milpbatch_validate", "yalps_milpbatch_solution", "yalps_milpbatch_search", "yalps_milpbatch_info",
)
MILPBATCH_MAX_BYTES = 4 << 20  # YALPS_MILPBATCH_MAX_BYTES: a node's tableau, root height + cuts rows
# every symbol include/yalps_lpvar.h declares (a fourth library, loaded on first use)
LPVAR_LIB_PATH = os.environ.get("YALPS_LPVAR_LIB") or os.path.join(HERE, "libyalps_lpvar.so")
SYMBOLS_LPVAR = (
    "yalps_lpvar_last_error", "yalps_lpvar_create", "yalps_lpvar_destroy", "yalps_lpvar_validate", "yalps_lpvar_solve",
    "yalps_lpvar_solution", "yalps_lpvar_tableau", "yalps_lpvar_info",
)
LPVAR_MAX_BYTES = 4 << 20  # YALPS_LPVAR_MAX_BYTES
# every symbol include/yalps_lpsens.h declares (a fifth library, loaded on first use)
LPSENS_LIB_PATH = os.environ.get("YALPS_LPSENS_LIB") or os.path.join(HERE, "libyalps_lpsens.so")
SYMBOLS_LPSENS = (
    "yalps_lpsens_last_error", "yalps_lpsens_create", "yalps_lpsens_destroy", "yalps_lpsens_validate", "yalps_lpsens_solve",
    "yalps_lpsens_solution", "yalps_lpsens_tableau", "yalps_lpsens_ranges", "yalps_lpsens_info",
)
LPSENS_MAX_BYTES = 4 << 20  # YALPS_LPSENS_MAX_BYTES
# every symbol include/yalps_lpwarm.h declares (a sixth library, loaded on first use)
LPWARM_LIB_PATH = os.environ.get("YALPS_LPWARM_LIB") or os.path.join(HERE, "libyalps_lpwarm.so")
SYMBOLS_LPWARM = (
    "yalps_lpwarm_last_error", "yalps_lpwarm_create", "yalps_lpwarm_destroy", "yalps_lpwarm_validate", "yalps_lpwarm_solve",
    "yalps_lpwarm_solution", "yalps_lpwarm_tableau", "yalps_lpwarm_info",
)
LPWARM_MAX_BYTES = 4 << 20  # YALPS_LPWARM_MAX_BYTES
# every symbol include/yalps_milptree.h declares (loaded on first use)
MILPTREE_LIB_PATH = os.environ.get("YALPS_MILPTREE_LIB") or os.path.join(HERE, "libyalps_milptree.so")
SYMBOLS_MILPTREE = (
    "yalps_milptree_last_error", "yalps_milptree_create", "yalps_milptree_destroy", "yalps_milptree_solve", "yalps_milptree_validate",
    "yalps_milptree_solution", "yalps_milptree_trace", "yalps_milptree_search", "yalps_milptree_info",
)
MILPTREE_MAX_BYTES = 4 << 20  # YALPS_MILPTREE_MAX_BYTES: a tree's largest possible node, root height + 2 * n_integers rows
# every symbol include/yalps_lpdense.h declares (loaded on first use)
LPDENSE_LIB_PATH = os.environ.get("YALPS_LPDENSE_LIB") or os.path.join(HERE, "libyalps_lpdense.so")
SYMBOLS_LPDENSE = (
    "yalps_lpdense_last_error", "yalps_lpdense_create", "yalps_lpdense_destroy", "yalps_lpdense_validate", "yalps_lpdense_solve",
    "yalps_lpdense_solve_duals", "yalps_lpdense_solution", "yalps_lpdense_tableau", "yalps_lpdense_info",
    "yalps_lpdense_validate_bounds", "yalps_lpdense_solve_bounds", "yalps_lpdense_validate_free", "yalps_lpdense_solve_free",
)
LPDENSE_MAX_BYTES = 4 << 20  # YALPS_LPDENSE_MAX_BYTES
MILPDENSE_LIB_PATH = os.environ.get("YALPS_MILPDENSE_LIB") or os.path.join(HERE, "libyalps_milpdense.so")
SYMBOLS_MILPDENSE = (
    "yalps_milpdense_create", "yalps_milpdense_destroy", "yalps_milpdense_validate", "yalps_milpdense_solve",
    "yalps_milpdense_overflowed", "yalps_milpdense_solution", "yalps_milpdense_trace", "yalps_milpdense_info",
    "yalps_milpdense_last_error", "yalps_milpdense_validate_bounds", "yalps_milpdense_solve_bounds",
    "yalps_milpdense_validate_free", "yalps_milpdense_solve_free")
MILPDENSE_MAX_BYTES = 4 << 20  # YALPS_MILPDENSE_MAX_BYTES: the largest possible node, root height + 2 * n_integers rows
LPBATCH_HBM_CLASS = 4        # yalps_lpbatch_class: 0..3 the LDS form, 4 the HBM form


class NativeError(RuntimeError):
    pass


# int32_t (*yalps_allgather_fn)(void *user, const double *send_host, double *recv_host, int64_t doubles_per_rank)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        f64p, i32p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
        L.yalps_last_error.restype = C.c_char_p
        L.yalps_device_count.restype = C.c_int32
        L.yalps_simplex_f64.restype = C.c_int32
        L.yalps_simplex_f64.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_double, C.c_double, C.c_int32, f64p]
        L.yalps_simplex_f64_ex.restype = C.c_int32
        L.yalps_simplex_f64_ex.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_double, C.c_double, C.c_int32,
                                           C.c_int32, f64p, C.POINTER(C.c_int64)]
        L.yalps_simplex_sparse_f64.restype = C.c_int32
        L.yalps_simplex_sparse_f64.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, C.c_double, C.c_double,
                                               C.c_int32, vp, vp, vp, f64p, C.POINTER(C.c_int64)]
        L.yalps_milp_f64.restype = C.c_int32
        L.yalps_milp_f64.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, C.c_double, C.c_double, C.c_double,
                                     C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_int32), f64p,
                                     vp, vp, vp, C.POINTER(C.c_int32), vp]
        L.yalps_tableau_download_solution.restype = C.c_int32
        L.yalps_tableau_download_solution.argtypes = [vp, vp, vp, vp]
        L.yalps_tableau_apply_cuts.restype = C.c_int32
        L.yalps_tableau_apply_cuts.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
        L.yalps_tableau_node_solve.restype = C.c_int32
        L.yalps_tableau_node_solve.argtypes = [vp, vp, C.c_int32, vp, vp, vp, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_double), vp, vp, vp]
        L.yalps_tableau_assemble.restype = C.c_int32
        L.yalps_tableau_assemble.argtypes = [vp, C.c_int32, C.c_int64, vp, vp, vp]
        L.yalps_ctx_create.restype = C.c_int32
        L.yalps_ctx_create.argtypes = [C.c_int32, C.POINTER(vp)]
        L.yalps_ctx_create_on_stream.restype = C.c_int32
        L.yalps_ctx_create_on_stream.argtypes = [C.c_int32, vp, C.POINTER(vp)]
        L.yalps_tableau_set_shard.restype = C.c_int32
        L.yalps_tableau_set_shard.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp]
        L.yalps_shard_slot_doubles.restype = C.c_int64
        L.yalps_shard_slot_doubles.argtypes = [vp]
        L.yalps_shard_begin.restype = C.c_int32
        L.yalps_shard_begin.argtypes = [vp, C.c_double, C.c_double, C.c_int32]
        L.yalps_shard_select.restype = C.c_int32
        L.yalps_shard_select.argtypes = [vp, vp]
        L.yalps_shard_apply.restype = C.c_int32
        L.yalps_shard_apply.argtypes = [vp, vp]
        L.yalps_shard_poll.restype = C.c_int32
        L.yalps_shard_poll.argtypes = [vp, C.POINTER(C.c_int32), f64p, C.POINTER(C.c_int64)]
        L.yalps_comm_unique_id.restype = C.c_int32
        L.yalps_comm_unique_id.argtypes = [vp]
        L.yalps_comm_create.restype = C.c_int32
        L.yalps_comm_create.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.yalps_comm_create_host.restype = C.c_int32
        L.yalps_comm_create_host.argtypes = [vp, ALLGATHER_FN, vp, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.yalps_comm_destroy.restype = None
        L.yalps_comm_destroy.argtypes = [vp]
        L.yalps_comm_info.restype = C.c_int32
        L.yalps_comm_info.argtypes = [vp, C.c_char_p, C.c_int32]
        L.yalps_shard_run.restype = C.c_int32
        L.yalps_shard_run.argtypes = [vp, vp, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32), f64p,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.yalps_batch_create.restype = C.c_int32
        L.yalps_batch_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.yalps_batch_destroy.restype = None
        L.yalps_batch_destroy.argtypes = [vp]
        L.yalps_batch_set_root.restype = C.c_int32
        L.yalps_batch_set_root.argtypes = [vp, vp, vp, vp]
        L.yalps_batch_solve.restype = C.c_int32
        L.yalps_batch_solve.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp,
                                        C.POINTER(C.c_float)]
        L.yalps_batch_download.restype = C.c_int32
        L.yalps_batch_download.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.yalps_ctx_destroy.restype = None
        L.yalps_ctx_destroy.argtypes = [vp]
        L.yalps_tableau_create.restype = C.c_int32
        L.yalps_tableau_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.yalps_tableau_destroy.restype = None
        L.yalps_tableau_destroy.argtypes = [vp]
        L.yalps_tableau_upload.restype = C.c_int32
        L.yalps_tableau_upload.argtypes = [vp, vp, C.c_int32, vp, vp]
        L.yalps_tableau_download.restype = C.c_int32
        L.yalps_tableau_download.argtypes = [vp, vp, vp, vp]
        L.yalps_tableau_download_rhs.restype = C.c_int32
        L.yalps_tableau_download_rhs.argtypes = [vp, vp]
        L.yalps_tableau_copy.restype = C.c_int32
        L.yalps_tableau_copy.argtypes = [vp, vp]
        L.yalps_tableau_height.restype = C.c_int32
        L.yalps_tableau_height.argtypes = [vp]
        L.yalps_tableau_info.restype = C.c_int32
        L.yalps_tableau_info.argtypes = [vp, C.c_char_p, C.c_int32]
        L.yalps_tableau_debug_stamps.restype = C.c_int32
        L.yalps_tableau_debug_stamps.argtypes = [vp, vp, C.c_int32, C.c_int32]
        L.yalps_tableau_solve.restype = C.c_int32
        L.yalps_tableau_solve.argtypes = [vp, C.c_double, C.c_double, C.c_int32, f64p, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_float)]
        L.yalps_tableau_pivot.restype = C.c_int32
        L.yalps_tableau_pivot.argtypes = [vp, C.c_int32, C.c_int32]
        L.yalps_tableau_bench_sweep.restype = C.c_int32
        L.yalps_tableau_bench_sweep.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
        L.yalps_dense_lp_f64.restype = None
        L.yalps_dense_lp_f64.argtypes = [C.c_int32, C.c_int32, C.c_double, vp]
        L.yalps_dense_lp_rows_f64.restype = None
        L.yalps_dense_lp_rows_f64.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, vp]
        L.yalps_round_to_precision.restype = C.c_double
        L.yalps_round_to_precision.argtypes = [C.c_double, C.c_double]
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise NativeError("yalps_hip error %d: %s" % (rc, lib().yalps_last_error().decode()))
    return rc


def _ptr(a, dtype):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous, (type(a), getattr(a, "dtype", None))
    return a.ctypes.data


def simplex_host(matrix, width, height, pos, var, precision=1e-8, max_pivots=8192.0, check_cycles=False,
                 copyback=COPYBACK_FULL):
    """The drop-in: in-place on host numpy arrays, like the reference's simplex(tableau, options).
    Returns (status, result, n_pivots)."""
    assert matrix.size >= width * height
    res, npiv = C.c_double(), C.c_int64()
    st = check(lib().yalps_simplex_f64_ex(_ptr(matrix, np.float64), width, height, _ptr(pos, np.int32),
                                          _ptr(var, np.int32), precision, float(max_pivots), int(bool(check_cycles)),
                                          copyback, C.byref(res), C.byref(npiv)))
    return STATUS[st], res.value, npiv.value


def simplex_sparse(width, height, row, col, val, precision=1e-8, max_pivots=8192.0, check_cycles=False):
    """Initial tableau given by its written cells (sorted by (row, col)); assembled and solved in HBM.
    Returns (status, result, n_pivots, col0, positionOfVariable, variableAtPosition)."""
    assert row.size == col.size == val.size
    col0 = np.empty(height, np.float64)
    pos, var = np.empty(width + height, np.int32), np.empty(width + height, np.int32)
    res, npiv = C.c_double(), C.c_int64()
    st = check(lib().yalps_simplex_sparse_f64(width, height, row.size, _ptr(row, np.int32), _ptr(col, np.int32),
                                              _ptr(val, np.float64), precision, float(max_pivots),
                                              int(bool(check_cycles)), col0.ctypes.data, pos.ctypes.data,
                                              var.ctypes.data, C.byref(res), C.byref(npiv)))
    return STATUS[st], res.value, npiv.value, col0, pos, var


def milp(matrix, width, height, pos, var, integers, sign, precision=1e-8, max_pivots=8192.0, check_cycles=False,
         tolerance=0.0, timeout=float("inf"), max_iterations=32768.0, node_batch=0):
    """The whole branch and cut in one native call (yalps_milp_f64).  Returns (status, result, height, col0, pos, var,
    stats) -- what solution() reads of the best tableau."""
    ints = np.ascontiguousarray(integers, np.int32)
    extra = 2 * ints.size
    col0 = np.empty(height + extra, np.float64)
    opos, ovar = np.empty(width + height + extra, np.int32), np.empty(width + height + extra, np.int32)
    st, h, res, stats = C.c_int32(), C.c_int32(), C.c_double(), np.zeros(3, np.int64)
    check(lib().yalps_milp_f64(_ptr(matrix, np.float64), width, height, _ptr(pos, np.int32), _ptr(var, np.int32),
                               ints.ctypes.data, ints.size, float(sign), precision, float(max_pivots), int(bool(check_cycles)),
                               float(tolerance), float(timeout), float(max_iterations), int(node_batch), C.byref(st),
                               C.byref(res), col0.ctypes.data, opos.ctypes.data, ovar.ctypes.data, C.byref(h),
                               stats.ctypes.data))
    n = h.value
    return (STATUS[st.value], res.value, n, col0[:n].copy(), opos[:width + n].copy(), ovar[:width + n].copy(),
            {"nodes_used": int(stats[0]), "nodes_evaluated": int(stats[1]), "batches": int(stats[2])})


class Context:
    def __init__(self, device=0, stream=None):
        """stream: an existing HIP stream handle (int) to enqueue on, e.g.
        torch.cuda.current_stream().cuda_stream; None = a private stream."""
        self.handle = C.c_void_p()
        if stream is None:
            check(lib().yalps_ctx_create(device, C.byref(self.handle)))
        else:
            check(lib().yalps_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(self.handle)))

    def close(self):
        if self.handle:
            lib().yalps_ctx_destroy(self.handle)
            self.handle = C.c_void_p()


def exchange_floor(ctx, workgroups=256, lanes=512, units=2, epochs=4000, variant=3):
    """us per round of the resident kernels' bare exchange on this chip (yalps_ctx_exchange_floor)."""
    us = C.c_float()
    check(lib().yalps_ctx_exchange_floor(ctx.handle, workgroups, lanes, units, epochs, variant, C.byref(us)))
    return us.value


class DeviceTableau:
    """A tableau resident in HBM."""

    def __init__(self, ctx, width, height_capacity):
        self.ctx, self.width, self.capacity = ctx, width, height_capacity
        self.handle = C.c_void_p()
        check(lib().yalps_tableau_create(ctx.handle, width, height_capacity, C.byref(self.handle)))

    @property
    def height(self):
        return lib().yalps_tableau_height(self.handle)

    def upload(self, matrix, height, pos, var):
        assert matrix.size >= self.width * height and pos.size >= self.width + height
        check(lib().yalps_tableau_upload(self.handle, _ptr(matrix, np.float64), height, _ptr(pos, np.int32),
                                         _ptr(var, np.int32)))

    def assemble(self, height, row, col, val):
        """Initial tableau from its written cells, sorted by (row, col) (yalps_tableau_assemble)."""
        assert row.size == col.size == val.size
        check(lib().yalps_tableau_assemble(self.handle, height, row.size, _ptr(row, np.int32), _ptr(col, np.int32),
                                           _ptr(val, np.float64)))

    def download(self, matrix=True, perms=True, perm_len=None):
        h, w = self.height, self.width
        n = perm_len if perm_len is not None else w + h
        m = np.empty(h * w, np.float64) if matrix else None
        pos = np.empty(n, np.int32) if perms else None
        var = np.empty(n, np.int32) if perms else None
        check(lib().yalps_tableau_download(self.handle, _ptr(m, np.float64), _ptr(pos, np.int32), _ptr(var, np.int32)))
        return m, pos, var

    def download_rhs(self):
        col0 = np.empty(self.height, np.float64)
        check(lib().yalps_tableau_download_rhs(self.handle, col0.ctypes.data))
        return col0

    def download_solution(self, perm_len=None):
        """(col0, positionOfVariable, variableAtPosition) with one wait (yalps_tableau_download_solution)."""
        n = perm_len if perm_len is not None else self.width + self.height
        col0, pos, var = np.empty(self.height, np.float64), np.empty(n, np.int32), np.empty(n, np.int32)
        check(lib().yalps_tableau_download_solution(self.handle, col0.ctypes.data, pos.ctypes.data, var.ctypes.data))
        return col0, pos, var

    def copy_from(self, other):
        check(lib().yalps_tableau_copy(self.handle, other.handle))

    def apply_cuts(self, root, cuts):
        """self = root's tableau + one row per cut (sign, variable, value), all on the device (yalps_tableau_apply_cuts)."""
        sign = np.array([c[0] for c in cuts] or [0], np.int32)
        var = np.array([c[1] for c in cuts] or [0], np.int32)
        val = np.array([c[2] for c in cuts] or [0.0], np.float64)
        check(lib().yalps_tableau_apply_cuts(self.handle, root.handle, len(cuts), sign.ctypes.data, var.ctypes.data,
                                             val.ctypes.data))

    def node_solve(self, root, cuts, precision=1e-8, max_pivots=8192.0, check_cycles=False):
        """applyCuts + simplex + what solution() reads, one native call (yalps_tableau_node_solve: three launches and one wait where the
        node takes the resident kernel).  Returns (status, result, height, col0, pos, var);
        the three arrays are meaningful for an optimal node."""
        sign = np.array([c[0] for c in cuts] or [0], np.int32)
        var = np.array([c[1] for c in cuts] or [0], np.int32)
        val = np.array([c[2] for c in cuts] or [0.0], np.float64)
        h = root.height + len(cuts)
        col0, p, v = np.empty(h), np.empty(self.width + h, np.int32), np.empty(self.width + h, np.int32)
        res = C.c_double()
        st = check(lib().yalps_tableau_node_solve(self.handle, root.handle, len(cuts), sign.ctypes.data, var.ctypes.data, val.ctypes.data,
                                                  precision, float(max_pivots), int(bool(check_cycles)), C.byref(res),
                                                  col0.ctypes.data, p.ctypes.data, v.ctypes.data))
        return STATUS[st], res.value, h, col0, p, v

    def solve(self, precision=1e-8, max_pivots=8192.0, check_cycles=False, timing=True):
        """Returns (status, result, n_pivots, gpu_ms); timing=False skips the HIP events (gpu_ms = 0)."""
        res, npiv, ms = C.c_double(), C.c_int64(), C.c_float()
        st = check(lib().yalps_tableau_solve(self.handle, precision, float(max_pivots), int(bool(check_cycles)),
                                             C.byref(res), C.byref(npiv), C.byref(ms) if timing else None))
        return STATUS[st], res.value, npiv.value, ms.value

    def info(self):
        """yalps_tableau_info as {key: value}; `launched` is every kernel the last solve launched, '+'-separated."""
        buf = C.create_string_buffer(2048)
        check(lib().yalps_tableau_info(self.handle, buf, 2048))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(" ") if "=" in kv)

    def debug_stamps(self, reset=True):
        """Diagnostic build only: (workgroups, 24) uint64 stage sums of the persistent launches (yalps_tableau_debug_stamps)."""
        out = np.zeros(1024 * 24, np.uint64)
        n = check(lib().yalps_tableau_debug_stamps(self.handle, out.ctypes.data, out.size, int(bool(reset))))
        return out[:n].reshape(-1, 24)

    def padding_check(self):
        """(non-finite, non-zero) doubles in the row padding of the current device buffer (yalps_tableau_padding_check)."""
        bad, nz = C.c_int64(), C.c_int64()
        check(lib().yalps_tableau_padding_check(self.handle, C.byref(bad), C.byref(nz)))
        return bad.value, nz.value

    def pivot(self, row, col):
        check(lib().yalps_tableau_pivot(self.handle, row, col))

    def bench_sweep(self, row, col, launches):
        us = C.c_float()
        check(lib().yalps_tableau_bench_sweep(self.handle, row, col, launches, C.byref(us)))
        return us.value

    # ---- row-sharded solve steps (yalps_amd/sharded.py drives them) ----
    def set_shard(self, rank, nranks, bounds, global_height, pos, var):
        b = np.ascontiguousarray(bounds, np.int32)
        assert b.size == nranks + 1 and pos.size == self.width + global_height
        check(lib().yalps_tableau_set_shard(self.handle, rank, nranks, b.ctypes.data, global_height,
                                            _ptr(pos, np.int32), _ptr(var, np.int32)))

    def shard_slot_doubles(self):
        return int(lib().yalps_shard_slot_doubles(self.handle))

    def shard_begin(self, precision, max_pivots, check_cycles=False):
        check(lib().yalps_shard_begin(self.handle, precision, float(max_pivots), int(bool(check_cycles))))

    def shard_select(self, send_ptr):
        check(lib().yalps_shard_select(self.handle, C.c_void_p(send_ptr)))

    def shard_apply(self, gathered_ptr):
        check(lib().yalps_shard_apply(self.handle, C.c_void_p(gathered_ptr)))

    def shard_run(self, comm, precision=1e-8, max_pivots=8192.0, check_every=64, check_cycles=False):
        """The whole row-sharded solve natively (yalps_shard_run): no Python between two pivots.
        Returns (status code, result, n_pivots, gpu_ms)."""
        st, res, npiv, ms = C.c_int32(), C.c_double(), C.c_int64(), C.c_float()
        check(lib().yalps_shard_run(self.handle, comm.handle, precision, float(max_pivots), int(bool(check_cycles)), int(check_every), C.byref(st),
                                    C.byref(res), C.byref(npiv), C.byref(ms)))
        return st.value, res.value, npiv.value, ms.value

    def shard_poll(self):
        st, res, npiv = C.c_int32(), C.c_double(), C.c_int64()
        check(lib().yalps_shard_poll(self.handle, C.byref(st), C.byref(res), C.byref(npiv)))
        return st.value, res.value, npiv.value

    def close(self):
        if self.handle:
            lib().yalps_tableau_destroy(self.handle)
            self.handle = C.c_void_p()


class Comm:
    """This rank's end of the sharded solve's exchange (yalps_comm): RCCL, or a host all-gather callback."""

    def __init__(self, handle, keep=None):
        self.handle, self._keep = handle, keep

    @staticmethod
    def unique_id():
        """128 bytes from ncclGetUniqueId: made on rank 0, handed to every rank by the host's own channel."""
        buf = C.create_string_buffer(128)
        check(lib().yalps_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def rccl(cls, ctx, unique_id, rank, nranks):
        h = C.c_void_p()
        check(lib().yalps_comm_create(ctx.handle, C.c_char_p(bytes(unique_id)), rank, nranks, C.byref(h)))
        return cls(h)

    @classmethod
    def host(cls, ctx, allgather, rank, nranks):
        """allgather(send: float64[n]) -> float64[nranks * n] on host arrays (e.g. a gloo all-gather)."""
        def thunk(_user, send, recv, n):
            try:
                out = allgather(np.ctypeslib.as_array(send, shape=(n,)).copy())
                np.ctypeslib.as_array(recv, shape=(nranks * n,))[:] = out
                return 0
            except Exception:  # (never unwind through the C frames)
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLGATHER_FN(thunk)
        h = C.c_void_p()
        check(lib().yalps_comm_create_host(ctx.handle, cb, None, rank, nranks, C.byref(h)))
        return cls(h, keep=cb)

    def info(self):
        buf = C.create_string_buffer(256)
        check(lib().yalps_comm_info(self.handle, buf, 256))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(" ") if "=" in kv)

    def close(self):
        if self.handle:
            lib().yalps_comm_destroy(self.handle)
            self.handle = C.c_void_p()


class NodeBatch:
    """Batched branch-and-cut node evaluation: the root's optimal tableau stays in HBM, every node
    (= a list of cuts (sign, variable, value)) gets its own workgroup (yalps_batch_*)."""

    def __init__(self, ctx, width, root_height, max_cuts, max_nodes):
        self.ctx, self.width, self.root_height = ctx, width, root_height
        self.max_cuts, self.max_nodes = max_cuts, max_nodes
        self.handle = C.c_void_p()
        check(lib().yalps_batch_create(ctx.handle, width, root_height, max_cuts, max_nodes, C.byref(self.handle)))

    def set_root(self, matrix, pos, var):
        check(lib().yalps_batch_set_root(self.handle, _ptr(matrix, np.float64), _ptr(pos, np.int32), _ptr(var, np.int32)))

    def solve(self, cut_lists, precision=1e-8, max_pivots=8192.0):
        """cut_lists: per node a sequence of (sign, variable, value).  Returns (status names,
        results, pivot counts, node heights, gpu_ms)."""
        count = len(cut_lists)
        off = np.zeros(count + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in cut_lists])
        flat = [c for cuts in cut_lists for c in cuts]
        sign = np.array([c[0] for c in flat] or [0], np.int32)
        var = np.array([c[1] for c in flat] or [0], np.int32)
        val = np.array([c[2] for c in flat] or [0.0], np.float64)
        st, res, piv, ms = np.empty(count, np.int32), np.empty(count, np.float64), np.empty(count, np.int64), C.c_float()
        check(lib().yalps_batch_solve(self.handle, count, off.ctypes.data, sign.ctypes.data, var.ctypes.data,
                                      val.ctypes.data, precision, float(max_pivots), st.ctypes.data, res.ctypes.data,
                                      piv.ctypes.data, C.byref(ms)))
        heights = self.root_height + np.diff(off)
        return [STATUS[k] for k in st], res, piv, heights, ms.value

    def download(self, node, height, matrix=False):
        w = self.width
        m = np.empty(height * w, np.float64) if matrix else None
        col0 = np.empty(height, np.float64)
        pos, var = np.empty(w + height, np.int32), np.empty(w + height, np.int32)
        check(lib().yalps_batch_download(self.handle, node, height, _ptr(m, np.float64), col0.ctypes.data,
                                         pos.ctypes.data, var.ctypes.data))
        return m, col0, pos, var

    def close(self):
        if self.handle:
            lib().yalps_batch_destroy(self.handle)
            self.handle = C.c_void_p()


def dense_lp(M, N, seed=42.0):
    """dense-LP(M,N,seed) of SURVEY.md 8(d) as a flat row-major (M+1)x(N+1) tableau."""
    m = np.zeros((M + 1) * (N + 1), np.float64)
    lib().yalps_dense_lp_f64(M, N, float(seed), m.ctypes.data)
    return m


def dense_lp_rows(M, N, seed, row_begin, row_end):
    """Rows [row_begin, row_end) of dense-LP(M,N,seed) (row 0 = objective row), flat row-major: one rank's share of a
    row-sharded tableau without the 8*(M+1)*(N+1) bytes of the whole."""
    row_end = min(row_end, M + 1)
    m = np.zeros(max(row_end - row_begin, 0) * (N + 1), np.float64)
    lib().yalps_dense_lp_rows_f64(M, N, float(seed), row_begin, row_end, m.ctypes.data)
    return m


def round_to_precision(x, precision):
    return lib().yalps_round_to_precision(x, precision)


_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
_BATCH_LIBS = {}    # prefix -> (path, {name behind the prefix: (restype, argtypes)}); every library also has _COMMON_SIGS
_loaded = {}        # prefix -> CDLL
_COMMON_SIGS = {"last_error": (C.c_char_p, None), "create": (_I32, [_I32, _VP, C.POINTER(_VP)]), "destroy": (None, [_VP]),
                "info": (_I32, [_VP, C.c_char_p, _I32])}


def _load_lib(prefix):
    """The library of _BATCH_LIBS[prefix], loaded once, its functions given their signatures."""
    L = _loaded.get(prefix)
    if L is None:
        path, sigs = _BATCH_LIBS[prefix]
        if not os.path.exists(path):
            raise NativeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = C.CDLL(path)
        for name, (restype, argtypes) in {**_COMMON_SIGS, **sigs}.items():
            fn = getattr(L, "%s_%s" % (prefix, name))
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        _loaded[prefix] = L
    return L


def _check(prefix, rc):
    if rc < 0:
        raise NativeError("%s error %d: %s" % (prefix, rc, getattr(_load_lib(prefix), prefix + "_last_error")().decode()))
    return rc


def _info_text(prefix, handle, first=1 << 12):
    """The text of <prefix>_info, the buffer grown to what the library says it needs (it names every rerun item)."""
    info = getattr(_load_lib(prefix), prefix + "_info")
    buf = C.create_string_buffer(first)
    need = _check(prefix, info(handle, buf, len(buf)))
    if need >= len(buf):
        buf = C.create_string_buffer(need + 1)
        _check(prefix, info(handle, buf, len(buf)))
    return buf.value.decode()


def _info_lines(text):
    """(head, kernels) of an info text: the key=value pairs of its first line, and of every further line as a dict."""
    lines = text.splitlines()
    head = dict(kv.split("=", 1) for kv in lines[0].split()) if lines else {}
    kernels = []
    for line in lines[1:]:
        kv = dict(x.split("=", 1) for x in line.split())
        kernels.append({k: (v if k == "kernel" else int(v)) for k, v in kv.items()})
    return head, kernels


def _batch_info(text, more=()):
    """The text of yalps_lpbatch_info / yalps_lpsens_info / yalps_lpvar_info as LpBatch.info()'s dict; `more`: further integer
    keys of the first line."""
    head, kernels = _info_lines(text)
    ids = head.get("rerun_lps", "[]").strip("[]")
    out = {k: int(head.get(k, 0)) for k in ("launches", "reruns", *more)}
    out.update(rerun_lps=[int(x) for x in ids.split(",") if x], kernels=kernels, text=text)
    return out


# yalps_lpbatch_* and yalps_lpsens_*: validate, solve, solution, tableau
_LP_SIGS = {"validate": (_I32, [_I32, _VP, _VP, _VP, _VP, _VP]),
            "solve": (_I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, C.POINTER(C.c_float)]),
            "solution": (_I32, [_VP, _I32, _VP, _VP, _VP]), "tableau": (_I32, [_VP, _I32, _VP])}


_BATCH_LIBS["yalps_lpbatch"] = (LPBATCH_LIB_PATH, {
    **_LP_SIGS, "class": (_I32, [_I32, _I32]), "lds_bytes": (_I64, [_I32, _I32]), "aux_hbm": (_I32, [_I32, _I32])})


def lpbatch_lib():
    return _load_lib("yalps_lpbatch")


def lpbatch_check(rc):
    return _check("yalps_lpbatch", rc)


def lpbatch_class(width, height):
    """Size class of a width x height LP: 0..3 the LDS form, 4 the HBM form, -1 not batchable (host only)."""
    return lpbatch_lib().yalps_lpbatch_class(int(width), int(height))


def lpbatch_lds_bytes(width, height):
    return lpbatch_lib().yalps_lpbatch_lds_bytes(int(width), int(height))


def lpbatch_aux_hbm(width, height):
    """1 where a width x height LP takes the aux form of the HBM class (colbuf / prow in HBM), 0 where not, -1 not batchable."""
    return lpbatch_lib().yalps_lpbatch_aux_hbm(int(width), int(height))


class PackedLps:
    """A heterogeneous batch as yalps_lpbatch_solve takes it: per LP width, height and options, all cells in three arrays."""

    def __init__(self, lps):
        """lps: a sequence of (width, height, row, col, val, precision, max_pivots, check_cycles)."""
        n = len(lps)
        self.count = n
        self.width = np.fromiter((lp[0] for lp in lps), np.int32, n)
        self.height = np.fromiter((lp[1] for lp in lps), np.int32, n)
        self.offsets = np.zeros(n + 1, np.int64)
        self.offsets[1:] = np.cumsum([lp[2].size for lp in lps])
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([lp[k] for lp in lps]), dt) if n else np.zeros(0, dt)
        self.row, self.col, self.val = cat(2, np.int32), cat(3, np.int32), cat(4, np.float64)
        assert self.row.size == self.col.size == self.val.size == self.offsets[-1]
        self.precision = np.fromiter((lp[5] for lp in lps), np.float64, n)
        self.max_pivots = np.fromiter((float(lp[6]) for lp in lps), np.float64, n)
        self.check_cycles = np.fromiter((int(bool(lp[7])) for lp in lps), np.int32, n)

    def validate(self):
        """The argument checks of yalps_lpbatch_solve, on the host (raises NativeError naming the LP)."""
        lpbatch_check(lpbatch_lib().yalps_lpbatch_validate(self.count, self.width.ctypes.data, self.height.ctypes.data,
                                                           self.offsets.ctypes.data, self.row.ctypes.data, self.col.ctypes.data))


def dense_cells(matrix, width, height):
    """(row, col, val) of a dense row-major tableau: every entry whose bits are not +0.0 (a -0.0 is a written cell)."""
    idx = np.flatnonzero(np.ascontiguousarray(matrix[:width * height]).view(np.int64))
    return (idx // width).astype(np.int32), (idx % width).astype(np.int32), np.ascontiguousarray(matrix[idx])


class LpBatch:
    """Many independent LPs per call, one workgroup per LP (yalps_lpbatch_*).  Belongs to one thread at a time."""
    _prefix = "yalps_lpbatch"

    def _call(self, name, *args):
        return _check(self._prefix, getattr(_load_lib(self._prefix), "%s_%s" % (self._prefix, name))(*args))

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        self._call("create", device, C.c_void_p(stream) if stream is not None else None, C.byref(self.handle))
        self.packed = None

    def solve(self, lps, keep_tableaux=False):
        """lps: a PackedLps or the sequence it is made from.  Returns (status names, results, pivot counts, gpu_ms)."""
        p = lps if isinstance(lps, PackedLps) else PackedLps(lps)
        n = p.count
        st, res, piv, ms = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int64), C.c_float()
        self.packed = None
        self._call("solve", self.handle, n, p.width.ctypes.data, p.height.ctypes.data, p.offsets.ctypes.data, p.row.ctypes.data,
                   p.col.ctypes.data, p.val.ctypes.data, p.precision.ctypes.data, p.max_pivots.ctypes.data, p.check_cycles.ctypes.data,
                   int(bool(keep_tableaux)), st.ctypes.data, res.ctypes.data, piv.ctypes.data, C.byref(ms))
        self.packed = p
        return [STATUS[k] for k in st], res, piv, ms.value

    def _shape(self, i):
        if self.packed is None or not 0 <= i < self.packed.count:
            raise NativeError("%s: no such LP in the last solve: %r" % (type(self).__name__, i))
        return int(self.packed.width[i]), int(self.packed.height[i])

    def solution(self, i):
        """(col0, positionOfVariable, variableAtPosition) of LP i of the last solve."""
        w, h = self._shape(i)
        col0 = np.empty(h, np.float64)
        pos, var = np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        self._call("solution", self.handle, i, col0.ctypes.data, pos.ctypes.data, var.ctypes.data)
        return col0, pos, var

    def tableau(self, i):
        """The whole final matrix of LP i of the last solve (solve(..., keep_tableaux=True)), flat row-major."""
        w, h = self._shape(i)
        m = np.empty(w * h, np.float64)
        self._call("tableau", self.handle, i, m.ctypes.data)
        return m

    def info(self):
        """{"launches": n, "reruns": n, "rerun_lps": [...], "kernels": [{kernel, class, lps, grid, lds, pass, hist_cap}], "text"}"""
        return _batch_info(_info_text(self._prefix, self.handle))

    def close(self):
        if self.handle:
            getattr(_load_lib(self._prefix), self._prefix + "_destroy")(self.handle)
            self.handle = C.c_void_p()


# ---------------------------------------------------------------------------------------------- libyalps_lpsens.so

_BATCH_LIBS["yalps_lpsens"] = (LPSENS_LIB_PATH, {**_LP_SIGS, "ranges": (_I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP])})


def lpsens_lib():
    return _load_lib("yalps_lpsens")


def lpsens_check(rc):
    return _check("yalps_lpsens", rc)


def lpsens_validate(packed):
    """The argument checks of yalps_lpsens_solve on a PackedLps, on the host (raises NativeError naming the LP)."""
    lpsens_check(lpsens_lib().yalps_lpsens_validate(packed.count, packed.width.ctypes.data, packed.height.ctypes.data,
                                                    packed.offsets.ctypes.data, packed.row.ctypes.data, packed.col.ctypes.data))


class LpSens(LpBatch):
    """LpBatch's interface over yalps_lpsens_*, plus ranges(i): many independent LPs per call, one workgroup per LP, and for
    every LP that ends optimal the five ranging arrays of its final tableau.  Belongs to one thread at a time.
    info() spells the kernels lp_sens_kernel<T[,check][,lds]>."""
    _prefix = "yalps_lpsens"

    def ranges(self, i):
        """(row0, col_up, col_dn, row_lo, row_hi) of LP i of the last solve, which must have ended optimal (NativeError
        otherwise): include/yalps_lpsens.h says what they hold."""
        w, h = self._shape(i)
        row0, col_up, col_dn = np.empty(w, np.float64), np.empty(w, np.float64), np.empty(w, np.float64)
        row_lo, row_hi = np.empty(h, np.float64), np.empty(h, np.float64)
        self._call("ranges", self.handle, i, row0.ctypes.data, col_up.ctypes.data, col_dn.ctypes.data, row_lo.ctypes.data,
                   row_hi.ctypes.data)
        return row0, col_up, col_dn, row_lo, row_hi


# ---------------------------------------------------------------------------------------------- libyalps_lpvar.so

_BATCH_LIBS["yalps_lpvar"] = (LPVAR_LIB_PATH, {
        "validate": (_I32, [_I32, _I32, _I64, _VP, _VP, _I32, _VP, _VP, _VP]),
        "solve": (_I32, [_VP, _I32, _I32, _I64, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP,
                         C.POINTER(C.c_float)]),
        "solution": (_I32, [_VP, _I32, _VP, _VP, _VP]), "tableau": (_I32, [_VP, _I32, _VP])})


def lpvar_lib():
    return _load_lib("yalps_lpvar")


def lpvar_check(rc):
    return _check("yalps_lpvar", rc)


class PackedVariants:
    """Variants of one LP as yalps_lpvar_solve takes them: the base's cells once, every variant's patch in three arrays."""

    def __init__(self, width, height, row, col, val, patches, options=None, flat=None):
        """row / col / val: the base's cells.  patches: per variant (row, col, val).  options: per variant (precision,
        max_pivots, check_cycles); None = the defaults of solve for every variant.
        flat = (offsets, row, col, val) gives the patches already concatenated (patches is then only counted)."""
        n = len(patches)
        self.count, self.width, self.height = n, int(width), int(height)
        self.row = np.ascontiguousarray(row, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)
        assert self.row.size == self.col.size == self.val.size
        if flat is not None:
            off, prow, pcol, pval = flat
            self.offsets = np.ascontiguousarray(off, np.int64)
            self.patch_row, self.patch_col = np.ascontiguousarray(prow, np.int32), np.ascontiguousarray(pcol, np.int32)
            self.patch_val = np.ascontiguousarray(pval, np.float64)
        else:
            self.offsets = np.zeros(n + 1, np.int64)
            self.offsets[1:] = np.cumsum([len(p[0]) for p in patches])
            cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(p[k], dt) for p in patches]), dt) if n else np.zeros(0, dt)
            self.patch_row, self.patch_col, self.patch_val = cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)
        assert self.offsets.size == n + 1 and self.patch_row.size == self.patch_col.size == self.patch_val.size
        if options is None:
            options = [(1e-8, 8192.0, False)] * n
        assert len(options) == n
        self.precision = np.fromiter((o[0] for o in options), np.float64, n)
        self.max_pivots = np.fromiter((float(o[1]) for o in options), np.float64, n)
        self.check_cycles = np.fromiter((int(bool(o[2])) for o in options), np.int32, n)

    def validate(self):
        """The argument checks of yalps_lpvar_solve, on the host (raises NativeError naming the variant)."""
        lpvar_check(lpvar_lib().yalps_lpvar_validate(
            self.width, self.height, self.row.size, self.row.ctypes.data, self.col.ctypes.data, self.count,
            self.offsets.ctypes.data, self.patch_row.ctypes.data, self.patch_col.ctypes.data))


class LpVariants:
    """Many variants of one LP per call, one workgroup per variant (yalps_lpvar_*).  Belongs to one thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        lpvar_check(lpvar_lib().yalps_lpvar_create(device, C.c_void_p(stream) if stream is not None else None,
                                                   C.byref(self.handle)))
        self.packed = None

    def solve(self, packed, keep_tableaux=False):
        """packed: a PackedVariants.  Returns (status names, results, pivot counts, gpu_ms)."""
        p = packed
        n = p.count
        st, res, piv, ms = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int64), C.c_float()
        self.packed = None
        lpvar_check(lpvar_lib().yalps_lpvar_solve(
            self.handle, p.width, p.height, p.row.size, p.row.ctypes.data, p.col.ctypes.data, p.val.ctypes.data, n,
            p.offsets.ctypes.data, p.patch_row.ctypes.data, p.patch_col.ctypes.data, p.patch_val.ctypes.data,
            p.precision.ctypes.data, p.max_pivots.ctypes.data, p.check_cycles.ctypes.data, int(bool(keep_tableaux)),
            st.ctypes.data, res.ctypes.data, piv.ctypes.data, C.byref(ms)))
        self.packed = p
        return [STATUS[k] for k in st], res, piv, ms.value

    def _check(self, i):
        if self.packed is None or not 0 <= i < self.packed.count:
            raise NativeError("LpVariants: no such variant in the last solve: %r" % (i,))
        return self.packed.width, self.packed.height

    def solution(self, i):
        """(col0, positionOfVariable, variableAtPosition) of variant i of the last solve."""
        w, h = self._check(i)
        col0 = np.empty(h, np.float64)
        pos, var = np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        lpvar_check(lpvar_lib().yalps_lpvar_solution(self.handle, i, col0.ctypes.data, pos.ctypes.data, var.ctypes.data))
        return col0, pos, var

    def tableau(self, i):
        """The whole final matrix of variant i of the last solve (solve(..., keep_tableaux=True)), flat row-major."""
        w, h = self._check(i)
        m = np.empty(w * h, np.float64)
        lpvar_check(lpvar_lib().yalps_lpvar_tableau(self.handle, i, m.ctypes.data))
        return m

    def info(self):
        """{"launches", "reruns", "rerun_lps": [...], "base_cells", "patch_cells", "image_bytes",
        "kernels": [{kernel, class, aux, lps, grid, lds, pass, hist_cap}], "text"}"""
        return _batch_info(_info_text("yalps_lpvar", self.handle), more=("base_cells", "patch_cells", "image_bytes"))

    def close(self):
        if self.handle:
            lpvar_lib().yalps_lpvar_destroy(self.handle)
            self.handle = C.c_void_p()


# ---------------------------------------------------------------------------------------------- libyalps_lpwarm.so

_BATCH_LIBS["yalps_lpwarm"] = (LPWARM_LIB_PATH, {
        "validate": (_I32, [_I32, _I32, _I64, _VP, _VP, _I32, _VP, _VP, _VP]),
        "solve": (_I32, [_VP, _I32, _I32, _I64, _VP, _VP, _VP, C.c_double, C.c_double, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                         _I32, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
        "solution": (_I32, [_VP, _I32, _VP, _VP, _VP]), "tableau": (_I32, [_VP, _I32, _VP])})


def lpwarm_lib():
    return _load_lib("yalps_lpwarm")


def lpwarm_check(rc):
    return _check("yalps_lpwarm", rc)


class PackedWarm(PackedVariants):
    """Variants of one LP as yalps_lpwarm_solve takes them: PackedVariants -- patches of the INITIAL tableau, here in row 0
    and column 0 only -- plus the options of the base's own solve."""

    def __init__(self, width, height, row, col, val, patches, options=None, flat=None, base_options=(1e-8, 8192.0, False)):
        super().__init__(width, height, row, col, val, patches, options, flat)
        self.base_precision, self.base_max_pivots = float(base_options[0]), float(base_options[1])
        self.base_check_cycles = int(bool(base_options[2]))

    def validate(self):
        """The argument checks of yalps_lpwarm_solve, on the host (raises NativeError naming the variant)."""
        lpwarm_check(lpwarm_lib().yalps_lpwarm_validate(
            self.width, self.height, self.row.size, self.row.ctypes.data, self.col.ctypes.data, self.count,
            self.offsets.ctypes.data, self.patch_row.ctypes.data, self.patch_col.ctypes.data))


class LpWarm:
    """Many variants of one LP per call, each reoptimised from the base's optimal tableau by one workgroup (yalps_lpwarm_*).
    Belongs to one thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        lpwarm_check(lpwarm_lib().yalps_lpwarm_create(device, C.c_void_p(stream) if stream is not None else None,
                                                     C.byref(self.handle)))
        self.packed = None
        self.base = None

    def solve(self, packed, keep_tableaux=False):
        """packed: a PackedWarm.  Returns (status names, results, pivot counts, gpu_ms) of the variants, or None where the
        base did not end optimal (nothing ran for the variants); self.base = (status name, result, pivots) of the base."""
        p = packed
        n = p.count
        st, res, piv, ms = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int64), C.c_float()
        bst, bres, bpiv = C.c_int32(), C.c_double(), C.c_int64()
        self.packed = self.base = None
        lpwarm_check(lpwarm_lib().yalps_lpwarm_solve(
            self.handle, p.width, p.height, p.row.size, p.row.ctypes.data, p.col.ctypes.data, p.val.ctypes.data,
            p.base_precision, p.base_max_pivots, p.base_check_cycles, n, p.offsets.ctypes.data, p.patch_row.ctypes.data,
            p.patch_col.ctypes.data, p.patch_val.ctypes.data, p.precision.ctypes.data, p.max_pivots.ctypes.data,
            p.check_cycles.ctypes.data, int(bool(keep_tableaux)), C.addressof(bst), C.addressof(bres), C.addressof(bpiv),
            st.ctypes.data, res.ctypes.data, piv.ctypes.data, C.byref(ms)))
        self.base = (STATUS[bst.value], bres.value, bpiv.value)
        if self.base[0] != "optimal":
            return None
        self.packed = p
        return [STATUS[k] for k in st], res, piv, ms.value

    def _check(self, i):
        if self.packed is None or not 0 <= i < self.packed.count:
            raise NativeError("LpWarm: no such variant in the last solve: %r" % (i,))
        return self.packed.width, self.packed.height

    def solution(self, i):
        """(col0, positionOfVariable, variableAtPosition) of variant i of the last solve."""
        w, h = self._check(i)
        col0 = np.empty(h, np.float64)
        pos, var = np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        lpwarm_check(lpwarm_lib().yalps_lpwarm_solution(self.handle, i, col0.ctypes.data, pos.ctypes.data, var.ctypes.data))
        return col0, pos, var

    def tableau(self, i):
        """The whole final matrix of variant i of the last solve (solve(..., keep_tableaux=True)), flat row-major."""
        w, h = self._check(i)
        m = np.empty(w * h, np.float64)
        lpwarm_check(lpwarm_lib().yalps_lpwarm_tableau(self.handle, i, m.ctypes.data))
        return m

    def info(self):
        """{"launches", "reruns", "rerun_lps": [...], "base_status", "base_pivots", "patch_cells", "records", "image_bytes",
        "kernels": [{kernel, class, aux, lps, grid, lds, pass, hist_cap}], "text"}"""
        return _batch_info(_info_text("yalps_lpwarm", self.handle),
                           more=("base_status", "base_pivots", "patch_cells", "records", "image_bytes"))

    def close(self):
        if self.handle:
            lpwarm_lib().yalps_lpwarm_destroy(self.handle)
            self.handle = C.c_void_p()


# ---------------------------------------------------------------------------------------------- libyalps_lpdense.so

class DenseOperand(C.Structure):
    """yalps_lpdense_operand: a device pointer and its element strides (batch, row, col), counted in doubles."""
    _fields_ = [("ptr", C.c_void_p), ("batch", C.c_int64), ("row", C.c_int64), ("col", C.c_int64)]


_DOP = C.POINTER(DenseOperand)
_BATCH_LIBS["yalps_lpdense"] = (LPDENSE_LIB_PATH, {
        "validate": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP]),
        "solve": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, C.c_double, C.c_double, _I32, _I32,
                         _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
        "solve_duals": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, C.c_double, C.c_double, _I32, _I32,
                               _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
        "validate_bounds": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP]),
        "solve_bounds": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, C.c_double,
                                C.c_double, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
        "validate_free": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP]),
        "solve_free": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, C.c_double,
                              C.c_double, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float)]),
        "solution": (_I32, [_VP, _I32, _VP, _VP, _VP]), "tableau": (_I32, [_VP, _I32, _VP])})


def lpdense_lib():
    return _load_lib("yalps_lpdense")


def lpdense_check(rc):
    return _check("yalps_lpdense", rc)


def _dense_operands(operands):
    """Five (ptr, batch, row, col) tuples (None: an operand without elements) as yalps_lpdense_operand structs."""
    assert len(operands) == 5
    return [DenseOperand(*(o if o is not None else (None, 0, 0, 0))) for o in operands]


def lpdense_validate(count, n, m_ub, m_eq, operands):
    """The host-only argument checks of yalps_lpdense_solve (raises NativeError with the reason); operands = (c, A_ub, b_ub,
    A_eq, b_eq), each (ptr, batch, row, col) or None.  No pointer is dereferenced."""
    ops = _dense_operands(operands)
    lpdense_check(lpdense_lib().yalps_lpdense_validate(int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops)))


def _dense_bounds(lb, ub, upper):
    """(lb descriptor or None, ub descriptor or None, n_upper, the int32 index array) of the bounds arguments."""
    idx = np.ascontiguousarray(upper, np.int32).reshape(-1)
    return (None if lb is None else C.byref(DenseOperand(*lb)), None if ub is None else C.byref(DenseOperand(*ub)), int(idx.size), idx)


def lpdense_validate_bounds(count, n, m_ub, m_eq, operands, lb=None, ub=None, upper=()):
    """The host-only argument checks of yalps_lpdense_solve_bounds: lpdense_validate's with the height that counts the
    len(upper) bound rows, plus lb / ub ((ptr, batch, row, col) or None: absent) and the index list."""
    ops = _dense_operands(operands)
    lbp, ubp, k, idx = _dense_bounds(lb, ub, upper)
    lpdense_check(lpdense_lib().yalps_lpdense_validate_bounds(int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops),
                                                              lbp, ubp, k, idx.ctypes.data))


def lpdense_validate_free(count, n, m_ub, m_eq, operands, lb=None, ub=None, upper=(), free=()):
    """The host-only argument checks of yalps_lpdense_solve_free: lpdense_validate_bounds' with the width that counts the
    len(free) twin columns, plus the index list of the free variables."""
    ops = _dense_operands(operands)
    lbp, ubp, k, idx = _dense_bounds(lb, ub, upper)
    fidx = np.ascontiguousarray(free, np.int32).reshape(-1)
    lpdense_check(lpdense_lib().yalps_lpdense_validate_free(int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops),
                                                            lbp, ubp, k, idx.ctypes.data, int(fidx.size), fidx.ctypes.data))


class LpDense:
    """Batches of dense LPs of one shape, operands and answers in device memory (yalps_lpdense_*).  Pointers are plain
    integers (a tensor's data_ptr()); nothing here imports torch.  Belongs to one thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        lpdense_check(lpdense_lib().yalps_lpdense_create(device, C.c_void_p(stream) if stream is not None else None,
                                                         C.byref(self.handle)))
        self.shape = None  # (count, width, height) of the last solve

    def solve(self, count, n, m_ub, m_eq, operands, maximize=False, precision=1e-8, max_pivots=8192.0, check_cycles=False,
              keep_tableaux=False, x=None, objective=None, status=None, pivots=None, ineqlin=None, eqlin=None, reduced=None,
              lb=None, ub=None, upper=(), upper_out=None, free=()):
        """operands = (c, A_ub, b_ub, A_eq, b_eq), each (device pointer, batch, row, col strides in doubles) or None where it
        has no element; x / objective / status / pivots: device pointers of contiguous float64 [count][n], float64 [count],
        int32 [count], int64 [count], or None; ineqlin / eqlin / reduced: the marginals (yalps_lpdense_solve_duals), device
        pointers of contiguous float64 [count][m_ub], [count][m_eq], [count][n], or None -- with all three None the call is
        yalps_lpdense_solve.  lb / ub: (device pointer, batch, row, col) of the bounds x >= lb and x[j] <= ub[j] for the
        ascending indices j of `upper` (a host sequence), or None; upper_out: device pointer of contiguous float64
        [count][len(upper)], the bound rows' marginals, or None -- with lb or ub given the call is yalps_lpdense_solve_bounds, and
        the tableau is len(upper) rows taller.  free: the ascending indices of the variables without a lower bound (a host
        sequence) -- with any the call is yalps_lpdense_solve_free, with or without lb / ub, and the tableau is len(free) columns
        wider.  The outputs are complete on return.  Returns gpu_ms."""
        ops = _dense_operands(operands)
        ms = C.c_float()
        self.shape = None
        head = (self.handle, int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops), int(bool(maximize)), float(precision),
                float(max_pivots), int(bool(check_cycles)), int(bool(keep_tableaux)), x, objective, status, pivots)
        k = 0
        if len(free):
            lbp, ubp, k, idx = _dense_bounds(lb, ub, upper)
            fidx = np.ascontiguousarray(free, np.int32).reshape(-1)
            lpdense_check(lpdense_lib().yalps_lpdense_solve_free(*head[:10], lbp, ubp, k, idx.ctypes.data, int(fidx.size), fidx.ctypes.data,
                                                                 *head[10:], ineqlin, eqlin, reduced, upper_out, C.byref(ms)))
        elif lb is not None or ub is not None:
            lbp, ubp, k, idx = _dense_bounds(lb, ub, upper)
            lpdense_check(lpdense_lib().yalps_lpdense_solve_bounds(*head[:10], lbp, ubp, k, idx.ctypes.data, *head[10:], ineqlin, eqlin,
                                                                   reduced, upper_out, C.byref(ms)))
        elif len(upper) or upper_out is not None:
            raise NativeError("LpDense.solve: upper / upper_out without lb or ub")
        elif ineqlin is None and eqlin is None and reduced is None:
            lpdense_check(lpdense_lib().yalps_lpdense_solve(*head, C.byref(ms)))
        else:
            lpdense_check(lpdense_lib().yalps_lpdense_solve_duals(*head, ineqlin, eqlin, reduced, C.byref(ms)))
        self.shape = (int(count), int(n) + 1 + len(free), 1 + int(m_ub) + 2 * int(m_eq) + k)
        return ms.value

    def _check(self, i):
        if self.shape is None or not 0 <= i < self.shape[0]:
            raise NativeError("LpDense: no such LP in the last solve: %r" % (i,))
        return self.shape[1], self.shape[2]

    def solution(self, i):
        """(col0, positionOfVariable, variableAtPosition) of LP i of the last solve, copied to the host."""
        w, h = self._check(i)
        col0 = np.empty(h, np.float64)
        pos, var = np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        lpdense_check(lpdense_lib().yalps_lpdense_solution(self.handle, i, col0.ctypes.data, pos.ctypes.data, var.ctypes.data))
        return col0, pos, var

    def tableau(self, i):
        """The whole final matrix of LP i of the last solve (solve(..., keep_tableaux=True)), flat row-major, on the host."""
        w, h = self._check(i)
        m = np.empty(w * h, np.float64)
        lpdense_check(lpdense_lib().yalps_lpdense_tableau(self.handle, i, m.ctypes.data))
        return m

    def info(self):
        """{"launches", "reruns", "rerun_lps": [...], "kernels": [{kernel, class, aux, lps, grid, lds, pass, hist_cap}], "text"}"""
        return _batch_info(_info_text("yalps_lpdense", self.handle))

    def close(self):
        if self.handle:
            lpdense_lib().yalps_lpdense_destroy(self.handle)
            self.handle = C.c_void_p()


# ---------------------------------------------------------------------------------------------- libyalps_milpbatch.so

# yalps_milpbatch_eval_fn / yalps_milpbatch_consumed_fn
MILP_EVAL_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                           C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32))
MILP_CONSUMED_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_double))


_BATCH_LIBS["yalps_milpbatch"] = (MILPBATCH_LIB_PATH, {
        "roots": (_I32, [_VP, _I32] + [_VP] * 12), "root": (_I32, [_VP, _I32, _VP, _VP, _VP, _VP]),
        "nodes": (_I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP]),
        "validate_nodes": (_I32, [_I32, _VP, _VP, _I32, _VP, _VP, _VP]), "node": (_I32, [_VP, _I32, _VP, _VP, _VP]),
        "node_tableau": (_I32, [_VP, _I32, _VP]), "solve": (_I32, [_VP, _I32] + [_VP] * 15 + [_I32, _VP, _VP, _VP, _VP]),
        "validate": (_I32, [_I32, _VP, _VP, _VP, _VP, _I32]), "solution": (_I32, [_VP, _I32, C.POINTER(_I32), _VP, _VP, _VP]),
        "search": (_I32, [_I32] + [_VP] * 14 + [_I32, MILP_EVAL_FN, MILP_CONSUMED_FN, _VP] + [_VP] * 8)})


def milpbatch_lib():
    return _load_lib("yalps_milpbatch")


def milpbatch_check(rc):
    return _check("yalps_milpbatch", rc)


class PackedMilps:
    """A batch of models with integers as yalps_milpbatch_solve takes it: PackedLps for the root LPs plus, per model, the integer
    variables, the objective sign and the branch-and-cut options."""

    def __init__(self, milps):
        """milps: a sequence of (width, height, row, col, val, integers, sign, options) with the reference's option keys
        (precision, maxPivots, checkCycles, tolerance, timeout, maxIterations)."""
        n = len(milps)
        self.lps = PackedLps([(m[0], m[1], m[2], m[3], m[4], m[7]["precision"], m[7]["maxPivots"], m[7]["checkCycles"]) for m in milps])
        self.count = n
        self.n_integers = np.fromiter((len(m[5]) for m in milps), np.int64, n)
        self.int_offsets = np.zeros(n + 1, np.int64)
        self.int_offsets[1:] = np.cumsum(self.n_integers)
        self.integers = np.ascontiguousarray(np.concatenate([np.asarray(m[5], np.int32) for m in milps]) if n else np.zeros(0), np.int32)
        f = lambda get: np.fromiter((float(get(m)) for m in milps), np.float64, n)
        self.sign = f(lambda m: m[6])
        self.tolerance, self.timeout = f(lambda m: m[7]["tolerance"]), f(lambda m: m[7]["timeout"])
        self.max_iterations = f(lambda m: m[7]["maxIterations"])

    def validate(self, node_batch=1):
        """The argument checks of yalps_milpbatch_solve on the integers and the node sizes, on the host."""
        milpbatch_check(milpbatch_lib().yalps_milpbatch_validate(self.count, self.lps.width.ctypes.data, self.lps.height.ctypes.data,
                                                                 self.int_offsets.ctypes.data, self.integers.ctypes.data, int(node_batch)))


def _pack_cuts(cut_lists):
    """cut_lists: per node a sequence of (sign, variable, value) -> (offsets, sign, var, val) as the C ABI takes them."""
    off = np.zeros(len(cut_lists) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in cut_lists])
    flat = [c for cuts in cut_lists for c in cuts]
    return (off, np.array([c[0] for c in flat], np.int32), np.array([c[1] for c in flat], np.int32),
            np.array([c[2] for c in flat], np.float64))


def milp_validate_nodes(root_width, root_height, root_index, cut_lists):
    """The argument checks of yalps_milpbatch_nodes against roots of the given shapes, on the host (raises NativeError naming the node)."""
    rw, rh = np.ascontiguousarray(root_width, np.int32), np.ascontiguousarray(root_height, np.int32)
    ri = np.ascontiguousarray(root_index, np.int32)
    off, _, var, _ = cut_lists if isinstance(cut_lists, tuple) else _pack_cuts(cut_lists)
    milpbatch_check(milpbatch_lib().yalps_milpbatch_validate_nodes(rw.size, rw.ctypes.data, rh.ctypes.data, ri.size, ri.ctypes.data,
                                                                   off.ctypes.data, var.ctypes.data))


class MilpBatch:
    """Many independent MILPs per call (yalps_milpbatch_*): a root pass that keeps every optimal root on the device, node passes
    over nodes of any mix of roots, and the lockstep branch and cut over both.  Belongs to one thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        milpbatch_check(milpbatch_lib().yalps_milpbatch_create(device, C.c_void_p(stream) if stream is not None else None,
                                                               C.byref(self.handle)))
        self.root_shapes, self.node_shapes, self.packed = None, None, None

    def roots(self, lps):
        """lps: a PackedLps or the sequence it is made from.  Returns (status names, results, pivot counts)."""
        p = lps if isinstance(lps, PackedLps) else PackedLps(lps)
        n = p.count
        st, res, piv = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int64)
        self.root_shapes = self.node_shapes = self.packed = None
        milpbatch_check(milpbatch_lib().yalps_milpbatch_roots(
            self.handle, n, p.width.ctypes.data, p.height.ctypes.data, p.offsets.ctypes.data, p.row.ctypes.data, p.col.ctypes.data,
            p.val.ctypes.data, p.precision.ctypes.data, p.max_pivots.ctypes.data, p.check_cycles.ctypes.data, st.ctypes.data,
            res.ctypes.data, piv.ctypes.data))
        self.root_shapes = (p.width.copy(), p.height.copy())
        return [STATUS[k] for k in st], res, piv

    def root(self, i, matrix=False):
        """(col0, positionOfVariable, variableAtPosition[, matrix]) of root i of the last root pass."""
        if self.root_shapes is None or not 0 <= i < self.root_shapes[0].size:
            raise NativeError("MilpBatch: no such root in the last root pass: %r" % (i,))
        w, h = int(self.root_shapes[0][i]), int(self.root_shapes[1][i])
        col0, pos, var = np.empty(h, np.float64), np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        m = np.empty(w * h, np.float64) if matrix else None
        milpbatch_check(milpbatch_lib().yalps_milpbatch_root(self.handle, i, col0.ctypes.data, pos.ctypes.data, var.ctypes.data,
                                                             m.ctypes.data if matrix else None))
        return (col0, pos, var, m) if matrix else (col0, pos, var)

    def nodes(self, root_index, cut_lists, max_pivots=None, keep_tableaux=False):
        """Node k = root root_index[k] of the last root pass + cut_lists[k] ((sign, variable, value) each).  max_pivots: None =
        each root's own, else one budget per node.  Returns (status names, results, pivot counts, heights)."""
        if self.root_shapes is None:
            raise NativeError("MilpBatch.nodes: no root pass to build nodes on")
        ri = np.ascontiguousarray(root_index, np.int32)
        off, sg, vr, vl = _pack_cuts(cut_lists)
        n = ri.size
        assert off.size == n + 1
        mp = None if max_pivots is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_pivots, np.float64), (n,)))
        st, res, piv, hg = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n, np.int32)
        self.node_shapes = None
        milpbatch_check(milpbatch_lib().yalps_milpbatch_nodes(
            self.handle, n, ri.ctypes.data, off.ctypes.data, sg.ctypes.data, vr.ctypes.data, vl.ctypes.data,
            mp.ctypes.data if mp is not None else None, int(bool(keep_tableaux)), st.ctypes.data, res.ctypes.data, piv.ctypes.data,
            hg.ctypes.data))
        self.node_shapes = (self.root_shapes[0][ri] if n else np.zeros(0, np.int32), hg)
        return [STATUS[k] for k in st], res, piv, hg

    def _node_shape(self, k):
        if self.node_shapes is None or not 0 <= k < self.node_shapes[1].size:
            raise NativeError("MilpBatch: no such node in the last node pass: %r" % (k,))
        return int(self.node_shapes[0][k]), int(self.node_shapes[1][k])

    def node(self, k):
        """(col0, positionOfVariable, variableAtPosition) of node k of the last node pass."""
        w, h = self._node_shape(k)
        col0, pos, var = np.empty(h, np.float64), np.empty(w + h, np.int32), np.empty(w + h, np.int32)
        milpbatch_check(milpbatch_lib().yalps_milpbatch_node(self.handle, k, col0.ctypes.data, pos.ctypes.data, var.ctypes.data))
        return col0, pos, var

    def node_tableau(self, k):
        """The whole final matrix of node k of the last node pass (nodes(..., keep_tableaux=True)), flat row-major."""
        w, h = self._node_shape(k)
        m = np.empty(w * h, np.float64)
        milpbatch_check(milpbatch_lib().yalps_milpbatch_node_tableau(self.handle, k, m.ctypes.data))
        return m

    def solve(self, milps, node_batch=8):
        """milps: a PackedMilps or the sequence it is made from.  Returns (status names, results, nodes used, nodes evaluated,
        {"rounds", "launches", "gpu_ms"})."""
        p = milps if isinstance(milps, PackedMilps) else PackedMilps(milps)
        n, lp = p.count, p.lps
        st, res, stats, call = np.empty(n, np.int32), np.empty(n, np.float64), np.zeros(2 * n, np.int64), np.zeros(3, np.int64)
        self.root_shapes = self.node_shapes = self.packed = None
        milpbatch_check(milpbatch_lib().yalps_milpbatch_solve(
            self.handle, n, lp.width.ctypes.data, lp.height.ctypes.data, lp.offsets.ctypes.data, lp.row.ctypes.data, lp.col.ctypes.data,
            lp.val.ctypes.data, p.int_offsets.ctypes.data, p.integers.ctypes.data, p.sign.ctypes.data, lp.precision.ctypes.data,
            lp.max_pivots.ctypes.data, lp.check_cycles.ctypes.data, p.tolerance.ctypes.data, p.timeout.ctypes.data,
            p.max_iterations.ctypes.data, int(node_batch), st.ctypes.data, res.ctypes.data, stats.ctypes.data, call.ctypes.data))
        self.packed = p
        self.root_shapes = (lp.width.copy(), lp.height.copy())
        return ([STATUS[k] for k in st], res, stats[0::2].copy(), stats[1::2].copy(),
                {"rounds": int(call[0]), "launches": int(call[1]), "gpu_ms": call[2] / 1000.0})

    def solution(self, i):
        """(height, col0, positionOfVariable, variableAtPosition) of the best tableau of model i of the last solve."""
        p = self.packed
        if p is None or not 0 <= i < p.count:
            raise NativeError("MilpBatch: no such model in the last solve: %r" % (i,))
        w, cap = int(p.lps.width[i]), int(p.lps.height[i]) + 2 * int(p.n_integers[i])
        col0, pos, var, h = np.empty(cap, np.float64), np.empty(w + cap, np.int32), np.empty(w + cap, np.int32), C.c_int32()
        milpbatch_check(milpbatch_lib().yalps_milpbatch_solution(self.handle, i, C.byref(h), col0.ctypes.data, pos.ctypes.data,
                                                                 var.ctypes.data))
        n = h.value
        return n, col0[:n].copy(), pos[:w + n].copy(), var[:w + n].copy()

    def info(self):
        """{"rounds", "launches", "reruns", "gpu_ms", "rerun_nodes": [k | (round, k)], "kernels": [{kernel, class, nodes | lps, grid,
        lds, pass, round, hist_cap}], "text"}"""
        text = _info_text("yalps_milpbatch", self.handle, first=1 << 14)
        head, kernels = _info_lines(text)
        ids = [x for x in head.get("rerun_nodes", "[]").strip("[]").split(",") if x]
        return {"rounds": int(head.get("rounds", 0)), "launches": int(head.get("launches", 0)), "reruns": int(head.get("reruns", 0)),
                "gpu_ms": int(head.get("gpu_us", 0)) / 1000.0,
                "rerun_nodes": [tuple(int(y) for y in x.split(":")) if ":" in x else int(x) for x in ids], "kernels": kernels, "text": text}

    def close(self):
        if self.handle:
            milpbatch_lib().yalps_milpbatch_destroy(self.handle)
            self.handle = C.c_void_p()


def milp_search(roots, evaluate, node_batch=8, consumed=None):
    """The lockstep branch and cut of yalps_milpbatch_solve with `evaluate` as its node evaluator (host only, no device).
    roots: per model (width, height, status name, result, col0, pos, var, integers, sign, options) -- the root solved.
    evaluate(nodes) with nodes = [(model index, [(sign, variable, value)])] returns per node (status name, result, col0, pos,
    var) (the last three are read of optimal nodes only).  consumed(model, eval, cuts), optional, sees every node a tree
    consumes, in its pop order.  Returns per model (status name, result, height, col0, pos, var, nodes used, nodes evaluated)
    and the number of rounds."""
    n = len(roots)
    i32 = lambda it: np.ascontiguousarray(np.fromiter(it, np.int32, n))
    f64 = lambda it: np.ascontiguousarray(np.fromiter((float(x) for x in it), np.float64, n))
    width, height = i32(r[0] for r in roots), i32(r[1] for r in roots)
    rstatus, rresult = i32(STATUS.index(r[2]) for r in roots), f64(r[3] for r in roots)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(r[k], dt) for r in roots]), dt) if n else np.zeros(0, dt)
    rcol0, rpos, rvar = cat(4, np.float64), cat(5, np.int32), cat(6, np.int32)
    nints = np.fromiter((len(r[7]) for r in roots), np.int64, n)
    ioff = np.zeros(n + 1, np.int64)
    ioff[1:] = np.cumsum(nints)
    ints = cat(7, np.int32)
    sign = f64(r[8] for r in roots)
    prec, tol = f64(r[9]["precision"] for r in roots), f64(r[9]["tolerance"] for r in roots)
    tmo, mit = f64(r[9]["timeout"] for r in roots), f64(r[9]["maxIterations"] for r in roots)
    failure = []

    def c_eval(user, count, model, off, sg, vr, vl, status, result, hout, col0, pos, var):
        try:
            nodes = [(model[k], [(sg[c], vr[c], vl[c]) for c in range(off[k], off[k + 1])]) for k in range(count)]
            at0 = atp = 0
            for k, ((m, cuts), (st, res, c0, p, v)) in enumerate(zip(nodes, evaluate(nodes))):
                h, w = int(height[m]) + len(cuts), int(width[m])
                status[k], result[k], hout[k] = STATUS.index(st), res, h
                if st == "optimal":
                    hout[k] = len(c0)  # (a node of another height is refused by the driver)
                    for j in range(min(h, len(c0))):
                        col0[at0 + j] = c0[j]
                    for j in range(min(w + h, len(p), len(v))):
                        pos[atp + j], var[atp + j] = p[j], v[j]
                at0, atp = at0 + h, atp + w + h
            return 0
        except BaseException as e:  # (no exception may cross the C frames)
            failure.append(e)
            return -1

    def c_consumed(user, model, ev, ncuts, sg, vr, vl):
        try:
            consumed(model, ev, [(sg[c], vr[c], vl[c]) for c in range(ncuts)])
        except BaseException as e:
            failure.append(e)

    caps = height.astype(np.int64) + 2 * nints
    c0_off, p_off = np.concatenate([[0], np.cumsum(caps)]), np.concatenate([[0], np.cumsum(caps + width)])
    st, res, hg = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int32)
    col0, pos, var = np.zeros(int(c0_off[-1]), np.float64), np.zeros(int(p_off[-1]), np.int32), np.zeros(int(p_off[-1]), np.int32)
    stats, rounds = np.zeros(2 * n, np.int64), C.c_int64()
    rc = milpbatch_lib().yalps_milpbatch_search(
        n, width.ctypes.data, height.ctypes.data, rstatus.ctypes.data, rresult.ctypes.data, rcol0.ctypes.data, rpos.ctypes.data,
        rvar.ctypes.data, ioff.ctypes.data, ints.ctypes.data, sign.ctypes.data, prec.ctypes.data, tol.ctypes.data, tmo.ctypes.data,
        mit.ctypes.data, int(node_batch), MILP_EVAL_FN(c_eval), MILP_CONSUMED_FN(c_consumed) if consumed else MILP_CONSUMED_FN(),
        None, st.ctypes.data, res.ctypes.data, hg.ctypes.data, col0.ctypes.data, pos.ctypes.data, var.ctypes.data, stats.ctypes.data,
        C.addressof(rounds))
    if failure:
        raise failure[0]
    milpbatch_check(rc)
    out = []
    for i in range(n):
        h, w = int(hg[i]), int(width[i])
        out.append((STATUS[st[i]], float(res[i]), h, col0[c0_off[i]:c0_off[i] + h].copy(), pos[p_off[i]:p_off[i] + w + h].copy(),
                    var[p_off[i]:p_off[i] + w + h].copy(), int(stats[2 * i]), int(stats[2 * i + 1])))
    return out, rounds.value


# ---------------------------------------------------------------------------------------------- libyalps_milptree.so

_BATCH_LIBS["yalps_milptree"] = (MILPTREE_LIB_PATH, {
        "solve": (_I32, [_VP, _I32] + [_VP] * 15 + [_I32, _VP, _VP, _VP, _VP]), "validate": (_I32, [_I32, _VP, _VP, _VP, _VP, _VP]),
        "solution": (_I32, [_VP, _I32, C.POINTER(_I32), _VP, _VP, _VP]), "trace": (_I32, [_VP, _I32, C.POINTER(_I32)] + [_VP] * 8),
        "search": (_I32, [_I32] + [_VP] * 14 + [_I32, _I32, MILP_EVAL_FN, MILP_CONSUMED_FN, _VP] + [_VP] * 8)})
STATUS_MILPTREE = STATUS + ("overflow",)  # YALPS_MILPTREE_OVERFLOW: the tree's frontier outgrew the largest arena


def milptree_lib():
    return _load_lib("yalps_milptree")


def milptree_check(rc):
    return _check("yalps_milptree", rc)


def milptree_validate(packed):
    """The argument checks of yalps_milptree_solve on the integers, the node sizes and the timeouts, on the host."""
    milptree_check(milptree_lib().yalps_milptree_validate(packed.count, packed.lps.width.ctypes.data, packed.lps.height.ctypes.data,
                                                          packed.int_offsets.ctypes.data, packed.integers.ctypes.data,
                                                          packed.timeout.ctypes.data))


class MilpTree:
    """Many independent MILPs per call, every branch-and-cut tree walked on the device (yalps_milptree_*): a root pass, then one
    launch of milp_tree_kernel per (size class, checkCycles) pair.  Belongs to one thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        milptree_check(milptree_lib().yalps_milptree_create(device, C.c_void_p(stream) if stream is not None else None,
                                                            C.byref(self.handle)))
        self.packed, self.trace_cap = None, 0

    def solve(self, milps, trace_cap=0):
        """milps: a PackedMilps or the sequence it is made from.  Returns (status names -- "overflow" among them --, results,
        nodes used, the sums of the nodes' pivots, {"reruns", "launches", "gpu_ms"})."""
        p = milps if isinstance(milps, PackedMilps) else PackedMilps(milps)
        n, lp = p.count, p.lps
        st, res, stats, call = np.empty(n, np.int32), np.empty(n, np.float64), np.zeros(2 * n, np.int64), np.zeros(3, np.int64)
        self.packed = None
        milptree_check(milptree_lib().yalps_milptree_solve(
            self.handle, n, lp.width.ctypes.data, lp.height.ctypes.data, lp.offsets.ctypes.data, lp.row.ctypes.data, lp.col.ctypes.data,
            lp.val.ctypes.data, p.int_offsets.ctypes.data, p.integers.ctypes.data, p.sign.ctypes.data, lp.precision.ctypes.data,
            lp.max_pivots.ctypes.data, lp.check_cycles.ctypes.data, p.tolerance.ctypes.data, p.timeout.ctypes.data,
            p.max_iterations.ctypes.data, int(trace_cap), st.ctypes.data, res.ctypes.data, stats.ctypes.data, call.ctypes.data))
        self.packed, self.trace_cap = p, int(trace_cap)
        return ([STATUS_MILPTREE[k] for k in st], res, stats[0::2].copy(), stats[1::2].copy(),
                {"reruns": int(call[0]), "launches": int(call[1]), "gpu_ms": call[2] / 1000.0})

    def _model(self, i):
        p = self.packed
        if p is None or not 0 <= i < p.count:
            raise NativeError("MilpTree: no such model in the last solve: %r" % (i,))
        return int(p.lps.width[i]), int(p.lps.height[i]), int(p.n_integers[i])

    def solution(self, i):
        """(height, col0, positionOfVariable, variableAtPosition) of the best tableau of model i of the last solve."""
        w, h0, ni = self._model(i)
        cap = h0 + 2 * ni
        col0, pos, var, h = np.empty(cap, np.float64), np.empty(w + cap, np.int32), np.empty(w + cap, np.int32), C.c_int32()
        milptree_check(milptree_lib().yalps_milptree_solution(self.handle, i, C.byref(h), col0.ctypes.data, pos.ctypes.data,
                                                              var.ctypes.data))
        n = h.value
        return n, col0[:n].copy(), pos[:w + n].copy(), var[:w + n].copy()

    def trace(self, i):
        """The first trace_cap nodes model i consumed, in pop order: [{"eval", "cuts": [(sign, variable, value)], "status",
        "result", "n_pivots", "height"}]."""
        w, h0, ni = self._model(i)
        cap, room = self.trace_cap, max(1, self.trace_cap * 2 * ni)
        ev, res = np.empty(cap, np.float64), np.empty(cap, np.float64)
        st, hg, piv, cnt = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64), C.c_int32()
        sg, vr, vl = np.empty(room, np.int32), np.empty(room, np.int32), np.empty(room, np.float64)
        milptree_check(milptree_lib().yalps_milptree_trace(self.handle, i, C.byref(cnt), ev.ctypes.data, st.ctypes.data, res.ctypes.data,
                                                           piv.ctypes.data, hg.ctypes.data, sg.ctypes.data, vr.ctypes.data, vl.ctypes.data))
        out, c = [], 0
        for k in range(cnt.value):
            nc = int(hg[k]) - h0
            out.append({"eval": float(ev[k]), "cuts": [(int(sg[c + q]), int(vr[c + q]), float(vl[c + q])) for q in range(nc)],
                        "status": STATUS[st[k]], "result": float(res[k]), "n_pivots": int(piv[k]), "height": int(hg[k])})
            c += nc
        return out

    def info(self):
        """{"launches", "reruns", "overflows", "gpu_ms", "rerun_trees": [...], "kernels": [{kernel, class, trees | lps, grid, lds,
        pass, hist_cap, arena}], "text"}"""
        text = _info_text("yalps_milptree", self.handle, first=1 << 14)
        head, kernels = _info_lines(text)
        ids = [int(x) for x in head.get("rerun_trees", "[]").strip("[]").split(",") if x]
        return {"launches": int(head.get("launches", 0)), "reruns": int(head.get("reruns", 0)), "overflows": int(head.get("overflows", 0)),
                "gpu_ms": int(head.get("gpu_us", 0)) / 1000.0, "rerun_trees": ids, "kernels": kernels, "text": text}

    def close(self):
        if self.handle:
            milptree_lib().yalps_milptree_destroy(self.handle)
            self.handle = C.c_void_p()


def milp_tree_search(roots, evaluate, arena=None, consumed=None, arena_max=None):
    """The search of yalps_milptree_solve -- the rules milp_tree_kernel runs -- on the host with `evaluate` as its node evaluator
    (no device).  roots, evaluate and consumed as milp_search takes them (evaluate sees one node per call); arena: heap entries
    of a tree's first arena (default 128), grown x 4 per rerun up to arena_max (default 65536), above which the tree's status is
    "overflow".  Returns per model (status name, result, height, col0, pos, var, nodes used, nodes evaluated) and the number of
    reruns."""
    n = len(roots)
    i32 = lambda it: np.ascontiguousarray(np.fromiter(it, np.int32, n))
    f64 = lambda it: np.ascontiguousarray(np.fromiter((float(x) for x in it), np.float64, n))
    width, height = i32(r[0] for r in roots), i32(r[1] for r in roots)
    rstatus, rresult = i32(STATUS.index(r[2]) for r in roots), f64(r[3] for r in roots)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(r[k], dt) for r in roots]), dt) if n else np.zeros(0, dt)
    rcol0, rpos, rvar = cat(4, np.float64), cat(5, np.int32), cat(6, np.int32)
    nints = np.fromiter((len(r[7]) for r in roots), np.int64, n)
    ioff = np.zeros(n + 1, np.int64)
    ioff[1:] = np.cumsum(nints)
    ints = cat(7, np.int32)
    sign = f64(r[8] for r in roots)
    prec, tol = f64(r[9]["precision"] for r in roots), f64(r[9]["tolerance"] for r in roots)
    tmo, mit = f64(r[9]["timeout"] for r in roots), f64(r[9]["maxIterations"] for r in roots)
    failure = []

    def c_eval(user, count, model, off, sg, vr, vl, status, result, hout, col0, pos, var):
        try:
            m = model[0]
            cuts = [(sg[c], vr[c], vl[c]) for c in range(off[0], off[1])]
            (st, res, c0, p, v), = evaluate([(m, cuts)])
            h, w = int(height[m]) + len(cuts), int(width[m])
            status[0], result[0], hout[0] = STATUS.index(st), res, h
            if st == "optimal":
                hout[0] = len(c0)  # (a node of another height is refused by the search)
                for j in range(min(h, len(c0))):
                    col0[j] = c0[j]
                for j in range(min(w + h, len(p), len(v))):
                    pos[j], var[j] = p[j], v[j]
            return 0
        except BaseException as e:  # (no exception may cross the C frames)
            failure.append(e)
            return -1

    def c_consumed(user, model, ev, ncuts, sg, vr, vl):
        try:
            consumed(model, ev, [(sg[c], vr[c], vl[c]) for c in range(ncuts)])
        except BaseException as e:
            failure.append(e)

    caps = height.astype(np.int64) + 2 * nints
    c0_off, p_off = np.concatenate([[0], np.cumsum(caps)]), np.concatenate([[0], np.cumsum(caps + width)])
    st, res, hg = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int32)
    col0, pos, var = np.zeros(int(c0_off[-1]), np.float64), np.zeros(int(p_off[-1]), np.int32), np.zeros(int(p_off[-1]), np.int32)
    stats, reruns = np.zeros(2 * n, np.int64), C.c_int64()
    first = 128 if arena is None else int(arena)
    rc = milptree_lib().yalps_milptree_search(
        n, width.ctypes.data, height.ctypes.data, rstatus.ctypes.data, rresult.ctypes.data, rcol0.ctypes.data, rpos.ctypes.data,
        rvar.ctypes.data, ioff.ctypes.data, ints.ctypes.data, sign.ctypes.data, prec.ctypes.data, tol.ctypes.data, tmo.ctypes.data,
        mit.ctypes.data, first, max(first, 65536) if arena_max is None else int(arena_max), MILP_EVAL_FN(c_eval),
        MILP_CONSUMED_FN(c_consumed) if consumed else MILP_CONSUMED_FN(), None, st.ctypes.data, res.ctypes.data, hg.ctypes.data,
        col0.ctypes.data, pos.ctypes.data, var.ctypes.data, stats.ctypes.data, C.addressof(reruns))
    if failure:
        raise failure[0]
    milptree_check(rc)
    out = []
    for i in range(n):
        h, w = int(hg[i]), int(width[i])
        out.append((STATUS_MILPTREE[st[i]], float(res[i]), h, col0[c0_off[i]:c0_off[i] + h].copy(), pos[p_off[i]:p_off[i] + w + h].copy(),
                    var[p_off[i]:p_off[i] + w + h].copy(), int(stats[2 * i]), int(stats[2 * i + 1])))
    return out, reruns.value


# ---------------------------------------------------------------------------------------------- libyalps_milpdense.so

_BATCH_LIBS["yalps_milpdense"] = (MILPDENSE_LIB_PATH, {
        "validate": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP]),
        "solve": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, C.c_double, C.c_double,
                         _I32, C.c_double, C.c_double, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
        "validate_bounds": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, _VP]),
        "solve_bounds": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, _VP, _I32,
                                C.c_double, C.c_double, _I32, C.c_double, C.c_double, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
        "validate_free": (_I32, [_I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, _VP, _I32, _VP]),
        "solve_free": (_I32, [_VP, _I32, _I32, _I32, _I32, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _DOP, _I32, _VP, _I32, _VP, _I32, _VP, _I32, _VP,
                              _I32, C.c_double, C.c_double, _I32, C.c_double, C.c_double, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
        "overflowed": (_I32, [_VP, _VP, _I32]),
        "solution": (_I32, [_VP, _I32, C.POINTER(_I32), C.POINTER(C.c_double), C.POINTER(_I32), _VP, _VP, _VP]),
        "trace": (_I32, [_VP, _I32, C.POINTER(_I32)] + [_VP] * 8)})


def milpdense_lib():
    return _load_lib("yalps_milpdense")


def milpdense_check(rc):
    return _check("yalps_milpdense", rc)


def _index_list(idx):
    return np.ascontiguousarray(np.asarray(list(idx), np.int64), np.int32)


def milpdense_validate(count, n, m_ub, m_eq, operands, integers=(), binaries=()):
    """The host-only argument checks of yalps_milpdense_solve (raises NativeError with the reason); operands as
    lpdense_validate takes them, integers / binaries: 0-based variable indices as the library takes them -- both ascending,
    `integers` holding every binary variable.  No pointer is dereferenced."""
    ops, ints, bins = _dense_operands(operands), _index_list(integers), _index_list(binaries)
    milpdense_check(milpdense_lib().yalps_milpdense_validate(int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops),
                                                             ints.size, ints.ctypes.data, bins.size, bins.ctypes.data))


def milpdense_validate_bounds(count, n, m_ub, m_eq, operands, integers=(), binaries=(), lb=None, ub=None, upper=()):
    """The host-only argument checks of yalps_milpdense_solve_bounds: milpdense_validate's with the height that counts the
    len(upper) bound rows, plus lb / ub ((ptr, batch, row, col) or None: absent) and the index list, which is ascending and
    names no binary variable."""
    ops, ints, bins = _dense_operands(operands), _index_list(integers), _index_list(binaries)
    lbp, ubp, k, idx = _dense_bounds(lb, ub, _index_list(upper))
    milpdense_check(milpdense_lib().yalps_milpdense_validate_bounds(
        int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops), lbp, ubp, k, idx.ctypes.data, ints.size, ints.ctypes.data,
        bins.size, bins.ctypes.data))


def milpdense_validate_free(count, n, m_ub, m_eq, operands, integers=(), binaries=(), lb=None, ub=None, upper=(), free=()):
    """The host-only argument checks of yalps_milpdense_solve_free: milpdense_validate_bounds' with the width that counts the
    len(free) twin columns and the largest node that counts the cuts of the free integer variables' twins, plus the index list
    of the free variables, which is ascending and names no binary variable."""
    ops, ints, bins = _dense_operands(operands), _index_list(integers), _index_list(binaries)
    lbp, ubp, k, idx = _dense_bounds(lb, ub, _index_list(upper))
    fidx = _index_list(free)
    milpdense_check(milpdense_lib().yalps_milpdense_validate_free(
        int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops), lbp, ubp, k, idx.ctypes.data, fidx.size, fidx.ctypes.data,
        ints.size, ints.ctypes.data, bins.size, bins.ctypes.data))


class MilpDense:
    """Batches of dense MILPs of one shape, operands and answers in device memory, every tree walked on the device
    (yalps_milpdense_*).  Pointers are plain integers (a tensor's data_ptr()); nothing here imports torch.  Belongs to one
    thread at a time."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        milpdense_check(milpdense_lib().yalps_milpdense_create(device, C.c_void_p(stream) if stream is not None else None,
                                                               C.byref(self.handle)))
        self.shape, self.trace_cap = None, 0  # (count, width, root height, integer columns) of the last solve

    def solve(self, count, n, m_ub, m_eq, operands, integers=(), binaries=(), maximize=False, precision=1e-8, max_pivots=8192.0,
              check_cycles=False, tolerance=0.0, max_iterations=32768.0, trace_cap=0, x=None, objective=None, status=None,
              nodes=None, node_pivots=None, root_pivots=None, lb=None, ub=None, upper=(), free=(), entry=None):
        """operands = (c, A_ub, b_ub, A_eq, b_eq) as LpDense.solve takes them; integers / binaries: ascending 0-based variable
        indices, `integers` the union of both sets; lb / ub: (device pointer, batch, row, col) of the bounds x >= lb and
        x[j] <= ub[j] for the ascending indices j of `upper` (a host sequence that names no binary variable), or None -- with lb
        or ub given the call is yalps_milpdense_solve_bounds, and the root is len(upper) rows taller; free: the ascending indices
        of the variables without a lower bound (a host sequence that names no binary variable) -- with any the call is
        yalps_milpdense_solve_free, with or without lb / ub, the tableau is len(free) columns wider and the twins of the free
        integer variables are integer columns too; entry="free" takes that entry point whatever `free` holds; x / objective / status / nodes / node_pivots / root_pivots: device pointers
        of contiguous float64 [count][n], float64 [count], int32 [count] and three int64 [count], or None.  The outputs are
        complete on return.  Returns {"reruns", "launches", "overflows", "root_ms", "tree_ms", "epilogue_ms", "gpu_ms"}."""
        ops, ints, bins = _dense_operands(operands), _index_list(integers), _index_list(binaries)
        call = np.zeros(6, np.int64)
        self.shape = None
        head = (self.handle, int(count), int(n), int(m_ub), int(m_eq), *(C.byref(o) for o in ops))
        tail = (ints.size, ints.ctypes.data, bins.size, bins.ctypes.data, int(bool(maximize)), float(precision), float(max_pivots),
                int(bool(check_cycles)), float(tolerance), float(max_iterations), int(trace_cap), x, objective, status, nodes, node_pivots,
                root_pivots, call.ctypes.data)
        k = 0
        fidx = _index_list(free)
        if fidx.size or entry == "free":
            lbp, ubp, k, idx = _dense_bounds(lb, ub, _index_list(upper))
            milpdense_check(milpdense_lib().yalps_milpdense_solve_free(*head, lbp, ubp, k, idx.ctypes.data, fidx.size, fidx.ctypes.data, *tail))
        elif lb is not None or ub is not None:
            lbp, ubp, k, idx = _dense_bounds(lb, ub, _index_list(upper))
            milpdense_check(milpdense_lib().yalps_milpdense_solve_bounds(*head, lbp, ubp, k, idx.ctypes.data, *tail))
        elif len(upper):
            raise NativeError("MilpDense.solve: upper without lb or ub")
        else:
            milpdense_check(milpdense_lib().yalps_milpdense_solve(*head, *tail))
        twins = len(set(fidx.tolist()) & set(ints.tolist()))
        self.shape = (int(count), int(n) + 1 + fidx.size, 1 + int(m_ub) + 2 * int(m_eq) + k + bins.size, ints.size + twins)
        self.trace_cap = int(trace_cap)
        root, tree, epi = (call[k] / 1000.0 for k in (3, 4, 5))
        return {"reruns": int(call[0]), "launches": int(call[1]), "overflows": int(call[2]), "root_ms": root, "tree_ms": tree,
                "epilogue_ms": epi, "gpu_ms": root + tree + epi}

    def overflowed(self):
        """The trees of the last solve whose frontier outgrew the largest arena (their rows hold NaN and the status 5)."""
        n = milpdense_check(milpdense_lib().yalps_milpdense_overflowed(self.handle, None, 0))
        ids = np.empty(n, np.int32)
        if n:
            milpdense_check(milpdense_lib().yalps_milpdense_overflowed(self.handle, ids.ctypes.data, n))
        return [int(i) for i in ids]

    def _model(self, i):
        if self.shape is None or not 0 <= i < self.shape[0]:
            raise NativeError("MilpDense: no such MILP in the last solve: %r" % (i,))
        return self.shape[1:]

    def solution(self, i):
        """(status name, result, height, col0, positionOfVariable, variableAtPosition) of MILP i of the last solve: the tree's
        status and result and its best tableau, copied to the host."""
        w, h0, ni = self._model(i)
        cap = h0 + 2 * ni
        col0, pos, var = np.empty(cap, np.float64), np.empty(w + cap, np.int32), np.empty(w + cap, np.int32)
        st, res, h = C.c_int32(), C.c_double(), C.c_int32()
        milpdense_check(milpdense_lib().yalps_milpdense_solution(self.handle, i, C.byref(st), C.byref(res), C.byref(h), col0.ctypes.data,
                                                                 pos.ctypes.data, var.ctypes.data))
        n = h.value
        return STATUS_MILPTREE[st.value], res.value, n, col0[:n].copy(), pos[:w + n].copy(), var[:w + n].copy()

    def trace(self, i):
        """The first trace_cap nodes MILP i consumed, in pop order, as MilpTree.trace gives them."""
        w, h0, ni = self._model(i)
        cap, room = self.trace_cap, max(1, self.trace_cap * 2 * ni)
        ev, res = np.empty(cap, np.float64), np.empty(cap, np.float64)
        st, hg, piv, cnt = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64), C.c_int32()
        sg, vr, vl = np.empty(room, np.int32), np.empty(room, np.int32), np.empty(room, np.float64)
        milpdense_check(milpdense_lib().yalps_milpdense_trace(self.handle, i, C.byref(cnt), ev.ctypes.data, st.ctypes.data, res.ctypes.data,
                                                              piv.ctypes.data, hg.ctypes.data, sg.ctypes.data, vr.ctypes.data, vl.ctypes.data))
        out, c = [], 0
        for k in range(cnt.value):
            nc = int(hg[k]) - h0
            out.append({"eval": float(ev[k]), "cuts": [(int(sg[c + q]), int(vr[c + q]), float(vl[c + q])) for q in range(nc)],
                        "status": STATUS[st[k]], "result": float(res[k]), "n_pivots": int(piv[k]), "height": int(hg[k])})
            c += nc
        return out

    def info(self):
        """{"launches", "reruns", "overflows", "gpu_ms", "root_ms", "tree_ms", "epilogue_ms", "rerun_lps": [...], "rerun_trees":
        [...], "kernels": [{kernel, class, lps | trees, grid, lds, pass, hist_cap[, aux | arena]}], "text"}"""
        text = _info_text("yalps_milpdense", self.handle, first=1 << 14)
        head, kernels = _info_lines(text)
        ids = lambda key: [int(x) for x in head.get(key, "[]").strip("[]").split(",") if x]
        out = {k: int(head.get(k, 0)) for k in ("launches", "reruns", "overflows")}
        out.update({k + "_ms": int(head.get(k + "_us", 0)) / 1000.0 for k in ("gpu", "root", "tree", "epilogue")})
        out.update(rerun_lps=ids("rerun_lps"), rerun_trees=ids("rerun_trees"), kernels=kernels, text=text)
        return out

    def close(self):
        if self.handle:
            milpdense_lib().yalps_milpdense_destroy(self.handle)
            self.handle = C.c_void_p()
