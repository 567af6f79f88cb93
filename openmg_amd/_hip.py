"""ctypes binding of libopenmg_hip.so (C ABI: include/openmg_hip.h).

There is deliberately NO fallback: if the shared library is missing, or no MI355X is
visible when a compute entry point is called, an exception is raised.
"""
import ctypes
import os

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMG_LIB_PATH") or os.path.join(_HERE, "lib", "libopenmg_hip.so")   # override: kernel A/B builds

OMG_OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_SINGULAR, ERR_NO_DIAGONAL, ERR_ALLOC, ERR_UNSUPPORTED = range(1, 8)
SMOOTH_GS_LEX, SMOOTH_GS_COLOUR, SMOOTH_JACOBI = 0, 1, 2
# zebra line smoother: the strongest axis of level 0 (LINE), or lines along the axis named by stride — X unit stride, Z slowest
SMOOTH_LINE, SMOOTH_LINE_X, SMOOTH_LINE_Y, SMOOTH_LINE_Z = 3, 4, 5, 6
# ... OR-ed onto one of those four (11 .. 14): the smoothed levels may be periodic — wrapped neighbours across the lines, cyclic lines along them
SMOOTH_LINE_WRAP = 8
PROFILE_CLASSES = 7
PROFILE_NAMES = ("smoother_set_sweep", "residual", "restrict", "prolong_add", "residual_norm", "plane_down", "plane_up")

SMOOTHERS = {
    "gs": SMOOTH_GS_LEX, "lex": SMOOTH_GS_LEX, "gauss-seidel": SMOOTH_GS_LEX, "gaussSeidel": SMOOTH_GS_LEX,
    "colour": SMOOTH_GS_COLOUR, "color": SMOOTH_GS_COLOUR, "rbgs": SMOOTH_GS_COLOUR,
    "red-black": SMOOTH_GS_COLOUR, "multicolour": SMOOTH_GS_COLOUR,
    "jacobi": SMOOTH_JACOBI, "weighted-jacobi": SMOOTH_JACOBI,
    "line": SMOOTH_LINE, "line-gs": SMOOTH_LINE,
    "line-periodic": SMOOTH_LINE | SMOOTH_LINE_WRAP,
}


class HipError(RuntimeError):
    """A libopenmg_hip.so call failed; .code holds the OMG_ERR_* value."""

    def __init__(self, code, message):
        super().__init__("libopenmg_hip: %s (code %d)" % (message, code))
        self.code = code


class CsrView(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int64), ("nnz", ctypes.c_int64),
                ("indptr", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("data", ctypes.c_void_p)]


class HierarchyOptions(ctypes.Structure):
    """omg_hierarchy_options in include/openmg_hip.h."""
    _fields_ = [("smoother", ctypes.c_int), ("omega", ctypes.c_double), ("dtype", ctypes.c_int), ("nullspace", ctypes.c_int)]


_P = ctypes.c_void_p
_I = ctypes.c_int
_D = ctypes.c_double
_PP = ctypes.POINTER(ctypes.c_void_p)
_CSR = ctypes.POINTER(CsrView)
_I64P = ctypes.POINTER(ctypes.c_int64)
_IP = ctypes.POINTER(ctypes.c_int)
_DP = ctypes.POINTER(ctypes.c_double)
_OPT = ctypes.POINTER(HierarchyOptions)

# name -> (restype, argtypes).  Must list EVERY symbol include/openmg_hip.h declares
# (tests/test_cabi_symbols.py checks that against the header).
SIGNATURES = {
    "omg_last_error": (ctypes.c_char_p, []),
    "omg_version": (ctypes.c_char_p, []),
    "omg_device_count": (_I, [_IP]),
    "omg_set_device": (_I, [_I]),
    "omg_hierarchy_create": (_I, [_I, _CSR, _CSR, _I, _D, _PP]),
    "omg_hierarchy_create_ex": (_I, [_I, _CSR, _CSR, _I, _D, _I, _PP]),
    "omg_hierarchy_create_from_fine": (_I, [_CSR, _I, _I64P, _I, _I, _D, _I, _PP]),
    "omg_hierarchy_create_opt": (_I, [_I, _CSR, _CSR, _OPT, _PP]),
    "omg_hierarchy_create_from_fine_opt": (_I, [_CSR, _I, _I64P, _I, _OPT, _PP]),
    "omg_hierarchy_nullspace": (_I, [_P, _IP]),
    "omg_level_project": (_I, [_P, _I, _P, _DP]),
    "omg_hierarchy_dtype": (_I, [_P, _IP]),
    "omg_hierarchy_update_fine": (_I, [_P, _P, ctypes.c_int64, _I]),
    "omg_hierarchy_can_update_fine": (_I, [_P, _IP]),
    "omg_kappa_assemble": (_I, [_I64P, _P, _I, _IP, _P, _I, _I, _DP, _P, _P, _P, _I]),
    "omg_hierarchy_create_from_kappa": (_I, [_I64P, _P, _I, _IP, _P, _I, _I, _DP, _I, _OPT, _PP]),
    "omg_hierarchy_update_kappa": (_I, [_P, _I64P, _P, _I, _IP, _P, _I, _I, _DP]),
    "omg_kappa_assemble_spaced": (_I, [_I64P, _P, _I, _IP, _P, _I, _I, _DP, _P, _P, _P, _P, _P, _P, _I]),
    "omg_hierarchy_create_from_kappa_spaced": (_I, [_I64P, _P, _I, _IP, _P, _I, _I, _DP, _P, _P, _P, _I, _OPT, _PP]),
    "omg_hierarchy_update_kappa_spaced": (_I, [_P, _I64P, _P, _I, _IP, _P, _I, _I, _DP, _P, _P, _P]),
    "omg_kappa_rhs": (_I, [_I64P, _P, _I, _IP, _DP, _P, _I, _I, _IP, _DP, _PP, _I, _P, _I]),
    "omg_kappa_rhs_spaced": (_I, [_I64P, _P, _I, _IP, _DP, _P, _P, _P, _P, _I, _I, _IP, _DP, _PP, _I, _P, _I]),
    "omg_kappa_flux": (_I, [_I64P, _P, _I, _IP, _DP, _P, _I, _IP, _DP, _PP, _I, _DP, _P, _P, _P, _I]),
    "omg_kappa_flux_spaced": (_I, [_I64P, _P, _I, _IP, _DP, _P, _P, _P, _P, _I, _IP, _DP, _PP, _I, _DP, _P, _P, _P, _I]),
    "omg_face_divergence": (_I, [_I64P, _P, _P, _P, _I, _P, _I]),
    "omg_faces_assemble": (_I, [_I64P, _P, _P, _P, _I, _IP, _P, _I, _I, _P, _P, _P, _I]),
    "omg_hierarchy_create_from_faces": (_I, [_I64P, _P, _P, _P, _I, _IP, _P, _I, _I, _I, _OPT, _PP]),
    "omg_hierarchy_update_faces": (_I, [_P, _I64P, _P, _P, _P, _I, _IP, _P, _I, _I]),
    "omg_faces_rhs": (_I, [_I64P, _P, _P, _P, _I, _IP, _P, _I, _I, _IP, _DP, _PP, _I, _P, _I]),
    "omg_faces_flux": (_I, [_I64P, _P, _P, _P, _I, _IP, _P, _I, _IP, _DP, _PP, _I, _DP, _P, _P, _P, _I]),
    "omg_resident_norms": (_I, [_P, _DP, _DP]),
    "omg_resident_projection": (_I, [_P, _I]),
    "omg_resident_project": (_I, [_P, _IP]),
    "omg_resident_project_update": (_I, [_P, _IP, _IP]),
    "omg_resident_projection_fetch": (_I, [_P, _I, _P]),
    "omg_resident_projection_time": (_I, [_P, _I, _DP, _DP, _DP]),
    "omg_hierarchy_destroy": (_I, [_P]),
    "omg_hierarchy_set_stream": (_I, [_P, _P]),
    "omg_hierarchy_sync": (_I, [_P]),
    "omg_hierarchy_level_rows": (_I, [_P, _I, _I64P]),
    "omg_hierarchy_level_sets": (_I, [_P, _I, _I64P]),
    "omg_hierarchy_set_info": (_I, [_P, _I, _I, _I64P, _I64P]),
    "omg_hierarchy_level_fused": (_I, [_P, _I, _IP]),
    "omg_hierarchy_level_flags": (_I, [_P, _I, _IP]),
    "omg_hierarchy_line_axis": (_I, [_P, _IP, _IP]),
    "omg_hierarchy_tail_info": (_I, [_P, _I64P]),
    "omg_hierarchy_use_plane": (_I, [_P, _I]),
    "omg_hierarchy_set_cycle": (_I, [_P, _I, _D]),
    "omg_hierarchy_get_cycle": (_I, [_P, _IP, _DP]),
    "omg_hierarchy_plane_info": (_I, [_P, _I, _I64P]),
    "omg_hierarchy_format_info": (_I, [_P, _I, _I, _I, _I64P]),
    "omg_format_selftest": (_I, [_CSR, _I, _I64P]),
    "omg_vcycle": (_I, [_P, _I, _P, _P, _I, _I, _DP]),
    "omg_vcycle_ex": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _DP]),
    "omg_vcycle_dev": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _DP]),
    "omg_resident_load_dev": (_I, [_P, _P, _P]),
    "omg_resident_fetch_dev": (_I, [_P, _P]),
    "omg_device_synchronize": (_I, []),
    "omg_device_mem_info": (_I, [_I64P, _I64P]),
    "omg_solve": (_I, [_P, _P, _P, _I, _I, _I, _D, _IP, _DP]),
    "omg_resident_load": (_I, [_P, _P, _P]),
    "omg_resident_cycle": (_I, [_P, _I, _I, _DP]),
    "omg_resident_cycles": (_I, [_P, _I, _I, _I, _DP]),
    "omg_resident_fetch": (_I, [_P, _P]),
    "omg_resident_spmv_time": (_I, [_P, _I, _DP]),
    "omg_resident_use_graph": (_I, [_P, _I]),
    "omg_resident_pcg": (_I, [_P, _I, _I, _I, _D, _IP, _DP, _DP, _IP]),
    "omg_profile_enable": (_I, [_P, _I]),
    "omg_profile_read": (_I, [_P, _I64P, _DP]),
    "omg_level_smooth": (_I, [_P, _I, _P, _P, _I]),
    "omg_level_residual": (_I, [_P, _I, _P, _P, _P, _DP]),
    "omg_level_spmv": (_I, [_P, _I, _P, _P]),
    "omg_level_spmv_dev": (_I, [_P, _I, _P, _P]),
    "omg_level_restrict": (_I, [_P, _I, _P, _P]),
    "omg_level_prolong_add": (_I, [_P, _I, _P, _P]),
    "omg_coarse_solve": (_I, [_P, _P, _P]),
    "omg_hierarchy_coarse_info": (_I, [_P, _I64P]),
    "omg_spmv": (_I, [_CSR, _P, _P]),
    "omg_residual": (_I, [_CSR, _P, _P, _P, _DP]),
    "omg_gauss_seidel": (_I, [_CSR, _P, _P, _I, _D, _I, _D, _IP]),
    "omg_direct_solve": (_I, [_CSR, _P, _P]),
    "omg_rap": (_I, [_CSR, _CSR, _PP, _I64P, _I64P, _I64P]),
    "omg_spgemm": (_I, [_CSR, _CSR, _PP, _I64P, _I64P, _I64P]),
    "omg_csr_result_fetch": (_I, [_P, _P, _P, _P]),
    "omg_csr_result_free": (_I, [_P]),
    "omg_restriction": (_I, [_I, _I64P, _P, _P, _P, _I64P, _I64P]),
    "omg_restriction_ex": (_I, [_I, _I64P, _IP, _P, _P, _P]),
    "omg_axis_couplings": (_I, [_CSR, _I, _I64P, _DP, _I64P]),
    "omg_semicoarsen_rule": (_I, [_I, _I64P, _DP, _I64P, _I, _I, _IP]),
    "omg_hierarchy_create_from_fine_semi": (_I, [_CSR, _I, _I64P, _I, _IP, ctypes.c_int64, _OPT, _PP]),
    "omg_hierarchy_coarsening": (_I, [_P, _I, _IP]),
    "omg_restriction_ragged": (_I, [_I, _I64P, _IP, _I, _P, _P, _P]),
    "omg_semicoarsen_rule_ragged": (_I, [_I, _I64P, _DP, _I64P, _I, _I, _I, _IP]),
    "omg_hierarchy_create_from_fine_ragged": (_I, [_CSR, _I, _I64P, _I, _IP, ctypes.c_int64, _I, _OPT, _PP]),
    "omg_host_checksum": (_I, [_P, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64)]),
    "omg_dist_create": (_I, [_I, _I, _I, _P, _CSR, _I64P, _I, _D, _PP]),
    "omg_dist_create_ex": (_I, [_I, _I, _I, _P, _CSR, _I64P, _I, _D, _I, _PP]),
    "omg_dist_destroy": (_I, [_P]),
    "omg_dist_set_tail": (_I, [_P, _P]),
    "omg_hierarchy_cycle_dev": (_I, [_P, _P, _P, _I, _I, _P]),
    "omg_dist_set_stream": (_I, [_P, _P]),
    "omg_dist_sync": (_I, [_P]),
    "omg_rccl_unique_id": (_I, [_P]),
    "omg_rccl_self_exchange_time": (_I, [ctypes.c_int64, _I, _DP]),
    "omg_pdist_create": (_I, [_I, _I, _I, _I, _I, _I, _P, _D, _PP]),
    "omg_pdist_destroy": (_I, [_P]),
    "omg_pdist_set_tail": (_I, [_P, _P]),
    "omg_pdist_connect": (_I, [_P, _P, _P]),
    "omg_peer_access": (_I, [_I, _I, _P]),
    "omg_pdist_p2p_handle_count": (_I, [_P, _P]),
    "omg_pdist_p2p_handles": (_I, [_P, _P, _I]),
    "omg_pdist_p2p_open": (_I, [_P, _I, _P, _I]),
    "omg_pdist_p2p_local": (_I, [_P, _P]),
    "omg_pdist_p2p_enable": (_I, [_P, _I]),
    "omg_pdist_p2p_status": (_I, [_P, _P]),
    "omg_pdist_p2p_layout": (_I, [_P, _I64P, _I, _IP, _I]),
    "omg_pdist_cycles_squares": (_I, [_P, _I, _P]),
    "omg_pdist_rccl_ranks": (_I, [_P, _IP]),
    "omg_pdist_load": (_I, [_P, _P, _P]),
    "omg_pdist_fetch": (_I, [_P, _P]),
    "omg_pdist_sync": (_I, [_P]),
    "omg_pdist_info": (_I, [_P, _I64P]),
    "omg_pdist_set_gate": (_I, [_P, _I]),
    "omg_pdist_trace": (_I, [_P, _I]),
    "omg_pdist_progress": (_I, [_P, ctypes.POINTER(ctypes.c_uint)]),
    "omg_pdist_cycles": (_I, [_P, _I, _P]),
    "omg_pdist_cycles_ex": (_I, [_P, _I, _I, _I, _P]),
    "omg_pdist_group_cycles_ex": (_I, [_P, _I, _I, _I, _P]),
    "omg_sdist_p2p_handle_count": (_I, [_P, _P]),
    "omg_sdist_p2p_handles": (_I, [_P, _P, _I]),
    "omg_sdist_p2p_open": (_I, [_P, _I, _P, _I]),
    "omg_sdist_p2p_local": (_I, [_P, _P]),
    "omg_sdist_p2p_enable": (_I, [_P, _I]),
    "omg_sdist_p2p_status": (_I, [_P, _P]),
    "omg_sdist_p2p_layout": (_I, [_P, _I64P, _I, _IP]),
    "omg_pdist_group_create": (_I, [_I, _P, _PP]),
    "omg_pdist_group_destroy": (_I, [_P]),
    "omg_pdist_group_cycles": (_I, [_P, _I, _P]),
    "omg_sdist_create": (_I, [_I, _I, _I, _I, _I, _I, _CSR, _D, _I, _PP]),
    "omg_sdist_destroy": (_I, [_P]),
    "omg_sdist_coarse_size": (_I, [_P, _I64P, _I64P, _I64P]),
    "omg_sdist_coarse_fetch": (_I, [_P, _P, _P, _P]),
    "omg_sdist_set_tail": (_I, [_P, _P]),
    "omg_sdist_connect": (_I, [_P, _P]),
    "omg_sdist_rccl_ranks": (_I, [_P, _IP]),
    "omg_sdist_info": (_I, [_P, _I, _I64P]),
    "omg_sdist_load": (_I, [_P, _P, _P]),
    "omg_sdist_fetch": (_I, [_P, _P]),
    "omg_sdist_sync": (_I, [_P]),
    "omg_sdist_cycles": (_I, [_P, _I, _I, _I, _P]),
    "omg_sdist_group_create": (_I, [_I, _P, _PP]),
    "omg_sdist_group_destroy": (_I, [_P]),
    "omg_sdist_group_cycles": (_I, [_P, _I, _I, _I, _P]),
    "omg_dist_connect": (_I, [_P, _P]),
    "omg_dist_rccl_ranks": (_I, [_P, _IP]),
    "omg_dist_load": (_I, [_P, _P, _P]),
    "omg_dist_fetch": (_I, [_P, _P]),
    "omg_dist_cycle": (_I, [_P, _I, _I, _DP]),
    "omg_dist_cycles": (_I, [_P, _I, _I, _I, _DP]),
    "omg_dist_spmv_time": (_I, [_P, _I, _DP]),
    "omg_dist_format_info": (_I, [_P, _I, _I, _I, _I64P]),
    "omg_dist_level_flags": (_I, [_P, _I, _IP]),
    "omg_dist_group_create": (_I, [_I, _PP, _PP]),
    "omg_dist_group_destroy": (_I, [_P]),
    "omg_dist_group_cycle": (_I, [_P, _I, _I, _DP]),
    "omg_dist_group_cycles": (_I, [_P, _I, _I, _I, _DP]),
}


class DistLevelView(ctypes.Structure):
    """omg_dist_level in include/openmg_hip.h."""
    _fields_ = [("A", CsrView), ("R", CsrView), ("n_halo", ctypes.c_int64),
                ("keys", ctypes.c_void_p), ("n_sets", ctypes.c_int32), ("n_peers", ctypes.c_int32),
                ("peers", ctypes.c_void_p), ("send_off", ctypes.c_void_p),
                ("send_idx", ctypes.c_void_p), ("recv_off", ctypes.c_void_p),
                ("set_group", ctypes.c_int32), ("entry_group", ctypes.c_void_p)]

_lib = None


def lib():
    """Load the shared library once.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C openmg_amd/csrc` (or __graft_entry__.build()). "
                "openmg_amd has no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code):
    if code != OMG_OK:
        raise HipError(code, lib().omg_last_error().decode("utf-8", "replace"))


def device_mem_info():
    """(free, total) bytes of the current device."""
    f, t = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().omg_device_mem_info(ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def device_count():
    n = ctypes.c_int(0)
    check(lib().omg_device_count(ctypes.byref(n)))
    return n.value


def require_gpu():
    if device_count() <= 0:
        raise HipError(ERR_NO_DEVICE, "no MI355X / HIP device visible; openmg_amd has no CPU fallback")


def smoother_code(kind):
    if isinstance(kind, int):
        return kind
    try:
        return SMOOTHERS[kind]
    except KeyError:
        raise ValueError("unknown smoother %r (choose from %s)" % (kind, sorted(set(SMOOTHERS))))


def is_line_smoother(code):
    """3 .. 6, and those with SMOOTH_LINE_WRAP: 11 .. 14 (7 and 15 are no codes)"""
    return isinstance(code, int) and not isinstance(code, bool) and 0 <= code < 16 and SMOOTH_LINE <= (code & ~SMOOTH_LINE_WRAP) <= SMOOTH_LINE_Z


def line_smoother_code(line_axis, shape, wrap=False):
    """The OMG_SMOOTH_LINE* code for parameters['lineAxis']: None / 'auto' (the strongest axis of level 0), or an index into
    problemShape = shape (C order: the last entry is the unit-stride axis X).  ValueError for anything else.  wrap: with
    SMOOTH_LINE_WRAP ('line-periodic')."""
    flag = SMOOTH_LINE_WRAP if wrap else 0
    if line_axis is None or (isinstance(line_axis, str) and line_axis == "auto"):
        return SMOOTH_LINE | flag
    dim = len(tuple(shape))
    if isinstance(line_axis, bool) or not isinstance(line_axis, (int, np.integer)) or not 0 <= int(line_axis) < dim or dim > 3:
        raise ValueError("lineAxis must be None, 'auto' or an index into problemShape (0 .. %d), not %r" % (dim - 1, line_axis))
    return (SMOOTH_LINE_X + (dim - 1 - int(line_axis))) | flag


CYCLE_V, CYCLE_F, CYCLE_W = 0, 1, 2
CYCLES = {"V": CYCLE_V, "F": CYCLE_F, "W": CYCLE_W}


def cycle_code(shape):
    """OMG_CYCLE_* for 'V' / 'F' / 'W' (or the code itself)."""
    if isinstance(shape, int) and not isinstance(shape, bool) and shape in CYCLES.values():
        return shape
    try:
        return CYCLES[shape]
    except (KeyError, TypeError):
        raise ValueError("unknown cycle shape %r (choose from 'V', 'F', 'W')" % (shape,))


def over_correction_of(value):
    """The over-correction factor as a float; ValueError unless it is finite and > 0."""
    try:
        alpha = float(value)
    except (TypeError, ValueError):
        raise ValueError("the over-correction factor must be a number, not %r" % (value,))
    if not np.isfinite(alpha) or alpha <= 0.0:
        raise ValueError("the over-correction factor must be finite and > 0, not %r" % (value,))
    return alpha


NULLSPACE_NONE, NULLSPACE_CONSTANT = 0, 1
NULLSPACES = {None: NULLSPACE_NONE, "constant": NULLSPACE_CONSTANT}


def nullspace_code(kind):
    """OMG_NULLSPACE_* for None / 'constant'; ValueError for anything else."""
    if kind is None or (isinstance(kind, str) and kind in NULLSPACES):
        return NULLSPACES[kind]
    raise ValueError("nullspace must be None or 'constant', not %r" % (kind,))


DTYPE_F64, DTYPE_F32, DTYPE_MIXED = 0, 1, 2


def dtype_code(dtype):
    """OMG_DTYPE_* for a numpy dtype / name; 'mixed' is OMG_DTYPE_MIXED (fp32 levels, fp64 outer state of level 0)."""
    if isinstance(dtype, int) and not isinstance(dtype, bool) and dtype in (DTYPE_F64, DTYPE_F32, DTYPE_MIXED):
        return dtype
    if isinstance(dtype, str) and dtype == "mixed":
        return DTYPE_MIXED
    dt = np.dtype(dtype)
    if dt == np.float64:
        return DTYPE_F64
    if dt == np.float32:
        return DTYPE_F32
    raise ValueError("dtype must be float64 or float32, not %r" % (dtype,))


def host_checksum(a):
    """64-bit digest of every byte of a NumPy array (omg_host_checksum: all host threads, no device)."""
    a = np.ascontiguousarray(a)
    out = ctypes.c_uint64(0)
    check(lib().omg_host_checksum(a.ctypes.data, a.nbytes, ctypes.byref(out)))
    return out.value


def as_csr(A):
    """CSR with int32 index arrays / float64 data; stored column order is kept as is."""
    if not sp.isspmatrix_csr(A):
        A = sp.csr_matrix(A)
    if A.nnz >= 2 ** 31 - 1 or max(A.shape) >= 2 ** 31 - 1:
        raise ValueError("operator too large for int32 indices; shard it first")
    if A.indptr.dtype != np.int32 or A.indices.dtype != np.int32 or A.data.dtype != np.float64 \
            or not (A.indptr.flags.c_contiguous and A.indices.flags.c_contiguous and A.data.flags.c_contiguous):
        A = sp.csr_matrix((np.ascontiguousarray(A.data, dtype=np.float64),
                           np.ascontiguousarray(A.indices, dtype=np.int32),
                           np.ascontiguousarray(A.indptr, dtype=np.int32)), shape=A.shape)
    return A


def csr_view(A):
    """(CsrView, keepalive) for a CSR matrix prepared by as_csr()."""
    v = CsrView(A.shape[0], A.shape[1], A.nnz, A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data)
    return v


def vec(x, n=None, copy=False):
    """Contiguous float64 1-D array (flattening (n,1) columns like the reference accepts)."""
    a = np.asarray(x, dtype=np.float64)
    a = a.reshape(-1)
    if copy or not a.flags.c_contiguous:
        a = np.array(a, dtype=np.float64, order="C", copy=True)
    if n is not None and a.size != n:
        raise ValueError("vector has %d entries, expected %d" % (a.size, n))
    return a


SIGMA_NONE, SIGMA_SCALAR, SIGMA_FIELD = 0, 1, 2


class KappaArgs:
    """The coefficient-field arguments of omg_kappa_assemble / omg_hierarchy_create_from_kappa / omg_hierarchy_update_kappa
    (include/openmg_hip.h) from what the Python entries take: kappa a float64 array (nz + 2, ny + 2, nx + 2), NumPy or a
    C-contiguous device array (__cuda_array_interface__); walls, sigma, scale as operators.stencil7_kappa takes them, sigma
    a device array too.  ValueError for what operators.kappa_arguments refuses — before any device work; the fields' values
    are checked by the kernel that reads them (HipError, ERR_INVALID, naming the cell).  spacing: None, or the cell widths
    (hz, hy, hx) of a stretched grid as operators.spacing_arguments takes them — host arrays, in place of scale.  .grid:
    problemShape; .shape: the operator's (n, n); .walls: the six codes (operators.WALL_CODES); .periodic: per axis (z, y, x)
    whether its walls are periodic; .nnz: the operator's entries; .spacing: the checked widths or None; .call: the C arguments of the
    *_spaced entries from `shape` to `hx` (three NULLs without widths: the entries without them); the object keeps the
    arrays alive."""

    def __init__(self, kappa, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), spacing=None):
        from . import _devarray, operators
        if isinstance(kappa, KappaArgs):           # (already checked: Hierarchy.from_kappa / update_kappa take one as it is)
            self.__dict__.update(kappa.__dict__)
            return
        k_dev = _devarray.is_device_array(kappa)
        if k_dev:
            k_shape = tuple(int(s) for s in kappa.__cuda_array_interface__["shape"])
        else:
            kappa = np.asarray(kappa)
            if kappa.dtype != np.float64:
                raise ValueError("kappa must be float64, not %s" % kappa.dtype)
            kappa = np.ascontiguousarray(kappa)
            k_shape = kappa.shape
        self.grid, self.walls, self.scale = operators.kappa_arguments(k_shape, walls, sigma, scale)
        self.spacing = None
        if spacing is not None:
            if not operators.unit_scale(self.scale):
                raise ValueError("spacing and scale exclude each other: the widths carry every factor")
            self.spacing = operators.spacing_arguments(self.grid, spacing)
        self.n = int(np.prod(self.grid))
        self.shape = (self.n, self.n)
        nz, ny, nx = self.grid
        self.periodic = operators.periodic_axes(self.walls)      # (z, y, x): along such an axis no neighbour is absent
        self.nnz = 7 * self.n - 2 * sum(self.n // e for e, wraps in zip(self.grid, self.periodic) if not wraps)
        if 7 * self.n >= 2 ** 31 - 1:
            raise ValueError("operator too large for int32 indices; shard it first")
        padded = int(np.prod(k_shape))
        s_dev = _devarray.is_device_array(sigma)
        if sigma is None:
            kind, s_ptr = SIGMA_NONE, None
        elif s_dev:
            kind, s_ptr = SIGMA_FIELD, _devarray.address(sigma, self.n, "sigma")
        elif np.ndim(sigma) == 0:
            sigma = np.array([float(sigma)], dtype=np.float64)
            kind, s_ptr = SIGMA_SCALAR, sigma.ctypes.data
        else:
            sigma = np.ascontiguousarray(sigma, dtype=np.float64)
            kind, s_ptr = SIGMA_FIELD, sigma.ctypes.data
        k_ptr = _devarray.address(kappa, padded, "kappa") if k_dev else kappa.ctypes.data
        self.on_device = k_dev or s_dev
        self._keep = (kappa, sigma)
        widths = (None,) * 3 if self.spacing is None else tuple(h.ctypes.data for h in self.spacing)
        self.call = ((ctypes.c_int64 * 3)(*self.grid), ctypes.c_void_p(k_ptr), int(k_dev), (ctypes.c_int * 6)(*self.walls),
                     ctypes.c_void_p(s_ptr), kind, int(s_dev), (ctypes.c_double * 3)(*self.scale)) + tuple(ctypes.c_void_p(p) for p in widths)

    def matrix(self):
        """The operator as a SciPy CSR in host memory, assembled on the device (kappa_assemble)."""
        indptr, indices, data = kappa_assemble(self)
        A = sp.csr_matrix((data, indices, indptr), shape=self.shape)
        A.has_sorted_indices = True
        return A

    def synchronize(self):
        """What the caller's library enqueued on the device arrays is complete before the library's own stream reads them."""
        if self.on_device:
            check(lib().omg_device_synchronize())


def kappa_assemble(kappa, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), pattern=True, out=None, spacing=None):
    """The 7-point operator of a coefficient field, assembled on the device (omg_kappa_assemble_spaced): the CSR arrays of
    operators.stencil7_kappa(kappa, walls, sigma, scale, spacing), bit for bit.  kappa, sigma: NumPy arrays or device arrays;
    spacing: host arrays.  walls may name 'periodic' for both walls of an axis: nnz and with it the sizes of `out` grow by
    2 n / extent per periodic axis (KappaArgs.nnz).
    Returns (indptr, indices, data) as NumPy arrays, indptr = indices = None with pattern=False (the values alone).
    out = (indptr, indices, data): device arrays to write into instead — int32 (n + 1), int32 (nnz), float64 (nnz); the
    first two None for the values alone — and returned as they are."""
    from . import _devarray
    a = KappaArgs(kappa, walls, sigma, scale, spacing)
    if out is not None:
        d_indptr, d_indices, d_data = out
        if (d_indptr is None) != (d_indices is None):
            raise ValueError("out: indptr and indices are given together or not at all")

        def int32_address(arr, count, what):
            iface = arr.__cuda_array_interface__
            if iface["typestr"] not in ("<i4", "=i4", "|i4") or iface.get("strides") is not None or tuple(iface["shape"]) != (count,):
                raise ValueError("out: %s must be a contiguous int32 device array of %d entries" % (what, count))
            return int(iface["data"][0])
        p_indptr = None if d_indptr is None else int32_address(d_indptr, a.n + 1, "indptr")
        p_indices = None if d_indices is None else int32_address(d_indices, a.nnz, "indices")
        p_data = _devarray.address(d_data, a.nnz, "out: data")
        check(lib().omg_device_synchronize())
        check(lib().omg_kappa_assemble_spaced(*a.call, ctypes.c_void_p(p_indptr), ctypes.c_void_p(p_indices), ctypes.c_void_p(p_data), 1))
        return out
    data = np.empty(a.nnz, dtype=np.float64)
    indptr = np.empty(a.n + 1, dtype=np.int32) if pattern else None
    indices = np.empty(a.nnz, dtype=np.int32) if pattern else None
    a.synchronize()
    check(lib().omg_kappa_assemble_spaced(*a.call, indptr.ctypes.data if pattern else None, indices.ctypes.data if pattern else None,
                                          data.ctypes.data, 0))
    return indptr, indices, data


VALUE_NONE, VALUE_SCALAR, VALUE_FIELD = 0, 1, 2


class _WallCall:
    """What kappa_rhs and kappa_flux share of their arguments, checked as operators.rhs_kappa checks them: kappa (NumPy, made
    contiguous, or a device array: .k_dev says which side every array of the call lies on), .grid, .wall (the six codes),
    .scale, .widths (three host arrays or three None), .values (None, a float or the array per wall), .n, .padded.
    .head(): the C arguments from `shape` to `hx`; .wall_values(): the kinds, scalars, field pointers and their side;
    .pointer(a, count, name): the address of an array on kappa's side; .host(a): a host array as contiguous float64,
    kept alive with the object.  `what` names the entry in the messages."""

    def __init__(self, what, kappa, walls, values, scale, spacing):
        from . import _devarray, operators
        self.what = what
        self.k_dev = _devarray.is_device_array(kappa)
        if self.k_dev:
            k_shape = tuple(int(s) for s in kappa.__cuda_array_interface__["shape"])
        else:
            kappa = np.asarray(kappa)
            if kappa.dtype != np.float64:
                raise ValueError("kappa must be float64, not %s" % kappa.dtype)
            kappa = np.ascontiguousarray(kappa)
            k_shape = kappa.shape
        self.kappa = kappa
        self.grid, self.wall, self.scale = operators.kappa_arguments(k_shape, walls, None, scale)
        self.widths = (None,) * 3
        if spacing is not None:
            if not operators.unit_scale(self.scale):
                raise ValueError("spacing and scale exclude each other: the widths carry every factor")
            self.widths = operators.spacing_arguments(self.grid, spacing)
        self.values = operators.wall_values_arguments(self.grid, self.wall, values)
        self.n, self.padded = int(np.prod(self.grid)), int(np.prod(k_shape))
        if self.padded >= 2 ** 31 - 1:
            raise ValueError("grid too large for int32 indices; shard it first")
        self.keep = [kappa]

    def same_side(self, named, names):
        """ValueError unless the arrays among `named` = [(name, array or float or None)] and the value fields lie on kappa's side."""
        from . import _devarray
        for name, a in list(named) + [("values[%d]" % w, v) for w, v in enumerate(self.values)]:
            if a is not None and not isinstance(a, float) and _devarray.is_device_array(a) != self.k_dev:
                raise ValueError("%s: %s must all be device arrays or all host arrays; %s is not on kappa's side" % (self.what, names, name))

    def pointer(self, a, count, name):
        from . import _devarray
        if self.k_dev:
            try:
                return _devarray.address(a, count, name)
            except TypeError as e:
                raise ValueError(str(e))
        return a.ctypes.data

    def host(self, a):
        if not self.k_dev:
            a = np.ascontiguousarray(a, dtype=np.float64)
            self.keep.append(a)
        return a

    def head(self):
        return ((ctypes.c_int64 * 3)(*self.grid), ctypes.c_void_p(self.pointer(self.kappa, self.padded, "kappa")), int(self.k_dev),
                (ctypes.c_int * 6)(*self.wall), (ctypes.c_double * 3)(*self.scale),
                *(ctypes.c_void_p(None if h is None else h.ctypes.data) for h in self.widths))

    def wall_values(self):
        from . import operators
        kinds, scalars, fields = [VALUE_NONE] * 6, [0.0] * 6, [None] * 6
        for w, v in enumerate(self.values):
            if v is None:
                continue
            if isinstance(v, float):
                kinds[w], scalars[w] = VALUE_SCALAR, v
                continue
            count = int(np.prod([self.grid[a] for a in operators.WALL_FACES[w]]))
            kinds[w], fields[w] = VALUE_FIELD, self.pointer(self.host(v), count, "values[%d]" % w)
        return (ctypes.c_int * 6)(*kinds), (ctypes.c_double * 6)(*scalars), (ctypes.c_void_p * 6)(*fields), int(self.k_dev)


def kappa_rhs(kappa, f=None, walls=None, values=None, scale=(1.0, 1.0, 1.0), spacing=None, out=None):
    """operators.rhs_kappa(kappa, f, walls, values, scale, spacing) made on the device (omg_kappa_rhs_spaced), bit for bit:
    the right-hand side that goes with the operator of kappa_assemble / Hierarchy.from_kappa — a source per cell, boundary
    values on Dirichlet walls, outward fluxes on Neumann walls (without spacing: flux times the cell width along the axis;
    the definition's docstring has the conventions).  kappa, f and the fields among `values`: NumPy arrays, or C-contiguous
    float64 device arrays — all of the arrays on the same side; scalars and None go with either; spacing: host arrays.
    out: with device arrays a device array of n entries to write into (may be f itself: in place), None for a new one; with
    host arrays None or a writeable contiguous float64 NumPy array.  Returns b in problemShape (a given `out` as it is).
    kappa's values are not checked here.  ValueError for what operators.rhs_kappa refuses, arrays on both sides, an `out`
    of the wrong size or side — before any device work."""
    from . import _devarray, operators
    c = _WallCall("kappa_rhs", kappa, walls, values, scale, spacing)
    f = operators.source_argument(c.grid, f)
    c.same_side([("f", f)], "kappa, f and the value fields")
    k_dev, n, grid = c.k_dev, c.n, c.grid
    if out is not None and _devarray.is_device_array(out) != k_dev:
        raise ValueError("kappa_rhs: `out` must be a device array exactly when kappa and f are device arrays")
    head = c.head()
    if f is None:
        f_kind, f_ptr = VALUE_NONE, None
    elif isinstance(f, float):
        c.keep.append(np.array([f], dtype=np.float64))
        f_kind, f_ptr = VALUE_SCALAR, c.keep[-1].ctypes.data
    else:
        f_kind, f_ptr = VALUE_FIELD, c.pointer(c.host(f), n, "f")
    wall_values = c.wall_values()
    if k_dev:
        b = _devarray.empty_like(c.kappa, n).reshape(grid) if out is None else out
        try:
            b_ptr = _devarray.address(b, n, "out")
        except TypeError as e:
            raise ValueError(str(e))
        check(lib().omg_device_synchronize())
    else:
        if out is None:
            b = np.empty(grid, dtype=np.float64)
        elif isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable and out.size == n:
            b = out
        else:
            raise ValueError("out must be a writeable contiguous float64 array of %d entries" % n)
        b_ptr = b.ctypes.data
    check(lib().omg_kappa_rhs_spaced(*head, ctypes.c_void_p(f_ptr), f_kind, int(k_dev and f_kind == VALUE_FIELD), *wall_values,
                                     ctypes.c_void_p(b_ptr), int(k_dev)))
    return b


def _extent_of(a, count):
    """(address, bytes) of a contiguous float64 array of `count` entries, NumPy or device; ValueError otherwise."""
    from . import _devarray
    if _devarray.is_device_array(a):
        try:
            return _devarray.address(a, count, "array"), 8 * count
        except TypeError as e:
            raise ValueError(str(e))
    return a.ctypes.data, 8 * count


def _share_bytes(p, q):
    return p[0] < q[0] + q[1] and q[0] < p[0] + p[1]


def _face_outputs(what, out, counts, shapes, on_device, like):
    """The three output arrays of kappa_flux — `out` checked (three contiguous float64 arrays of the face sizes on the
    inputs' side) or new ones —, and their addresses."""
    from . import _devarray
    if out is None:
        if on_device:
            out = tuple(_devarray.empty_like(like, c).reshape(s) for c, s in zip(counts, shapes))
        else:
            out = tuple(np.empty(s, dtype=np.float64) for s in shapes)
    else:
        try:
            out = tuple(out)
        except TypeError:
            raise ValueError("%s: `out` must be three face arrays (Fz, Fy, Fx)" % what)
        if len(out) != 3:
            raise ValueError("%s: `out` must be three face arrays (Fz, Fy, Fx), not %d" % (what, len(out)))
    pointers = []
    for name, a, count in zip(("Fz", "Fy", "Fx"), out, counts):
        if _devarray.is_device_array(a) != on_device:
            raise ValueError("%s: the face array %s must be a device array exactly when kappa and u are device arrays" % (what, name))
        if on_device:
            try:
                pointers.append(_devarray.address(a, count, name))
            except TypeError as e:
                raise ValueError(str(e))
        elif isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable and a.size == count:
            pointers.append(a.ctypes.data)
        else:
            raise ValueError("%s: the face array %s must be a writeable contiguous float64 array of %d entries" % (what, name, count))
    return out, pointers


def kappa_flux(kappa, u, walls=None, values=None, scale=(1.0, 1.0, 1.0), spacing=None, out=None, alpha=None):
    """operators.flux_kappa(kappa, u, walls, values, scale, spacing) made on the device (omg_kappa_flux_spaced), bit for bit,
    in one launch: the fluxes (Fz, Fy, Fx) of -kappa grad u along +z, +y, +x through every face, with the operator's own
    coefficients and factor — in-grid faces, the seam faces of periodic axes (faces 0 and e the same bits), Dirichlet and
    Neumann wall faces with the boundary data `values` of kappa_rhs (the definition's docstring has the signs and
    conventions).  kappa, u and the fields among `values`: NumPy arrays, or C-contiguous float64 device arrays — all on one
    side; u of problemShape or of n entries; spacing: host arrays.  out: None for new arrays, or three arrays (Fz, Fy, Fx) on
    the inputs' side to write into (returned as they are).  alpha (needs `out`): out = out + alpha * F instead — one
    multiplication and one addition per face.  Returns the three arrays in face shape.  kappa's values are not checked.
    ValueError — before any device work — for what operators.flux_kappa refuses, arrays on both sides, outputs of the
    wrong size or side, alpha without `out` or not finite, an `out` that overlaps u, kappa or another output (threads read
    their neighbours' u: the fluxes cannot be made in place)."""
    from . import operators
    c = _WallCall("kappa_flux", kappa, walls, values, scale, spacing)
    u = operators.solution_argument(c.grid, u)
    k_dev, n, padded, grid = c.k_dev, c.n, c.padded, c.grid
    shapes = operators.face_shapes(grid)
    counts = [int(np.prod(s)) for s in shapes]
    if max(counts) >= 2 ** 31 - 1:
        raise ValueError("grid too large for int32 indices; shard it first")
    if alpha is not None:
        if out is None:
            raise ValueError("kappa_flux: alpha needs `out`, the arrays alpha * F is added to")
        try:
            alpha = float(alpha)
        except (TypeError, ValueError):
            raise ValueError("kappa_flux: alpha must be None or a finite number, not %r" % (alpha,))
        if not np.isfinite(alpha):
            raise ValueError("kappa_flux: alpha must be finite, not %r" % alpha)
    c.same_side([("u", u)], "kappa, u and the value fields")
    head = c.head()
    k_ptr, u_ptr = head[1].value, c.pointer(c.host(u), n, "u")
    wall_values = c.wall_values()
    kappa = c.kappa
    faces, f_ptrs = _face_outputs("kappa_flux", out, counts, shapes, k_dev, kappa)
    spans = [(p, 8 * count) for p, count in zip(f_ptrs, counts)]
    for d, span in enumerate(spans):
        if _share_bytes(span, (u_ptr, 8 * n)) or _share_bytes(span, (k_ptr, 8 * padded)):
            raise ValueError("kappa_flux: the face array %s of `out` overlaps u or kappa: the fluxes cannot be made in place" % "zyx"[d])
        if any(_share_bytes(span, other) for other in spans[:d]):
            raise ValueError("kappa_flux: the face arrays of `out` overlap each other")
    if k_dev:
        check(lib().omg_device_synchronize())
    check(lib().omg_kappa_flux_spaced(*head, ctypes.c_void_p(u_ptr), int(k_dev), *wall_values,
                                      None if alpha is None else ctypes.byref(ctypes.c_double(alpha)),
                                      *(ctypes.c_void_p(p) for p in f_ptrs), int(k_dev)))
    return faces


def face_divergence(faces, out=None):
    """operators.divergence_faces(Fz, Fy, Fx) made on the device (omg_face_divergence), bit for bit: the cell balance
    ((Fz[k+1] - Fz[k]) + (Fy[j+1] - Fy[j])) + (Fx[i+1] - Fx[i]) of three face arrays — NumPy arrays, or C-contiguous float64
    device arrays, all on one side, in the face shapes of one grid.  out: None for a new array, or an array of n entries on
    the faces' side (returned as it is).  Returns the cell array in problemShape.  ValueError — before any device work — for
    another count or other shapes, arrays on both sides, an `out` of the wrong size or side or one that overlaps a face array."""
    from . import _devarray, operators
    try:
        faces = tuple(faces)
    except TypeError:
        raise ValueError("face_divergence: `faces` must be three face arrays (Fz, Fy, Fx)")
    if len(faces) != 3:
        raise ValueError("face_divergence: `faces` must be three face arrays (Fz, Fy, Fx), not %d" % len(faces))
    on_device = _devarray.is_device_array(faces[0])
    if any(_devarray.is_device_array(a) != on_device for a in faces):
        raise ValueError("face_divergence: the face arrays must all be device arrays or all host arrays")
    if not on_device:
        faces = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in faces)
    grid = operators.grid_of_faces(tuple(a.__cuda_array_interface__["shape"] if on_device else a.shape for a in faces))
    n = int(np.prod(grid))
    counts = [int(np.prod(s)) for s in operators.face_shapes(grid)]
    if max(counts) >= 2 ** 31 - 1:
        raise ValueError("grid too large for int32 indices; shard it first")
    if out is not None and _devarray.is_device_array(out) != on_device:
        raise ValueError("face_divergence: `out` must be a device array exactly when the face arrays are device arrays")
    spans = [_extent_of(a, c) for a, c in zip(faces, counts)]
    if on_device:
        d = _devarray.empty_like(faces[0], n).reshape(grid) if out is None else out
        try:
            d_ptr = _devarray.address(d, n, "out")
        except TypeError as e:
            raise ValueError(str(e))
    else:
        if out is None:
            d = np.empty(grid, dtype=np.float64)
        elif isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable and out.size == n:
            d = out
        else:
            raise ValueError("out must be a writeable contiguous float64 array of %d entries" % n)
        d_ptr = d.ctypes.data
    if any(_share_bytes((d_ptr, 8 * n), span) for span in spans):
        raise ValueError("face_divergence: `out` overlaps a face array")
    if on_device:
        check(lib().omg_device_synchronize())
    check(lib().omg_face_divergence((ctypes.c_int64 * 3)(*grid), *(ctypes.c_void_p(p) for p, _ in spans), int(on_device),
                                    ctypes.c_void_p(d_ptr), int(on_device)))
    return d


class FaceArgs:
    """KappaArgs' twin for one coefficient per face: the arguments of omg_faces_assemble / omg_hierarchy_create_from_faces /
    omg_hierarchy_update_faces from what the Python entries take.  faces = (Cz, Cy, Cx): three float64 arrays in the face
    shapes of one grid (operators.face_shapes), all NumPy arrays or all C-contiguous device arrays; walls and sigma as
    operators.stencil7_faces takes them, sigma a device array too.  ValueError for what operators.faces_arguments refuses,
    another count, dtype or size, arrays on both sides — before any device work; the coefficients' values are checked by the
    kernel that reads them (HipError, ERR_INVALID, naming the face).  .grid: problemShape; .shape: the operator's (n, n);
    .walls: the six codes; .periodic: per axis; .nnz; .counts: the entries of the three arrays; .faces_on_device; .pointers;
    .head: the C arguments from `shape` to `walls`; .call: those and sigma's; the object keeps the arrays alive."""

    def __init__(self, faces, walls=None, sigma=None):
        from . import _devarray, operators
        if isinstance(faces, FaceArgs):            # (already checked: Hierarchy.from_faces / update_faces take one as it is)
            self.__dict__.update(faces.__dict__)
            return
        try:
            faces = tuple(faces)
        except TypeError:
            raise ValueError("faces must be three coefficient arrays (Cz, Cy, Cx), not %r" % (faces,))
        if len(faces) != 3:
            raise ValueError("faces must be three coefficient arrays (Cz, Cy, Cx), not %d" % len(faces))
        f_dev = _devarray.is_device_array(faces[0])
        if any(_devarray.is_device_array(a) != f_dev for a in faces):
            raise ValueError("the face coefficients must all be device arrays or all host arrays")
        if f_dev:
            shapes = tuple(tuple(int(s) for s in a.__cuda_array_interface__["shape"]) for a in faces)
        else:
            faces = tuple(np.asarray(a) for a in faces)
            for name, a in zip(("Cz", "Cy", "Cx"), faces):
                if a.dtype != np.float64:
                    raise ValueError("the face coefficients %s must be float64, not %s" % (name, a.dtype))
            faces = tuple(np.ascontiguousarray(a) for a in faces)
            shapes = tuple(a.shape for a in faces)
        self.grid, self.walls = operators.faces_arguments(shapes, walls, sigma)
        self.n = int(np.prod(self.grid))
        self.shape = (self.n, self.n)
        self.periodic = operators.periodic_axes(self.walls)
        self.nnz = 7 * self.n - 2 * sum(self.n // e for e, wraps in zip(self.grid, self.periodic) if not wraps)
        self.counts = [int(np.prod(s)) for s in shapes]
        if 7 * self.n >= 2 ** 31 - 1 or max(self.counts) >= 2 ** 31 - 1:
            raise ValueError("operator too large for int32 indices; shard it first")
        if f_dev:
            try:
                self.pointers = [_devarray.address(a, c, name) for a, c, name in zip(faces, self.counts, ("Cz", "Cy", "Cx"))]
            except TypeError as e:
                raise ValueError(str(e))
        else:
            self.pointers = [a.ctypes.data for a in faces]
        s_dev = _devarray.is_device_array(sigma)
        if sigma is None:
            kind, s_ptr = SIGMA_NONE, None
        elif s_dev:
            kind, s_ptr = SIGMA_FIELD, _devarray.address(sigma, self.n, "sigma")
        elif np.ndim(sigma) == 0:
            sigma = np.array([float(sigma)], dtype=np.float64)
            kind, s_ptr = SIGMA_SCALAR, sigma.ctypes.data
        else:
            sigma = np.ascontiguousarray(sigma, dtype=np.float64)
            kind, s_ptr = SIGMA_FIELD, sigma.ctypes.data
        self.faces = faces
        self.faces_on_device = f_dev
        self.on_device = f_dev or s_dev
        self._keep = (faces, sigma)
        self.head = ((ctypes.c_int64 * 3)(*self.grid), *(ctypes.c_void_p(p) for p in self.pointers), int(f_dev), (ctypes.c_int * 6)(*self.walls))
        self.call = self.head + (ctypes.c_void_p(s_ptr), kind, int(s_dev))

    def matrix(self):
        """The operator as a SciPy CSR in host memory, assembled on the device (faces_assemble)."""
        indptr, indices, data = faces_assemble(self)
        A = sp.csr_matrix((data, indices, indptr), shape=self.shape)
        A.has_sorted_indices = True
        return A

    def synchronize(self):
        """What the caller's library enqueued on the device arrays is complete before the library's own stream reads them."""
        if self.on_device:
            check(lib().omg_device_synchronize())


def faces_assemble(faces, walls=None, sigma=None, pattern=True, out=None):
    """The 7-point operator of one coefficient per face, assembled on the device (omg_faces_assemble): the CSR arrays of
    operators.stencil7_faces(faces, walls, sigma), bit for bit.  faces: three NumPy arrays or three device arrays; sigma
    either.  Returns (indptr, indices, data) as NumPy arrays, indptr = indices = None with pattern=False; out = (indptr,
    indices, data): device arrays to write into instead, as kappa_assemble takes them."""
    from . import _devarray
    a = FaceArgs(faces, walls, sigma)
    if out is not None:
        d_indptr, d_indices, d_data = out
        if (d_indptr is None) != (d_indices is None):
            raise ValueError("out: indptr and indices are given together or not at all")

        def int32_address(arr, count, what):
            iface = arr.__cuda_array_interface__
            if iface["typestr"] not in ("<i4", "=i4", "|i4") or iface.get("strides") is not None or tuple(iface["shape"]) != (count,):
                raise ValueError("out: %s must be a contiguous int32 device array of %d entries" % (what, count))
            return int(iface["data"][0])
        p_indptr = None if d_indptr is None else int32_address(d_indptr, a.n + 1, "indptr")
        p_indices = None if d_indices is None else int32_address(d_indices, a.nnz, "indices")
        p_data = _devarray.address(d_data, a.nnz, "out: data")
        check(lib().omg_device_synchronize())
        check(lib().omg_faces_assemble(*a.call, ctypes.c_void_p(p_indptr), ctypes.c_void_p(p_indices), ctypes.c_void_p(p_data), 1))
        return out
    data = np.empty(a.nnz, dtype=np.float64)
    indptr = np.empty(a.n + 1, dtype=np.int32) if pattern else None
    indices = np.empty(a.nnz, dtype=np.int32) if pattern else None
    a.synchronize()
    check(lib().omg_faces_assemble(*a.call, indptr.ctypes.data if pattern else None, indices.ctypes.data if pattern else None,
                                   data.ctypes.data, 0))
    return indptr, indices, data


def _face_wall_values(what, a, values, named):
    """The boundary values of faces_rhs / faces_flux for the FaceArgs a — checked (operators.wall_values_arguments), on the
    coefficients' side like the arrays among `named` = [(name, array or float or None)] — as the C arguments (kinds, scalars,
    field pointers, their side) and the list of arrays to keep alive."""
    from . import _devarray, operators
    values = operators.wall_values_arguments(a.grid, a.walls, values)
    dev = a.faces_on_device
    for name, v in list(named) + [("values[%d]" % w, v) for w, v in enumerate(values)]:
        if v is not None and not isinstance(v, float) and _devarray.is_device_array(v) != dev:
            raise ValueError("%s: the coefficients, %s and the value fields must all be device arrays or all host arrays; %s is not on "
                             "the coefficients' side" % (what, named[0][0], name))
    kinds, scalars, fields, keep = [VALUE_NONE] * 6, [0.0] * 6, [None] * 6, []
    for w, v in enumerate(values):
        if v is None:
            continue
        if isinstance(v, float):
            kinds[w], scalars[w] = VALUE_SCALAR, v
            continue
        count = int(np.prod([a.grid[axis] for axis in operators.WALL_FACES[w]]))
        kinds[w], fields[w] = VALUE_FIELD, _side_pointer(dev, v, count, "values[%d]" % w, keep)
    return ((ctypes.c_int * 6)(*kinds), (ctypes.c_double * 6)(*scalars), (ctypes.c_void_p * 6)(*fields), int(dev)), keep


def _side_pointer(on_device, v, count, name, keep):
    """The address of a float64 array of `count` entries on the given side; a host array is made contiguous and kept."""
    from . import _devarray
    if on_device:
        try:
            return _devarray.address(v, count, name)
        except TypeError as e:
            raise ValueError(str(e))
    v = np.ascontiguousarray(v, dtype=np.float64)
    keep.append(v)
    return v.ctypes.data


def faces_rhs(faces, f=None, walls=None, values=None, out=None):
    """operators.rhs_faces(faces, f, walls, values) made on the device (omg_faces_rhs), bit for bit: the right-hand side that
    goes with the operator of faces_assemble / Hierarchy.from_faces.  faces (or a FaceArgs), f and the fields among `values`:
    NumPy arrays or all device arrays; out as kappa_rhs takes it (a device `out` may be f: in place).  Returns b in
    problemShape (a given `out` as it is).  The coefficients' values are not checked here.  ValueError — before any device
    work — for what operators.rhs_faces refuses, arrays on both sides, an `out` of the wrong size or side."""
    from . import _devarray, operators
    a = FaceArgs(faces, walls)
    f = operators.source_argument(a.grid, f)
    wall_values, keep = _face_wall_values("faces_rhs", a, values, [("f", f)])
    dev, n, grid = a.faces_on_device, a.n, a.grid
    if out is not None and _devarray.is_device_array(out) != dev:
        raise ValueError("faces_rhs: `out` must be a device array exactly when the coefficients and f are device arrays")
    if f is None:
        f_kind, f_ptr = VALUE_NONE, None
    elif isinstance(f, float):
        keep.append(np.array([f], dtype=np.float64))
        f_kind, f_ptr = VALUE_SCALAR, keep[-1].ctypes.data
    else:
        f_kind, f_ptr = VALUE_FIELD, _side_pointer(dev, f, n, "f", keep)
    if dev:
        b = _devarray.empty_like(a.faces[0], n).reshape(grid) if out is None else out
        try:
            b_ptr = _devarray.address(b, n, "out")
        except TypeError as e:
            raise ValueError(str(e))
        check(lib().omg_device_synchronize())
    else:
        if out is None:
            b = np.empty(grid, dtype=np.float64)
        elif isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable and out.size == n:
            b = out
        else:
            raise ValueError("out must be a writeable contiguous float64 array of %d entries" % n)
        b_ptr = b.ctypes.data
    check(lib().omg_faces_rhs(*a.head, ctypes.c_void_p(f_ptr), f_kind, int(dev and f_kind == VALUE_FIELD), *wall_values,
                              ctypes.c_void_p(b_ptr), int(dev)))
    return b


def faces_flux(faces, u, walls=None, values=None, out=None, alpha=None):
    """operators.flux_faces(faces, u, walls, values) made on the device (omg_faces_flux), bit for bit, in one launch: F = C
    (u_lo - u_hi) on every face with the boundary data `values` of faces_rhs.  faces (or a FaceArgs), u and the value fields:
    NumPy arrays or all device arrays; out, alpha as kappa_flux takes them (alpha needs `out`: out = out + alpha * F).
    Returns the three arrays in face shape.  ValueError — before any device work — for what operators.flux_faces refuses,
    arrays on both sides, outputs of the wrong size or side, alpha without `out` or not finite, an `out` that overlaps u, a
    coefficient array or another output."""
    from . import operators
    a = FaceArgs(faces, walls)
    u = operators.solution_argument(a.grid, u)
    dev, n, grid = a.faces_on_device, a.n, a.grid
    shapes = operators.face_shapes(grid)
    if alpha is not None:
        if out is None:
            raise ValueError("faces_flux: alpha needs `out`, the arrays alpha * F is added to")
        try:
            alpha = float(alpha)
        except (TypeError, ValueError):
            raise ValueError("faces_flux: alpha must be None or a finite number, not %r" % (alpha,))
        if not np.isfinite(alpha):
            raise ValueError("faces_flux: alpha must be finite, not %r" % alpha)
    wall_values, keep = _face_wall_values("faces_flux", a, values, [("u", u)])
    u_ptr = _side_pointer(dev, u, n, "u", keep)
    faces_out, f_ptrs = _face_outputs("faces_flux", out, a.counts, shapes, dev, a.faces[0])
    spans = [(p, 8 * count) for p, count in zip(f_ptrs, a.counts)]
    inputs = [(u_ptr, 8 * n)] + [(p, 8 * count) for p, count in zip(a.pointers, a.counts)]
    for d, span in enumerate(spans):
        if any(_share_bytes(span, other) for other in inputs):
            raise ValueError("faces_flux: the face array %s of `out` overlaps u or a coefficient array: the fluxes cannot be made in place" % "zyx"[d])
        if any(_share_bytes(span, other) for other in spans[:d]):
            raise ValueError("faces_flux: the face arrays of `out` overlap each other")
    if dev:
        check(lib().omg_device_synchronize())
    check(lib().omg_faces_flux(*a.head, ctypes.c_void_p(u_ptr), int(dev), *wall_values,
                               None if alpha is None else ctypes.byref(ctypes.c_double(alpha)),
                               *(ctypes.c_void_p(p) for p in f_ptrs), int(dev)))
    return faces_out


class Hierarchy:
    """Device-resident A/R hierarchy (omg_hierarchy)."""

    def __init__(self, A_list, R_list, smoother="gs", omega=1.0, dtype="float64", nullspace=None):
        """dtype: precision the levels are stored and computed in on the device ("float64", the
        reference's, or "float32"; "mixed": float32 levels with level 0's outer state in float64, for the resident
        entries); host vectors are float64 either way.  nullspace: None, or 'constant' for a singular operator with
        zero row and column sums (pure Neumann, periodic): the coarsest operator is inverted on the complement of the
        constants, resident_load projects the right-hand side and resident_fetch the iterate (OMG_NULLSPACE_CONSTANT)."""
        self._h = None
        if len(R_list) != len(A_list) - 1:
            raise ValueError("need len(R) == len(A) - 1")
        self.nullspace_kind = nullspace_code(nullspace)
        # (host copies for the call alone: the device copy is complete when it returns)
        A = [as_csr(M) for M in A_list]
        R = [as_csr(M) for M in R_list]
        arrA = (CsrView * len(A))(*[csr_view(M) for M in A])
        arrR = (CsrView * max(len(R), 1))(*[csr_view(M) for M in R])
        opt, h = self._options(smoother, omega, dtype)
        self.n_levels = len(A)
        self.sizes = [M.shape[0] for M in A]
        check(lib().omg_hierarchy_create_opt(self.n_levels, arrA, arrR, ctypes.byref(opt), ctypes.byref(h)))
        self._adopt(h)

    @classmethod
    def _blank(cls, nullspace):
        """An instance without a handle (what __del__ needs is set before anything can raise) that knows its null space:
        the first check of every from_* constructor."""
        self = cls.__new__(cls)
        self._h = None
        self.nullspace_kind = nullspace_code(nullspace)
        return self

    def _options(self, smoother, omega, dtype):
        """Sets smoother, omega and dtype from the caller's names; returns the creating entry's options (with the null space
        already set) and the empty handle it fills."""
        self.smoother = smoother_code(smoother)
        self.omega = float(omega)
        self.dtype = dtype_code(dtype)
        return HierarchyOptions(self.smoother, self.omega, self.dtype, self.nullspace_kind), ctypes.c_void_p()

    def _adopt(self, h):
        """Takes over the handle a creating entry returned."""
        self._h = h
        self._A = self._R = None

    @classmethod
    def from_fine(cls, A_in, shape, n_restrictions, smoother="gs", omega=1.0, dtype="float64", nullspace=None):
        """mgSolve's setup on the device (omg_hierarchy_create_from_fine_opt): restrictions, Galerkin products and the
        qualification of the levels all in HBM; len(sizes) = n_restrictions + 1.  nullspace: as for Hierarchy()."""
        self = cls._blank(nullspace)
        A0 = as_csr(A_in)
        shape = tuple(int(s) for s in shape)
        arr = (ctypes.c_int64 * len(shape))(*shape)
        opt, h = self._options(smoother, omega, dtype)
        self.n_levels = int(n_restrictions) + 1
        self.sizes = [A0.shape[0] // (2 ** len(shape)) ** l for l in range(self.n_levels)]
        v = csr_view(A0)
        check(lib().omg_hierarchy_create_from_fine_opt(ctypes.byref(v), len(shape), arr, int(n_restrictions), ctypes.byref(opt),
                                                       ctypes.byref(h)))
        self._adopt(h)
        return self

    @classmethod
    def from_fine_semi(cls, A_in, shape, n_restrictions, factors=None, min_size=0, smoother="gs", omega=1.0, dtype="float64",
                       nullspace=None, oddExtents=None):
        """mgSolve's setup with semicoarsening on the device (omg_hierarchy_create_from_fine_semi).  factors: one tuple of 1 or 2
        per axis of `shape` for each of the n_restrictions restrictions, or None = 'auto': the rule picks them level by level, at
        most n_restrictions of them, ending early where no axis can be coarsened or (after the first restriction) the coarse level
        would have <= min_size rows.  .coarsening lists what was built, .level_shapes every level's grid.
        oddExtents: None, or 'merge' — a factor 2 on any extent >= 4 (omg_hierarchy_create_from_fine_ragged)."""
        self = cls._blank(nullspace)
        A0 = as_csr(A_in)
        shape = tuple(int(s) for s in shape)
        dim = len(shape)
        arr = (ctypes.c_int64 * dim)(*shape)
        n_restrictions = int(n_restrictions)
        flat = None
        if factors is not None:
            factors = [tuple(int(f) for f in entry) for entry in factors]
            if len(factors) != n_restrictions or any(len(entry) != dim for entry in factors):
                raise ValueError("factors needs n_restrictions entries of one factor per axis of the shape")
            flat = (ctypes.c_int * max(n_restrictions * dim, 1))(*[f for entry in factors for f in entry])
        opt, h = self._options(smoother, omega, dtype)
        v = csr_view(A0)
        check(lib().omg_hierarchy_create_from_fine_ragged(ctypes.byref(v), dim, arr, n_restrictions, flat, int(min_size),
                                                          odd_code(oddExtents), ctypes.byref(opt), ctypes.byref(h)))
        self._adopt(h)
        used = []
        f3 = (ctypes.c_int * 3)()
        for level in range(n_restrictions):
            if lib().omg_hierarchy_coarsening(h, level, f3) != OMG_OK:      # (past the last restriction built)
                break
            used.append(tuple(int(f3[d]) for d in range(dim)))
        self._set_coarsening(shape, used, oddExtents)
        self.n_levels = len(used) + 1
        self.sizes = [int(np.prod(s)) for s in self.level_shapes]
        return self

    def _set_coarsening(self, shape, factors, oddExtents=None):
        """Records the factors of every restriction and the grid of every level (None: not a semicoarsened hierarchy), and
        the 'oddExtents' key they were chosen under (an odd extent halves to its floor)."""
        self.odd_extents = None if factors is None else oddExtents
        self.coarsening = None if factors is None else [tuple(int(f) for f in entry) for entry in factors]
        self.level_shapes = None
        if factors is not None:
            self.level_shapes = [tuple(int(s) for s in shape)]
            for entry in self.coarsening:
                self.level_shapes.append(tuple(s // f for s, f in zip(self.level_shapes[-1], entry)))

    coarsening = None          # [(factor per axis), ...] per restriction of a semicoarsened hierarchy, else None
    level_shapes = None        # [(extent per axis), ...] per level of a semicoarsened hierarchy, else None
    odd_extents = None         # 'merge' where the factors were chosen with parameters['oddExtents'] = 'merge', else None

    def update_fine(self, data, on_device=False):
        """New values for the fine operator, same pattern (omg_hierarchy_update_fine).  data: the CSR's value array as a
        float64 NumPy array, or — on_device — (device pointer, number of entries).  Takes a from_fine hierarchy whose
        smoothed levels all run the 27-point kernels, or whose level 0 runs the 7-point var7 passes and whose smoothed levels
        are var7 or host-coded; afterwards it is the hierarchy from_fine builds from the new operator, bit for bit."""
        if on_device:
            ptr, nnz = data
            check(lib().omg_hierarchy_update_fine(self._h, ctypes.c_void_p(int(ptr)), int(nnz), 1))
        else:
            d = np.ascontiguousarray(data, dtype=np.float64)
            check(lib().omg_hierarchy_update_fine(self._h, d.ctypes.data, d.size, 0))

    @classmethod
    def from_kappa(cls, kappa, n_restrictions, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), smoother="gs", omega=1.0,
                   dtype="float64", nullspace=None, spacing=None):
        """from_fine of operators.stencil7_kappa(kappa, walls, sigma, scale, spacing) without that matrix ever being on the
        host (omg_hierarchy_create_from_kappa_spaced): level 0 is assembled in HBM from the field — a NumPy array or a device array —,
        the rest is from_fine's own sequence, the result the same object bit for bit.  With periodic walls no fused path takes
        the levels: the chain is made in HBM, fetched once and set up by the ordinary route — Hierarchy(A_list, R_list) of the
        definition's lists, bit for bit; can_update_fine() is then False."""
        self = cls._blank(nullspace)
        a = KappaArgs(kappa, walls, sigma, scale, spacing)
        opt, h = self._options(smoother, omega, dtype)
        self.n_levels = int(n_restrictions) + 1
        self.sizes = [a.n // 8 ** l for l in range(self.n_levels)]
        a.synchronize()
        check(lib().omg_hierarchy_create_from_kappa_spaced(*a.call, int(n_restrictions), ctypes.byref(opt), ctypes.byref(h)))
        self._adopt(h)
        return self

    def update_kappa(self, kappa, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), spacing=None):
        """update_fine with the values of operators.stencil7_kappa(kappa, walls, sigma, scale, spacing), made on the device
        (omg_hierarchy_update_kappa_spaced): with device arrays nothing crosses to the host.  Takes the hierarchies update_fine
        takes whose level 0 is the 7-point operator on kappa's grid (HipError ERR_INVALID otherwise — a hierarchy with
        periodic walls among them, and periodic walls on a hierarchy with the in-grid pattern — and for a kappa or sigma
        out of range; the hierarchy is then as before)."""
        a = KappaArgs(kappa, walls, sigma, scale, spacing)
        a.synchronize()
        check(lib().omg_hierarchy_update_kappa_spaced(self._h, *a.call))

    @classmethod
    def from_faces(cls, faces, n_restrictions, walls=None, sigma=None, smoother="gs", omega=1.0, dtype="float64", nullspace=None):
        """from_fine of operators.stencil7_faces(faces, walls, sigma) without that matrix ever being on the host
        (omg_hierarchy_create_from_faces): level 0 is assembled in HBM from the three face arrays — NumPy arrays or device
        arrays —, the rest is from_fine's own sequence, the result the same object bit for bit (with periodic walls: the
        ordinary route's, as from_kappa)."""
        self = cls._blank(nullspace)
        a = FaceArgs(faces, walls, sigma)
        opt, h = self._options(smoother, omega, dtype)
        self.n_levels = int(n_restrictions) + 1
        self.sizes = [a.n // 8 ** l for l in range(self.n_levels)]
        a.synchronize()
        check(lib().omg_hierarchy_create_from_faces(*a.call, int(n_restrictions), ctypes.byref(opt), ctypes.byref(h)))
        self._adopt(h)
        return self

    def update_faces(self, faces, walls=None, sigma=None):
        """update_fine with the values of operators.stencil7_faces(faces, walls, sigma), made on the device
        (omg_hierarchy_update_faces): with device arrays nothing crosses to the host.  Takes the hierarchies update_kappa
        takes (HipError ERR_INVALID otherwise, and for a coefficient or sigma out of range; the hierarchy is then as before)."""
        a = FaceArgs(faces, walls, sigma)
        a.synchronize()
        check(lib().omg_hierarchy_update_faces(self._h, *a.call))

    def can_update_fine(self):
        """Whether update_fine takes this hierarchy (omg_hierarchy_can_update_fine)."""
        yes = ctypes.c_int(0)
        check(lib().omg_hierarchy_can_update_fine(self._h, ctypes.byref(yes)))
        return bool(yes.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().omg_hierarchy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- whole cycles -------------------------------------------------------------------
    def vcycle(self, b, x, pre, post, level=0):
        """x is updated in place; returns the residual norm."""
        n = self.sizes[level]
        b = vec(b, n)
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.size == n
        norm = ctypes.c_double(0.0)
        check(lib().omg_vcycle(self._h, level, b.ctypes.data, x.ctypes.data, int(pre), int(post), ctypes.byref(norm)))
        return norm.value

    def vcycle_ex(self, b, x_in, x_out, x_pre, pre, post, level=0):
        """omg_vcycle_ex: x_in (None: zeros) -> x_out; x_pre (None: not wanted) receives the iterate after the
        pre-smoothing sweeps (the reference's in-place smoother overwrites `initial` with it).  Returns the norm."""
        n = self.sizes[level]
        b = vec(b, n)
        for a in (x_in, x_out, x_pre):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous and a.size == n)
        norm = ctypes.c_double(0.0)
        check(lib().omg_vcycle_ex(self._h, level, b.ctypes.data, None if x_in is None else x_in.ctypes.data, x_out.ctypes.data,
                                  None if x_pre is None else x_pre.ctypes.data, int(pre), int(post), ctypes.byref(norm)))
        return norm.value

    def vcycle_dev(self, b_ptr, x_in_ptr, x_out_ptr, x_pre_ptr, pre, post, level=0):
        """omg_vcycle_dev: vcycle_ex on DEVICE arrays given by address (double, natural numbering; 0 / None: absent).
        Returns the norm; the outputs are complete on return."""
        norm = ctypes.c_double(0.0)
        check(lib().omg_vcycle_dev(self._h, level, ctypes.c_void_p(int(b_ptr)), ctypes.c_void_p(int(x_in_ptr or 0)),
                                   ctypes.c_void_p(int(x_out_ptr)), ctypes.c_void_p(int(x_pre_ptr or 0)), int(pre), int(post),
                                   ctypes.byref(norm)))
        return norm.value

    def resident_load_dev(self, b_ptr, x0_ptr=None):
        check(lib().omg_resident_load_dev(self._h, ctypes.c_void_p(int(b_ptr)), ctypes.c_void_p(int(x0_ptr or 0))))

    def resident_fetch_dev(self, x_ptr):
        check(lib().omg_resident_fetch_dev(self._h, ctypes.c_void_p(int(x_ptr))))

    def solve(self, b, x, pre, post, max_cycles, threshold):
        n = self.sizes[0]
        b = vec(b, n)
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.size == n
        cycles = ctypes.c_int(0)
        norm = ctypes.c_double(0.0)
        check(lib().omg_solve(self._h, b.ctypes.data, x.ctypes.data, int(pre), int(post), int(max_cycles),
                              float(threshold), ctypes.byref(cycles), ctypes.byref(norm)))
        return cycles.value, norm.value

    def cycle_dev(self, b_dev, x_dev, pre, post, hip_stream=None):
        """One cycle from a zero iterate on DEVICE vectors (addresses of level-0 doubles in natural numbering):
        omg_hierarchy_cycle_dev, enqueued on `hip_stream` (None: the hierarchy's own), no host synchronisation."""
        check(lib().omg_hierarchy_cycle_dev(self._h, ctypes.c_void_p(int(b_dev)), ctypes.c_void_p(int(x_dev)), int(pre), int(post),
                                            ctypes.c_void_p(hip_stream or 0)))

    # -- resident ------------------------------------------------------------------------
    def resident_load(self, b, x0=None):
        b = vec(b, self.sizes[0])
        x0 = None if x0 is None else vec(x0, self.sizes[0])        # kept alive until the call returns
        check(lib().omg_resident_load(self._h, b.ctypes.data, None if x0 is None else x0.ctypes.data))

    def resident_cycle(self, pre, post, want_norm=True):
        if want_norm:
            norm = ctypes.c_double(0.0)
            check(lib().omg_resident_cycle(self._h, int(pre), int(post), ctypes.byref(norm)))
            return norm.value
        check(lib().omg_resident_cycle(self._h, int(pre), int(post), None))
        return None

    def resident_cycles(self, pre, post, n_cycles):
        """n_cycles V-cycles back to back; returns every cycle's residual norm (omg_resident_cycles)."""
        norms = (ctypes.c_double * max(int(n_cycles), 1))()
        check(lib().omg_resident_cycles(self._h, int(pre), int(post), int(n_cycles), norms))
        return [float(norms[k]) for k in range(int(n_cycles))]

    def resident_fetch(self, out=None):
        """The resident iterate as a new array, or written into `out` (contiguous float64 of level 0's size)."""
        if out is None:
            x = np.empty(self.sizes[0], dtype=np.float64)
        else:
            x = out
            if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous and x.flags.writeable
                    and x.size == self.sizes[0]):
                raise ValueError("out must be a writeable contiguous float64 array of %d entries" % self.sizes[0])
        check(lib().omg_resident_fetch(self._h, x.ctypes.data))
        return x

    def resident_pcg(self, pre, post, max_iter, threshold=0.0):
        """Flexible CG preconditioned by one zero-start V(pre, post) cycle per iteration, from the resident iterate
        (omg_resident_pcg).  Returns (iterations, norms ndarray of the recurrence norm per iteration, true_norm, breakdown);
        the solution stays resident (resident_fetch)."""
        max_iter = int(max_iter)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        norms = np.zeros(max_iter, dtype=np.float64)
        it, tn, bd = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_int(0)
        check(lib().omg_resident_pcg(self._h, int(pre), int(post), max_iter, float(threshold), ctypes.byref(it),
                                     norms.ctypes.data_as(_DP), ctypes.byref(tn), ctypes.byref(bd)))
        return int(it.value), norms[:it.value].copy(), float(tn.value), bool(bd.value)

    def resident_norms(self, rhs=True, residual=True):
        """(||b||, ||b - A x||) of the resident state without a cycle (omg_resident_norms); None for the one not asked
        for.  The state is untouched: what runs afterwards has the bits it would have had."""
        nb, nr = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(lib().omg_resident_norms(self._h, ctypes.byref(nb) if rhs else None, ctypes.byref(nr) if residual else None))
        return (nb.value if rhs else None), (nr.value if residual else None)

    def projection(self, capacity):
        """Room for `capacity` (1..64) earlier solutions, the set empty; 0 frees it (omg_resident_projection)."""
        check(lib().omg_resident_projection(self._h, int(capacity)))

    def resident_project(self):
        """The resident iterate <- the A-best approximation of the solution in the set's span, from the resident b
        (omg_resident_project; enqueued only).  Returns the vectors used; 0: nothing was launched."""
        used = ctypes.c_int(0)
        check(lib().omg_resident_project(self._h, ctypes.byref(used)))
        return int(used.value)

    def resident_project_update(self):
        """After the solve: what the resident iterate adds to the projected start joins the set
        (omg_resident_project_update).  Returns (the set's size afterwards, whether the direction was kept)."""
        size, kept = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().omg_resident_project_update(self._h, ctypes.byref(size), ctypes.byref(kept)))
        return int(size.value), bool(kept.value)

    def projection_fetch(self, index):
        """Vector `index` of the set as a host array in the caller's numbering (omg_resident_projection_fetch)."""
        v = np.empty(self.sizes[0], dtype=np.float64)
        check(lib().omg_resident_projection_fetch(self._h, int(index), v.ctypes.data))
        return v

    def projection_time(self, reps=20):
        """Average milliseconds of one launch of (the set's inner products with the resident b, pcg's single inner product
        on the same length, the linear combination over the set): omg_resident_projection_time."""
        dots, dot, comb = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(lib().omg_resident_projection_time(self._h, int(reps), ctypes.byref(dots), ctypes.byref(dot), ctypes.byref(comb)))
        return dots.value, dot.value, comb.value

    def spmv_time(self, reps=20):
        """Average milliseconds of one fine-grid y = A[0] x launch on the resident operator."""
        ms = ctypes.c_double(0.0)
        check(lib().omg_resident_spmv_time(self._h, int(reps), ctypes.byref(ms)))
        return ms.value

    def use_graph(self, enable=True):
        check(lib().omg_resident_use_graph(self._h, 1 if enable else 0))

    def set_stream(self, hip_stream):
        check(lib().omg_hierarchy_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)))

    def sync(self):
        check(lib().omg_hierarchy_sync(self._h))

    def device_dtype(self):
        """np.dtype the levels are held in on the device (omg_hierarchy_dtype): float32 for a mixed hierarchy too."""
        code = ctypes.c_int(-1)
        check(lib().omg_hierarchy_dtype(self._h, ctypes.byref(code)))
        return np.dtype(np.float32 if code.value in (DTYPE_F32, DTYPE_MIXED) else np.float64)

    @property
    def nullspace(self):
        """None or 'constant': the null space the hierarchy was made for (omg_hierarchy_nullspace)."""
        code = ctypes.c_int(-1)
        check(lib().omg_hierarchy_nullspace(self._h, ctypes.byref(code)))
        return {v: k for k, v in NULLSPACES.items()}[code.value]

    def project(self, level, x):
        """(x - mean(x), mean) of a vector of `level`, formed on the device in the level's precision and ordering
        (omg_level_project: the projection kernels of a null-space hierarchy, on any hierarchy)."""
        out = vec(x, self.sizes[level], copy=True)
        mean = ctypes.c_double(0.0)
        check(lib().omg_level_project(self._h, int(level), out.ctypes.data, ctypes.byref(mean)))
        return out, mean.value

    def level_sets(self, level):
        v = ctypes.c_int64(0)
        check(lib().omg_hierarchy_level_sets(self._h, level, ctypes.byref(v)))
        return v.value

    def level_fused(self, level):
        v = ctypes.c_int(0)
        check(lib().omg_hierarchy_level_fused(self._h, level, ctypes.byref(v)))
        return bool(v.value)

    def level_flags(self, level):
        """dict(fused_last_set=bool, scatter_prolong=bool, union_walk=bool, march=bool, plane=bool, stencil27=bool, var7=bool,
        march_scan=bool, tail_fused=bool, line=bool) of a smoothed level.  tail_fused: a V(1,1) cycle of the hierarchy's shape runs
        this level's up pass inside the fused tail launch (OMG_TAIL_FUSE).  line: the zebra line smoother (OMG_SMOOTH_LINE*)."""
        f = ctypes.c_int(0)
        check(lib().omg_hierarchy_level_flags(self._h, int(level), ctypes.byref(f)))
        return {"fused_last_set": bool(f.value & 1), "scatter_prolong": bool(f.value & 2), "union_walk": bool(f.value & 16),
                "march": bool(f.value & 32), "plane": bool(f.value & 64), "stencil27": bool(f.value & 128), "var7": bool(f.value & 256),
                "march_scan": bool(f.value & 512), "tail_fused": bool(f.value & 1024), "line": bool(f.value & 2048)}

    @property
    def line_axis(self):
        """The axis the line smoother's lines follow, as an index into the grid's shape in C order (the last axis is the
        unit-stride one), or None for a hierarchy made with another smoother (omg_hierarchy_line_axis)."""
        axis, dim = ctypes.c_int(-1), ctypes.c_int(0)
        check(lib().omg_hierarchy_line_axis(self._h, ctypes.byref(axis), ctypes.byref(dim)))
        return None if axis.value < 0 else dim.value - 1 - axis.value

    def tail_info(self):
        """(fused tail launches put on the stream so far, how many of them by replaying a graph): omg_hierarchy_tail_info"""
        out = (ctypes.c_int64 * 2)()
        check(lib().omg_hierarchy_tail_info(self._h, out))
        return int(out[0]), int(out[1])

    def use_plane(self, enable=True):
        """Plane-pipelined passes on / off (omg_hierarchy_use_plane; same iterate either way)."""
        check(lib().omg_hierarchy_use_plane(self._h, 1 if enable else 0))

    def set_cycle(self, shape="V", over_correction=1.0):
        """Shape ('V', 'F', 'W') and over-correction factor of every cycle run on this hierarchy from now on
        (omg_hierarchy_set_cycle); repeating the current setting does nothing."""
        check(lib().omg_hierarchy_set_cycle(self._h, cycle_code(shape), over_correction_of(over_correction)))

    def get_cycle(self):
        """(shape, over-correction factor) as set: ('V', 1.0) unless set_cycle has been called."""
        code, alpha = ctypes.c_int(-1), ctypes.c_double(0.0)
        check(lib().omg_hierarchy_get_cycle(self._h, ctypes.byref(code), ctypes.byref(alpha)))
        return {v: k for k, v in CYCLES.items()}[code.value], alpha.value

    PLANE_FIELDS = ("nx", "ny", "nz", "tile_x", "tile_y", "tile_z", "workgroups", "threads")

    def plane_info(self, level):
        out = (ctypes.c_int64 * len(self.PLANE_FIELDS))()
        check(lib().omg_hierarchy_plane_info(self._h, int(level), out))
        return dict(zip(self.PLANE_FIELDS, [int(v) for v in out]))

    def set_info(self, level, s):
        """(rows, stored entries) of smoother set `s` of a level."""
        rows, nnz = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().omg_hierarchy_set_info(self._h, level, s, ctypes.byref(rows), ctypes.byref(nnz)))
        return rows.value, nnz.value

    FORMAT_FIELDS = ("rows", "nnz", "blocks", "pattern_blocks", "pattern_rows", "pattern_nnz",
                     "coldict_nnz", "valdict_nnz", "format_bytes", "csr_bytes", "ell_blocks", "ell_nnz")

    def format_info(self, level, op="A", set=-1):
        """How A / R / P (= R^T) of `level` is held in HBM (omg_hierarchy_format_info)."""
        out = (ctypes.c_int64 * len(self.FORMAT_FIELDS))()
        check(lib().omg_hierarchy_format_info(self._h, int(level), {"A": 0, "R": 1, "P": 2}[op], int(set), out))
        return dict(zip(self.FORMAT_FIELDS, [int(v) for v in out]))

    def profile_enable(self, classes=True):
        """True = every class, False = off, or an iterable of class names (PROFILE_NAMES)."""
        if classes is True:
            mask = -1
        elif not classes:
            mask = 0
        else:
            mask = 0
            for name in classes:
                mask |= 1 << PROFILE_NAMES.index(name)
        check(lib().omg_profile_enable(self._h, mask))

    def profile_read(self):
        n = (ctypes.c_int64 * PROFILE_CLASSES)()
        ms = (ctypes.c_double * PROFILE_CLASSES)()
        check(lib().omg_profile_read(self._h, n, ms))
        return {PROFILE_NAMES[i]: (int(n[i]), float(ms[i])) for i in range(PROFILE_CLASSES)}

    # -- single operations -----------------------------------------------------------------
    def smooth(self, level, b, x, iterations):
        n = self.sizes[level]
        b = vec(b, n)
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.size == n
        check(lib().omg_level_smooth(self._h, level, b.ctypes.data, x.ctypes.data, int(iterations)))
        return x

    def residual(self, level, b, x, want_norm=False):
        n = self.sizes[level]
        b, x = vec(b, n), vec(x, n)
        r = np.empty(n)
        if want_norm:
            norm = ctypes.c_double(0.0)
            check(lib().omg_level_residual(self._h, level, b.ctypes.data, x.ctypes.data, r.ctypes.data, ctypes.byref(norm)))
            return r, norm.value
        check(lib().omg_level_residual(self._h, level, b.ctypes.data, x.ctypes.data, r.ctypes.data, None))
        return r

    def spmv(self, level, x):
        """A[level] x on the operator as the hierarchy holds it (omg_level_spmv)."""
        n = self.sizes[level]
        x = vec(x, n)
        y = np.empty(n)
        check(lib().omg_level_spmv(self._h, level, x.ctypes.data, y.ctypes.data))
        return y

    def spmv_dev(self, level, x_ptr, y_ptr):
        """omg_level_spmv_dev: spmv on DEVICE arrays given by address (double, the caller's numbering; y may be x).  The
        resident right-hand side and iterate are not touched; returns after the hierarchy's stream has finished."""
        check(lib().omg_level_spmv_dev(self._h, level, ctypes.c_void_p(int(x_ptr)), ctypes.c_void_p(int(y_ptr))))

    def restrict(self, level, fine):
        fine = vec(fine, self.sizes[level])
        out = np.empty(self.sizes[level + 1])
        check(lib().omg_level_restrict(self._h, level, fine.ctypes.data, out.ctypes.data))
        return out

    def prolong_add(self, level, coarse, fine):
        coarse = vec(coarse, self.sizes[level + 1])
        out = vec(fine, self.sizes[level], copy=True)
        check(lib().omg_level_prolong_add(self._h, level, coarse.ctypes.data, out.ctypes.data))
        return out

    def coarse_info(self):
        """dict(blocks, n, half_bandwidth, bytes_per_solve) of the coarsest level's direct solver:
        blocks == 1 is the explicit inverse, > 1 substructuring along the band."""
        out = (ctypes.c_int64 * 4)()
        check(lib().omg_hierarchy_coarse_info(self._h, out))
        return {"blocks": int(out[0]), "n": int(out[1]), "half_bandwidth": int(out[2]), "bytes_per_solve": int(out[3])}

    def coarse_solve(self, b):
        b = vec(b, self.sizes[-1])
        x = np.empty(self.sizes[-1])
        check(lib().omg_coarse_solve(self._h, b.ctypes.data, x.ctypes.data))
        return x


# ---- standalone ------------------------------------------------------------------------
def format_selftest(A, dtype="float64"):
    """Code A into the device format on the host, decode, compare bit for bit (no GPU needed);
    returns the format statistics (Hierarchy.FORMAT_FIELDS).  Raises HipError on a mismatch."""
    A = as_csr(A)
    out = (ctypes.c_int64 * len(Hierarchy.FORMAT_FIELDS))()
    v = csr_view(A)
    check(lib().omg_format_selftest(ctypes.byref(v), dtype_code(dtype), out))
    return dict(zip(Hierarchy.FORMAT_FIELDS, [int(x) for x in out]))


def spmv(A, x):
    A = as_csr(A)
    x = vec(x, A.shape[1])
    y = np.empty(A.shape[0])
    v = csr_view(A)
    check(lib().omg_spmv(ctypes.byref(v), x.ctypes.data, y.ctypes.data))
    return y


def residual(A, b, x, want_norm=False):
    A = as_csr(A)
    b, x = vec(b, A.shape[0]), vec(x, A.shape[1])
    r = np.empty(A.shape[0])
    v = csr_view(A)
    if want_norm:
        norm = ctypes.c_double(0.0)
        check(lib().omg_residual(ctypes.byref(v), b.ctypes.data, x.ctypes.data, r.ctypes.data, ctypes.byref(norm)))
        return r, norm.value
    check(lib().omg_residual(ctypes.byref(v), b.ctypes.data, x.ctypes.data, r.ctypes.data, None))
    return r


def gauss_seidel(A, b, x, smoother="gs", omega=1.0, iterations=None, threshold=None):
    """x (contiguous float64) is updated in place; returns the number of sweeps done."""
    A = as_csr(A)
    b = vec(b, A.shape[0])
    assert x.dtype == np.float64 and x.flags.c_contiguous and x.size == A.shape[0]
    v = csr_view(A)
    done = ctypes.c_int(0)
    check(lib().omg_gauss_seidel(ctypes.byref(v), b.ctypes.data, x.ctypes.data, smoother_code(smoother),
                                 float(omega), -1 if iterations is None else int(iterations),
                                 -1.0 if threshold is None else float(threshold), ctypes.byref(done)))
    return done.value


def direct_solve(A, b):
    A = as_csr(A)
    b = vec(b, A.shape[0])
    x = np.empty(A.shape[0])
    v = csr_view(A)
    check(lib().omg_direct_solve(ctypes.byref(v), b.ctypes.data, x.ctypes.data))
    return x


def _product(fn, X, Y):
    X, Y = as_csr(X), as_csr(Y)
    vx, vy = csr_view(X), csr_view(Y)
    res = ctypes.c_void_p()
    nr, nc, nnz = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(fn(ctypes.byref(vx), ctypes.byref(vy), ctypes.byref(res), ctypes.byref(nr),
             ctypes.byref(nc), ctypes.byref(nnz)))
    indptr = np.empty(nr.value + 1, dtype=np.int32)
    indices = np.empty(max(nnz.value, 0), dtype=np.int32)
    data = np.empty(max(nnz.value, 0), dtype=np.float64)
    check(lib().omg_csr_result_fetch(res, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data))
    return sp.csr_matrix((data, indices, indptr), shape=(nr.value, nc.value))


def rap(R, A):
    """Galerkin product (R A) R^T on the device -> scipy CSR (sorted columns)."""
    return _product(lib().omg_rap, R, A)


def spgemm(X, Y):
    """Sparse product X Y on the device -> scipy CSR (sorted columns)."""
    return _product(lib().omg_spgemm, X, Y)


def restriction(shape):
    """operators.restriction(shape) built on the device -> scipy CSR."""
    shape = tuple(int(s) for s in shape)
    dim = len(shape)
    N = int(np.prod(shape))
    n = N // (2 ** dim)
    arr = (ctypes.c_int64 * dim)(*shape)
    indptr = np.empty(n + 1, dtype=np.int32)
    indices = np.empty(n * (2 ** dim), dtype=np.int32)
    data = np.empty(n * (2 ** dim), dtype=np.float64)
    nr, nnz = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().omg_restriction(dim, arr, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data,
                                ctypes.byref(nr), ctypes.byref(nnz)))
    k = nnz.value
    if k and int(indices[:k].max()) >= N:
        # the reference's LIL assignment raises the same for shapes its offsets overrun
        raise IndexError("column index (%d) out of range" % int(indices[:k].max()))
    return sp.csr_matrix((data[:k], indices[:k], indptr[:nr.value + 1]), shape=(nr.value, N))


ODD_REFUSE, ODD_MERGE = 0, 1


def odd_code(oddExtents):
    """OMG_ODD_* of parameters['oddExtents']: None or 'merge'; ValueError for anything else."""
    if oddExtents is None:
        return ODD_REFUSE
    if isinstance(oddExtents, str) and oddExtents == "merge":
        return ODD_MERGE
    raise ValueError("parameters['oddExtents'] must be None or 'merge', not %r" % (oddExtents,))


def restriction_ex(shape, factors, oddExtents=None):
    """The plain C-order aggregation of the grid `shape` by `factors` (1 or 2 per axis) built on the device -> scipy CSR
    (omg_restriction_ragged); HipError (ERR_INVALID) for factors it does not take.  oddExtents 'merge': a 2 on any extent
    >= 4, an odd extent's last aggregate takes three cells; every entry keeps the weight 1 / prod(factors)."""
    odd = odd_code(oddExtents)
    shape = tuple(int(s) for s in shape)
    factors = tuple(int(f) for f in factors)
    dim = len(shape)
    if len(factors) != dim:
        raise ValueError("need one factor per axis of the shape %s, not %r" % (shape, factors))
    N = int(np.prod(shape))
    n = int(np.prod([s // f for s, f in zip(shape, factors)])) if all(f > 0 for f in factors) else 0
    indptr = np.empty(n + 1, dtype=np.int32)
    indices = np.empty(max(N, 1), dtype=np.int32)
    data = np.empty(max(N, 1), dtype=np.float64)
    check(lib().omg_restriction_ragged(dim, (ctypes.c_int64 * dim)(*shape), (ctypes.c_int * dim)(*factors), odd, indptr.ctypes.data,
                                       indices.ctypes.data, data.ctypes.data))
    R = sp.csr_matrix((data[:N], indices[:N], indptr), shape=(n, N))
    R.has_sorted_indices = True
    return R


def axis_couplings(A, shape):
    """(sums, counts, off_axis) of a grid operator (omg_axis_couplings): per axis of `shape` the sum of |a_ij| and the number
    of the stored entries at column offset +- the axis's stride, and the number of stored entries at any other non-zero offset."""
    A = as_csr(A)
    shape = tuple(int(s) for s in shape)
    dim = len(shape)
    sums = (ctypes.c_double * 3)()
    counts = (ctypes.c_int64 * 4)()
    v = csr_view(A)
    check(lib().omg_axis_couplings(ctypes.byref(v), dim, (ctypes.c_int64 * dim)(*shape), sums, counts))
    return tuple(float(sums[a]) for a in range(dim)), tuple(int(counts[a]) for a in range(dim)), int(counts[3])


def semicoarsen_rule(shape, sums, counts, off_axis=0, line_axis=None, level=0, oddExtents=None):
    """The factors (1 or 2 per axis of `shape`) the 'auto' rule picks for one level from its couplings
    (omg_semicoarsen_rule_ragged, a host function: no device).  All ones: no axis can be coarsened.  HipError
    (ERR_UNSUPPORTED) when off_axis != 0.  oddExtents 'merge': an axis is eligible when its extent is >= 4, odd or even."""
    odd = odd_code(oddExtents)
    shape = tuple(int(s) for s in shape)
    dim = len(shape)
    s3 = (ctypes.c_double * 3)(*([float(x) for x in sums] + [0.0] * (3 - dim)))
    c4 = (ctypes.c_int64 * 4)(*([int(x) for x in counts] + [0] * (3 - dim) + [int(off_axis)]))
    f3 = (ctypes.c_int * 3)()
    check(lib().omg_semicoarsen_rule_ragged(dim, (ctypes.c_int64 * dim)(*shape), s3, c4, -1 if line_axis is None else int(line_axis),
                                            int(level), odd, f3))
    return tuple(int(f3[d]) for d in range(dim))
