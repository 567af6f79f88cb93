"""parameters['nullspace'] / Hierarchy(nullspace=...) on the host side: what is refused before any device work, the
ctypes table, and the no-GPU failure mode of the new constructor.  CPU only."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip

NEW_ENTRIES = ("omg_hierarchy_create_opt", "omg_hierarchy_create_from_fine_opt", "omg_hierarchy_nullspace", "omg_level_project")


def ring(n):
    """periodic 1-D Laplacian: zero row and column sums"""
    i = np.arange(n)
    return sp.csr_matrix(sp.coo_matrix((np.concatenate([2.0 * np.ones(n), -np.ones(n), -np.ones(n)]),
                                        (np.concatenate([i, i, i]), np.concatenate([i, (i + 1) % n, (i - 1) % n]))), shape=(n, n)))


@pytest.mark.parametrize("bad", ["Constant", "const", 1, True, 0, "", ("constant",)])
def test_unknown_nullspace_is_a_value_error_before_any_device_work(bad):
    A0 = ring(16)
    b = np.ones(16)
    p = {"problemShape": (16,), "gridLevels": 1, "cycles": 1, "nullspace": bad}
    with pytest.raises(ValueError, match="nullspace"):
        openmg_amd.mgSolve(A0, b, dict(p))
    R = [sp.csr_matrix(np.kron(np.eye(8), [[0.5, 0.5]]))]
    A = [A0, sp.csr_matrix(R[0] @ A0 @ R[0].T)]
    with pytest.raises(ValueError, match="nullspace"):
        openmg_amd.mgCycle(A, b, 0, R, {"coarsestLevel": 1, "preIterations": 1, "postIterations": 1, "nullspace": bad})
    with pytest.raises(ValueError, match="nullspace"):
        _hip.Hierarchy(A, R, nullspace=bad)
    with pytest.raises(ValueError, match="nullspace"):
        _hip.Hierarchy.from_fine(A0, (4, 4), 1, nullspace=bad)


def test_codes_and_the_default():
    assert _hip.nullspace_code(None) == _hip.NULLSPACE_NONE == 0
    assert _hip.nullspace_code("constant") == _hip.NULLSPACE_CONSTANT == 1
    assert openmg_amd._nullspace_of({}) is None
    assert openmg_amd._nullspace_of({"nullspace": None}) is None
    assert openmg_amd._nullspace_of({"nullspace": "constant"}) == "constant"
    assert "nullspace" not in openmg_amd.defaults              # opt-in: the reference's defaults stay the reference's


def test_the_cache_key_tells_a_nullspace_hierarchy_from_a_plain_one():
    A0 = ring(16)
    R = [sp.csr_matrix(np.kron(np.eye(8), [[0.5, 0.5]]))]
    A = [A0, sp.csr_matrix(R[0] @ A0 @ R[0].T)]
    plain = openmg_amd._fingerprint(A, R, 2, 0, 1.0, 0)
    assert plain == openmg_amd._fingerprint(A, R, 2, 0, 1.0, 0, None)
    assert plain != openmg_amd._fingerprint(A, R, 2, 0, 1.0, 0, "constant")


def test_the_ctypes_table_lists_the_new_entries():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _hip.SIGNATURES, name
        assert hasattr(handle, name), name
    assert [f[0] for f in _hip.HierarchyOptions._fields_] == ["smoother", "omega", "dtype", "nullspace"]
    # int, double, int, int with the double 8-byte aligned: the C struct's layout
    assert ctypes.sizeof(_hip.HierarchyOptions) == 24
    assert _hip.HierarchyOptions.omega.offset == 8 and _hip.HierarchyOptions.dtype.offset == 16 and _hip.HierarchyOptions.nullspace.offset == 20


def views(A):
    A = [_hip.as_csr(M) for M in A]
    return A, (_hip.CsrView * len(A))(*[_hip.csr_view(M) for M in A])


def test_bad_options_are_refused_without_a_device():
    """an unknown nullspace kind, an unknown dtype and a null options pointer are OMG_ERR_INVALID, checked before the device is asked for"""
    keep, arrA = views([ring(8)])
    arrR = (_hip.CsrView * 1)()
    out = ctypes.c_void_p()
    for opt in (_hip.HierarchyOptions(0, 1.0, 0, 2), _hip.HierarchyOptions(0, 1.0, 0, -1), _hip.HierarchyOptions(0, 1.0, 7, 1)):
        code = _hip.lib().omg_hierarchy_create_opt(1, arrA, arrR, ctypes.byref(opt), ctypes.byref(out))
        assert code == _hip.ERR_INVALID and not out.value
        shape = (ctypes.c_int64 * 2)(4, 2)
        code = _hip.lib().omg_hierarchy_create_from_fine_opt(arrA, 2, shape, 1, ctypes.byref(opt), ctypes.byref(out))
        assert code == _hip.ERR_INVALID and not out.value
    assert b"nullspace" in _hip.lib().omg_last_error() or b"dtype" in _hip.lib().omg_last_error()
    assert _hip.lib().omg_hierarchy_create_opt(1, arrA, arrR, None, ctypes.byref(out)) == _hip.ERR_INVALID
    # every creating entry checks its options in the one place: the same refusals, the handle null, no device asked for
    shape = (ctypes.c_int64 * 2)(4, 2)
    field = _hip.KappaArgs(np.ones((6, 6, 6)), None, None, (1.0, 1.0, 1.0), None)
    entries = {"create_opt": lambda o: _hip.lib().omg_hierarchy_create_opt(1, arrA, arrR, o, ctypes.byref(out)),
               "from_fine_opt": lambda o: _hip.lib().omg_hierarchy_create_from_fine_opt(arrA, 2, shape, 1, o, ctypes.byref(out)),
               "from_fine_ragged": lambda o: _hip.lib().omg_hierarchy_create_from_fine_ragged(arrA, 2, shape, 1, None, 0, 0, o, ctypes.byref(out)),
               "from_kappa_spaced": lambda o: _hip.lib().omg_hierarchy_create_from_kappa_spaced(*field.call, 1, o, ctypes.byref(out))}
    for name, entry in entries.items():
        for opt, text in ((_hip.HierarchyOptions(0, 1.0, 0, 2), b"unknown nullspace kind"), (_hip.HierarchyOptions(0, 1.0, 0, -1), b"unknown nullspace kind"),
                          (_hip.HierarchyOptions(0, 1.0, 7, 1), b"unknown dtype"), (None, b"options are null")):
            out.value = 1                                                # (the entry itself clears the handle)
            code = entry(None if opt is None else ctypes.byref(opt))
            assert code == _hip.ERR_INVALID and not out.value and _hip.lib().omg_last_error() == text, (name, _hip.lib().omg_last_error())
    kind = ctypes.c_int(5)
    assert _hip.lib().omg_hierarchy_nullspace(None, ctypes.byref(kind)) == _hip.ERR_INVALID
    assert _hip.lib().omg_level_project(None, 0, None, None) == _hip.ERR_INVALID


@pytest.mark.skipif(_hip.device_count() > 0, reason="checks the no-GPU failure mode")
def test_create_opt_without_a_device_fails_loudly():
    keep, arrA = views([ring(8)])
    arrR = (_hip.CsrView * 1)()
    out = ctypes.c_void_p()
    opt = _hip.HierarchyOptions(0, 1.0, 0, _hip.NULLSPACE_CONSTANT)
    code = _hip.lib().omg_hierarchy_create_opt(1, arrA, arrR, ctypes.byref(opt), ctypes.byref(out))
    assert code == _hip.ERR_NO_DEVICE and not out.value
    with pytest.raises(_hip.HipError) as e:
        _hip.Hierarchy([ring(8)], [], nullspace="constant")
    assert e.value.code == _hip.ERR_NO_DEVICE
