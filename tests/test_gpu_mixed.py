"""Mixed-precision solves (OMG_DTYPE_MIXED; mgSolve 'dtype': 'mixed'): fp32 levels and V-cycles inside fp64 iterations on
the finest level.  Mixed PCG and mixed defect correction must reach fp64 accuracy (an fp32 hierarchy cannot), report
fp64 norms of b - A x, repeat bit for bit, give the same bits on both setup routes and after update_fine, and refuse the
entries that would hand back an fp32-accurate answer."""
import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc
from test_gpu_pcg import _kind, pcg_gpu
from test_gpu_var7_update import DeviceValues

pytestmark = pytest.mark.gpu

OMG_ERR_UNSUPPORTED = 7


def plane_kind(n=32):
    """0.1 * Poisson: constants that float cannot represent (a solve that read rounded ones would stall near 1e-8)."""
    shape = (n,) * 3
    A0 = sp.csr_matrix(0.1 * operators.stencil_poisson(shape))
    R = orc.restriction_list(shape, 3, 8)
    A = orc.coefficient_list(A0, R)
    b = np.random.default_rng(7).standard_normal(A0.shape[0])
    return A, R, b, {"smoother": "colour"}, "plane"


def kind(name):
    if name == "plane":
        return plane_kind()
    A, R, b, kw, _, flag = _kind(name)
    return A, R, b, kw, flag


def true_norm(A0, b, x):
    return np.linalg.norm(b - A0 @ x)


def same_norm(got, A0, b, x, rel):
    """got == ||b - A0 x|| to `rel`, up to the rounding of forming b - A0 x in fp64 at all"""
    t = true_norm(A0, b, x)
    floor = 1e-14 * (np.linalg.norm(b) + np.linalg.norm(abs(A0) @ np.abs(x)))
    return abs(got - t) <= rel * t + floor


KINDS3 = ["plane", "var7_sym", "var7_general", "s27", "gs", "jacobi"]


@pytest.mark.parametrize("name", KINDS3 + ["tile2d", "1d"])
def test_mixed_pcg_reaches_fp64_accuracy(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    monkeypatch.setenv("OMG_VAR7_SYM", "0" if name == "var7_general" else "1")
    A, R, b, kw, flag = kind(name)
    nb = np.linalg.norm(b)
    budget = 300
    with _hip.Hierarchy(A, R, **kw) as h64:
        its64, _, _, _, _ = pcg_gpu(h64, b, 1, 1, budget, 1e-8 * nb)
        _, _, _, _, x64 = pcg_gpu(h64, b, 1, 1, budget, 1e-10 * nb)
    with _hip.Hierarchy(A, R, **dict(kw, dtype="mixed")) as hm:
        assert hm.device_dtype() == np.float32
        if flag:
            assert hm.level_flags(0)[flag], name
        itsm, _, _, bd, _ = pcg_gpu(hm, b, 1, 1, budget, 1e-8 * nb)
        assert not bd
        assert itsm <= its64 + 2, (name, itsm, its64)
        _, _, tn, bd, xm = pcg_gpu(hm, b, 1, 1, budget, 1e-10 * nb)
        assert not bd
    with _hip.Hierarchy(A, R, **dict(kw, dtype="float32")) as h32:
        _, _, _, _, x32 = pcg_gpu(h32, b, 1, 1, budget, 1e-10 * nb)
    tm = true_norm(A[0], b, xm)
    assert same_norm(tn, A[0], b, xm, 1e-12), (tn, tm)
    if name in KINDS3:
        assert tm <= 1e-10 * nb, (name, tm / nb)
    else:
        assert tm <= max(1e-10 * nb, 10 * true_norm(A[0], b, x64)), (name, tm / nb)
    assert true_norm(A[0], b, x32) > 1e-8 * nb, name


@pytest.mark.parametrize("name", ["plane", "var7_sym", "gs"])
def test_defect_correction(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    monkeypatch.setenv("OMG_VAR7_SYM", "1")
    A, R, b, kw, _ = kind(name)
    nb = np.linalg.norm(b)
    with _hip.Hierarchy(A, R, **kw) as h64:
        h64.resident_load(b)
        h64.resident_cycle(1, 1)
        x1_64 = h64.resident_fetch()
    with _hip.Hierarchy(A, R, **dict(kw, dtype="mixed")) as hm:
        hm.resident_load(b)
        norms, xs = [], []
        for _ in range(6):
            norms.append(hm.resident_cycle(1, 1))
            xs.append(hm.resident_fetch())
        for nk, xk in zip(norms, xs):
            assert same_norm(nk, A[0], b, xk, 1e-12), (nk, true_norm(A[0], b, xk))
        np.testing.assert_allclose(xs[0], x1_64, rtol=0, atol=1e-5 * np.abs(x1_64).max())
        # the batched entry gives the same bits as single cycles, and the run goes on to fp64 accuracy
        hm.resident_load(b)
        batch = hm.resident_cycles(1, 1, 400)
        assert np.array_equal(batch[:6], np.array(norms))
        assert batch[-1] <= 1e-10 * nb, batch[-1] / nb
        assert true_norm(A[0], b, hm.resident_fetch()) <= 1e-10 * nb


@pytest.mark.parametrize("name", ["plane", "var7_sym"])
def test_bits_repeat_and_graph_mode_changes_nothing(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    monkeypatch.setenv("OMG_VAR7_SYM", "1")
    A, R, b, kw, _ = kind(name)
    tol = 1e-10 * np.linalg.norm(b)

    def both(h):
        p = pcg_gpu(h, b, 1, 1, 200, tol)
        h.resident_load(b)
        c = h.resident_cycles(1, 1, 5)
        return p, c, h.resident_fetch()

    with _hip.Hierarchy(A, R, **dict(kw, dtype="mixed")) as h:
        first, second = both(h), both(h)
        h.use_graph(True)
        graphed = both(h)
        h.use_graph(False)
    for other in (second, graphed):
        assert other[0][0] == first[0][0] and other[0][2] == first[0][2]
        assert np.array_equal(other[0][1], first[0][1]) and np.array_equal(other[0][4], first[0][4])
        assert np.array_equal(other[1], first[1]) and np.array_equal(other[2], first[2])


def _fine(name, shape):
    if name == "plane":
        return sp.csr_matrix(0.1 * operators.stencil_poisson(shape))
    if name == "var7":
        return operators.stencil7_variable(shape, seed=1)
    return sp.csr_matrix(operators.stencil27_variable(shape))


@pytest.mark.parametrize("name", ["plane", "var7", "s27"])
def test_lists_route_and_from_fine_agree(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (32, 32, 32)
    A0 = _fine(name, shape)
    R = operators.restrictionList(shape, 2, 8)
    A = operators.coeffecientList(A0, R)
    b = np.random.default_rng(9).standard_normal(A0.shape[0])
    tol = 1e-10 * np.linalg.norm(b)
    out = []
    for h in (_hip.Hierarchy(A, R, smoother="colour", dtype="mixed"),
              _hip.Hierarchy.from_fine(A0, shape, len(R), smoother="colour", dtype="mixed")):
        with h:
            flags = h.level_flags(0)
            p = pcg_gpu(h, b, 1, 1, 200, tol)
            h.resident_load(b)
            c = h.resident_cycles(1, 1, 4)
            out.append((flags, p, c, h.resident_fetch()))
    (f1, p1, c1, x1), (f2, p2, c2, x2) = out
    assert f1 == f2 and f1[{"plane": "plane", "var7": "var7", "s27": "stencil27"}[name]]
    assert p1[0] == p2[0] and np.array_equal(p1[1], p2[1]) and np.array_equal(p1[4], p2[4]) and p1[2] == p2[2]
    assert np.array_equal(c1, c2) and np.array_equal(x1, x2)
    assert true_norm(A0, b, p1[4]) <= 1e-10 * np.linalg.norm(b)


@pytest.mark.parametrize("name", ["var7", "s27"])
def test_update_fine_gives_the_fresh_bits(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (32, 32, 32)
    if name == "var7":
        A1, A2 = operators.stencil7_variable(shape, seed=1), operators.stencil7_variable(shape, seed=2)
    else:
        A1 = sp.csr_matrix(operators.stencil27_variable(shape, seed=1))
        A2 = sp.csr_matrix(operators.stencil27_variable(shape, seed=2))
    assert np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices)
    b = np.random.default_rng(3).standard_normal(A1.shape[0])
    tol = 1e-10 * np.linalg.norm(b)

    def run(h):
        p = pcg_gpu(h, b, 1, 1, 200, tol)
        h.resident_load(b)
        return p, h.resident_cycles(1, 1, 3), h.resident_fetch()

    with _hip.Hierarchy.from_fine(A2, shape, 2, "colour", dtype="mixed") as fresh, \
            _hip.Hierarchy.from_fine(A1, shape, 2, "colour", dtype="mixed") as h:
        want = run(fresh)
        h.update_fine(A2.data)
        got = run(h)
    assert got[0][0] == want[0][0] and np.array_equal(got[0][1], want[0][1]) and np.array_equal(got[0][4], want[0][4])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert true_norm(A2, b, got[0][4]) <= 1e-10 * np.linalg.norm(b)


# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as tests/test_gpu_pcg.py does)
MGSOLVE = """
import sys
import numpy as np
import scipy.sparse as sp
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import openmg_amd
from openmg_amd import operators
A0 = sp.csr_matrix(0.1 * operators.stencil_poisson((32, 32, 32)))
b = np.random.default_rng(5).standard_normal(A0.shape[0])
nb = np.linalg.norm(b)
for accel in (None, "cg"):
    p = lambda **kw: dict({"problemShape": (32, 32, 32), "gridLevels": 3, "preIterations": 1, "postIterations": 1,
                           "cycles": 600, "threshold": 1e-10 * nb, "smoother": "colour", "dtype": "mixed", "accel": accel}, **kw)
    u, info = openmg_amd.mgSolve(A0, b, p(giveInfo=True))              # the lists route
    u2 = openmg_amd.mgSolve(A0, b, p())                                 # the device setup route
    ud = openmg_amd.mgSolve(A0, torch.tensor(b, device="cuda"), p())
    assert u.dtype == np.float64 and ud.dtype == torch.float64 and ud.is_cuda
    assert np.array_equal(u, u2) and np.array_equal(ud.cpu().numpy(), u), accel
    t = np.linalg.norm(b - A0 @ u)
    assert t <= 1e-10 * nb, (accel, t / nb)
    assert abs(info["norm"] - t) <= 1e-12 * t + 1e-14 * nb, (accel, info["norm"], t)
print("mixed mgSolve ok")
"""


def test_mgsolve_mixed_both_accels_host_and_device_b():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", MGSOLVE, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "mixed mgSolve ok" in p.stdout, p.stderr[-3000:]


def test_refused_entries_and_dtype():
    A, R, b, kw, _ = plane_kind(16)
    n = b.size
    x = np.zeros(n)
    with _hip.Hierarchy(A, R, **dict(kw, dtype="mixed")) as h:
        assert h.device_dtype() == np.float32
        code = ctypes_code(h)
        assert code == _hip.DTYPE_MIXED
        calls = [lambda: h.vcycle(b, x, 1, 1), lambda: h.vcycle_ex(b, None, x, None, 1, 1),
                 lambda: h.solve(b, x, 1, 1, 2, 0.0)]
        with DeviceValues(b) as (bd, _), DeviceValues(x) as (xd, _):
            calls += [lambda: h.vcycle_dev(bd, None, xd, None, 1, 1), lambda: h.cycle_dev(bd, xd, 1, 1)]
            for call in calls:
                with pytest.raises(_hip.HipError, match="resident") as e:
                    call()
                assert e.value.code == OMG_ERR_UNSUPPORTED
        # the per-level operations act on the fp32 levels
        assert h.spmv(0, b).dtype == np.float64
    with pytest.raises(_hip.HipError, match="INVALID|update|from_fine|27-point"):
        with _hip.Hierarchy.from_fine(sp.csr_matrix(0.1 * operators.stencil_poisson((16, 16, 16))), (16, 16, 16), 2,
                                      "colour", dtype="mixed") as hp:
            hp.update_fine(np.ones(hp_nnz(16)))


def hp_nnz(n):
    return operators.stencil_poisson((n, n, n)).nnz


def ctypes_code(h):
    import ctypes
    c = ctypes.c_int(-1)
    _hip.check(_hip.lib().omg_hierarchy_dtype(h._h, ctypes.byref(c)))
    return c.value


def test_256_plane_reaches_1e10():
    shape = (256, 256, 256)
    A0 = sp.csr_matrix(0.1 * operators.stencil_poisson(shape))
    b = np.random.default_rng(1).standard_normal(A0.shape[0])
    nb = np.linalg.norm(b)
    p = {"problemShape": shape, "gridLevels": 5, "preIterations": 1, "postIterations": 1, "cycles": 200,
         "threshold": 1e-10 * nb, "smoother": "colour", "dtype": "mixed", "accel": "cg"}
    u = openmg_amd.mgSolve(A0, b, p)
    assert true_norm(A0, b, u) <= 1e-10 * nb
