"""Flexible preconditioned CG on the resident finest level (omg_resident_pcg, csrc/pcg.hip; mgSolve's 'accel': 'cg'):
against a CPU FCG(1) written around the oracle's own V-cycle, on every kind of level, bit-repeatable, and in the resident
contract."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-8


@functools.lru_cache(maxsize=None)
def _problem(name, n, grids):
    shape = (n,) * 3
    A0 = operators.stencil_poisson(shape) if name == "poisson" else operators.stencil7_variable(shape)
    R = orc.restriction_list(shape, grids - 1, 8)
    A = orc.coefficient_list(A0, R)
    b = np.random.default_rng(7).standard_normal(A0.shape[0])
    return A0, A, R, b


_smoothers = {}


def smoother_for(kind, A):
    key = (kind, id(A[0]))
    if key not in _smoothers:
        _smoothers[key] = orc.make_smoother(kind, A)
    return _smoothers[key]


def fcg_cpu(A, R, b, kind, pre, post, tol, maxit, x0=None):
    """The yardstick: FCG(1), Polak-Ribiere, one oracle V-cycle from zero per iteration."""
    sm = smoother_for(kind, A)
    par = {"coarsestLevel": len(R), "preIterations": pre, "postIterations": post}
    M = lambda r: orc.mg_cycle(A, r, 0, R, par, smoother=sm)[0]
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b - A[0] @ x
    z = M(r)
    p = z.copy()
    rho = r @ z
    norms = []
    for _ in range(maxit):
        q = A[0] @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        norms.append(np.linalg.norm(r))
        if norms[-1] < tol:
            break
        z = M(r)
        beta = -alpha * (z @ q) / rho
        rho = r @ z
        p = z + beta * p
    return np.array(norms), x


def pcg_gpu(h, b, pre, post, maxit, tol, x0=None):
    h.resident_load(b, x0)
    its, norms, tn, bd = h.resident_pcg(pre, post, maxit, tol)
    return its, norms, tn, bd, h.resident_fetch()


def plain_reaches(h, b, pre, post, n, tol):
    """Do n plain V-cycles from zero reach tol?"""
    h.resident_load(b)
    return h.resident_cycles(pre, post, n)[-1] < tol


@pytest.mark.parametrize("route", ["lists", "from_fine"])
@pytest.mark.parametrize("pre,post", [(1, 1), (1, 0)])
@pytest.mark.parametrize("name", ["poisson", "var7"])
def test_against_the_cpu_yardstick(name, pre, post, route):
    A0, A, R, b = _problem(name, 32, 4)
    tol = TOL * np.linalg.norm(b)
    want_norms, want_x = fcg_cpu(A, R, b, "colour", pre, post, tol, 200)
    if route == "lists":
        h = _hip.Hierarchy(A, R, smoother="colour")
    else:
        h = _hip.Hierarchy.from_fine(A0, (32, 32, 32), 3, smoother="colour")
    with h:
        its, norms, tn, bd, x = pcg_gpu(h, b, pre, post, 200, tol)
    assert not bd
    assert abs(its - len(want_norms)) <= 1, (its, len(want_norms))
    m = min(its, len(want_norms))
    np.testing.assert_allclose(norms[:m], want_norms[:m], rtol=1e-8)
    np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
    assert tn <= 2 * tol


def _kind(name):
    """(A list, R list, b, Hierarchy kwargs, oracle smoother kind, the level-0 flag that must hold)"""
    if name in ("plane", "gs", "jacobi", "fp32"):
        _, A, R, b = _problem("poisson", 32, 4)
        kw = {"smoother": {"gs": "gs", "jacobi": "jacobi"}.get(name, "colour")}
        if name == "jacobi":
            kw["omega"] = 2.0 / 3.0
        if name == "fp32":
            kw["dtype"] = "float32"
        return A, R, b, kw, kw["smoother"], {"plane": "plane", "fp32": "plane", "gs": "march"}.get(name)
    if name.startswith("var7"):
        _, A, R, b = _problem("var7", 32, 4)
        return A, R, b, {"smoother": "colour"}, "colour", "var7"
    if name == "s27":
        from test_gpu_plane import aggregation
        shape = (32, 32, 32)
        A, R = [sp.csr_matrix(operators.stencil27_variable(shape))], []
        for l in range(2):
            R.append(aggregation(tuple(s >> l for s in shape)))
            Ac = sp.csr_matrix((R[-1] @ A[-1]) @ R[-1].T)
            Ac.sort_indices()
            A.append(Ac)
        b = np.random.default_rng(3).standard_normal(A[0].shape[0])
        return A, R, b, {"smoother": "colour"}, "colour", "stencil27"
    if name == "tile2d":
        shape = (256, 256)
        A0 = operators.stencil_poisson(shape)
        R = orc.restriction_list(shape, 4, 8)
        A = orc.coefficient_list(A0, R)
        b = np.random.default_rng(4).standard_normal(A0.shape[0])
        return A, R, b, {"smoother": "colour"}, "colour", "plane"
    if name == "1d":
        A0 = sp.csr_matrix(orc.poisson((4096,), sparse=True))
        R = orc.restriction_list((4096,), 5, 8)
        A = orc.coefficient_list(A0, R)
        b = np.random.default_rng(5).standard_normal(4096)
        return A, R, b, {"smoother": "colour"}, "colour", None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["plane", "var7_sym", "var7_general", "s27", "tile2d", "1d", "gs", "jacobi", "fp32"])
def test_every_kind_converges(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    monkeypatch.setenv("OMG_VAR7_SYM", "0" if name == "var7_general" else "1")
    A, R, b, kw, kind, flag = _kind(name)
    rel = 1e-5 if name == "fp32" else TOL
    tol = rel * np.linalg.norm(b)
    want = len(fcg_cpu(A, R, b, kind, 1, 1, tol, 300)[0])
    with _hip.Hierarchy(A, R, **kw) as h:
        if flag:
            assert h.level_flags(0)[flag], name
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 300, tol)
        assert not bd and norms[-1] < tol and np.isfinite(x).all()
        assert its <= want + 2, (name, its, want)
        assert not plain_reaches(h, b, 1, 1, its, tol), name
        if name == "plane":
            # the generic path (p update, the row kernels' SpMV, dot) on the same hierarchy
            h.use_plane(False)
            its2, norms2, _, _, _ = pcg_gpu(h, b, 1, 1, 300, tol)
            assert its2 == its
            np.testing.assert_allclose(norms2, norms, rtol=1e-12)


@pytest.mark.parametrize("name", ["plane", "var7_sym"])
def test_bits_repeat_and_graph_mode_changes_nothing(monkeypatch, name):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    monkeypatch.setenv("OMG_VAR7_SYM", "1")
    A, R, b, kw, _, _ = _kind(name)
    tol = TOL * np.linalg.norm(b)
    with _hip.Hierarchy(A, R, **kw) as h:
        first = pcg_gpu(h, b, 1, 1, 100, tol)
        second = pcg_gpu(h, b, 1, 1, 100, tol)
        h.use_graph(True)
        h.resident_load(b)
        h.resident_cycle(1, 1)            # (a captured cycle exists; the PCG still runs eagerly)
        graphed = pcg_gpu(h, b, 1, 1, 100, tol)
        h.use_graph(False)
    for other in (second, graphed):
        assert other[0] == first[0]
        assert np.array_equal(other[1], first[1])
        assert np.array_equal(other[4], first[4])
        assert other[2] == first[2]


def test_resident_contract():
    _, A, R, b = _problem("poisson", 32, 4)
    x0 = np.random.default_rng(11).standard_normal(b.size)
    want_norms, want_x = fcg_cpu(A, R, b, "colour", 1, 1, 0.0, 3, x0=x0)
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 3, 0.0, x0=x0)
        assert its == 3 and not bd
        np.testing.assert_allclose(norms, want_norms, rtol=1e-8)
        np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
        true = np.linalg.norm(b - A[0] @ x)
        assert abs(tn - true) <= 1e-12 * true, (tn, true)
        assert np.array_equal(h.resident_fetch(), x)
        n1 = h.resident_cycle(1, 1)
        after = h.resident_fetch()
    with _hip.Hierarchy(A, R, smoother="colour") as fresh:
        fresh.resident_load(b, x)
        n2 = fresh.resident_cycle(1, 1)
        assert np.array_equal(fresh.resident_fetch(), after)
        assert n1 == n2


def _params(**kw):
    p = {"problemShape": (32, 32, 32), "gridLevels": 3, "preIterations": 1, "postIterations": 1, "smoother": "colour",
         "cycles": 0, "threshold": 0.0, "giveInfo": True, "minSize": 8}
    p.update(kw)
    return p


# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as tests/devarray_worker.py does)
DEVICE_B = """
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import openmg_amd
from openmg_amd import operators
A0 = operators.stencil_poisson((32, 32, 32))
b = np.random.default_rng(7).standard_normal(A0.shape[0])
p = lambda: {"problemShape": (32, 32, 32), "gridLevels": 3, "smoother": "colour", "preIterations": 1, "postIterations": 1,
             "cycles": 0, "threshold": 1e-8 * np.linalg.norm(b), "accel": "cg"}
ud = openmg_amd.mgSolve(A0, torch.tensor(b, device="cuda"), p())
assert isinstance(ud, torch.Tensor) and ud.is_cuda
assert np.array_equal(ud.cpu().numpy(), openmg_amd.mgSolve(A0, b, p()))
print("device b ok")
"""


def test_mgsolve_accel_cg_with_a_device_b():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_B, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "device b ok" in p.stdout, p.stderr[-3000:]


def test_mgsolve_accel_cg():
    A0, A, R, b = _problem("poisson", 32, 4)
    tol = TOL * np.linalg.norm(b)
    u, info = openmg_amd.mgSolve(A0, b, _params(threshold=tol, accel="cg"))
    assert info["norm"] <= 2 * tol and 5 <= info["cycle"] <= 40
    assert abs(info["norm"] - np.linalg.norm(b - A0 @ u)) <= 1e-6 * info["norm"]
    # 'cycles' caps the iterations; the dict is completed exactly as without 'accel'
    p_cg, p_plain = _params(cycles=4, accel="cg"), _params(cycles=4)
    _, info = openmg_amd.mgSolve(A0, b, p_cg)
    openmg_amd.mgSolve(A0, b, p_plain)
    assert info["cycle"] == 4
    p_cg.pop("accel")
    assert p_cg == p_plain
    # threshold and cycles together: whichever comes first
    _, info = openmg_amd.mgSolve(A0, b, _params(cycles=200, threshold=1e-3 * np.linalg.norm(b), accel="cg"))
    assert info["cycle"] < 200
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A0, b, _params(accel="cg"))
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A0, b, _params(threshold=1.0, accel="gmres"))
    # mgCycle ignores the key
    x1, i1 = openmg_amd.mgCycle(A, b, 0, R, {"coarsestLevel": 3, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg"})
    x2, i2 = openmg_amd.mgCycle(A, b, 0, R, {"coarsestLevel": 3, "preIterations": 1, "postIterations": 1, "smoother": "colour"})
    assert np.array_equal(x1, x2)
    openmg_amd.clear_cache()


def inclusion_operator(n=32):
    """-div(kappa grad u) on n^3 cells, kappa = 1 or 1e3 (20 % of the cells), harmonic-mean face couplings, Dirichlet faces
    adding the cell's kappa to the diagonal."""
    kappa = np.where(np.random.default_rng(1).random((n, n, n)) < 0.2, 1e3, 1.0)
    idx = np.arange(n ** 3).reshape(n, n, n)
    rows, cols, vals = [], [], []
    diag = np.zeros((n, n, n))
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        k1, k2 = kappa[tuple(lo)], kappa[tuple(hi)]
        w = 2.0 * k1 * k2 / (k1 + k2)
        i1, i2 = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [i1, i2]
        cols += [i2, i1]
        vals += [-w.ravel(), -w.ravel()]
        diag[tuple(lo)] += w
        diag[tuple(hi)] += w
        first, last = [slice(None)] * 3, [slice(None)] * 3
        first[ax], last[ax] = 0, n - 1
        diag[tuple(first)] += kappa[tuple(first)]
        diag[tuple(last)] += kappa[tuple(last)]
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3))
    A.sort_indices()
    return A


def test_high_contrast_inclusions():
    A0 = inclusion_operator()
    b = np.random.default_rng(2).standard_normal(A0.shape[0])
    tol = TOL * np.linalg.norm(b)
    p = _params(threshold=tol, cycles=200, gridLevels=3, accel="cg")
    u, info = openmg_amd.mgSolve(A0, b, p)
    assert info["norm"] < 2 * tol and info["cycle"] < 200, info["cycle"]
    R = orc.restriction_list((32, 32, 32), 3, 8)
    A = orc.coefficient_list(A0, R)
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        assert not plain_reaches(h, b, 1, 1, 400, tol)


def test_indefinite_shift_breaks_down_cleanly():
    n = 32
    A0 = operators.stencil_poisson((n,) * 3)
    l1 = 2 - 2 * np.cos(np.pi / (n + 1))
    l2 = 2 - 2 * np.cos(2 * np.pi / (n + 1))
    sigma = 0.5 * (3 * l1 + (2 * l1 + l2))               # between the two smallest eigenvalues
    As = sp.csr_matrix(A0 - sigma * sp.identity(A0.shape[0], format="csr"))
    As.sort_indices()
    R = orc.restriction_list((n,) * 3, 3, 8)
    A = orc.coefficient_list(As, R)
    b = np.random.default_rng(9).standard_normal(As.shape[0])
    tol = TOL * np.linalg.norm(b)
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 200, tol)
    assert np.isfinite(x).all() and np.isfinite(norms).all()
    assert bd or its == 200 or norms[-1] < tol
    p = _params(threshold=tol, cycles=200, gridLevels=3, accel="cg")
    if bd:
        with pytest.raises(RuntimeError, match="iteration %d" % (its + 1)):
            openmg_amd.mgSolve(As, b, p)
    else:
        u = openmg_amd.mgSolve(As, b, p)[0]
        assert np.isfinite(u).all()
