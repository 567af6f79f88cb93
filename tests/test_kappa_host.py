"""operators.stencil7_kappa, the SciPy definition of the 7-point operator of a coefficient field that the device assembly
(csrc/kappa.hip) is pinned to: equal to stencil7_variable bit for bit on that function's kappa, symmetric, Neumann rows sum
to sigma, every refusal; the three C entries are declared, bound and exported; Solver.from_kappa refuses bad arguments
before it touches a device.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import openmg
import openmg_amd
from openmg_amd import _hip, operators

import kappa_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def variable_kappa(shape, seed=2024):
    nz, ny, nx = shape
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(10.0))


@pytest.mark.parametrize("shape", [(6, 5, 4), (16, 16, 16)])
def test_defaults_give_stencil7_variable_bit_for_bit(shape):
    A = operators.stencil7_kappa(variable_kappa(shape))
    B = operators.stencil7_variable(shape)
    assert A.shape == B.shape and A.indptr.dtype == np.int32 and A.indices.dtype == np.int32 and A.data.dtype == np.float64
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)
    assert A.has_sorted_indices


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 9), (2, 3, 70)])
@pytest.mark.parametrize("scale", kc.SCALES)
def test_symmetric_bit_for_bit_and_neumann_rows_sum_to_sigma(shape, scale):
    sigma = kc.sigma_of("field", shape)
    for wname in kc.WALLS:
        A = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS[wname], sigma, scale)
        assert (A != A.T).nnz == 0                         # (face(a, b) and a + b commute: the two entries of a face are one number)
        on_diagonal = A.indices == np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        assert (A.data[on_diagonal] > 0).all() and (A.data[~on_diagonal] < 0).all()
    A = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS["neumann"], sigma, scale)
    # a row's diagonal is the sum of its six couplings (+ sigma), each rounded once: the row sum is sigma to a few ulp of the diagonal
    rows = np.asarray(A.sum(axis=1)).ravel()
    assert np.all(np.abs(rows - sigma.ravel()) <= 8 * np.finfo(float).eps * A.diagonal())
    # a Dirichlet wall adds its face to the diagonal only: the row sums of the cells at that wall exceed sigma
    M = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS["mixed"], sigma, scale)
    nz, ny, nx = shape
    excess = (np.asarray(M.sum(axis=1)).ravel() - sigma.ravel()).reshape(shape)
    assert (excess[-1] > 0).all() and (excess[:, 0] > 0).all() and (excess[:, :, 0] > 0).all() and (excess[:, :, -1] > 0).all()
    inner = excess[:-1, 1:, 1:-1]                          # (-z and +y are Neumann)
    assert np.all(np.abs(inner) <= 8 * np.finfo(float).eps * M.diagonal().reshape(shape)[:-1, 1:, 1:-1])


def test_scalar_sigma_and_scale_enter_as_stated():
    shape = (4, 4, 4)
    k = kc.kappa_of(shape)
    A0 = operators.stencil7_kappa(k)
    A1 = operators.stencil7_kappa(k, sigma=0.375)
    assert np.array_equal(A1.indices, A0.indices)
    d = A0.indices == np.repeat(np.arange(64), np.diff(A0.indptr))
    assert np.array_equal(A1.data[d], A0.data[d] + 0.375) and np.array_equal(A1.data[~d], A0.data[~d])
    A2 = operators.stencil7_kappa(k, scale=(4.0, 4.0, 4.0))   # (a power of two: every entry scales exactly)
    assert np.array_equal(A2.data, 4.0 * A0.data)


def test_refusals():
    shape = (4, 5, 6)
    k = kc.kappa_of(shape)
    ok = operators.stencil7_kappa
    for bad in (k[0], k[None], k[:, :, :2], np.ones((2, 5, 5))):          # rank; no cells
        with pytest.raises(ValueError):
            ok(bad)
    with pytest.raises(ValueError):
        ok(k.astype(np.float32))
    for value in (np.nan, np.inf, 0.0, -1.0):
        for cell in ((2, 3, 4), (0, 3, 4), (2, 3, 7), (5, 1, 1)):           # a cell; ghost cells behind -z, +x, +z
            kb = k.copy()
            kb[cell] = value
            with pytest.raises(ValueError):
                ok(kb)
    # a ghost cell behind a Neumann wall is not read; an edge ghost cell never is
    kb = k.copy()
    kb[0, 3, 4] = np.nan
    kb[0, 0, 3] = -1.0
    A = ok(kb, walls=("neumann",) + ("dirichlet",) * 5)
    assert np.isfinite(A.data).all()
    for sigma in (-0.5, np.nan, np.inf, np.full(shape, -1.0), np.ones((4, 5, 5)), np.ones(4), "x"):
        with pytest.raises(ValueError):
            ok(k, sigma=sigma)
    field = np.ones(shape)
    field[1, 1, 1] = np.nan
    with pytest.raises(ValueError):
        ok(k, sigma=field)
    for scale in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (np.inf, 1.0, 1.0), (np.nan, 1.0, 1.0), (1.0, 1.0), 2.0, ("a", 1, 1)):
        with pytest.raises(ValueError):
            ok(k, scale=scale)
    for walls in (("dirichlet",) * 5, ("dirichlet",) * 5 + ("periodic",), ("neumann",) * 7, (0,) * 6):
        with pytest.raises(ValueError):
            ok(k, walls=walls)


def test_the_alias_package_exports_the_generator():
    assert openmg.operators.stencil7_kappa is operators.stencil7_kappa
    from openmg.operators import stencil7_kappa  # noqa: F401


def test_the_three_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name, n_args in (("omg_kappa_assemble", 12), ("omg_hierarchy_create_from_kappa", 11), ("omg_hierarchy_update_kappa", 9)):
        assert ("int %s(" % name) in text
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args
        assert hasattr(handle, name)
    for const in ("OMG_WALL_DIRICHLET 0", "OMG_WALL_NEUMANN   1", "OMG_SIGMA_NONE   0", "OMG_SIGMA_SCALAR 1", "OMG_SIGMA_FIELD  2"):
        assert "#define " + const in text
    assert (_hip.SIGMA_NONE, _hip.SIGMA_SCALAR, _hip.SIGMA_FIELD) == (0, 1, 2) and operators.WALLS == ("dirichlet", "neumann")


def test_solver_from_kappa_refuses_bad_arguments_before_device_work(monkeypatch):
    # (any device work would go through the library: none may be reached)
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (8, 8, 8)
    k = kc.kappa_of(shape)
    p = {"gridLevels": 2, "cycles": 2, "smoother": "colour"}
    S = openmg_amd.Solver.from_kappa
    bad = [lambda: S(k[0], p), lambda: S(k.astype(np.float32), p), lambda: S(k, dict(p, problemShape=(8, 8, 4))),
           lambda: S(k, dict(p, problemShape=(512,))), lambda: S(k, p, walls=("dirichlet",) * 5), lambda: S(k, p, walls=("wall",) * 6),
           lambda: S(k, p, sigma=-1.0), lambda: S(k, p, sigma=np.nan), lambda: S(k, p, sigma=np.ones((8, 8, 4))),
           lambda: S(k, p, scale=(1.0, 0.0, 1.0)), lambda: S(k, p, scale=(1.0, np.inf, 1.0)), lambda: S(k, p, scale=(1.0, 1.0)),
           lambda: S(k, dict(p, smoother="nope")), lambda: S(k, dict(p, accel="gmres")), lambda: S(k, dict(p, rtol=-1.0))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: _hip.KappaArgs(k[0]), lambda: _hip.Hierarchy.from_kappa(k, 1, scale=(0.0, 1.0, 1.0)),
                 lambda: _hip.kappa_assemble(k, walls=("x",) * 6)):
        with pytest.raises(ValueError):
            call()
    a = _hip.KappaArgs(k, kc.WALLS["mixed"], 0.5, (4.0, 1.0, 0.25))
    assert a.grid == shape and a.shape == (512, 512) and a.nnz == 7 * 512 - 6 * 64 and a.walls == (1, 0, 0, 1, 0, 0)
