"""operators.rhs_kappa, the NumPy definition of the right-hand side that goes with operators.stencil7_kappa (the device
kernel of csrc/kappa.hip is pinned to it bit for bit: tests/test_gpu_kappa_rhs.py): every refusal, consistency with the
operator's wall coefficients, exactness on linear fields (the test that pins both sign conventions), second order on a
manufactured problem, the ghost cells it must not read; the new C entries are declared and bound.  CPU only."""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import openmg_amd
from openmg_amd import _hip, operators

import kappa_rhs_cases as rc
from kappa_rhs_cases import D, N, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def bad_calls(shape):
    """(walls, f, values, scale, spacing) that every layer must refuse with ValueError."""
    nz, ny, nx = shape
    ok_spacing = tuple(rc.widths(n, 1.5, "mirror") for n in shape)
    periodic_x = (D, D, N, N, P, P)
    return [
        (None, np.ones((nz, ny)), None, (1.0,) * 3, None),                          # f of another shape
        (None, np.ones(nz * ny * nx), None, (1.0,) * 3, None),                      # ... flattened
        (None, "f", None, (1.0,) * 3, None),
        (None, None, (1.0,) * 5, (1.0,) * 3, None),                                 # wrong count
        (None, None, (1.0,) * 7, (1.0,) * 3, None),
        (None, None, 1.0, (1.0,) * 3, None),
        (None, None, (np.ones((ny, nx + 1)),) + (None,) * 5, (1.0,) * 3, None),     # wrong shape on -z
        (None, None, (None, None, np.ones((ny, nx)), None, None, None), (1.0,) * 3, None),    # a z-wall field on -y
        (None, None, (None,) * 5 + (np.ones(nz * ny),), (1.0,) * 3, None),          # 1-D on +x
        (None, None, ("g",) + (None,) * 5, (1.0,) * 3, None),
        (periodic_x, None, (None,) * 4 + (1.0, None), (1.0,) * 3, None),            # a value on a periodic wall
        (periodic_x, None, (None,) * 5 + (np.ones((nz, ny)),), (1.0,) * 3, None),
        ((D,) * 5, None, None, (1.0,) * 3, None),                                   # what kappa_arguments refuses
        ((D, D, D, D, P, D), None, None, (1.0,) * 3, None),
        (None, None, None, (1.0, 0.0, 1.0), None),
        (None, None, None, (2.0, 1.0, 1.0), ok_spacing),                            # spacing and scale exclude each other
        (None, None, None, (1.0,) * 3, ok_spacing[:2]),                             # what spacing_arguments refuses
        (None, None, None, (1.0,) * 3, (ok_spacing[0], ok_spacing[1], -ok_spacing[2])),
    ]


def test_every_refusal_is_a_value_error_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (3, 4, 5)
    kappa = np.ones(tuple(n + 2 for n in shape))
    for walls, f, values, scale, spacing in bad_calls(shape):
        for fn in (operators.rhs_kappa, _hip.kappa_rhs):
            with pytest.raises(ValueError):
                fn(kappa, f, walls, values, scale, spacing)
    for fn in (operators.rhs_kappa, _hip.kappa_rhs):
        for bad in (kappa[0], kappa.astype(np.float32), np.ones((2, 5, 5))):
            with pytest.raises(ValueError):
                fn(bad)
    # out: a NumPy array of another size, or not float64
    for out in (np.empty(59), np.empty(shape, dtype=np.float32), np.empty((3, 4, 10))[:, :, ::2]):
        with pytest.raises(ValueError):
            _hip.kappa_rhs(kappa, out=out)

    class FakeDevice:
        def __init__(self, shape):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (4096, False), "version": 2, "strides": None}
    # arrays on both sides; an `out` on the other side; a device `out` of another size
    for call in (lambda: _hip.kappa_rhs(kappa, FakeDevice(shape)),
                 lambda: _hip.kappa_rhs(FakeDevice(kappa.shape), np.ones(shape)),
                 lambda: _hip.kappa_rhs(FakeDevice(kappa.shape), 1.0, values=(np.ones((4, 5)),) + (None,) * 5),
                 lambda: _hip.kappa_rhs(kappa, out=FakeDevice((60,))),
                 lambda: _hip.kappa_rhs(FakeDevice(kappa.shape), out=np.empty(60)),
                 lambda: _hip.kappa_rhs(FakeDevice(kappa.shape), out=FakeDevice((59,)))):
        with pytest.raises(ValueError):
            call()


def test_solver_rhs_wants_a_from_kappa_solver_and_its_grid(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    s = openmg_amd.Solver.__new__(openmg_amd.Solver)      # (no device here: the object alone, as __init__ leaves a matrix solver)
    s._hierarchy = object()
    kappa = np.ones((5, 6, 7))
    with pytest.raises(ValueError, match="from_kappa"):
        s.rhs(kappa)
    s._kappa = ((3, 4, 5), None, (1.0, 1.0, 1.0), None)
    with pytest.raises(ValueError, match="grid"):
        s.rhs(np.ones((5, 6, 8)))
    for walls, f, values, scale, spacing in bad_calls((3, 4, 5))[:10]:
        with pytest.raises(ValueError):
            s.rhs(kappa, f, values)
    s._hierarchy = None                                    # (__del__ closes nothing)


def two_decades(shape, seed=7):
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=tuple(n + 2 for n in shape)) * np.log(10.0))


@pytest.mark.parametrize("shape", [(4, 5, 6), (1, 1, 1), (2, 7, 3)])
@pytest.mark.parametrize("grid", ["scale", "spacing"])
def test_all_dirichlet_value_one_is_the_operator_applied_to_ones(shape, grid):
    kappa = two_decades(shape)
    if grid == "scale":
        how = dict(scale=(0.3, 1.7, 2.9))
    else:       # ghost widths 0 along z, the boundary cell's along y, something else along x
        how = dict(spacing=(rc.widths(shape[0], 1.2, 0.0), rc.widths(shape[1], 1.8, "mirror"), rc.widths(shape[2], 0.0, 0.013)))
    A = operators.stencil7_kappa(kappa, **how)
    b = operators.rhs_kappa(kappa, values=(1.0,) * 6, **how)
    assert b.shape == shape and b.dtype == np.float64
    # per row: both are the sum of the row's wall coefficients — b adds them, A @ 1 cancels the in-grid faces out of the
    # diagonal's sum; seven roundings in each, every one at most an ulp of the row's sum of magnitudes
    bound = 16 * EPS * np.asarray(abs(A).sum(axis=1)).ravel()
    assert np.all(np.abs(A @ np.ones(A.shape[0]) - b.ravel()) <= bound)
    # fields of ones are the scalar
    fields = tuple(np.ones((shape[a], shape[c])) for a, c in rc.WALL_AXES)
    assert np.array_equal(operators.rhs_kappa(kappa, values=fields, **how), b)


LINEAR_WALLS = [(D, N, N, D, D, N), (N, D, D, N, N, D), (D,) * 6]


@pytest.mark.parametrize("walls", LINEAR_WALLS)
@pytest.mark.parametrize("grid", ["uniform", "stretched mirror", "stretched face", "stretched mixed"])
def test_a_linear_field_is_reproduced_exactly(walls, grid):
    shape = (6, 7, 9)
    if grid == "uniform":
        spacing = None
    else:
        ghosts = {"stretched mirror": ("mirror",) * 3, "stretched face": (0.0,) * 3, "stretched mixed": (0.0, "mirror", 0.02)}[grid]
        spacing = tuple(rc.widths(n, 1.6, g) for n, g in zip(shape, ghosts))
    kappa, scale, values, u = rc.linear_problem(shape, walls, spacing)
    A = operators.stencil7_kappa(kappa, walls, None, scale, spacing)
    b = operators.rhs_kappa(kappa, None, walls, values, scale, spacing)
    # A u - b = 0 row by row: Dirichlet value and Neumann flux enter with the signs that make the discrete problem
    # consistent (a wrong sign of either leaves a defect of the size of the wall coefficient times u)
    bound = 64 * EPS * (abs(A) @ np.abs(u.ravel()))
    defect = np.abs(A @ u.ravel() - b.ravel())
    assert np.all(defect <= bound), (defect / bound).max()


def manufactured(n):
    """u = sin(2 x + 0.3) cos(1.5 y + 0.2) exp(0.8 z), kappa = 1 + 0.5 sin(x + 2 y + 0.5 z) on n^3 cells of the unit box:
    Dirichlet data on the x and y walls (at the mirrored ghost-cell centres), fluxes through the z walls, f = -div(kappa grad u)
    at the cell centres.  Returns the max-norm error of the discrete solution."""
    h = 1.0 / n
    c = (np.arange(-1, n + 1) + 0.5) * h                   # centres, ghost cells included
    Z, Y, X = c[:, None, None], c[None, :, None], c[None, None, :]

    def u_of(z, y, x):
        return np.sin(2.0 * x + 0.3) * np.cos(1.5 * y + 0.2) * np.exp(0.8 * z)

    def kappa_of(z, y, x):
        return 1.0 + 0.5 * np.sin(x + 2.0 * y + 0.5 * z)
    kappa = kappa_of(Z, Y, X)
    z, y, x = Z[1:-1], Y[:, 1:-1], X[:, :, 1:-1]
    u = u_of(z, y, x)
    ux = 2.0 * np.cos(2.0 * x + 0.3) * np.cos(1.5 * y + 0.2) * np.exp(0.8 * z)
    uy = -1.5 * np.sin(2.0 * x + 0.3) * np.sin(1.5 * y + 0.2) * np.exp(0.8 * z)
    uz = 0.8 * u
    lap = (-4.0 - 2.25 + 0.64) * u
    dk = 0.5 * np.cos(x + 2.0 * y + 0.5 * z)              # d kappa / dx; y: twice, z: half of it
    f = -(dk * ux + 2.0 * dk * uy + 0.5 * dk * uz + kappa_of(z, y, x) * lap)
    walls = (N, N, D, D, D, D)
    yx = (y[0], x[0])                                      # (n, 1), (1, n): the faces of a z wall
    zx = (z[:, 0], x[0])
    zy = (z[:, 0], y[0].reshape(1, n))
    values = [
        -kappa_of(0.0, *yx) * 0.8 * u_of(0.0, *yx) * h,    # outward flux through -z (times the cell width: no spacing)
        kappa_of(1.0, *yx) * 0.8 * u_of(1.0, *yx) * h,
        u_of(zx[0], -0.5 * h, zx[1]), u_of(zx[0], 1.0 + 0.5 * h, zx[1]),
        u_of(zy[0], zy[1], -0.5 * h), u_of(zy[0], zy[1], 1.0 + 0.5 * h)]
    scale = (1.0 / h ** 2,) * 3
    A = operators.stencil7_kappa(kappa, walls, None, scale)
    b = operators.rhs_kappa(kappa, f, walls, values, scale)
    uh = spla.spsolve(A.tocsc(), b.ravel())
    return float(np.abs(uh - u.ravel()).max())


def test_second_order_on_a_manufactured_problem():
    errors = [manufactured(n) for n in (8, 16, 32)]
    ratios = [errors[0] / errors[1], errors[1] / errors[2]]
    print("max-norm errors at 8^3, 16^3, 32^3: %.3e %.3e %.3e; ratios %.3f %.3f" % (tuple(errors) + tuple(ratios)))
    assert ratios[1] > 3.0, (errors, ratios)               # (first order: 2, second order: 4)


@pytest.mark.parametrize("grid", ["scale", "spacing"])
def test_ghost_cells_that_play_no_part_are_not_read(grid):
    shape = (4, 5, 6)
    walls = (N, D, D, D, P, P)                             # -z Neumann, +z / -y with values, +y Dirichlet without, x periodic
    kappa, values = rc.random_case(shape, walls, ("field", "scalar", "field", "none", "none", "none"))
    how = dict(scale=(0.3, 1.7, 2.9)) if grid == "scale" else dict(spacing=tuple(rc.widths(n, 1.4, "mirror") for n in shape))
    f = np.random.default_rng(1).standard_normal(shape)
    b = operators.rhs_kappa(kappa, f, walls, values, **how)
    poisoned = rc.poison_unread_ghosts(kappa, walls, values)
    assert np.isnan(poisoned[0]).all() and np.isnan(poisoned[:, -1]).all() and np.isnan(poisoned[:, :, 0]).all()
    assert np.isfinite(poisoned[-1, 1:-1, 1:-1]).all() and np.isfinite(poisoned[1:-1, 0, 1:-1]).all()
    with np.errstate(all="raise"):
        again = operators.rhs_kappa(poisoned, f, walls, values, **how)
    assert np.isfinite(again).all() and np.array_equal(again, b)
    # no values at all: the volume term alone, whatever the ghost layer holds
    assert np.array_equal(operators.rhs_kappa(rc.poison_unread_ghosts(kappa, walls, None), f, walls, None, **how),
                          f * operators.cell_volumes(how["spacing"]) + 0.0 if grid == "spacing" else f + 0.0)


def test_volume_term_and_signed_zero():
    shape = (2, 3, 4)
    kappa = two_decades(shape)
    spacing = tuple(rc.widths(n, 1.1, "mirror") for n in shape)
    assert np.array_equal(operators.rhs_kappa(kappa, 2.5, spacing=spacing), 2.5 * operators.cell_volumes(spacing))
    assert np.array_equal(operators.rhs_kappa(kappa, 2.5), np.full(shape, 2.5))
    zero = operators.rhs_kappa(kappa, np.full(shape, -0.0))
    assert not np.signbit(zero).any()                      # (-0.0 + +0.0 = +0.0: what the kernel's sum gives as well)
    assert not np.signbit(operators.rhs_kappa(kappa)).any() and not operators.rhs_kappa(kappa).any()


def test_the_new_entries_are_declared_and_bound_and_the_options_keep_their_layout():
    text = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    for name, n_args in (("omg_kappa_rhs", 14), ("omg_kappa_rhs_spaced", 17), ("omg_level_spmv_dev", 4)):
        assert ("int %s(" % name) in text
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args
    for const in ("OMG_VALUE_NONE   0", "OMG_VALUE_SCALAR 1", "OMG_VALUE_FIELD  2"):
        assert "#define " + const in text
    assert (_hip.VALUE_NONE, _hip.VALUE_SCALAR, _hip.VALUE_FIELD) == (0, 1, 2)
    assert [name for name, _ in _hip.HierarchyOptions._fields_] == ["smoother", "omega", "dtype", "nullspace"]
    import ctypes
    assert [t for _, t in _hip.HierarchyOptions._fields_] == [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    assert hasattr(openmg_amd.Solver, "rhs") and hasattr(openmg_amd.Solver, "matvec") and hasattr(_hip.Hierarchy, "spmv_dev")
