"""operators.stencil7_kappa(..., spacing=...): the SciPy definition of the 7-point finite-volume operator of
-div(kappa grad u) + sigma u on a stretched tensor-product grid that the device assembly (csrc/kappa.hip, SPACED) is pinned
to.  Symmetric bit for bit, Neumann rows sum to zero, uniform power-of-two widths give the scaled uniform operator bit for
bit, second order on a tanh-clustered grid, every refusal before any device work.  CPU only."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import openmg
import openmg_amd
from openmg_amd import _hip, operators

import kappa_cases as kc
import stretched_cases as sc

EPS = np.finfo(float).eps


@pytest.mark.parametrize("zero", [False, True], ids=["ghosts", "zero-ghosts"])
@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 9), (2, 3, 70)])
def test_symmetric_bit_for_bit(shape, zero):
    A = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS["mixed"], kc.sigma_of("field", shape), spacing=sc.widths_of(shape, zero=zero))
    # (the two cells of a face form the same two products da b, db a, a commutative sum and the same area)
    assert (A != A.T).nnz == 0
    on_diagonal = A.indices == np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    assert np.isfinite(A.data).all() and (A.data[on_diagonal] > 0).all() and (A.data[~on_diagonal] < 0).all()
    assert A.indptr.dtype == np.int32 and A.indices.dtype == np.int32 and A.has_sorted_indices


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 9), (2, 3, 70)])
def test_all_neumann_rows_sum_to_zero(shape):
    A = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS["neumann"], None, spacing=sc.widths_of(shape))
    d = A.diagonal()
    rows = A @ np.ones(A.shape[0])
    # The bound, with u = EPS / 2.  The diagonal is the six couplings c >= 0 (a Neumann wall face: +0.0) added in a chain
    # of five rounded sums, so d = S (1 + t), |t| <= 5 u / (1 - 5 u), S their exact sum.  The row sum adds the seven
    # entries of the row in column order; every partial sum lies between -S and d, so each of its six rounded sums errs
    # by at most u max(S, d).  Together |row sum| <= 5 u S + 6 u max(S, d) + O(u^2) < 12 u d = 6 EPS d.
    assert np.all(np.abs(rows) <= 6 * EPS * d)
    assert (d > 0).all()


@pytest.mark.parametrize("wname", list(kc.WALLS))
@pytest.mark.parametrize("skind", kc.SIGMAS)
def test_uniform_power_of_two_widths_give_the_scaled_uniform_operator_bit_for_bit(wname, skind):
    shape, h = (5, 7, 9), (0.25, 0.5, 0.125)
    V = h[0] * h[1] * h[2]
    spacing = tuple(np.full(s + 2, w) for s, w in zip(shape, h))
    kappa, sigma = kc.kappa_of(shape), kc.sigma_of(skind, shape)
    A = operators.stencil7_kappa(kappa, kc.WALLS[wname], sigma, spacing=spacing)
    scaled = None if sigma is None else (sigma * V if np.ndim(sigma) else float(sigma) * V)
    B = operators.stencil7_kappa(kappa, kc.WALLS[wname], scaled, scale=tuple(V / w ** 2 for w in h))
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def test_cell_volumes():
    shape = (5, 7, 9)
    hz, hy, hx = sc.widths_of(shape, zero=True)
    vol = operators.cell_volumes((hz, hy, hx))
    assert vol.shape == shape and vol.dtype == np.float64
    assert np.array_equal(vol, (hz[1:-1, None, None] * hy[None, 1:-1, None]) * hx[None, None, 1:-1])
    assert np.array_equal(operators.cell_volumes([list(hz), list(hy), list(hx)]), vol)
    # sigma enters as sigma * vol: the difference of the diagonals is that product, rounded once more by the sum
    k = kc.kappa_of(shape)
    A0 = operators.stencil7_kappa(k, spacing=(hz, hy, hx))
    A1 = operators.stencil7_kappa(k, sigma=0.375, spacing=(hz, hy, hx))
    assert np.array_equal(A1.diagonal(), A0.diagonal() + 0.375 * vol.ravel())
    for bad in ((hz, hy), (hz, hy, -hx), 3.0):
        with pytest.raises(ValueError):
            operators.cell_volumes(bad)


# ---- order of accuracy --------------------------------------------------------------------------------------------------
def boundary_layer_error(n):
    """Max-norm error of the finite-volume solution of -div(kappa grad u) = f on the unit box, u = sin(pi z) sin(pi y) sin(pi x),
    kappa = 1 + 0.5 sin(2 z + y) cos(x), faces clustered by the tanh map with beta = 2 (z), 1 (y), 0.5 (x), Dirichlet walls
    on the faces themselves (ghost widths 0)."""
    faces = [sc.tanh_faces(n, beta) for beta in (2.0, 1.0, 0.5)]
    widths = [np.diff(f) for f in faces]
    spacing = tuple(sc.padded(w, "wall") for w in widths)
    # cell centres, the ghost centres half a boundary-cell width outside
    centres = [np.concatenate(([f[0] - 0.5 * w[0]], 0.5 * (f[1:] + f[:-1]), [f[-1] + 0.5 * w[-1]])) for f, w in zip(faces, widths)]
    Z, Y, X = np.meshgrid(*centres, indexing="ij")
    kappa = 1.0 + 0.5 * np.sin(2.0 * Z + Y) * np.cos(X)
    z, y, x = Z[1:-1, 1:-1, 1:-1], Y[1:-1, 1:-1, 1:-1], X[1:-1, 1:-1, 1:-1]
    pi = np.pi
    u = np.sin(pi * z) * np.sin(pi * y) * np.sin(pi * x)
    grad_u = (pi * np.cos(pi * z) * np.sin(pi * y) * np.sin(pi * x), pi * np.sin(pi * z) * np.cos(pi * y) * np.sin(pi * x),
              pi * np.sin(pi * z) * np.sin(pi * y) * np.cos(pi * x))
    grad_k = (np.cos(2.0 * z + y) * np.cos(x), 0.5 * np.cos(2.0 * z + y) * np.cos(x), -0.5 * np.sin(2.0 * z + y) * np.sin(x))
    # f = -div(kappa grad u) = -(grad kappa . grad u) - kappa laplace u,  laplace u = -3 pi^2 u
    f = 3.0 * pi ** 2 * kappa[1:-1, 1:-1, 1:-1] * u - sum(gk * gu for gk, gu in zip(grad_k, grad_u))
    A = operators.stencil7_kappa(kappa, spacing=spacing)
    got = spla.spsolve(A.tocsc(), (f * operators.cell_volumes(spacing)).ravel())
    return np.abs(got - u.ravel()).max(), widths[0].max() / widths[0].min()


def test_second_order_on_a_tanh_clustered_grid():
    errors, ratios = zip(*(boundary_layer_error(n) for n in (8, 16, 32)))
    rates = (errors[0] / errors[1], errors[1] / errors[2])
    print("max-norm errors %s, ratios %.2f %.2f, widest / narrowest z cell %.1f" % (" ".join("%.3e" % e for e in errors), rates[0], rates[1], ratios[2]))
    # a first-order scheme gives 2, a second-order one 4; a wrong area, distance or harmonic weight gives about 2 or no convergence
    assert rates[0] >= 3.5 and rates[1] >= 3.5
    assert ratios[2] > 10.0                                    # (the grid is stretched in earnest)


# ---- refusals -----------------------------------------------------------------------------------------------------------
class FakeDeviceArray:
    """Something with __cuda_array_interface__ that is not a NumPy array (never dereferenced: the refusal comes first)."""

    def __init__(self, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (4096, False), "version": 2, "strides": None}

    def __len__(self):
        return self.__cuda_array_interface__["shape"][0]


def bad_spacings(shape):
    hz, hy, hx = sc.widths_of(shape)

    def put(axis, index, value):
        sp = [hz.copy(), hy.copy(), hx.copy()]
        sp[axis][index] = value
        return tuple(sp)
    return [(hz, hy), (hz, hy, hx, hx), 1.0, (hz[:-1], hy, hx), (hz, np.append(hy, 1.0), hx), (hz, hy, hx[None]), (hz, hy, "abc"),
            put(0, 2, np.nan), put(1, 1, np.inf), put(2, 0, np.nan), put(0, -1, np.inf),            # not finite: cells and ghosts
            put(0, 1, 0.0), put(1, 3, -1.0), put(2, -2, 0.0),                                           # an interior width <= 0
            put(0, 0, -0.5), put(2, -1, -1e-300),                                                       # a ghost width < 0
            (FakeDeviceArray(shape[0] + 2), hy, hx), FakeDeviceArray(3)]


def test_spacing_arguments():
    shape = (4, 5, 6)
    hz, hy, hx = sc.widths_of(shape, zero=True)
    got = operators.spacing_arguments(shape, (list(hz), hy.astype(np.float32).astype(np.float64)[::1], hx))
    assert len(got) == 3 and all(g.dtype == np.float64 and g.flags.c_contiguous and g.ndim == 1 for g in got)
    assert np.array_equal(got[0], hz) and np.array_equal(got[2], hx) and got[0][-1] == 0.0 and got[2][0] == 0.0
    strided = np.repeat(hy, 2)[::2]
    assert np.array_equal(operators.spacing_arguments(shape, (hz, strided, hx))[1], hy)
    for bad in bad_spacings(shape):
        with pytest.raises(ValueError):
            operators.spacing_arguments(shape, bad)
    with pytest.raises(ValueError, match="host"):
        operators.spacing_arguments(shape, (FakeDeviceArray(6), hy, hx))
    with pytest.raises(ValueError, match="host"):
        operators.spacing_arguments(shape, FakeDeviceArray(3))


def test_refusals_before_any_device_work(monkeypatch):
    # (any device work would go through the library: none may be reached)
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (8, 8, 8)
    k = kc.kappa_of(shape)
    good = sc.widths_of(shape)
    p = {"gridLevels": 2, "cycles": 2, "smoother": "colour"}
    entries = [lambda sp, **kw: operators.stencil7_kappa(k, spacing=sp, **kw),
               lambda sp, **kw: _hip.KappaArgs(k, spacing=sp, **kw),
               lambda sp, **kw: _hip.kappa_assemble(k, spacing=sp, **kw),
               lambda sp, **kw: _hip.Hierarchy.from_kappa(k, 1, spacing=sp, **kw),
               lambda sp, **kw: openmg_amd.Solver.from_kappa(k, p, spacing=sp, **kw)]
    for entry in entries:
        for bad in bad_spacings(shape):
            with pytest.raises(ValueError):
                entry(bad)
        for scale in ((4.0, 1.0, 0.25), (1.0, 1.0, 2.0)):
            with pytest.raises(ValueError):
                entry(good, scale=scale)
    wrong_grid = sc.widths_of((8, 8, 4))
    with pytest.raises(ValueError):
        openmg_amd.Solver.from_kappa(k, p, spacing=wrong_grid)
    a = _hip.KappaArgs(k, kc.WALLS["mixed"], 0.5, spacing=good)
    assert a.grid == shape and a.scale == (1.0, 1.0, 1.0) and all(np.array_equal(x, y) for x, y in zip(a.spacing, good))
    assert _hip.KappaArgs(k).spacing is None
    assert _hip.KappaArgs(a).spacing is a.spacing                      # (taken as it is)


# ---- what does not change -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wname,skind,scale", [((5, 7, 9), "mixed", "field", (4.0, 1.0, 0.25)), ((4, 4, 4), "dirichlet", "none", (1.0, 1.0, 1.0)),
                                                     ((2, 3, 70), "neumann", "field", (4.0, 1.0, 0.25)), ((4, 4, 4), "mixed", "scalar", (1.0, 1.0, 1.0))])
def test_without_spacing_the_arrays_are_todays(shape, wname, skind, scale):
    want = kc.definition(shape, wname, skind, scale)
    got = operators.stencil7_kappa(kc.kappa_of(shape), kc.WALLS[wname], kc.sigma_of(skind, shape), scale, spacing=None)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)
    # ... and they are the closed form of today's definition, evaluated here for one interior row
    nz, ny, nx = shape
    if min(shape) >= 3:
        kap = kc.kappa_of(shape)
        c = kap[2, 2, 2]
        face = lambda b, s: ((2.0 * c) * b) / (c + b) * s                               # noqa: E731
        w = [face(kap[1, 2, 2], scale[0]), face(kap[2, 1, 2], scale[1]), face(kap[2, 2, 1], scale[2]),
             face(kap[2, 2, 3], scale[2]), face(kap[2, 3, 2], scale[1]), face(kap[3, 2, 2], scale[0])]
        d = ((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]
        sigma = kc.sigma_of(skind, shape)
        if sigma is not None:
            d = d + (sigma[1, 1, 1] if np.ndim(sigma) else sigma)
        r = (1 * ny + 1) * nx + 1
        assert got[r, r] == d and got[r, r + 1] == -w[3] and got[r, r - nx] == -w[1]


def test_the_alias_package_exports_the_helpers():
    assert openmg.operators.cell_volumes is operators.cell_volumes
    assert openmg.operators.spacing_arguments is operators.spacing_arguments
    from openmg.operators import cell_volumes, stencil7_kappa  # noqa: F401
    assert operators.kappa_arguments((6, 6, 6)) == ((4, 4, 4), (0,) * 6, (1.0, 1.0, 1.0))    # (signature and return value as before)
