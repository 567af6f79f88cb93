"""operators.flux_kappa and operators.divergence_faces, the NumPy definitions of the face fluxes of a solution and of their
cell balance (the device kernels of csrc/kappa.hip are pinned to them bit for bit: tests/test_gpu_kappa_flux.py): the
discrete identity with the operator and its right-hand side, the operator's own columns out of unit vectors bit for bit,
exact fluxes of a linear field, the seam faces, the ghost cells that must not be read, the Neumann sign at both walls, every
refusal; the new C entries are declared and bound.  CPU only."""
import os

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import kappa_flux_cases as fc
import kappa_rhs_cases as rc
from kappa_flux_cases import EPS, same_bits
from kappa_rhs_cases import D, N, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wname", list(fc.WALLSETS))
@pytest.mark.parametrize("shape", fc.SHAPES[:5])
def test_the_balance_of_the_fluxes_is_the_operator_applied_minus_its_right_hand_side(shape, wname):
    walls = fc.WALLSETS[wname]
    if not fc.takes(shape, walls):
        with pytest.raises(ValueError):
            operators.flux_kappa(np.ones(tuple(n + 2 for n in shape)), np.ones(shape), walls)
        return
    u = fc.solution(shape)
    sigmas = [None, 0.37, np.random.default_rng(5).uniform(0.0, 2.0, size=shape)]
    worst = 0.0
    for vname, kinds in fc.VALUE_KINDS.items():
        kappa, values = fc.case(shape, walls, kinds)
        for how in fc.grids_of(shape):
            for sigma in sigmas:
                left, right, bound = fc.identity_sides(kappa, u, walls, values, sigma, how)
                ratio = np.abs(left - right) / np.where(bound > 0.0, bound, 1.0)
                worst = max(worst, float(ratio.max()) * 32)
                assert np.all(np.abs(left - right) <= bound), (vname, sorted(how), type(sigma).__name__, float(ratio.max()))
    print("worst deviation: %.2f eps (|A||u| + |b|)" % worst)


@pytest.mark.parametrize("wname", list(fc.WALLSETS))
@pytest.mark.parametrize("grid", [0, 1, 2])
def test_a_unit_vector_gives_the_operators_column_bit_for_bit(wname, grid):
    shape, walls = (3, 4, 5), fc.WALLSETS[wname]
    n = int(np.prod(shape))
    kappa, _ = fc.case(shape, walls, None)
    how = fc.grids_of(shape)[grid]
    A = operators.stencil7_kappa(kappa, walls, None, **how).toarray()
    for m in range(n):
        u = np.zeros(n)
        u[m] = 1.0
        column = operators.divergence_faces(*operators.flux_kappa(kappa, u, walls, None, **how)).ravel()
        others = np.arange(n) != m
        # (an entry that is not in the pattern: a zero of either sign)
        assert np.array_equal(column[others], A[others, m]), m
        stored = others & (A[:, m] != 0.0)
        assert same_bits(column[stored], A[stored, m]), m
        assert abs(column[m] - A[m, m]) <= 4 * EPS * A[m, m], m


LINEAR_WALLS = [(D, N, N, D, D, N), (N, D, D, N, N, D), (D,) * 6, (N,) * 6]


@pytest.mark.parametrize("walls", LINEAR_WALLS)
@pytest.mark.parametrize("grid", ["uniform", "stretched mirror", "stretched face", "stretched mixed"])
def test_a_linear_field_has_the_exact_flux_on_every_face(walls, grid):
    shape = (6, 7, 9)
    if grid == "uniform":
        spacing = None
    else:
        ghosts = {"stretched mirror": ("mirror",) * 3, "stretched face": (0.0,) * 3, "stretched mixed": (0.0, "mirror", 0.02)}[grid]
        spacing = tuple(rc.widths(n, 1.6, g) for n, g in zip(shape, ghosts))
    kappa, scale, values, u = rc.linear_problem(shape, walls, spacing)
    F = operators.flux_kappa(kappa, u, walls, values, scale, spacing)
    slope = (rc.GAMMA, rc.BETA, rc.ALPHA)                  # du/dz, du/dy, du/dx
    for axis in range(3):
        if spacing is None:
            # scale = 1 / h^2 and the difference of u over one cell is slope h: -kappa slope / h
            want = np.full(F[axis].shape, -1.7 * slope[axis] * shape[axis])
        else:
            H = [np.asarray(h)[1:-1] for h in spacing]
            a, b = [d for d in range(3) if d != axis]
            area = H[a][:, None] * H[b][None, :]
            want = np.broadcast_to(np.expand_dims(-1.7 * slope[axis] * area, axis), F[axis].shape)
        assert F[axis].shape == operators.face_shapes(shape)[axis]
        assert np.all(np.abs(F[axis] - want) <= 1e-12 * np.abs(want)), (axis, float(np.abs(F[axis] / want - 1.0).max()))


@pytest.mark.parametrize("wname", ["periodic x", "periodic y", "periodic z", "periodic xyz"])
def test_the_seam_faces_hold_the_same_bits_and_the_inner_face_expression(wname):
    shape, walls = (4, 5, 6), fc.WALLSETS[wname]
    kappa, values = fc.case(shape, walls, fc.VALUE_KINDS["mixture"])
    u = fc.solution(shape)
    for how in fc.grids_of(shape):
        F = operators.flux_kappa(kappa, u, walls, values, **how)
        A = operators.stencil7_kappa(kappa, walls, None, **how)
        idx = np.arange(u.size).reshape(shape)
        for axis in range(3):
            if walls[2 * axis] != P:
                continue
            first, last = np.take(F[axis], 0, axis), np.take(F[axis], shape[axis], axis)
            assert same_bits(first, last)
            lo, hi = np.take(idx, shape[axis] - 1, axis), np.take(idx, 0, axis)
            c = -np.asarray(A[lo.ravel(), hi.ravel()]).reshape(lo.shape)
            assert same_bits(first, c * (np.take(u, shape[axis] - 1, axis) - np.take(u, 0, axis)))


@pytest.mark.parametrize("grid", [0, 1, 2])
def test_ghost_cells_behind_neumann_and_periodic_walls_are_not_read(grid):
    shape = (4, 5, 6)
    u = fc.solution(shape)
    for walls in ((N, D, D, N, P, P), (N,) * 6, (P,) * 6, (P, P, N, D, D, N)):
        for kinds in fc.VALUE_KINDS.values():
            kappa, values = fc.case(shape, walls, kinds)
            how = fc.grids_of(shape)[grid]
            poisoned = fc.poison(kappa, walls)
            for w, kind in enumerate(walls):
                layer = np.take(poisoned, -1 if w % 2 else 0, w // 2)
                inner = layer[1:-1, 1:-1]
                assert np.isfinite(inner).all() if kind == D else np.isnan(layer).all()
            with np.errstate(all="raise"):
                again = operators.flux_kappa(poisoned, u, walls, values, **how)
            for a, b in zip(again, operators.flux_kappa(kappa, u, walls, values, **how)):
                assert np.isfinite(a).all() and same_bits(a, b)


def test_the_neumann_value_enters_with_its_sign_at_both_walls():
    shape = (3, 4, 5)
    kappa, _ = fc.case(shape, (N,) * 6, None)
    u = fc.solution(shape)
    q = [0.5, 0.75, -1.25, 2.0, 3.0, -0.125]               # outward kappa du/dn per wall
    spacing = tuple(rc.widths(n, 1.2, "mirror") for n in shape)
    H = [h[1:-1] for h in spacing]
    for how, factor in ((dict(scale=fc.SCALE), lambda axis: fc.SCALE[axis]),
                        (dict(spacing=spacing), lambda axis: np.multiply.outer(*[H[d] for d in range(3) if d != axis]))):
        F = operators.flux_kappa(kappa, u, (N,) * 6, q, **how)
        for axis in range(3):
            t_lo, t_hi = q[2 * axis] * factor(axis), q[2 * axis + 1] * factor(axis)
            assert np.array_equal(np.take(F[axis], 0, axis), np.broadcast_to(t_lo, np.take(F[axis], 0, axis).shape))
            assert np.array_equal(np.take(F[axis], shape[axis], axis), np.broadcast_to(-t_hi, np.take(F[axis], 0, axis).shape))
        # ... which is the right-hand side's term moved to the other side: the balance of a constant u is -b
        flat = operators.flux_kappa(kappa, np.full(shape, 2.5), (N,) * 6, q, **how)
        assert np.allclose(operators.divergence_faces(*flat), -operators.rhs_kappa(kappa, None, (N,) * 6, q, **how), rtol=1e-13, atol=0.0)
    # no value: +0.0, and a wall face never depends on u
    F = operators.flux_kappa(kappa, u, (N,) * 6)
    for axis in range(3):
        for m in (0, shape[axis]):
            face = np.take(F[axis], m, axis)
            assert not face.any() and not np.signbit(face).any()


def test_divergence_faces_is_the_balance_in_the_stated_order():
    shape = (3, 4, 5)
    rng = np.random.default_rng(11)
    Fz, Fy, Fx = (rng.standard_normal(s) for s in operators.face_shapes(shape))
    d = operators.divergence_faces(Fz, Fy, Fx)
    assert d.shape == shape and d.dtype == np.float64
    for k, j, i in ((0, 0, 0), (2, 3, 4), (1, 2, 3)):
        assert d[k, j, i] == ((Fz[k + 1, j, i] - Fz[k, j, i]) + (Fy[k, j + 1, i] - Fy[k, j, i])) + (Fx[k, j, i + 1] - Fx[k, j, i])
    assert operators.face_shapes(shape) == ((4, 4, 5), (3, 5, 5), (3, 4, 6))
    for bad in ((Fz, Fy, Fx[:, :, :-1]), (Fz[:-1], Fy, Fx), (Fy, Fz, Fx), (Fz.ravel(), Fy.ravel(), Fx.ravel()), (Fz[0], Fy[0], Fx[0]),
                (np.ones((1, 2, 2)), np.ones((0, 3, 2)), np.ones((0, 2, 3)))):
        with pytest.raises(ValueError):
            operators.divergence_faces(*bad)
        with pytest.raises(ValueError):
            _hip.face_divergence(bad)


def bad_calls(shape):
    """(u, walls, values, scale, spacing) that every layer must refuse with ValueError."""
    nz, ny, nx = shape
    ok_spacing = tuple(rc.widths(n, 1.5, "mirror") for n in shape)
    periodic_x = (D, D, N, N, P, P)
    u = np.ones(shape)
    return [
        (np.ones((nz, ny)), None, None, (1.0,) * 3, None),                           # u of another shape
        (np.ones(nz * ny * nx + 1), None, None, (1.0,) * 3, None),
        (np.ones((nx, ny, nz)), None, None, (1.0,) * 3, None),
        (None, None, None, (1.0,) * 3, None),
        (1.0, None, None, (1.0,) * 3, None),
        (u, None, (1.0,) * 5, (1.0,) * 3, None),                                     # wrong count
        (u, None, 1.0, (1.0,) * 3, None),
        (u, None, (np.ones((ny, nx + 1)),) + (None,) * 5, (1.0,) * 3, None),         # wrong shape on -z
        (u, None, (None,) * 5 + (np.ones(nz * ny),), (1.0,) * 3, None),              # 1-D on +x
        (u, None, ("g",) + (None,) * 5, (1.0,) * 3, None),
        (u, periodic_x, (None,) * 4 + (1.0, None), (1.0,) * 3, None),                # a value on a periodic wall
        (u, (D,) * 5, None, (1.0,) * 3, None),                                       # what kappa_arguments refuses
        (u, (D, D, D, D, P, D), None, (1.0,) * 3, None),
        (u, None, None, (1.0, 0.0, 1.0), None),
        (u, None, None, (2.0, 1.0, 1.0), ok_spacing),                                # spacing and scale exclude each other
        (u, None, None, (1.0,) * 3, ok_spacing[:2]),                                 # what spacing_arguments refuses
        (u, None, None, (1.0,) * 3, (ok_spacing[0], ok_spacing[1], -ok_spacing[2])),
    ]


class FakeDevice:
    def __init__(self, shape, address=4096):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (address, False), "version": 2, "strides": None}


def test_every_refusal_is_a_value_error_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (3, 4, 5)
    kappa, u = np.ones(tuple(n + 2 for n in shape)), np.ones(shape)
    for v, walls, values, scale, spacing in bad_calls(shape):
        for fn in (operators.flux_kappa, _hip.kappa_flux):
            with pytest.raises(ValueError):
                fn(kappa, v, walls, values, scale, spacing)
    for fn in (operators.flux_kappa, _hip.kappa_flux):
        for bad in (kappa[0], kappa.astype(np.float32), np.ones((2, 5, 5))):
            with pytest.raises(ValueError):
                fn(bad, u)
    # u is accepted flat, (n,) or (n, 1), as solve returns it
    for flat in (u.ravel(), u.reshape(-1, 1)):
        assert all(same_bits(a, b) for a, b in zip(operators.flux_kappa(kappa, flat), operators.flux_kappa(kappa, u)))
    faces = lambda: [np.zeros(s) for s in operators.face_shapes(shape)]
    good = faces()
    # out: another count, another size, another dtype, not contiguous, read-only; alpha without out, alpha not finite or no number
    locked = faces()
    locked[1].flags.writeable = False
    for out in (good[:2], good[0], [good[0], good[1], np.zeros(shape)], [good[1], good[0], good[2]],
                [good[0].astype(np.float32), good[1], good[2]], [good[0], good[1], np.zeros((3, 4, 12))[:, :, ::2]], locked):
        with pytest.raises(ValueError):
            _hip.kappa_flux(kappa, u, out=out)
    for more in (dict(alpha=1.0), dict(out=good, alpha=np.inf), dict(out=good, alpha=np.nan), dict(out=good, alpha="a")):
        with pytest.raises(ValueError):
            _hip.kappa_flux(kappa, u, **more)
    # an out that overlaps u, kappa or another face array: views of one buffer
    pool = np.zeros(1000)
    n, (cz, cy, cx) = u.size, [int(np.prod(s)) for s in operators.face_shapes(shape)]
    u_in, k_in = pool[100:100 + n], pool[300:300 + kappa.size].reshape(kappa.shape)
    k_in[...] = 1.0
    for out in ([pool[21:21 + cz], good[1], good[2]],                      # its last entry is u's first
                [good[0], good[1], pool[100 + n - 1:100 + n - 1 + cx]],     # its first entry is u's last
                [good[0], pool[500:500 + cy], good[2]],                     # inside kappa
                [good[0], good[1][:], good[1].reshape(-1)[:cx].reshape(good[2].shape) if cx <= cy else good[2]]):
        with pytest.raises(ValueError, match="overlap"):
            _hip.kappa_flux(k_in, u_in, out=out)
    # arrays on both sides; outputs on the other side; device outputs of another size; device views into u and kappa
    d_kappa, d_u = FakeDevice(kappa.shape, 1 << 20), FakeDevice(shape, 2 << 20)
    d_faces = lambda base=3 << 20: [FakeDevice(s, base + (1 << 16) * a) for a, s in enumerate(operators.face_shapes(shape))]
    for call in (lambda: _hip.kappa_flux(kappa, d_u),
                 lambda: _hip.kappa_flux(d_kappa, u),
                 lambda: _hip.kappa_flux(d_kappa, d_u, values=(np.ones((4, 5)),) + (None,) * 5),
                 lambda: _hip.kappa_flux(kappa, u, out=d_faces()),
                 lambda: _hip.kappa_flux(d_kappa, d_u, out=good),
                 lambda: _hip.kappa_flux(d_kappa, d_u, out=d_faces()[:2] + [FakeDevice(shape, 5 << 20)]),
                 lambda: _hip.kappa_flux(d_kappa, FakeDevice(shape, 2 << 20), out=d_faces()[:2] + [FakeDevice((3, 4, 6), (2 << 20) + 8)]),
                 lambda: _hip.kappa_flux(d_kappa, d_u, out=[FakeDevice((4, 4, 5), (1 << 20) + 64)] + d_faces()[1:]),
                 lambda: _hip.kappa_flux(d_kappa, d_u, out=d_faces(), alpha=np.inf)):
        with pytest.raises(ValueError):
            call()
    # face_divergence: sides, sizes, overlap
    for call in (lambda: _hip.face_divergence([good[0], good[1], d_faces()[2]]),
                 lambda: _hip.face_divergence(good, out=np.zeros(59)),
                 lambda: _hip.face_divergence(good, out=FakeDevice((60,))),
                 lambda: _hip.face_divergence(d_faces(), out=np.zeros(60)),
                 lambda: _hip.face_divergence(d_faces(), out=FakeDevice((61,), 7 << 20)),
                 lambda: _hip.face_divergence(good, out=good[0].reshape(-1)[:60]),
                 lambda: _hip.face_divergence(d_faces(), out=FakeDevice((60,), (3 << 20) + 8 * 79)),
                 lambda: _hip.face_divergence(good[:2])):
        with pytest.raises(ValueError):
            call()


def test_solver_fluxes_and_divergence_want_a_from_kappa_solver_and_its_grid(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    s = openmg_amd.Solver.__new__(openmg_amd.Solver)      # (no device here: the object alone, as __init__ leaves a matrix solver)
    s._hierarchy = object()
    kappa, u = np.ones((5, 6, 7)), np.ones(60)
    faces = [np.zeros(sh) for sh in operators.face_shapes((3, 4, 5))]
    with pytest.raises(ValueError, match="from_kappa"):
        s.fluxes(kappa, u)
    with pytest.raises(ValueError, match="from_kappa"):
        s.divergence(faces)
    s._kappa = ((3, 4, 5), None, (1.0, 1.0, 1.0), None)
    with pytest.raises(ValueError, match="grid"):
        s.fluxes(np.ones((5, 6, 8)), u)
    with pytest.raises(ValueError, match="grid"):
        s.divergence([np.zeros(sh) for sh in operators.face_shapes((3, 4, 6))])
    for call in (lambda: s.divergence(faces[:2]), lambda: s.divergence(faces[0]), lambda: s.fluxes(kappa, u[:-1]),
                 lambda: s.fluxes(kappa, u, alpha=-1.0), lambda: s.fluxes(kappa, u, values=(1.0,) * 5)):
        with pytest.raises(ValueError):
            call()
    s._hierarchy = None                                    # (__del__ closes nothing)


def test_the_new_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    for name, n_args in (("omg_kappa_flux", 16), ("omg_kappa_flux_spaced", 19), ("omg_face_divergence", 7)):
        assert ("int %s(" % name) in text
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args
    for name in ("fluxes", "divergence"):
        assert hasattr(openmg_amd.Solver, name)
    for name in ("flux_kappa", "divergence_faces", "face_shapes"):
        assert hasattr(operators, name)
