"""operators.stencil7_faces / rhs_faces / flux_faces / face_coefficients_kappa, the NumPy definitions the face-coefficient
kernels (csrc/kappa.hip) are pinned to: the tie to stencil7_kappa bit for bit, symmetry, row sums, the flux identity, a
unit vector's column, what is refused and what is tolerated; _hip.FaceArgs and its entries and Solver.from_faces refuse bad
arguments before they touch a device; the five C entries are declared, bound and exported.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import faces_cases as fc
from faces_cases import D, N, P, same_bits, same_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps

TIE_WALLS = {"dirichlet": (D,) * 6, "mixed": (N, D, D, N, D, D), "periodic zx": (P, P, D, N, P, P), "periodic": (P,) * 6}


@pytest.mark.parametrize("shape, wname", [(shape, wname) for shape in [(4, 4, 4), (5, 7, 9), (2, 3, 70), (3, 3, 70), (16, 16, 16)]
                                          for wname in sorted(TIE_WALLS) if fc.takes(shape, TIE_WALLS[wname])])
def test_the_tie_to_stencil7_kappa_bit_for_bit(shape, wname):
    """stencil7_faces(face_coefficients_kappa(k, w, scale, spacing), w, sigma) is stencil7_kappa(k, w, sigma, scale, spacing) in
    indptr, indices and data — with scale factors and with random widths (the spaced sigma as sigma * cell_volumes)."""
    walls = TIE_WALLS[wname]
    kappa = fc.kappa_of(shape)
    for how in (dict(scale=fc.SCALE), dict(spacing=fc.widths_of(shape))):
        C = operators.face_coefficients_kappa(kappa, walls, **how)
        assert tuple(a.shape for a in C) == operators.face_shapes(shape)
        for skind in fc.SIGMAS:
            sigma = fc.sigma_of(skind, shape)
            carried = sigma if sigma is None or "scale" in how else sigma * operators.cell_volumes(how["spacing"])
            A = operators.stencil7_faces(C, walls, carried)
            B = operators.stencil7_kappa(kappa, walls, sigma, **how)
            assert A.indptr.dtype == np.int32 and A.indices.dtype == np.int32 and A.has_sorted_indices
            assert same_csr(A, B), (sorted(how), skind)
        # +0.0 on the faces of Neumann walls, the seam's bits in both C[0] and C[e]
        for axis in range(3):
            first, last = np.moveaxis(C[axis], axis, 0)[0], np.moveaxis(C[axis], axis, 0)[-1]
            if walls[2 * axis] == N:
                assert same_bits(first, np.zeros(first.shape))
            if walls[2 * axis + 1] == N:
                assert same_bits(last, np.zeros(last.shape))
            if walls[2 * axis] == P:
                assert same_bits(first, last)


@pytest.mark.parametrize("shape, wname, skind", fc.assembly_cases())
def test_symmetric_bit_for_bit_with_the_faces_as_entries(shape, wname, skind):
    walls = fc.WALLS[wname]
    A = fc.definition(shape, wname, skind)
    assert (A != A.T).nnz == 0
    assert np.isfinite(A.data).all()                       # (the NaN on every face that is not read never arrives)
    C = fc.faces_of(shape, walls)
    n = A.shape[0]
    idx = np.arange(n).reshape(shape)
    for axis in range(3):
        e = shape[axis]
        lo, hi = np.moveaxis(idx, axis, 0)[:-1].ravel(), np.moveaxis(idx, axis, 0)[1:].ravel()
        inner = np.moveaxis(C[axis], axis, 0)[1:e].ravel()
        assert same_bits(np.asarray(A[lo, hi]).ravel(), -inner) and same_bits(np.asarray(A[hi, lo]).ravel(), -inner)
        if walls[2 * axis] == P:
            first, last = np.moveaxis(idx, axis, 0)[0].ravel(), np.moveaxis(idx, axis, 0)[-1].ravel()
            seam = np.moveaxis(C[axis], axis, 0)[0].ravel()
            assert same_bits(np.asarray(A[first, last]).ravel(), -seam) and same_bits(np.asarray(A[last, first]).ravel(), -seam)


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 9), (3, 3, 70)])
@pytest.mark.parametrize("walls", [(N,) * 6, (P,) * 6, (P, P, N, N, P, P)])
def test_zero_row_sums_with_neumann_or_periodic_walls_and_no_sigma(shape, walls):
    A = operators.stencil7_faces(fc.faces_of(shape, walls), walls)
    rows = np.asarray(A.sum(axis=1)).ravel()
    # the diagonal is the sum of the six couplings, each addition rounded once: a few ulp of the diagonal
    assert np.all(np.abs(rows) <= 8 * EPS * A.diagonal())
    # a Dirichlet wall adds its face to the diagonal only
    B = operators.stencil7_faces(fc.faces_of(shape, (D,) * 6), (D,) * 6)
    excess = np.asarray(B.sum(axis=1)).reshape(shape)
    assert (excess[0] > 0).all() and (excess[:, -1] > 0).all() and (excess[:, :, 0] > 0).all()


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 9), (3, 3, 70)])
@pytest.mark.parametrize("wname", sorted(fc.WALLS))
def test_the_balance_of_the_fluxes_is_the_operator_applied_minus_its_right_hand_side(shape, wname):
    walls = fc.WALLS[wname]
    u = fc.solution(shape)
    faces = fc.faces_of(shape, walls)
    worst = 0.0
    for vname, kinds in fc.VALUE_KINDS.items():
        values = fc.values_of(shape, walls, kinds)
        for skind in fc.SIGMAS:
            left, right, bound = fc.identity_sides(faces, u, walls, values, fc.sigma_of(skind, shape))
            ratio = np.abs(left - right) / np.where(bound > 0.0, bound, 1.0)
            worst = max(worst, float(ratio.max()) * 32)
            assert np.all(np.abs(left - right) <= bound), (vname, skind, float(ratio.max()))
    print("worst deviation: %.2f eps (|A||u| + |b|)" % worst)


@pytest.mark.parametrize("wname", sorted(fc.WALLS))
def test_a_unit_vector_gives_the_operators_column_bit_for_bit(wname):
    shape = (3, 4, 5)
    walls = fc.WALLS[wname]
    faces = fc.faces_of(shape, walls)
    A = operators.stencil7_faces(faces, walls).toarray()
    n = A.shape[0]
    for cell in range(n):
        u = np.zeros(n)
        u[cell] = 1.0
        F = operators.flux_faces(faces, u, walls)
        balance = operators.divergence_faces(*F).ravel()
        column = A[:, cell]
        off = np.arange(n) != cell
        # every off-diagonal entry is one face's flux, bit for bit; the diagonal is the sum of six in another order
        assert same_bits(balance[off] + 0.0, column[off] + 0.0), cell
        assert abs(balance[cell] - column[cell]) <= 8 * EPS * column[cell]


def test_rhs_and_flux_as_stated():
    shape = (3, 4, 5)
    walls = (N, D, D, N, D, D)
    faces = fc.faces_of(shape, walls)
    values = fc.values_of(shape, walls, ("field", "scalar", "scalar", "field", "field", "none"))
    f = np.random.default_rng(7).standard_normal(shape)
    b = operators.rhs_faces(faces, f, walls, values)
    expect = f.copy()
    terms = [np.zeros(shape) for _ in range(6)]
    terms[0][0] = values[0]                                # Neumann -z: the flux itself
    terms[1][-1] = faces[0][-1] * values[1]                # Dirichlet +z: C[e] g
    terms[2][:, 0] = faces[1][:, 0] * values[2]
    terms[3][:, -1] = values[3]
    terms[4][:, :, 0] = faces[2][:, :, 0] * values[4]
    expect = (((((expect + terms[0]) + terms[2]) + terms[4]) + terms[5]) + terms[3]) + terms[1]
    assert same_bits(b, expect)
    assert same_bits(operators.rhs_faces(faces, None, walls, None), np.zeros(shape))
    assert same_bits(operators.rhs_faces(faces, 0.5, walls, None), np.full(shape, 0.5))
    u = fc.solution(shape)
    Fz, Fy, Fx = operators.flux_faces(faces, u, walls, values)
    assert same_bits(Fz[0], values[0]) and same_bits(Fz[-1], faces[0][-1] * (u[-1] - values[1]))
    assert same_bits(Fy[:, 0], faces[1][:, 0] * (values[2] - u[:, 0])) and same_bits(Fy[:, -1], -values[3])
    assert same_bits(Fx[:, :, -1], faces[2][:, :, -1] * (u[:, :, -1] - 0.0))
    assert same_bits(Fx[:, :, 1:-1], faces[2][:, :, 1:-1] * (u[:, :, :-1] - u[:, :, 1:]))
    # a periodic axis: faces 0 and e hold the same bits, made of C[0]
    walls = (P,) * 6
    faces = fc.faces_of(shape, walls)
    for axis, F in enumerate(operators.flux_faces(faces, u, walls)):
        F, C, v = np.moveaxis(F, axis, 0), np.moveaxis(faces[axis], axis, 0), np.moveaxis(u, axis, 0)
        assert same_bits(F[0], F[-1]) and same_bits(F[0], C[0] * (v[-1] - v[0]))
    # flux_kappa's output can be fed back as coefficients unchanged: both seam entries hold the same bits
    k = fc.kappa_of(shape)
    G = operators.flux_kappa(k, u + 3.0 * np.arange(u.size).reshape(shape), walls)
    assert all(same_bits(np.moveaxis(g, a, 0)[0], np.moveaxis(g, a, 0)[-1]) for a, g in enumerate(G))


def test_what_is_refused_and_what_is_tolerated():
    shape = (4, 5, 6)
    walls = (N, D, D, D, P, P)
    ok = operators.stencil7_faces
    good = fc.faces_of(shape, walls, poison=False)
    # a coefficient that is 0, negative, NaN or inf on a face that is read: an in-grid face, a Dirichlet wall face, the seam
    for value in (0.0, -1.0, np.nan, np.inf):
        for array, face in ((0, (2, 3, 4)), (0, (4, 1, 1)), (1, (1, 0, 2)), (1, (1, 5, 2)), (1, (1, 2, 2)), (2, (1, 1, 0)), (2, (3, 4, 3))):
            bad = [a.copy() for a in good]
            bad[array][face] = value
            with pytest.raises(ValueError, match="finite and > 0"):
                ok(bad, walls)
    # NaN in a Neumann wall's faces and in C[e] of a periodic axis is accepted, and changes nothing
    poisoned = [a.copy() for a in good]
    poisoned[0][0] = np.nan
    poisoned[2][:, :, -1] = np.nan
    assert same_csr(ok(poisoned, walls, 0.5), ok(good, walls, 0.5))
    u = fc.solution(shape)
    assert all(same_bits(a, b) for a, b in zip(operators.flux_faces(poisoned, u, walls), operators.flux_faces(good, u, walls)))
    assert same_bits(operators.rhs_faces(poisoned, 1.0, walls, (2.0, 1.0, None, 0.5, None, None)),
                     operators.rhs_faces(good, 1.0, walls, (2.0, 1.0, None, 0.5, None, None)))
    # shapes, count, dtype
    for bad in (good[:2], good[0], [good[1], good[0], good[2]], [good[0], good[1], np.ones((4, 5, 6))], [a.astype(np.float32) for a in good],
                [good[0], good[1], good[2].astype(np.float32)], [np.ones((1, 5, 6)), np.ones((0, 6, 6)), np.ones((0, 5, 7))]):
        for fn in (lambda c: ok(c, walls), lambda c: operators.rhs_faces(c, None, walls), lambda c: operators.flux_faces(c, u, walls)):
            with pytest.raises(ValueError):
                fn(bad)
    for w in ((D,) * 5, (D,) * 5 + (P,), ("wall",) * 6, (0,) * 6):
        with pytest.raises(ValueError):
            ok(good, w)
    with pytest.raises(ValueError, match="extent >= 3"):
        ok(fc.faces_of((2, 3, 4), (D,) * 6), (P, P, D, D, D, D))
    for sigma in (-0.5, np.nan, np.inf, np.full(shape, -1.0), np.ones((4, 5, 5)), "x"):
        with pytest.raises(ValueError):
            ok(good, walls, sigma)
    # a value on a periodic wall; an f, a u, a value field of another shape
    for call in (lambda: operators.rhs_faces(good, None, walls, (None,) * 4 + (1.0, None)),
                 lambda: operators.flux_faces(good, u, walls, (None,) * 5 + (np.ones((4, 5)),)),
                 lambda: operators.rhs_faces(good, np.ones((4, 5, 5)), walls),
                 lambda: operators.rhs_faces(good, None, walls, (np.ones((5, 5)),) + (None,) * 5),
                 lambda: operators.rhs_faces(good, None, walls, (1.0,) * 5),
                 lambda: operators.flux_faces(good, u[1:], walls),
                 lambda: operators.flux_faces(good, None, walls)):
        with pytest.raises(ValueError):
            call()


class FakeDevice:
    """An object with the device-array interface and an address that is never followed."""

    def __init__(self, shape, address=4096, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (address, False), "version": 2, "strides": None}


def test_every_refusal_of_the_device_entries_is_a_value_error_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (3, 4, 5)
    shapes = operators.face_shapes(shape)
    good, u = [np.ones(s) for s in shapes], np.ones(shape)
    d_good = [FakeDevice(s, (1 + a) << 20) for a, s in enumerate(shapes)]
    d_u = FakeDevice(shape, 5 << 20)
    entries = (lambda c, **k: _hip.FaceArgs(c, **k), lambda c, **k: _hip.faces_assemble(c, **k), lambda c, **k: _hip.faces_rhs(c, **k),
               lambda c, **k: _hip.faces_flux(c, u if not _hip_is_device(c) else d_u, **k),
               lambda c, **k: _hip.Hierarchy.from_faces(c, 1, **k))
    # wrong face shapes, another count, float32, arrays on both sides — host and device
    for bad in (good[:2], good[0], [good[1], good[0], good[2]], [good[0], good[1], np.ones(shape)], [a.astype(np.float32) for a in good],
                [good[0], good[1], d_good[2]], [d_good[0], good[1], good[2]], [d_good[0], d_good[1], FakeDevice(shape, 3 << 20)],
                [d_good[0], d_good[1], FakeDevice(shapes[2], 3 << 20, "<f4")]):
        for entry in entries:
            with pytest.raises(ValueError):
                entry(bad)
    for entry in entries:
        for w in ((D,) * 5, (P, D, D, D, D, D), ("wall",) * 6):
            with pytest.raises(ValueError):
                entry(good, walls=w)
    with pytest.raises(ValueError):
        _hip.FaceArgs(good, sigma=-1.0)
    with pytest.raises(ValueError):
        _hip.FaceArgs(good, sigma=np.ones((3, 4, 4)))
    a = _hip.FaceArgs(good, (N, D, D, N, P, P), 0.5)
    assert a.grid == shape and a.shape == (60, 60) and a.walls == (1, 0, 0, 1, 2, 2) and a.periodic == (False, False, True)
    assert a.nnz == 7 * 60 - 2 * (20 + 15) and a.counts == [80, 75, 72] and not a.faces_on_device
    assert _hip.FaceArgs(a) is not a and _hip.FaceArgs(a).call is a.call
    assert _hip.FaceArgs(d_good).faces_on_device
    # a value on a periodic wall; values and f on the other side; alpha without out; outputs of the wrong kind; overlaps
    walls = (D, D, D, D, P, P)
    for call in (lambda: _hip.faces_rhs(good, None, walls, (None,) * 4 + (1.0, None)),
                 lambda: _hip.faces_flux(good, u, walls, (None,) * 5 + (2.0,)),
                 lambda: _hip.faces_rhs(good, d_u),
                 lambda: _hip.faces_rhs(d_good, u),
                 lambda: _hip.faces_rhs(d_good, None, None, (np.ones((4, 5)),) + (None,) * 5),
                 lambda: _hip.faces_rhs(good, None, None, (FakeDevice((4, 5)),) + (None,) * 5),
                 lambda: _hip.faces_rhs(good, np.ones((3, 4, 4))),
                 lambda: _hip.faces_rhs(good, out=np.zeros(59)),
                 lambda: _hip.faces_rhs(good, out=d_u),
                 lambda: _hip.faces_rhs(d_good, out=np.zeros(60)),
                 lambda: _hip.faces_flux(good, d_u),
                 lambda: _hip.faces_flux(d_good, u),
                 lambda: _hip.faces_flux(good, u[1:]),
                 lambda: _hip.faces_flux(good, u, alpha=-1.0),
                 lambda: _hip.faces_flux(good, u, out=[np.zeros(s) for s in shapes], alpha=np.inf),
                 lambda: _hip.faces_flux(good, u, out=[np.zeros(s) for s in shapes], alpha="a"),
                 lambda: _hip.faces_flux(good, u, out=[np.zeros(s) for s in shapes][:2]),
                 lambda: _hip.faces_flux(good, u, out=[np.zeros(s, dtype=np.float32) for s in shapes]),
                 lambda: _hip.faces_flux(good, u, out=[FakeDevice(s, (9 + a) << 20) for a, s in enumerate(shapes)]),
                 lambda: _hip.faces_flux(d_good, d_u, out=[np.zeros(s) for s in shapes])):
        with pytest.raises(ValueError):
            call()
    pool = np.ones(1000)
    n, (cz, cy, cx) = u.size, [int(np.prod(s)) for s in shapes]
    u_in = pool[100:100 + n]
    c_in = [pool[300:300 + cz].reshape(shapes[0]), pool[400:400 + cy].reshape(shapes[1]), pool[500:500 + cx].reshape(shapes[2])]
    fresh = [np.zeros(s) for s in shapes]
    for out in ([pool[21:21 + cz], fresh[1], fresh[2]],                    # its last entry is u's first
                [fresh[0], fresh[1], pool[300 + cz - 1:300 + cz - 1 + cx]],  # its first entry is Cz's last
                [fresh[0], c_in[1], fresh[2]],                              # a coefficient array itself: nothing is made in place
                [fresh[0], fresh[1], fresh[1].reshape(-1)[:cx]]):           # two outputs in one buffer
        with pytest.raises(ValueError, match="overlap"):
            _hip.faces_flux(c_in, u_in, out=out)
    with pytest.raises(ValueError, match="overlap"):
        _hip.faces_flux(d_good, d_u, out=[d_good[0], FakeDevice(shapes[1], 9 << 20), FakeDevice(shapes[2], 10 << 20)], alpha=-1.0)


def _hip_is_device(c):
    try:
        return any(hasattr(a, "__cuda_array_interface__") and not isinstance(a, np.ndarray) for a in c)
    except TypeError:
        return False


def test_solver_from_faces_refuses_bad_arguments_before_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (8, 8, 8)
    C = fc.faces_of(shape, (D,) * 6)
    p = {"gridLevels": 2, "cycles": 2, "smoother": "colour"}
    S = openmg_amd.Solver.from_faces
    bad = [lambda: S(C[:2], p), lambda: S(C[0], p), lambda: S([a.astype(np.float32) for a in C], p), lambda: S([C[0], C[1], C[1]], p),
           lambda: S(C, dict(p, problemShape=(8, 8, 4))), lambda: S(C, dict(p, problemShape=(512,))), lambda: S(C, p, walls=(D,) * 5),
           lambda: S(C, p, walls=("wall",) * 6), lambda: S(C, p, walls=(P,) + (D,) * 5), lambda: S(C, p, sigma=-1.0),
           lambda: S(C, p, sigma=np.nan), lambda: S(C, p, sigma=np.ones((8, 8, 4))), lambda: S(C, dict(p, smoother="nope")),
           lambda: S(C, dict(p, accel="gmres")), lambda: S(C, dict(p, rtol=-1.0)), lambda: S(C, p, projection=65)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        S(C, p, None, None, 4)                             # (projection is keyword-only, as on every constructor)


def test_each_kind_of_solver_refuses_the_other_kinds_methods(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (3, 4, 5)
    kappa, u = np.ones((5, 6, 7)), np.ones(60)
    faces = [np.ones(s) for s in operators.face_shapes(shape)]

    def solver(**fields):                                  # (no device here: the object alone, as __init__ leaves it)
        s = openmg_amd.Solver.__new__(openmg_amd.Solver)
        s._hierarchy = object()
        for name, value in fields.items():
            setattr(s, name, value)
        return s
    plain = solver()
    for call in (lambda: plain.rhs(faces), lambda: plain.fluxes(faces, u), lambda: plain.divergence(faces),
                 lambda: plain.update_kappa(kappa), lambda: plain.update_faces(faces)):
        with pytest.raises(ValueError, match="not made by"):
            call()
    of_kappa = solver(_kappa=(shape, None, (1.0, 1.0, 1.0), None))
    with pytest.raises(ValueError, match="from_faces"):
        of_kappa.update_faces(faces)
    of_faces = solver(_faces=(shape, None))
    with pytest.raises(ValueError, match="from_kappa"):
        of_faces.update_kappa(kappa)
    # on a from_faces solver rhs and fluxes want the three arrays of ITS grid
    other = [np.ones(s) for s in operators.face_shapes((3, 4, 6))]
    for call in (lambda: of_faces.rhs(kappa), lambda: of_faces.fluxes(kappa, u), lambda: of_faces.rhs(other), lambda: of_faces.fluxes(other, u),
                 lambda: of_faces.update_faces(other), lambda: of_faces.update_faces(faces[:2]), lambda: of_faces.divergence(other),
                 lambda: of_faces.fluxes(faces, u, alpha=-1.0), lambda: of_faces.fluxes(faces, u[:-1]),
                 lambda: of_faces.rhs(faces, values=(1.0,) * 5)):
        with pytest.raises(ValueError):
            call()
    for s in (plain, of_kappa, of_faces):
        s._hierarchy = None                                # (__del__ closes nothing)


def test_the_five_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name, n_args in (("omg_faces_assemble", 13), ("omg_hierarchy_create_from_faces", 12), ("omg_hierarchy_update_faces", 10),
                         ("omg_faces_rhs", 15), ("omg_faces_flux", 17)):
        assert ("int %s(" % name) in text
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args
        assert hasattr(handle, name)
    for name in ("from_faces", "update_faces"):
        assert hasattr(openmg_amd.Solver, name) and hasattr(_hip.Hierarchy, name)
    for name in ("stencil7_faces", "rhs_faces", "flux_faces", "face_coefficients_kappa", "faces_arguments"):
        assert hasattr(operators, name)
