"""Periodic axes in operators.stencil7_kappa, the SciPy definition the device assembly (csrc/kappa.hip) is
pinned to: an independent construction, structure for every set of periodic axes, invariance under a shift round the
seam, the spaced form, the order of the discretisation, and every refusal before any device work.  CPU only."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import periodic_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_matrix(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(A.data, B.data))


def sorted_csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


# ---- an independent construction ----------------------------------------------------------------------------------------
def circulant(n, s):
    """The periodic 1-D operator s * (2, -1, -1 round the ring), dense loops: nothing of the code under test."""
    C = np.zeros((n, n))
    for i in range(n):
        C[i, i] += 2.0 * s
        C[i, (i + 1) % n] -= s
        C[i, (i - 1) % n] -= s
    return sp.csr_matrix(C)


@pytest.mark.parametrize("shape", [(3, 4, 5), (4, 4, 4)])
def test_unit_kappa_is_the_kronecker_sum_of_three_circulants_exactly(shape):
    scale = (4.0, 0.5, 2.0)                                   # (powers of two: every product and sum below is exact)
    nz, ny, nx = shape
    A = operators.stencil7_kappa(np.ones((nz + 2, ny + 2, nx + 2)), pc.walls_of(pc.ALL), scale=scale)
    eye = sp.identity
    K = (sp.kron(sp.kron(circulant(nz, scale[0]), eye(ny)), eye(nx)) + sp.kron(sp.kron(eye(nz), circulant(ny, scale[1])), eye(nx))
         + sp.kron(sp.kron(eye(nz), eye(ny)), circulant(nx, scale[2])))
    K = sorted_csr(K)
    assert A.nnz == 7 * nz * ny * nx == K.nnz
    assert np.array_equal(A.indptr, K.indptr) and np.array_equal(A.indices, K.indices) and np.array_equal(A.data, K.data)


# ---- structure ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", pc.OTHERS)
@pytest.mark.parametrize("axes", pc.AXIS_SETS, ids=pc.axes_id)
@pytest.mark.parametrize("shape", [(3, 3, 3), (4, 5, 6)])
def test_structure_for_every_set_of_periodic_axes(shape, axes, other):
    kappa, sigma = pc.kappa_of(shape), pc.sigma_of("field", shape)
    walls = pc.walls_of(axes, other)
    A = pc.definition(shape, axes, other, "field")
    n = int(np.prod(shape))
    assert A.shape == (n, n) and A.indptr.dtype == np.int32 and A.indices.dtype == np.int32 and A.data.dtype == np.float64
    assert abs(A - A.T).max() == 0.0
    assert A.has_sorted_indices and all(np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0) for r in range(n))
    assert A.nnz == pc.expected_nnz(shape, axes) == _hip.KappaArgs(kappa, walls).nnz
    on_diagonal = A.indices == np.repeat(np.arange(n), np.diff(A.indptr))
    assert on_diagonal.sum() == n and (A.data[on_diagonal] > 0).all() and (A.data[~on_diagonal] < 0).all()
    # the ghost layers along the periodic axes are never read
    B = operators.stencil7_kappa(pc.nan_ghosts(kappa, axes), walls, sigma, pc.SCALE)
    assert same_matrix(A, B)
    # the rows of the cells that touch no wall are the in-grid operator's rows
    G = operators.stencil7_kappa(kappa, pc.walls_of((), other), sigma, pc.SCALE)
    idx = np.arange(n).reshape(shape)
    for r in idx[1:-1, 1:-1, 1:-1].ravel():
        a, g = slice(A.indptr[r], A.indptr[r + 1]), slice(G.indptr[r], G.indptr[r + 1])
        assert np.array_equal(A.indices[a], G.indices[g]) and np.array_equal(A.data[a], G.data[g])
    # without 'periodic' nothing changes: the walls' codes are those of WALLS
    assert operators.WALLS == ("dirichlet", "neumann") and operators.WALL_CODES == {"dirichlet": 0, "neumann": 1, "periodic": 2}


def test_a_periodic_row_sums_to_sigma_and_a_dirichlet_wall_adds_to_it():
    shape = (4, 5, 6)
    sigma = pc.sigma_of("field", shape)
    A = pc.definition(shape, pc.ALL, "dirichlet", "field")
    rows = np.asarray(A.sum(axis=1)).ravel()
    assert np.all(np.abs(rows - sigma.ravel()) <= 8 * np.finfo(float).eps * A.diagonal())
    M = pc.definition(shape, (0, 2), "dirichlet", "field")                 # y keeps its Dirichlet walls
    excess = (np.asarray(M.sum(axis=1)).ravel() - sigma.ravel()).reshape(shape)
    assert (excess[:, 0] > 0).all() and (excess[:, -1] > 0).all()
    assert np.all(np.abs(excess[:, 1:-1]) <= 8 * np.finfo(float).eps * M.diagonal().reshape(shape)[:, 1:-1])


# ---- the seam is an interior face ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("spaced", [False, True], ids=["scale", "spacing"])
@pytest.mark.parametrize("axis,shift", [(0, 1), (1, 2), (2, 1), (2, -3)])
def test_shifting_the_field_round_the_box_permutes_the_operator_bit_for_bit(axis, shift, spaced):
    shape = (4, 5, 6)
    n = int(np.prod(shape))
    walls = pc.walls_of(pc.ALL)
    kappa, sigma = pc.kappa_of(shape, decades=1.0), pc.sigma_of("field", shape)           # two decades
    widths = pc.spacing_of(shape)

    def padded(cells):
        out = np.full(tuple(s + 2 for s in shape), np.nan)               # (the ghost layers are not read)
        out[1:-1, 1:-1, 1:-1] = cells
        return out

    def operator(k, s, h):
        return operators.stencil7_kappa(k, walls, s, spacing=h) if spaced else operators.stencil7_kappa(k, walls, s, pc.SCALE)
    A = operator(kappa, sigma, widths)
    moved = [w.copy() for w in widths]
    moved[axis][1:-1] = np.roll(widths[axis][1:-1], shift)
    B = operator(padded(np.roll(kappa[1:-1, 1:-1, 1:-1], shift, axis)), np.roll(sigma, shift, axis), tuple(moved))
    old = np.roll(np.arange(n).reshape(shape), shift, axis).ravel()      # the cell a new position's values came from
    assert same_matrix(B, sorted_csr(A[old][:, old]))


# ---- widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", pc.AXIS_SETS, ids=pc.axes_id)
def test_spaced_operator_is_symmetric_and_equal_widths_give_the_scale_form(axes):
    shape = (3, 4, 5)
    kappa, sigma = pc.kappa_of(shape), pc.sigma_of("field", shape)
    for other in pc.OTHERS:
        A = pc.definition(shape, axes, other, "field", True)
        assert abs(A - A.T).max() == 0.0 and A.nnz == pc.expected_nnz(shape, axes)
        hz, hy, hx = 0.5, 2.0, 0.25                                      # (powers of two: every product is exact)
        V = hz * hy * hx
        equal = tuple(np.full(s + 2, h) for s, h in zip(shape, (hz, hy, hx)))
        S = operators.stencil7_kappa(kappa, pc.walls_of(axes, other), sigma, spacing=equal)
        T = operators.stencil7_kappa(kappa, pc.walls_of(axes, other), sigma * V, scale=(V / hz ** 2, V / hy ** 2, V / hx ** 2))
        assert same_matrix(S, T)


# ---- order --------------------------------------------------------------------------------------------------------------
def max_error(n):
    """u = sin 2 pi z sin 2 pi y sin 2 pi x on the periodic unit box, -lap u + u = f: the largest error of the discrete
    solution at the cell centres (conjugate gradients to rounding: sigma = 1 makes the operator definite)."""
    h = 1.0 / n
    x = (np.arange(n) + 0.5) * h
    s = np.sin(2.0 * np.pi * x)
    u = (s[:, None, None] * s[None, :, None] * s[None, None, :]).ravel()
    f = (12.0 * np.pi ** 2 + 1.0) * u
    A = operators.stencil7_kappa(np.ones((n + 2,) * 3), pc.walls_of(pc.ALL), 1.0, (1.0 / h ** 2,) * 3)
    v = np.zeros_like(f)
    r = f.copy()
    p = r.copy()
    rr = r @ r
    for _ in range(2000):
        Ap = A @ p
        alpha = rr / (p @ Ap)
        v += alpha * p
        r -= alpha * Ap
        new = r @ r
        if np.sqrt(new) <= 1e-13 * np.linalg.norm(f):
            break
        p = r + (new / rr) * p
        rr = new
    assert np.linalg.norm(f - A @ v) <= 1e-11 * np.linalg.norm(f)
    return np.abs(v - u).max()


def test_second_order_on_the_periodic_box():
    ratio = max_error(16) / max_error(32)
    print("periodic box: max error 16^3 / 32^3 = %.4f" % ratio)
    assert ratio >= 3.5                                                  # (second order tends to 4; measured 3.85)


# ---- refusals, before any device work -----------------------------------------------------------------------------------
UNPAIRED = [("dirichlet",) * 5 + ("periodic",), ("periodic",) + ("dirichlet",) * 5, ("periodic", "neumann") + ("periodic",) * 4,
            ("periodic", "periodic", "dirichlet", "periodic", "neumann", "neumann")]


def test_refusals_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_hip, "lib", no_device)
    shape = (8, 8, 8)
    k = pc.kappa_of(shape)
    p = {"gridLevels": 2, "cycles": 2, "smoother": "colour"}
    thin = pc.kappa_of((8, 2, 8))                                        # an extent of 2 along y
    flat = pc.kappa_of((1, 8, 8))
    calls = []
    for walls in UNPAIRED:
        calls += [lambda w=walls: operators.stencil7_kappa(k, w), lambda w=walls: operators.kappa_arguments(k.shape, w),
                  lambda w=walls: _hip.KappaArgs(k, w), lambda w=walls: _hip.kappa_assemble(k, w),
                  lambda w=walls: _hip.Hierarchy.from_kappa(k, 1, w), lambda w=walls: openmg_amd.Solver.from_kappa(k, p, w)]
    for field, axes in ((thin, (1,)), (thin, pc.ALL), (flat, (0,)), (flat, (0, 2))):
        w = pc.walls_of(axes)
        calls += [lambda f=field, w=w: operators.stencil7_kappa(f, w), lambda f=field, w=w: _hip.KappaArgs(f, w),
                  lambda f=field, w=w: _hip.kappa_assemble(f, w), lambda f=field, w=w: _hip.Hierarchy.from_kappa(f, 1, w),
                  lambda f=field, w=w: openmg_amd.Solver.from_kappa(f, p, w),
                  lambda f=field, w=w: openmg_amd.Solver.from_kappa(f, p, w, spacing=pc.spacing_of(tuple(s - 2 for s in f.shape)))]
    calls += [lambda: operators.stencil7_kappa(k, ("periodic",) * 5), lambda: operators.stencil7_kappa(k, ("Periodic",) * 6),
              lambda: operators.stencil7_kappa(k, (2,) * 6)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    # the axes of extent 2 that are not periodic are fine, and so is every extent >= 3
    a = _hip.KappaArgs(thin, pc.walls_of((0, 2), "mixed"), 0.5, (4.0, 1.0, 0.25))
    assert a.grid == (8, 2, 8) and a.periodic == (True, False, True) and a.walls == (2, 2, 1, 0, 2, 2) and a.nnz == 7 * 128 - 2 * 64
    a = _hip.KappaArgs(pc.kappa_of((3, 3, 3)), pc.walls_of(pc.ALL))
    assert a.nnz == 7 * 27 and a.periodic == (True, True, True)
    assert _hip.KappaArgs(k, pc.walls_of(())).periodic == (False, False, False)


class NoDeviceHierarchy:
    coarsening = None

    def can_update_fine(self):
        return False

    def close(self):
        pass


def test_solver_update_wants_the_periodic_pattern_on_a_periodic_solver(monkeypatch):
    # (the pattern check runs on the host before the hierarchy is asked anything: a solver put together without a device)
    shape = (4, 5, 6)
    walls = pc.walls_of((0, 2))
    kappa = pc.kappa_of(shape)
    s = openmg_amd.Solver.__new__(openmg_amd.Solver)
    s._hierarchy = NoDeviceHierarchy()
    s._kappa = (shape, walls, (1.0, 1.0, 1.0), None)
    s._pattern_of(_hip.KappaArgs(kappa, walls))
    rebuilt = []
    monkeypatch.setattr(openmg_amd.Solver, "_rebuild", lambda self, A: rebuilt.append(A))
    with pytest.raises(ValueError):
        s.update(operators.stencil7_kappa(kappa))                        # the in-grid pattern
    with pytest.raises(ValueError):
        s.update(operators.stencil7_kappa(kappa, pc.walls_of(pc.ALL)))   # another set of periodic axes
    assert not rebuilt
    A_new = operators.stencil7_kappa(pc.kappa_of(shape, seed=3), walls, 0.25)
    s.update(A_new)
    assert rebuilt == [A_new]
    s._hierarchy = None


def test_the_header_names_the_code_and_keeps_the_two_it_had():
    text = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    for const in ("OMG_WALL_DIRICHLET 0", "OMG_WALL_NEUMANN   1", "OMG_WALL_PERIODIC  2"):
        assert "#define " + const in text
