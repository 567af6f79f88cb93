"""The face fluxes of a solution and their cell balance made in HBM (csrc/kappa.hip kappa_flux_kernel and
face_divergence_kernel): _hip.kappa_flux against the NumPy definition operators.flux_kappa bit for bit — every
wall kind, value kind, with scale factors and with cell widths, signed zeros in u, NaN in every ghost cell that must not be
read —, device arrays, given outputs, accumulation and the refused aliases, _hip.face_divergence against
operators.divergence_faces, the discrete identity through Solver.fluxes / divergence / matvec / rhs, and a whole projection
step on device arrays.  Needs an MI355X: run with -m gpu."""
import ctypes

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import kappa_flux_cases as fc
import kappa_rhs_cases as rc
from kappa_flux_cases import EPS, same_bits
from kappa_gpu import DeviceArray, params
from kappa_rhs_cases import D, N, P

pytestmark = pytest.mark.gpu


class DeviceView:
    """`count` doubles of a DeviceArray's buffer from entry `first` on, in `shape`: an alias of it (the owner keeps the memory)."""

    def __init__(self, owner, first, shape):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (owner.d.value + 8 * first, False),
                                         "version": 2, "strides": None}


def device_faces(shape, fill=np.nan):
    return [DeviceArray(np.full(s, fill)) for s in operators.face_shapes(shape)]


@pytest.mark.parametrize("wname", list(fc.WALLSETS))
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_the_kernel_has_the_bits_of_the_definition(shape, wname):
    walls = fc.WALLSETS[wname]
    if not fc.takes(shape, walls):
        # (an extent below 3 cannot be periodic: both layers refuse it, nothing else to compare)
        with pytest.raises(ValueError):
            _hip.kappa_flux(np.ones(tuple(n + 2 for n in shape)), np.ones(shape), walls)
        return
    u = fc.solution(shape)
    failures = []
    for vname, kinds in fc.VALUE_KINDS.items():
        kappa, values = fc.case(shape, walls, kinds)
        poisoned = fc.poison(kappa, walls)
        for how in fc.grids_of(shape):
            want = operators.flux_kappa(kappa, u, walls, values, **how)
            got = _hip.kappa_flux(poisoned, u, walls, values, **how)
            for axis in range(3):
                if not (np.isfinite(got[axis]).all() and same_bits(got[axis], want[axis])):
                    failures.append((vname, sorted(how), "zyx"[axis], int((got[axis].view(np.uint64) != want[axis].view(np.uint64)).sum())))
    assert not failures, failures


@pytest.mark.parametrize("wname", ["mixed", "periodic y", "periodic xyz"])
def test_device_arrays_given_outputs_and_accumulation(wname):
    shape, walls = (5, 6, 9), fc.WALLSETS[wname]
    kappa, values = fc.case(shape, walls, fc.VALUE_KINDS["mixture"])
    poisoned = fc.poison(kappa, walls)
    u = fc.solution(shape)
    d_kappa, d_u = DeviceArray(poisoned), DeviceArray(u.ravel())          # (u flat, as solve returns it)
    d_values = None if values is None else [DeviceArray(v) if isinstance(v, np.ndarray) else v for v in values]
    rng = np.random.default_rng(19)
    for how in fc.grids_of(shape):
        want = operators.flux_kappa(kappa, u, walls, values, **how)
        # device arrays; a given `out` comes back as it is
        out = device_faces(shape)
        back = _hip.kappa_flux(d_kappa, d_u, walls, d_values, out=out, **how)
        assert all(a is b for a, b in zip(back, out))
        assert all(same_bits(a.numpy(), w) for a, w in zip(out, want))
        # host arrays: `out` given and `out` new
        mine = [np.full(s, np.nan) for s in operators.face_shapes(shape)]
        back = _hip.kappa_flux(poisoned, u, walls, values, out=mine, **how)
        assert all(a is b for a, b in zip(back, mine)) and all(same_bits(a, w) for a, w in zip(mine, want))
        assert all(same_bits(a, w) for a, w in zip(_hip.kappa_flux(poisoned, u, walls, values, **how), want))
        # out = out + alpha F: one multiplication, one addition
        for alpha in (1.0, -1.0, 0.37):
            start = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
            expect = [s0 + alpha * w for s0, w in zip(start, want)]
            acc = [DeviceArray(s0) for s0 in start]
            _hip.kappa_flux(d_kappa, d_u, walls, d_values, out=acc, alpha=alpha, **how)
            assert all(same_bits(a.numpy(), e) for a, e in zip(acc, expect)), alpha
            host = [s0.copy() for s0 in start]
            _hip.kappa_flux(poisoned, u, walls, values, out=host, alpha=alpha, **how)
            assert all(same_bits(a, e) for a, e in zip(host, expect)), alpha


def test_an_output_that_aliases_u_or_kappa_is_refused_and_nothing_is_launched():
    shape, walls = (5, 6, 9), fc.WALLSETS["mixed"]
    n = int(np.prod(shape))
    kappa, _ = fc.case(shape, walls, None)
    counts = [int(np.prod(s)) for s in operators.face_shapes(shape)]
    # u inside a larger buffer, so that a face array can lie over it
    pool = np.random.default_rng(2).standard_normal(2 * n + 200)
    d_pool, d_kappa = DeviceArray(pool), DeviceArray(kappa)
    d_u = DeviceView(d_pool, 100, (n,))
    good = device_faces(shape, 7.0)
    aliases = [[DeviceView(d_pool, 100, operators.face_shapes(shape)[0]), good[1], good[2]],            # starts where u starts
               [good[0], DeviceView(d_pool, 100 + n - 1, operators.face_shapes(shape)[1]), good[2]],    # its first entry is u's last
               [good[0], good[1], DeviceView(d_kappa, 5, operators.face_shapes(shape)[2])],             # a view into kappa's buffer
               [good[0], DeviceView(good[0], 0, operators.face_shapes(shape)[1]), good[2]]]             # two outputs over each other
    assert kappa.size >= 5 + counts[2]
    for out in aliases:
        for alpha in (None, -1.0):
            with pytest.raises(ValueError, match="overlap"):
                _hip.kappa_flux(d_kappa, d_u, walls, out=out, alpha=alpha)
    assert np.array_equal(d_pool.numpy(), pool) and np.array_equal(d_kappa.numpy(), kappa)
    assert all((a.numpy() == 7.0).all() for a in good)
    # u itself has n entries, fewer than any face array: refused as well
    with pytest.raises(ValueError):
        _hip.kappa_flux(d_kappa, d_u, walls, out=[d_u, good[1], good[2]])
    # the C entry refuses the same on its own
    lib = _hip.lib()
    grid = (ctypes.c_int64 * 3)(*shape)
    wall = (ctypes.c_int * 6)(*[operators.WALL_CODES[w] for w in walls])
    u_ptr, k_ptr = d_pool.d.value + 800, d_kappa.d.value
    f = [a.d.value for a in good]
    alpha = ctypes.c_double(-1.0)

    def call(shape=grid, kappa=k_ptr, u=u_ptr, a=None, fz=f[0], fy=f[1], fx=f[2]):
        return lib.omg_kappa_flux(shape, kappa, 1, wall, None, u, 1, None, None, None, 1, a, fz, fy, fx, 1)
    assert call() == _hip.OMG_OK and call(a=ctypes.byref(alpha)) == _hip.OMG_OK
    for bad in (lambda: call(fz=u_ptr), lambda: call(fx=k_ptr + 40), lambda: call(fy=f[0]), lambda: call(u=None), lambda: call(kappa=None),
                lambda: call(fz=None), lambda: call(a=ctypes.byref(ctypes.c_double(np.inf))), lambda: call(a=ctypes.byref(ctypes.c_double(np.nan))),
                lambda: call(shape=(ctypes.c_int64 * 3)(1 << 10, 1 << 10, 1 << 11))):                  # face arrays beyond int32
        assert bad() == _hip.ERR_INVALID
    assert lib.omg_face_divergence(grid, f[0], f[1], f[2], 1, f[0] + 8, 1) == _hip.ERR_INVALID
    assert lib.omg_face_divergence(grid, f[0], f[1], None, 1, u_ptr, 1) == _hip.ERR_INVALID


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_the_divergence_has_the_bits_of_the_definition(shape):
    n = int(np.prod(shape))
    rng = np.random.default_rng(31)
    faces = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
    faces[0].ravel()[::4] = 0.0
    want = operators.divergence_faces(*faces)
    got = _hip.face_divergence(faces)
    assert got.shape == shape and same_bits(got, want)
    mine = np.full(n, np.nan)
    assert _hip.face_divergence(faces, out=mine) is mine and same_bits(mine.reshape(shape), want)
    d_faces, d_out = [DeviceArray(a) for a in faces], DeviceArray(np.full(n, np.nan))
    assert _hip.face_divergence(d_faces, out=d_out) is d_out and same_bits(d_out.numpy().reshape(shape), want)
    with pytest.raises(ValueError, match="overlap"):
        _hip.face_divergence(d_faces, out=DeviceView(d_faces[2], 0, (n,)))
    assert same_bits(d_faces[2].numpy(), faces[2])


IDENTITY = {"dirichlet fields": ((D,) * 6, ("field",) * 6, "scale", 0.37),
            "mixed spacing": ((N, D, D, N, D, N), ("field", "none", "scalar", "field", "none", "scalar"), "spacing", "field"),
            "periodic xyz": ((P,) * 6, None, "spacing", 0.5)}


@pytest.mark.parametrize("name", list(IDENTITY))
@pytest.mark.parametrize("where", ["host", "device"])
def test_the_identity_through_the_solver(name, where):
    shape = (8, 8, 8)
    n = 512
    walls, kinds, grid, sigma = IDENTITY[name]
    kappa, values = fc.case(shape, walls, kinds)
    how = fc.grids_of(shape)[0 if grid == "scale" else 2]
    if isinstance(sigma, str):
        sigma = np.random.default_rng(5).uniform(0.0, 2.0, size=shape)
    u = fc.solution(shape)
    A = operators.stencil7_kappa(kappa, walls, sigma, **how)
    b = operators.rhs_kappa(kappa, None, walls, values, **how)
    bound = 32 * EPS * (abs(A) @ np.abs(u.ravel()) + np.abs(b.ravel()))
    with openmg_amd.Solver.from_kappa(kappa, params(shape, 2, 4), walls, sigma, **how) as s:
        if where == "device":
            d_kappa, d_u = DeviceArray(fc.poison(kappa, walls)), DeviceArray(u.ravel())
            d_values = None if values is None else [DeviceArray(v) if isinstance(v, np.ndarray) else v for v in values]
            F = device_faces(shape)
            s.fluxes(d_kappa, d_u, d_values, out=F)
            assert all(same_bits(a.numpy(), w) for a, w in zip(F, operators.flux_kappa(kappa, u, walls, values, **how)))
            d_div, d_Au, d_b = DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n))
            assert s.divergence(F, out=d_div) is d_div
            s.matvec(d_u, out=d_Au)
            s.rhs(d_kappa, values=d_values, out=d_b)
            div, Au, rhs = d_div.numpy(), d_Au.numpy(), d_b.numpy()
        else:
            F = s.fluxes(kappa, u.ravel(), values)
            assert [a.shape for a in F] == list(operators.face_shapes(shape))
            div = s.divergence(F)
            assert div.shape == (n,)
            Au, rhs = s.matvec(u.ravel()), s.rhs(kappa, None, values)
        left = div + fc.sigma_term(sigma, u, how).ravel()
        right = Au - rhs
        ratio = float((np.abs(left - right) / bound).max())
        print("worst deviation: %.2f eps (|A||u| + |b|)" % (32 * ratio))
        assert np.all(np.abs(left - right) <= bound), ratio


def test_a_projection_step_leaves_a_divergence_free_field():
    shape, walls = (16, 16, 16), (N, N, N, N, P, P)
    n, rtol = int(np.prod(shape)), 1e-8
    rng = np.random.default_rng(77)
    kappa = np.exp(rng.uniform(-1.0, 1.0, size=tuple(e + 2 for e in shape)))
    # face velocities (times area): random, periodic in x — the seam faces equal —, none through the solid walls
    W = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
    W[0][0] = W[0][-1] = 0.0
    W[1][:, 0] = W[1][:, -1] = 0.0
    W[2][:, :, -1] = W[2][:, :, 0]
    p = params(shape, 3, 100, accel="cg", rtol=rtol, nullspace="constant")
    d_kappa = DeviceArray(fc.poison(kappa, walls))
    d_W = [DeviceArray(a) for a in W]
    d_b, d_q, d_after = DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n))
    with openmg_amd.Solver.from_kappa(d_kappa, p, walls) as s:
        assert s.divergence(d_W, out=d_b) is d_b
        b = d_b.numpy()
        assert same_bits(b.reshape(shape), operators.divergence_faces(*W))
        _, info = s.solve(d_b, out=d_q)
        assert info["norm"] <= rtol * info["rhs_norm"] and info["cycle"] < 100
        back = s.fluxes(d_kappa, d_q, out=d_W, alpha=-1.0)
        assert all(a is c for a, c in zip(back, d_W))
        s.divergence(d_W, out=d_after)
    after = [a.numpy() for a in d_W]
    ratio = float(np.linalg.norm(d_after.numpy()) / np.linalg.norm(b))
    print("||divergence(W)|| / ||b|| = %.3e after the step, the solve's %.3e (%d iterations)" % (ratio, info["norm"] / info["rhs_norm"], info["cycle"]))
    assert ratio <= 2 * rtol
    assert same_bits(after[2][:, :, 0], after[2][:, :, -1])
    # the solid walls stay closed, and the correction is the definition's
    assert not after[0][0].any() and not after[0][-1].any() and not after[1][:, 0].any() and not after[1][:, -1].any()
    F = operators.flux_kappa(kappa, d_q.numpy(), walls)
    assert all(same_bits(a, w0 + -1.0 * f) for a, w0, f in zip(after, W, F))


def test_solver_fluxes_and_divergence_refuse_another_solver_and_another_grid():
    shape = (8, 8, 8)
    kappa = rc.random_case(shape, (D,) * 6, ("none",) * 6)[0]
    u = np.ones(512)
    faces = [np.zeros(s) for s in operators.face_shapes(shape)]
    with openmg_amd.Solver(operators.stencil7_kappa(kappa), params(shape, 2, 4)) as s:
        with pytest.raises(ValueError, match="from_kappa"):
            s.fluxes(kappa, u)
        with pytest.raises(ValueError, match="from_kappa"):
            s.divergence(faces)
    with openmg_amd.Solver.from_kappa(kappa, params(shape, 2, 4)) as s:
        with pytest.raises(ValueError, match="grid"):
            s.fluxes(np.ones((10, 10, 12)), u)
        with pytest.raises(ValueError, match="grid"):
            s.divergence([np.zeros(sh) for sh in operators.face_shapes((8, 8, 10))])
        # a resident solve is not disturbed by either
        h = s.hierarchy
        b = np.random.default_rng(29).standard_normal(512)
        h.resident_load(b)
        h.resident_cycle(1, 1)
        undisturbed = h.resident_fetch().copy()
        h.resident_load(b)
        h.resident_cycle(1, 1)
        F = s.fluxes(kappa, u)
        s.divergence(F)
        assert np.array_equal(h.resident_fetch(), undisturbed)
    with pytest.raises(RuntimeError):
        s.fluxes(kappa, u)
