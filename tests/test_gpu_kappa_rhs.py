"""The right-hand side of a coefficient-field operator made in HBM (csrc/kappa.hip kappa_rhs_kernel) and the
routes built on it: _hip.kappa_rhs against the NumPy definition operators.rhs_kappa bit for bit — every wall kind, value
kind, source kind, with scale factors and with cell widths, NaN in every ghost cell that must not be read —, device arrays
and in-place output, Solver.rhs + Solver.solve reproducing a linear field, and Solver.matvec / Hierarchy.spmv_dev against
Hierarchy.spmv.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import kappa_rhs_cases as rc
from kappa_gpu import DeviceArray, params
from kappa_rhs_cases import D, N, P

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1),
          (1, 5, 7),
          (3, 3, 3),
          (5, 6, 9),        # 270 cells: a workgroup boundary inside a line and a ragged last group
          (4, 8, 16)]       # exactly two groups
WALLSETS = {"dirichlet": (D,) * 6, "neumann": (N,) * 6, "mixed": (N, D, D, N, D, N),
            "periodic x": (D, N, N, D, P, P), "periodic y": (N, D, P, P, D, N), "periodic z": (P, P, D, N, N, D),
            "periodic xyz": (P,) * 6}
VALUE_KINDS = {"none": None, "scalars": ("scalar",) * 6, "fields": ("field",) * 6,
               "mixture": ("field", "none", "scalar", "field", "none", "scalar")}
SCALE = (0.3, 1.7, 2.9)


def takes(shape, walls):
    return all(shape[axis] >= 3 for axis in range(3) if walls[2 * axis] == P)


def grids_of(shape):
    """scale factors; cell widths with ghost widths 0; cell widths with ghost widths that are not 0"""
    return [dict(scale=SCALE),
            dict(spacing=tuple(rc.widths(n, 1.3, 0.0) for n in shape)),
            dict(spacing=(rc.widths(shape[0], 1.3, "mirror"), rc.widths(shape[1], 0.0, 0.021), rc.widths(shape[2], 1.7, "mirror")))]


def sources_of(shape):
    field = np.random.default_rng(17).standard_normal(shape)
    field.ravel()[::3] = -0.0
    return [None, 0.75, field]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("wname", list(WALLSETS))
@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernel_has_the_bits_of_the_definition(shape, wname):
    walls = WALLSETS[wname]
    if not takes(shape, walls):
        # (an extent below 3 cannot be periodic: both layers refuse it, nothing else to compare)
        with pytest.raises(ValueError):
            _hip.kappa_rhs(np.ones(tuple(n + 2 for n in shape)), walls=walls)
        return
    failures = []
    for vname, kinds in VALUE_KINDS.items():
        kappa, values = rc.random_case(shape, walls, kinds or ("none",) * 6)
        if kinds is None:
            values = None
        poisoned = rc.poison_unread_ghosts(kappa, walls, values)
        for how in grids_of(shape):
            for f in sources_of(shape):
                want = operators.rhs_kappa(kappa, f, walls, values, **how)
                got = _hip.kappa_rhs(poisoned, f, walls, values, **how)
                if not (np.isfinite(got).all() and same_bits(got, want)):
                    failures.append((vname, sorted(how), type(f).__name__, int((got.view(np.uint64) != want.view(np.uint64)).sum())))
    assert not failures, failures
    if wname == "periodic xyz":                            # no wall at all: the volume term alone
        f = sources_of(shape)[2]
        assert same_bits(_hip.kappa_rhs(kappa, f, walls), f + 0.0)


@pytest.mark.parametrize("wname", ["mixed", "periodic y"])
def test_device_arrays_give_the_bits_of_host_arrays_and_out_may_be_f(wname):
    shape, walls = (5, 6, 9), WALLSETS[wname]
    n = int(np.prod(shape))
    kappa, values = rc.random_case(shape, walls, VALUE_KINDS["mixture"])
    poisoned = rc.poison_unread_ghosts(kappa, walls, values)
    f = sources_of(shape)[2]
    d_kappa = DeviceArray(poisoned)
    d_values = [DeviceArray(v) if isinstance(v, np.ndarray) else v for v in values]
    for how in grids_of(shape):
        for source in (f, 0.75, None):
            want = operators.rhs_kappa(kappa, source, walls, values, **how)
            d_f = DeviceArray(source) if isinstance(source, np.ndarray) else source
            out = DeviceArray(np.full(n, np.nan))
            assert _hip.kappa_rhs(d_kappa, d_f, walls, d_values, out=out, **how) is out
            assert same_bits(out.numpy().reshape(shape), want)
            if d_f is not None and not isinstance(d_f, float):
                assert _hip.kappa_rhs(d_kappa, d_f, walls, d_values, out=d_f, **how) is d_f      # in place
                assert same_bits(d_f.numpy(), want)
    # a host `out` for host arrays
    mine = np.empty(shape)
    assert _hip.kappa_rhs(poisoned, f, walls, values, out=mine, **how) is mine
    assert same_bits(mine, operators.rhs_kappa(kappa, f, walls, values, **how))
    # refusals that need real device arrays: size, residency
    for call in (lambda: _hip.kappa_rhs(d_kappa, DeviceArray(f), walls, d_values, out=DeviceArray(np.zeros(n + 1))),
                 lambda: _hip.kappa_rhs(d_kappa, DeviceArray(f), walls, d_values, out=np.empty(n)),
                 lambda: _hip.kappa_rhs(poisoned, f, walls, values, out=DeviceArray(np.zeros(n))),
                 lambda: _hip.kappa_rhs(d_kappa, f, walls, d_values, out=DeviceArray(np.zeros(n))),
                 lambda: _hip.kappa_rhs(d_kappa, DeviceArray(f), walls, values, out=DeviceArray(np.zeros(n))),
                 lambda: _hip.kappa_rhs(d_kappa, DeviceArray(f.astype(np.float32)), walls, d_values, out=DeviceArray(np.zeros(n)))):
        with pytest.raises(ValueError):
            call()


def test_the_c_entry_refuses_bad_arguments():
    import ctypes
    lib = _hip.lib()
    shape = (ctypes.c_int64 * 3)(3, 4, 5)
    kappa, b = np.ones((5, 6, 7)), np.empty(60)
    kinds = lambda *k: (ctypes.c_int * 6)(*k)
    scalars = (ctypes.c_double * 6)(*([1.0] * 6))
    no_fields = (ctypes.c_void_p * 6)()

    def call(walls=None, value_kinds=None, fields=no_fields, f=None, f_kind=0, shape=shape, out=b):
        return lib.omg_kappa_rhs(shape, kappa.ctypes.data, 0, walls, None, f, f_kind, 0, value_kinds, scalars, fields, 0,
                                 None if out is None else out.ctypes.data, 0)
    assert call() == _hip.OMG_OK and not b.any()
    assert call(value_kinds=kinds(1, 1, 1, 1, 1, 1)) == _hip.OMG_OK and b.reshape(3, 4, 5)[1, 1, 1] == 0.0 and b[0] == 3.0
    periodic_x = (ctypes.c_int * 6)(0, 0, 1, 1, 2, 2)
    for bad in (lambda: call(walls=periodic_x, value_kinds=kinds(0, 0, 0, 0, 1, 0)),         # a value on a periodic wall
                lambda: call(value_kinds=kinds(2, 0, 0, 0, 0, 0)),                           # a field announced and NULL
                lambda: call(value_kinds=kinds(3, 0, 0, 0, 0, 0)),
                lambda: call(f_kind=2), lambda: call(f_kind=7, f=b.ctypes.data), lambda: call(out=None),
                lambda: call(walls=(ctypes.c_int * 6)(0, 0, 0, 0, 2, 0)),
                lambda: call(shape=(ctypes.c_int64 * 3)(1 << 12, 1 << 12, 1 << 12))):          # n beyond int32
        assert bad() == _hip.ERR_INVALID
    assert call() == _hip.OMG_OK


# ---- end to end: Solver.from_kappa, Solver.rhs, Solver.solve ------------------------------------------------------------
E2E_SHAPE = (16, 16, 16)
# The 2-norm condition numbers of the two operators below, measured once on the CPU (numpy.linalg.eigvalsh of
# operators.stencil7_kappa(...).toarray(), 4096 rows): lambda_max / lambda_min = 2.570 / 3.789e-3 = 678 with Dirichlet y
# walls; lambda_max / lambda_2 = 2.570 / 2.004e-3 = 1283 on the complement of the constants with every wall Neumann or
# periodic.  ||u - u*|| / ||u*|| <= cond ||b - A u|| / ||b||, and the solve stops at 1e-10 ||b||: that supports 6.8e-8 and
# 1.3e-7, not the 1e-8 first hoped for.
E2E_BOUND = {"dirichlet y": 678 * 1e-10, "neumann": 1283 * 1e-10}


def e2e_problem(kind):
    walls = (N, N, D, D, P, P) if kind == "dirichlet y" else (N, N, N, N, P, P)
    spacing = (rc.widths(16, 0.0, "mirror"), rc.widths(16, 1.5, 0.0), rc.widths(16, 0.0, "mirror"))      # stretched y, values on the wall faces
    kappa_x = np.exp(np.sin(2.0 * np.pi * (np.arange(16) + 0.5) / 16.0) * np.log(3.0))                    # kappa varies along the periodic axis
    kappa, scale, values, u = rc.linear_problem(E2E_SHAPE, walls, spacing, kappa_x=kappa_x)
    return walls, spacing, kappa, values, u


@pytest.mark.parametrize("kind", ["dirichlet y", "neumann"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_rhs_then_solve_reproduces_the_linear_field(kind, where):
    walls, spacing, kappa, values, u_exact = e2e_problem(kind)
    n = u_exact.size
    p = params(E2E_SHAPE, 3, 60, accel="cg", cycle="F", overCorrection=1.8, rtol=1e-10)
    if kind == "neumann":
        p["nullspace"] = "constant"
    with openmg_amd.Solver.from_kappa(kappa, p, walls, spacing=spacing) as s:
        if where == "device":
            d_b = DeviceArray(np.full(n, np.nan))
            d_values = [None if v is None else DeviceArray(v) for v in values]
            assert s.rhs(DeviceArray(kappa), values=d_values, out=d_b) is d_b
            b = d_b.numpy()
            assert same_bits(b, s.rhs(kappa, values=values))
            d_u = DeviceArray(np.zeros(n))
            _, info = s.solve(d_b, out=d_u)
            u = d_u.numpy()
        else:
            b = s.rhs(kappa, values=values)
            assert b.shape == (n,) and same_bits(b, operators.rhs_kappa(kappa, None, walls, values, spacing=spacing).ravel())
            u, info = s.solve(b)
        assert info["norm"] <= 1e-10 * info["rhs_norm"] and info["cycle"] < 60
        got, want, b_held = u, u_exact.ravel(), b
        if kind == "neumann":
            assert abs(b.sum()) <= 64 * np.finfo(float).eps * np.abs(b).sum()        # (the data are compatible)
            got, want, b_held = u - u.mean(), want - want.mean(), b - b.mean()      # (solve projects b and returns mean 0)
        error = np.linalg.norm(got - want) / np.linalg.norm(want)
        print("relative error %.3e after %d iterations (bound %.1e)" % (error, info["cycle"], E2E_BOUND[kind]))
        assert error <= E2E_BOUND[kind]
        # ||b - A u|| formed with matvec is the norm the solve reported (the fp64 floor of tests/test_gpu_cycle_shapes.py)
        A0 = operators.stencil7_kappa(kappa, walls, None, spacing=spacing)
        k = int(np.diff(A0.indptr).max())
        floor = 2.0 * (k + 2) * 2.0 ** -53 * float(np.linalg.norm(np.abs(b_held) + abs(A0) @ np.abs(u)))
        if where == "device":
            d_y = DeviceArray(np.zeros(n))
            assert s.matvec(d_u, out=d_y) is d_y
            Au = d_y.numpy()
            assert np.array_equal(Au, s.matvec(u))
        else:
            Au = s.matvec(u)
        residual = float(np.linalg.norm(b_held - Au))
        assert abs(residual - info["norm"]) <= 1e-10 * info["norm"] + floor, (residual, info["norm"], floor)


# ---- Solver.matvec --------------------------------------------------------------------------------------------------
# (5, 6, 9) and (8, 12, 20) are set up through the host lists whatever the smoother — the device setup takes grids whose first
# and last extents are equal and even on every restricted level —, so the plain device route, where no host matrix exists,
# is met at (8, 12, 8).  One restriction: level 0 is the level matvec is about.
@pytest.mark.parametrize("route, shape", [("from_kappa", (5, 6, 9)), ("from_kappa", (8, 12, 20)), ("device route", (8, 12, 8)),
                                          ("line", (5, 6, 9)), ("line", (8, 12, 20))])
def test_matvec_is_the_hierarchys_spmv(shape, route):
    n = int(np.prod(shape))
    kappa = rc.random_case(shape, (D,) * 6, ("none",) * 6)[0]
    p = params(shape, 2 if route == "device route" else 1, 4)
    if route == "line":
        s = openmg_amd.Solver(operators.stencil7_kappa(kappa), dict(p, smoother="line"))
    else:
        s = openmg_amd.Solver.from_kappa(kappa, p)
    with s:
        if route == "device route":
            assert s.A is None and s.hierarchy.n_levels == 3
        h = s.hierarchy
        x = np.random.default_rng(23).standard_normal(n)
        want = h.spmv(0, x)
        assert np.allclose(want, operators.stencil7_kappa(kappa) @ x, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        assert np.array_equal(s.matvec(x), want)
        mine = np.empty(n)
        assert s.matvec(x, out=mine) is mine and np.array_equal(mine, want)
        d_x, d_y = DeviceArray(x), DeviceArray(np.full(n, np.nan))
        assert s.matvec(d_x, out=d_y) is d_y and np.array_equal(d_y.numpy(), want)
        assert s.matvec(d_x, out=d_x) is d_x and np.array_equal(d_x.numpy(), want)       # in place
        for call in (lambda: s.matvec(x[:-1]), lambda: s.matvec(x, out=np.empty(n + 1)), lambda: s.matvec(DeviceArray(x), out=DeviceArray(x[:-1]))):
            with pytest.raises(ValueError):
                call()
        for call in (lambda: s.matvec(x, out=d_y), lambda: s.matvec(d_y, out=mine)):
            with pytest.raises(TypeError):
                call()
        # between resident_load and resident_fetch a device matvec disturbs nothing
        b = np.random.default_rng(29).standard_normal(n)
        h.resident_load(b)
        h.resident_cycle(1, 1)
        undisturbed = h.resident_fetch().copy()
        h.resident_load(b)
        h.resident_cycle(1, 1)
        s.matvec(DeviceArray(x), out=d_y)
        assert np.array_equal(h.resident_fetch(), undisturbed) and np.array_equal(d_y.numpy(), want)
        h.resident_cycle(1, 1)                              # (... and the solve goes on)
    with pytest.raises(RuntimeError):
        s.matvec(x)


def test_matvec_refuses_a_mixed_hierarchy():
    shape = (8, 8, 8)
    kappa = rc.random_case(shape, (D,) * 6, ("none",) * 6)[0]
    with openmg_amd.Solver.from_kappa(kappa, params(shape, 2, 4, dtype="mixed", accel="cg")) as s:
        with pytest.raises(ValueError, match="mixed"):
            s.matvec(np.ones(512))
        with pytest.raises(_hip.HipError) as e:
            s.hierarchy.spmv_dev(0, 4096, 4096)
        assert e.value.code == _hip.ERR_UNSUPPORTED
