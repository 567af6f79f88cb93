"""The 7-point operator of one coefficient per face, assembled in HBM (csrc/kappa.hip faces_values_kernel, faces_rhs_kernel,
faces_flux_kernel), and the routes built on it: _hip.faces_assemble against the NumPy definition
operators.stencil7_faces, its tie to kappa_assemble, the refusal of a bad value, Hierarchy.from_faces / update_faces against
from_fine / update_fine of that definition, Solver.from_faces / update_faces against Solver(A), rhs and fluxes against
operators.rhs_faces / flux_faces, and a projection step on device arrays.  Every comparison but the two identities is bit
for bit and with the definition or an existing route, never with the code under test.  Needs an MI355X: run with -m gpu."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import faces_cases as fc
from faces_cases import D, EPS, N, P, same_bits, same_csr
from kappa_gpu import DeviceArray, flags, params, run, run_pcg, same, same_solve, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device(arrays):
    return [DeviceArray(a) for a in arrays]


# ---- assembly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wname,skind", fc.assembly_cases())
def test_assembly_is_the_definition_bit_for_bit(shape, wname, skind):
    want = fc.definition(shape, wname, skind)
    walls = fc.WALLS[wname]
    faces, sigma = fc.faces_of(shape, walls), fc.sigma_of(skind, shape)        # (NaN on every face that must not be read)
    n, nnz = want.shape[0], want.nnz

    def check(indptr, indices, data, where):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
        assert same_bits(indptr, want.indptr) and same_bits(indices, want.indices) and same_bits(data, want.data), where
    # host arrays in, host arrays out; the values alone
    check(*_hip.faces_assemble(faces, walls, sigma), "host")
    none_p, none_i, data = _hip.faces_assemble(faces, walls, sigma, pattern=False)
    assert none_p is None and none_i is None and same_bits(data, want.data)
    # device arrays in, device arrays out (poisoned first: every entry is written)
    d_faces = device(faces)
    d_sigma = DeviceArray(sigma) if skind == "field" else sigma
    out = (DeviceArray(np.full(n + 1, -7, dtype=np.int32)), DeviceArray(np.full(nnz, -7, dtype=np.int32)), DeviceArray(np.full(nnz, np.nan)))
    assert _hip.faces_assemble(d_faces, walls, d_sigma, out=out) is out
    check(out[0].numpy(), out[1].numpy(), out[2].numpy(), "device")
    # device in, host out; host in, device values alone
    check(*_hip.faces_assemble(d_faces, walls, d_sigma), "device in, host out")
    only = DeviceArray(np.full(nnz, np.nan))
    _hip.faces_assemble(faces, walls, sigma, out=(None, None, only))
    assert same_bits(only.numpy(), want.data)


def test_both_store_paths_write_the_same_array():
    # OMG_KAPPA_STAGE is read once per process: the other path in a child
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import faces_cases as fc\nfrom openmg_amd import _hip\n"
            "for shape, wname, skind in fc.assembly_cases():\n"
            "    if skind != 'field':\n"
            "        continue\n"
            "    want = fc.definition(shape, wname, skind)\n"
            "    p, i, d = _hip.faces_assemble(fc.faces_of(shape, fc.WALLS[wname]), fc.WALLS[wname], fc.sigma_of(skind, shape))\n"
            "    assert fc.same_bits(d, want.data) and fc.same_bits(p, want.indptr) and fc.same_bits(i, want.indices), (shape, wname)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    for stage in ("0", "1"):
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMG_KAPPA_STAGE=stage), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-4000:]


# ---- the tie ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7, 9), (16, 16, 16)])
@pytest.mark.parametrize("wname", ["mixed", "periodic zx", "periodic"])
def test_the_tie_to_kappa_assemble_on_the_device(shape, wname):
    walls = fc.WALLS[wname]
    kappa, sigma = fc.kappa_of(shape), fc.sigma_of("field", shape)
    for how in (dict(scale=fc.SCALE), dict(spacing=fc.widths_of(shape))):
        C = operators.face_coefficients_kappa(kappa, walls, **how)
        carried = sigma if "scale" in how else sigma * operators.cell_volumes(how["spacing"])
        got = _hip.faces_assemble(C, walls, carried)
        want = _hip.kappa_assemble(kappa, walls, sigma, **how)
        assert all(same_bits(a, b) for a, b in zip(got, want)), sorted(how)


# ---- refusal --------------------------------------------------------------------------------------------------------------
def test_a_bad_value_is_refused_naming_the_face_by_the_ordering_rule_and_the_next_call_works():
    shape = (5, 7, 9)
    walls = (D,) * 6
    faces, sigma = fc.faces_of(shape, walls), fc.sigma_of("field", shape)
    want = fc.definition(shape, "dirichlet", "field")

    def refused(c, s, text, w=walls):
        with pytest.raises(_hip.HipError) as e:
            _hip.faces_assemble(c, w, s)
        assert e.value.code == _hip.ERR_INVALID and text in str(e.value), str(e.value)
        assert same_bits(_hip.faces_assemble(faces, walls, sigma)[2], want.data)       # the same process, the next call
    for value in (np.nan, 0.0, -2.0, np.inf):
        bad = [a.copy() for a in faces]
        bad[1][2, 3, 4] = value
        bad[1][4, 1, 1] = value                                          # a later face of the array: the smallest index is named
        bad[2][0, 0, 5] = value                                          # a smaller index in a LATER array: Cy comes before Cx
        refused(bad, sigma, "Cy at face (2, 3, 4)")
        bad[0][5, 6, 8] = value                                          # the very last face of Cz, behind the Dirichlet wall +z
        refused(bad, sigma, "Cz at face (5, 6, 8)")
    # a wall face behind a Dirichlet wall; behind a Neumann wall the same array assembles, as the definition does
    bad = [a.copy() for a in faces]
    bad[2][3, 2, 0] = np.nan
    refused(bad, sigma, "Cx at face (3, 2, 0)")
    neumann_x = (D, D, D, D, N, D)
    assert same_bits(_hip.faces_assemble(bad, neumann_x, sigma)[2], operators.stencil7_faces(bad, neumann_x, sigma).data)
    # sigma; a coefficient and a sigma in one call: the coefficient is named
    s = sigma.copy()
    s[1, 0, 8] = -0.25
    s[4, 6, 8] = np.nan
    refused(faces, s, "sigma at cell (1, 0, 8)")
    bad = [a.copy() for a in faces]
    bad[2][4, 6, 9] = np.inf                                             # (later in its array than sigma's cell in its own)
    refused(bad, s, "Cx at face (4, 6, 9)")
    refused(device(faces), DeviceArray(s), "sigma at cell (1, 0, 8)")
    refused(device(bad), DeviceArray(sigma), "Cx at face (4, 6, 9)")


# ---- creation and update ----------------------------------------------------------------------------------------------------
VAR7 = [((16, 16, 16), 3, ["var7", "host"]), ((32, 32, 32), 4, ["var7", "var7", "host"])]
SETTINGS = [("dirichlet", "none"), ("mixed", "field")]


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("wname,skind", SETTINGS)
@pytest.mark.parametrize("shape,grids,kinds", VAR7)
def test_from_faces_and_update_faces_against_from_fine_and_update_fine(monkeypatch, shape, grids, kinds, wname, skind, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")               # (by default only levels of 128^3 and more take the var7 passes)
    walls, sigma = fc.WALLS[wname], fc.sigma_of(skind, shape)
    c1, c2 = fc.faces_of(shape, walls, seed=21), fc.faces_of(shape, walls, seed=22)
    A1, A2 = fc.definition(shape, wname, skind, 21), fc.definition(shape, wname, skind, 22)
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour", dtype=dtype) as ref, \
            _hip.Hierarchy.from_faces(c1, grids - 1, walls, sigma, smoother="colour", dtype=dtype) as h:
        assert flags(h) == flags(ref)
        assert ["var7" if f["var7"] else "host" for f in flags(h)] == kinds
        assert h.can_update_fine() and ref.can_update_fine()
        assert h.sizes == ref.sizes and h.device_dtype() == ref.device_dtype()
        first = go(ref, b, x0, 5)
        assert same(go(h, b, x0, 5), first)
        # update: against a fresh from_faces of the new arrays and against update_fine of the definition's values
        h.update_faces(c2, walls, sigma)
        ref.update_fine(A2.data)
        second = go(ref, b, x0, 5)
        assert not np.array_equal(second[1], first[1])
        assert same(go(h, b, x0, 5), second)
        with _hip.Hierarchy.from_faces(device(c2), grids - 1, walls, sigma, smoother="colour", dtype=dtype) as fresh:
            assert flags(fresh) == flags(ref)
            assert same(go(fresh, b, x0, 5), second)
        # back again, from device arrays (the hierarchy's value array is reused); the resident b and x stay across an update
        h.resident_load(b, x0)
        h.update_faces(device(c1), walls, sigma)
        ref.resident_load(b, x0)
        ref.update_fine(A1.data)
        assert np.array_equal(h.resident_fetch(), ref.resident_fetch())
        assert h.resident_cycle(1, 1) == ref.resident_cycle(1, 1)
        assert same(go(h, b, x0, 5), first)
        # refused coefficients leave the hierarchy as it is; so do arrays of another grid and periodic walls
        bad = [a.copy() for a in c2]
        bad[0][5, 5, 5] = np.nan
        with pytest.raises(_hip.HipError) as e:
            h.update_faces(bad, walls, sigma)
        assert e.value.code == _hip.ERR_INVALID and "Cz at face (5, 5, 5)" in str(e.value)
        for other, w in ((fc.faces_of((8, 8, 8), walls), walls), (c2, (P, P) + tuple(walls[2:]))):
            with pytest.raises(_hip.HipError) as e:
                h.update_faces(other, w, None)
            assert e.value.code == _hip.ERR_INVALID
        assert same(go(h, b, x0, 5), first)


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
def test_constant_coefficients_give_the_plane_hierarchy_and_update_faces_refuses_it(dtype):
    shape, grids = (16, 16, 16), 3
    faces = [np.full(s, 1.5) for s in operators.face_shapes(shape)]
    A = operators.stencil7_faces(faces)
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy.from_fine(A, shape, grids - 1, "colour", dtype=dtype) as ref, \
            _hip.Hierarchy.from_faces(faces, grids - 1, smoother="colour", dtype=dtype) as h:
        assert flags(h) == flags(ref) and all(f["plane"] for f in flags(h))
        assert h.can_update_fine() == ref.can_update_fine() and not h.can_update_fine()
        want = go(ref, b, x0, 5)
        assert same(go(h, b, x0, 5), want)
        with pytest.raises(_hip.HipError) as e:
            h.update_faces(fc.faces_of(shape, (D,) * 6))
        assert e.value.code == _hip.ERR_INVALID
        assert same(go(h, b, x0, 5), want)                               # still cycles as before


# ---- Solver ---------------------------------------------------------------------------------------------------------------
def rhs_of(shape, seed=5):
    return np.random.default_rng(seed).standard_normal(int(np.prod(shape)))


def test_solver_from_faces_three_time_steps_in_place_with_device_arrays(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (16, 16, 16), 3
    n = int(np.prod(shape))
    walls, sigma = fc.WALLS["mixed"], fc.sigma_of("field", shape)
    b = rhs_of(shape)
    p = params(shape, grids, 6, accel="cg")
    steps = [fc.faces_of(shape, walls, seed=30 + step) for step in range(4)]
    d_b, d_sigma, d_u = DeviceArray(b), DeviceArray(sigma), DeviceArray(np.zeros(n))
    with openmg_amd.Solver.from_faces(device(steps[0]), p, walls, d_sigma) as s:
        assert s.A is None and s.R is None and s.parameters["problemShape"] == shape
        h = s.hierarchy
        assert h.can_update_fine() and h.level_flags(0)["var7"]
        for step in range(4):
            if step:
                s.update_faces(device(steps[step]), sigma=d_sigma)
                assert s.hierarchy is h                                   # (in place: the same hierarchy)
            _, info = s.solve(d_b, out=d_u)
            with openmg_amd.Solver.from_faces(steps[step], p, walls, sigma) as fresh:
                assert flags(fresh.hierarchy) == flags(h)
                u, want = fresh.solve(b)
            assert same_bits(d_u.numpy(), u) and info["norms"] == want["norms"] and info["cycle"] == want["cycle"], step
        # update(A_new) compares with the pattern formed on this first use
        A = operators.stencil7_faces(steps[1], walls, sigma)
        s.update(A)
        with openmg_amd.Solver(A, p) as ref:
            assert same_solve(s.solve(b), ref.solve(b))
        with pytest.raises(ValueError):
            s.update(operators.stencil27_variable(shape))
        with pytest.raises(ValueError):
            s.update_kappa(fc.kappa_of(shape))
        with pytest.raises(ValueError):
            s.update_faces(fc.faces_of((8, 8, 8), walls))
        with openmg_amd.Solver.from_kappa(fc.kappa_of(shape), p, walls) as of_kappa:
            with pytest.raises(ValueError):
                of_kappa.update_faces(steps[1])


@pytest.mark.parametrize("more", [{"smoother": "line"}, {"coarsening": "auto"}], ids=["line", "semi"])
def test_solver_from_faces_orthotropic_with_the_line_smoother_and_semicoarsening(more):
    shape = (16, 16, 16)
    walls = fc.WALLS["mixed"]
    faces = list(fc.faces_of(shape, walls, seed=61))
    faces2 = list(fc.faces_of(shape, walls, seed=62))
    for C in (faces, faces2):                                             # two decades per array, z a hundred times the others
        for axis in range(3):
            C[axis] = np.sqrt(np.cbrt(C[axis])) * (100.0 if axis == 0 else 1.0)
    A, A2 = operators.stencil7_faces(faces, walls), operators.stencil7_faces(faces2, walls)
    b = rhs_of(shape)
    p = params(shape, 3, 6, **more)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_faces(faces, p, walls) as s:
        got, want = s.solve(b), ref.solve(b)
        assert same_solve(got, want)
        assert got[1].get("lineAxis") == want[1].get("lineAxis") and got[1].get("coarsening") == want[1].get("coarsening")
        if "coarsening" in more:
            assert want[1]["coarsening"][0] == (2, 1, 1)                  # (the strong axis alone is coarsened first)
        else:
            assert want[1]["lineAxis"] == 0
        s.update_faces(faces2)                                            # (a new hierarchy, as Solver.update builds one)
        ref.update(A2)
        assert same_solve(s.solve(b), ref.solve(b))


def test_solver_from_faces_all_periodic(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, walls = (16, 16, 16), (P,) * 6
    faces, faces2 = fc.faces_of(shape, walls, seed=71), fc.faces_of(shape, walls, seed=72)
    sigma = fc.sigma_of("field", shape)
    A, A2 = operators.stencil7_faces(faces, walls, sigma), operators.stencil7_faces(faces2, walls, sigma)
    b = rhs_of(shape)
    p = params(shape, 3, 6)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_faces(device(faces), p, walls, sigma) as s:
        assert flags(s.hierarchy) == flags(ref.hierarchy) and not s.hierarchy.can_update_fine()
        assert same_solve(s.solve(b), ref.solve(b))
        old = s.hierarchy
        s.update_faces(faces2, sigma=sigma)
        assert s.hierarchy is not old                                     # (rebuilt)
        ref.update(A2)
        assert same_solve(s.solve(b), ref.solve(b))
        s.update(A)                                                       # (the periodic pattern, formed on first use)
        ref.update(A)
        assert same_solve(s.solve(b), ref.solve(b))
    for more in ({"smoother": "line"}, {"coarsening": "auto"}):
        with pytest.raises(_hip.HipError) as e:
            openmg_amd.Solver.from_faces(faces, params(shape, 3, 6, **more), walls, sigma)
        assert e.value.code == _hip.ERR_UNSUPPORTED
    # without sigma the operator is singular: the constant null space (coefficients over one decade: six iterations get somewhere)
    mild = [np.sqrt(np.cbrt(a)) for a in faces]
    S = operators.stencil7_faces(mild, walls)
    b0 = b - b.mean()
    q = params(shape, 3, 6, nullspace="constant", accel="cg")
    with openmg_amd.Solver(S, q) as ref, openmg_amd.Solver.from_faces(mild, q, walls) as s:
        got, want = s.solve(b0), ref.solve(b0)
        assert same_solve(got, want) and abs(got[0].mean()) < 1e-10 * np.abs(got[0]).max()
        assert got[1]["norm"] < 1e-2 * got[1]["rhs_norm"]


def test_update_faces_empties_the_projection_set(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, walls = (16, 16, 16), (D,) * 6
    faces, faces2 = fc.faces_of(shape, walls, seed=81), fc.faces_of(shape, walls, seed=82)
    p = params(shape, 3, 6)
    with openmg_amd.Solver.from_faces(faces, p, walls, projection=4) as s, openmg_amd.Solver.from_faces(faces2, p, walls) as fresh:
        for seed in (1, 2):
            _, info = s.solve(rhs_of(shape, seed))
        assert s.projection_size == 2 and info["basis"] == 2
        s.update_faces(faces2)
        assert s.projection_size == 0
        b = rhs_of(shape, 3)
        got, want = s.solve(b), fresh.solve(b)
        assert got[1]["projected"] == 0 and got[1]["basis"] == 1
        assert same_bits(got[0], want[0]) and got[1]["norms"] == want[1]["norms"]


# ---- rhs and fluxes -----------------------------------------------------------------------------------------------------------
BITS_SHAPES = [(4, 4, 4), (5, 7, 9), (3, 3, 70), (16, 16, 16)]


@pytest.mark.parametrize("wname", sorted(fc.WALLS) + ["neumann"])
@pytest.mark.parametrize("shape", BITS_SHAPES)
def test_rhs_and_fluxes_have_the_bits_of_the_definitions(shape, wname):
    walls = (N,) * 6 if wname == "neumann" else fc.WALLS[wname]
    faces = fc.faces_of(shape, walls)                                     # (NaN on every face that must not be read)
    u = fc.solution(shape)
    f = np.random.default_rng(9).standard_normal(shape)
    d_faces, d_u, d_f = device(faces), DeviceArray(u.ravel()), DeviceArray(f)
    rng = np.random.default_rng(19)
    failures = []
    for vname, kinds in fc.VALUE_KINDS.items():
        values = fc.values_of(shape, walls, kinds)
        d_values = None if values is None else [DeviceArray(v) if isinstance(v, np.ndarray) else v for v in values]
        for source, d_source in ((None, None), (0.625, 0.625), (f, d_f)):
            want = operators.rhs_faces(faces, source, walls, values)
            got = _hip.faces_rhs(faces, source, walls, values)
            d_out = DeviceArray(np.full(shape, np.nan))
            assert _hip.faces_rhs(d_faces, d_source, walls, d_values, out=d_out) is d_out
            if not (same_bits(got, want) and same_bits(d_out.numpy(), want)):
                failures.append(("rhs", vname, type(source).__name__))
        # in place: out = f
        mine = DeviceArray(f)
        _hip.faces_rhs(d_faces, mine, walls, d_values, out=mine)
        if not same_bits(mine.numpy(), operators.rhs_faces(faces, f, walls, values)):
            failures.append(("rhs in place", vname))
        want = operators.flux_faces(faces, u, walls, values)
        got = _hip.faces_flux(faces, u, walls, values)
        d_out = device([np.full(s, np.nan) for s in operators.face_shapes(shape)])
        back = _hip.faces_flux(d_faces, d_u, walls, d_values, out=d_out)
        assert all(a is b for a, b in zip(back, d_out))
        for axis in range(3):
            if not (np.isfinite(got[axis]).all() and same_bits(got[axis], want[axis]) and same_bits(d_out[axis].numpy(), want[axis])):
                failures.append(("flux", vname, "zyx"[axis]))
        # out = out + alpha F: one multiplication, one addition
        start = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
        expect = [s0 + -1.0 * w for s0, w in zip(start, want)]
        acc, host = device(start), [s0.copy() for s0 in start]
        _hip.faces_flux(d_faces, d_u, walls, d_values, out=acc, alpha=-1.0)
        _hip.faces_flux(faces, u, walls, values, out=host, alpha=-1.0)
        if not all(same_bits(a.numpy(), e) and same_bits(h, e) for a, h, e in zip(acc, host, expect)):
            failures.append(("flux accumulated", vname))
    assert not failures, failures


class DeviceView:
    """`shape` doubles of a DeviceArray's buffer from entry `first` on: an alias of it (the owner keeps the memory)."""

    def __init__(self, owner, first, shape):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (owner.d.value + 8 * first, False),
                                         "version": 2, "strides": None}


def test_an_output_that_overlaps_an_input_is_refused_and_nothing_is_launched():
    shape, walls = (5, 6, 9), fc.WALLS["mixed"]
    n = int(np.prod(shape))
    shapes = operators.face_shapes(shape)
    faces = fc.faces_of(shape, walls, poison=False)
    pool = np.random.default_rng(2).standard_normal(2 * n + 200)
    d_pool, d_faces = DeviceArray(pool), device(faces)
    d_u = DeviceView(d_pool, 100, (n,))
    good = device([np.full(s, 7.0) for s in shapes])
    aliases = [[DeviceView(d_pool, 100, shapes[0]), good[1], good[2]],              # starts where u starts
               [good[0], DeviceView(d_pool, 100 + n - 1, shapes[1]), good[2]],      # its first entry is u's last
               [d_faces[0], good[1], good[2]],                                      # a coefficient array itself
               [good[0], good[1], DeviceView(d_faces[0], 3, shapes[2])],            # a view into another coefficient array
               [good[0], DeviceView(good[0], 0, shapes[1]), good[2]]]               # two outputs over each other
    for out in aliases:
        for alpha in (None, -1.0):
            with pytest.raises(ValueError, match="overlap"):
                _hip.faces_flux(d_faces, d_u, walls, out=out, alpha=alpha)
    assert np.array_equal(d_pool.numpy(), pool) and all(same_bits(a.numpy(), c) for a, c in zip(d_faces, faces))
    assert all((a.numpy() == 7.0).all() for a in good)
    # the C entry refuses the same on its own
    lib = _hip.lib()
    grid = (ctypes.c_int64 * 3)(*shape)
    wall = (ctypes.c_int * 6)(*[operators.WALL_CODES[w] for w in walls])
    u_ptr = d_pool.d.value + 800
    c = [a.d.value for a in d_faces]
    f = [a.d.value for a in good]
    alpha = ctypes.c_double(-1.0)

    def call(shape=grid, cz=c[0], u=u_ptr, a=None, fz=f[0], fy=f[1], fx=f[2]):
        return lib.omg_faces_flux(shape, cz, c[1], c[2], 1, wall, u, 1, None, None, None, 1, a, fz, fy, fx, 1)
    assert call() == _hip.OMG_OK and call(a=ctypes.byref(alpha)) == _hip.OMG_OK
    for bad in (lambda: call(fz=u_ptr), lambda: call(fx=c[1] + 40), lambda: call(fy=c[1]), lambda: call(fy=f[0]), lambda: call(u=None),
                lambda: call(cz=None), lambda: call(fz=None), lambda: call(a=ctypes.byref(ctypes.c_double(np.inf))),
                lambda: call(shape=(ctypes.c_int64 * 3)(1 << 10, 1 << 10, 1 << 11))):                  # face arrays beyond int32
        assert bad() == _hip.ERR_INVALID


IDENTITY = {"dirichlet fields": ((D,) * 6, ("field",) * 6, 0.37),
            "mixed": ((N, D, D, N, D, N), ("field", "none", "scalar", "field", "none", "scalar"), "field"),
            "periodic": ((P,) * 6, None, 0.5)}


@pytest.mark.parametrize("name", list(IDENTITY))
@pytest.mark.parametrize("where", ["host", "device"])
def test_the_identity_through_the_solver(name, where):
    shape, n = (8, 8, 8), 512
    walls, kinds, sigma = IDENTITY[name]
    faces = fc.faces_of(shape, walls)
    values = fc.values_of(shape, walls, kinds)
    if isinstance(sigma, str):
        sigma = fc.sigma_of("field", shape)
    u = fc.solution(shape)
    A = operators.stencil7_faces(faces, walls, sigma)
    b = operators.rhs_faces(faces, None, walls, values)
    bound = 32 * EPS * (abs(A) @ np.abs(u.ravel()) + np.abs(b.ravel()))
    with openmg_amd.Solver.from_faces(faces, params(shape, 2, 4), walls, sigma) as s:
        if where == "device":
            d_faces, d_u = device(faces), DeviceArray(u.ravel())
            d_values = None if values is None else [DeviceArray(v) if isinstance(v, np.ndarray) else v for v in values]
            F = device([np.full(sh, np.nan) for sh in operators.face_shapes(shape)])
            s.fluxes(d_faces, d_u, d_values, out=F)
            assert all(same_bits(a.numpy(), w) for a, w in zip(F, operators.flux_faces(faces, u, walls, values)))
            d_div, d_Au, d_b = DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n))
            assert s.divergence(F, out=d_div) is d_div
            s.matvec(d_u, out=d_Au)
            s.rhs(d_faces, values=d_values, out=d_b)
            div, Au, rhs = d_div.numpy(), d_Au.numpy(), d_b.numpy()
        else:
            F = s.fluxes(faces, u.ravel(), values)
            assert [a.shape for a in F] == list(operators.face_shapes(shape))
            div = s.divergence(F)
            assert div.shape == (n,)
            Au, rhs = s.matvec(u.ravel()), s.rhs(faces, None, values)
            assert same_bits(rhs, b.ravel())
        left = div + (0.0 if sigma is None else (np.broadcast_to(sigma, shape) * u).ravel())
        right = Au - rhs
        ratio = float((np.abs(left - right) / bound).max())
        print("worst deviation: %.2f eps (|A||u| + |b|)" % (32 * ratio))
        assert np.all(np.abs(left - right) <= bound), ratio


# ---- a projection step --------------------------------------------------------------------------------------------------------
def test_a_projection_step_on_face_densities_leaves_a_divergence_free_field():
    shape, walls = (16, 16, 16), (N,) * 6
    n, rtol = int(np.prod(shape)), 1e-8
    rng = np.random.default_rng(77)
    # beta = 1 / rho on the faces from the arithmetic mean of a two-fluid density (the faces of the walls are not read)
    z, y, x = np.meshgrid(*(np.arange(-0.5, e + 1.0) for e in shape), indexing="ij")
    rho = np.where((z - 6.0) ** 2 + (y - 8.0) ** 2 + (x - 9.0) ** 2 < 25.0, 10.0, 1.0)          # a drop of the heavy fluid
    C = [2.0 / (rho[:-1, 1:-1, 1:-1] + rho[1:, 1:-1, 1:-1]), 2.0 / (rho[1:-1, :-1, 1:-1] + rho[1:-1, 1:, 1:-1]),
         2.0 / (rho[1:-1, 1:-1, :-1] + rho[1:-1, 1:-1, 1:])]
    C[0][0] = C[0][-1] = np.nan
    C[1][:, 0] = C[1][:, -1] = np.nan
    C[2][:, :, 0] = C[2][:, :, -1] = np.nan
    # face velocities (times area): random, none through the solid walls
    W = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
    W[0][0] = W[0][-1] = 0.0
    W[1][:, 0] = W[1][:, -1] = 0.0
    W[2][:, :, 0] = W[2][:, :, -1] = 0.0
    p = params(shape, 3, 100, accel="cg", rtol=rtol, nullspace="constant")
    d_C, d_W = device(C), device(W)
    d_b, d_q, d_after = DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n)), DeviceArray(np.zeros(n))
    with openmg_amd.Solver.from_faces(d_C, p, walls) as s:
        assert s.divergence(d_W, out=d_b) is d_b
        b = d_b.numpy()
        assert same_bits(b.reshape(shape), operators.divergence_faces(*W))
        _, info = s.solve(d_b, out=d_q)
        assert info["norm"] <= rtol * info["rhs_norm"] and info["cycle"] < 100
        back = s.fluxes(d_C, d_q, out=d_W, alpha=-1.0)
        assert all(a is c for a, c in zip(back, d_W))
        s.divergence(d_W, out=d_after)
    after = [a.numpy() for a in d_W]
    ratio = float(np.linalg.norm(d_after.numpy()) / np.linalg.norm(b))
    print("||divergence(W)|| / ||b|| = %.3e after the step, the solve's %.3e (%d iterations)" % (ratio, info["norm"] / info["rhs_norm"], info["cycle"]))
    assert ratio <= 2 * rtol                                              # (tests/test_gpu_kappa_flux.py's bound for the same statement)
    # the solid walls stay closed, and the correction is the definition's
    assert not after[0][0].any() and not after[0][-1].any() and not after[1][:, 0].any() and not after[1][:, -1].any()
    F = operators.flux_faces(C, d_q.numpy(), walls)
    assert all(same_bits(a, w0 + -1.0 * f) for a, w0, f in zip(after, W, F))
