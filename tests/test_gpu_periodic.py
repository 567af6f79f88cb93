"""Periodic axes assembled in HBM (csrc/kappa.hip) and the routes built on them: omg_kappa_assemble against the
SciPy definition operators.stencil7_kappa, Hierarchy.from_kappa against Hierarchy(A_list, R_list) of that definition,
Solver.from_kappa / update_kappa / update against Solver(A).  Every comparison is bit for bit and with the existing routes,
never with the code under test.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import periodic_cases as pc
from kappa_gpu import DeviceArray, flags, params, run, run_pcg, same, same_solve, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 3, 3),        # 27 rows: the minimum extents, one partial workgroup
          (3, 5, 7),        # 105 rows: odd extents
          (6, 10, 12),      # 720 rows: three workgroups, the last ragged, seams inside a workgroup
          (4, 4, 64),       # 1024 rows: one workgroup is exactly one 256-row plane
          (8, 8, 8)]


# ---- assembly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", pc.AXIS_SETS, ids=pc.axes_id)
@pytest.mark.parametrize("shape", SHAPES)
def test_assembly_is_the_scipy_definition_bit_for_bit(shape, axes):
    # host arrays in and out: the three kinds of other walls x every sigma kind x both forms of the face
    pc.check_assembly(shape, axes)
    # the other ways in and out, on the form with a sigma field: once with scale factors, once with widths
    kappa = pc.nan_ghosts(pc.kappa_of(shape), axes)
    sigma = pc.sigma_of("field", shape)
    for other, spaced in (("mixed", False), ("dirichlet", True)):
        walls = pc.walls_of(axes, other)
        want = pc.definition(shape, axes, other, "field", spaced)
        kw = {"spacing": pc.spacing_of(shape)} if spaced else {"scale": pc.SCALE}
        n, nnz = want.shape[0], want.nnz
        assert nnz == pc.expected_nnz(shape, axes)
        none_p, none_i, data = _hip.kappa_assemble(kappa, walls, sigma, pattern=False, **kw)
        assert none_p is None and none_i is None and np.array_equal(data, want.data)
        assert not np.signbit(data[data == 0.0]).any()
        # device arrays in, device arrays out (poisoned first: every entry is written)
        d_kappa, d_sigma = DeviceArray(kappa), DeviceArray(sigma)
        out = (DeviceArray(np.full(n + 1, -7, dtype=np.int32)), DeviceArray(np.full(nnz, -7, dtype=np.int32)), DeviceArray(np.full(nnz, np.nan)))
        assert _hip.kappa_assemble(d_kappa, walls, d_sigma, out=out, **kw) is out
        assert pc.same_csr((out[0].numpy(), out[1].numpy(), out[2].numpy()), want)
        assert pc.same_csr(_hip.kappa_assemble(d_kappa, walls, d_sigma, **kw), want)
        only = DeviceArray(np.full(nnz, np.nan))
        _hip.kappa_assemble(kappa, walls, sigma, out=(None, None, only), **kw)
        assert np.array_equal(only.numpy(), want.data)
        # an `out` sized for the in-grid pattern is refused: the sizes follow the periodic nnz
        with pytest.raises(ValueError):
            _hip.kappa_assemble(kappa, walls, sigma, out=(None, None, DeviceArray(np.zeros(pc.expected_nnz(shape, ())))), **kw)


def test_the_unstaged_store_path_writes_the_same_arrays():
    # OMG_KAPPA_STAGE is read once per process: the other path in a child; one shape per set of axes
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import periodic_cases as pc\n"
            "shapes = [(3, 5, 7), (6, 10, 12), (4, 4, 64), (8, 8, 8), (3, 3, 3), (6, 10, 12), (6, 10, 12)]\n"
            "for shape, axes in zip(shapes, pc.AXIS_SETS):\n"
            "    pc.check_assembly(shape, axes)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMG_KAPPA_STAGE="0"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-4000:]


def test_ghost_layers_are_not_read_and_bad_cells_are_named():
    shape = (5, 7, 9)
    axes = (0, 2)                                                        # z and x periodic, y with walls
    kappa, sigma = pc.kappa_of(shape), pc.sigma_of("field", shape)
    walls = pc.walls_of(axes, "dirichlet")
    want = pc.definition(shape, axes, "dirichlet", "field")
    assert pc.same_csr(_hip.kappa_assemble(pc.nan_ghosts(kappa, axes), walls, sigma, pc.SCALE), want)

    def refused(k, text, w=walls):
        with pytest.raises(_hip.HipError) as e:
            _hip.kappa_assemble(k, w, sigma, pc.SCALE)
        assert e.value.code == _hip.ERR_INVALID and text in str(e.value), str(e.value)
        assert pc.same_csr(_hip.kappa_assemble(kappa, walls, sigma, pc.SCALE), want)     # the same process, the next call
    for value in (np.nan, 0.0, -2.0, np.inf):
        k = pc.nan_ghosts(kappa, axes)
        k[1, 3, 1] = value                                               # cell (0, 2, 0): on both seams
        k[5, 4, 9] = value                                               # a later cell: the first one is named
        refused(k, "kappa at cell (0, 2, 0)")
    # the ghost cell behind a Dirichlet wall of the axis that is not periodic is still checked ...
    k = pc.nan_ghosts(kappa, axes)
    k[3, 0, 4] = -1.0                                                    # behind -y of cell (2, 0, 3)
    refused(k, "kappa at cell (2, -1, 3)")
    with pytest.raises(ValueError):
        operators.stencil7_kappa(k, walls, sigma, pc.SCALE)
    # ... and not behind a Neumann wall
    w = pc.walls_of(axes, "mixed")                                       # -y Neumann
    assert pc.same_csr(_hip.kappa_assemble(k, w, sigma, pc.SCALE), pc.definition(shape, axes, "mixed", "field"))


# ---- hierarchies ----------------------------------------------------------------------------------------------------------
def lists_of(A0, shape, restrictions):
    R = operators.restrictionList(shape, restrictions - 1, 1)
    assert len(R) == restrictions
    return operators.coeffecientList(A0, R), R


# (walls, sigma kind, null space): the singular all-periodic operator, and periodic x and z between Dirichlet walls in y
SETTINGS = {"box": (pc.walls_of(pc.ALL), "none", "constant"), "channel": (pc.walls_of((0, 2), "dirichlet"), "field", None)}
HIERARCHY_CASES = [(shape, smoother, setting, "float64") for shape in ((8, 8, 8), (16, 16, 16), (16, 8, 16), (8, 16, 32))
                   for smoother in ("colour", "gs", "jacobi") for setting in SETTINGS]
HIERARCHY_CASES += [((16, 16, 16), "colour", "box", "float32"), ((16, 8, 16), "colour", "channel", "mixed")]


@pytest.mark.parametrize("shape,smoother,setting,dtype", HIERARCHY_CASES)
def test_from_kappa_is_the_hierarchy_made_from_the_definitions_lists(shape, smoother, setting, dtype):
    # two restrictions: at 8^3 a periodic axis reaches extent 2 on the coarsest level, where both neighbours are one column
    walls, skind, nullspace = SETTINGS[setting]
    if shape[0] != shape[2] and nullspace:
        # (the reference's restriction of a grid whose first and last extent differ is not the plain aggregation, SURVEY Q6:
        # its Galerkin operators lose the constant null space, so the box gets a sigma there and is solved as it is)
        skind, nullspace = "scalar", None
    kappa, sigma = pc.nan_ghosts(pc.kappa_of(shape, decades=1.0), pc.ALL if setting == "box" else (0, 2)), pc.sigma_of(skind, shape)
    A0 = operators.stencil7_kappa(kappa, walls, sigma, pc.SCALE)
    A, R = lists_of(A0, shape, 2)
    omega = 0.8 if smoother == "jacobi" else 1.0
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy(A, R, smoother=smoother, omega=omega, dtype=dtype, nullspace=nullspace) as ref:
        want = go(ref, b, x0, 3)
        assert np.isfinite(want[0]).all()
        if shape[0] == shape[2]:
            # omg_hierarchy_create_from_kappa: level 0 in HBM, the chain on the device, then the ordinary route
            made = _hip.Hierarchy.from_kappa(kappa, 2, walls, sigma, pc.SCALE, smoother=smoother, omega=omega, dtype=dtype, nullspace=nullspace)
        else:
            # a shape the device setup does not take: Solver.from_kappa assembles into host arrays and goes through the lists
            # (gridLevels 3 allows three restrictions; minSize 8 ends the hierarchy after two, at 64 rows)
            p = {"problemShape": shape, "gridLevels": 3, "minSize": 8, "cycles": 1, "smoother": smoother, "omega": omega, "dtype": dtype}
            if nullspace:
                p["nullspace"] = nullspace
            made = openmg_amd.Solver.from_kappa(kappa, p, walls, sigma, pc.SCALE)
        with made as m:
            h = m if isinstance(m, _hip.Hierarchy) else m.hierarchy
            assert h.n_levels == 3 and flags(h) == flags(ref)
            assert not h.can_update_fine()
            assert same(go(h, b, x0, 3), want)


@pytest.mark.parametrize("shape,restrictions,constant", [((32, 32, 32), 3, True), ((128, 128, 128), 3, False)], ids=["constant-32", "random-128"])
def test_no_fused_plan_takes_a_periodic_level(shape, restrictions, constant):
    # constant kappa: seven constants per row, what the plane passes look for; 128^3: the size from which var7 takes levels
    walls = pc.walls_of(pc.ALL)
    kappa = np.full(tuple(s + 2 for s in shape), 1.5) if constant else pc.kappa_of(shape, decades=1.0)
    sigma, nullspace = (None, "constant") if constant else (0.375, None)
    A0 = operators.stencil7_kappa(kappa, walls, sigma)
    A, R = lists_of(A0, shape, restrictions)
    b, x0 = vectors(shape)
    with _hip.Hierarchy(A, R, smoother="colour", nullspace=nullspace) as ref, \
            _hip.Hierarchy.from_kappa(kappa, restrictions, walls, sigma, smoother="colour", nullspace=nullspace) as h:
        for f in flags(h) + flags(ref):
            assert not (f["plane"] or f["stencil27"] or f["var7"]), f
        assert flags(h) == flags(ref) and not h.can_update_fine()
        assert same(run(h, b, x0, 2), run(ref, b, x0, 2))


def test_update_kappa_of_the_c_interface_refuses_a_periodic_hierarchy_and_leaves_it(monkeypatch):
    shape = (16, 16, 16)
    walls = pc.walls_of((2,), "dirichlet")
    k1, k2 = pc.kappa_of(shape, seed=11, decades=1.0), pc.kappa_of(shape, seed=21, decades=1.0)
    b, x0 = vectors(shape)
    with _hip.Hierarchy.from_kappa(k1, 2, walls, smoother="colour") as h:
        want = run(h, b, x0, 3)
        for w in (walls, None):                                          # the same walls; the in-grid ones
            with pytest.raises(_hip.HipError) as e:
                h.update_kappa(k2, w)
            assert e.value.code == _hip.ERR_INVALID
        assert same(run(h, b, x0, 3), want)
    # ... and a hierarchy with the in-grid pattern refuses periodic walls
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")               # (by default only levels of 128^3 and more take the var7 passes)
    with _hip.Hierarchy.from_kappa(k1, 2, smoother="colour") as h:
        assert h.can_update_fine()
        want = run(h, b, x0, 3)
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(k2, walls)
        assert e.value.code == _hip.ERR_INVALID
        assert same(run(h, b, x0, 3), want)


# ---- Solver ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", [{}, {"accel": "cg"}, {"cycle": "F", "overCorrection": 1.8, "accel": "cg", "dtype": "mixed"}],
                         ids=["plain", "cg", "mixed-F-cg"])
@pytest.mark.parametrize("shape", [(16, 16, 16), (16, 8, 16)])
def test_solver_with_periodic_x_and_z_between_dirichlet_walls(shape, more):
    walls = pc.walls_of((0, 2), "dirichlet")
    sigma = pc.sigma_of("field", shape)
    k1, k2 = pc.nan_ghosts(pc.kappa_of(shape, 30, 1.0), (0, 2)), pc.nan_ghosts(pc.kappa_of(shape, 31, 1.0), (0, 2))
    A1, A2 = operators.stencil7_kappa(k1, walls, sigma, pc.SCALE), operators.stencil7_kappa(k2, walls, sigma, pc.SCALE)
    b = pc.rhs_of(shape)[0]
    p = params(shape, 3, 80, rtol=1e-8, **more)
    with openmg_amd.Solver(A1, p) as ref, openmg_amd.Solver.from_kappa(k1, p, walls, sigma, pc.SCALE) as s:
        assert s.A is None and s.R is None and not s.hierarchy.can_update_fine() and flags(s.hierarchy) == flags(ref.hierarchy)
        first = ref.solve(b)
        assert first[1]["norm"] <= 1e-8 * first[1]["rhs_norm"] and first[1]["cycle"] < 80
        assert same_solve(s.solve(b), first)
        # a new field: a new hierarchy, the bits of a fresh solver
        s.update_kappa(k2, sigma=sigma)
        with openmg_amd.Solver.from_kappa(k2, p, walls, sigma, pc.SCALE) as fresh, openmg_amd.Solver(A2, p) as ref2:
            second = fresh.solve(b)
            assert same_solve(ref2.solve(b), second)
        assert same_solve(s.solve(b), second) and not np.array_equal(second[0], first[0])
        # a refused field leaves the old operator solving as before
        bad = k2.copy()
        bad[5, 5, 5] = np.nan
        with pytest.raises(_hip.HipError) as e:
            s.update_kappa(bad, sigma=sigma)
        assert e.value.code == _hip.ERR_INVALID and "kappa at cell (4, 4, 4)" in str(e.value)
        assert same_solve(s.solve(b), second)
        # update(A_new) wants the periodic pattern
        with pytest.raises(ValueError):
            s.update(operators.stencil7_kappa(k1, None, sigma, pc.SCALE))
        assert same_solve(s.solve(b), second)
        s.update(A1)
        assert same_solve(s.solve(b), first)


@pytest.mark.parametrize("more", [{}, {"accel": "cg", "cycle": "F", "overCorrection": 1.8}], ids=["plain", "F-cg"])
def test_solver_on_the_periodic_box_returns_a_zero_mean_solution(more):
    shape = (16, 16, 16)
    walls = pc.walls_of(pc.ALL)
    kappa = pc.nan_ghosts(pc.kappa_of(shape, 40, 1.0), pc.ALL)
    # (sigma = 0: the constants are its null space; an isotropic grid: a point smoother is no match for pc.SCALE's 16 : 1
    # without a Dirichlet wall or a sigma, and how fast it converges is not what this test is about)
    A = operators.stencil7_kappa(kappa, walls)
    b = pc.rhs_of(shape)[0]
    p = params(shape, 3, 300, rtol=1e-8, nullspace="constant", **more)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls) as s:
        got, want = s.solve(b), ref.solve(b)
        assert same_solve(got, want) and got[1]["norm"] <= 1e-8 * got[1]["rhs_norm"]
        assert abs(got[0].mean()) < 1e-10 * np.abs(got[0]).max()
        assert np.linalg.norm(A @ got[0] - (b - b.mean())) <= 1e-7 * np.linalg.norm(b)


def test_named_factors_solve_and_line_and_auto_stay_clean_errors():
    shape = (16, 16, 16)
    walls = pc.walls_of((2,), "dirichlet")                               # periodic x
    kappa, sigma = pc.kappa_of(shape, 50, 1.0), 0.375
    A = operators.stencil7_kappa(kappa, walls, sigma)
    b = pc.rhs_of(shape)[0]
    p = params(shape, 2, 80, rtol=1e-8, coarsening=[(1, 2, 2), (2, 2, 2)])       # (gridLevels 2: up to two restrictions, the list is consumed exactly)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls, sigma) as s:
        got = s.solve(b)
        assert same_solve(got, ref.solve(b)) and got[1]["coarsening"] == [(1, 2, 2), (2, 2, 2)] and got[1]["cycle"] < 80
    p = params(shape, 3, 80, rtol=1e-8, oddExtents="merge")
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls, sigma) as s:
        assert same_solve(s.solve(b), ref.solve(b))
    for more in ({"smoother": "line"}, {"coarsening": "auto"}):
        for make in (lambda q: openmg_amd.Solver.from_kappa(kappa, q, walls, sigma), lambda q: openmg_amd.Solver(A, q)):
            with pytest.raises(_hip.HipError) as e:
                make(params(shape, 3, 80, rtol=1e-8, **more))
            assert e.value.code == _hip.ERR_UNSUPPORTED, more


def test_device_fields_give_the_bits_of_host_fields():
    shape = (16, 16, 16)
    walls = pc.walls_of((0, 2), "mixed")
    kappa, sigma = pc.nan_ghosts(pc.kappa_of(shape, 60, 1.0), (0, 2)), pc.sigma_of("field", shape)
    b, x0 = vectors(shape)
    d_kappa, d_sigma = DeviceArray(kappa), DeviceArray(sigma)
    with _hip.Hierarchy.from_kappa(kappa, 2, walls, sigma, pc.SCALE, smoother="colour") as host, \
            _hip.Hierarchy.from_kappa(d_kappa, 2, walls, d_sigma, pc.SCALE, smoother="colour") as dev:
        assert same(run(dev, b, x0, 3), run(host, b, x0, 3))
    p = params(shape, 3, 80, rtol=1e-8, accel="cg")
    with openmg_amd.Solver.from_kappa(kappa, p, walls, sigma, pc.SCALE) as host, \
            openmg_amd.Solver.from_kappa(d_kappa, p, walls, d_sigma, pc.SCALE) as dev:
        assert same_solve(dev.solve(b), host.solve(b))
