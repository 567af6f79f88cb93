"""The constant-coefficient passes with seven DIFFERENT couplings (tests/stencils.py).

Every level on the headline path is a constant-coefficient star stencil held as seven constants c[0..6] = (-K, -J, -I,
diagonal, +I, +J, +K): the marching, block and 2-D tile kernels and the matrix-free SpMV of openmg_amd/csrc/plane.hip, the
slab passes of dist.hip, plane_step_kernel / defect_plane_kernel of pcg.hip, plane_constants() and build_device() in
hierarchy.hip / plane.hip, the lexicographic sweeps of march.hip.  PlanePlan::build accepts any seven constants, but every
other GPU test of these kernels builds its operator from operators.stencil_poisson (times a scalar, or with whole rows
scaled): all six off-diagonals of a row are equal there on every level, so a kernel that read c[0] for c[6], -J for +J in
the mirrored up pass, the wrong slot for a ghost plane, or filled the constants from the wrong offset would pass them all.

Here the operator is UNSYM7 / UNSYM5 (all couplings different, unsymmetric) — SYM7 only where a run to convergence of
the conjugate gradients needs symmetry; the FCG and mixed-precision kernels see UNSYM7 too — on boxes
with three different extents (a cube hides a swap of two axes).  References: the set-by-set schedule of the same
hierarchy (the generic CSR row kernels, which tests/test_gpu_property.py pins to the CPU oracle on arbitrary CSR) — the
iterate bit for bit — and the CPU oracle itself.  Tolerances are the project's own: np.array_equal on iterates; close()
of tests/test_gpu_plane.py on norms (1e-13 in fp64, 1e-12 in fp32; 1e-12 / 1e-6 between the two marching directions);
against the oracle BASELINE's 1e-10 on every norm (plus norm_floor) and CYC on the iterate, from
tests/test_gpu_cycle_shapes.py; for FCG and mixed precision the gates of tests/test_gpu_pcg.py and tests/test_gpu_mixed.py.

CASES in tests/stencils.py lists every (set, shape, grids) used below; tests/test_stencils_host.py checks without a GPU
that each of them has one value per offset on every level — the condition under which 'this level must carry the plane
flag' is a fair assertion."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, _hip_dist
from oracle import mg_oracle as orc
from stencils import (FCG_BOX, FCG_LARGE, MARCHING, MIRROR, ORACLE, ROUGH_CASE, SETS, SLABS, SPMV, TILE2D, UNSYM7, hierarchy,
                      level_shapes, line_problem, stencil_constant)
from test_gpu_cycle_shapes import CYC, norm_floor, norms_agree, restated_cycles
from test_gpu_march import scaled_rows, smooth_on_device, sweep
from test_gpu_mixed import same_norm, true_norm
from test_gpu_pcg import fcg_cpu, pcg_gpu
from test_gpu_plane import close, run
from test_gpu_plane_dist import slabs

pytestmark = pytest.mark.gpu

SWEEPS = ((1, 1), (2, 1), (1, 0), (0, 1), (0, 0))
DTYPES = ("float64", "float32")
PLANE_KEYS = ("OMG_PLANE", "OMG_PLANE_TILE", "OMG_PLANE_BLOCK", "OMG_PLANE_LA2", "OMG_PLANE_MIRROR")


@pytest.fixture(autouse=True)
def restore_environment():
    saved = dict(os.environ)
    yield
    os.environ.clear()
    os.environ.update(saved)


def set_env(env):
    """The plane switches for the hierarchies made from here on: exactly `env` (restore_environment puts the rest back)."""
    for k in PLANE_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)


@functools.lru_cache(maxsize=None)
def problem(name, shape, grids):
    """Galerkin lists, a right-hand side and a first iterate (both exact in fp32 too); shared, never written to."""
    A, R = hierarchy(shape, grids, SETS[name])
    rng = np.random.default_rng(41)
    n = A[0].shape[0]
    b = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    x0 = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    for v in (b, x0):
        v.setflags(write=False)
    return A, R, b, x0


def relaxed_flags(h, grids):
    return [h.level_flags(l)["plane"] for l in range(grids - 1)]


_set_schedule = {}


def set_schedule(name, shape, grids, dtype):
    """{(pre, post): (norms, x)}: three cycles from x0 on the set-by-set schedule (a hierarchy made under OMG_PLANE=0; the caller
    sets its own environment afterwards)."""
    key = (name, shape, grids, dtype)
    if key not in _set_schedule:
        A, R, b, x0 = problem(name, shape, grids)
        set_env({"OMG_PLANE": "0"})
        with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
            assert not any(relaxed_flags(h, grids))
            _set_schedule[key] = {sw: run(h, b, sw[0], sw[1], 3, x0) for sw in SWEEPS}
    return _set_schedule[key]


def norm_tol(dtype):
    return 1e-13 if dtype == "float64" else 1e-12


def differences(got, ref, dtype):
    """None, or what differs: the iterate bit for bit, the norms as tests/test_gpu_plane.py compares them."""
    if not np.all(np.isfinite(got[1])) or not np.all(np.isfinite(got[0])):
        return "not finite"
    if not np.array_equal(got[1], ref[1]):
        return "%d entries of the iterate differ, by up to %.3e" % (int(np.sum(got[1] != ref[1])), np.abs(got[1] - ref[1]).max())
    if not close(got[0], ref[0], norm_tol(dtype)):
        return "norms %r against %r" % (got[0], ref[0])
    return None


# ---------------------------------------- a. marching, block and look-ahead kernels == the set schedule --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,grids,env,tile", MARCHING)
def test_marching_and_block_kernels_have_the_bits_of_the_set_schedule(shape, grids, env, tile, dtype):
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    ref = set_schedule("UNSYM7", shape, grids, dtype)
    set_env(env)
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
        assert all(relaxed_flags(h, grids)), (shape, relaxed_flags(h, grids))
        info = h.plane_info(0)
        assert (info["nz"], info["ny"], info["nx"]) == tuple(shape)
        if tile:
            for level in range(grids - 1):
                info = h.plane_info(level)
                assert [info["tile_x"], info["tile_y"], info["tile_z"]] == [int(v) for v in tile.split(",")], (level, info)
        for sw in SWEEPS:
            bad = differences(run(h, b, sw[0], sw[1], 3, x0), ref[sw], dtype)
            assert bad is None, (shape, env, dtype, sw, bad)


# ---------------------------------------------------------------------------------- b. the mirrored up pass --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,grids", MIRROR)
def test_up_pass_marching_down_or_up_is_one_iterate_and_the_set_schedule_s(shape, grids, dtype):
    """OMG_PLANE_MIRROR (read per call): the up pass marching from the last plane to the first exchanges the roles of
    -K / +K along the march, not in the row."""
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    ref = set_schedule("UNSYM7", shape, grids, dtype)
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
        assert all(relaxed_flags(h, grids))
        for sw in SWEEPS:
            os.environ["OMG_PLANE_MIRROR"] = "1"
            down = run(h, b, sw[0], sw[1], 3, x0)
            os.environ["OMG_PLANE_MIRROR"] = "0"
            up = run(h, b, sw[0], sw[1], 3, x0)
            assert np.array_equal(down[1], up[1]), (shape, dtype, sw, int(np.sum(down[1] != up[1])))
            assert close(down[0], up[0], 1e-6 if dtype == "float32" else 1e-12), (shape, dtype, sw, down[0], up[0])
            for name, got in (("down", down), ("up", up)):
                bad = differences(got, ref[sw], dtype)
                assert bad is None, (shape, dtype, sw, name, bad)


# ------------------------------------------------------------------------------ c. batches and graph replay --
@pytest.mark.parametrize("dtype", DTYPES)
def test_batches_and_graph_replay_have_the_bits_of_single_cycles(dtype):
    shape, grids = (16, 24, 20), 3
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    ref = set_schedule("UNSYM7", shape, grids, dtype)
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
        assert all(relaxed_flags(h, grids))
        single = {sw: run(h, b, sw[0], sw[1], 3, x0) for sw in ((1, 1), (1, 0))}
        for sw, want in single.items():
            assert differences(want, ref[sw], dtype) is None, (sw, differences(want, ref[sw], dtype))
            h.resident_load(b, x0)
            batch = h.resident_cycles(sw[0], sw[1], 1) + h.resident_cycles(sw[0], sw[1], 2)
            assert batch == want[0] and np.array_equal(h.resident_fetch(), want[1]), ("batch", dtype, sw)
        h.use_graph(True)
        for sw, want in single.items():
            graph = run(h, b, sw[0], sw[1], 3, x0)
            assert graph[0] == want[0] and np.array_equal(graph[1], want[1]), ("graph", dtype, sw)
        h.use_graph(False)


# -------------------------------------------------------------------------------------- d. 2-D tile passes --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("smoother", ["colour", "jacobi"])
@pytest.mark.parametrize("shape,grids", TILE2D)
def test_2d_tile_passes_have_the_bits_of_the_set_schedule(shape, grids, smoother, dtype):
    A, R, b, x0 = problem("UNSYM5", shape, grids)
    kw = {"smoother": smoother, "dtype": dtype}
    if smoother == "jacobi":
        kw["omega"] = 2.0 / 3.0
    set_env({})
    with _hip.Hierarchy(A, R, **kw) as h:
        assert all(relaxed_flags(h, grids)), (shape, smoother, relaxed_flags(h, grids))
        info = h.plane_info(0)
        assert (info["nz"], info["ny"], info["nx"]) == (1,) + tuple(shape)
        for sw in SWEEPS:
            h.use_plane(True)
            got = run(h, b, sw[0], sw[1], 3, x0)
            h.use_plane(False)
            assert not h.level_flags(0)["plane"]
            ref = run(h, b, sw[0], sw[1], 3, x0)
            bad = differences(got, ref, dtype)
            assert bad is None, (shape, smoother, dtype, sw, bad)


# ------------------------------------------------------------------------------------ e. matrix-free SpMV --
@pytest.mark.parametrize("name,shape", SPMV)
def test_matrix_free_spmv(name, shape):
    """plane_spmv_kernel against the row kernels on the same operator — same bits — and against SciPy's product, within
    the tolerances of tests/test_gpu_plane.py test_matrix_free_spmv_of_a_plane_level."""
    A, R, _, x = problem(name, shape, 2)
    set_env({})
    for dtype in DTYPES:
        with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
            assert h.level_flags(0)["plane"]
            got = h.spmv(0, x)
            h.use_plane(False)
            ref = h.spmv(0, x)
        assert np.array_equal(got, ref), (shape, dtype, int(np.sum(got != ref)), np.abs(got - ref).max())
        np.testing.assert_allclose(got, A[0] @ x, rtol=1e-13 if dtype == "float64" else 1e-5, atol=1e-12 if dtype == "float64" else 1e-5)


# ----------------------------------------------------------------------------------- f. against the oracle --
@functools.lru_cache(maxsize=None)
def oracle_problem(name, shape, grids):
    A, R, _, _ = problem(name, shape, grids)
    b = A[0] @ np.random.default_rng(12345).random(A[0].shape[0])
    b.setflags(write=False)
    return {"A": A, "R": R, "A0": A[0], "b": b, "sm": orc.make_smoother("colour", A)}


def against_the_oracle(pr, h, what):
    """Four V(1,1) and V(2,1) cycles against orc.mg_cycle, four ('F', 1.5) cycles against the restatement of
    tests/test_gpu_cycle_shapes.py (the factor is a kernel argument of exactly these passes)."""
    A, R, b = pr["A"], pr["R"], pr["b"]
    for pre, post in ((1, 1), (2, 1)):
        p = {"preIterations": pre, "postIterations": post, "coarsestLevel": len(R)}
        h.set_cycle("V", 1.0)
        h.resident_load(b)
        norms, want, xo = [], [], None
        for _ in range(4):
            norms.append(h.resident_cycle(pre, post))
            xo, info = orc.mg_cycle(A, b, 0, R, p, initial=xo, smoother=pr["sm"])
            want.append(info["norm"])
        x = h.resident_fetch()
        print("%s V(%d,%d): norms %r, oracle %r, iterate max diff %.2e" % (what, pre, post, norms, want, np.abs(x - xo).max()))
        assert norms_agree(norms, want, norm_floor(pr["A0"], b, xo)), (what, pre, post, norms, want)
        assert np.allclose(x, xo, **CYC), (what, pre, post, np.abs(x - xo).max())
        assert want[-1] < 0.1 * want[0]
    want, xo = restated_cycles(pr, "F", 1.5, 1, 1, 4)
    h.set_cycle("F", 1.5)
    h.resident_load(b)
    norms = [h.resident_cycle(1, 1) for _ in range(4)]
    x = h.resident_fetch()
    h.set_cycle("V", 1.0)
    print("%s F 1.5: norms %r, restatement %r, iterate max diff %.2e" % (what, norms, list(want), np.abs(x - xo).max()))
    assert norms_agree(norms, want, norm_floor(pr["A0"], b, xo)), (what, norms, want)
    assert np.allclose(x, xo, **CYC), (what, np.abs(x - xo).max())


@pytest.mark.parametrize("name,shape,grids", ORACLE)
def test_cycles_against_the_oracle(name, shape, grids):
    pr = oracle_problem(name, shape, grids)
    set_env({})
    with _hip.Hierarchy(pr["A"], pr["R"], smoother="colour") as h:
        assert all(relaxed_flags(h, grids)), relaxed_flags(h, grids)
        against_the_oracle(pr, h, "%s %r" % (name, shape))


# ------------------------------------------------------------------------------------------------ g. slabs --
@pytest.mark.parametrize("pre,post", [(1, 1), (1, 0)])
@pytest.mark.parametrize("shape,grids,n_dist", SLABS)
def test_plane_slabs_have_the_bits_of_the_single_gpu_cycle(shape, grids, n_dist, pre, post):
    """PlaneDistGroup as tests/test_gpu_plane_dist.py runs it: the one place where -K and +K cross a ghost plane."""
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    assert _hip_dist.star_coefficients(A[0], shape) == list(UNSYM7)
    for l, sh in enumerate(level_shapes(shape, n_dist)):
        c = _hip_dist.star_coefficients(A[l], sh)
        assert len(set(c)) == 7 and c[3] > 0 and all(v < 0 for v in c[:3] + c[4:]), (l, c)
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        assert all(relaxed_flags(h, grids))
        h.resident_load(b, x0)
        want_norms = [h.resident_cycle(pre, post) for _ in range(3)]
        want = h.resident_fetch()
    for n_ranks in (1, 2, 4):
        assert (shape[0] >> (n_dist - 1)) // n_ranks >= 2          # every distributed level needs two planes per rank
        g = _hip_dist.PlaneDistGroup(slabs(A, R, shape, n_ranks, n_dist, b, x0))
        try:
            norms = g.cycles(2, pre, post) + g.cycles(1, pre, post)
            got = np.concatenate([r.fetch() for r in g.ranks])
        finally:
            g.close()
        assert np.array_equal(got, want), (shape, n_ranks, pre, post, int(np.sum(got != want)), np.abs(got - want).max())
        np.testing.assert_allclose(norms, want_norms, rtol=1e-13)


# ----------------------------------------------------------------------------------------- h. device setup --
def test_device_setup_routes_agree_with_the_lists_route():
    """Hierarchy.from_fine (build_device, plane_check_kernel) and mgSolve, on a cube (the reference's restriction is the
    plain aggregation only there): the bits of the lists route built from info['A'] and info['R']."""
    shape, grids = (16, 16, 16), 3
    A0 = stencil_constant(shape, UNSYM7)
    _, _, b, x0 = problem("UNSYM7", shape, grids)
    set_env({})
    p = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0,
         "giveInfo": True, "smoother": "colour"}
    try:
        u, info = openmg_amd.mgSolve(A0, b, dict(p))
        u2 = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=False))          # (without the lists: the device setup route)
    finally:
        openmg_amd.clear_cache()
    assert len(info["A"]) == grids and len(info["R"]) == grids - 1
    with _hip.Hierarchy(info["A"], info["R"], smoother="colour") as h:
        assert all(relaxed_flags(h, grids)), relaxed_flags(h, grids)
        zero = run(h, b, 1, 1, 3)
    assert info["norm"] == zero[0][-1] and np.array_equal(u, zero[1]) and np.array_equal(u2, zero[1])
    for dtype in DTYPES + ("mixed",):
        with _hip.Hierarchy(info["A"], info["R"], smoother="colour", dtype=dtype) as h, \
                _hip.Hierarchy.from_fine(A0, shape, grids - 1, smoother="colour", dtype=dtype) as f:
            assert all(relaxed_flags(f, grids)), (dtype, relaxed_flags(f, grids))
            for pre, post, first in ((1, 1, None), (2, 1, x0)):
                want, got = run(h, b, pre, post, 3, first), run(f, b, pre, post, 3, first)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (dtype, pre, post)


# ----------------------------------------------------------------------------------------------- i. ROUGH7 --
def test_constants_that_are_not_dyadic():
    """ROUGH7's coarse sums may round differently from row to row; a level may then decline the plane passes, and that is
    correct: results only — default build against OMG_PLANE=0, and against the oracle.  The flags are reported, not asserted."""
    shape, grids = ROUGH_CASE
    pr = oracle_problem("ROUGH7", shape, grids)
    A, R, b, x0 = problem("ROUGH7", shape, grids)
    ref = set_schedule("ROUGH7", shape, grids, "float64")
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        flags = relaxed_flags(h, grids)
        print("ROUGH7 %r: plane flags of the relaxed levels %r" % (shape, flags))
        for sw in SWEEPS:
            bad = differences(run(h, b, sw[0], sw[1], 3, x0), ref[sw], "float64")
            assert bad is None, ("plane flags", flags, sw, bad)
        against_the_oracle(pr, h, "ROUGH7 %r (plane flags %r)" % (shape, flags))


# ---------------------------------------------------------------------------- j. FCG and mixed precision --
@functools.lru_cache(maxsize=None)
def fcg_problem(shape, grids):
    A, R, _, _ = problem("SYM7", shape, grids)
    rng = np.random.default_rng(7)
    b, x0 = rng.standard_normal(A[0].shape[0]), rng.standard_normal(A[0].shape[0])
    for v in (b, x0):
        v.setflags(write=False)
    return A, R, b, x0


@functools.lru_cache(maxsize=None)
def yardstick(shape, grids, rel, maxit):
    A, R, b, _ = fcg_problem(shape, grids)
    return fcg_cpu(A, R, b, "colour", 1, 1, rel * np.linalg.norm(b), maxit)


def test_fcg_on_a_box_against_the_cpu_yardstick():
    """plane_step_kernel on a box with three extents (a swap of ny and nz in its slot decomposition cannot hide) and three
    axis couplings: the gates of tests/test_gpu_pcg.py test_against_the_cpu_yardstick, then the generic path."""
    shape, grids = FCG_BOX
    A, R, b, _ = fcg_problem(shape, grids)
    tol = 1e-8 * np.linalg.norm(b)
    want_norms, want_x = yardstick(shape, grids, 1e-8, 200)
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        assert h.level_flags(0)["plane"]
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 200, tol)
        print("FCG %r: device %d iterations, yardstick %d" % (shape, its, len(want_norms)))
        assert not bd
        assert abs(its - len(want_norms)) <= 1, (its, len(want_norms))
        m = min(its, len(want_norms))
        np.testing.assert_allclose(norms[:m], want_norms[:m], rtol=1e-8)
        np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
        assert tn <= 2 * tol
        h.use_plane(False)
        its2, norms2, _, _, _ = pcg_gpu(h, b, 1, 1, 200, tol)
        assert its2 == its
        np.testing.assert_allclose(norms2, norms, rtol=1e-12)


def test_mixed_precision_on_a_box_against_the_fp64_yardstick():
    """dtype='mixed' on the same problem, gated as tests/test_gpu_mixed.py gates it: the outer fp64 operator of a plane
    level is seven constants read from the caller's CSR (plane_constants) and applied by plane_step_kernel /
    defect_plane_kernel.  _hip does not expose the constants, and the library reports no norm before the first correction:
    they are checked through the first reported norm from a random x0 — ||b - A0 x1|| of the iterate x1 it belongs to, to
    1e-12 relative — where a wrong constant shows in the first digit."""
    shape, grids = FCG_BOX
    A, R, b, x0 = fcg_problem(shape, grids)
    nb = np.linalg.norm(b)
    want_norms, _ = yardstick(shape, grids, 1e-10, 200)
    x1_64 = orc.mg_cycle(A, b, 0, R, {"preIterations": 1, "postIterations": 1, "coarsestLevel": len(R)},
                         smoother=orc.make_smoother("colour", A))[0]
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype="mixed") as hm:
        assert hm.device_dtype() == np.float32 and hm.level_flags(0)["plane"]
        # the seven outer constants, through the first norm from a random first iterate
        hm.resident_load(b, x0)
        n1 = hm.resident_cycle(1, 1)
        x1 = hm.resident_fetch()
        t1 = true_norm(A[0], b, x1)
        assert t1 > 1e-3 * nb
        assert abs(n1 - t1) <= 1e-12 * t1, (n1, t1)
        its, _, tn, bd, xm = pcg_gpu(hm, b, 1, 1, 200, 1e-10 * nb, x0)
        assert not bd and same_norm(tn, A[0], b, xm, 1e-12), (tn, true_norm(A[0], b, xm))
        # FCG from zero against the fp64 yardstick
        its, _, tn, bd, xm = pcg_gpu(hm, b, 1, 1, 200, 1e-10 * nb)
        print("mixed FCG %r: device %d iterations, fp64 yardstick %d" % (shape, its, len(want_norms)))
        assert not bd
        assert its <= len(want_norms) + 2, (its, len(want_norms))
        tm = true_norm(A[0], b, xm)
        assert same_norm(tn, A[0], b, xm, 1e-12), (tn, tm)
        assert tm <= 1e-10 * nb, tm / nb
        # defect correction
        hm.resident_load(b)
        norms, xs = [], []
        for _ in range(6):
            norms.append(hm.resident_cycle(1, 1))
            xs.append(hm.resident_fetch())
        for nk, xk in zip(norms, xs):
            assert same_norm(nk, A[0], b, xk, 1e-12), (nk, true_norm(A[0], b, xk))
        np.testing.assert_allclose(xs[0], x1_64, rtol=0, atol=1e-5 * np.abs(x1_64).max())
        hm.resident_load(b)
        batch = hm.resident_cycles(1, 1, 400)
        assert np.array_equal(batch[:6], np.array(norms))
        assert batch[-1] <= 1e-10 * nb, batch[-1] / nb
        assert true_norm(A[0], b, hm.resident_fetch()) <= 1e-10 * nb


def test_mixed_defect_correction_with_seven_different_outer_constants():
    """SYM7 cannot tell -J from +J: c[1] == c[5].  Defect correction is plain multigrid and needs no symmetry, so here
    UNSYM7 goes through plane_constants() and defect_plane_kernel, from a random first iterate: every reported norm is
    ||b - A0 x|| of the iterate it belongs to (1e-12; a wrong constant or offset shows in the first digit), the first iterate
    is the oracle's fp64 cycle from the same start to fp32 accuracy, batches repeat single cycles, and the run reaches fp64
    accuracy, as tests/test_gpu_mixed.py test_defect_correction gates them."""
    shape, grids = FCG_BOX
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    nb = np.linalg.norm(b)
    x1_64 = orc.mg_cycle(A, b, 0, R, {"preIterations": 1, "postIterations": 1, "coarsestLevel": len(R)}, initial=x0.copy(),
                         smoother=orc.make_smoother("colour", A))[0]
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype="mixed") as hm:
        assert hm.device_dtype() == np.float32 and hm.level_flags(0)["plane"]
        hm.resident_load(b, x0)
        norms, xs = [], []
        for _ in range(6):
            norms.append(hm.resident_cycle(1, 1))
            xs.append(hm.resident_fetch())
        t1 = true_norm(A[0], b, xs[0])
        assert t1 > 1e-3 * nb and abs(norms[0] - t1) <= 1e-12 * t1, (norms[0], t1)
        for nk, xk in zip(norms, xs):
            assert same_norm(nk, A[0], b, xk, 1e-12), (nk, true_norm(A[0], b, xk))
        np.testing.assert_allclose(xs[0], x1_64, rtol=0, atol=1e-5 * np.abs(x1_64).max())
        hm.resident_load(b, x0)
        batch = hm.resident_cycles(1, 1, 60)
        assert np.array_equal(batch[:6], np.array(norms))
        assert batch[-1] <= 1e-10 * nb, batch[-1] / nb
        assert true_norm(A[0], b, hm.resident_fetch()) <= 1e-10 * nb


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_six_fcg_iterations_with_seven_different_constants(dtype):
    """plane_step_kernel on UNSYM7: six iterations with threshold 0 are pure arithmetic on any matrix (its symmetric part is
    positive definite, so (p, A p) > 0), compared with the same iterations on the generic path (use_plane(False): norms to
    1e-12, as tests/test_gpu_pcg.py) and with fcg_cpu (its gates: norms to 1e-8, the iterate to 1e-8 max|x|) in fp64.  Mixed: the
    outer operator is the seven constants of plane_constants(); the reported true norm is ||b - A0 x|| of the fetched
    iterate, and the norms follow the fp64 yardstick while an fp32 preconditioner can (tests/test_gpu_fp32.py's 1e-3)."""
    shape, grids = FCG_BOX
    A, R, b, x0 = problem("UNSYM7", shape, grids)
    want_norms, want_x = fcg_cpu(A, R, b, "colour", 1, 1, 0.0, 6, x0=x0)
    assert len(want_norms) == 6 and want_norms[-1] < 0.1 * want_norms[0]
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
        assert h.level_flags(0)["plane"]
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 6, 0.0, x0)
        print("FCG UNSYM7 %s: norms rel diff %r" % (dtype, np.abs(norms / want_norms - 1.0)))
        assert its == 6 and not bd
        assert same_norm(tn, A[0], b, x, 1e-12), (tn, true_norm(A[0], b, x))
        if dtype == "float64":
            np.testing.assert_allclose(norms, want_norms, rtol=1e-8)
            np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
            h.use_plane(False)
            its2, norms2, _, _, x2 = pcg_gpu(h, b, 1, 1, 6, 0.0, x0)
            assert its2 == its
            np.testing.assert_allclose(norms2, norms, rtol=1e-12)
        else:
            np.testing.assert_allclose(norms, want_norms, rtol=1e-3)
            np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-3 * np.abs(want_x).max())


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_fcg_with_more_than_256_partials_per_reduction(dtype):
    """163 840 cells: 320 partials for the streaming kernels (640 chunks of 256 threads x 2 doubles), 640 for
    plane_step_kernel — fold()'s strided loop over part[t + 256] runs, against a reference.  Ten iterations, threshold 0."""
    shape, grids = FCG_LARGE
    A, R, b, _ = fcg_problem(shape, grids)
    want_norms, want_x = yardstick(shape, grids, 0.0, 10)
    assert len(want_norms) == 10
    set_env({})
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
        assert h.level_flags(0)["plane"]
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 10, 0.0)
    print("FCG %r %s: norms rel diff %r" % (shape, dtype, np.abs(norms / want_norms - 1.0)))
    assert its == 10 and not bd
    np.testing.assert_allclose(norms, want_norms, rtol=1e-8)
    assert same_norm(tn, A[0], b, x, 1e-12), (tn, true_norm(A[0], b, x))


@functools.lru_cache(maxsize=None)
def line_yardstick(rel):
    A, R, b = line_problem()
    return fcg_cpu(A, R, b, "gs", 1, 1, rel * np.linalg.norm(b), 300)


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
def test_scalar_tails_of_the_streaming_kernels(dtype):
    """n = 4099: n mod 2 = 1 and n mod 4 = 3, so the scalar tails of dots / dot / pupdate / update / residual / defect_add
    run in every element width.  fp64: the gates of test_against_the_cpu_yardstick; fp32 (to 1e-5 ||b||) and mixed: those of
    tests/test_gpu_pcg.py test_every_kind_converges and tests/test_gpu_mixed.py."""
    A, R, b = line_problem()
    nb = np.linalg.norm(b)
    rel = {"float64": 1e-8, "float32": 1e-5, "mixed": 1e-10}[dtype]
    tol = rel * nb
    want_norms, want_x = line_yardstick(rel)
    assert want_norms[-1] < tol
    with _hip.Hierarchy(A, R, smoother="gs", dtype=dtype) as h:
        its, norms, tn, bd, x = pcg_gpu(h, b, 1, 1, 300, tol)
        print("1-D FCG %s: device %d iterations, yardstick %d" % (dtype, its, len(want_norms)))
        assert not bd and np.isfinite(x).all() and norms[-1] < tol
        if dtype == "float64":
            assert abs(its - len(want_norms)) <= 1, (its, len(want_norms))
            m = min(its, len(want_norms))
            np.testing.assert_allclose(norms[:m], want_norms[:m], rtol=1e-8)
            np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
            assert tn <= 2 * tol
        else:
            assert its <= len(want_norms) + 2, (its, len(want_norms))
        if dtype == "mixed":
            tm = true_norm(A[0], b, x)
            assert same_norm(tn, A[0], b, x, 1e-12), (tn, tm)
            assert tm <= max(1e-10 * nb, 10 * true_norm(A[0], b, want_x)), tm / nb
            # defect correction: defect_add_kernel's tail
            h.resident_load(b)
            nk = h.resident_cycle(1, 1)
            xk = h.resident_fetch()
            assert same_norm(nk, A[0], b, xk, 1e-12), (nk, true_norm(A[0], b, xk))
            x1 = orc.mg_cycle(A, b, 0, R, {"preIterations": 1, "postIterations": 1, "coarsestLevel": len(R)})[0]
            np.testing.assert_allclose(xk, x1, rtol=0, atol=1e-5 * np.abs(x1).max())


# -------------------------------------------------------------------------------- k. lexicographic sweeps --
@pytest.mark.parametrize("rows", ["constant", "scaled"])
@pytest.mark.parametrize("shape", [(12, 20, 30), (17, 9, 33), (5, 64, 16)])
def test_wavefront_sweep_with_seven_different_couplings(shape, rows):
    rng = np.random.default_rng(11)
    A = stencil_constant(shape, UNSYM7)
    if rows == "scaled":
        A = scaled_rows(A, rng)
    n = A.shape[0]
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    for its in (1, 3):
        got = sweep(A, b, x0, its, march=True)
        ref = sweep(A, b, x0, its, march=False)
        assert np.array_equal(got, ref), (shape, rows, its, int(np.sum(got != ref)), np.abs(got - ref).max())
    want = orc.gauss_seidel(A, b, x0.copy(), iterations=2)
    for march in (True, False):
        np.testing.assert_allclose(sweep(A, b, x0, 2, march=march), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("shape", [(12, 20, 30), (9, 12, 130)])
def test_line_scan_sweep_with_seven_different_couplings(shape):
    """OMG_MARCH_SCAN=1 against the wavefront kernel, to the tolerance of tests/test_gpu_march.py
    test_line_scan_sweep_against_the_wavefront_kernel."""
    rng = np.random.default_rng(5)
    A = stencil_constant(shape, UNSYM7)
    n = A.shape[0]
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    for its in (1, 3):
        got, flags = smooth_on_device(A, b, x0, its, "float64", scan=True)
        ref, ref_flags = smooth_on_device(A, b, x0, its, "float64", scan=False)
        assert flags["march"] and flags["march_scan"] and ref_flags["march"] and not ref_flags["march_scan"]
        assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(np.abs(ref)), (shape, its, np.max(np.abs(got - ref)))
    got, _ = smooth_on_device(A, b, x0, 2, "float64", scan=True)
    np.testing.assert_allclose(got, orc.gauss_seidel(A, b, x0.copy(), iterations=2), rtol=1e-11, atol=1e-13)
