"""The zebra line smoother on PERIODIC operators ('smoother': 'line-periodic'; OMG_SMOOTH_LINE* | OMG_SMOOTH_LINE_WRAP,
csrc/line.hip) against the restatement of tests/line_periodic_cases.py, which solves every colour's lines with SuperLU in
float64 and never touches the code under test.  A case is "named axes periodic, lines along axis" (shapes in C order):
wrapped neighbours across the lines (the seam lines are each other's neighbours, in a full and in a ragged bundle), cyclic
lines along a periodic axis (unit stride and strided, even and odd lengths, m = 3, the two special cells in a whole group
and in the ragged tail), a wrap level below the finest, all axes periodic with and without a null space, 2-D.

Gates: tests/test_gpu_line.py's — a sweep to rtol 1e-9 / atol 1e-11 in fp64 and to 200 eps32 * line_condition * max(1,
max|x|) in fp32 (line_condition over the block WITH its corner entries), every cycle's norm to 1e-10 relative plus
norm_floor, the iterate to the fp64 gate.  Needs an MI355X: run with -m gpu."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import line_periodic_cases as lp
from kappa_gpu import DeviceArray, same_solve

pytestmark = pytest.mark.gpu

WRAP = _hip.SMOOTH_LINE_WRAP


def wrap_code(pr, axis):
    return _hip.line_smoother_code(axis, pr["shape"], wrap=True)


def open_wrap(pr, axis, **kw):
    h = _hip.Hierarchy(pr["A"], pr["R"], smoother=wrap_code(pr, axis), nullspace=pr["nullspace"], **kw)
    assert h.level_flags(0)["line"] and not h.level_flags(0)["fused_last_set"] and not h.level_flags(0)["plane"]
    assert h.line_axis == axis and h.smoother == wrap_code(pr, axis) and _hip.is_line_smoother(h.smoother)
    return h


def device_cycles(h, b, pre, post, n, x0=None):
    h.resident_load(b, x0)
    norms = [h.resident_cycle(pre, post) for _ in range(n)]
    return np.array(norms), h.resident_fetch()


def same_run(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------- 1. one and two sweeps on every smoothed level ------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", lp.PERIODIC)
def test_sweeps_per_level_are_the_restated_sweeps(name, dtype):
    pr = lp.problem(name)
    rng = np.random.default_rng(8)
    axes = lp.admissible_axes(pr)
    assert pr["axis"] in axes
    for axis in axes:
        with open_wrap(pr, axis, dtype=dtype) as h:
            for level in range(len(pr["R"])):
                assert h.level_flags(level)["line"]
                n = pr["A"][level].shape[0]
                b, x0 = rng.standard_normal(n), rng.standard_normal(n)
                for sweeps in (1, 2):
                    got = h.smooth(level, b, x0.copy(), sweeps)
                    want = lp.zebra(name, level, axis, b, x0, sweeps)
                    err = np.abs(got - want).max()
                    print("%s axis %d level %d %s (periodic %s), %d sweep(s): max diff %.2e of max|x| %.2e"
                          % (name, axis, level, dtype, lp.periodic_on(pr, level), sweeps, err, np.abs(want).max()))
                    if dtype == "float64":
                        assert np.allclose(got, want, **lp.CYC), (name, axis, level, sweeps, err)
                    else:
                        tol = 200 * lp.EPS32 * lp.line_condition(pr, level, axis) * max(1.0, np.abs(want).max())
                        assert err <= tol, (name, axis, level, sweeps, err, tol)


# ------------------------------------------------- 2. five cycles against the restatement ------
@pytest.mark.parametrize("name", lp.PERIODIC)
def test_five_cycles_follow_the_restatement(name):
    pr = lp.problem(name)
    axis = pr["axis"]
    sm = lp.smoother_of(pr, "line", axis)
    failures = []
    with open_wrap(pr, axis) as h:
        for pre, post in lp.SWEEPS:
            for shape, alpha in lp.SHAPES:
                want_norms, want_x = lp.restated_cycles(pr, sm, shape, alpha, pre, post, 5)
                h.set_cycle(shape, alpha)
                norms, x = device_cycles(h, pr["b"], pre, post, 5)
                floor = lp.norm_floor(pr["A0"], pr["b"], want_x)
                d = max(abs(a - c) / c for a, c in zip(norms, want_norms))
                print("%s %s alpha %.1f V(%d,%d): norms %.3e -> %.3e, rel diff %.2e, floor %.2e, iterate max diff %.2e"
                      % (name, shape, alpha, pre, post, want_norms[0], want_norms[-1], d, floor, np.abs(x - want_x).max()))
                ok = all(abs(a - c) <= lp.NORM_RTOL * c + floor for a, c in zip(norms, want_norms)) and np.allclose(x, want_x, **lp.CYC)
                if not ok:
                    failures.append((shape, alpha, pre, post, d, float(np.abs(x - want_x).max())))
    assert not failures, failures


# ----------------------------------------- 3. in-grid operators: the flag changes no bit ------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", lp.IN_GRID)
def test_in_grid_operators_have_the_bits_of_the_plain_code(name, dtype):
    pr = lp.problem(name)
    rng = np.random.default_rng(9)
    plain = _hip.line_smoother_code(pr["axis"], pr["shape"])
    for code in (plain, _hip.SMOOTH_LINE):                    # the named axis, and the library's own choice
        with _hip.Hierarchy(pr["A"], pr["R"], smoother=code, dtype=dtype) as h0, \
                _hip.Hierarchy(pr["A"], pr["R"], smoother=code | WRAP, dtype=dtype) as h1:
            assert h0.line_axis == h1.line_axis == pr["axis"] and h1.smoother == code | WRAP
            for level in range(len(pr["R"])):
                assert h0.level_flags(level) == h1.level_flags(level)
                n = pr["A"][level].shape[0]
                b, x0 = rng.standard_normal(n), rng.standard_normal(n)
                assert np.array_equal(h0.smooth(level, b, x0.copy(), 1), h1.smooth(level, b, x0.copy(), 1))
            assert same_run(device_cycles(h0, pr["b"], 1, 1, 3), device_cycles(h1, pr["b"], 1, 1, 3))


# ------------------------------------------------------------------------- 4. the axis 'auto' ---
def test_auto_counts_the_wrapped_entries_and_has_the_bits_of_the_explicit_axis():
    pr = lp.problem("auto")
    A, shape = sp.coo_matrix(pr["A0"]), pr["shape"]
    # this test's own expectation: the largest sum of |a_ij| per axis, an entry belonging to the axis along which its row
    # and its column differ — the wrapped ones included
    rc, cc = np.array(np.unravel_index(A.row, shape)), np.array(np.unravel_index(A.col, shape))
    differs = rc != cc
    assert (differs.sum(axis=0) <= 1).all()
    sums = [float(np.abs(A.data[differs[a]]).sum()) for a in range(3)]
    print("sum |a| per axis:", sums)
    assert int(np.argmax(sums)) == 1 and sums[1] > 10 * max(sums[0], sums[2])
    with _hip.Hierarchy(pr["A"], pr["R"], smoother=_hip.SMOOTH_LINE | WRAP) as h:
        assert h.line_axis == 1 and h.smoother == 11
        auto = device_cycles(h, pr["b"], 1, 1, 2)
    with open_wrap(pr, 1) as h:
        explicit = device_cycles(h, pr["b"], 1, 1, 2)
    assert same_run(auto, explicit)
    with _hip.Hierarchy(pr["A"], pr["R"], smoother="line-periodic") as h:
        assert h.line_axis == 1 and same_run(device_cycles(h, pr["b"], 1, 1, 2), explicit)
    # a wrapped axis that is the strong one: 'ringx' (factor 100 along the periodic unit-stride axis)
    ring = lp.problem("ringx")
    with _hip.Hierarchy(ring["A"], ring["R"], smoother="line-periodic") as h:
        assert h.line_axis == 2
        auto = device_cycles(h, ring["b"], 1, 1, 2)
    with open_wrap(ring, 2) as h:
        assert same_run(auto, device_cycles(h, ring["b"], 1, 1, 2))


# --------------------------------------------------------------------------- 5. convergence ------
@pytest.mark.parametrize("name,cpu_cycles", [("chan", 8), ("chanN", 10)])
def test_convergence_on_the_channel(name, cpu_cycles):
    """(8, 32, 8), z and x periodic, y clustered by tanh(beta = 3), 3 grids, V(1,1) sweeps in F(1.8) cycles: 'line-periodic'
    along y needs the restatement's number of cycles to 1e-8 ||b|| (+-1; at most 20 — 8 with Dirichlet walls, 10 with
    Neumann walls and the constant null space), and 'colour' run for that many cycles stays at the norm its own restatement
    (the oracle's red-black sweep) predicts, more than 1e3 targets away."""
    pr = lp.problem(name)
    b = pr["b"]
    nb = float(np.linalg.norm(b))
    target = 1e-8 * nb
    want = lp.restated_cycles_to(pr, lp.smoother_of(pr, "line", 1), "F", 1.8, 1, 1, target, 40)
    print("restated 'line-periodic' on %s: %d cycles (%d on the CPU when the case was written)" % (name, len(want), cpu_cycles))
    assert want[-1] < target and len(want) <= 20, want
    with open_wrap(pr, 1) as h:
        h.set_cycle("F", 1.8)
        h.resident_load(b)
        norms = []
        while len(norms) < len(want) + 2:
            norms.append(h.resident_cycle(1, 1))
            if norms[-1] < target:
                break
    print("line-periodic F(1.8): device %d cycles, restatement %d; device norms / ||b||:" % (len(norms), len(want)), np.array(norms) / nb)
    assert norms[-1] < target and abs(len(norms) - len(want)) <= 1, (len(norms), len(want))
    colour_want = lp.restated_cycles(pr, lp.smoother_of(pr, "colour", None), "F", 1.8, 1, 1, len(want))[0][-1]
    with _hip.Hierarchy(pr["A"], pr["R"], smoother="colour", nullspace=pr["nullspace"]) as h:
        h.set_cycle("F", 1.8)
        h.resident_load(b)
        colour_norm = h.resident_cycles(1, 1, len(want))[-1]
    print("colour F(1.8) after %d cycles: %.3e ||b|| (restated %.3e ||b||)" % (len(want), colour_norm / nb, colour_want / nb))
    assert colour_want > 1e3 * target, (colour_want, target)
    assert colour_norm >= (1.0 - 1e-6) * colour_want, (colour_norm, colour_want)


# ---------------------------------------------------------------- 6. what is refused, and how ---
def create_code(A, R, smoother, dtype=_hip.DTYPE_F64):
    A = [_hip.as_csr(M) for M in A]
    R = [_hip.as_csr(M) for M in R]
    arrA = (_hip.CsrView * len(A))(*[_hip.csr_view(M) for M in A])
    arrR = (_hip.CsrView * max(len(R), 1))(*[_hip.csr_view(M) for M in R])
    out = ctypes.c_void_p()
    code = _hip.lib().omg_hierarchy_create_ex(len(A), arrA, arrR, smoother, 1.0, dtype, ctypes.byref(out))
    message = _hip.lib().omg_last_error().decode()
    if out.value:
        _hip.lib().omg_hierarchy_destroy(out)
    return code, message


def test_refusals_leave_the_process_usable():
    ring = lp.problem("ringx")

    def usual():
        with open_wrap(ring, 2) as h:
            return device_cycles(h, ring["b"], 1, 1, 2)

    before = usual()
    # an odd periodic extent across the lines
    odd = lp.problem("odd")
    for axis in (0, 2):
        code, message = create_code(odd["A"], odd["R"], wrap_code(odd, axis))
        assert code == _hip.ERR_UNSUPPORTED and "level 0" in message and "extent 9" in message and "coarsening" in message, (code, message)
    assert same_run(usual(), before)
    # the plain codes keep refusing a periodic operator
    for smoother in (_hip.SMOOTH_LINE, _hip.SMOOTH_LINE_X, _hip.SMOOTH_LINE_Y, _hip.SMOOTH_LINE_Z):
        code, message = create_code(ring["A"], ring["R"], smoother)
        assert code == _hip.ERR_UNSUPPORTED and "level 0" in message and "in-grid neighbours" in message, (smoother, code, message)
    assert same_run(usual(), before)
    # cyclic lines whose cross couplings are all (stored) zeros, no sigma: every line's block is singular
    shape = (16, 24)
    A0 = lp.face_operator(shape, (0.0, 1.0), seed=5, periodic=(1,))
    assert A0.nnz == 5 * A0.shape[0] - 2 * shape[1] and np.count_nonzero(A0.data) < A0.nnz
    Rl, _ = lp.aggregation(shape)
    Ac = sp.csr_matrix(Rl @ A0 @ Rl.T + sp.identity(Rl.shape[0]))
    code, message = create_code([A0, Ac], [Rl], _hip.line_smoother_code(1, shape, wrap=True))
    assert code == _hip.ERR_INVALID and "pivot" in message and "row" in message, (code, message)
    # (with the cross couplings there the same construction is taken)
    A1 = lp.face_operator(shape, (1.0, 1.0), seed=5, periodic=(1,))
    assert create_code([A1, sp.csr_matrix(Rl @ A1 @ Rl.T)], [Rl], _hip.line_smoother_code(1, shape, wrap=True))[0] == _hip.OMG_OK
    assert same_run(usual(), before)
    # the flag alone, the flag on a point smoother, 7 | 8 and 7
    for smoother in (8, 9, 10, 15, 7, 16 | 3, 32 | 11):
        code, message = create_code(ring["A"], ring["R"], smoother)
        assert code == _hip.ERR_INVALID, (smoother, code, message)
    # lines along Z on a 2-D grid
    sq = lp.problem("sqring")
    assert create_code(sq["A"], sq["R"], _hip.SMOOTH_LINE_Z | WRAP)[0] == _hip.ERR_INVALID
    assert same_run(usual(), before)
    # the entries that do not take the line codes do not take these
    cube = (8, 8, 8)
    for code_line in (11, 12):
        with pytest.raises(_hip.HipError) as e:
            _hip.Hierarchy.from_fine(operators.stencil_poisson(cube), cube, 1, smoother=code_line)
        assert e.value.code == _hip.ERR_UNSUPPORTED
        with pytest.raises(_hip.HipError) as e:
            _hip.gauss_seidel(ring["A0"], ring["b"], np.zeros(ring["b"].size), smoother=code_line, iterations=1)
        assert e.value.code == _hip.ERR_UNSUPPORTED
    # 'coarsening': 'auto' on a periodic operator
    p = {"problemShape": ring["shape"], "gridLevels": 2, "preIterations": 1, "postIterations": 1, "cycles": 2, "threshold": 0.0,
         "smoother": "line-periodic", "coarsening": "auto", "minSize": 1}
    for spelled in (None, 2):
        with pytest.raises(_hip.HipError) as e:
            openmg_amd.mgSolve(ring["A0"], ring["b"], dict(p, lineAxis=spelled))
        assert e.value.code == _hip.ERR_UNSUPPORTED
    assert same_run(usual(), before)
    with _hip.Hierarchy(ring["A"], ring["R"], smoother="colour") as h:
        assert h.line_axis is None and not h.level_flags(0)["line"]


# --------------------------------------------------------------------------- 7. on top ------
def chan_params(**more):
    return dict({"problemShape": lp.CHAN_SHAPE, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "smoother": "line-periodic",
                 "cycles": 40, "threshold": 0.0, "rtol": 1e-8, "minSize": 1, "cycle": "F", "overCorrection": 1.8}, **more)


def test_mgsolve_and_solver_from_kappa_on_the_channel():
    kappa, walls, spacing = lp.chan_arguments()
    pr = lp.problem("chan")
    A0, b = pr["A0"], pr["b"]
    nb = float(np.linalg.norm(b))
    p = chan_params()
    with openmg_amd.Solver(operators.stencil7_kappa(kappa, walls, None, spacing=spacing), dict(p)) as ref:
        assert ref.hierarchy.level_flags(0)["line"] and ref.hierarchy.level_flags(1)["line"] and ref.hierarchy.line_axis == 1
        want = ref.solve(b)
    assert want[1]["lineAxis"] == 1 and want[1]["norm"] <= 1e-8 * nb and want[1]["cycle"] <= 20
    assert np.linalg.norm(b - A0 @ want[0]) <= 2e-8 * nb
    with openmg_amd.Solver.from_kappa(kappa, dict(p), walls, None, spacing=spacing) as s:
        got = s.solve(b)
        assert same_solve(got, want) and got[1]["lineAxis"] == 1
        # device arrays
        d_kappa = DeviceArray(kappa)
        with openmg_amd.Solver.from_kappa(d_kappa, dict(p), walls, None, spacing=spacing) as dev:
            assert same_solve(dev.solve(b), want)
        # an explicit axis, and the smoother that does not get there
        with openmg_amd.Solver.from_kappa(kappa, dict(p, lineAxis=1), walls, None, spacing=spacing) as named:
            assert same_solve(named.solve(b), want)
        # update_kappa: a new setup (can_update_fine is false), the bits of a fresh solver
        assert not s.hierarchy.can_update_fine()
        kappa2 = lp.chan_arguments(seed=32)[0]
        s.update_kappa(kappa2)
        assert s.hierarchy.level_flags(0)["line"] and s.hierarchy.line_axis == 1
        with openmg_amd.Solver.from_kappa(kappa2, dict(p), walls, None, spacing=spacing) as fresh:
            second = fresh.solve(b)
        assert same_solve(s.solve(b), second) and not np.array_equal(second[0], want[0])
    # mgSolve: the same hierarchy, the same bits
    mp = {k: v for k, v in p.items() if k != "rtol"}
    u, info = openmg_amd.mgSolve(A0, b, dict(mp, giveInfo=True, cycles=want[1]["cycle"]))
    assert info["lineAxis"] == 1 and info["cycle"] == want[1]["cycle"]
    assert np.array_equal(u, want[0]) and info["norm"] == want[1]["norm"]
    openmg_amd.clear_cache()


@pytest.mark.parametrize("more", [{"accel": "cg"}, {"dtype": "mixed"}, {"accel": "cg", "dtype": "mixed"}])
def test_fcg_and_mixed_precision_reach_1e_8_on_the_channel(more):
    pr = lp.problem("chan")
    A0, b = pr["A0"], pr["b"]
    nb = float(np.linalg.norm(b))
    # (the solve stops on its own norm — FCG's is the recurrence's — at half the target; the TRUE residual is held to 1e-8)
    with openmg_amd.Solver(A0, chan_params(rtol=5e-9, **more)) as s:
        u, info = s.solve(b)
    print("chan %s: %d iterations, true residual %.2e ||b||" % (more, info["cycle"], np.linalg.norm(b - A0 @ u) / nb))
    assert info["cycle"] <= 20 and info["lineAxis"] == 1
    assert np.linalg.norm(b - A0 @ u) <= 1e-8 * nb
    openmg_amd.clear_cache()


def test_a_named_coarsening_on_the_ring():
    """x first, then all three: level 1 is (8, 12, 8), still periodic along x — its lines cyclic, of length 8"""
    pr = lp.problem("ringx")
    A0, b = pr["A0"], pr["b"]
    nb = float(np.linalg.norm(b))
    factors = [(1, 1, 2), (2, 2, 2)]
    p = {"problemShape": pr["shape"], "gridLevels": 2, "preIterations": 1, "postIterations": 1, "smoother": "line-periodic",
         "cycles": 30, "threshold": 1e-8 * nb, "minSize": 1, "coarsening": factors, "giveInfo": True}
    u, info = openmg_amd.mgSolve(A0, b, dict(p))
    assert info["coarsening"] == factors and tuple(info["levelShapes"][1]) == (8, 12, 8) and info["lineAxis"] == 2
    assert info["cycle"] < 30 and np.linalg.norm(b - A0 @ u) <= 1e-8 * nb * (1.0 + 1e-6)
    with _hip.Hierarchy(info["A"], info["R"], smoother=wrap_code(pr, 2)) as h:
        assert h.level_flags(1)["line"]
        norms, x = device_cycles(h, b, 1, 1, info["cycle"])
    assert np.array_equal(x, u)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["ringx", "wrap"])
def test_runs_batches_and_graphs_agree_bit_for_bit(name, dtype):
    pr = lp.problem(name)
    b = pr["b"]
    with open_wrap(pr, pr["axis"], dtype=dtype) as h:
        first = device_cycles(h, b, 1, 1, 4)
        again = device_cycles(h, b, 1, 1, 4)
        assert same_run(first, again)
        h.resident_load(b)
        batch = h.resident_cycles(1, 1, 4)
        assert np.array_equal(np.array(batch), first[0]) and np.array_equal(h.resident_fetch(), first[1])
        h.use_graph(True)
        for _ in range(2):                                   # (captured, then replayed)
            h.resident_load(b)
            replay = h.resident_cycles(1, 1, 4)
            assert np.array_equal(np.array(replay), first[0]) and np.array_equal(h.resident_fetch(), first[1])
        single = device_cycles(h, b, 1, 1, 4)
        assert same_run(single, first)
        h.use_graph(False)
        doubled = device_cycles(h, 2.0 * b, 1, 1, 4)
        assert np.array_equal(doubled[0], 2.0 * first[0]) and np.array_equal(doubled[1], 2.0 * first[1])
    with open_wrap(pr, pr["axis"], dtype=dtype) as h2:         # a second hierarchy
        assert same_run(device_cycles(h2, b, 1, 1, 4), first)
