"""Semicoarsening on the device (parameters['coarsening']; omg_restriction_ex, omg_axis_couplings,
omg_hierarchy_create_from_fine_semi) against NumPy and the oracle's cycles on the lists mgSolve hands back.

Gates: the project's own — norms_agree / CYC / norm_floor of tests/test_gpu_cycle_shapes.py for fp64 cycles, the fp32
gates of tests/test_gpu_fp32.py (norms to 1e-3 relative above the fp32 floor 64 eps32 ||A||_inf ||x||_inf sqrt(n), the
iterate to 1e-3 of its largest entry), tests/test_gpu_pcg.py's for FCG (norms to 1e-8, iterate to 1e-8 of its largest
entry, iterations +- 1), tests/test_gpu_mixed.py's same_norm, and bit-for-bit equality between routes, repeats, graph
replay and Solver against mgSolve.  The factor sequences and cycle counts are those tests/test_semicoarsen_host.py fixes
with the oracle (tests/semicoarsen_cases.py).  Needs an MI355X: run with -m gpu."""
import functools
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

import semicoarsen_cases as sc
from stencils import UNSYM5, UNSYM7, stencil_constant
from test_gpu_cycle_shapes import CYC, device_cycles, norm_floor, norms_agree, restated_cycles
from test_gpu_mixed import same_norm, true_norm
from test_gpu_nullspace import mean_of, regularised_solve
from test_gpu_pcg import fcg_cpu

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SETTINGS = [("V", 1.0, 1, 1), ("V", 1.0, 2, 1), ("V", 1.0, 1, 0), ("F", 1.8, 1, 1)]


def all_factors(dim):
    return [f for f in itertools.product((1, 2), repeat=dim) if any(v == 2 for v in f)]


# ------------------------------------------------------------------------------- restriction --
@pytest.mark.parametrize("shape", [(8, 12, 20), (4, 6, 8), (6, 10)])
def test_restriction_ex_is_the_numpy_aggregation(shape):
    for f in all_factors(len(shape)):
        got, want = _hip.restriction_ex(shape, f), sc.aggregation(shape, f)
        assert got.shape == want.shape, f
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), f
        assert np.array_equal(got.data, want.data), f
        via = operators.restriction(shape, factors=f)
        assert np.array_equal(via.indices, want.indices) and np.array_equal(via.data, want.data)


def test_all_twos_on_a_cube_is_the_reference_restriction():
    got, want = _hip.restriction_ex((8, 8, 8), (2, 2, 2)), operators.restriction((8, 8, 8))
    assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)


def test_restriction_ex_refusals_leave_the_process_usable():
    for shape, f in (((8, 12, 21), (1, 1, 2)), ((8, 12, 2), (1, 1, 2)), ((8, 12, 20), (3, 1, 1)), ((8, 12, 20), (1, 1, 1)),
                     ((8, 12, 20), (0, 2, 2)), ((64,), (2,))):
        with pytest.raises(_hip.HipError) as e:
            _hip.restriction_ex(shape, f)
        assert e.value.code == _hip.ERR_INVALID, (shape, f)
        ok = _hip.restriction_ex((4, 6), (2, 1))
        assert np.array_equal(ok.indices, sc.aggregation((4, 6), (2, 1)).indices)


# --------------------------------------------------------------------------------- couplings --
COUPLED = [("UNSYM7", (8, 12, 20)), ("UNSYM5", (10, 22)), ("var7", (8, 12, 20))]


@pytest.mark.parametrize("name,shape", COUPLED, ids=[c[0] for c in COUPLED])
def test_axis_couplings_against_numpy(name, shape):
    A = operators.stencil7_variable(shape) if name == "var7" else stencil_constant(shape, {"UNSYM7": UNSYM7, "UNSYM5": UNSYM5}[name])
    sums, counts, off = _hip.axis_couplings(A, shape)
    want_s, want_c, want_off = sc.couplings(A, shape)
    print(name, sums, want_s, counts, off)
    assert counts == want_c and off == want_off == 0
    assert len(set(want_s)) == len(shape)                             # (all different: a swapped axis would show)
    for a, b in zip(sums, want_s):
        assert abs(a - b) <= 1e-12 * b
    again = _hip.axis_couplings(A, shape)
    assert np.array_equal(np.array(again[0]).view(np.uint64), np.array(sums).view(np.uint64)) and again[1:] == (counts, off)


def test_a_27_point_operator_is_counted_and_refused_by_the_rule():
    shape = (6, 6, 6)
    A = operators.stencil27_variable(shape)
    sums, counts, off = _hip.axis_couplings(A, shape)
    want = sc.couplings(A, shape)
    assert counts == want[1] and off == want[2] > 0
    with pytest.raises(_hip.HipError) as e:
        _hip.semicoarsen_rule(shape, sums, counts, off, level=0)
    assert e.value.code == _hip.ERR_UNSUPPORTED and "level 0" in str(e.value)


# ------------------------------------------------------------------------------- hierarchies --
def var7_x100(shape):
    """stencil7_variable with the couplings along x (unit stride) scaled by 100, the diagonal keeping the row sums' excess"""
    A = sp.csr_matrix(operators.stencil7_variable(shape))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    along_x = np.abs(A.indices - rows) == 1
    extra = np.bincount(rows[along_x], weights=-99.0 * A.data[along_x], minlength=A.shape[0])
    A.data[along_x] *= 100.0
    A = sp.csr_matrix(A + sp.diags(extra))
    A.sort_indices()
    return A


OPERATORS = {
    "yx10": lambda s: sc.aniso(s, (1, 10, 10)),
    "yx100": lambda s: sc.aniso(s, (1, 100, 100)),
    "z100x10": lambda s: sc.aniso(s, (100, 1, 10)),
    "iso": lambda s: sc.aniso(s, (1, 1, 1)),
    "var7x100": var7_x100,
    "neumann": lambda s: sc.aniso(s, (1, 100, 100), neumann=True),
    "sq100": lambda s: sc.aniso(s, (1, 100)),
}
HIER = [(n, s) for s in ((16, 16, 16), (8, 12, 20)) for n in ("yx10", "yx100", "z100x10", "iso", "var7x100", "neumann")] + [("sq100", (16, 24))]


@functools.lru_cache(maxsize=None)
def hier_case(name, shape):
    """The operator, b, and what the host says of it: the factor sequence of SciPy lists under the exported rule; then ONE
    mgSolve (fp64, 'auto', the lists route) whose lists the oracle runs on."""
    A0 = OPERATORS[name](shape)
    rng = np.random.default_rng(12345)
    b = rng.standard_normal(A0.shape[0])
    nullspace = "constant" if name == "neumann" else None
    if nullspace:
        b -= b.mean()
    host = sc.lists(A0, shape, "auto", 3, min_size=1)
    p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 5, "threshold": 0.0,
         "giveInfo": True, "smoother": "colour", "minSize": 1, "coarsening": "auto", "nullspace": nullspace}
    u, info = openmg_amd.mgSolve(A0, b, dict(p))
    b.setflags(write=False)
    return {"A0": A0, "b": b, "p": p, "u": u, "info": info, "host_factors": host[2], "host_shapes": host[3], "nullspace": nullspace,
            "A": info["A"], "R": info["R"], "shape": shape}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shape", HIER, ids=["%s-%s" % (n, "x".join(map(str, s))) for n, s in HIER])
def test_hierarchies_against_the_oracle(monkeypatch, name, shape, dtype):
    c = hier_case(name, shape)
    info, A, R, b = c["info"], c["A"], c["R"], c["b"]
    assert info["coarsening"] == c["host_factors"] and info["levelShapes"] == c["host_shapes"]
    assert [M.shape[0] for M in A] == [int(np.prod(s)) for s in c["host_shapes"]]
    for Rl, ext, f in zip(R, c["host_shapes"], c["host_factors"]):
        want = sc.aggregation(ext, f)
        assert np.array_equal(Rl.indices, want.indices) and np.array_equal(Rl.data, want.data)
    if c["nullspace"]:
        # the oracle with tests/test_gpu_nullspace.py's coarse solve (A_c + gamma 1 1^T) on the projected b (its mean is 0 already),
        # the iterate projected on the way out, at that file's gates
        monkeypatch.setattr(orc, "coarse_solve", regularised_solve)
    pr = {"A": A, "R": R, "b": b, "sm": orc.make_smoother("colour", A)}
    failures = []
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype, nullspace=c["nullspace"]) as h:
        for l in range(len(R)):
            assert not h.level_flags(l)["plane"] or c["host_factors"][l] == (2,) * len(shape)
        for kind, alpha, pre, post in SETTINGS:
            want_norms, want_x = restated_cycles(pr, kind, alpha, pre, post, 5, dtype=np.float64 if dtype == "float64" else np.float32)
            if c["nullspace"]:
                want_x = want_x - mean_of(want_x)
            h.set_cycle(kind, alpha)
            norms, x = device_cycles(h, b, pre, post, 5)
            print(name, shape, dtype, kind, alpha, pre, post, "norm rel diff %.2e iterate diff %.2e"
                  % (max(abs(a - w) / w for a, w in zip(norms, want_norms)), np.abs(x - want_x).max()))
            if dtype == "float64" and c["nullspace"]:
                good = (norms_agree(norms, want_norms, norm_floor(c["A0"], b, want_x)) and np.abs(x - want_x).max() <= 1e-9 * np.abs(want_x).max()
                        and abs(mean_of(x)) <= 64 * 2.0 ** -52 * np.abs(x).max())
            elif dtype == "float64":
                good = norms_agree(norms, want_norms, norm_floor(c["A0"], b, want_x)) and np.allclose(x, want_x, **CYC)
            else:
                floor = 64 * EPS32 * float(abs(c["A0"]).sum(axis=1).max()) * np.abs(want_x).max() * np.sqrt(b.size)
                # (1e-3 relative while the residual is above the fp32 floor, the floor itself below it)
                good = (all(abs(a - w) <= 1e-3 * w + floor for a, w in zip(norms, want_norms))
                        and np.abs(x - want_x).max() <= 1e-3 * np.abs(want_x).max())
            if not good:
                failures.append((kind, alpha, pre, post))
    assert not failures, failures
    if dtype == "float64" and not c["nullspace"]:
        want_norms, want_x = restated_cycles(pr, "V", 1.0, 1, 1, 5)
        assert norms_agree([info["norm"]], [want_norms[-1]], norm_floor(c["A0"], b, want_x)) and np.allclose(c["u"], want_x, **CYC)


# ------------------------------------------------------------------------------------ routes --
ROUTES = [
    ("yx100 auto", (16, 16, 16), (1, 100, 100), 3, "auto", "float64"),
    ("yx100 auto f32", (16, 16, 16), (1, 100, 100), 3, "auto", "float32"),
    ("yx100 named", (16, 16, 16), (1, 100, 100), 3, [(1, 2, 2), (1, 2, 2), (2, 2, 2)], "float64"),
    ("box auto", (8, 12, 20), (100, 1, 10), 3, "auto", "float64"),
    ("box named", (8, 12, 20), (1, 10, 10), 2, [(1, 2, 2), (2, 1, 1)], "float64"),
    ("square auto", (16, 24), (1, 100), 3, "auto", "float64"),
    ("cube32 x4: full coarsening below", (32, 32, 32), (1, 1, 4), 3, "auto", "float64"),
]


@pytest.mark.parametrize("name,shape,c,levels,coarsening,dtype", ROUTES, ids=[r[0] for r in ROUTES])
def test_device_route_gives_the_hierarchy_of_the_lists_route(name, shape, c, levels, coarsening, dtype):
    A0 = sc.aniso(shape, c)
    rng = np.random.default_rng(5)
    b = A0 @ rng.random(A0.shape[0])
    p = {"problemShape": shape, "gridLevels": levels, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0,
         "smoother": "colour", "dtype": dtype, "minSize": 1, "coarsening": coarsening}
    pa, pb = dict(p), dict(p, giveInfo=True)
    x_dev = openmg_amd.mgSolve(A0, b, pa)                             # the device route (giveInfo off)
    x_host, info = openmg_amd.mgSolve(A0, b, pb)                      # the lists route
    assert pa["coarsestLevel"] == pb["coarsestLevel"] == len(info["R"]) == len(info["coarsening"])
    assert np.array_equal(x_dev, x_host), (name, int(np.sum(x_dev != x_host)))
    if coarsening != "auto":
        assert info["coarsening"] == coarsening
    named = None if coarsening == "auto" else coarsening
    with _hip.Hierarchy.from_fine_semi(A0, shape, levels, named, min_size=1, smoother="colour", dtype=dtype) as h, \
            _hip.Hierarchy(info["A"], info["R"], smoother="colour", dtype=dtype) as g:
        assert h.sizes == g.sizes == [M.shape[0] for M in info["A"]]
        assert h.coarsening == info["coarsening"] and h.level_shapes == info["levelShapes"]
        assert not h.can_update_fine()
        flags = [h.level_flags(l)["plane"] for l in range(len(info["R"]))]
        assert flags == [g.level_flags(l)["plane"] for l in range(len(info["R"]))]
        for l, f in enumerate(info["coarsening"]):
            assert not flags[l] or f == (2,) * len(shape)
        if name.startswith("cube32"):
            # 1 : 1 : 4 -> (1, 1, 2), then isotropic (1 : 1/2 : 1/2 on the threshold): a rows parent over plane children
            assert info["coarsening"] == [(1, 1, 2), (2, 2, 2), (2, 2, 2)] and flags == [False, True, True]
        h.resident_load(b)
        g.resident_load(b)
        assert h.resident_norms() == g.resident_norms()
        assert h.resident_cycles(2, 1, 3) == g.resident_cycles(2, 1, 3)
        assert np.array_equal(h.resident_fetch(), g.resident_fetch())
        h.set_cycle("F", 1.8)
        g.set_cycle("F", 1.8)
        h.resident_load(b)
        g.resident_load(b)
        assert h.resident_cycles(1, 1, 3) == g.resident_cycles(1, 1, 3)
        assert np.array_equal(h.resident_fetch(), g.resident_fetch())


def test_the_c_entry_checks_its_factors_and_reports_what_it_built():
    A0 = sc.aniso((16, 16, 16), (1, 100, 100))
    for bad in ([(1, 1, 1)], [(1, 2, 3)], [(1, 2, 2)] * 4):          # the fourth (1, 2, 2) meets extent 2
        with pytest.raises(_hip.HipError) as e:
            _hip.Hierarchy.from_fine_semi(A0, (16, 16, 16), len(bad), bad, smoother="colour")
        assert e.value.code == _hip.ERR_INVALID
    with pytest.raises(_hip.HipError) as e:
        _hip.Hierarchy.from_fine_semi(A0, (16, 16, 16), 2, None, smoother=_hip.SMOOTH_LINE_X)
    assert e.value.code == _hip.ERR_UNSUPPORTED
    # 'auto' stops where minSize says so, and where nothing is left to coarsen
    with _hip.Hierarchy.from_fine_semi(A0, (16, 16, 16), 6, None, min_size=100, smoother="colour") as h:
        assert h.coarsening == [(1, 2, 2), (1, 2, 2)] and h.sizes == [4096, 1024, 256]      # (the third would leave 64 <= 100)
    with _hip.Hierarchy.from_fine_semi(A0, (16, 16, 16), 9, None, min_size=0, smoother="colour") as h:
        assert h.level_shapes[-1] == (2, 2, 2) and all(min(s) >= 2 for s in h.level_shapes)
        f3 = (_hip.ctypes.c_int * 3)()
        assert _hip.lib().omg_hierarchy_coarsening(h._h, len(h.coarsening), f3) == _hip.ERR_INVALID
    with _hip.Hierarchy.from_fine(operators.stencil_poisson((16, 16, 16)), (16, 16, 16), 2, smoother="colour") as h:
        assert h.coarsening is None
        assert _hip.lib().omg_hierarchy_coarsening(h._h, 0, f3) == _hip.ERR_INVALID


# ------------------------------------------------------------------------------- convergence --
@pytest.mark.parametrize("name", ["yx100", "line_yx100"])
def test_semicoarsening_converges_where_full_coarsening_stalls(name):
    """1 : 100 : 100, V(1,1) to 1e-8 ||b||: with 'auto' the device takes the oracle's count; without the key the relative
    residual after that many cycles is still above 1e-3.  (Without the feature the key is ignored and the first half fails.)

    Red-black, (16, 16, 16): 32 cycles with 'auto' (the oracle's count), 2.47e-3 ||b|| without the key after 32 (166 to 1e-8).

    Zebra lines along x, (32, 32, 32) — the table's row for this smoother (tests/semicoarsen_cases.py says why it is not the
    16^3 one: a deciding norm within 1 % of the threshold): 41 cycles with 'auto', 1.22e-3 ||b|| without the key after 41
    (193 to 1e-8), both the oracle's figures."""
    shape, c, kind, line_axis = sc.TABLE[name][:4]
    want = sc.TABLE[name][6]
    A0 = sc.aniso(shape, c)
    b = np.array(sc.rhs(A0.shape[0]))
    nb = float(np.linalg.norm(b))
    p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 400, "threshold": sc.TOL * nb,
         "giveInfo": True, "smoother": kind, "minSize": sc.MIN_SIZE}
    if kind == "line":
        p["lineAxis"] = line_axis
    u, info = openmg_amd.mgSolve(A0, b, dict(p, coarsening="auto"))
    print(name, "auto:", info["cycle"], info["norm"] / nb)
    assert info["coarsening"] == sc.TABLE[name][5]
    assert info["cycle"] == want and info["norm"] < sc.TOL * nb
    assert np.linalg.norm(b - A0 @ u) < 1.01 * sc.TOL * nb
    u_dev = openmg_amd.mgSolve(A0, b, dict(p, coarsening="auto", giveInfo=False))
    assert np.array_equal(u_dev, u)
    _, full = openmg_amd.mgSolve(A0, b, dict(p, cycles=want, threshold=0.0))
    print(name, "full after %d cycles:" % want, full["norm"] / nb)
    assert full["cycle"] == want and full["norm"] > 1e-3 * nb and "coarsening" not in full


# ------------------------------------------------------------------------------- composition --
@functools.lru_cache(maxsize=None)
def composed():
    c = hier_case("yx100", (16, 16, 16))
    return c, dict(c["p"], cycles=200, threshold=1e-8 * float(np.linalg.norm(c["b"])))


def test_with_conjugate_gradients():
    c, p = composed()
    tol = p["threshold"]
    want_norms, want_x = fcg_cpu(c["A"], c["R"], np.array(c["b"]), "colour", 1, 1, tol, 200)
    u, info = openmg_amd.mgSolve(c["A0"], c["b"], dict(p, accel="cg"))
    assert info["coarsening"] == c["host_factors"]
    assert abs(info["cycle"] - len(want_norms)) <= 1, (info["cycle"], len(want_norms))
    np.testing.assert_allclose(u, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
    assert info["norm"] <= 2 * tol
    with _hip.Hierarchy.from_fine_semi(c["A0"], c["shape"], 3, None, min_size=1, smoother="colour") as h:
        h.resident_load(c["b"])
        its, norms, tn, bd = h.resident_pcg(1, 1, 200, tol)
        assert not bd and abs(its - len(want_norms)) <= 1
        m = min(its, len(want_norms))
        np.testing.assert_allclose(norms[:m], want_norms[:m], rtol=1e-8)
    assert len(want_norms) < sc.TABLE["yx100"][6]                     # (fewer iterations than plain cycles)


def test_with_mixed_precision():
    c, p = composed()
    nb = float(np.linalg.norm(c["b"]))
    for accel in (None, "cg"):
        u, info = openmg_amd.mgSolve(c["A0"], c["b"], dict(p, dtype="mixed", accel=accel, threshold=1e-10 * nb, cycles=400))
        assert same_norm(info["norm"], c["A0"], c["b"], u, 1e-12), (accel, info["norm"], true_norm(c["A0"], c["b"], u))
        assert true_norm(c["A0"], c["b"], u) <= 1e-10 * nb and info["coarsening"] == c["host_factors"]
        u_dev = openmg_amd.mgSolve(c["A0"], c["b"], dict(p, dtype="mixed", accel=accel, threshold=1e-10 * nb, cycles=400, giveInfo=False))
        assert np.array_equal(u_dev, u)


def test_through_solver():
    c, p = composed()
    A0, b = c["A0"], np.array(c["b"])
    u, info = openmg_amd.mgSolve(A0, b, dict(p))
    for give in (False, True):
        with openmg_amd.Solver(A0, dict(p, giveInfo=give)) as s:
            assert s.hierarchy.coarsening == c["host_factors"] and s.hierarchy.level_shapes == c["host_shapes"]
            us, si = s.solve(b)
            assert np.array_equal(us, u) and si["cycle"] == info["cycle"] and si["norm"] == info["norm"]
            assert si["coarsening"] == c["host_factors"] and si["levelShapes"] == c["host_shapes"]
            again, _ = s.solve(b)
            assert np.array_equal(again, u)                             # repeats: bit for bit
            z = s.apply(b)
            want_z, _ = openmg_amd.mgCycle(c["A"], b, 0, c["R"], dict(p, coarsestLevel=len(c["R"])))
            assert np.array_equal(z, want_z)
            s.hierarchy.use_graph(True)
            graphed, gi = s.solve(b)
            s.hierarchy.use_graph(False)
            assert np.array_equal(graphed, u) and gi["norm"] == info["norm"]  # graph replay: bit for bit
            # update: the factors chosen at construction are kept (the new operator alone would choose others), a new hierarchy
            A1 = sc.aniso(c["shape"], (100, 1, 1))
            assert np.array_equal(A1.indices, A0.indices) and not s.hierarchy.can_update_fine()
            old = s.hierarchy
            s.update(A1)
            assert s.hierarchy is not old and s.hierarchy.coarsening == c["host_factors"]
            u1, _ = s.solve(b, cycles=4, threshold=0.0)
            want1, i1 = openmg_amd.mgSolve(A1, b, dict(p, coarsening=c["host_factors"], cycles=4, threshold=0.0))
            assert np.array_equal(u1, want1) and i1["coarsening"] == c["host_factors"]
        with pytest.raises(RuntimeError):
            s.solve(b)


# (PyTorch-ROCm must initialise its own copy of the HIP runtime before this package's library touches the GPU: a process of
# its own, as in tests/test_gpu_solver.py)
DEVICE_ARRAYS = """
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import openmg_amd
import semicoarsen_cases as sc
shape = (16, 16, 16)
A0 = sc.aniso(shape, (1, 100, 100))
b = np.array(sc.rhs(A0.shape[0]))
p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 5, "threshold": 0.0,
     "smoother": "colour", "minSize": 1, "coarsening": "auto"}
for kw in ({}, {"accel": "cg"}, {"dtype": "mixed"}, {"giveInfo": True}, {"smoother": "line", "lineAxis": 2}):
    uh = openmg_amd.mgSolve(A0, b, dict(p, **kw))
    ud = openmg_amd.mgSolve(A0, torch.tensor(b, device="cuda"), dict(p, **kw))
    if kw.get("giveInfo"):
        assert ud[1]["coarsening"] == uh[1]["coarsening"] == [(1, 2, 2)] * 3 and ud[1]["norm"] == uh[1]["norm"]
        uh, ud = uh[0], ud[0]
    assert isinstance(ud, torch.Tensor) and ud.is_cuda and np.array_equal(ud.cpu().numpy(), uh), kw
with openmg_amd.Solver(A0, p) as s:
    uh, ih = s.solve(b)
    ud, idv = s.solve(torch.tensor(b, device="cuda"))
    assert np.array_equal(ud.cpu().numpy(), uh) and idv == ih and ih["coarsening"] == [(1, 2, 2)] * 3
    assert np.array_equal(s.apply(torch.tensor(b, device="cuda")).cpu().numpy(), s.apply(b))
print("device arrays ok")
"""


def test_device_arrays_have_the_bits_of_the_host_calls():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "device arrays ok" in p.stdout, p.stderr[-3000:]


# --------------------------------------------------------------------------------- refusals --
def test_auto_refuses_a_27_point_operator_and_named_factors_run_it():
    shape = (8, 8, 8)
    A0 = operators.stencil27_variable(shape)
    b = A0 @ np.random.default_rng(3).random(A0.shape[0])
    p = {"problemShape": shape, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "cycles": 5, "threshold": 0.0,
         "smoother": "colour", "minSize": 1}
    for give in (False, True):
        with pytest.raises(_hip.HipError) as e:
            openmg_amd.mgSolve(A0, b, dict(p, coarsening="auto", giveInfo=give))
        assert e.value.code == _hip.ERR_UNSUPPORTED and "level 0" in str(e.value), str(e.value)
    named = [(1, 2, 2), (2, 1, 1)]
    u, info = openmg_amd.mgSolve(A0, b, dict(p, coarsening=named, giveInfo=True))
    assert info["coarsening"] == named and info["levelShapes"] == [(8, 8, 8), (8, 4, 4), (4, 4, 4)]
    u_dev = openmg_amd.mgSolve(A0, b, dict(p, coarsening=named))
    assert np.array_equal(u_dev, u)
    pr = {"A": info["A"], "R": info["R"], "b": b, "sm": orc.make_smoother("colour", info["A"])}
    want_norms, want_x = restated_cycles(pr, "V", 1.0, 1, 1, 5)
    assert norms_agree([info["norm"]], [want_norms[-1]], norm_floor(A0, b, want_x)) and np.allclose(u, want_x, **CYC)


def test_the_multi_gpu_entries_refuse_the_key():
    from openmg_amd import dist
    with pytest.raises(ValueError, match="multi-GPU"):
        dist.build_all_ranks(None, None, coarsening="auto")
    with pytest.raises(ValueError, match="multi-GPU"):
        dist.make_tail(None, (8, 8, 8), 2, coarsening=[(1, 2, 2)])


def test_full_is_the_call_without_the_key():
    shape = (32, 32, 32)
    A0 = operators.stencil_poisson(shape)
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    for give in (False, True):
        p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0.0,
             "smoother": "colour", "giveInfo": give}
        r0, r1, r2 = (openmg_amd.mgSolve(A0, b, dict(p, **kw)) for kw in ({}, {"coarsening": "full"}, {"coarsening": None}))
        if give:
            assert r0[1]["norm"] == r1[1]["norm"] == r2[1]["norm"] and "coarsening" not in r1[1]
            r0, r1, r2 = r0[0], r1[0], r2[0]
        assert np.array_equal(r0, r1) and np.array_equal(r0, r2)
