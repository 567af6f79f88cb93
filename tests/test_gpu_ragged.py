"""Grids of any extent on the device (parameters['oddExtents'] = 'merge'; omg_restriction_ragged,
omg_hierarchy_create_from_fine_ragged) against NumPy, SciPy and the oracle (tests/ragged_cases.py).

Gates: restriction matrices exactly; the two setup routes, repeats, Solver against mgSolve and "nothing changes where nothing
is odd" bit for bit; cycle counts equal to the oracle's and every cycle's norm to 1e-10 relative (the project's parity
bound); the other comparisons at the gates tests/test_gpu_semicoarsen.py uses for the same kind (norms_agree / CYC /
norm_floor of tests/test_gpu_cycle_shapes.py for fp64 cycles, 1e-3 above the fp32 floor for fp32, tests/test_gpu_pcg.py's for
FCG, tests/test_gpu_mixed.py's same_norm).  Needs an MI355X: run with -m gpu."""
import ctypes
import functools
import hashlib
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

import ragged_cases as rc
import semicoarsen_cases as sc
from test_gpu_cycle_shapes import CYC, norm_floor, norms_agree, restated_cycles
from test_gpu_mixed import same_norm, true_norm
from test_gpu_pcg import fcg_cpu

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
U64 = 2.0 ** -53
SHAPES = [(4, 5), (5, 4), (7, 9), (13, 10), (5, 5, 5), (4, 6, 7), (9, 14, 21), (5, 7, 11)]


def factor_tuples(shape):
    """every tuple with at least one 2, a 2 only on an axis that can take it (extent >= 4) — also those that leave an odd axis at 1"""
    return [f for f in itertools.product((1, 2), repeat=len(shape)) if any(v == 2 for v in f) and all(v == 1 or e >= 4 for e, v in zip(shape, f))]


def same_csr(got, want):
    return (got.shape == want.shape and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            and np.array_equal(got.data, want.data))


def base(shape, levels=3, **kw):
    p = {"problemShape": shape, "gridLevels": levels, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0.0,
         "smoother": "colour", "minSize": rc.MIN_SIZE, "oddExtents": "merge"}
    p.update(kw)
    return p


# ------------------------------------------------------------------------------- restriction --
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restriction_ragged_is_the_yardsticks_matrix(shape):
    tuples = factor_tuples(shape)
    assert len(tuples) == 2 ** len(shape) - 1                       # (every extent of these shapes is >= 4)
    for f in tuples:
        want = rc.aggregation(shape, f)
        assert same_csr(_hip.restriction_ex(shape, f, "merge"), want), f
        assert same_csr(operators.restriction(shape, factors=f, oddExtents="merge"), want), f
    assert any(np.diff(rc.aggregation(shape, f).indptr).max() > np.prod(f) for f in tuples) == any(e % 2 for e in shape)


@pytest.mark.parametrize("shape", [(8, 12, 20), (4, 6, 8), (6, 10)], ids=lambda s: "x".join(map(str, s)))
def test_on_even_shapes_it_is_restriction_ex(shape):
    for f in factor_tuples(shape):
        assert same_csr(_hip.restriction_ex(shape, f, "merge"), _hip.restriction_ex(shape, f)), f
        assert same_csr(_hip.restriction_ex(shape, f, None), sc.aggregation(shape, f)), f


def test_restriction_ragged_refusals_leave_the_process_usable():
    def code_of(shape, f, odd):
        dim = len(shape)
        n = int(np.prod(shape))
        indptr, indices, data = np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
        return _hip.lib().omg_restriction_ragged(dim, (ctypes.c_int64 * dim)(*shape), (ctypes.c_int * dim)(*f), odd, indptr.ctypes.data,
                                                 indices.ctypes.data, data.ctypes.data)
    for shape, f in (((8, 12, 3), (1, 1, 2)), ((3, 9), (2, 1)), ((9, 9, 9), (1, 1, 1)), ((9, 9), (1, 1)), ((9, 9, 9), (3, 1, 1)),
                     ((9, 9, 9), (0, 2, 2)), ((9, 9, 2), (2, 2, 2))):
        assert code_of(shape, f, _hip.ODD_MERGE) == _hip.ERR_INVALID, (shape, f)
        with pytest.raises(_hip.HipError) as e:
            _hip.restriction_ex(shape, f, "merge")
        assert e.value.code == _hip.ERR_INVALID
    assert code_of((9, 9, 9), (2, 2, 2), _hip.ODD_REFUSE) == _hip.ERR_INVALID      # without the flag an odd extent is refused
    assert code_of((9, 9, 9), (2, 2, 2), 2) == _hip.ERR_INVALID                    # a flag that is neither
    assert code_of((9, 9, 9), (2, 2, 2), _hip.ODD_MERGE) == _hip.OMG_OK
    with pytest.raises(_hip.HipError):
        _hip.restriction_ex((9, 9, 9), (2, 2, 2))
    assert same_csr(_hip.restriction_ex((4, 5), (2, 2), "merge"), rc.aggregation((4, 5), (2, 2)))


# ------------------------------------------------------------------------------ Galerkin lists --
def var7(shape):
    return sp.csr_matrix(operators.stencil7_variable(shape))


LISTS = [
    ("iso box", (9, 14, 21), lambda s: sc.aniso(s, (1, 1, 1)), None),
    ("iso cube", (15, 15, 15), lambda s: sc.aniso(s, (1, 1, 1)), "full"),
    ("yx100 auto", (15, 15, 15), lambda s: sc.aniso(s, (1, 100, 100)), "auto"),
    ("var7 box", (9, 14, 21), var7, None),
    ("var7 auto", (9, 14, 21), var7, "auto"),
    ("square", (13, 10), lambda s: sc.aniso(s, (1, 1)), None),
    ("named, an odd axis left at 1", (9, 14, 21), lambda s: sc.aniso(s, (1, 1, 1)), [(1, 2, 2), (2, 1, 2), (2, 2, 1)]),
    ("27-point (the SpGEMM pair)", (7, 9, 11), lambda s: sp.csr_matrix(operators.stencil27_variable(s)), None),
]


@pytest.mark.parametrize("name,shape,make,coarsening", LISTS, ids=[c[0] for c in LISTS])
def test_galerkin_lists_against_scipy(name, shape, make, coarsening):
    """R exactly; A: the yardstick's pattern, and every value to the rounding of a sum of at most 27 * 27 products taken in
    another order: 2 * 729 u (|R| |A| |R|^T) entry by entry (the device follows SciPy's order, so they are in fact equal —
    printed)."""
    A0 = make(shape)
    R, A, factors = operators.semicoarsenedLists(A0, shape, coarsening, 2, rc.MIN_SIZE, oddExtents="merge")
    yard = "full" if coarsening is None else coarsening
    wA, wR, wf, wshapes = rc.lists(A0, shape, yard, 3, min_size=rc.MIN_SIZE)
    assert factors == wf and len(R) == len(wR) and len(A) == len(wA)
    assert [M.shape[0] for M in A] == [int(np.prod(s)) for s in wshapes]
    for Rl, want in zip(R, wR):
        assert same_csr(Rl, want)
    for l, (Al, want) in enumerate(zip(A[1:], wA[1:])):
        Al = sp.csr_matrix(Al)
        Al.sort_indices()
        assert np.array_equal(Al.indptr, want.indptr) and np.array_equal(Al.indices, want.indices), (name, l)
        rows = np.repeat(np.arange(want.shape[0]), np.diff(want.indptr))
        bound = np.asarray(sp.csr_matrix(abs(wR[l]) @ abs(wA[l]) @ abs(wR[l]).T)[rows, want.indices]).ravel()
        print(name, l + 1, "equal bits:", np.array_equal(Al.data, want.data), "max diff / bound %.2e" % (np.abs(Al.data - want.data) / bound).max())
        assert np.all(np.abs(Al.data - want.data) <= 2 * 729 * U64 * bound), (name, l)


# ------------------------------------------------------------------------------------ routes --
ROUTES = [
    ("yx100 auto", (15, 15, 15), lambda s: sc.aniso(s, (1, 100, 100)), "auto", "float64"),
    ("yx100 full", (15, 15, 15), lambda s: sc.aniso(s, (1, 100, 100)), "full", "float64"),
    ("iso17 full f32", (17, 17, 17), lambda s: sc.aniso(s, (1, 1, 1)), None, "float32"),
    ("var7 auto", (9, 14, 21), var7, "auto", "float64"),
    ("var7 full", (9, 14, 21), var7, None, "float64"),
    ("square full", (13, 10), lambda s: sc.aniso(s, (1, 1)), None, "float64"),
    ("box named", (9, 14, 21), lambda s: sc.aniso(s, (1, 10, 10)), [(1, 2, 2), (2, 1, 2), (2, 2, 1)], "float64"),
]


ROUTE_BITS = {}       # name -> the iterate with the fused Galerkin kernel: the SpGEMM pair must give the same


@pytest.mark.parametrize("fused_product", ["1", "0"], ids=["rap_aggregation", "spgemm pair"])
@pytest.mark.parametrize("name,shape,make,coarsening,dtype", ROUTES, ids=[r[0] for r in ROUTES])
def test_device_route_gives_the_hierarchy_of_the_lists_route(monkeypatch, name, shape, make, coarsening, dtype, fused_product):
    """Same factors, same level shapes, the iterate and the norms of three cycles bit for bit — with the fused Galerkin kernel
    (it takes a ragged R as it is: full cover, R.nnz == n, 27 members x 7 entries within its hash capacity) and with the two
    sparse products it falls back to."""
    monkeypatch.setenv("OMG_RAP_FUSED", fused_product)
    A0 = make(shape)
    b = A0 @ np.random.default_rng(5).random(A0.shape[0])
    p = base(shape, dtype=dtype, coarsening=coarsening)
    pa, pb = dict(p), dict(p, giveInfo=True)
    x_dev = openmg_amd.mgSolve(A0, b, pa)                             # the device route (giveInfo off)
    x_host, info = openmg_amd.mgSolve(A0, b, pb)                      # the lists route
    assert pa["coarsestLevel"] == pb["coarsestLevel"] == len(info["R"]) == len(info["coarsening"])
    assert np.array_equal(x_dev, x_host), (name, int(np.sum(x_dev != x_host)))
    assert np.array_equal(ROUTE_BITS.setdefault(name, x_host), x_host)
    yard = "full" if coarsening is None else coarsening
    want = rc.lists(A0, shape, yard, 3, min_size=rc.MIN_SIZE)
    assert info["coarsening"] == want[2] and info["levelShapes"] == want[3]
    named = None if coarsening == "auto" else info["coarsening"]
    with _hip.Hierarchy.from_fine_semi(A0, shape, 3 if named is None else len(named), named, min_size=rc.MIN_SIZE, smoother="colour",
                                       dtype=dtype, oddExtents="merge") as h, \
            _hip.Hierarchy(info["A"], info["R"], smoother="colour", dtype=dtype) as g:
        assert h.sizes == g.sizes == [M.shape[0] for M in info["A"]]
        assert h.coarsening == info["coarsening"] and h.level_shapes == info["levelShapes"] and h.odd_extents == "merge"
        assert not h.can_update_fine()
        assert [h.level_flags(l) for l in range(len(info["R"]))] == [g.level_flags(l) for l in range(len(info["R"]))]
        h.resident_load(b)
        g.resident_load(b)
        assert h.resident_norms() == g.resident_norms()
        assert h.resident_cycles(1, 1, 3) == g.resident_cycles(1, 1, 3)
        assert np.array_equal(h.resident_fetch(), g.resident_fetch())
        if dtype == "float64":
            assert np.array_equal(h.resident_fetch(), x_host)


def test_the_c_entry_checks_its_factors_and_reports_what_it_built():
    A0 = sc.aniso((15, 15, 15), (1, 1, 1))
    for bad in ([(1, 1, 1)], [(1, 2, 3)], [(2, 2, 2)] * 3):              # the third (2, 2, 2) meets extent 3
        with pytest.raises(_hip.HipError) as e:
            _hip.Hierarchy.from_fine_semi(A0, (15, 15, 15), len(bad), bad, smoother="colour", oddExtents="merge")
        assert e.value.code == _hip.ERR_INVALID
    with pytest.raises(_hip.HipError) as e:                              # without the flag: today's refusal
        _hip.Hierarchy.from_fine_semi(A0, (15, 15, 15), 1, [(2, 2, 2)], smoother="colour")
    assert e.value.code == _hip.ERR_INVALID and "even extent" in str(e.value)
    with pytest.raises(_hip.HipError) as e:                              # 'auto' without the flag: no axis of 15^3 is eligible
        _hip.Hierarchy.from_fine_semi(A0, (15, 15, 15), 2, None, smoother="colour")
    assert e.value.code == _hip.ERR_INVALID
    v, opt, out = _hip.csr_view(A0), _hip.HierarchyOptions(_hip.smoother_code("colour"), 1.0, _hip.DTYPE_F64, 0), ctypes.c_void_p()
    assert _hip.lib().omg_hierarchy_create_from_fine_ragged(ctypes.byref(v), 3, (ctypes.c_int64 * 3)(15, 15, 15), 2, None, 0, 2,
                                                            ctypes.byref(opt), ctypes.byref(out)) == _hip.ERR_INVALID and not out.value
    # 'auto' ends where nothing is left to coarsen, and where minSize says so
    with _hip.Hierarchy.from_fine_semi(A0, (15, 15, 15), 9, None, min_size=0, smoother="colour", oddExtents="merge") as h:
        assert h.coarsening == [(2, 2, 2)] * 2 and h.level_shapes == [(15,) * 3, (7,) * 3, (3,) * 3] and h.sizes == [3375, 343, 27]
        f3 = (ctypes.c_int * 3)()
        assert _hip.lib().omg_hierarchy_coarsening(h._h, 1, f3) == _hip.OMG_OK and tuple(f3) == (2, 2, 2)
        assert _hip.lib().omg_hierarchy_coarsening(h._h, 2, f3) == _hip.ERR_INVALID
    with _hip.Hierarchy.from_fine_semi(A0, (15, 15, 15), 9, None, min_size=27, smoother="colour", oddExtents="merge") as h:
        assert h.sizes == [3375, 343]                                    # (the second restriction would leave 27 <= 27)


# ------------------------------------------------------------------------------ oracle parity --
@pytest.mark.parametrize("name", sorted(rc.TABLE))
def test_oracle_parity_on_every_table_row(name):
    """mgSolve to 1e-8 ||b||: the oracle's cycle count, and every cycle's norm (Solver reports them all; its bits are
    mgSolve's) within 1e-10 relative of the oracle's — the project's parity gate, norms_agree: 1e-10 relative beyond what
    norm_floor says fp64 itself leaves open in ||b - A x|| (the last cycles stand at 1e-8 ||b||, where two correct
    evaluations of the residual in another order differ by more than 1e-10 of it).

    Measured on an MI355X, the plain relative difference |device - oracle| / oracle: over the first half of each row's
    cycles at most 2.6e-12 (line_x100), 1e-12 and less on the other rows; over all cycles 4.5e-10 (iso15), 6.5e-10 (box9),
    9.0e-10 (iso17), 9.4e-10 (auto_yx100), 1.3e-9 (box5), 1.5e-9 (line_x100), 2.9e-9 (neumann_box9), 5.9e-9 (sq13), each in
    one of the last three cycles, where norm_floor allows 1e-6 to 8e-6 of the norm; the iterates agree to 1.5e-16 … 1.2e-15
    of their largest entry.  A bare 1e-10 on every cycle would fail on those last cycles on every row."""
    c = rc.case(name)
    shape, kind, neumann = c["shape"], c["kind"], c["neumann"]
    b = np.array(c["b"])
    nb = float(np.linalg.norm(b))
    p = base(shape, c["restrictions"], cycles=400, threshold=rc.TOL * nb, giveInfo=True, smoother=kind,
             coarsening=None if c["coarsening"] == "full" else c["coarsening"], nullspace="constant" if neumann else None)
    if kind == "line":
        p["lineAxis"] = c["line_axis"]
    u, info = openmg_amd.mgSolve(c["A0"], b, dict(p))
    assert info["coarsening"] == c["factors"] == rc.TABLE[name][7] and info["levelShapes"] == c["shapes"]
    for Rl, want in zip(info["R"], c["R"]):
        assert same_csr(Rl, want)
    with openmg_amd.Solver(c["A0"], dict(p)) as s:
        us, si = s.solve(b)
    rel = [abs(a - w) / w for a, w in zip(si["norms"], c["norms"])]
    worst = max(rel)
    floor = norm_floor(c["A0"], b, c["x"])
    print(name, "cycles", info["cycle"], "oracle", c["cycles"], "worst norm rel diff %.2e (cycle %d), over the first half %.2e, floor / last norm %.2e"
          % (worst, 1 + rel.index(worst), max(rel[:max(1, len(rel) // 2)]), floor / c["norms"][-1]),
          "iterate diff %.2e" % (np.abs(u - c["x"]).max() / np.abs(c["x"]).max()))
    assert info["cycle"] == c["cycles"] == rc.TABLE[name][9] and info["norm"] < rc.TOL * nb
    assert np.array_equal(us, u) and si["cycle"] == info["cycle"] and si["norm"] == info["norm"] and len(si["norms"]) == c["cycles"]
    assert norms_agree(si["norms"], c["norms"], floor), worst
    assert np.linalg.norm(b - c["A0"] @ u) < 1.01 * rc.TOL * nb
    u_dev = openmg_amd.mgSolve(c["A0"], b, dict(p, giveInfo=False))
    assert np.array_equal(u_dev, u)


# ------------------------------------------------------------------------------- composition --
@functools.lru_cache(maxsize=None)
def box():
    """(9, 14, 21), isotropic, 'full' with 'merge': the yardstick's lists and ONE mgSolve whose lists are theirs"""
    shape = (9, 14, 21)
    A0 = sc.aniso(shape, (1, 1, 1))
    A, R, factors, shapes = rc.lists(A0, shape, "full", 3, min_size=rc.MIN_SIZE)
    return {"shape": shape, "A0": A0, "A": A, "R": R, "factors": factors, "shapes": shapes, "b": rc.rhs_of(A0.shape[0])}


@pytest.mark.parametrize("kind", ["gs", "jacobi", "colour", "line"])
@pytest.mark.parametrize("cycle,alpha", [("V", 1.0), ("F", 1.8)])
def test_with_every_smoother_and_an_f_cycle(kind, cycle, alpha):
    c = box()
    b = np.array(c["b"])
    sm = sc.make_zebra(c["A"], c["shapes"], 2) if kind == "line" else orc.make_smoother(kind, c["A"])
    want_norms, want_x = restated_cycles({"A": c["A"], "R": c["R"], "b": b, "sm": sm}, cycle, alpha, 1, 1, 5)
    p = base(c["shape"], cycles=5, giveInfo=True, smoother=kind, cycle=cycle, overCorrection=alpha)
    if kind == "line":
        p["lineAxis"] = 2
    u, info = openmg_amd.mgSolve(c["A0"], b, dict(p))
    print(kind, cycle, alpha, "norm rel diff %.2e iterate diff %.2e" % (abs(info["norm"] - want_norms[-1]) / want_norms[-1], np.abs(u - want_x).max()))
    assert info["coarsening"] == c["factors"] and info["levelShapes"] == c["shapes"]
    assert norms_agree([info["norm"]], [want_norms[-1]], norm_floor(c["A0"], b, want_x)) and np.allclose(u, want_x, **CYC)
    assert np.array_equal(openmg_amd.mgSolve(c["A0"], b, dict(p, giveInfo=False)), u)


def test_with_float32_levels():
    c = box()
    b = np.array(c["b"])
    pr = {"A": c["A"], "R": c["R"], "b": b, "sm": orc.make_smoother("colour", c["A"])}
    want_norms, want_x = restated_cycles(pr, "V", 1.0, 1, 1, 5, dtype=np.float32)
    u, info = openmg_amd.mgSolve(c["A0"], b, base(c["shape"], cycles=5, giveInfo=True, dtype="float32"))
    floor = 64 * EPS32 * float(abs(c["A0"]).sum(axis=1).max()) * np.abs(want_x).max() * np.sqrt(b.size)
    assert abs(info["norm"] - want_norms[-1]) <= 1e-3 * want_norms[-1] + floor
    assert np.abs(u - want_x).max() <= 1e-3 * np.abs(want_x).max()
    assert np.array_equal(openmg_amd.mgSolve(c["A0"], b, base(c["shape"], cycles=5, dtype="float32")), u)


def test_with_conjugate_gradients_and_mixed_precision():
    c = box()
    b = np.array(c["b"])
    nb = float(np.linalg.norm(b))
    tol = 1e-8 * nb
    want_norms, want_x = fcg_cpu(c["A"], c["R"], b, "colour", 1, 1, tol, 200)
    u, info = openmg_amd.mgSolve(c["A0"], b, base(c["shape"], cycles=200, threshold=tol, giveInfo=True, accel="cg"))
    assert info["coarsening"] == c["factors"]
    assert abs(info["cycle"] - len(want_norms)) <= 1, (info["cycle"], len(want_norms))
    np.testing.assert_allclose(u, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
    assert info["norm"] <= 2 * tol and len(want_norms) < rc.TABLE["box9"][9]
    for accel in (None, "cg"):
        p = base(c["shape"], cycles=400, threshold=1e-10 * nb, giveInfo=True, dtype="mixed", accel=accel)
        u, info = openmg_amd.mgSolve(c["A0"], b, dict(p))
        assert same_norm(info["norm"], c["A0"], b, u, 1e-12), (accel, info["norm"], true_norm(c["A0"], b, u))
        assert true_norm(c["A0"], b, u) <= 1e-10 * nb and info["coarsening"] == c["factors"]
        assert np.array_equal(openmg_amd.mgSolve(c["A0"], b, dict(p, giveInfo=False)), u)


def test_through_solver():
    c = box()
    A0, b = c["A0"], np.array(c["b"])
    nb = float(np.linalg.norm(b))
    p = base(c["shape"], cycles=200, threshold=1e-8 * nb, giveInfo=True)
    u, info = openmg_amd.mgSolve(A0, b, dict(p))
    assert info["cycle"] == rc.TABLE["box9"][9]
    for give in (False, True):
        with openmg_amd.Solver(A0, dict(p, giveInfo=give)) as s:
            assert s.hierarchy.coarsening == c["factors"] and s.hierarchy.level_shapes == c["shapes"] and s.hierarchy.odd_extents == "merge"
            us, si = s.solve(b)
            assert np.array_equal(us, u) and si["cycle"] == info["cycle"] and si["norm"] == info["norm"]
            assert si["coarsening"] == c["factors"] and si["levelShapes"] == c["shapes"]
            again, _ = s.solve(b)
            assert np.array_equal(again, u)                             # repeats: bit for bit
            # warm start: from the solution of a nearby right-hand side fewer cycles, and the same answer to the tolerance
            b2 = b + 1e-3 * np.array(sc.rhs(b.size))[::-1]
            cold, ci = s.solve(b2, threshold=1e-8 * np.linalg.norm(b2))
            warm, wi = s.solve(b2, initial=u, threshold=1e-8 * np.linalg.norm(b2))
            assert 0 < wi["cycle"] < ci["cycle"] and wi["norm"] < 1e-8 * np.linalg.norm(b2)
            assert np.linalg.norm(b2 - A0 @ warm) < 1.01e-8 * np.linalg.norm(b2)
            z = s.apply(b)
            want_z, _ = openmg_amd.mgCycle(info["A"], b, 0, info["R"], dict(p, coarsestLevel=len(info["R"])))
            assert np.array_equal(z, want_z)
            # update: the factors and the key are kept, a new hierarchy
            A1 = sc.aniso(c["shape"], (100, 1, 1))
            assert np.array_equal(A1.indices, A0.indices) and not s.hierarchy.can_update_fine()
            old = s.hierarchy
            s.update(A1)
            assert s.hierarchy is not old and s.hierarchy.coarsening == c["factors"] and s.hierarchy.odd_extents == "merge"
            u1, _ = s.solve(b, cycles=4, threshold=0.0)
            want1, i1 = openmg_amd.mgSolve(A1, b, dict(p, cycles=4, threshold=0.0, giveInfo=True))
            assert np.array_equal(u1, want1) and i1["coarsening"] == c["factors"]
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
shape = (9, 14, 21)
A0 = sc.aniso(shape, (1, 1, 1))
b = np.array(sc.rhs(A0.shape[0]))
want = [(2, 2, 2), (2, 2, 2), (1, 1, 2)]
p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 5, "threshold": 0.0,
     "smoother": "colour", "minSize": 1, "oddExtents": "merge"}
for kw in ({}, {"accel": "cg"}, {"dtype": "mixed"}, {"giveInfo": True}, {"coarsening": "auto"}, {"smoother": "line", "lineAxis": 2}):
    uh = openmg_amd.mgSolve(A0, b, dict(p, **kw))
    ud = openmg_amd.mgSolve(A0, torch.tensor(b, device="cuda"), dict(p, **kw))
    if kw.get("giveInfo"):
        assert ud[1]["coarsening"] == uh[1]["coarsening"] == want and ud[1]["norm"] == uh[1]["norm"]
        uh, ud = uh[0], ud[0]
    assert isinstance(ud, torch.Tensor) and ud.is_cuda and np.array_equal(ud.cpu().numpy(), uh), kw
with openmg_amd.Solver(A0, p) as s:
    uh, ih = s.solve(b)
    ud, idv = s.solve(torch.tensor(b, device="cuda"))
    assert np.array_equal(ud.cpu().numpy(), uh) and idv == ih and ih["coarsening"] == want
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


# ------------------------------------------------------- nothing changes where nothing is odd --
@pytest.mark.parametrize("name,levels", [("iso16", 3), ("box_yx10", 2), ("box_z100x10", 3)])
def test_auto_on_even_grids_is_auto_without_the_key(name, levels):
    """Rows of tests/semicoarsen_cases.py whose level grids are all even as far as they are coarsened here.  box_yx10 runs
    (8, 12, 20) -> (8, 6, 10) -> (8, 3, 5): that far nothing is odd, and two restrictions are compared.  Its THIRD restriction
    acts on (8, 3, 5), where the extent 5 is eligible with 'merge' and the stronger coupled: the rule then picks (1, 1, 2) where
    it picks (2, 1, 1) without the key (the yardstick's lists say the same), so that restriction is no case of this test."""
    shape, c = sc.TABLE[name][:2]
    A0 = sc.aniso(shape, c)
    b = np.array(sc.rhs(A0.shape[0]))
    p = base(shape, levels, coarsening="auto")
    del p["oddExtents"]
    assert rc.lists(A0, shape, "auto", levels, min_size=rc.MIN_SIZE)[2] == sc.TABLE[name][5][:levels]
    if name == "box_yx10":
        assert rc.lists(A0, shape, "auto", 3, min_size=rc.MIN_SIZE)[2] == [(1, 2, 2), (1, 2, 2), (1, 1, 2)]
    for give in (False, True):
        r0 = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=give))
        r1 = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=give, oddExtents="merge"))
        r2 = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=give, oddExtents=None))
        if give:
            assert r0[1]["coarsening"] == r1[1]["coarsening"] == sc.TABLE[name][5][:levels] and r0[1]["norm"] == r1[1]["norm"] == r2[1]["norm"]
            assert r0[1]["levelShapes"] == r1[1]["levelShapes"]
            r0, r1, r2 = r0[0], r1[0], r2[0]
        assert np.array_equal(r0, r1) and np.array_equal(r0, r2)


def test_full_on_a_power_of_two_cube_is_todays_full():
    shape = (16, 16, 16)
    A0 = operators.stencil_poisson(shape)
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    for levels in (2, 3):
        for give in (False, True):
            p = base(shape, levels, giveInfo=give)
            del p["oddExtents"]
            r0 = openmg_amd.mgSolve(A0, b, dict(p))
            r1 = openmg_amd.mgSolve(A0, b, dict(p, oddExtents="merge"))
            r2 = openmg_amd.mgSolve(A0, b, dict(p, oddExtents="merge", coarsening="full"))
            if give:
                assert "coarsening" not in r0[1] and r1[1]["coarsening"] == r2[1]["coarsening"] == [(2, 2, 2)] * levels
                assert r0[1]["norm"] == r1[1]["norm"] == r2[1]["norm"]
                for M0, M1 in zip(r0[1]["A"] + r0[1]["R"], r1[1]["A"] + r1[1]["R"]):
                    assert same_csr(sp.csr_matrix(M0), sp.csr_matrix(M1))
                r0, r1, r2 = r0[0], r1[0], r2[0]
            assert np.array_equal(r0, r1) and np.array_equal(r0, r2), (levels, give)


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


# Recorded on an MI355X with the library of the commit before 'oddExtents' existed (three V(1,1) cycles, 'colour', fp64,
# giveInfo on / off the same): the residual norm as float.hex() and the SHA-256 of the iterate's bytes.
PARENT_BITS = {
    "full": ("0x1.bcf1f4a714255p+0", "fdeabcbb96be29091bfc6e1beb4ad2f5d7900dbf48e8e3f1c0fb8bfa0c6824df"),
    "auto": ("0x1.4a0d4dbc29df4p+0", "319ec206c84c0829b299992ab2616cabf017a39ca7c8af08e4b122bc3202f01f"),
}


@pytest.mark.parametrize("which", ["full", "auto"])
def test_without_the_key_the_parent_builds_bits(which):
    """The default path (poisson 32^3, 4 grids: the device route's fused passes) and a semicoarsened one ((16, 16, 16),
    1 : 100 : 100, 'auto': omg_hierarchy_create_from_fine_semi, now a call of the ragged entry with OMG_ODD_REFUSE)."""
    if which == "full":
        shape = (32, 32, 32)
        A0 = operators.stencil_poisson(shape)
        b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
        p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0.0, "smoother": "colour"}
    else:
        shape = (16, 16, 16)
        A0 = sc.aniso(shape, (1, 100, 100))
        b = np.array(sc.rhs(A0.shape[0]))
        p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0.0, "smoother": "colour",
             "minSize": 1, "coarsening": "auto"}
    u, info = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=True))
    u_dev = openmg_amd.mgSolve(A0, b, dict(p))
    print(which, float(info["norm"]).hex(), digest(u), digest(u_dev))
    assert (float(info["norm"]).hex(), digest(u)) == PARENT_BITS[which] and digest(u_dev) == PARENT_BITS[which][1]


# ------------------------------------------------------------------------ fused levels survive --
def test_even_levels_above_a_ragged_one_keep_their_fused_passes():
    """Constant-coefficient (20, 20, 20) runs 20 -> 10 -> 5 -> 2: levels 0 and 1 restrict by the even 2^3 aggregation and carry
    the flags they have in the two-restriction hierarchy without the key; level 2 (5^3 -> 2^3, three-cell aggregates) carries
    none of the pass flags and runs the set-by-set row kernels."""
    shape = (20, 20, 20)
    A0 = operators.stencil_poisson(shape)
    named = operators.coarseningOf(None, shape, 2, rc.MIN_SIZE, "merge")
    assert named == [(2, 2, 2)] * 3

    def raw(h, l):
        f = ctypes.c_int(0)
        _hip.check(_hip.lib().omg_hierarchy_level_flags(h._h, l, ctypes.byref(f)))
        return f.value
    with _hip.Hierarchy.from_fine_semi(A0, shape, 3, named, min_size=rc.MIN_SIZE, smoother="colour", oddExtents="merge") as h, \
            _hip.Hierarchy.from_fine(A0, shape, 2, smoother="colour") as g:
        assert h.level_shapes == [(20,) * 3, (10,) * 3, (5,) * 3, (2,) * 3] and g.sizes == h.sizes[:3]
        print("flags with the key", [raw(h, l) for l in range(3)], "without", [raw(g, l) for l in range(2)])
        for l in (0, 1):
            assert raw(h, l) == raw(g, l) and h.level_flags(l)["plane"]
        last = h.level_flags(2)
        assert not (last["plane"] or last["var7"] or last["stencil27"])
    # the same through mgSolve, against the oracle on the lists it hands back
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    u, info = openmg_amd.mgSolve(A0, b, base(shape, cycles=5, giveInfo=True))
    assert info["levelShapes"] == [(20,) * 3, (10,) * 3, (5,) * 3, (2,) * 3]
    pr = {"A": info["A"], "R": info["R"], "b": b, "sm": orc.make_smoother("colour", info["A"])}
    want_norms, want_x = restated_cycles(pr, "V", 1.0, 1, 1, 5)
    assert norms_agree([info["norm"]], [want_norms[-1]], norm_floor(A0, b, want_x)) and np.allclose(u, want_x, **CYC)
    assert np.array_equal(openmg_amd.mgSolve(A0, b, base(shape, cycles=5)), u)


# ------------------------------------------------------------------------------------- memory --
def test_destroying_a_ragged_hierarchy_gives_its_memory_back():
    """Free device memory after create / destroy is what it was: four rounds leave less than half of ONE hierarchy's
    footprint behind (a hierarchy leaked per round would leave four)."""
    shape = (41, 41, 41)
    A0 = sc.aniso(shape, (1, 1, 1))
    b = np.array(sc.rhs(A0.shape[0]))

    def run(probe=False):
        with _hip.Hierarchy.from_fine_semi(A0, shape, 4, None, min_size=rc.MIN_SIZE, smoother="colour", oddExtents="merge") as h:
            assert h.level_shapes[1:] == [(20,) * 3, (10,) * 3, (5,) * 3, (2,) * 3]
            h.resident_load(b)
            h.resident_cycles(1, 1, 2)
            return _hip.device_mem_info()[0] if probe else None
    run()                                                             # (code object, streams, caches: allocated once)
    free0 = _hip.device_mem_info()[0]
    during = run(probe=True)
    footprint = free0 - during
    for _ in range(4):
        run()
    free1 = _hip.device_mem_info()[0]
    print("footprint", footprint, "left behind", free0 - free1)
    assert footprint > 0 and free0 - free1 < footprint // 2, (free0, during, free1)
