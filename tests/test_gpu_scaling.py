"""Every solve path under power-of-two rescaling, and the numerators at the edges of plane.hip's quotients().

Multiplying by 2^k is exact while nothing under- or overflows, so for a kernel that computes the schedule's algorithm
with no hidden absolute constant, cycle(2^ka A, 2^kb b) has the BITS of 2^(kb - ka) cycle(A, b) and every norm is 2^kb
times the unscaled one.  tests/test_scaling_host.py pins that the CPU oracle has this property for every family,
smoother and pair used here; the device is then compared with ITSELF: the same calls on (A, b, x0) and on
(s A, t b, (t / s) x0), iterates as bits (the sign of a zero counts), norms with ==.

Pairs (ka, kb), fp64 hierarchies: (0, 0), (40, -60), (-300, 0), (0, 300), and ka = kb = k with k chosen from the fine
operator's diagonal c3 so that |c3| 2^k lies just inside and just outside 2^400 and 2^-400 (plane.hip fast_div; for the
Poisson diagonal 6 = 1.5 * 2^2 that is 397 / 398 and -402 / -403).  fp32 hierarchies: (24, -24) and (-30, 30) only — a
subnormal float is rounded, which breaks exactness legitimately.  s = t = -1 (negation is exact) on the cycle and
coarse-solve cases; not on FCG, which requires (p, q) > 0 by design.  Mixed hierarchies: the operator is stored as
float, so ka stays small, and kb goes to +-400.

Exemptions (a pair the reference itself is not bitwise for): none — tests/test_scaling_host.py passes every pair.

Every path is selected the way the tests of that path select it and asserts its level_flags / plane_info, so that a case
cannot silently run another kernel."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import scaling_cases as sc

pytestmark = pytest.mark.gpu


# ---- the paths ----------------------------------------------------------------------------------------------------
def planes(levels):
    def check(h, case, s=1.0):
        for l in range(levels):
            assert h.level_flags(l)["plane"], (case["family"], l, h.level_flags(l))
        info = h.plane_info(0)
        shape = case["family"][1]
        assert tuple(info[k] for k in ("nz", "ny", "nx")[3 - len(shape):]) == tuple(shape), info
    return check


def flag(name, levels=1, absent=()):
    def check(h, case, s=1.0):
        for l in range(levels):
            f = h.level_flags(l)
            assert f[name] and not any(f[a] for a in absent), (case["family"], l, f)
    return check


def diagonals_inside(case, s):
    d = np.abs(sc.family(*case["family"])[0].diagonal()) * abs(s)
    return bool(np.all((d >= 2.0 ** -400) & (d <= 2.0 ** 400)))


def march_in_range(h, case, s=1.0):
    """march.hip's plans take a level whose diagonals all lie within 2^-400 .. 2^400 (its quotient's range) and leave
    any other to the level schedule: by design, so the flag is pinned on both sides of the edge.  The level schedule
    adds the squares of a norm in another order, so a pair beyond the edge is compared with the unscaled operator on
    the level schedule (the *_sets cases: OMG_MARCH=0), bit for bit like every other."""
    assert h.level_flags(0)["march"] == diagonals_inside(case, s), (case["family"], s, h.level_flags(0))


def no_march(h, case, s=1.0):
    assert not h.level_flags(0)["march"], h.level_flags(0)


def tail_fused(h, case, s=1.0):
    planes(2)(h, case)
    assert h.level_flags(1)["tail_fused"], h.level_flags(1)


def constant_nullspace(h, case, s=1.0):
    assert h.nullspace == "constant" and h.coarse_info()["n"] == h.sizes[-1]


def sets_only(h, case, s=1.0):
    f = h.level_flags(0)
    assert not (f["plane"] or f["march"] or f["var7"] or f["stencil27"]), f


def case(family, smoother, check, env=None, omega=1.0, dtype="float64", route="lists", nullspace=None, prepare=None):
    return dict(family=family, smoother=smoother, check=check, env=env or {}, omega=omega, dtype=dtype, route=route,
                nullspace=nullspace, prepare=prepare)


BLOCK = ("poisson", (16, 16, 16), 3)
MARCH = ("poisson", (16, 24, 20), 3)
VAR7 = ("var7", (16, 20, 36), 2)
S27 = ("s27", (8, 12, 20), 2)

CASES = {
    # the block-in-LDS kernel on the 8^3 level below the marching finest level
    "block": case(BLOCK, "colour", planes(2)),
    "march_la2": case(MARCH, "colour", planes(2), {"OMG_PLANE_BLOCK": "0", "OMG_PLANE_LA2": "1"}),
    "march_la1": case(MARCH, "colour", planes(2), {"OMG_PLANE_BLOCK": "0", "OMG_PLANE_LA2": "0"}),
    "tile2d_colour": case(("poisson", (64, 64), 3), "colour", planes(2)),
    "tile2d_jacobi": case(("poisson", (64, 64), 3), "jacobi", planes(2), omega=2.0 / 3.0),
    "tail": case(("reference", (64, 64, 64), 3), "colour", tail_fused, {"OMG_TAIL_FUSE": "2"}, route="from_fine"),
    "lex_constant": case(("poisson", (16, 16, 16), 2), "gs", march_in_range),
    "lex_rows": case(("rows", (16, 16, 16), 2), "gs", march_in_range),
    "lex_line": case(("line", (4096,), 2), "gs", march_in_range),
    "lex_constant_sets": case(("poisson", (16, 16, 16), 2), "gs", no_march, {"OMG_MARCH": "0"}),
    "lex_rows_sets": case(("rows", (16, 16, 16), 2), "gs", no_march, {"OMG_MARCH": "0"}),
    "lex_line_sets": case(("line", (4096,), 2), "gs", no_march, {"OMG_MARCH": "0"}),
    "var7_sym": case(VAR7, "colour", flag("var7", absent=("plane",)), {"OMG_VAR7_MIN": "4096", "OMG_VAR7_SYM": "1"}),
    "var7_general": case(VAR7, "colour", flag("var7", absent=("plane",)), {"OMG_VAR7_MIN": "4096", "OMG_VAR7_SYM": "0"}),
    "s27": case(S27, "colour", flag("stencil27")),
    "s27_fp32": case(S27, "colour", flag("stencil27"), dtype="float32"),
    "block_fp32": case(BLOCK, "colour", planes(2), dtype="float32"),
    "csr_block": case(BLOCK, "colour", None, prepare=lambda h: h.use_plane(False)),
    "csr_irregular": case(("irregular", None, 2), "colour", sets_only, omega=0.5),
    "neumann": case(("neumann", (8, 8, 8), 2), "colour", constant_nullspace, nullspace="constant"),
    "cycle_F": case(BLOCK, "colour", planes(2), prepare=lambda h: h.set_cycle("F", 1.8)),
    "cycle_W": case(BLOCK, "colour", planes(2), prepare=lambda h: h.set_cycle("W", 1.0)),
    "block_mixed": case(BLOCK, "colour", planes(2), dtype="mixed"),
}


def vectors(c):
    A0, Rs, b, x0 = sc.family(*c["family"])
    if c["dtype"] == "float32":
        b, x0 = sc.as_float32(b), sc.as_float32(x0)
    return A0, Rs, b, x0


def open_case(name, s=1.0):
    """the case's hierarchy for s * A, made under the case's switches (the caller holds sc.environment(c['env']))"""
    c = CASES[name]
    A0, Rs, _, _ = vectors(c)
    As = sc.scaled(A0, s)
    kw = dict(smoother=c["smoother"], omega=c["omega"], dtype=c["dtype"], nullspace=c["nullspace"])
    if c["route"] == "from_fine":
        h = _hip.Hierarchy.from_fine(As, c["family"][1], len(Rs), **kw)
    else:
        h = _hip.Hierarchy(sc.galerkin(As, Rs), Rs, **kw)
    if c["check"] is not None:
        c["check"](h, c, s)
    if c["prepare"] is not None:
        c["prepare"](h)
        if name == "csr_block":
            assert not h.level_flags(0)["plane"]
    return h


def cycles(h, b, x0):
    """V(1,1) and V(1,0), three cycles each: batched from x0, single calls from zero"""
    out = []
    for pre, post in sc.SWEEPS:
        h.resident_load(b, x0)
        out += [("norms", np.array(h.resident_cycles(pre, post, sc.CYCLES))), ("x", h.resident_fetch())]
        h.resident_load(b)
        out += [("norms", np.array([h.resident_cycle(pre, post) for _ in range(sc.CYCLES)])), ("x", h.resident_fetch())]
    return out


def tail_cycles(h, b, x0):
    before = h.tail_info()[0]
    out = cycles(h, b, x0)
    return out + [("count", h.tail_info()[0] - before)]


def neumann_calls(h, b, x0):
    """the projection (b scales by t, its mean too), gamma through the coarse solve, and the cycles"""
    pb, mean = h.project(0, b)
    bc = np.asarray(h.restrict(0, pb))
    return [("b", pb), ("b", np.array([mean])), ("x", h.coarse_solve(bc))] + cycles(h, b, x0)


def fcg(h, b, x0):
    out = []
    for start in (x0, None):
        h.resident_load(b, start)
        its, norms, tn, bd = h.resident_pcg(1, 1, 12, 0.0)
        out += [("count", its), ("count", bd), ("norms", norms), ("norms", np.array([tn])), ("x", h.resident_fetch())]
    return out


def mixed_calls(h, b, x0):
    out = fcg(h, b, x0)
    h.resident_load(b, x0)
    out += [("norms", np.array(h.resident_cycles(1, 1, 6))), ("x", h.resident_fetch())]
    return out


CALLS = {"tail": tail_cycles, "neumann": neumann_calls, "block_mixed": mixed_calls}


def run(name, calls, pair=(0, 0), sign=1):
    c = CASES[name]
    _, _, b, x0 = vectors(c)
    s, t, f = sc.factors(pair, sign)
    with sc.environment(c["env"]):
        with open_case(name, s) as h:
            return calls(h, t * b, f * x0)


@functools.lru_cache(maxsize=None)
def baseline(name, calls):
    out = run(name, calls)
    assert all(np.all(np.isfinite(v)) for _, v in out), name
    return out


def pairs_of(name):
    c = CASES[name]
    if c["dtype"] == "float32":
        return [(p, 1) for p in sc.PAIRS32]
    if c["dtype"] == "mixed":
        return [(p, 1) for p in ((0, 0), (24, -24), (0, -400), (0, -110), (0, 130), (0, 400))]
    return [(p, 1) for p in sc.pairs64(sc.diagonal_of(*c["family"]))] + [((0, 0), -1)]


def expand(names, signed=True):
    return [pytest.param(n, p, s, id="%s-%s%s" % (n, sc.pair_id(p), "-negated" if s < 0 else ""))
            for n in names for p, s in pairs_of(n) if signed or s > 0]


def check(name, calls, pair, sign):
    c = CASES[name]
    if c["check"] is march_in_range and not diagonals_inside(c, sc.factors(pair, sign)[0]):
        base = baseline(name + "_sets", calls)
    else:
        base = baseline(name, calls)
    if name == "tail":
        assert base[-1] == ("count", 4 * sc.CYCLES), base[-1]        # one fused launch per cycle
    got = run(name, calls, pair, sign)
    sc.assert_equivariant(base, got, pair, sign, name)


# ---- 1. cycles on every path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pair,sign", expand([n for n in CASES if n != "block_mixed"]))
def test_cycles_are_equivariant(name, pair, sign):
    check(name, CALLS.get(name, cycles), pair, sign)


# ---- 2. FCG and the mixed entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pair,sign", expand(["block", "var7_sym"], signed=False))
def test_fcg_is_equivariant(name, pair, sign):
    """iteration count, every recurrence norm, the true norm, the iterate"""
    check(name, fcg, pair, sign)


@pytest.mark.parametrize("name,pair,sign", expand(["block_mixed"]))
def test_mixed_entries_are_equivariant(name, pair, sign):
    """resident_pcg and resident_cycles of a mixed hierarchy: the fp32 cycle is handed fl32(2^-e r), e from a norm of
    the iteration, so b may have any size fp64 takes"""
    check(name, mixed_calls, pair, sign)


def test_mixed_fcg_of_a_tiny_right_hand_side_takes_the_iterations_of_the_unscaled_solve():
    """2^-110 b (and 2^130 b) to rtol 1e-10: the iterations, every norm and the iterate of the solve of b, scaled.
    Before the fp32 cycle was handed fl32(2^-e r) this failed.  What that build gave here (16^3, three grids):
        b          16 iterations, true norm / ||b|| 4.692e-11
        2^-110 b   16 iterations as well, no breakdown, but true norm / ||b|| 4.719e-11 and other norms from the
                   first subnormal fl32(r) on (the last one 5.5682...34387e-42 against 2^-110 * the unscaled
                   5.5682...33032e-42): the count alone did not show it at this size, the bits did
        2^130 b    0 iterations, breakdown: the first cast overflowed to inf
    and resident_pcg / resident_cycles / mgSolve at 2^+-400 b ended in a breakdown in iteration 1."""
    c = CASES["block_mixed"]
    _, _, b, _ = vectors(c)
    tol = 1e-10 * float(np.linalg.norm(b))
    out = {}
    for kb in (0, -110, 130):
        t = math.ldexp(1.0, kb)
        with open_case("block_mixed") as h:
            h.resident_load(t * b)
            its, norms, tn, bd = h.resident_pcg(1, 1, 200, tol * t)
            out[kb] = (its, bd, norms, tn, h.resident_fetch())
        print("mixed FCG, b * 2^%d: iterations %d, breakdown %s, true norm / ||b|| %.3e" % (kb, its, bd, tn / (t * np.linalg.norm(b))))
    its, bd, norms, tn, x = out[0]
    assert not bd and tn <= 2 * tol
    for kb in (-110, 130):
        t = math.ldexp(1.0, kb)
        assert out[kb][0] == its and not out[kb][1], (kb, out[kb][0], its, out[kb][1])
        assert np.all(out[kb][2] == t * norms) and out[kb][3] == t * tn
        assert sc.same_bits(out[kb][4], t * x), (kb,) + sc.differing(out[kb][4], t * x)


@pytest.mark.parametrize("kb", [0, -200, 130])            # (norms down to 2^-230 * 1e-10: their squares stay normal doubles)
def test_mixed_warm_start_far_from_the_right_hand_side(kb):
    """||b - A x0|| is 2^200 times ||b||: the exponent of ||b|| would leave fl32(2^-e r0) = inf, so the start takes the
    exponent of ||r0|| itself and writes the cycle's right-hand side once more (pcg_fold_start, pcg_lower).  The cycles
    and FCG follow the fp64 hierarchy's to float accuracy, and scale with 2^kb bit for bit like every other start."""
    c = CASES["block_mixed"]
    A0, Rs, b, x0 = vectors(c)
    small = math.ldexp(1.0, -200) * b
    t = math.ldexp(1.0, kb)
    with open_case("block_mixed") as h:
        base = mixed_calls(h, small, x0)
        got = mixed_calls(h, t * small, t * x0)
    with open_case("block") as h64:
        want = mixed_calls(h64, small, x0)
    sc.assert_equivariant(base, got, (0, kb), 1, "far warm start")
    assert all(np.all(np.isfinite(v)) for _, v in base)
    its, norms = base[0][1], base[2][1]
    assert its == 12 and not base[1][1] and norms[-1] < 1e-8 * np.linalg.norm(A0 @ x0)
    np.testing.assert_allclose(norms[:4], want[2][1][:4], rtol=1e-3)
    cyc, cyc64 = base[-2][1], want[-2][1]
    np.testing.assert_allclose(cyc, cyc64, rtol=1e-3)


@pytest.mark.parametrize("kb", [-400, -110, 130, 400])
def test_mgsolve_mixed_cg_is_equivariant(kb):
    shape = (16, 16, 16)
    A0 = sp.csr_matrix(operators.stencil_poisson(shape))
    b = np.random.default_rng(97).standard_normal(A0.shape[0])
    p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 8, "threshold": 0.0,
         "giveInfo": True, "smoother": "colour", "dtype": "mixed", "accel": "cg", "minSize": 4}
    t = math.ldexp(1.0, kb)
    try:
        u, info = openmg_amd.mgSolve(A0, b, dict(p))
        v, scaled_info = openmg_amd.mgSolve(A0, t * b, dict(p))
    finally:
        openmg_amd.clear_cache()
    assert np.all(np.isfinite(u)) and info["cycle"] == scaled_info["cycle"] == 8
    assert scaled_info["norm"] == t * info["norm"]
    assert sc.same_bits(v, t * u), (kb,) + sc.differing(v, t * u)


# ---- 3. Solver.solve --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sc.pairs64(6.0), ids=sc.pair_id)
def test_solver_solve_is_equivariant(pair):
    shape = (16, 16, 16)
    A0, _, b, x0 = sc.family(*BLOCK)
    p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 100, "threshold": 0.0,
         "smoother": "colour", "minSize": 4}
    s, t, f = sc.factors(pair)
    res = []
    for As, bs, xs in ((A0, b, x0), (sc.scaled(A0, s), t * b, f * x0)):
        with openmg_amd.Solver(As, dict(p)) as solver:
            assert solver.hierarchy.level_flags(0)["plane"] and solver.hierarchy.level_flags(1)["plane"]
            out = []
            for start in (None, xs):
                u, info = solver.solve(bs, initial=None if start is None else start.copy(), rtol=1e-8)
                out += [("count", info["cycle"]), ("norms", np.array(info["norms"])),
                        ("norms", np.array([info["norm"], info["rhs_norm"], info["initial_norm"]])), ("x", u)]
            res.append(out)
    assert 0 < res[0][0][1] < 100
    sc.assert_equivariant(res[0], res[1], pair, 1, "Solver.solve")


# ---- 4. the coarse solvers ----------------------------------------------------------------------------------------------
COARSE = {"sine": {}, "inverse": {"OMG_COARSE_BLOCKS": "1"}, "substructured": {"OMG_COARSE_BLOCKS": "3"},
          "chain": {"OMG_COARSE_CHAIN": "1", "OMG_COARSE_SINE": "0"}}


@functools.lru_cache(maxsize=None)
def coarse_problem():
    A = sp.csr_matrix(operators.stencil_poisson((12, 12, 12)))
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def coarse_baseline(kind):
    A, b = coarse_problem()
    with sc.environment(COARSE[kind]):
        x = _hip.direct_solve(A, b)
    assert np.all(np.isfinite(x)) and np.linalg.norm(b - A @ x) <= 1e-9 * np.linalg.norm(b)
    return x


@pytest.mark.parametrize("pair,sign", [(p, 1) for p in sc.pairs64(6.0)] + [((0, 0), -1)],
                         ids=lambda v: sc.pair_id(v) if isinstance(v, tuple) else ("negated" if v < 0 else "plain"))
@pytest.mark.parametrize("kind", list(COARSE))
def test_direct_solve_is_equivariant(kind, pair, sign):
    A, b = coarse_problem()
    x = coarse_baseline(kind)
    s, t, f = sc.factors(pair, sign)
    with sc.environment(COARSE[kind]):
        got = _hip.direct_solve(sc.scaled(A, s), t * b)
    assert sc.same_bits(got, x * f), (kind, pair, sign) + sc.differing(got, x * f)


# ---- 5. numerators at the edges of quotients() -----------------------------------------------------------------------
EDGE_CASES = ["block", "march_la1", "tile2d_colour", "tile2d_jacobi", "tail"]


def edge_vectors(name):
    """b with 0.0, -0.0, 5e-324, 1e-300, 1e300 and values whose numerators have the exponents 400 (plain) and 401 (not),
    -400 (plain) and -401 (not), each alone among ordinary values, far from the next one: a wave meets at most one of
    them — the waves over the stretches in between meet none — and the grid's first and last cells hold two that are
    not plain.  x0 is finite everywhere, and zero on the cell and the neighbours of every small value, so that the
    numerator of the first relaxation there is b itself (those cells are red: every neighbour is still x0's)."""
    A0, _, b, x0 = vectors(CASES[name])
    shape = CASES[name]["family"][1]
    n = A0.shape[0]
    b, x0 = b.copy(), x0.copy()
    specials = [0.0, -0.0, 5e-324, 1e-300, 1e300, 1.5 * 2.0 ** 400, 1.5 * 2.0 ** 401, 1.5 * 2.0 ** -400, 1.5 * 2.0 ** -401,
                -1e300, -1.5 * 2.0 ** 401, -5e-324]
    idx = np.arange(n).reshape(shape)
    parity = np.indices(shape).sum(axis=0) % 2
    reds = idx[parity == 0]
    gap = max(130, n // (len(specials) + 2))
    assert gap * (len(specials) + 1) < n, (name, n)
    where = []
    for k, v in enumerate(specials):
        at = int(reds[np.searchsorted(reds, (k + 1) * gap)])      # the first red cell at or after (k + 1) * gap
        where.append(at)
        b[at] = v
        if abs(v) < 1.0:
            nb = A0.indices[A0.indptr[at]:A0.indptr[at + 1]]
            x0[nb] = 0.0
            if math.copysign(1.0, v) < 0:
                x0[at] = -0.0                                      # (the sign of the quotient's zero shows only next to -0.0)
    assert all(q - p >= 128 for p, q in zip(where, where[1:]))
    b[0], b[n - 1] = 1e300, 1.5 * 2.0 ** 401
    return b, x0


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_numerators_have_the_bits_of_the_division(name):
    """one cycle of one sweep (and V(1,1)) on the plane passes and on the set-by-set schedule, which divides"""
    c = CASES[name]
    b, x0 = edge_vectors(name)
    with sc.environment(c["env"]):
        with open_case(name) as h:
            for pre, post in ((1, 0), (1, 1)):
                h.use_plane(True)
                if c["check"] is not None:
                    c["check"](h, c)
                h.resident_load(b, x0)
                h.resident_cycle(pre, post)
                got = h.resident_fetch()
                h.use_plane(False)
                assert not h.level_flags(0)["plane"]
                h.resident_load(b, x0)
                h.resident_cycle(pre, post)
                want = h.resident_fetch()
                assert np.all(np.isfinite(want)), name
                assert sc.same_bits(got, want), (name, pre, post) + sc.differing(got, want)


@pytest.mark.parametrize("name", EDGE_CASES)
def test_a_negative_zero_numerator(name):
    """b = 0 with one -0.0 (a red cell, then a black one).  The relaxation is the reference's
    x[i] = x[i] + (b[i] - A_i x) / A[i, i] (openmg/solvers.py:68): the quotient is ADDED to x[i].  The refined-reciprocal
    sequence of quotients() gives +0.0 from a numerator of -0.0 where the division gives -0.0 (fma(-c, -0, -0) = +0), but
    from a zero start x[i] = +0.0 + (-0.0 / c3) = +0.0 on every schedule and on the CPU oracle
    (tests/test_scaling_host.py), whichever zero the quotient was; V(1,0), V(0,1), V(1,1).  With x[i] = -0.0 at the
    start as well, the plane passes still leave the bits of the set-by-set schedule: the coarse correction, +0.0 here,
    is added after the sweep, and a post-smoothing sweep then starts from +0.0 again."""
    c = CASES[name]
    A0 = vectors(c)[0]
    n = A0.shape[0]
    c3 = np.float64(A0.diagonal()[0])
    want_bits = np.array([np.float64(0.0) + np.float64(-0.0) / c3]).view(np.uint64)[0]
    assert want_bits == 0
    shape = c["family"][1]
    parity = (np.indices(shape).sum(axis=0) % 2).ravel()
    with sc.environment(c["env"]):
        with open_case(name) as h:
            for colour in (0, 1):
                i = int(np.flatnonzero(parity == colour)[n // 4])
                b = np.zeros(n)
                b[i] = -0.0
                start = np.zeros(n)
                start[i] = -0.0
                for x0 in (None, start):
                    for pre, post in ((1, 0), (0, 1), (1, 1)):
                        res = {}
                        for plane in (True, False):
                            h.use_plane(plane)
                            h.resident_load(b, x0)
                            h.resident_cycle(pre, post)
                            res[plane] = h.resident_fetch()
                        what = (name, colour, x0 is None, pre, post, float(res[True][i]).hex(), float(res[False][i]).hex())
                        assert sc.same_bits(res[True], res[False]), what + sc.differing(res[True], res[False])
                        if x0 is None:
                            assert res[True].view(np.uint64)[i] == want_bits, what
