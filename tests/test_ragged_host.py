"""Grids of any extent (parameters['oddExtents'] = 'merge') without a GPU: the rule through the library's exported host
functions (omg_semicoarsen_rule_ragged needs no device), the cases of tests/ragged_cases.py restated with the oracle — which
fixes the factor sequences, level shapes and cycle counts tests/test_gpu_ragged.py compares the device with —, and
ValueError for every malformed use of the key before any device work (where no device is visible a call that reached the
library's device entries would raise HipError instead)."""
import ctypes
import itertools

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import ragged_cases as rc
import semicoarsen_cases as sc
from test_semicoarsen_host import RULE


def rule_c(name, shape, sums, counts, line_axis, odd=None):
    """(code, factors) of the C entry `name`, called directly; odd None: the entry without the flag"""
    dim = len(shape)
    s3 = (ctypes.c_double * 3)(*(list(sums) + [0.0] * (3 - dim)))
    c4 = (ctypes.c_int64 * 4)(*(list(counts) + [0] * (3 - dim) + [0]))
    f3 = (ctypes.c_int * 3)()
    args = [dim, (ctypes.c_int64 * dim)(*shape), s3, c4, -1 if line_axis is None else line_axis, 0]
    code = getattr(_hip.lib(), name)(*(args + ([] if odd is None else [odd]) + [f3]))
    return code, tuple(int(f3[d]) for d in range(dim))


def test_the_rule_with_odd_refuse_is_the_rule_without_the_flag():
    n = 0
    extents = (2, 3, 4, 5, 6, 7, 16)
    couplings = ((1.0, 1.0, 1.0), (1.0, 10.0, 100.0), (100.0, 1.0, 10.0), (5.0, 10.0, 2.5), (0.0, 10.0, 10.0))
    for shape in itertools.product(extents, repeat=3):
        for sums in couplings:
            for line_axis in (None, 0, 2):
                old = rule_c("omg_semicoarsen_rule", shape, sums, (10, 10, 10), line_axis)
                new = rule_c("omg_semicoarsen_rule_ragged", shape, sums, (10, 10, 10), line_axis, _hip.ODD_REFUSE)
                assert old == new and old[0] == _hip.OMG_OK, (shape, sums, line_axis)
                assert all(f == 1 or (e >= 4 and e % 2 == 0) for e, f in zip(shape, old[1]))
                n += 1
    for shape in itertools.product(extents, repeat=2):
        assert rule_c("omg_semicoarsen_rule", shape, (1.0, 3.0), (7, 9), None) == \
            rule_c("omg_semicoarsen_rule_ragged", shape, (1.0, 3.0), (7, 9), None, _hip.ODD_REFUSE)
    assert n == 7 ** 3 * 5 * 3
    # the existing table, through the Python binding with the key left out and with None
    for sums, counts, shape, line_axis, want in RULE:
        assert _hip.semicoarsen_rule(shape, sums, counts, 0, line_axis, oddExtents=None) == want


def test_a_flag_that_is_neither_is_refused():
    code, _ = rule_c("omg_semicoarsen_rule_ragged", (8, 8, 8), (1.0, 1.0, 1.0), (10, 10, 10), None, 2)
    assert code == _hip.ERR_INVALID
    for bad in ("MERGE", "refuse", 1, True, 0, ""):
        with pytest.raises(ValueError, match="oddExtents"):
            _hip.odd_code(bad)
    assert _hip.odd_code(None) == _hip.ODD_REFUSE == 0 and _hip.odd_code("merge") == _hip.ODD_MERGE == 1


@pytest.mark.parametrize("extent,eligible", [(2, False), (3, False), (4, True), (5, True), (6, True), (7, True)])
def test_eligibility_with_merge_is_extent_at_least_four(extent, eligible):
    for axis in range(3):
        shape = tuple(extent if a == axis else 2 for a in range(3))
        got = _hip.semicoarsen_rule(shape, (1.0, 1.0, 1.0), (10, 10, 10), oddExtents="merge")
        assert got == tuple(2 if (a == axis and eligible) else 1 for a in range(3)), shape
    assert operators.canHalve(extent, "merge") == eligible
    assert operators.canHalve(extent) == (eligible and extent % 2 == 0)


# the line-axis and tie rows of tests/test_semicoarsen_host.py's table on odd extents: (sums, counts, extents, line axis, factors)
ODD_RULE = [
    ((6.0, 6.0, 6.0), (6, 6, 6), (15, 17, 21), None, (2, 2, 2)),
    ((1.0, 10.0, 10.0), (10, 10, 10), (15, 15, 15), None, (1, 2, 2)),
    ((100.0, 1.0, 10.0), (10, 10, 10), (15, 9, 7), None, (2, 1, 1)),
    # ties coarsen: exactly half the strongest mean, and one ulp below it does not
    ((5.0, 10.0, 2.5), (10, 10, 10), (15, 15, 15), None, (2, 2, 1)),
    ((np.nextafter(5.0, 0.0), 10.0, 5.0), (10, 10, 10), (15, 15, 15), None, (1, 2, 2)),
    # the strongest axis is odd: today it stands aside, with 'merge' it is the reference
    ((1.0, 10.0, 1000.0), (10, 10, 10), (16, 16, 15), None, (1, 1, 2)),
    # ... and below 4 it still stands aside
    ((1.0, 10.0, 1000.0), (10, 10, 10), (16, 15, 3), None, (1, 2, 1)),
    ((6.0, 10.0, 1000.0), (10, 10, 10), (15, 15, 3), None, (2, 2, 1)),
    # no eligible axis: the hierarchy ends
    ((1.0, 10.0, 1000.0), (10, 10, 10), (2, 3, 3), None, (1, 1, 1)),
    ((1.0, 1.0), (4, 4), (3, 3), None, (1, 1)),
    # the line axis stands back from the maximum and is always coarsened when eligible
    ((1.0, 100.0, 100.0), (10, 10, 10), (15, 15, 15), 2, (1, 2, 2)),
    ((1.0, 10.0, 100.0), (10, 10, 10), (15, 15, 15), 2, (1, 2, 2)),
    ((1.0, 1.0, 100.0), (10, 10, 10), (15, 15, 15), 2, (2, 2, 2)),
    ((1.0, 1.0, 100.0), (10, 10, 10), (16, 16, 15), 2, (2, 2, 2)),       # (without the key: (2, 2, 1), the line axis not eligible)
    ((1.0, 1.0, 100.0), (10, 10, 10), (15, 15, 3), 2, (2, 2, 1)),        # line axis not eligible: never coarsened
    ((1.0, 1.0, 100.0), (10, 10, 10), (3, 3, 15), 2, (1, 1, 2)),         # the line axis alone is eligible: it is the reference
    ((100.0, 1.0, 1.0), (10, 10, 10), (15, 15, 15), 0, (2, 2, 2)),
    # 2-D
    ((1.0, 100.0), (10, 10), (15, 25), None, (1, 2)),
    ((100.0, 60.0), (10, 10), (13, 10), None, (2, 2)),
]


@pytest.mark.parametrize("sums,counts,shape,line_axis,want", ODD_RULE)
def test_rule_table_on_odd_extents(sums, counts, shape, line_axis, want):
    assert _hip.semicoarsen_rule(shape, sums, counts, 0, line_axis, oddExtents="merge") == want
    # on the even extents next to them the key changes nothing
    even = tuple(e + e % 2 if e >= 4 else e for e in shape)
    assert _hip.semicoarsen_rule(even, sums, counts, 0, line_axis, oddExtents="merge") == _hip.semicoarsen_rule(even, sums, counts, 0, line_axis)


def test_check_factors_and_coarsening_of():
    of = operators.coarseningOf
    assert operators.checkFactors((5, 8), (2, 1), "merge") == (2, 1)
    assert operators.checkFactors((5, 8), (2, 2), oddExtents="merge") == (2, 2)
    with pytest.raises(ValueError, match="a factor of 2 needs an even extent >= 4: axis 0 of the level's grid \\(5, 8\\) has 5"):
        operators.checkFactors((5, 8), (2, 1))
    for odd in (None, "merge"):
        with pytest.raises(ValueError, match="extent >= 4"):
            operators.checkFactors((3, 8), (2, 1), odd)
        with pytest.raises(ValueError):
            operators.checkFactors((5, 8), (1, 1), odd)
        with pytest.raises(ValueError):
            operators.checkFactors((5, 8), (3, 1), odd)
    with pytest.raises(ValueError, match="oddExtents"):
        operators.checkFactors((5, 8), (2, 1), "join")
    # named tuples: consumed by the depth rule with floor extents
    seq = [(2, 2, 2), (2, 2, 2), (1, 1, 2)]
    assert of(seq, (9, 14, 21), 2, 1, "merge") == seq
    assert of(seq, (9, 14, 21), 5, 1, "merge") == seq               # (2, 3, 2): nothing left to coarsen
    assert of(seq, (9, 14, 21), 2, 20, "merge") == seq[:2]           # 2 x 3 x 5 = 30 > 20, 2 x 3 x 2 = 12 <= 20
    with pytest.raises(ValueError, match="even extent"):
        of(seq, (9, 14, 21), 2, 1)
    with pytest.raises(ValueError, match="extent >= 4"):
        of([(2, 2, 2), (2, 2, 2), (1, 2, 2)], (9, 14, 21), 2, 1, "merge")         # a 2 on extent 3
    with pytest.raises(ValueError, match="restriction 1 is reached"):
        of(seq[:1], (9, 14, 21), 2, 1, "merge")                      # (4, 7, 10) can still be coarsened
    assert of("auto", (9, 14, 21), 2, 1, "merge") == "auto"
    # None / 'full': the reference's hierarchy without the key, a named one with it
    assert of(None, (9, 14, 21), 2, 1) is None and of("full", (9, 14, 21), 2, 1, None) is None
    for name, row in rc.TABLE.items():
        if row[5] == "full":
            assert of(None, row[0], row[4] - 1, rc.MIN_SIZE, "merge") == of("full", row[0], row[4] - 1, rc.MIN_SIZE, "merge") == row[7], name
    assert of(None, (16, 16, 16), 5, 8, "merge") == [(2, 2, 2)] * 2     # minSize 8 stops at 4^3, as restrictionList does
    assert of(None, (100, 100, 100), 4, 8, "merge") == [(2, 2, 2)] * 5
    boxes = of("full", (300, 150, 75), 9, 0, "merge")                # ... (9, 4, 2) -> (4, 2, 2) -> (2, 2, 2)
    assert boxes == [(2, 2, 2)] * 5 + [(2, 2, 1), (2, 1, 1)]
    with pytest.raises(ValueError, match="no axis"):
        of(None, (3, 3, 2), 2, 1, "merge")
    with pytest.raises(ValueError):
        of(None, (100,), 2, 1, "merge")                              # 1-D
    with pytest.raises(ValueError, match="oddExtents"):
        of(None, (9, 14, 21), 2, 1, "MERGE")


A15 = sc.aniso((15, 15, 15), (1, 1, 1))


@pytest.mark.parametrize("kw", [
    {"oddExtents": "MERGE"}, {"oddExtents": "refuse"}, {"oddExtents": 1}, {"oddExtents": True}, {"oddExtents": ["merge"]},
    {"oddExtents": "merge", "dense": True},
    {"oddExtents": "merge", "coarsening": [(2, 2, 2), (2, 2, 2), (2, 2, 2)]},            # the third 2 meets extent 3
    {"oddExtents": "merge", "coarsening": [(2, 2, 2)]},                                     # shorter than the depth reached
    {"oddExtents": "merge", "coarsening": "semi"},
    {"oddExtents": "merge", "problemShape": (3375,)},
    {"coarsening": [(2, 2, 2), (2, 2, 2)]},                                                  # without the key: a 2 on 15
], ids=repr)
def test_malformed_use_raises_value_error_before_any_device_work(kw):
    p = {"problemShape": (15, 15, 15), "gridLevels": 3, "cycles": 1, "minSize": 1, "smoother": "colour"}
    b = np.ones(A15.shape[0])
    for extra in ({}, {"giveInfo": True}, {"smoother": "line"}):
        with pytest.raises(ValueError):
            openmg_amd.mgSolve(A15, b, dict(p, **extra, **kw))
    with pytest.raises(ValueError):
        openmg_amd.Solver(A15, dict(p, **kw))


def test_dist_entries_refuse_the_key():
    from openmg_amd import dist
    for value in ("merge", "anything"):
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.refuse_odd_extents(value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.build_all_ranks(None, None, oddExtents=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.build_this_rank(None, 0, None, None, oddExtents=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.make_tail(None, (9, 9, 9), 2, oddExtents=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.RankSetup(None, 0, None, oddExtents=value)
    dist.refuse_odd_extents(None)


@pytest.mark.parametrize("shape", [(4, 5), (7, 9), (13, 10), (5, 5, 5), (4, 6, 7), (9, 14, 21), (25, 25, 25)])
def test_the_yardsticks_aggregation_is_one(shape):
    """Every fine cell in exactly one aggregate, one weight, 1 .. 3 members along an axis — what the reference's own
    restriction() does not give on an odd extent — and on even extents semicoarsen_cases' aggregation."""
    for f in itertools.product((1, 2), repeat=len(shape)):
        if all(v == 1 for v in f) or any(v == 2 and e < 4 for e, v in zip(shape, f)):
            continue
        R = rc.aggregation(shape, f)
        coarse = tuple(e // v for e, v in zip(shape, f))
        assert R.shape == (int(np.prod(coarse)), int(np.prod(shape))) and R.nnz == R.shape[1]
        assert np.array_equal(np.diff(R.tocsc().indptr), np.ones(R.shape[1], dtype=int))
        assert np.all(R.data == 1.0 / np.prod(f))
        per_row = np.diff(R.indptr).reshape(coarse)
        want = np.ones(coarse, dtype=int)
        for axis, (e, v) in enumerate(zip(shape, f)):
            m = np.full(e // v, v)
            m[-1] += e - v * (e // v)
            want = want * m.reshape([-1 if a == axis else 1 for a in range(len(shape))])
        assert np.array_equal(per_row, want)
        even = tuple(e - e % 2 if v == 2 else e for e, v in zip(shape, f))
        assert (rc.aggregation(even, f) != sc.aggregation(even, f)).nnz == 0


@pytest.mark.parametrize("name", sorted(rc.TABLE))
def test_table_restated_with_the_oracle(name):
    """Factors, level shapes and cycles to 1e-8 ||b|| of every row as recorded in ragged_cases.TABLE; no deciding norm, and
    none before it, within 1 % of the threshold; no axis collapses."""
    want_factors, want_shapes, want_cycles = rc.TABLE[name][7:10]
    c = rc.case(name)
    target = rc.TOL * float(np.linalg.norm(c["b"]))
    print(name, c["factors"], c["shapes"], c["cycles"], c["norms"][-1] / target, c["norms"][-2] / target)
    assert c["factors"] == want_factors and c["shapes"] == want_shapes
    assert all(min(s) >= 2 for s in c["shapes"])
    assert [M.shape[0] for M in c["A"]] == [int(np.prod(s)) for s in c["shapes"]]
    assert c["cycles"] == want_cycles
    assert c["norms"][-1] < 0.99 * target and c["norms"][-2] > 1.01 * target
    if c["neumann"]:
        for M in c["A"]:                                             # uniform weights keep the constant null space on every level
            assert abs(M @ np.ones(M.shape[0])).max() <= 1e-12 * abs(M).max()


def test_the_merged_cell_costs_a_few_cycles_and_nothing_more():
    """(16, 16, 16) takes 35 cycles and (20, 20, 20) 43 with the same operator, smoother and three restrictions: the odd
    cubes between and beside them lie in that range."""
    counts = {}
    for e in (16, 20):
        A0 = sc.aniso((e,) * 3, (1, 1, 1))
        A, R, factors, shapes = rc.lists(A0, (e,) * 3, "full", 3, min_size=rc.MIN_SIZE)
        assert factors == [(2, 2, 2)] * 3
        counts[e] = rc.cycles_to(A, R, rc.rhs_of(A0.shape[0]), sc.smoother_of("colour", A, shapes))[0]
    assert counts == {16: 35, 20: 43}
    assert counts[16] <= rc.case("iso15")["cycles"] <= counts[20] and counts[16] <= rc.case("iso17")["cycles"] <= counts[20]
