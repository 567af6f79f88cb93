"""Semicoarsening (parameters['coarsening']) without a GPU: the 'auto' rule through the library's exported host function
(omg_semicoarsen_rule needs no device), the cases of tests/semicoarsen_cases.py restated with the oracle
(oracle.mg_oracle.mg_cycle on SciPy-built lists) — which fixes the factor sequences and cycle counts
tests/test_gpu_semicoarsen.py compares the device with —, and ValueError for every malformed 'coarsening' before any
device work (where no device is visible a call that reached the library's device entries would raise HipError instead)."""
import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import semicoarsen_cases as sc

# (sums, counts, extents, line axis) -> factors.  Means are sums / counts.
RULE = [
    # isotropic: everything
    ((6.0, 6.0, 6.0), (6, 6, 6), (16, 16, 16), None, (2, 2, 2)),
    # two strong axes, one strong axis, three strengths
    ((1.0, 10.0, 10.0), (10, 10, 10), (16, 16, 16), None, (1, 2, 2)),
    ((1.0, 1.0, 100.0), (10, 10, 10), (16, 16, 16), None, (1, 1, 2)),
    ((100.0, 1.0, 10.0), (10, 10, 10), (16, 16, 16), None, (2, 1, 1)),
    # ties coarsen: exactly half the strongest mean ...
    ((5.0, 10.0, 2.5), (10, 10, 10), (16, 16, 16), None, (2, 2, 1)),
    # ... and one ulp below it does not
    ((np.nextafter(5.0, 0.0), 10.0, 5.0), (10, 10, 10), (16, 16, 16), None, (1, 2, 2)),
    # the MEAN decides, not the sum: extents (16, 4, 4) give the weak axis more entries (the sum would sit on the threshold)
    ((480.0, 1920.0, 1920.0), (480, 384, 384), (16, 4, 4), None, (1, 2, 2)),
    ((960.0, 480.0, 480.0), (480, 384, 384), (16, 4, 4), None, (2, 2, 2)),
    # the strongest axis cannot be coarsened (odd, or below 4): the strongest ELIGIBLE axis is the reference
    ((1.0, 10.0, 1000.0), (10, 10, 10), (16, 16, 15), None, (1, 2, 1)),
    ((1.0, 10.0, 1000.0), (10, 10, 10), (16, 16, 2), None, (1, 2, 1)),
    ((6.0, 10.0, 1000.0), (10, 10, 10), (16, 16, 2), None, (2, 2, 1)),
    # no eligible axis: the hierarchy ends
    ((1.0, 10.0, 1000.0), (10, 10, 10), (2, 3, 6 + 1), None, (1, 1, 1)),
    ((1.0, 1.0), (4, 4), (2, 2), None, (1, 1)),
    # the line axis stands back from the maximum and is always coarsened when eligible
    ((1.0, 100.0, 100.0), (10, 10, 10), (16, 16, 16), 2, (1, 2, 2)),
    ((1.0, 10.0, 100.0), (10, 10, 10), (16, 16, 16), 2, (1, 2, 2)),      # (plain rule: (1, 1, 2))
    ((1.0, 1.0, 100.0), (10, 10, 10), (16, 16, 16), 2, (2, 2, 2)),       # (plain rule: (1, 1, 2))
    ((1.0, 1.0, 100.0), (10, 10, 10), (16, 16, 15), 2, (2, 2, 1)),       # line axis not eligible: never coarsened
    ((1.0, 1.0, 100.0), (10, 10, 10), (3, 3, 16), 2, (1, 1, 2)),         # the line axis alone is eligible: it is the reference
    ((100.0, 1.0, 1.0), (10, 10, 10), (16, 16, 16), 0, (2, 2, 2)),
    # 2-D
    ((1.0, 100.0), (10, 10), (16, 24), None, (1, 2)),
    ((100.0, 60.0), (10, 10), (16, 24), None, (2, 2)),
    # an axis without stored entries has strength 0
    ((0.0, 10.0, 10.0), (0, 10, 10), (16, 16, 16), None, (1, 2, 2)),
]


@pytest.mark.parametrize("sums,counts,shape,line_axis,want", RULE)
def test_rule_table(sums, counts, shape, line_axis, want):
    assert _hip.semicoarsen_rule(shape, sums, counts, 0, line_axis) == want


def test_rule_refuses_off_axis_entries_naming_the_level():
    with pytest.raises(_hip.HipError) as e:
        _hip.semicoarsen_rule((6, 6, 6), (1.0, 1.0, 1.0), (10, 10, 10), off_axis=8, level=2)
    assert e.value.code == _hip.ERR_UNSUPPORTED and "level 2" in str(e.value) and "name the factors" in str(e.value)
    with pytest.raises(_hip.HipError) as e:
        _hip.semicoarsen_rule((6, 6, 6), (1.0, 1.0, 1.0), (10, 10, 10), line_axis=3)
    assert e.value.code == _hip.ERR_INVALID


def test_mean_not_sum_on_16_4_4():
    """1 : 10 : 10 on (16, 4, 4) after two (1, 2, 2) steps: the plain sums sit exactly on the threshold, the means do not."""
    A, R, factors, shapes = sc.lists(sc.aniso((16, 16, 16), (1, 10, 10)), (16, 16, 16), [(1, 2, 2), (1, 2, 2)], 2, min_size=1)
    assert shapes[-1] == (16, 4, 4)
    s, c, off = sc.couplings(A[-1], shapes[-1])
    assert off == 0 and 2.0 * s[0] == s[1] == s[2]                   # on the threshold by the sum
    assert 2.0 * s[0] * c[1] < s[1] * c[0]                           # clearly below it by the mean
    assert _hip.semicoarsen_rule(shapes[-1], s, c, off) == (1, 2, 2)


@pytest.mark.parametrize("name", sorted(sc.TABLE))
def test_table_restated_with_the_oracle(name):
    """Factor sequence and cycles to 1e-8 ||b|| of every row, 'auto' against full coarsening; the counts recorded in
    semicoarsen_cases.TABLE are the oracle's and no deciding norm lies within 1 % of the threshold."""
    want_factors, want_semi, want_full = sc.TABLE[name][5:8]
    semi, full = sc.case(name, "auto"), sc.case(name, "full")
    target = sc.TOL * float(np.linalg.norm(semi["b"]))
    print(name, semi["factors"], "semi", semi["cycles"], semi["norms"][-1] / target, "full", full["cycles"], full["norms"][-1] / target)
    assert semi["factors"] == want_factors
    assert all(min(s) >= 2 for s in semi["shapes"])                  # no axis collapses
    assert semi["cycles"] == want_semi
    assert semi["norms"][-1] < 0.99 * target and semi["norms"][-2] > 1.01 * target
    assert full["cycles"] == want_full
    assert full["norms"][-1] < 0.99 * target and full["norms"][-2] > 1.01 * target
    assert semi["cycles"] <= full["cycles"]
    if max(sc.TABLE[name][1]) >= 100 and (semi["kind"] == "colour" or name == "line_yx100"):
        # a strong anisotropy the smoother does not deal with: full coarsening stalls, semicoarsening does not
        assert full["cycles"] >= 3 * semi["cycles"]


def test_isotropic_keeps_todays_hierarchy_and_anisotropy_returns_to_its_rate():
    iso = sc.case("iso16", "auto")
    full = sc.case("iso16", "full")
    assert iso["factors"] == full["factors"] == [(2, 2, 2)] * 3
    for a, b in zip(iso["A"], full["A"]):
        assert (a != b).nnz == 0
    assert iso["cycles"] == full["cycles"]
    for name in ("yx10", "yx100", "x100", "z100x10"):
        assert sc.case(name)["cycles"] <= iso["cycles"]


def test_cube32_one_strong_axis():
    """32^3, 1 : 1 : 100, red-black: full coarsening needs several times the cycles; the isotropic operator the same either
    way."""
    counts = {}
    for c in ((1, 1, 100), (1, 1, 1)):
        A0 = sc.aniso((32, 32, 32), c)
        b = sc.rhs(A0.shape[0])
        for how in ("auto", "full"):
            A, R, factors, shapes = sc.lists(A0, (32, 32, 32), how, 3, min_size=1)
            counts[c, how] = sc.cycles_to(A, R, b, sc.smoother_of("colour", A, shapes))[0]
    print(counts)
    assert counts[(1, 1, 1), "auto"] == counts[(1, 1, 1), "full"]
    assert counts[(1, 1, 100), "full"] >= 4 * counts[(1, 1, 100), "auto"]
    assert counts[(1, 1, 100), "auto"] <= counts[(1, 1, 1), "full"]


def test_aggregation_and_operators_checks():
    for shape, f in (((8, 12, 20), (3, 1, 1)), ((8, 12, 20), (1, 1, 1)), ((8, 12, 21), (1, 1, 2)), ((8, 12, 2), (1, 1, 2)),
                     ((8, 12, 20), (2, 2)), ((8, 12, 20), (2.0, 1, 1)), ((8, 12, 20), (True, 2, 1)), ((8, 12, 20), 2)):
        with pytest.raises(ValueError):
            operators.restriction(shape, factors=f)
    assert operators.checkFactors((8, 12, 20), [2, 1, np.int64(2)]) == (2, 1, 2)


A16 = sc.aniso((16, 16, 16), (1, 100, 100))
BAD = [
    "semi", "AUTO", 7, 2.5, True, [], [()], [(1, 1, 1)] * 3, [(2, 2)] * 3, [(2, 2, 2, 2)] * 3, [(3, 1, 1)] * 3, [(0, 2, 2)] * 3,
    [(1, 2.0, 2)] * 3, [(1, "2", 2)] * 3, [(1, 2, 2), 5, (1, 2, 2)], [(1, 2, 2)],                      # shorter than the depth reached
    [(1, 2, 2), (1, 2, 2), (1, 1, 1)], [(2, 2, 2), (2, 2, 2), (2, 2, 2), (2, 2, 2)][:3] + [None],
]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b)[:40] for b in BAD])
def test_malformed_coarsening_raises_value_error_before_any_device_work(bad):
    p = {"problemShape": (16, 16, 16), "gridLevels": 3, "cycles": 1, "minSize": 1, "smoother": "colour", "coarsening": bad}
    if isinstance(bad, list) and len(bad) == 4:
        p["gridLevels"] = 4                                           # (the fourth entry is reached, and is not a tuple)
    b = np.ones(A16.shape[0])
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A16, b, dict(p))
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A16, b, dict(p, giveInfo=True))
    with pytest.raises(ValueError):
        openmg_amd.Solver(A16, dict(p))


def test_extent_checks_follow_the_levels():
    b = np.ones(A16.shape[0])
    base = {"problemShape": (16, 16, 16), "gridLevels": 3, "cycles": 1, "minSize": 1, "smoother": "colour"}
    # 16 -> 8 -> 4 -> 2: a fourth factor of 2 on that axis meets extent 2
    with pytest.raises(ValueError, match="even extent >= 4"):
        openmg_amd.mgSolve(A16, b, dict(base, gridLevels=4, coarsening=[(1, 1, 2)] * 4))
    # odd extent
    A = sc.aniso((6, 10, 9), (1, 1, 1))
    with pytest.raises(ValueError, match="even extent >= 4"):
        openmg_amd.mgSolve(A, np.ones(A.shape[0]), dict(base, problemShape=(6, 10, 9), gridLevels=1, coarsening=[(1, 1, 2)]))
    # 1-D, a shape that does not match the operator, the dense path
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A16, b, dict(base, problemShape=(4096,), coarsening="auto"))
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A16, b, dict(base, problemShape=(16, 16, 8), coarsening="auto"))
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(A16, b, dict(base, dense=True, coarsening="auto"))


def test_depth_rule_consumes_the_sequence_like_restriction_list():
    of = operators.coarseningOf
    assert of(None) is None and of("full") is None
    assert of("auto", (16, 16, 16), 2, 8) == "auto"
    seq = [(1, 2, 2), (1, 2, 2), (1, 2, 2), (2, 1, 1)]
    assert of(seq, (16, 16, 16), 2, 8) == seq[:3]                    # gridLevels 3: three restrictions
    assert of(seq, (16, 16, 16), 3, 8) == seq                        # 8 x 2 x 2 = 32 rows > 8
    assert of(seq, (16, 16, 16), 3, 32) == seq[:3]                   # minSize stops the fourth
    assert of(seq[:1], (16, 16, 16), 3, 10 ** 6) == seq[:1]          # the first restriction is always built
    assert of([(2, 2)], (4, 4), 5, 0) == [(2, 2)]                 # nothing left to coarsen: the hierarchy ends


def test_dist_entries_refuse_semicoarsening():
    from openmg_amd import dist
    for value in ("auto", [(1, 2, 2)]):
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.refuse_coarsening(value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.build_all_ranks(None, None, coarsening=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.build_this_rank(None, 0, None, None, coarsening=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.make_tail(None, (8, 8, 8), 2, coarsening=value)
        with pytest.raises(ValueError, match="multi-GPU"):
            dist.RankSetup(None, 0, None, coarsening=value)
    dist.refuse_coarsening(None)
    dist.refuse_coarsening("full")
