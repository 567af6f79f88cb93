"""parameters['cycle'] / parameters['overCorrection'] without a GPU: bad values are refused before any device work, the
C ABI carries the two new entries, and the restatement of tests/test_gpu_cycle_shapes.py visits the levels as often as
an F- / W-cycle must (level l, 1 <= l < L: l + 1 / 2^l times; the coarsest level L: L / 2^(L-1) times; V: once)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small():
    shape = (8, 8, 8)
    A0 = operators.stencil_poisson(shape)
    return shape, A0, np.ones(A0.shape[0])


BAD = [{"cycle": "X"}, {"cycle": "f"}, {"cycle": 1}, {"cycle": None},
       {"overCorrection": 0}, {"overCorrection": -1}, {"overCorrection": float("nan")}, {"overCorrection": float("inf")},
       {"cycle": "F", "overCorrection": -0.5}, {"overCorrection": "much"}]


@pytest.mark.parametrize("bad", BAD)
def test_mgsolve_refuses_bad_values_before_any_device_work(bad):
    shape, A0, b = small()
    p = {"problemShape": shape, "gridLevels": 2, "cycles": 3, "threshold": 0.0}
    p.update(bad)
    with pytest.raises(ValueError, match="cycle|overCorrection"):
        openmg_amd.mgSolve(A0, b, p)


@pytest.mark.parametrize("bad", BAD)
def test_mgcycle_refuses_bad_values_before_any_device_work(bad):
    shape, A0, b = small()
    R = orc.restriction_list(shape, 0, 1)
    A = orc.coefficient_list(A0, R)
    p = {"coarsestLevel": len(R), "preIterations": 1, "postIterations": 1}
    p.update(bad)
    with pytest.raises(ValueError, match="cycle|overCorrection"):
        openmg_amd.mgCycle(A, b, 0, R, p)


def test_good_values_are_accepted_by_the_checks():
    assert openmg_amd._cycle_of({}) == ("V", 1.0)
    assert openmg_amd._cycle_of({"cycle": "W", "overCorrection": 1.8}) == ("W", 1.8)
    assert openmg_amd._cycle_of({"cycle": "F", "overCorrection": np.float32(1.5)}) == ("F", 1.5)
    assert [_hip.cycle_code(s) for s in "VFW"] == [_hip.CYCLE_V, _hip.CYCLE_F, _hip.CYCLE_W]


def test_the_c_abi_carries_the_two_entries():
    header = open(os.path.join(ROOT, "include", "openmg_hip.h")).read()
    for name in ("omg_hierarchy_set_cycle", "omg_hierarchy_get_cycle"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _hip.SIGNATURES
        assert hasattr(_hip.lib(), name), name
    for name, value in (("OMG_CYCLE_V", _hip.CYCLE_V), ("OMG_CYCLE_F", _hip.CYCLE_F), ("OMG_CYCLE_W", _hip.CYCLE_W)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert len(_hip.SIGNATURES["omg_hierarchy_set_cycle"][1]) == 3 and len(_hip.SIGNATURES["omg_hierarchy_get_cycle"][1]) == 3


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_the_restatement_visits_the_levels_as_the_table_says(L):
    from test_gpu_cycle_shapes import prolongations, restated_cycle
    n = 256
    A0 = sp.csr_matrix(orc.poisson((n,), sparse=True))
    R = orc.restriction_list((n,), L - 1, 1)
    A = orc.coefficient_list(A0, R)
    assert len(R) == L
    b = A0 @ np.random.default_rng(1).random(n)
    P = prolongations(R, 1.8)
    for shape in "VFW":
        count = {}
        x = restated_cycle(A, R, P, b, 0, L, 1, 1, shape, None, None, count)
        assert np.isfinite(x).all()
        want = {0: 1}
        for l in range(1, L):
            want[l] = {"V": 1, "F": l + 1, "W": 2 ** l}[shape]
        want[L] = {"V": 1, "F": L, "W": 2 ** (L - 1)}[shape]
        assert count == want, (shape, L, count, want)


def test_the_restatement_with_v_and_factor_one_is_the_oracle_cycle():
    from test_gpu_cycle_shapes import prolongations, restated_cycle
    shape = (8, 8, 8)
    A0 = operators.stencil_poisson(shape)
    R = orc.restriction_list(shape, 0, 1)
    A = orc.coefficient_list(A0, R)
    b = A0 @ np.random.default_rng(2).random(A0.shape[0])
    sm = orc.make_smoother("colour", A)
    x0 = np.random.default_rng(3).random(b.size)
    want, _ = orc.mg_cycle(A, b, 0, R, {"coarsestLevel": len(R), "preIterations": 1, "postIterations": 1}, initial=x0.copy(), smoother=sm)
    got = restated_cycle(A, R, prolongations(R, 1.0), b, 0, len(R), 1, 1, "V", sm, x0)
    assert np.array_equal(got, want)


def test_the_progress_lines_follow_the_recursion(capsys):
    openmg_amd._announce_descent(3, "F")
    got = capsys.readouterr().out.splitlines()
    assert got == ["calling mgCycle at level 0",
                   " calling mgCycle at level 1", "  calling mgCycle at level 2", "   direct solving at level 3",
                   "  calling mgCycle at level 2", "   direct solving at level 3",
                   " calling mgCycle at level 1", "  calling mgCycle at level 2", "   direct solving at level 3"]
    openmg_amd._announce_descent(3, "V")
    assert capsys.readouterr().out.splitlines() == ["calling mgCycle at level 0", " calling mgCycle at level 1",
                                                    "  calling mgCycle at level 2", "   direct solving at level 3"]
