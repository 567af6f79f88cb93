"""openmg_amd.Solver without a GPU: the keys are checked before any device work (ValueError, never HipError), the stop
target is a pure function, and the shared loops stop at the first norm below it.  CPU only."""
import numpy as np
import pytest

import openmg
import openmg_amd
from openmg_amd import _hip, _solver, operators

SHAPE = (8, 8, 8)
PARAMS = {"problemShape": SHAPE, "gridLevels": 2, "smoother": "colour", "cycles": 3}


@pytest.mark.parametrize("bad", [{"accel": "x"}, {"cycle": "Q"}, {"overCorrection": 0}, {"nullspace": "y"}, {"dtype": "float16"},
                                 {"dtype": "no such type"}, {"smoother": "zebra"}, {"rtol": -1.0}, {"rtol": float("nan")}])
def test_invalid_keys_raise_value_error_before_any_device_work(bad):
    A = operators.stencil_poisson(SHAPE)
    p = dict(PARAMS, **bad)
    given = dict(p)
    with pytest.raises(ValueError) as e:
        openmg_amd.Solver(A, p)
    assert not isinstance(e.value, _hip.HipError)
    assert p == given and "coarsestLevel" not in p


def test_solver_is_exported_by_both_packages_and_leaves_the_defaults_alone():
    assert "Solver" in openmg_amd.__all__ and openmg.Solver is openmg_amd.Solver
    before = dict(openmg_amd.defaults)
    try:
        openmg_amd.Solver(operators.stencil_poisson(SHAPE), dict(PARAMS)).close()
    except _hip.HipError:
        pass                                      # (no GPU: the setup itself is refused, after the checks)
    assert openmg_amd.defaults == before


def test_stop_target():
    t = _solver.stop_target
    assert t(0, 0.5, 0.0, 100.0) == 0.5                       # threshold alone
    assert t(0, 0.0, 1e-3, 100.0) == 0.1                      # rtol alone: relative to ||b||
    assert t(0, 0.5, 1e-3, 100.0) == 0.5 and t(0, 0.05, 1e-3, 100.0) == 0.1      # the larger of the two
    assert t(7, 0.0, 0.0, 100.0) == 0.0 and t(7, -1.0, 0.0, 100.0) == 0.0        # count only
    assert t(0, 0.5, 1e-3, float("nan")) == 0.5              # (a right-hand side that is not finite: the cycles report it)
    assert t(3, 0.0, 0.0) is None                             # the check alone
    for cycles, threshold, rtol in ((0, 0.0, 0.0), (0, -1.0, 0.0), (-2, 0.0, 0.0)):
        with pytest.raises(ValueError):
            t(cycles, threshold, rtol)
    for rtol in (-1e-3, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError):
            t(5, 0.0, rtol)


class ScriptedHierarchy:
    """the resident entries the loops call, returning scripted norms"""

    def __init__(self, norms):
        self.norms, self.k = list(norms), 0

    def resident_cycle(self, pre, post):
        self.k += 1
        return self.norms[self.k - 1]

    def resident_cycles(self, pre, post, n):
        self.k += n
        return self.norms[self.k - n:self.k]

    def resident_pcg(self, pre, post, max_iter, threshold):
        out = []
        while len(out) < max_iter:
            out.append(self.norms[self.k])
            self.k += 1
            if threshold > 0 and out[-1] < threshold:
                break
        return len(out), np.array(out), out[-1], False


NORMS = [8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.125]


@pytest.mark.parametrize("loop", [openmg_amd._solve_cycles, openmg_amd._solve_cg])
def test_the_loops_stop_at_the_first_norm_below_the_target_and_report_every_norm(loop):
    for threshold, rtol, first in ((1.5, 0.0, 4), (0.0, 0.1, 5), (1.5, 0.1, 4), (0.3, 0.5, 2)):
        target = _solver.stop_target(0, threshold, rtol, 10.0)
        assert first == 1 + next(k for k, v in enumerate(NORMS) if v < target)
        seen = []
        done, norm = loop(ScriptedHierarchy(NORMS), {"cycles": 0, "threshold": target}, 1, 1, 2, False, "V",
                          lambda k, v: seen.append((k, v)))
        assert done == first and norm == NORMS[first - 1]
        assert seen == [(k + 1, NORMS[k]) for k in range(first)]
    # a count caps it, with and without a target
    for cycles, target, want in ((3, 0.0, 3), (3, 0.3, 3), (6, 1.5, 4)):
        seen = []
        done, _ = loop(ScriptedHierarchy(NORMS), {"cycles": cycles, "threshold": target}, 1, 1, 2, False, "V",
                       lambda k, v: seen.append(k))
        assert done == want and seen == list(range(1, want + 1))
    # without an observer: mgSolve's own call
    assert loop(ScriptedHierarchy(NORMS), {"cycles": 0, "threshold": 1.5}, 1, 1, 2, False)[0] == 4
