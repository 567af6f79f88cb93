"""Fischer's projection onto earlier solutions as tests/projection_cases.py restates it — the definition
openmg_amd.Solver(..., projection=L) is held to on the GPU (tests/test_gpu_projection.py) — with SciPy direct solves in the
place of the multigrid solve, and the argument check of Solver's `projection`.  CPU only."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import openmg_amd
from projection_cases import Projection, gram_error, operator, rhs

SHAPE = (16, 16, 16)


@pytest.fixture(scope="module")
def direct():
    lu = spla.splu(operator(SHAPE).tocsc())
    return lambda b, start: (lu.solve(b), 1)


def test_set_stays_a_orthonormal_and_restarts_exactly_when_full(direct):
    A = operator(SHAPE)
    P = Projection(A, 4)
    sizes, used = [], []
    for t in range(20):
        b = rhs(SHAPE, t)
        x, cycles, n_used, kept = P.solve(b, direct)
        assert kept and np.linalg.norm(b - A @ x) <= 1e-12 * np.linalg.norm(b)
        err = P.gram_error()
        print("step %2d: used %d, size %d, max |X^T A X - I| = %.2e" % (t, n_used, len(P.X), err))
        assert err <= 1e-12
        sizes.append(len(P.X))
        used.append(n_used)
    assert sizes == [1, 2, 3, 4] * 5
    assert used == [0, 1, 2, 3] + [4, 1, 2, 3] * 4      # (the step that finds the set full still starts from all of it)
    assert P.restarts == 4


def test_right_hand_side_in_a_times_span_is_reproduced(direct):
    A = operator(SHAPE)
    P = Projection(A, 8)
    for t in range(5):
        P.solve(rhs(SHAPE, t), direct)
    assert len(P.X) == 5
    c = np.array([0.7, -1.3, 2.1, 0.05, -0.4])
    want = c @ np.stack(P.X)
    start, alpha = P.project(A @ want)
    assert np.abs(np.array(alpha) - c).max() <= 1e-12 * np.abs(c).max()
    assert np.abs(start - want).max() <= 1e-12 * np.abs(want).max()


def test_repeated_direction_is_dropped_by_the_2_to_minus_26_rule(direct):
    A = operator(SHAPE)
    P = Projection(A, 8)
    for t in range(3):
        P.solve(rhs(SHAPE, t), direct)
    before = [x.copy() for x in P.X]
    start, alpha = P.project(rhs(SHAPE, 3))
    # a solve that moved along directions the set already holds: what is left after the orthogonalisation is rounding
    assert not P.update(start + 0.5 * P.X[0] - 0.25 * P.X[2], alpha)
    assert len(P.X) == 3 and all(np.array_equal(a, b) for a, b in zip(before, P.X))
    # a direction with a part of 1e-3 outside the span keeps (1e-3)^2 of its energy, far above 2^-26: kept
    fresh = direct(rhs(SHAPE, 7), None)[0]
    fresh = fresh - sum((x @ (A @ fresh)) * x for x in P.X)
    fresh /= np.sqrt(fresh @ (A @ fresh))
    assert P.update(start + P.X[1] + 1e-3 * fresh, alpha) and len(P.X) == 4
    assert gram_error(P.X, A) <= 1e-12
    # ... and one with a part of 1e-5 keeps 1e-10 < 2^-26 = 1.5e-8: dropped
    start, alpha = P.project(rhs(SHAPE, 3))
    other = direct(rhs(SHAPE, 11), None)[0]
    other = other - sum((x @ (A @ other)) * x for x in P.X)
    other /= np.sqrt(other @ (A @ other))
    assert not P.update(start + P.X[1] + 1e-5 * other, alpha) and len(P.X) == 4


def test_a_solve_that_ran_no_cycle_adds_nothing(direct):
    A = operator(SHAPE)
    P = Projection(A, 4)
    P.solve(rhs(SHAPE, 0), direct)
    x, cycles, used, kept = P.solve(rhs(SHAPE, 1), lambda b, start: (start, 0))
    assert (cycles, used, kept, len(P.X)) == (0, 1, False, 1)


@pytest.mark.parametrize("bad", [-1, 65, "x", 1.5, True])
def test_solver_refuses_a_bad_capacity_before_any_device_work(bad, monkeypatch):
    def no_setup(*a, **k):
        raise AssertionError("the setup ran")

    monkeypatch.setattr(openmg_amd, "_setup", no_setup)
    p = {"problemShape": SHAPE, "gridLevels": 3, "cycles": 1}
    with pytest.raises(ValueError, match="projection"):
        openmg_amd.Solver(operator(SHAPE), p, projection=bad)
    from projection_cases import kappa_field
    with pytest.raises(ValueError, match="projection"):
        openmg_amd.Solver.from_kappa(kappa_field(SHAPE), {"gridLevels": 3, "cycles": 1}, projection=bad)
