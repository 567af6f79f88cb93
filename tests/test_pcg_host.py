"""mgSolve's 'accel' key without a GPU: a value other than None / 'cg' is refused before any device work; and the CPU
yardstick of tests/test_gpu_pcg.py (FCG(1) around the oracle's V-cycle) needs fewer iterations than plain cycles."""
import numpy as np
import pytest

import openmg_amd
from openmg_amd import operators
from oracle import mg_oracle as orc


def test_unknown_accel_is_a_value_error_before_any_device_work():
    A0 = operators.stencil_poisson((8, 8, 8))
    b = np.ones(A0.shape[0])
    p = {"problemShape": (8, 8, 8), "gridLevels": 2, "cycles": 3, "threshold": 0.0, "accel": "bicgstab"}
    with pytest.raises(ValueError, match="accel"):
        openmg_amd.mgSolve(A0, b, p)
    with pytest.raises(ValueError, match="accel"):
        openmg_amd.mgSolve(A0, b, dict(p, accel="CG"))


def test_yardstick_beats_plain_cycles():
    from test_gpu_pcg import fcg_cpu
    shape = (16, 16, 16)
    A0 = operators.stencil_poisson(shape)
    R = orc.restriction_list(shape, 2, 8)
    A = orc.coefficient_list(A0, R)
    b = np.random.default_rng(7).standard_normal(A0.shape[0])
    tol = 1e-8 * np.linalg.norm(b)
    norms, x = fcg_cpu(A, R, b, "colour", 1, 1, tol, 100)
    assert norms[-1] < tol and np.linalg.norm(b - A0 @ x) < 2 * tol
    sm = orc.make_smoother("colour", A)
    par = {"coarsestLevel": len(R), "preIterations": 1, "postIterations": 1}
    xo, plain = None, 0
    while plain < 3 * len(norms):
        xo, info = orc.mg_cycle(A, b, 0, R, par, initial=xo, smoother=sm)
        plain += 1
        if info["norm"] < tol:
            break
    assert len(norms) < plain, (len(norms), plain)
