"""The mixed-precision dtype without a GPU: its code, mgCycle's refusal before any device work (also at the coarsest level,
where mgCycle would otherwise solve on the host), and the header's constant."""
import os
import re

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_code():
    assert _hip.dtype_code("mixed") == _hip.DTYPE_MIXED == 2
    assert _hip.dtype_code(2) == 2
    assert _hip.dtype_code("float32") == 1 and _hip.dtype_code("float64") == 0
    with pytest.raises(ValueError):
        _hip.dtype_code("float16")


@pytest.mark.parametrize("level", [0, 1])
def test_mgcycle_refuses_mixed(level):
    shape = (8, 8, 8)
    A0 = operators.stencil_poisson(shape)
    R = orc.restriction_list(shape, 1, 2)
    A = orc.coefficient_list(A0, R)
    b = np.ones(A[level].shape[0])
    p = {"coarsestLevel": 1, "preIterations": 1, "postIterations": 1, "dtype": "mixed"}
    with pytest.raises(ValueError, match="mgSolve"):
        openmg_amd.mgCycle(A, b, level, R, p)


def test_header_defines_mixed():
    with open(os.path.join(ROOT, "include", "openmg_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+OMG_DTYPE_MIXED\s+2\b", text)
