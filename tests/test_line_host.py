"""The zebra line smoother's host side without a GPU: parameters['lineAxis'] is checked before any device work (ValueError,
never HipError), the names and codes agree with include/openmg_hip.h, and 'zebra' is still no smoother.  CPU only."""
import os
import re

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "openmg_hip.h")
BOX, SQUARE = (4, 6, 8), (6, 8)


def params(shape, **kw):
    return dict({"problemShape": shape, "gridLevels": 1, "smoother": "line", "cycles": 2}, **kw)


@pytest.mark.parametrize("shape,bad", [(BOX, 3), (BOX, -1), (BOX, "q"), (BOX, 1.5), (SQUARE, 2), (BOX, True), (BOX, "x")])
def test_a_bad_line_axis_raises_value_error_before_any_device_work(shape, bad):
    A = operators.stencil_poisson(shape)
    b = np.ones(A.shape[0])
    for run in (lambda p: openmg_amd.mgSolve(A, b, p), lambda p: openmg_amd.Solver(A, p),
                lambda p: openmg_amd.mgCycle([A, A], b, 0, [A], dict(p, coarsestLevel=1, preIterations=1, postIterations=1))):
        p = params(shape, lineAxis=bad)
        with pytest.raises(ValueError) as e:
            run(p)
        assert not isinstance(e.value, _hip.HipError)
        assert "lineAxis" in str(e.value)


def test_an_explicit_axis_needs_the_shape_it_indexes():
    A = operators.stencil_poisson(BOX)
    with pytest.raises(ValueError):
        openmg_amd.mgCycle([A, A], np.ones(A.shape[0]), 0, [A], {"smoother": "line", "lineAxis": 1, "coarsestLevel": 1,
                                                                 "preIterations": 1, "postIterations": 1})


@pytest.mark.parametrize("name", ["zebra", "sor", "lines", "Line"])
def test_zebra_is_still_no_smoother(name):
    with pytest.raises(ValueError):
        _hip.smoother_code(name)
    with pytest.raises(ValueError) as e:
        openmg_amd.Solver(operators.stencil_poisson(BOX), params(BOX, smoother=name))
    assert not isinstance(e.value, _hip.HipError)


def test_the_names_and_codes_are_the_headers():
    text = open(HEADER).read()
    define = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(OMG_\w+)\s+(\d+)\b", text)}
    assert define["OMG_SMOOTH_LINE"] == _hip.SMOOTH_LINE == 3
    assert (define["OMG_SMOOTH_LINE_X"], define["OMG_SMOOTH_LINE_Y"], define["OMG_SMOOTH_LINE_Z"]) \
        == (_hip.SMOOTH_LINE_X, _hip.SMOOTH_LINE_Y, _hip.SMOOTH_LINE_Z) == (4, 5, 6)
    assert define["OMG_LEVEL_LINE"] == 2048
    # a free bit: no other level flag has it
    assert [k for k, v in define.items() if k.startswith("OMG_LEVEL_") and v & 2048] == ["OMG_LEVEL_LINE"]
    assert _hip.smoother_code("line") == _hip.SMOOTH_LINE == _hip.smoother_code("line-gs")
    assert "omg_hierarchy_line_axis" in _hip.SIGNATURES
    # the struct keeps its layout
    assert [f[0] for f in _hip.HierarchyOptions._fields_] == ["smoother", "omega", "dtype", "nullspace"]


def test_line_axis_is_an_index_into_the_shape_in_c_order():
    code = _hip.line_smoother_code
    for auto in (None, "auto"):
        assert code(auto, BOX) == code(auto, SQUARE) == _hip.SMOOTH_LINE
    # the last entry of problemShape is the unit-stride axis X, the first the slowest
    assert [code(a, BOX) for a in (0, 1, 2)] == [_hip.SMOOTH_LINE_Z, _hip.SMOOTH_LINE_Y, _hip.SMOOTH_LINE_X]
    assert [code(a, SQUARE) for a in (0, 1)] == [_hip.SMOOTH_LINE_Y, _hip.SMOOTH_LINE_X]
    assert code(np.int64(2), BOX) == _hip.SMOOTH_LINE_X
    assert all(_hip.is_line_smoother(c) for c in (3, 4, 5, 6)) and not any(_hip.is_line_smoother(c) for c in (0, 1, 2, 7, "line"))


def test_other_smoothers_never_read_line_axis():
    from openmg_amd import _smoother_of
    assert _smoother_of({"smoother": "colour", "lineAxis": "nonsense"}) == (_hip.SMOOTH_GS_COLOUR, 1.0)
    assert _smoother_of({"smoother": "line"}) == (_hip.SMOOTH_LINE, 1.0)
    assert _smoother_of({"smoother": "line", "lineAxis": 0, "problemShape": BOX}) == (_hip.SMOOTH_LINE_Z, 1.0)
