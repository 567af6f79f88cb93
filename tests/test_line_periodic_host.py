"""The host side of the line smoother on periodic operators ('smoother': 'line-periodic', OMG_SMOOTH_LINE* |
OMG_SMOOTH_LINE_WRAP) without a GPU: the name and the codes agree with include/openmg_hip.h, parameters['lineAxis'] is
resolved and checked as for 'line', the restatement's line solves (tests/line_periodic_cases.py) agree with dense solves,
and a seam row of operators.stencil7_kappa has the thirteen-slot column order the plan relies on.  CPU only."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators

import line_periodic_cases as lp

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "openmg_hip.h")
BOX, SQUARE = (4, 6, 8), (6, 8)


def test_line_periodic_is_a_smoother_and_other_bad_names_are_not():
    assert _hip.smoother_code("line-periodic") == _hip.SMOOTH_LINE | _hip.SMOOTH_LINE_WRAP == 11
    assert _hip.smoother_code("line") == 3
    for name in ("line-wrap", "periodic", "Line-Periodic", "line_periodic", "zebra"):
        with pytest.raises(ValueError):
            _hip.smoother_code(name)
        with pytest.raises(ValueError) as e:
            openmg_amd.Solver(operators.stencil_poisson(BOX), {"problemShape": BOX, "gridLevels": 1, "smoother": name, "cycles": 2})
        assert not isinstance(e.value, _hip.HipError)


def test_the_codes_are_the_headers():
    text = open(HEADER).read()
    define = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(OMG_\w+)\s+(\d+)\b", text)}
    assert define["OMG_SMOOTH_LINE_WRAP"] == _hip.SMOOTH_LINE_WRAP == 8
    assert (define["OMG_SMOOTH_LINE"], define["OMG_SMOOTH_LINE_X"], define["OMG_SMOOTH_LINE_Y"], define["OMG_SMOOTH_LINE_Z"]) == (3, 4, 5, 6)
    # the flag is a bit none of the smoother codes has
    assert not any(v & 8 for k, v in define.items() if k.startswith("OMG_SMOOTH_") and k != "OMG_SMOOTH_LINE_WRAP")
    # no new C entry, the same options struct
    assert [f[0] for f in _hip.HierarchyOptions._fields_] == ["smoother", "omega", "dtype", "nullspace"]
    assert not [name for name in _hip.SIGNATURES if "wrap" in name or "cyclic" in name]


def test_is_line_smoother_on_both_ranges():
    assert [_hip.is_line_smoother(c) for c in (3, 4, 5, 6, 7)] == [True, True, True, True, False]
    assert [_hip.is_line_smoother(c) for c in (11, 12, 13, 14, 15)] == [True, True, True, True, False]
    assert not any(_hip.is_line_smoother(c) for c in (0, 1, 2, 8, 9, 10, 16, 19, -5, "line-periodic", True, None))


def test_line_smoother_code_with_the_flag():
    code = _hip.line_smoother_code
    for auto in (None, "auto"):
        assert code(auto, BOX, wrap=True) == code(auto, SQUARE, wrap=True) == 11
        assert code(auto, BOX) == code(auto, BOX, wrap=False) == 3
    assert [code(a, BOX, wrap=True) for a in (0, 1, 2)] == [14, 13, 12]
    assert [code(a, SQUARE, wrap=True) for a in (0, 1)] == [13, 12]
    assert [code(a, BOX) for a in (0, 1, 2)] == [6, 5, 4]
    assert code(np.int64(2), BOX, wrap=True) == 12
    # the axis of a named code: strip the flag, then subtract
    assert [(c & ~8) - _hip.SMOOTH_LINE_X for c in (12, 13, 14)] == [0, 1, 2]


def test_line_axis_is_resolved_as_for_line():
    from openmg_amd import _smoother_of
    assert _smoother_of({"smoother": "line-periodic"}) == (11, 1.0)
    assert _smoother_of({"smoother": "line-periodic", "lineAxis": "auto", "problemShape": BOX}) == (11, 1.0)
    assert _smoother_of({"smoother": "line-periodic", "lineAxis": 0, "problemShape": BOX}) == (14, 1.0)
    assert _smoother_of({"smoother": "line-periodic", "lineAxis": 1, "problemShape": SQUARE}) == (12, 1.0)
    assert _smoother_of({"smoother": "line", "lineAxis": 0, "problemShape": BOX}) == (6, 1.0)


@pytest.mark.parametrize("shape,bad", [(BOX, 3), (BOX, -1), (BOX, "q"), (BOX, 1.5), (SQUARE, 2), (BOX, True), (BOX, "x")])
def test_a_bad_line_axis_raises_value_error_before_any_device_work(shape, bad):
    A = operators.stencil_poisson(shape)
    b = np.ones(A.shape[0])
    for run in (lambda p: openmg_amd.mgSolve(A, b, p), lambda p: openmg_amd.Solver(A, p),
                lambda p: openmg_amd.mgCycle([A, A], b, 0, [A], dict(p, coarsestLevel=1, preIterations=1, postIterations=1))):
        p = {"problemShape": shape, "gridLevels": 1, "smoother": "line-periodic", "cycles": 2, "lineAxis": bad}
        with pytest.raises(ValueError) as e:
            run(p)
        assert not isinstance(e.value, _hip.HipError)
        assert "lineAxis" in str(e.value)
    with pytest.raises(ValueError):
        openmg_amd.mgCycle([A, A], b, 0, [A], {"smoother": "line-periodic", "lineAxis": 1, "coarsestLevel": 1, "preIterations": 1,
                                                "postIterations": 1})


@pytest.mark.parametrize("name", ["ringx", "odd", "tiny", "box", "sqring", "sqwrap", "chan"])
def test_the_restated_sweep_solves_its_lines_like_a_dense_solve(name):
    """one colour at a time: the rows of that colour of A x = b hold afterwards, to rounding, and the other colour's
    entries are untouched; and every line's block, taken out densely, gives the same values"""
    pr = lp.problem(name)
    rng = np.random.default_rng(2)
    for level in range(len(pr["R"])):
        A, shape = sp.csr_matrix(pr["A"][level]), pr["shapes"][level]
        n = A.shape[0]
        for axis in lp.admissible_axes(pr):
            T, C, blocks = lp.split(name, level, axis)
            assert abs(T + C - A).max() == 0.0
            b, x0 = rng.standard_normal(n), rng.standard_normal(n)
            x = x0.copy()
            for rows, lu in blocks:
                before = x.copy()
                x[rows] = lu.solve((b - C @ x)[rows])
                other = np.setdiff1d(np.arange(n), rows)
                assert np.array_equal(x[other], before[other])
                scale = float(abs(A).sum(axis=1).max()) * max(1.0, np.abs(x).max())
                assert np.abs((b - A @ x)[rows]).max() <= 1e-12 * lp.line_condition(pr, level, axis) * scale
                # one line of this colour, densely: its cells are the grid line through the colour's first row
                first = np.unravel_index(rows[0], shape)
                cells = np.array([np.ravel_multi_index(first[:axis] + (i,) + first[axis + 1:], shape) for i in range(shape[axis])])
                dense = A[cells][:, cells].toarray()
                assert np.count_nonzero(dense) == (3 * len(cells) if len(cells) >= 3 and axis in lp.periodic_on(pr, level) else 3 * len(cells) - 2)
                want = np.linalg.solve(dense, (b - C @ before)[cells])
                assert np.allclose(x[cells], want, rtol=1e-11, atol=1e-13)
            assert np.array_equal(x, lp.zebra(name, level, axis, b, x0, 1))


@pytest.mark.parametrize("m", [3, 4, 5, 8, 9, 16, 17, 64, 136, 139])
def test_the_cyclic_recurrence_agrees_with_a_dense_solve(m):
    """the LU with a fill row and a fill column that csrc/line.hip stores, transcribed in NumPy: against
    numpy.linalg.solve on strictly dominant blocks and on one of condition ~1e4"""
    rng = np.random.default_rng(m)
    for margin, gate in ((0.5, 1e-13), (1e-4, 1e-10)):
        low, up = -rng.uniform(0.5, 2.0, m), -rng.uniform(0.5, 2.0, m)
        diag = -(low + up) + rng.uniform(margin, 2.0 * margin, m)
        M = np.diag(diag) + np.diag(low[1:], -1) + np.diag(up[:-1], 1)
        M[0, m - 1], M[m - 1, 0] = low[0], up[m - 1]
        r = rng.standard_normal(m)
        x = lp.cyclic_solve(low, diag, up, r)
        want = np.linalg.solve(M, r)
        assert np.abs(x - want).max() <= gate * np.abs(want).max(), (m, margin, np.abs(x - want).max() / np.abs(want).max())


def test_seam_rows_of_stencil7_kappa_have_the_thirteen_slot_order():
    """columns ascending, the wrapped neighbour of a periodic axis between its own in-grid offset and the next axis':
    -(nz-1) sk, -sk, -(ny-1) sj, -sj, -(nx-1), -1, 0, +1, +(nx-1), +sj, +(ny-1) sj, +sk, +(nz-1) sk"""
    nz, ny, nx = shape = (4, 5, 6)
    kappa = np.exp(np.random.default_rng(1).uniform(-0.5, 0.5, (nz + 2, ny + 2, nx + 2)))
    A = sp.csr_matrix(operators.stencil7_kappa(kappa, ("periodic",) * 6))
    assert A.nnz == 7 * A.shape[0] and A.has_sorted_indices
    sj, sk = nx, nx * ny
    slots = [-(nz - 1) * sk, -sk, -(ny - 1) * sj, -sj, -(nx - 1), -1, 0, 1, nx - 1, sj, (ny - 1) * sj, sk, (nz - 1) * sk]
    assert slots == sorted(slots) and len(set(slots)) == 13
    for r in range(A.shape[0]):
        k, j, i = np.unravel_index(r, shape)
        want = [slots[0] if k == nz - 1 else None, slots[1] if k > 0 else None, slots[2] if j == ny - 1 else None,
                slots[3] if j > 0 else None, slots[4] if i == nx - 1 else None, slots[5] if i > 0 else None, 0,
                slots[7] if i < nx - 1 else None, slots[8] if i == 0 else None, slots[9] if j < ny - 1 else None,
                slots[10] if j == 0 else None, slots[11] if k < nz - 1 else None, slots[12] if k == 0 else None]
        got = (A.indices[A.indptr[r]:A.indptr[r + 1]] - r).tolist()
        assert got == [w for w in want if w is not None], (r, got)
    # row 0 holds column (e - 1) s of every periodic axis, and of no other
    walls = ("periodic", "periodic", "dirichlet", "dirichlet", "periodic", "periodic")
    B = sp.csr_matrix(operators.stencil7_kappa(kappa, walls))
    row0 = B.indices[B.indptr[0]:B.indptr[1]].tolist()
    assert (nz - 1) * sk in row0 and (nx - 1) in row0 and (ny - 1) * sj not in row0
    # the scan that reads the grid off the couplings: the first row not coupled to its predecessor is row nx, the first
    # line not coupled to the previous one is line ny — on the periodic pattern as on any other
    has = lambda M, r, c: c in M.indices[M.indptr[r]:M.indptr[r + 1]]
    for M in (A, B):
        assert next(r for r in range(1, M.shape[0]) if not has(M, r, r - 1)) == nx
        assert next(q for q in range(1, nz * ny) if not has(M, q * nx, (q - 1) * nx)) == ny
    # the shared cases' own face operator has the same order
    pr = lp.problem("box")
    assert lp.periodic_on(pr, 0) == (0, 1, 2) and lp.periodic_on(pr, 1) == (0, 1, 2)
    assert lp.periodic_on(lp.problem("chan"), 1) == (0, 2)
