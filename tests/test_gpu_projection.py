"""openmg_amd.Solver(..., projection=L): every solve starts from the projection of its solution onto up to L earlier ones,
kept in HBM as an A-orthonormal set (csrc/project.hip).

Yardsticks: the SciPy matrix of the operator on the host — the set's Gram matrix, every solve's residual, the projected
start formed again in NumPy from the fetched set —, a solver built without the argument (off is off, bit for bit), a fresh
solver (clearing), and the same sequence warm-started from the previous solution (fewer cycles).  The problems are those of
tests/projection_cases.py: kappa = exp(U(-1, 1)), a right-hand side of six smooth modes with slowly turning amplitudes plus
fixed noise.  Needs an MI355X: run with -m gpu."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import operators
from projection_cases import gram_error, kappa_field, operator, rhs

pytestmark = pytest.mark.gpu

RAGGED = (10, 6, 14)            # n = 840: 420 chunks of 16 bytes in double — two workgroups — and 210 in float; 2 grids
CUBE = (16, 16, 16)
NEUMANN = ("neumann",) * 6


def params(shape, grids, **kw):
    p = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "cycles": 200,
         "threshold": 0.0, "rtol": 1e-8, "smoother": "colour", "minSize": 1}
    p.update(kw)
    return p


def residual_bound(b, rtol):
    """What ||b - A u|| by SciPy may be when the device stopped below rtol ||b||, on every kind of hierarchy"""
    return 1.001 * rtol * np.linalg.norm(b)


def run_sequence(A, shape, p, capacity, steps, check=True, nullspace=False):
    """`steps` solves of the drifting b on a fresh solver; with check every solve's residual, the set's Gram matrix and its
    size are held to the yardsticks.  Returns the list of (u, info)."""
    dtype = p.get("dtype", "float64")
    gram_tol = 1e-4 if dtype == "float32" else 1e-10
    out = []
    with openmg_amd.Solver(A, p, projection=capacity) as s:
        assert s.projection_size == 0 and s.projection_basis() == []
        for t in range(steps):
            b = rhs(shape, t)
            u, info = s.solve(b)
            out.append((u, info))
            if not check:
                continue
            bp = b - b.mean() if nullspace else b
            res = np.linalg.norm(bp - A @ u)
            X = s.projection_basis()
            err = gram_error(X, A)
            print("  step %2d: projected %d, basis %d, cycles %3d, start %.2e ||b||, residual %.3e (bound %.3e), max |X^T A X - I| = %.2e"
                  % (t, info["projected"], info["basis"], info["cycle"], info["initial_norm"] / info["rhs_norm"], res,
                     residual_bound(bp, p["rtol"]), err))
            assert res <= residual_bound(bp, p["rtol"])
            assert info["cycle"] > 0
            assert info["basis"] == s.projection_size == len(X) == t % capacity + 1        # 1, 2, ..., L, 1, 2, ...
            assert info["projected"] == (0 if t == 0 else (t - 1) % capacity + 1)
            assert err <= gram_tol
            if nullspace:
                assert abs(u.mean()) <= 1e-12 * np.abs(u).max()
                for x in X:
                    assert abs(x.mean()) <= 1e-12 * np.abs(x).max()
    return out


# ------------------------------------------------------------------------------ 1. off is off --
def test_projection_0_and_an_empty_set_have_the_bits_of_the_plain_solver():
    A, p = operator(CUBE), params(CUBE, 3)
    b = rhs(CUBE, 0)
    with openmg_amd.Solver(A, p) as s:
        want, winfo = s.solve(b)
        want_cg, wcg = s.solve(b, accel="cg")
    for off in (0, None):
        with openmg_amd.Solver(A, p, projection=off) as s:
            u, info = s.solve(b)
            assert np.array_equal(u, want) and info == winfo
            assert s.projection_size == 0 and s.projection_basis() == []
    with openmg_amd.Solver(A, p, projection=4) as s:
        u, info = s.solve(b)                                # (the set is empty: today's zero-start path)
        assert np.array_equal(u, want) and (info.pop("projected"), info.pop("basis")) == (0, 1) and info == winfo
        u, info = s.solve(b, project=False, accel="cg")     # (project=False: the plain solve, the set left alone)
        assert np.array_equal(u, want_cg) and (info.pop("projected"), info.pop("basis")) == (0, 1) and info == wcg
        assert s.projection_size == 1


# --------------------------------------------------------------------------------- 2. the set --
@pytest.mark.parametrize("capacity", [1, 4, 5, 8])
@pytest.mark.parametrize("shape, grids", [(RAGGED, 2), (CUBE, 3)])
def test_set_is_a_orthonormal_and_restarts_when_full(shape, grids, capacity):
    run_sequence(operator(shape), shape, params(shape, grids), capacity, 10)


# ------------------------------------------------------------------------ 3. Solver.project --
@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_project_is_the_sum_over_the_fetched_set(dtype):
    """(b, the set and the sum are double on both hierarchies; on an fp32 one b and the set are float, and no gate of
    1e-9 applies)"""
    A = operator(RAGGED)
    p = params(RAGGED, 2, dtype=dtype)
    with openmg_amd.Solver(A, p, projection=8) as s:
        assert np.array_equal(s.project(rhs(RAGGED, 0)), np.zeros(A.shape[0]))          # (an empty set)
        for t in range(5):
            s.solve(rhs(RAGGED, t))
        X = s.projection_basis()
        assert len(X) == 5
        b = rhs(RAGGED, 9)
        want = sum((x @ b) * x for x in X)
        got = s.project(b)
        diff = np.abs(got - want).max()
        gate = 1e-9 * np.abs(want).max()                    # (the iterate gate)
        print("  %s: max |project(b) - sum (x_i . b) x_i| = %.2e (gate %.2e)" % (dtype, diff, gate))
        assert diff <= gate
        out = np.empty(A.shape[0])
        assert s.project(b, out=out) is out and np.array_equal(out, got)
        assert s.projection_size == 5 and all(np.array_equal(a, c) for a, c in zip(X, s.projection_basis()))
        # the probe's timing entry runs the same launches and leaves the set and the next projection as they were
        s.hierarchy.resident_load(b)
        assert all(ms > 0.0 for ms in s.hierarchy.projection_time(2))
        assert np.array_equal(s.project(b), got) and all(np.array_equal(a, c) for a, c in zip(X, s.projection_basis()))


# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as in tests/test_gpu_solver.py)
DEVICE_ARRAYS = """
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import openmg_amd
from projection_cases import operator, rhs
shape = (10, 6, 14)
A = operator(shape)
p = {"problemShape": shape, "gridLevels": 1, "preIterations": 1, "postIterations": 1, "cycles": 200, "threshold": 0.0,
     "rtol": 1e-8, "smoother": "colour", "minSize": 1}
with openmg_amd.Solver(A, p, projection=4) as sh, openmg_amd.Solver(A, p, projection=4) as sd:
    for t in range(6):
        b = rhs(shape, t)
        uh, ih = sh.solve(b)
        ud, idv = sd.solve(torch.tensor(b, device="cuda"))
        assert isinstance(ud, torch.Tensor) and np.array_equal(ud.cpu().numpy(), uh) and idv == ih, t
    b = rhs(shape, 9)
    want = sh.project(b)
    bd = torch.tensor(b, device="cuda")
    got = sd.project(bd)
    assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    out = torch.empty_like(bd)
    assert sd.project(bd, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(bd.cpu().numpy(), b)
    try:
        sd.project(b, out=out)
    except TypeError:
        pass
    else:
        raise AssertionError("a device `out` with a host `b` was accepted")
print("device arrays ok")
"""


def test_device_arrays_have_the_bits_of_the_host_calls():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "device arrays ok" in p.stdout, p.stderr[-3000:]


# -------------------------------------------------------------------------------- 4. exactness --
def test_a_multiple_of_an_earlier_right_hand_side_needs_no_cycle():
    A, p = operator(CUBE), params(CUBE, 3)
    b1 = rhs(CUBE, 0)
    with openmg_amd.Solver(A, p, projection=4) as s:
        s.solve(b1)
        X = s.projection_basis()
        u, info = s.solve(2.5 * b1, rtol=1e-6)
        print("  start %.3e ||b||" % (info["initial_norm"] / info["rhs_norm"]))
        assert info["cycle"] == 0 and info["projected"] == 1 and info["basis"] == 1 and info["norms"] == []
        assert info["norm"] == info["initial_norm"]
        assert np.linalg.norm(2.5 * b1 - A @ u) <= 1.001 * 1e-6 * np.linalg.norm(2.5 * b1)
        after = s.projection_basis()
        assert len(after) == 1 and np.array_equal(after[0], X[0])


# ----------------------------------------------------------------- 5. fewer cycles, determinism --
@functools.lru_cache(maxsize=None)
def sixteen_steps():
    return run_sequence(operator(CUBE), CUBE, params(CUBE, 3), 8, 16)


def test_fewer_cycles_than_a_warm_start():
    """16^3, 3 grids, 'colour', V(1,1), rtol 1e-8, L = 8, 16 steps: the total over the sequence, never per step (the step
    after a restart may cost a cycle more).  The CPU restatement of tests/projection_cases.py around the CPU cycle gives
    220 / 413 = 0.53 with the lexicographic smoother and 235 / 439 = 0.535 with the colour smoother."""
    A, p = operator(CUBE), params(CUBE, 3)
    projected = sum(info["cycle"] for _, info in sixteen_steps())
    warm, u_prev = 0, None
    with openmg_amd.Solver(A, p) as s:
        for t in range(16):
            u_prev, info = s.solve(rhs(CUBE, t), initial=u_prev)
            warm += info["cycle"]
    print("  cycles over 16 steps: projected %d, warm-started %d, ratio %.3f" % (projected, warm, projected / warm))
    assert projected <= 0.8 * warm


def test_the_sequence_has_the_same_bits_in_two_fresh_solvers():
    again = run_sequence(operator(CUBE), CUBE, params(CUBE, 3), 8, 16, check=False)
    for (u, info), (v, jnfo) in zip(sixteen_steps(), again):
        assert np.array_equal(u, v) and info == jnfo


# ------------------------------------------------------------------------------------ 6. paths --
@pytest.mark.parametrize("name, kw", [
    ("cg", {"accel": "cg"}),
    ("float32", {"dtype": "float32", "rtol": 1e-3}),
    ("float32 cg", {"dtype": "float32", "rtol": 1e-3, "accel": "cg"}),
    ("mixed", {"dtype": "mixed"}),
    ("mixed cg", {"dtype": "mixed", "accel": "cg"}),
    ("F 1.8", {"cycle": "F", "overCorrection": 1.8}),
    ("F 1.8 cg", {"cycle": "F", "overCorrection": 1.8, "accel": "cg"}),
])
def test_paths_on_the_variable_coefficient_operator(name, kw):
    run_sequence(operator(CUBE), CUBE, params(CUBE, 3, **kw), 4, 6)


@pytest.mark.parametrize("shape, kw", [
    (CUBE, {"smoother": "line"}),
    (CUBE, {"coarsening": "auto"}),
    ((9, 10, 7), {"oddExtents": "merge"}),
], ids=["line", "coarsening-auto", "oddExtents-merge"])
def test_the_other_kinds_of_hierarchy(shape, kw):
    """(nothing in the projection depends on the level kinds: the line smoother, a semicoarsened hierarchy, a merged odd extent)"""
    run_sequence(operator(shape), shape, params(shape, 3, **kw), 4, 6)


@pytest.mark.parametrize("kw", [{}, {"accel": "cg"}, {"dtype": "mixed"}])
def test_constant_null_space_on_the_all_neumann_operator(kw):
    A = operator(CUBE, NEUMANN)
    assert np.abs(A @ np.ones(A.shape[0])).max() <= 1e-12 * abs(A).max()
    run_sequence(A, CUBE, params(CUBE, 3, nullspace="constant", **kw), 4, 6, nullspace=True)


@pytest.mark.parametrize("kw", [{}, {"accel": "cg"}, {"dtype": "mixed"}, {"dtype": "float32", "rtol": 1e-3}])
def test_constant_coefficient_poisson_on_the_fused_passes(kw):
    shape = (32, 32, 32)
    A = operators.stencil_poisson(shape)
    p = params(shape, 3, **kw)
    with openmg_amd.Solver(A, p) as s:
        flags = [s.hierarchy.level_flags(l) for l in range(2)]
        print("  level flags:", [[k for k, v in f.items() if v] for f in flags])
        assert flags[0]["plane"]
    run_sequence(A, shape, p, 4, 6)


@pytest.mark.parametrize("var7", [False, True])
def test_variable_coefficient_levels_run_the_row_kernels_or_var7(var7, monkeypatch):
    """(the other tests on the variable-coefficient operator run level 0 on the row kernels: 16^3 is below the size from
    which a level takes the var7 passes, unless OMG_VAR7_MIN says otherwise)"""
    if var7:
        monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    p = params(CUBE, 3)
    with openmg_amd.Solver(operator(CUBE), p) as s:
        flags = s.hierarchy.level_flags(0)
        print("  level 0 flags:", [k for k, v in flags.items() if v])
        assert flags["var7"] == var7 and not flags["plane"]
    run_sequence(operator(CUBE), CUBE, p, 4, 6)


# --------------------------------------------------------------------- 7. clearing and errors --
def fresh_solve(A, p, b):
    with openmg_amd.Solver(A, p) as s:
        return s.solve(b)


@pytest.mark.parametrize("in_place", [True, False])
def test_update_empties_the_set(in_place, monkeypatch):
    """in place: level 0 on the var7 passes (update_fine); rebuilt: the lexicographic smoother (a new hierarchy)"""
    if in_place:
        monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    A = operator(CUBE)
    A_new = operators.stencil7_kappa(kappa_field(CUBE) * 1.5 + 0.25)
    A_new.sort_indices()
    p = params(CUBE, 3, smoother="colour" if in_place else "gs")
    b = rhs(CUBE, 3)
    want, winfo = fresh_solve(A_new, p, b)
    with openmg_amd.Solver(A, p, projection=4) as s:
        assert s.hierarchy.can_update_fine() == in_place
        for t in range(3):
            s.solve(rhs(CUBE, t))
        assert s.projection_size == 3
        s.update(A_new)
        assert s.projection_size == 0 and s.projection_basis() == []
        u, info = s.solve(b)
        assert (info.pop("projected"), info.pop("basis")) == (0, 1)
        assert np.array_equal(u, want) and info == winfo
        # ... and the set of the new operator is orthonormal for the new operator
        s.solve(rhs(CUBE, 4))
        assert s.projection_size == 2 and gram_error(s.projection_basis(), A_new) <= 1e-10
        s.projection_clear()
        assert s.projection_size == 0
        u, info = s.solve(b)
        assert np.array_equal(u, want) and info["projected"] == 0


@pytest.mark.parametrize("in_place", [True, False])
def test_update_kappa_empties_the_set(in_place, monkeypatch):
    if in_place:
        monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    kappa = kappa_field(CUBE)
    p = params(CUBE, 3)
    p.pop("problemShape")
    b = rhs(CUBE, 3)
    with openmg_amd.Solver.from_kappa(kappa * 1.5 + 0.25, p) as s:
        want, winfo = s.solve(b)
    with openmg_amd.Solver.from_kappa(kappa, p, projection=4) as s:
        assert s.hierarchy.can_update_fine() == in_place
        for t in range(3):
            s.solve(rhs(CUBE, t))
        assert s.projection_size == 3
        s.update_kappa(kappa * 1.5 + 0.25)
        assert s.projection_size == 0
        u, info = s.solve(b)
        assert (info.pop("projected"), info.pop("basis")) == (0, 1)
        assert np.array_equal(u, want) and info == winfo


def test_argument_errors_and_a_closed_solver():
    A, p = operator(RAGGED), params(RAGGED, 2)
    b = rhs(RAGGED, 0)
    s = openmg_amd.Solver(A, p, projection=2)
    with pytest.raises(ValueError, match="initial"):
        s.solve(b, initial=np.zeros(b.size))
    with pytest.raises(ValueError, match="initial"):
        s.solve(b, initial=np.zeros(b.size), project=True)
    u, info = s.solve(b, initial=np.zeros(b.size), project=False)
    assert s.projection_size == 0 and info["projected"] == 0 and info["basis"] == 0
    plain = openmg_amd.Solver(A, p)
    with pytest.raises(ValueError, match="projection"):
        plain.solve(b, project=True)
    with pytest.raises(ValueError, match="projection"):
        plain.project(b)
    assert plain.projection_size == 0 and plain.projection_basis() == []
    plain.projection_clear()
    assert np.array_equal(plain.solve(b, project=False)[0], u)
    plain.close()
    s.close()
    for call in (lambda: s.project(b), lambda: s.projection_size, s.projection_clear, s.projection_basis, lambda: s.solve(b)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_the_entries_refuse_what_they_cannot_do():
    import scipy.sparse as sp
    from openmg_amd import _hip
    # a single-level hierarchy solves directly and keeps no set
    with _hip.Hierarchy([sp.identity(8, format="csr") * 2.0], [], smoother="gs") as h:
        with pytest.raises(_hip.HipError) as e:
            h.projection(2)
        assert e.value.code == _hip.ERR_INVALID
        h.projection(0)
    A = operator(RAGGED)
    with openmg_amd.Solver(A, params(RAGGED, 2)) as s:
        h = s.hierarchy
        for bad in (-1, 65):
            with pytest.raises(_hip.HipError) as e:
                h.projection(bad)
            assert e.value.code == _hip.ERR_INVALID
        h.resident_load(rhs(RAGGED, 0))
        with pytest.raises(_hip.HipError) as e:
            h.resident_project()                            # (no set)
        assert e.value.code == _hip.ERR_INVALID
        h.projection(2)
        with pytest.raises(_hip.HipError) as e:
            h.resident_project_update()                     # (no projection on this right-hand side)
        assert e.value.code == _hip.ERR_INVALID
        with pytest.raises(_hip.HipError) as e:
            h.projection_fetch(0)                           # (the set is empty)
        assert e.value.code == _hip.ERR_INVALID
        assert h.resident_project() == 0
        with pytest.raises(_hip.HipError) as e:
            h.projection_time(2)                            # (nothing to time: the set is empty)
        assert e.value.code == _hip.ERR_INVALID
        h.projection(0)
        u, info = s.solve(rhs(RAGGED, 0))                   # (the hierarchy is as usable as before)
        assert np.linalg.norm(rhs(RAGGED, 0) - A @ u) <= 1.001e-8 * np.linalg.norm(rhs(RAGGED, 0))
