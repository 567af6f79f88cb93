"""openmg_amd.Solver (set up once, solve many right-hand sides), omg_resident_norms and omg_hierarchy_can_update_fine.

Yardsticks: mgSolve itself (a solve from zero must have its bits), a _hip.Hierarchy driven by hand (a warm start must
have the bits of resident_load(b, x0) plus resident_cycle calls), NumPy on the caller's operator (the two norms), and the
CPU restatement of tests/test_gpu_cycle_shapes.py with that file's gates: every cycle's norm to 1e-10 relative plus
norm_floor, the iterate to rtol 1e-9; fp32 norms to the floor of tests/test_gpu_fp32.py.  The problems are that file's,
and a pure-Neumann 16^3 Laplacian written here.  Needs an MI355X: run with -m gpu."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc
from test_gpu_cycle_shapes import (CYC, EPS32, norm_floor, norms_agree, problem, prolongations, restated_cycle,
                                   restated_norm)
from test_gpu_nullspace import mean_of, regularised_solve

pytestmark = pytest.mark.gpu

NAMES = ["poisson32", "wavefront", "var7", "stencil27", "square_jacobi", "line", "neumann"]


# ------------------------------------------------------------------------------------ problems --
def neumann_1d(n):
    """1-D Laplacian with Neumann ends: diagonal 1, 2, ..., 2, 1, off-diagonals -1 (zero row sums)"""
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    return sp.diags([-np.ones(n - 1), d, -np.ones(n - 1)], [-1, 0, 1], format="csr")


@functools.lru_cache(maxsize=None)
def get(name):
    """test_gpu_cycle_shapes.problem(name), or the Neumann problem in the same form (with 'nullspace')"""
    if name != "neumann":
        return dict(problem(name), nullspace=None)
    shape = (16, 16, 16)
    L, I = neumann_1d(16), sp.identity(16, format="csr")
    A0 = sp.csr_matrix(sp.kron(sp.kron(L, I), I) + sp.kron(sp.kron(I, L), I) + sp.kron(sp.kron(I, I), L))
    A0.sort_indices()
    R = orc.restriction_list(shape, 1, 1)
    A = orc.coefficient_list(A0, R)
    assert len(A) == 3
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    return {"name": name, "shape": shape, "A0": A0, "A": A, "R": R, "b": b, "sm": orc.make_smoother("colour", A),
            "kw": {"smoother": "colour"}, "kind": "colour", "env": {}, "flag": None, "nullspace": "constant"}


def setenv(pr, monkeypatch):
    for k, v in pr["env"].items():
        monkeypatch.setenv(k, v)


def params(pr, **kw):
    p = {"problemShape": pr["shape"], "gridLevels": len(pr["R"]), "preIterations": 1, "postIterations": 1, "cycles": 3,
         "threshold": 0.0, "smoother": pr["kind"], "minSize": 1}
    if pr["nullspace"]:
        p["nullspace"] = pr["nullspace"]
    p.update(kw)
    return p


def projected(pr, b):
    """b as the device holds it: minus its mean where the problem has the constant null space"""
    return b - mean_of(b) if pr["nullspace"] else b


def check_flag(pr, h):
    if pr["flag"]:
        assert h.level_flags(0)[pr["flag"]], pr["name"]


def open_lists(pr, **more):
    return _hip.Hierarchy(pr["A"], pr["R"], **dict(pr["kw"], nullspace=pr["nullspace"], **more))


def restated_cycles(pr, b, shape, alpha, pre, post, n, x0=None, monkeypatch=None):
    """test_gpu_cycle_shapes.restated_cycles for any b; with a null space the coarse solve is the regularised one the
    device inverts for (tests/test_gpu_nullspace.py), b is projected first and the iterate on the way out"""
    if pr["nullspace"]:
        monkeypatch.setattr(orc, "coarse_solve", regularised_solve)
    A, R = pr["A"], pr["R"]
    P = prolongations(R, alpha)
    bp = projected(pr, b)
    x, norms = x0, []
    for _ in range(n):
        x = restated_cycle(A, R, P, bp, 0, len(R), pre, post, shape, pr["sm"], x)
        norms.append(restated_norm(A, bp, x))
    x = np.asarray(x).ravel()
    return np.array(norms), (x - mean_of(x) if pr["nullspace"] else x)


def count_constructions(monkeypatch):
    """every _hip.Hierarchy made from here on, by either constructor"""
    count = {"n": 0}
    init, from_fine = _hip.Hierarchy.__init__, _hip.Hierarchy.from_fine.__func__

    def counted_init(self, *a, **k):
        count["n"] += 1
        return init(self, *a, **k)

    def counted_from_fine(cls, *a, **k):
        count["n"] += 1
        return from_fine(cls, *a, **k)

    monkeypatch.setattr(_hip.Hierarchy, "__init__", counted_init)
    monkeypatch.setattr(_hip.Hierarchy, "from_fine", classmethod(counted_from_fine))
    return count


def settings_of(pr):
    t = 1e-6 * np.linalg.norm(pr["b"])
    return [("three cycles", dict(cycles=3)),
            ("threshold only", dict(cycles=0, threshold=t)),
            ("cg", dict(cycles=0, threshold=t, accel="cg")),
            ("mixed", dict(cycles=0, threshold=t, dtype="mixed")),
            ("mixed cg", dict(cycles=0, threshold=t, dtype="mixed", accel="cg")),
            ("float32", dict(cycles=3, dtype="float32")),
            ("F 1.8", dict(cycles=3, cycle="F", overCorrection=1.8))]


# ------------------------------------------------------------------ 1. the bits of mgSolve --
@pytest.mark.parametrize("name", NAMES)
def test_a_solve_from_zero_has_the_bits_of_mgsolve(monkeypatch, name):
    pr = get(name)
    setenv(pr, monkeypatch)
    A0, b = pr["A0"], pr["b"]
    nb = np.linalg.norm(projected(pr, b))
    for label, kw in settings_of(pr):
        p = params(pr, **kw)
        given = dict(p)
        with openmg_amd.Solver(A0, p) as s:
            assert p == given and "rtol" not in openmg_amd.defaults            # the caller's dict and the defaults stay
            check_flag(pr, s.hierarchy)
            u, info = s.solve(b)
        want, winfo = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=True))
        print("%s %s: %d cycles, norm %.6e (mgSolve %d, %.6e), rhs_norm rel diff %.2e"
              % (name, label, info["cycle"], info["norm"], winfo["cycle"], winfo["norm"], abs(info["rhs_norm"] - nb) / nb))
        assert np.array_equal(u, want), (name, label, int(np.sum(u != want)))
        assert info["cycle"] == winfo["cycle"] and info["norm"] == winfo["norm"], (name, label, info, winfo["norm"])
        assert len(info["norms"]) == info["cycle"]
        # (rhs_norm is that of b AS IT IS HELD: an fp32 hierarchy holds fl32(b), each entry within eps32 / 2 of b's, the
        # projection one more rounding — the norm within eps32 relative; measured 3e-10 to 6e-10)
        assert abs(info["rhs_norm"] - nb) <= (EPS32 if kw.get("dtype") == "float32" else 1e-12) * nb
        assert info["initial_norm"] == info["rhs_norm"]
        if "accel" not in kw:
            assert info["norms"][-1] == info["norm"]


# ------------------------------------------------------------------------------- 2. reuse --
@pytest.mark.parametrize("name", ["poisson32", "stencil27", "line", "neumann"])
def test_one_solver_many_right_hand_sides(monkeypatch, name):
    pr = get(name)
    setenv(pr, monkeypatch)
    A0, b1 = pr["A0"], pr["b"]
    b2 = A0 @ np.random.default_rng(99).random(b1.size)
    p = params(pr)
    other = dict(accel="cg", cycle="F", overCorrection=1.8)
    want1, i1 = openmg_amd.mgSolve(A0, b1, dict(p, giveInfo=True))
    want2, i2 = openmg_amd.mgSolve(A0, b2, dict(p, giveInfo=True))
    want3, i3 = openmg_amd.mgSolve(A0, b2, dict(p, giveInfo=True, **other))
    count = count_constructions(monkeypatch)
    with openmg_amd.Solver(A0, p) as s:
        u1, j1 = s.solve(b1)
        u2, j2 = s.solve(b2)
        u1b, j1b = s.solve(b1)
        assert np.array_equal(u1b, u1) and j1b == j1
        assert np.array_equal(u1, want1) and np.array_equal(u2, want2)
        assert (j1["cycle"], j1["norm"], j2["cycle"], j2["norm"]) == (i1["cycle"], i1["norm"], i2["cycle"], i2["norm"])
        u3, j3 = s.solve(b2, **other)                      # other settings through overrides ...
        assert np.array_equal(u3, want3) and (j3["cycle"], j3["norm"]) == (i3["cycle"], i3["norm"])
        assert not np.array_equal(u3, u2)
        u2b, j2b = s.solve(b2)                             # ... and back: nothing of them is left behind
        assert np.array_equal(u2b, u2) and j2b == j2
        if pr["nullspace"]:
            for u in (u1, u2, u3):
                assert abs(mean_of(u)) <= 1e-12 * np.abs(u).max()
    assert count["n"] == 1, count


# -------------------------------------------------------------------------- 3. warm start --
@pytest.mark.parametrize("name", NAMES)
def test_a_warm_start_has_the_bits_of_the_resident_entries_and_follows_the_restatement(monkeypatch, name):
    pr = get(name)
    setenv(pr, monkeypatch)
    A0, b = pr["A0"], pr["b"]
    x0 = np.random.default_rng(5).standard_normal(b.size)
    with openmg_amd.Solver(A0, params(pr, giveInfo=True)) as s:
        check_flag(pr, s.hierarchy)
        u, info = s.solve(b, initial=x0, cycles=3)
        with _hip.Hierarchy(s.A, s.R, **dict(pr["kw"], nullspace=pr["nullspace"])) as h:
            h.resident_load(b, x0)
            norms = [h.resident_cycle(1, 1) for _ in range(3)]
            want = h.resident_fetch()
        assert np.array_equal(u, want) and info["norms"] == norms and info["cycle"] == 3 and info["norm"] == norms[-1]
        bp = projected(pr, b)
        r0 = np.linalg.norm(bp - A0 @ x0)
        assert abs(info["initial_norm"] - r0) <= 1e-10 * r0 + norm_floor(A0, bp, x0)
        cpu_norms, cpu_x = restated_cycles(pr, b, "V", 1.0, 1, 1, 3, x0, monkeypatch)
        print("%s: norms rel diff %.2e, iterate max diff %.2e"
              % (name, max(abs(a - c) / c for a, c in zip(norms, cpu_norms)), np.abs(u - cpu_x).max()))
        assert norms_agree(info["norms"], cpu_norms, norm_floor(A0, bp, cpu_x))
        assert np.allclose(u, cpu_x, **CYC)
        # a start that is already good enough: no cycle, the iterate handed back
        fine, _ = s.solve(b, cycles=200, threshold=0.0, rtol=1e-10, accel="cg")
        assert np.linalg.norm(bp - A0 @ fine) <= 2e-10 * np.linalg.norm(bp)
        again, info2 = s.solve(b, initial=fine, cycles=0, threshold=0.0, rtol=1e-8)
        assert info2["cycle"] == 0 and info2["norms"] == [] and info2["norm"] == info2["initial_norm"]
        assert info2["initial_norm"] < 1e-8 * info2["rhs_norm"]
        if pr["nullspace"]:
            assert np.abs(again - fine).max() <= 1e-14 * np.abs(fine).max()      # (the second projection may move an ulp)
        else:
            assert np.array_equal(again, fine)


# -------------------------------------------------------------------------- 4. stop rules --
@pytest.mark.parametrize("name", ["poisson32", "wavefront", "neumann"])
def test_the_relative_stop_rule_counts_what_the_norms_say(monkeypatch, name):
    pr = get(name)
    A0, b = pr["A0"], pr["b"]
    bp = projected(pr, b)
    target = 1e-6 * np.linalg.norm(bp)
    # on the restatement no norm lies within 1e-9 relative of the target, ten times the parity gate: rounding cannot move
    # the count (the condition of test_cycles_to_1e8_equal_the_restatement_and_f_needs_a_quarter_of_v)
    cpu_norms, _ = restated_cycles(pr, b, "F", 1.8, 1, 1, 40, None, monkeypatch)
    assert cpu_norms[-1] < target and min(abs(nk - target) for nk in cpu_norms) > 1e-9 * target
    with openmg_amd.Solver(A0, params(pr, cycle="F", overCorrection=1.8)) as s:
        _, long = s.solve(b, cycles=40)
        assert len(long["norms"]) == long["cycle"] == 40
        first = 1 + next(k for k, nk in enumerate(long["norms"]) if nk < 1e-6 * long["rhs_norm"])
        u, info = s.solve(b, cycles=0, rtol=1e-6)
        print("%s: %d cycles to 1e-6 (restatement %d)" % (name, info["cycle"], 1 + int(np.argmax(cpu_norms < target))))
        assert info["cycle"] == first == 1 + int(np.argmax(cpu_norms < target))
        assert len(info["norms"]) == info["cycle"] and info["norms"] == long["norms"][:first]
        assert abs(info["rhs_norm"] - np.linalg.norm(bp)) <= 1e-12 * np.linalg.norm(bp)
        # 'threshold' and 'rtol' together: the larger target rules
        _, both = s.solve(b, cycles=0, rtol=1e-6, threshold=1e-3 * long["rhs_norm"])
        assert both["cycle"] == 1 + next(k for k, nk in enumerate(long["norms"]) if nk < 1e-3 * long["rhs_norm"])
        _, capped = s.solve(b, cycles=2, rtol=1e-6)
        assert capped["cycle"] == 2
        with pytest.raises(ValueError):
            s.solve(b, cycles=0, threshold=0.0, rtol=0.0)
        with pytest.raises(ValueError):
            s.solve(b, smoother="gs")
        with pytest.raises(ValueError):
            s.solve(b, dtype="float32")
        again, info3 = s.solve(b, cycles=0, rtol=1e-6)                  # (the refused calls left nothing behind)
        assert np.array_equal(again, u) and info3 == info


# -------------------------------------------------------------------- 5. omg_resident_norms --
@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("name", NAMES)
def test_resident_norms_on_every_kind_of_level_zero(monkeypatch, name, dtype):
    pr = get(name)
    setenv(pr, monkeypatch)
    A0, b = pr["A0"], pr["b"]
    bp = projected(pr, b)
    x0 = np.random.default_rng(5).standard_normal(b.size)
    xmax = max(np.abs(x0).max(), 1.0)                                    # (b = A0 @ x with max |x| < 1)
    floor32 = 64 * EPS32 * float(abs(A0).sum(axis=1).max()) * xmax * np.sqrt(b.size)       # tests/test_gpu_fp32.py

    def gate(want, x):
        return floor32 if dtype == "float32" else 1e-10 * want + norm_floor(A0, bp, x)

    with open_lists(pr, dtype=dtype) as h:
        check_flag(pr, h)
        assert not h.can_update_fine()                                   # (made from lists)
        # the plain sequence, nothing in between
        h.resident_load(b, x0)
        plain_norms, plain_x = [], []
        for _ in range(2):
            plain_norms.append(h.resident_cycle(1, 1))
            plain_x.append(h.resident_fetch())
        # the same with the norms read before, between and after the cycles
        h.resident_load(b, x0)
        nb, n0 = h.resident_norms()
        want_b, want_0 = np.linalg.norm(bp), np.linalg.norm(bp - A0 @ x0)
        print("%s %s: ||b|| rel diff %.2e, ||b - A x0|| rel diff %.2e" % (name, dtype, abs(nb - want_b) / want_b, abs(n0 - want_0) / want_0))
        assert abs(nb - want_b) <= gate(want_b, 0 * x0), (nb, want_b)
        assert abs(n0 - want_0) <= gate(want_0, x0), (n0, want_0)
        assert h.resident_norms(rhs=True, residual=False) == (nb, None)
        assert h.resident_norms(rhs=False, residual=True) == (None, n0)                  # the same bits from run to run
        for k in range(2):
            norm = h.resident_cycle(1, 1)
            after = h.resident_norms()[1]
            x = h.resident_fetch()
            print("  cycle %d: norm %.6e, omg_resident_norms %.6e" % (k + 1, norm, after))
            assert norm == plain_norms[k] and np.array_equal(x, plain_x[k]), (name, dtype, k)
            assert abs(after - norm) <= gate(norm, x), (k, after, norm)
        # ... and when the cycles are replayed from a graph
        h.use_graph(True)
        h.resident_load(b, x0)
        h.resident_norms()
        norms = []
        for _ in range(2):
            norms.append(h.resident_cycle(1, 1))
            h.resident_norms()
            norms.append(h.resident_fetch())
        assert norms[0::2] == plain_norms and np.array_equal(norms[1], plain_x[0]) and np.array_equal(norms[3], plain_x[1]), (name, dtype, "graph")
        h.use_graph(False)
        # ... and FCG after the call
        h.resident_load(b, x0)
        want = h.resident_pcg(1, 1, 3)
        want_x = h.resident_fetch()
        h.resident_load(b, x0)
        h.resident_norms()
        got = h.resident_pcg(1, 1, 3)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2] and np.array_equal(h.resident_fetch(), want_x)


def test_resident_norms_needs_a_resident_state():
    pr = get("wavefront")
    with open_lists(pr) as h:
        nb, nr = ctypes.c_double(0), ctypes.c_double(0)
        assert _hip.lib().omg_resident_norms(h._h, ctypes.byref(nb), ctypes.byref(nr)) == _hip.ERR_INVALID
        h.resident_load(pr["b"])
        assert _hip.lib().omg_resident_norms(h._h, None, None) == _hip.OMG_OK


# ------------------------------------------------------------------------------ 6. update --
@pytest.mark.parametrize("name", ["var7", "stencil27"])
def test_update_in_place_where_the_hierarchy_takes_new_coefficients(monkeypatch, name):
    pr = get(name)
    setenv(pr, monkeypatch)
    make = operators.stencil7_variable if name == "var7" else operators.stencil27_variable
    A0, b = pr["A0"], pr["b"]
    A_new = make(pr["shape"], 7)
    assert np.array_equal(A_new.indices, A0.indices) and not np.array_equal(A_new.data, A0.data)
    p = params(pr)
    with openmg_amd.Solver(A_new, p) as fresh:
        want, winfo = fresh.solve(b)
        want_cg, wcg = fresh.solve(b, accel="cg")
    count = count_constructions(monkeypatch)
    with openmg_amd.Solver(A0, p) as s:
        check_flag(pr, s.hierarchy)
        assert s.hierarchy.can_update_fine()
        old, _ = s.solve(b)
        s.update(A_new)
        u, info = s.solve(b)
        assert np.array_equal(u, want) and info == winfo and not np.array_equal(u, old)
        u, info = s.solve(b, accel="cg")
        assert np.array_equal(u, want_cg) and info == wcg
        s.update(A0)                                                       # ... and back
        assert np.array_equal(s.solve(b)[0], old)
    assert count["n"] == 1, count


def test_update_by_a_new_setup_where_it_does_not_and_a_refused_pattern(monkeypatch):
    pr = get("poisson32")
    A0, b = pr["A0"], pr["b"]
    A_new = sp.csr_matrix((2.0 * A0.data, A0.indices, A0.indptr), shape=A0.shape)
    p = params(pr)
    with openmg_amd.Solver(A_new, p) as fresh:
        want, winfo = fresh.solve(b)
    count = count_constructions(monkeypatch)
    with openmg_amd.Solver(A0, p) as s:
        assert not s.hierarchy.can_update_fine()
        old, oinfo = s.solve(b)
        with pytest.raises(ValueError):
            s.update(operators.stencil27_variable(pr["shape"]))           # another pattern
        with pytest.raises(ValueError):
            s.update(operators.stencil_poisson((16, 16, 16)))             # another size
        u, info = s.solve(b)
        assert np.array_equal(u, old) and info == oinfo and count["n"] == 1
        s.update(A_new)
        assert count["n"] == 2
        check_flag(pr, s.hierarchy)
        u, info = s.solve(b)
        assert np.array_equal(u, want) and info == winfo and not np.array_equal(u, old)
    assert count["n"] == 2


# -------------------------------------------------------------------------- 7. null space --
def test_an_operator_without_the_null_space_is_refused_at_construction():
    pr = get("wavefront")
    with pytest.raises(_hip.HipError):
        openmg_amd.Solver(pr["A0"], params(pr, nullspace="constant"))


# ------------------------------------------------------------------------------- 8. apply --
@pytest.mark.parametrize("shape,alpha", [("V", 1.0), ("F", 1.8)])
def test_apply_is_mgcycle_from_zero(shape, alpha):
    pr = get("poisson32")
    r = np.random.default_rng(8).standard_normal(pr["b"].size)
    try:
        with openmg_amd.Solver(pr["A0"], params(pr, giveInfo=True, cycle=shape, overCorrection=alpha)) as s:
            z = s.apply(r)
            cp = {"coarsestLevel": len(s.R), "preIterations": 1, "postIterations": 1, "smoother": "colour", "cycle": shape,
                  "overCorrection": alpha}
            want = openmg_amd.mgCycle(s.A, r, 0, s.R, cp)[0]
            assert np.array_equal(z, want)
            out = np.empty_like(r)
            s.solve(pr["b"])                                               # (a solve in between leaves nothing an apply sees)
            assert s.apply(r, out=out) is out and np.array_equal(out, want)
        with openmg_amd.Solver(pr["A0"], params(pr, dtype="mixed")) as s:
            with pytest.raises(ValueError):
                s.apply(r)
    finally:
        openmg_amd.clear_cache()


# ----------------------------------------------------------------------- 9. device arrays --
# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as in tests/test_gpu_cycle_shapes.py)
DEVICE_ARRAYS = """
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import openmg_amd
from openmg_amd import operators
shape = (32, 32, 32)
A0 = operators.stencil_poisson(shape)
b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
x0 = np.random.default_rng(3).random(b.size)
p = {"problemShape": shape, "gridLevels": 3, "preIterations": 1, "postIterations": 1, "cycles": 3, "threshold": 0.0,
     "smoother": "colour", "minSize": 1}
with openmg_amd.Solver(A0, p) as s:
    for kw in ({}, {"accel": "cg"}, {"cycles": 0, "rtol": 1e-6, "cycle": "F", "overCorrection": 1.8}):
        uh, ih = s.solve(b, initial=x0, **kw)
        bd, xd = torch.tensor(b, device="cuda"), torch.tensor(x0, device="cuda")
        ud, idv = s.solve(bd, initial=xd, **kw)
        assert isinstance(ud, torch.Tensor) and ud.is_cuda
        assert np.array_equal(ud.cpu().numpy(), uh) and idv == ih, kw
        assert np.array_equal(xd.cpu().numpy(), x0) and np.array_equal(bd.cpu().numpy(), b)
        out = torch.empty_like(bd)
        assert s.solve(bd, initial=xd, out=out, **kw)[0] is out and np.array_equal(out.cpu().numpy(), uh)
    u0, _ = s.solve(torch.tensor(b, device="cuda"))
    assert np.array_equal(u0.cpu().numpy(), s.solve(b)[0])
    try:
        s.solve(b, initial=torch.tensor(x0, device="cuda"))
    except TypeError:
        pass
    else:
        raise AssertionError("a device `initial` with a host `b` was accepted")
    zh = s.apply(b)
    zd = s.apply(torch.tensor(b, device="cuda"))
    assert isinstance(zd, torch.Tensor) and np.array_equal(zd.cpu().numpy(), zh)
    out = torch.empty(b.size, dtype=torch.float64, device="cuda")
    assert s.apply(torch.tensor(b, device="cuda"), out=out) is out and np.array_equal(out.cpu().numpy(), zh)
print("device arrays ok")
"""


def test_device_arrays_have_the_bits_of_the_host_calls():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "device arrays ok" in p.stdout, p.stderr[-3000:]


# ------------------------------------------------------------------------------ 10. guards --
def test_a_norm_that_is_not_finite_raises_and_the_solver_stays_usable():
    pr = get("poisson32")
    A0, b = pr["A0"], pr["b"]
    p = params(pr, cycles=0, threshold=1e-6 * np.linalg.norm(b))
    want, winfo = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=True))
    bad = b.copy()
    bad[0] = np.nan
    with openmg_amd.Solver(A0, p) as s:
        with pytest.raises(RuntimeError, match="cycle 1 "):
            s.solve(bad)                                    # (mgSolve would cycle for ever: nan < threshold is never true)
        with pytest.raises(RuntimeError, match="1"):
            s.solve(bad, accel="cg")
        u, info = s.solve(b)
        assert np.array_equal(u, want) and (info["cycle"], info["norm"]) == (winfo["cycle"], winfo["norm"])


def test_a_closed_solver_refuses_every_call():
    pr = get("wavefront")
    s = openmg_amd.Solver(pr["A0"], params(pr))
    s.solve(pr["b"])
    s.close()
    s.close()
    for call in (lambda: s.solve(pr["b"]), lambda: s.apply(pr["b"]), lambda: s.update(pr["A0"]), lambda: s.hierarchy):
        with pytest.raises(RuntimeError):
            call()
