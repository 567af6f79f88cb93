"""F- and W-cycles and the over-correction factor (parameters['cycle'], parameters['overCorrection'];
omg_hierarchy_set_cycle) against a restatement of the recursion written here from the oracle's own pieces — smoother,
residual, products, direct solve — which never touches the code under test:

    cycle(l, b, x, k):   coarsest level: direct solve.  Otherwise smooth (pre), b_c = R[l] (b - A[l] x), e = 0,
                         visit level l + 1 once (k = 'V', or l + 1 is the coarsest level) or twice ('F': an F- then a
                         V-cycle; 'W': two W-cycles; the second visit starts from the first one's e with the same b_c),
                         x += P'[l] e, smooth (post) — P'[l] = R[l]^T with every stored entry a replaced by fl(alpha a),
                         rounded once to the level's precision.

Gates: the project's own — tests/test_gpu_parity.py (every cycle's norm to 1e-10 relative — plus what fp64 cannot resolve
in a residual norm, norm_floor below —, the iterate to rtol 1e-9),
tests/test_gpu_fp32.py for fp32 levels, tests/test_gpu_pcg.py and tests/test_gpu_mixed.py for the accelerated and the
mixed-precision solves.  Needs an MI355X: run with -m gpu."""
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

pytestmark = pytest.mark.gpu

CYC = dict(rtol=1e-9, atol=1e-11)      # iterate after several cycles (tests/test_gpu_parity.py)
NORM_RTOL = 1e-10                      # BASELINE.json parity gate
EPS32 = float(np.finfo(np.float32).eps)

SETTINGS = [("F", 1.0), ("F", 1.5), ("F", 1.8), ("W", 1.0), ("W", 1.5), ("W", 1.8), ("V", 1.5)]
SWEEPS = [(1, 1), (2, 1), (1, 0), (0, 1)]


# ------------------------------------------------------------------------------ the restatement --
def visits_of(shape, level, coarsest):
    if shape == "V" or level + 1 == coarsest:
        return [shape]
    return ["F", "V"] if shape == "F" else ["W", "W"]


def prolongations(R, alpha, dtype=np.float64):
    """R[l]^T with every stored entry a replaced by fl(alpha * a) in the levels' precision."""
    out = []
    for Rl in R:
        P = sp.csr_matrix(sp.csr_matrix(Rl).T)
        a = P.data.astype(dtype).astype(np.float64)
        P.data = (np.float64(alpha) * a).astype(dtype).astype(np.float64)
        out.append(P)
    return out


def relax(sm, A, b, x, its, level):
    if its <= 0:
        return x
    return orc.smooth(A, b, x, its) if sm is None else sm(A, b, x, its, level)


def restated_cycle(A, R, P, b, level, coarsest, pre, post, shape, sm, x=None, count=None):
    b = np.asarray(b, dtype=np.float64).ravel()
    N = b.size
    if count is not None:
        count[level] = count.get(level, 0) + 1
    if level == coarsest:
        return orc.coarse_solve(A[level], b.reshape((N, 1)))
    u = np.zeros(N) if x is None else np.array(x, dtype=np.float64).ravel()
    u = relax(sm, A[level], b, u, pre, level)
    NH = R[level].shape[0]
    r = orc.get_residual(b, A[level], u, N)
    bc = np.asarray(orc.flexible_mmult(R[level], r.reshape((N, 1)))).reshape((NH,))
    e = None
    for s in visits_of(shape, level, coarsest):
        e = restated_cycle(A, R, P, bc, level + 1, coarsest, pre, post, s, sm, e, count)
    u = np.asarray(u).reshape((N,)) + np.asarray(orc.flexible_mmult(P[level], e.reshape((NH, 1)))).reshape((N,))
    u = relax(sm, A[level], b, u, post, level)
    return u


def restated_norm(A, b, u, level=0):
    return float(np.linalg.norm(orc.get_residual(b, A[level], u, b.size)))


def restated_cycles(pr, shape, alpha, pre, post, n, x0=None, dtype=np.float64):
    A, R = pr["A"], pr["R"]
    P = prolongations(R, alpha, dtype)
    x, norms = x0, []
    for _ in range(n):
        x = restated_cycle(A, R, P, pr["b"], 0, len(R), pre, post, shape, pr["sm"], x)
        norms.append(restated_norm(A, pr["b"], x))
    return np.array(norms), x


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


U64 = 2.0 ** -53


def norm_floor(A0, b, x):
    """What fp64 itself leaves open in ||b - A0 x||: a row of k stored entries is evaluated with a componentwise error of
    at most (k + 2) u (|b| + |A0| |x|) (u = 2^-53), whatever the order of its sum, so two correct evaluations of the norm
    may differ by twice the 2-norm of that.  It matters where a few cycles have taken the residual down to 1e-10 ||b|| and
    below (the 1-D problem with V(2,1): 3.5e-11 ||b|| after five cycles, the iterates equal to 2 ulp, the norms to 4e-9)."""
    k = int(np.diff(sp.csr_matrix(A0).indptr).max())
    return 2.0 * (k + 2) * U64 * float(np.linalg.norm(np.abs(b) + abs(A0) @ np.abs(x)))


def norms_agree(got, want, floor):
    """BASELINE.json's parity gate, 1e-10 relative, on every cycle's norm — beyond what norm_floor says fp64 cannot resolve"""
    return all(abs(a - c) <= NORM_RTOL * c + floor for a, c in zip(got, want))


# ------------------------------------------------------------------------------------ problems --
@functools.lru_cache(maxsize=None)
def problem(name):
    """A, R (the oracle's lists), b, the oracle's smoother, the Hierarchy's keyword arguments, the level-0 flag that must hold"""
    env, flag, omega = {}, None, 2.0 / 3.0
    if name == "poisson32":
        shape, grids, kind, flag = (32, 32, 32), 4, "colour", "plane"
        A0 = operators.stencil_poisson(shape)
    elif name == "box":
        shape, grids, kind, flag = (16, 32, 16), 3, "colour", "plane"
        A0 = operators.stencil_poisson(shape)
    elif name in ("square_colour", "square_jacobi"):
        shape, grids, kind, flag = (64, 64), 4, name.split("_")[1], "plane"
        A0 = operators.stencil_poisson(shape)
    elif name == "line":
        shape, grids, kind = (4096,), 4, "gs"
        A0 = sp.csr_matrix(orc.poisson(shape, sparse=True))
    elif name == "wavefront":
        shape, grids, kind, flag = (16, 16, 16), 3, "gs", "march"
        A0 = operators.stencil_poisson(shape)
    elif name == "var7":
        shape, grids, kind, flag = (16, 16, 16), 3, "colour", "var7"
        A0 = operators.stencil7_variable(shape)
        env = {"OMG_VAR7_MIN": "4096"}                      # (by default only levels of 128^3 and more take the passes)
    elif name == "stencil27":
        shape, grids, kind, flag = (16, 16, 16), 3, "colour", "stencil27"
        A0 = operators.stencil27_variable(shape)
    elif name == "poisson64":
        shape, grids, kind, flag = (64, 64, 64), 5, "colour", "plane"
        A0 = operators.stencil_poisson(shape)
    else:
        raise KeyError(name)
    R = orc.restriction_list(shape, grids - 2, 1)
    A = orc.coefficient_list(A0, R)
    assert len(A) == grids
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    kw = {"smoother": kind}
    if kind == "jacobi":
        kw["omega"] = omega
    return {"name": name, "shape": shape, "A0": A0, "A": A, "R": R, "b": b, "sm": orc.make_smoother(kind, A, omega=omega),
            "kw": kw, "kind": kind, "env": env, "flag": flag}


def open_hierarchy(pr, monkeypatch, **more):
    for k, v in pr["env"].items():
        monkeypatch.setenv(k, v)
    h = _hip.Hierarchy(pr["A"], pr["R"], **dict(pr["kw"], **more))
    if pr["flag"]:
        assert h.level_flags(0)[pr["flag"]], pr["name"]
    return h


def device_cycles(h, b, pre, post, n, x0=None):
    h.resident_load(b, x0)
    norms = [h.resident_cycle(pre, post) for _ in range(n)]
    return np.array(norms), h.resident_fetch()


def solve_params(pr, **kw):
    p = {"problemShape": pr["shape"], "gridLevels": len(pr["R"]), "preIterations": 1, "postIterations": 1, "cycles": 3,
         "threshold": 0.0, "giveInfo": True, "smoother": pr["kind"], "minSize": 1}
    p.update(kw)
    return p


# ------------------------------------------------------------------------- 1. the default stays --
@pytest.mark.parametrize("name", ["poisson32", "var7", "stencil27", "line"])
def test_v_with_factor_one_is_the_call_without_the_keys(monkeypatch, name):
    pr = problem(name)
    for k, v in pr["env"].items():
        monkeypatch.setenv(k, v)
    x0, i0 = openmg_amd.mgSolve(pr["A0"], pr["b"], solve_params(pr))
    x1, i1 = openmg_amd.mgSolve(pr["A0"], pr["b"], solve_params(pr, cycle="V", overCorrection=1.0))
    assert np.array_equal(x0, x1) and i0["norm"] == i1["norm"] and i0["cycle"] == i1["cycle"] == 3
    with open_hierarchy(pr, monkeypatch) as h:
        assert h.get_cycle() == ("V", 1.0)
        want = device_cycles(h, pr["b"], 1, 1, 3)
        h.set_cycle("V", 1.0)
        got = device_cycles(h, pr["b"], 1, 1, 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        h.set_cycle("F", 1.8)
        device_cycles(h, pr["b"], 1, 1, 1)
        h.set_cycle("V", 1.0)                      # ... and back: nothing of the other setting is left behind
        got = device_cycles(h, pr["b"], 1, 1, 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_bad_settings_are_refused_by_the_library():
    pr = problem("wavefront")
    with _hip.Hierarchy(pr["A"], pr["R"], smoother="gs") as h:
        for shape, alpha in ((3, 1.0), (-1, 1.0), (0, 0.0), (1, -1.5), (2, float("nan")), (0, float("inf"))):
            rc = _hip.lib().omg_hierarchy_set_cycle(h._h, shape, alpha)
            assert rc == _hip.ERR_INVALID, (shape, alpha, rc)
        assert h.get_cycle() == ("V", 1.0)
        h.set_cycle("W", 1.8)
        assert h.get_cycle() == ("W", 1.8)


# ------------------------------------------------------------- 2. parity with the restatement --
@pytest.mark.parametrize("name", ["poisson32", "box", "square_colour", "square_jacobi", "line", "wavefront", "var7", "stencil27"])
def test_every_shape_and_factor_against_the_restatement(monkeypatch, name):
    pr = problem(name)
    worst = (0.0, None)
    failures = []
    with open_hierarchy(pr, monkeypatch) as h:
        for pre, post in SWEEPS:
            for shape, alpha in SETTINGS:
                want_norms, want_x = restated_cycles(pr, shape, alpha, pre, post, 5)
                h.set_cycle(shape, alpha)
                norms, x = device_cycles(h, pr["b"], pre, post, 5)
                d = max(rel(a, c) for a, c in zip(norms, want_norms))
                if d > worst[0]:
                    worst = (d, (shape, alpha, pre, post))
                print("%s %s alpha %.1f V(%d,%d): norms rel diff %.2e, iterate max diff %.2e"
                      % (name, shape, alpha, pre, post, d, np.abs(x - want_x).max()))
                if not (norms_agree(norms, want_norms, norm_floor(pr["A0"], pr["b"], want_x)) and np.allclose(x, want_x, **CYC)):
                    failures.append((shape, alpha, pre, post, d, float(np.abs(x - want_x).max())))
    print("worst norm difference:", worst)
    assert not failures, failures


def test_fp32_levels_track_the_restatement(monkeypatch):
    """tests/test_gpu_fp32.py's gates for whole cycles, F-cycles with a factor float cannot represent: the restatement
    (fp64 arithmetic, the weight rounded to fp32 as the levels hold it) is followed to 1e-3 while the residual is above the
    fp32 floor, and the fp32 iterate ends with a true residual no worse than the restatement's plus that floor."""
    pr = problem("poisson32")
    n64, x64 = restated_cycles(pr, "F", 1.8, 1, 1, 12, dtype=np.float32)
    with open_hierarchy(pr, monkeypatch, dtype="float32") as h:
        h.set_cycle("F", 1.8)
        n32, x32 = device_cycles(h, pr["b"], 1, 1, 12)
    A0, b = pr["A0"], pr["b"]
    floor = 64 * EPS32 * float(abs(A0).sum(axis=1).max()) * 1.0 * np.sqrt(b.size)      # (b = A0 @ x, max |x| < 1)
    above = n64 > 50 * floor
    assert above.sum() >= 2
    np.testing.assert_allclose(n32[above], n64[above], rtol=1e-3)
    true_r = np.linalg.norm(b - A0 @ x32)
    assert true_r <= 1.001 * n64[-1] + floor, (true_r, n64[-1], floor)
    assert abs(n32[-1] - true_r) <= floor, (n32[-1], true_r, floor)
    assert np.abs(x32 - x64).max() <= 1e-3 * np.abs(x64).max()


# --------------------------------------------- 3. fused passes == the set schedule, bit for bit --
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["poisson32", "box", "square_colour", "square_jacobi", "var7", "stencil27"])
def test_fused_passes_have_the_bits_of_the_set_schedule(monkeypatch, name, dtype):
    pr = problem(name)
    rng = np.random.default_rng(5)
    b, x0 = pr["b"], rng.standard_normal(pr["b"].size)
    if dtype == "float32":
        b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
    with open_hierarchy(pr, monkeypatch, dtype=dtype) as h:
        for shape in ("F", "W"):
            h.set_cycle(shape, 1.8)
            for pre, post in SWEEPS + [(2, 2)]:
                for start in (x0, None):
                    h.use_plane(True)
                    got = device_cycles(h, b, pre, post, 3, start)
                    h.use_plane(False)
                    want = device_cycles(h, b, pre, post, 3, start)
                    assert np.array_equal(got[1], want[1]), (name, dtype, shape, pre, post, start is None, int(np.sum(got[1] != want[1])))
                    np.testing.assert_allclose(got[0], want[0], rtol=1e-12 if dtype == "float64" else 1e-6)


# --------------------------------------------------------------------------- 4. exact linearity --
@pytest.mark.parametrize("name", ["poisson32", "square_colour", "var7", "stencil27", "line"])
def test_the_cycle_is_exactly_linear(monkeypatch, name):
    pr = problem(name)
    with open_hierarchy(pr, monkeypatch) as h:
        for shape in ("F", "W"):
            h.set_cycle(shape, 1.8)
            n1, x1 = device_cycles(h, pr["b"], 1, 1, 2)
            n2, x2 = device_cycles(h, 2.0 * pr["b"], 1, 1, 2)
            assert np.array_equal(x2, 2.0 * x1), (name, shape)
            np.testing.assert_allclose(n2, 2.0 * n1, rtol=1e-14)


# ------------------------------------------- 5. single, batched and graph-replayed cycles agree --
@pytest.mark.parametrize("name", ["poisson32", "square_jacobi", "var7", "line"])
def test_single_batched_and_replayed_cycles_and_a_change_of_shape(monkeypatch, name):
    pr = problem(name)
    b = pr["b"]
    fresh = {}
    for setting in (("V", 1.0), ("F", 1.8)):
        with open_hierarchy(pr, monkeypatch) as h:
            h.set_cycle(*setting)
            fresh[setting] = device_cycles(h, b, 1, 1, 4)
    with open_hierarchy(pr, monkeypatch) as h:
        h.set_cycle("F", 1.8)
        h.resident_load(b)
        batch = h.resident_cycles(1, 1, 4)
        assert np.array_equal(batch, fresh[("F", 1.8)][0]) and np.array_equal(h.resident_fetch(), fresh[("F", 1.8)][1])
        h.use_graph(True)
        for setting in (("V", 1.0), ("F", 1.8), ("V", 1.0), ("F", 1.8)):      # (a graph captured under one setting must not serve the other)
            h.set_cycle(*setting)
            got = device_cycles(h, b, 1, 1, 4)
            assert np.array_equal(got[0], fresh[setting][0]), (name, setting)
            assert np.array_equal(got[1], fresh[setting][1]), (name, setting)
        h.use_graph(False)


# ------------------------------------------------------------------------------------ 6. mgCycle --
def cycle_params(pr, **kw):
    p = {"coarsestLevel": len(pr["R"]), "preIterations": 1, "postIterations": 1, "smoother": pr["kind"]}
    p.update(kw)
    return p


def test_mgcycle_obeys_both_keys_at_level_zero_and_one():
    pr = problem("poisson32")
    A, R, b = pr["A"], pr["R"], pr["b"]
    x0 = np.random.default_rng(3).random(b.size)
    b1 = np.asarray(R[0] @ b).ravel()
    try:
        first = {}
        for rounds in range(2):             # (the second round finds the hierarchy cached with the OTHER setting)
            for shape, alpha in (("V", 1.0), ("F", 1.8), ("W", 1.5)):
                P = prolongations(R, alpha)
                for level, rhs, start in ((0, b, x0), (0, b, None), (1, b1, None)):
                    u, info = openmg_amd.mgCycle(A, rhs, level, R, cycle_params(pr, cycle=shape, overCorrection=alpha),
                                                 initial=None if start is None else start.copy())
                    want = restated_cycle(A, R, P, rhs, level, len(R), 1, 1, shape, pr["sm"], start)
                    np.testing.assert_allclose(u, want, **CYC)
                    assert rel(info["norm"], restated_norm(A, rhs, want, level)) < NORM_RTOL, (shape, alpha, level)
                    key = (shape, alpha, level, start is None)
                    if rounds == 0:
                        first[key] = u
                    else:
                        assert np.array_equal(u, first[key]), key
        assert not np.array_equal(first[("V", 1.0, 0, True)], first[("F", 1.8, 0, True)])
    finally:
        openmg_amd.clear_cache()


def test_mgcycle_announces_the_recursion(capsys):
    pr = problem("wavefront")                   # three grids: levels 0, 1 and the direct solve at 2
    try:
        openmg_amd.mgCycle(pr["A"], pr["b"], 0, pr["R"], cycle_params(pr, cycle="W", verbose=True))
    finally:
        openmg_amd.clear_cache()
    lines = [l for l in capsys.readouterr().out.splitlines() if "level" in l]
    assert lines == ["calling mgCycle at level 0", " calling mgCycle at level 1", "  direct solving at level 2",
                     " calling mgCycle at level 1", "  direct solving at level 2"]


# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as tests/devarray_worker.py does)
DEVICE_ARRAYS = """
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import openmg_amd
from openmg_amd import operators
from oracle import mg_oracle as orc
shape = (32, 32, 32)
A0 = operators.stencil_poisson(shape)
R = orc.restriction_list(shape, 2, 1)
A = orc.coefficient_list(A0, R)
b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
b1 = np.asarray(R[0] @ b).ravel()
x0 = np.random.default_rng(3).random(b.size)
seen = []
for shape_key, alpha in (("V", 1.0), ("F", 1.8), ("W", 1.5), ("V", 1.0)):
    p = {"coarsestLevel": 3, "preIterations": 1, "postIterations": 1, "smoother": "colour", "cycle": shape_key, "overCorrection": alpha}
    for level, rhs, start in ((0, b, x0), (1, b1, None)):
        uh, ih = openmg_amd.mgCycle(A, rhs, level, R, dict(p), initial=None if start is None else start.copy())
        ud, idv = openmg_amd.mgCycle(A, torch.tensor(rhs, device="cuda"), level, R, dict(p),
                                     initial=None if start is None else torch.tensor(start, device="cuda"))
        assert isinstance(ud, torch.Tensor) and ud.is_cuda
        assert np.array_equal(ud.cpu().numpy(), uh) and idv["norm"] == ih["norm"], (shape_key, alpha, level)
        seen.append(uh)
assert np.array_equal(seen[0], seen[6]) and not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[2], seen[4])
print("device arrays ok")
"""


def test_mgcycle_with_device_arrays_has_the_bits_of_the_host_calls():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "device arrays ok" in p.stdout, p.stderr[-3000:]


# ---------------------------------------------------------------- 7. PCG and mixed precision --
def fcg_restated(pr, shape, alpha, pre, post, tol, maxit):
    """FCG(1), Polak-Ribiere (tests/test_gpu_pcg.py fcg_cpu), one restated cycle from zero per iteration."""
    A, R, b = pr["A"], pr["R"], pr["b7"]
    P = prolongations(R, alpha)
    M = lambda r: restated_cycle(A, R, P, r, 0, len(R), pre, post, shape, pr["sm"])
    x = np.zeros_like(b)
    r = b - A[0] @ x
    z = M(r)
    p = z.copy()
    rho = r @ z
    norms = []
    for _ in range(maxit):
        q = A[0] @ p
        a = rho / (p @ q)
        x += a * p
        r -= a * q
        norms.append(np.linalg.norm(r))
        if norms[-1] < tol:
            break
        z = M(r)
        beta = -a * (z @ q) / rho
        rho = r @ z
        p = z + beta * p
    return np.array(norms), x


def defect_correction_restated(pr, shape, alpha, pre, post, tol, maxit):
    """x += M(b - A x): what dtype='mixed' iterates in fp64 around its fp32 cycles."""
    A, R, b = pr["A"], pr["R"], pr["b7"]
    P = prolongations(R, alpha, np.float32)
    x = np.zeros_like(b)
    norms, xs = [], []
    for _ in range(maxit):
        x = x + restated_cycle(A, R, P, b - A[0] @ x, 0, len(R), pre, post, shape, pr["sm"])
        norms.append(np.linalg.norm(b - A[0] @ x))
        xs.append(x.copy())
        if norms[-1] < tol:
            break
    return np.array(norms), xs


def true_norm(A0, b, x):
    return np.linalg.norm(b - A0 @ x)


def same_norm(got, A0, b, x, rtol):
    """tests/test_gpu_mixed.py: got == ||b - A0 x|| to rtol, up to the rounding of forming b - A0 x in fp64 at all"""
    t = true_norm(A0, b, x)
    floor = 1e-14 * (np.linalg.norm(b) + np.linalg.norm(abs(A0) @ np.abs(x)))
    return abs(got - t) <= rtol * t + floor


def problem7():
    pr = dict(problem("poisson32"))
    pr["b7"] = np.random.default_rng(7).standard_normal(pr["b"].size)
    return pr


def test_pcg_with_an_over_corrected_f_cycle(monkeypatch):
    pr = problem7()
    b = pr["b7"]
    tol = 1e-8 * np.linalg.norm(b)
    want_norms, want_x = fcg_restated(pr, "F", 1.8, 1, 1, tol, 200)
    plain_norms, _ = fcg_restated(pr, "V", 1.0, 1, 1, tol, 200)
    assert len(want_norms) < len(plain_norms), (len(want_norms), len(plain_norms))
    with open_hierarchy(pr, monkeypatch) as h:
        h.set_cycle("F", 1.8)
        h.resident_load(b)
        its, norms, tn, bd = h.resident_pcg(1, 1, 200, tol)
        x = h.resident_fetch()
    print("FCG iterations: device %d, restatement %d (plain V-cycle preconditioner: %d)" % (its, len(want_norms), len(plain_norms)))
    assert not bd
    assert abs(its - len(want_norms)) <= 1, (its, len(want_norms))
    m = min(its, len(want_norms))
    np.testing.assert_allclose(norms[:m], want_norms[:m], rtol=1e-8)
    np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
    assert tn <= 2 * tol
    true = true_norm(pr["A"][0], b, x)
    assert abs(tn - true) <= 1e-12 * true + 1e-14 * np.linalg.norm(b), (tn, true)
    # through mgSolve (its own Galerkin products: the same iteration to rounding)
    u, info = openmg_amd.mgSolve(pr["A0"], b, solve_params(pr, cycles=0, threshold=tol, accel="cg", cycle="F", overCorrection=1.8))
    assert abs(info["cycle"] - len(want_norms)) <= 1
    np.testing.assert_allclose(u, want_x, rtol=0, atol=1e-8 * np.abs(want_x).max())
    assert info["norm"] <= 2 * tol


@pytest.mark.parametrize("accel", [None, "cg"])
def test_mixed_precision_with_an_over_corrected_f_cycle(monkeypatch, accel):
    pr = problem7()
    A0, b = pr["A"][0], pr["b7"]
    nb = np.linalg.norm(b)
    with open_hierarchy(pr, monkeypatch, dtype="mixed") as hm:
        assert hm.device_dtype() == np.float32
        hm.set_cycle("F", 1.8)
        hm.resident_load(b)
        if accel == "cg":
            want_norms, _ = fcg_restated(pr, "F", 1.8, 1, 1, 1e-10 * nb, 200)
            its, norms, tn, bd = hm.resident_pcg(1, 1, 200, 1e-10 * nb)
            xm = hm.resident_fetch()
            print("mixed FCG iterations: device %d, fp64 restatement %d" % (its, len(want_norms)))
            assert not bd
            assert its <= len(want_norms) + 2, (its, len(want_norms))
        else:
            want_norms, want_xs = defect_correction_restated(pr, "F", 1.8, 1, 1, 1e-10 * nb, 200)
            norms, xs = [], []
            for _ in range(len(want_norms) + 2):
                norms.append(hm.resident_cycle(1, 1))
                xs.append(hm.resident_fetch())
                if norms[-1] < 1e-10 * nb:
                    break
            print("mixed defect corrections: device %d, restatement %d" % (len(norms), len(want_norms)))
            for nk, xk in zip(norms, xs):
                assert same_norm(nk, A0, b, xk, 1e-12), (nk, true_norm(A0, b, xk))
            np.testing.assert_allclose(xs[0], want_xs[0], rtol=0, atol=1e-5 * np.abs(want_xs[0]).max())
            assert norms[-1] < 1e-10 * nb, (len(norms), norms[-1] / nb)
            tn, xm = norms[-1], xs[-1]
    tm = true_norm(A0, b, xm)
    assert same_norm(tn, A0, b, xm, 1e-12), (tn, tm)
    assert tm <= 1e-10 * nb, tm / nb
    # through mgSolve: the same count, a true fp64 norm
    u, info = openmg_amd.mgSolve(pr["A0"], b, solve_params(pr, cycles=0, threshold=1e-10 * nb, accel=accel, dtype="mixed",
                                                         cycle="F", overCorrection=1.8))
    assert true_norm(A0, b, u) <= 1e-10 * nb and same_norm(info["norm"], A0, b, u, 1e-12)


# ------------------------------------------------------------------------------- 8. convergence --
def restated_count(pr, shape, alpha, tol, limit):
    P = prolongations(pr["R"], alpha)
    x, norms = None, []
    while len(norms) < limit:
        x = restated_cycle(pr["A"], pr["R"], P, pr["b8"], 0, len(pr["R"]), 1, 1, shape, pr["sm"], x)
        norms.append(restated_norm(pr["A"], pr["b8"], x))
        if norms[-1] < tol:
            break
    return norms


def test_cycles_to_1e8_equal_the_restatement_and_f_needs_a_quarter_of_v(monkeypatch):
    """7-point 64^3, 5 grids, V(1,1), red-black, a seeded random right-hand side, target 1e-8 ||b||: the device needs the
    restatement's number of cycles for (V, 1) and for (F, 1.8) — no norm of the restatement lies within 1e-9 relative of the
    target, ten times the parity gate, so rounding cannot move a count — and the restatement's F(1.8) count is at most a
    quarter of its V count (13 against 86 when this was written)."""
    pr = dict(problem("poisson64"))
    pr["b8"] = np.random.default_rng(2024).standard_normal(pr["b"].size)
    tol = 1e-8 * np.linalg.norm(pr["b8"])
    counts = {}
    for shape, alpha in (("V", 1.0), ("F", 1.8)):
        norms = restated_count(pr, shape, alpha, tol, 150)
        assert norms[-1] < tol
        assert min(abs(nk - tol) for nk in norms) > 1e-9 * tol
        u, info = openmg_amd.mgSolve(pr["A0"], pr["b8"], solve_params(pr, cycles=0, threshold=tol, cycle=shape, overCorrection=alpha))
        print("%s alpha %.1f: device %d cycles, restatement %d; last norm rel diff %.2e"
              % (shape, alpha, info["cycle"], len(norms), rel(info["norm"], norms[-1])))
        assert info["cycle"] == len(norms), (shape, alpha, info["cycle"], len(norms))
        assert rel(info["norm"], norms[-1]) < 1e-8                # (1e-10 per cycle compounds over up to 86 of them)
        assert abs(info["norm"] - true_norm(pr["A0"], pr["b8"], u)) <= 1e-6 * info["norm"]
        counts[shape] = len(norms)
    assert 4 * counts["F"] <= counts["V"], counts
