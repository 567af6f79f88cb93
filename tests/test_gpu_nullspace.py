"""Singular operators with the constant null space (pure Neumann, periodic): Hierarchy(nullspace='constant') and
parameters['nullspace'].  Needs an MI355X.

The CPU yardstick is the oracle's own cycle (orc.mg_cycle with orc.make_smoother) with ONE function swapped through
monkeypatch: orc.coarse_solve becomes np.linalg.solve(Ac + gamma 1 1^T, b), gamma = (sum_i a_ii / n) / n — the
regularised solve the device's coarse solver inverts for.  The oracle's b is projected first (a b with a mean stalls at
|mean b| sqrt(n)), the oracle's iterate before it is compared with the fetched one (Gauss-Seidel lets its mean drift).

Gates are the project's own: 1e-10 relative on every cycle's norm and rtol 1e-9 of max|x| on the iterate
(tests/test_gpu_parity.py), rtol 1e-10 of max|x| on a coarse solve (tests/test_gpu_coarse.py); fp32 follows the fp64
yardstick to 1e-3 on norms and 1e-3 max|x| on the iterate (tests/test_gpu_fp32.py)."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

EPS = {"float64": float(np.finfo(np.float64).eps), "float32": float(np.finfo(np.float32).eps)}


# ---- operators -----------------------------------------------------------------------------------------------------
def grid_laplacian(shape, periodic=False):
    """the grid's graph Laplacian (diagonal = number of neighbours; periodic: wrap-around couplings), sorted CSR"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols = [], []
    for ax in range(len(shape)):
        if periodic:
            a, b = idx, np.roll(idx, -1, axis=ax)
        else:
            lo = [slice(None)] * len(shape)
            hi = [slice(None)] * len(shape)
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            a, b = idx[tuple(lo)], idx[tuple(hi)]
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
    W = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A = sp.csr_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
    A.sort_indices()
    return A


def neumann_var(shape, seed=2024):
    """operators.stencil7_variable with its diagonal replaced by minus the sum of its off-diagonals: zero row sums, the
    pattern and the symmetry of the operator tests/test_gpu_var7.py runs through the fused passes"""
    A = sp.csr_matrix(operators.stencil7_variable(shape, seed))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    off = np.where(A.indices == rows, 0.0, A.data)
    diag = -np.add.reduceat(off, A.indptr[:-1])
    A.data = np.where(A.indices == rows, diag[rows], A.data)
    return A


@functools.lru_cache(maxsize=None)
def lists(kind, shape, restrictions, min_size=4, factor=1.0):
    """(A, R) by the oracle's restriction_list / coefficient_list; never modified"""
    A0 = {"neumann": lambda: grid_laplacian(shape), "periodic": lambda: grid_laplacian(shape, True), "var": lambda: neumann_var(shape)}[kind]()
    if factor != 1.0:
        A0 = sp.csr_matrix((factor * A0.data, A0.indices, A0.indptr), shape=A0.shape)
    R = orc.restriction_list(shape, restrictions - 1, min_size)
    assert len(R) == restrictions
    return orc.coefficient_list(A0, R), R


def gamma_of(Ac):
    n = Ac.shape[0]
    return (float(Ac.diagonal().sum()) / n) / n


def regularised_solve(A, b):
    """what replaces orc.coarse_solve: np.linalg.solve(Ac + gamma ones, b)"""
    Ad = A.toarray() if sp.issparse(A) else np.asarray(A)
    n = Ad.shape[0]
    return np.ravel(np.linalg.solve(Ad + gamma_of(sp.csr_matrix(Ad)) * np.ones((n, n)), np.asarray(b, dtype=np.float64).reshape(-1)))


def mean_of(x):
    return math.fsum(x) / x.size


def yardstick(A, R, b, x0, pre, post, n_cycles, kind, omega=2.0 / 3.0):
    """the oracle's cycles on the projected b; the iterate projected on the way out"""
    sm = orc.make_smoother(kind, A, omega)
    p = {"coarsestLevel": len(R), "preIterations": pre, "postIterations": post}
    bp = b - mean_of(b)
    x = None if x0 is None else x0.copy()
    norms = []
    for _ in range(n_cycles):
        x, info = orc.mg_cycle(A, bp, 0, R, p, initial=x, smoother=sm)
        norms.append(info["norm"])
    return norms, x - mean_of(x)


def device_cycles(h, b, x0, pre, post, n_cycles):
    h.resident_load(b, x0)
    norms = h.resident_cycles(pre, post, n_cycles)
    return norms, h.resident_fetch()


# ---- 1. the projection kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_projection_kernel(dtype):
    """levels of 8, 64, 512, 4096 rows (less than a wave, one workgroup, several) and 16 * 20 * 36 = 11520 (no power of two,
    no multiple of 1024), in the levels' colour orderings"""
    from test_gpu_plane import aggregation
    eps = EPS[dtype]
    A, R = lists("neumann", (16, 16, 16), 3)
    B0 = operators.stencil_poisson((16, 20, 36))                          # (Dirichlet: an ordinary hierarchy, a plane level)
    RB = aggregation((16, 20, 36))
    BC = sp.csr_matrix((RB @ B0) @ RB.T)
    rng = np.random.default_rng(11)
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype, nullspace="constant") as h, \
            _hip.Hierarchy([B0, BC], [RB], smoother="colour", dtype=dtype) as g:
        assert h.nullspace == "constant" and g.nullspace is None          # (project works on either)
        assert h.sizes == [4096, 512, 64, 8] and g.sizes[0] == 11520
        for hh, level in [(h, 3), (h, 2), (h, 1), (h, 0), (g, 0)]:
            n = hh.sizes[level]
            x = rng.standard_normal(n) + 0.7
            keep = x.copy()
            y, mean = hh.project(level, x)
            assert np.array_equal(x, keep)                                 # (the caller's array is not written)
            big = np.abs(x).max()
            bound = (1e-13 if dtype == "float64" else 4 * eps) * big
            want_mean = mean_of(x)
            print("project", dtype, n, "max err %.3e  mean err %.3e  bound %.3e" % (np.abs(y - (x - want_mean)).max(), abs(mean - want_mean), bound))
            assert np.abs(y - (x - want_mean)).max() <= bound
            assert abs(mean - want_mean) <= bound
            y2, mean2 = hh.project(level, x)
            assert np.array_equal(y, y2) and mean == mean2                 # deterministic sums
            again, left = hh.project(level, y)
            print("        second projection removes %.3e (4 eps max|x| = %.3e)" % (left, 4 * eps * big))
            assert abs(left) <= 4 * eps * big


# ---- 2. the coarse solve -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,restrictions", [("neumann", (4, 4, 4), 1), ("neumann", (8, 8, 8), 1), ("periodic", (8, 8), 1),
                                                     ("var", (8, 8, 8), 2)])
def test_coarse_solve_is_the_pseudo_inverse_plus_a_constant(kind, shape, restrictions):
    A, R = lists(kind, shape, restrictions, 2)
    Ac = A[-1].toarray()
    n = Ac.shape[0]
    assert n == {("neumann", (4, 4, 4)): 8, ("neumann", (8, 8, 8)): 64, ("periodic", (8, 8)): 16, ("var", (8, 8, 8)): 8}[(kind, shape)]
    b = np.random.default_rng(3).standard_normal(n) + 0.25
    with _hip.Hierarchy(A, R, smoother="colour", nullspace="constant") as h:
        x = h.coarse_solve(b)
        assert h.coarse_info()["blocks"] == 1 and h.coarse_info()["n"] == n
    want = np.linalg.pinv(Ac) @ b
    tol = 1e-10 * np.abs(x).max()
    print("coarse", kind, shape, "pinv err %.3e  mean err %.3e  tol %.3e" % (np.abs((x - mean_of(x)) - want).max(), abs(mean_of(x) - mean_of(b) / (gamma_of(A[-1]) * n)), tol))
    assert np.abs((x - mean_of(x)) - want).max() <= tol
    assert abs(mean_of(x) - mean_of(b) / (gamma_of(A[-1]) * n)) <= tol


# ---- 3. cycles against the yardstick -------------------------------------------------------------------------------
CYCLE_CASES = [("neumann", (8, 8, 8), 2, "colour", "float64", False), ("neumann", (8, 8, 8), 2, "gs", "float64", False),
               ("neumann", (8, 8, 8), 2, "jacobi", "float64", False), ("periodic", (8, 8, 8), 2, "colour", "float64", False),
               ("periodic", (16, 16), 2, "gs", "float64", False), ("var", (16, 16, 16), 2, "colour", "float64", True),
               ("var", (16, 16, 16), 2, "colour", "float32", True)]


@pytest.mark.parametrize("kind,shape,restrictions,smoother,dtype,var7", CYCLE_CASES)
def test_cycles_against_the_regularised_oracle(monkeypatch, kind, shape, restrictions, smoother, dtype, var7):
    monkeypatch.setattr(orc, "coarse_solve", regularised_solve)
    if var7:
        monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    A, R = lists(kind, shape, restrictions, 8 if var7 else 4)
    n = A[0].shape[0]
    rng = np.random.default_rng(7)
    b = rng.standard_normal(n) + 0.3
    x0 = rng.standard_normal(n)
    norm_tol, x_tol = (1e-10, 1e-9) if dtype == "float64" else (1e-3, 1e-3)
    omega = 2.0 / 3.0
    with _hip.Hierarchy(A, R, smoother=smoother, omega=omega if smoother == "jacobi" else 1.0, dtype=dtype, nullspace="constant") as h:
        assert bool(h.level_flags(0)["var7"]) == var7
        for pre, post, cycles in ((1, 1, 3), (2, 1, 1)):
            for start in (None, x0):
                want_norms, want_x = yardstick(A, R, b, start, pre, post, cycles, smoother, omega)
                norms, x = device_cycles(h, b, start, pre, post, cycles)
                for k in range(cycles):
                    print(kind, shape, smoother, dtype, (pre, post), "zero" if start is None else "random", "cycle", k,
                          "norm rel diff %.3e" % (abs(norms[k] - want_norms[k]) / want_norms[k]))
                    assert abs(norms[k] - want_norms[k]) <= norm_tol * want_norms[k]
                print("    iterate diff %.3e of max|x| %.3e" % (np.abs(x - want_x).max(), np.abs(want_x).max()))
                assert np.abs(x - want_x).max() <= x_tol * np.abs(want_x).max()
                if var7:
                    h.use_plane(False)
                    norms_s, x_s = device_cycles(h, b, start, pre, post, cycles)
                    h.use_plane(True)
                    assert np.array_equal(x, x_s)                           # the fused passes: the set schedule's bits
                    np.testing.assert_allclose(norms, norms_s, rtol=1e-12 if dtype == "float64" else 1e-6)
        # F-cycles with over-correction: the fused passes (where there are any) against the set-by-set schedule
        h.set_cycle("F", 1.8)
        got = device_cycles(h, b, x0, 1, 1, 2)
        h.use_plane(False)
        want = device_cycles(h, b, x0, 1, 1, 2)
        assert np.array_equal(got[1], want[1]) and np.all(np.isfinite(got[1]))
        np.testing.assert_allclose(got[0], want[0], rtol=1e-12 if dtype == "float64" else 1e-6)
        assert abs(mean_of(got[1])) <= 64 * EPS[dtype] * np.abs(got[1]).max()


# ---- 4. mgSolve end to end -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [{"accel": "cg"}, {"accel": "cg", "dtype": "mixed"}, {"cycle": "F", "overCorrection": 1.8}],
                         ids=["cg", "cg-mixed", "F-1.8"])
@pytest.mark.parametrize("kind", ["var", "neumann"])
def test_mgsolve_pure_neumann_end_to_end(monkeypatch, kind, extra):
    """FAILS WITHOUT THE FEATURE (all six cases, run against the parent build): the key is ignored, the coarsest operator's
    near-zero pivot gives corrections of size 1e16, FCG breaks down (RuntimeError in iteration 1 or 16) and the F-cycles use
    up all 200 cycles without reaching the threshold.  The counts taken with the feature are printed (15 / 15 / 20 on the
    variable-coefficient operator, 13 / 13 / 10 on the Neumann Laplacian: profiles/nullspace_128.txt); 'cycles' = 200 is only a
    cap against a run that never stops."""
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (16, 16, 16)
    A0 = neumann_var(shape) if kind == "var" else grid_laplacian(shape)
    n = A0.shape[0]
    b = A0 @ np.random.default_rng(12345).random(n) + 0.3
    assert abs(mean_of(b) - 0.3) < 1e-12
    keep = b.copy()
    bp = b - mean_of(b)
    threshold = 1e-8 * float(np.linalg.norm(bp))
    p = dict({"problemShape": shape, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "smoother": "colour", "minSize": 8,
              "nullspace": "constant", "threshold": threshold, "cycles": 200, "giveInfo": True}, **extra)
    u, info = openmg_amd.mgSolve(A0, b, dict(p))
    assert np.array_equal(b, keep)                                         # the caller's b is untouched
    print("mgSolve", kind, extra, "took", info["cycle"], "cycles / iterations; norm %.3e (threshold %.3e)" % (info["norm"], threshold))
    assert info["norm"] < threshold
    host = float(np.linalg.norm(bp - A0 @ u))
    print("    SciPy's norm %.6e, returned %.6e, |mean u| %.3e, max|u| %.3e" % (host, info["norm"], abs(mean_of(u)), np.abs(u).max()))
    assert abs(host - info["norm"]) <= 1e-6 * info["norm"]
    assert abs(mean_of(u)) <= 1e-13 * np.abs(u).max()
    # without giveInfo the whole setup stays on the device (the variable-coefficient level runs the fused passes): the same u
    u_dev = openmg_amd.mgSolve(A0, b, dict(p, giveInfo=False))
    assert np.array_equal(u_dev, u)


class DeviceVector:
    """a float64 vector in HBM (hipMalloc / hipMemcpy / hipFree through the HIP runtime the library has loaded)"""

    def __init__(self, data):
        import ctypes
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        data = np.ascontiguousarray(data, dtype=np.float64)
        self.size = data.size
        self.d = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.d), data.nbytes) == 0
        assert self.hip.hipMemcpy(self.d, data.ctypes.data, data.nbytes, 1) == 0

    def host(self):
        out = np.empty(self.size)
        assert self.hip.hipMemcpy(out.ctypes.data, self.d, out.nbytes, 2) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.d)


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_device_arrays_are_projected_like_host_arrays(dtype):
    """omg_resident_load_dev / omg_resident_fetch_dev (what mgSolve calls for a device-array b): the bits of the host entries,
    the caller's device b untouched"""
    A, R = lists("neumann", (16, 16, 16), 2, 8)
    n = A[0].shape[0]
    rng = np.random.default_rng(4)
    b = rng.standard_normal(n) + 0.3
    x0 = rng.standard_normal(n) + 1.0
    with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype, nullspace="constant") as h:
        want = device_cycles(h, b, x0, 1, 1, 3)
        with DeviceVector(b) as bd, DeviceVector(x0) as xd, DeviceVector(np.zeros(n)) as out:
            h.resident_load_dev(bd.d.value, xd.d.value)
            norms = h.resident_cycles(1, 1, 3)
            h.resident_fetch_dev(out.d.value)
            assert norms == want[0] and np.array_equal(out.host(), want[1])
            assert np.array_equal(bd.host(), b) and np.array_equal(xd.host(), x0)
        assert abs(mean_of(want[1])) <= 1e-13 * np.abs(want[1]).max()
        # a later cycle continues from the projected iterate: the residual does not see the null component
        more = h.resident_cycles(1, 1, 1)
        assert more[0] < want[0][-1]


# ---- 5. determinism and reuse --------------------------------------------------------------------------------------
def test_pcg_is_deterministic_on_a_nullspace_hierarchy():
    A, R = lists("neumann", (16, 16, 16), 2, 8)
    b = np.random.default_rng(5).standard_normal(A[0].shape[0]) + 0.3
    out = []
    with _hip.Hierarchy(A, R, smoother="colour", nullspace="constant") as h:
        for _ in range(2):
            h.resident_load(b)
            its, norms, true_norm, breakdown = h.resident_pcg(1, 1, 8)
            out.append((its, norms, true_norm, breakdown, h.resident_fetch()))
    assert out[0][0] == out[1][0] == 8 and not out[0][3]
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert np.array_equal(out[0][4], out[1][4])
    assert out[0][1][-1] < 1e-3 * out[0][1][0]


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_update_fine_keeps_the_null_space(monkeypatch, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (16, 16, 16)
    A1 = neumann_var(shape)
    A2 = sp.csr_matrix((2.0 * A1.data, A1.indices, A1.indptr), shape=A1.shape)
    b = np.random.default_rng(9).standard_normal(A1.shape[0]) + 0.3
    with _hip.Hierarchy.from_fine(A2, shape, 2, "colour", dtype=dtype, nullspace="constant") as fresh, \
            _hip.Hierarchy.from_fine(A1, shape, 2, "colour", dtype=dtype, nullspace="constant") as h:
        assert h.level_flags(0)["var7"] and h.nullspace == "constant"
        first = device_cycles(h, b, None, 1, 1, 3)
        h.update_fine(A2.data)
        assert h.nullspace == "constant" and h.coarse_info()["blocks"] == 1
        got = device_cycles(h, b, None, 1, 1, 3)
        want = device_cycles(fresh, b, None, 1, 1, 3)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[1], first[1])


def test_mgcycle_does_not_share_a_hierarchy_across_the_key():
    A, R = lists("neumann", (8, 8, 8), 2)
    A, R = list(A), list(R)
    b = np.random.default_rng(2).standard_normal(A[0].shape[0])
    b -= mean_of(b)
    p = {"coarsestLevel": 2, "preIterations": 1, "postIterations": 1, "smoother": "colour"}
    openmg_amd.clear_cache()
    try:
        x1, i1 = openmg_amd.mgCycle(A, b, 0, R, dict(p, nullspace="constant"))
        assert np.all(np.isfinite(x1)) and i1["norm"] < np.linalg.norm(b)
        for trust in (False, True):
            try:
                x2, _ = openmg_amd.mgCycle(A, b, 0, R, dict(p, trustOperators=trust))
            except _hip.HipError as e:
                assert e.code == _hip.ERR_SINGULAR                      # the plain hierarchy cannot factor the singular operator
            else:
                assert not np.array_equal(x2, x1)
        x3, _ = openmg_amd.mgCycle(A, b, 0, R, dict(p, nullspace="constant", trustOperators=True))
        assert np.array_equal(x3, x1)
    finally:
        openmg_amd.clear_cache()


def lists_dirichlet():
    shape = (4, 4, 4)
    R = orc.restriction_list(shape, 0, 2)
    return orc.coefficient_list(operators.stencil_poisson(shape), R), R


# ---- 6. errors -----------------------------------------------------------------------------------------------------
def test_errors():
    shape = (8, 8, 8)
    D = sp.csr_matrix(operators.poisson(shape))                           # Dirichlet: row sums far from zero
    R = orc.restriction_list(shape, 0, 4)
    A = orc.coefficient_list(D, R)
    with pytest.raises(_hip.HipError) as e:
        _hip.Hierarchy(A, R, smoother="colour", nullspace="constant")
    assert e.value.code == _hip.ERR_INVALID and "null space" in str(e.value)
    with pytest.raises(_hip.HipError) as e:
        openmg_amd.mgSolve(D, np.ones(512), {"problemShape": shape, "gridLevels": 1, "cycles": 1, "nullspace": "constant", "minSize": 4})
    assert e.value.code == _hip.ERR_INVALID
    # one level, a periodic chain of 16386 rows: refused before anything is factored
    n = 16386
    i = np.arange(n)
    ring = sp.csr_matrix((np.concatenate([2.0 * np.ones(n), -np.ones(n), -np.ones(n)]),
                          (np.concatenate([i, i, i]), np.concatenate([i, (i + 1) % n, (i - 1) % n]))), shape=(n, n))
    with pytest.raises(_hip.HipError) as e:
        _hip.Hierarchy([ring], [], nullspace="constant")
    assert e.value.code == _hip.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        openmg_amd.mgSolve(ring, np.ones(n), {"problemShape": (n,), "gridLevels": 1, "cycles": 1, "nullspace": "neumann"})
    # the multi-GPU runners refuse a tail hierarchy with a null space
    A, R = lists("neumann", (4, 4, 4), 1, 2)
    with _hip.Hierarchy(A, R, smoother="colour", nullspace="constant") as tail:
        for fn in ("omg_dist_set_tail", "omg_pdist_set_tail", "omg_sdist_set_tail"):
            assert getattr(_hip.lib(), fn)(None, tail._h) == _hip.ERR_UNSUPPORTED       # (asked before anything else)
    with _hip.Hierarchy(*lists_dirichlet(), smoother="colour") as tail:
        assert _hip.lib().omg_dist_set_tail(None, tail._h) == _hip.ERR_INVALID           # an ordinary tail: the null runner is what is wrong
