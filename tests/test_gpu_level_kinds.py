"""Hierarchies whose levels are of DIFFERENT kinds: a row-kernel level above a plane, a var7 or a 27-point level, and the
reverse — the pairs for which a parent decides how its child's zero iterate comes about (hierarchy.hip enter_child: told
x_zero, cleared or first-relaxed by the restricting launch, or a memset).  The other cycle tests run levels of one kind, or a
pass level above small row-kernel levels.

32 x 32 x 32, four levels (32^3, 16^3, 8^3 smoothed, 4^3 solved directly), the oracle's Galerkin lists, red-black /
8-colour Gauss-Seidel.  One level is forced onto the row kernels by storing its operator with every row's columns in
DESCENDING order — the same operator; the plans take ascending columns only —, the others are stored sorted.  Kinds, as
omg_hierarchy_level_flags reports them: [K, rows, ...] and [rows, K, ...] for K = plane, var7 (OMG_VAR7_MIN=4096: a 16^3
level qualifies, the 8^3 level below it does not and runs the row kernels) and stencil27.  Level 2 (8^3) is stored sorted
and takes what it qualifies for — plane and stencil27: K again, var7: the row kernels —, printed with the others.

Gate: the fused passes against the set schedule of the SAME hierarchy (use_plane on / off) — the iterate bit for bit, the
norms to the tolerance tests/test_gpu_plane.py (plane) and tests/test_gpu_var7.py (var7, 27-point) hold fused against
set-by-set norms to — through every entry: single and batched resident cycles, vcycle_ex at levels 0 and 1, the zero-start
cycle on device vectors, and the resident cycles replayed from a graph; and one hierarchy per family against the
restatement of tests/test_gpu_cycle_shapes.py at that file's gates.  Needs an MI355X: run with -m gpu."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from openmg_amd import _hip, operators
from oracle import mg_oracle as orc
from test_gpu_cycle_shapes import CYC, device_cycles, norm_floor, norms_agree, restated_cycles
from test_gpu_plane import close as plane_norms_close

pytestmark = pytest.mark.gpu

SHAPE = (32, 32, 32)
SWEEPS = [(1, 1), (2, 1), (1, 0), (0, 1), (2, 2)]
FAMILIES = {"plane": (operators.stencil_poisson, {}),
            "var7": (operators.stencil7_variable, {"OMG_VAR7_MIN": "4096"}),
            "stencil27": (operators.stencil27_variable, {})}
ROWS_LEVEL = {"K_rows": 1, "rows_K": 0}


def descending(A):
    """The same CSR operator with every row's columns stored in descending order."""
    A = sp.csr_matrix(A).sorted_indices()
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    flip = A.indptr[row] + A.indptr[row + 1] - 1 - np.arange(A.nnz)
    D = sp.csr_matrix((A.data[flip], A.indices[flip], A.indptr.copy()), shape=A.shape)
    assert not np.all(np.diff(D.indices[:D.indptr[1]]) > 0) and abs(D - A).nnz == 0
    return D


@functools.lru_cache(maxsize=None)
def lists(family):
    make, env = FAMILIES[family]
    A0 = make(SHAPE)
    R = orc.restriction_list(SHAPE, 2, 1)
    A = [sp.csr_matrix(M).sorted_indices() for M in orc.coefficient_list(A0, R)]
    assert [M.shape[0] for M in A] == [32768, 4096, 512, 64]
    rng = np.random.default_rng(12345)
    b = A[0] @ rng.random(A[0].shape[0])
    return {"A0": A[0], "A": A, "R": R, "b": b, "x0": rng.standard_normal(b.size), "x1": rng.standard_normal(A[1].shape[0]),
            "b1": np.asarray(R[0] @ b).ravel(), "sm": orc.make_smoother("colour", A), "env": env}


def kinds_of(h):
    out = []
    for l in range(3):
        f = h.level_flags(l)
        assert not f["march"] and not f["line"]
        fused = [k for k in ("plane", "var7", "stencil27") if f[k]]
        assert len(fused) <= 1, f
        out.append(fused[0] if fused else "rows")
    return out


def open_mixed(family, order, monkeypatch):
    pr = lists(family)
    for k, v in pr["env"].items():
        monkeypatch.setenv(k, v)
    A = [descending(M) if l == ROWS_LEVEL[order] else M for l, M in enumerate(pr["A"])]
    h = _hip.Hierarchy(A, pr["R"], smoother="colour")
    kinds = kinds_of(h)
    print(family, order, "level kinds:", kinds)
    assert kinds[:2] == ([family, "rows"] if order == "K_rows" else ["rows", family]), kinds
    assert kinds[2] in (family, "rows"), kinds
    return pr, h


class DeviceVectors:
    """b and a NaN-filled x in HBM, from the HIP runtime the library itself is linked against (tests/test_gpu_plane.py)"""

    def __init__(self, b):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.b, self.bd, self.xd = b, ctypes.c_void_p(), ctypes.c_void_p()

    def __enter__(self):
        x = np.full(self.b.size, np.nan)
        assert self.hip.hipMalloc(ctypes.byref(self.bd), self.b.nbytes) == 0 and self.hip.hipMalloc(ctypes.byref(self.xd), x.nbytes) == 0
        assert self.hip.hipMemcpy(self.bd, self.b.ctypes.data, self.b.nbytes, 1) == 0
        assert self.hip.hipMemcpy(self.xd, x.ctypes.data, x.nbytes, 1) == 0
        return self

    def fetch(self):
        x = np.empty(self.b.size)
        assert self.hip.hipMemcpy(x.ctypes.data, self.xd, x.nbytes, 2) == 0
        return x

    def __exit__(self, *exc):
        self.hip.hipFree(self.bd)
        self.hip.hipFree(self.xd)


def resident_entries(h, pr, pre, post):
    """two single cycles, then three batched ones: (norms, iterates)"""
    h.resident_load(pr["b"], pr["x0"])
    norms = [h.resident_cycle(pre, post) for _ in range(2)]
    xs = [h.resident_fetch()]
    norms += h.resident_cycles(pre, post, 3)
    xs.append(h.resident_fetch())
    return norms, xs


def every_entry(h, pr, pre, post):
    norms, xs = resident_entries(h, pr, pre, post)
    for level, b, start in ((0, pr["b"], pr["x0"]), (1, pr["b1"], pr["x1"])):
        x_out, x_pre = np.full(b.size, np.nan), np.full(b.size, np.nan)
        norms.append(h.vcycle_ex(b, start.copy(), x_out, x_pre, pre, post, level))
        xs += [x_out, x_pre]
    with DeviceVectors(pr["b"]) as d:                       # the zero-start cycle: no norm
        h.cycle_dev(d.bd.value, d.xd.value, pre, post)
        h.sync()
        xs.append(d.fetch())
    h.use_graph(True)
    try:
        n, x = resident_entries(h, pr, pre, post)
    finally:
        h.use_graph(False)
    return norms + n, xs + x


@pytest.mark.parametrize("shape", ["V", "F"])
@pytest.mark.parametrize("order", sorted(ROWS_LEVEL))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_mixed_kinds_have_the_bits_of_the_set_schedule(monkeypatch, family, order, shape):
    pr, h = open_mixed(family, order, monkeypatch)
    with h:
        h.set_cycle(shape, 1.0)                             # (F: the second visit enters the child with nothing skipped)
        for pre, post in SWEEPS:
            h.use_plane(True)
            assert kinds_of(h)[ROWS_LEVEL[order] ^ 1] == family
            got = every_entry(h, pr, pre, post)
            h.use_plane(False)
            assert kinds_of(h) == ["rows"] * 3
            want = every_entry(h, pr, pre, post)
            for k, (xg, xw) in enumerate(zip(got[1], want[1])):
                assert not np.isnan(xw).any()
                assert np.array_equal(xg, xw), (family, order, shape, pre, post, k, int(np.sum(xg != xw)))
            worst = max(abs(a - c) / abs(c) for a, c in zip(got[0], want[0]))
            print("%s %s %s V(%d,%d): %d iterates equal, norms rel diff %.2e" % (family, order, shape, pre, post, len(got[1]), worst))
            if family == "plane":
                assert plane_norms_close(got[0], want[0]), (pre, post, got[0], want[0])
            else:
                np.testing.assert_allclose(got[0], want[0], rtol=1e-12)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_rows_parent_above_a_fused_child_against_the_restatement(monkeypatch, family):
    pr, h = open_mixed(family, "rows_K", monkeypatch)
    failures = []
    with h:
        for shape in ("V", "F"):
            h.set_cycle(shape, 1.0)
            for pre, post in SWEEPS:
                want_norms, want_x = restated_cycles(pr, shape, 1.0, pre, post, 3)
                norms, x = device_cycles(h, pr["b"], pre, post, 3)
                d = max(abs(a - c) / c for a, c in zip(norms, want_norms))
                print("%s %s V(%d,%d): norms rel diff %.2e, iterate max diff %.2e" % (family, shape, pre, post, d, np.abs(x - want_x).max()))
                if not (norms_agree(norms, want_norms, norm_floor(pr["A0"], pr["b"], want_x)) and np.allclose(x, want_x, **CYC)):
                    failures.append((shape, pre, post, d, float(np.abs(x - want_x).max())))
    assert not failures, failures
