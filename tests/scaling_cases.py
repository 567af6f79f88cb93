"""What tests/test_scaling_host.py and tests/test_gpu_scaling.py share: the operators, right-hand sides and power-of-two
scale pairs of the rescaling tests, and the bitwise comparison.

Multiplying by 2^k is exact in IEEE arithmetic while nothing under- or overflows, so an algorithm without a hidden
absolute constant gives cycle(2^ka A, 2^kb b) = 2^(kb - ka) cycle(A, b) BIT FOR BIT, every residual norm times 2^kb.
A pair is (ka, kb); a sign of -1 negates both A and b (also exact; the iterate is then unchanged)."""
import contextlib
import functools
import math
import os

import numpy as np
import scipy.sparse as sp

from openmg_amd import operators
from oracle import mg_oracle as orc

import stencils

SWEEPS = ((1, 1), (1, 0))
CYCLES = 3
PAIRS32 = [(24, -24), (-30, 30)]


def edge_exponents(c3):
    """(k just inside, k just outside) for |c3| 2^k against 2^400, then against 2^-400: plane.hip's fast_div is
    0x1p-400 <= |c3| <= 0x1p400."""
    m, e = math.frexp(abs(float(c3)))                       # |c3| = m 2^e, 0.5 <= m < 1
    hi_in = 400 - e + (1 if m == 0.5 else 0)                # the largest k with |c3| 2^k <= 2^400
    lo_in = -399 - e                                        # the smallest k with |c3| 2^k >= 2^-400
    ks = (hi_in, hi_in + 1, lo_in, lo_in - 1)
    inside = [2.0 ** -400 <= math.ldexp(abs(float(c3)), k) <= 2.0 ** 400 for k in ks]
    assert inside == [True, False, True, False], (c3, ks, inside)
    return ks


def pairs64(c3):
    """baseline, moderate, large on A only, large on b only, and ka = kb = k at both edges of fast_div.
    |kb - ka| <= 300 and |kb| <= 420: the sum of squares of a norm stays finite in double."""
    out = [(0, 0), (40, -60), (-300, 0), (0, 300)] + [(k, k) for k in edge_exponents(c3)]
    assert all(abs(kb - ka) <= 300 and abs(kb) <= 420 for ka, kb in out), out
    return out


def pair_id(p):
    return "A%+d_b%+d" % p


def scaled(M, factor):
    """factor * M with the stored pattern and order of M"""
    M = sp.csr_matrix(M)
    return sp.csr_matrix((M.data * factor, M.indices.copy(), M.indptr.copy()), shape=M.shape)


def galerkin(A0, Rs):
    """[A0, R0 A0 R0^T, ...] with sorted columns"""
    A = [sp.csr_matrix(A0)]
    for R in Rs:
        Ac = sp.csr_matrix((R @ A[-1]) @ R.T)
        Ac.sort_indices()
        A.append(Ac)
    return A


def aggregations(shape, grids):
    sh, Rs = tuple(shape), []
    for _ in range(grids - 1):
        Rs.append(stencils.line_aggregation(sh[0]) if len(sh) == 1 else stencils.aggregation(sh))
        sh = tuple(s // 2 for s in sh)
    return Rs


def grid_laplacian(shape):
    """the grid's graph Laplacian (pure Neumann: zero row sums), sorted CSR — tests/test_gpu_nullspace.py's"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols = [], []
    for ax in range(len(shape)):
        lo, hi = [slice(None)] * len(shape), [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)], idx[tuple(hi)]
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
    W = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A = sp.csr_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
    A.sort_indices()
    return A


def regularised_solve(A, b):
    """the coarse solve of a constant-null-space hierarchy (tests/test_gpu_nullspace.py): (Ac + gamma ones)^-1 b"""
    Ad = A.toarray() if sp.issparse(A) else np.asarray(A)
    n = Ad.shape[0]
    gamma = (float(np.trace(Ad)) / n) / n
    return np.ravel(np.linalg.solve(Ad + gamma * np.ones((n, n)), np.asarray(b, dtype=np.float64).reshape(-1)))


@functools.lru_cache(maxsize=None)
def irregular():
    """One operator of tests/test_gpu_property.py's banded_operators(): the derandomised draw with the most stored
    entries per row among the first few (unsorted stored order, per-entry values, a few perturbed rows)."""
    from hypothesis import HealthCheck, given, settings
    from test_gpu_property import banded_operators
    got = []

    @settings(deadline=None, max_examples=12, suppress_health_check=list(HealthCheck), derandomize=True, database=None)
    @given(banded_operators())
    def draw(case):
        got.append(case[0])

    draw()
    A = max((M for M in got if M.shape[0] <= 1500), key=lambda M: M.nnz / M.shape[0])
    A = sp.csr_matrix((A.data.copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    A.has_sorted_indices = False
    return A


def pair_restriction(n):
    pairs = np.arange(n) // 2
    return sp.csr_matrix((np.full(n, 0.5), (pairs, np.arange(n))), shape=(int(pairs[-1]) + 1, n))


@functools.lru_cache(maxsize=None)
def family(name, shape, grids):
    """(A0, [R], b, x0) of an operator family on `shape` over `grids` grids; nothing of it is ever modified.
    poisson: the 7- / 5- / 3-point Laplacian with the plain aggregation; reference: the same with the reference's own
    restriction (what from_fine builds); rows: the Laplacian with rows scaled by a few factors (per-row coefficients);
    line: the 1-D (-1, 2.5, -1) operator; var7 / s27: variable 7- and 27-point coefficients; irregular: see irregular();
    neumann: the grid's graph Laplacian."""
    rng = np.random.default_rng(97)
    if name in ("poisson", "reference"):
        A0 = sp.csr_matrix(operators.stencil_poisson(shape))
    elif name == "rows":
        from test_gpu_march import scaled_rows
        A0 = scaled_rows(operators.stencil_poisson(shape), np.random.default_rng(11))
    elif name == "line":
        A0 = stencils.stencil_constant(shape, (0, 0, -1.0, 2.5, -1.0, 0, 0))
    elif name == "var7":
        A0 = sp.csr_matrix(operators.stencil7_variable(shape, 2024))
    elif name == "s27":
        A0 = sp.csr_matrix(operators.stencil27_variable(shape, 2024))
    elif name == "irregular":
        A0 = irregular()
    elif name == "neumann":
        A0 = grid_laplacian(shape)
    else:
        raise KeyError(name)
    if name in ("reference", "neumann"):
        Rs = orc.restriction_list(shape, grids - 2, 4)
        assert len(Rs) == grids - 1
    elif name == "irregular":
        assert grids == 2
        Rs = [pair_restriction(A0.shape[0])]
    else:
        Rs = aggregations(shape, grids)
    n = A0.shape[0]
    b = rng.standard_normal(n)
    if name == "neumann":
        b = b + 0.3
    x0 = rng.standard_normal(n)
    for v in (b, x0, A0.data):
        v.setflags(write=False)
    return A0, Rs, b, x0


def diagonal_of(name, shape, grids):
    """the diagonal the edge pairs are chosen from: the largest of the fine operator"""
    return float(np.abs(family(name, shape, grids)[0].diagonal()).max())


def as_float32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def factors(pair, sign=1):
    """(s, t, t / s) of a pair: the factors of A, of b, and of x"""
    ka, kb = pair
    return sign * math.ldexp(1.0, ka), sign * math.ldexp(1.0, kb), math.ldexp(1.0, kb - ka)


def same_bits(got, want):
    """equal as bits: the sign of a zero counts (np.array_equal does not see it)"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def differing(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    return int(bad.size), [(int(i), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:3]]


def assert_equivariant(base, other, pair, sign=1, what=""):
    """base / other: lists of ('x', array) | ('b', array) | ('norms', array) | ('count', int) from the same calls on
    (A, b, x0) and on (s A, t b, (t / s) x0): iterates scale by t / s, what is linear in b alone by t, norms by |t|,
    counts stay."""
    s, t, f = factors(pair, sign)
    assert len(base) == len(other)
    for k, ((kind, u), (kind2, v)) in enumerate(zip(base, other)):
        assert kind == kind2
        if kind in ("x", "b"):
            want = np.asarray(u) * (f if kind == "x" else t)
            assert np.all(np.isfinite(v)), (what, pair, sign, k, "not finite")
            assert same_bits(v, want), (what, pair, sign, k) + differing(v, want)
        elif kind == "norms":
            u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
            assert u.shape == v.shape and np.all(v == abs(t) * u), (what, pair, sign, k, "norms", list(v), list(abs(t) * u))
        else:
            assert u == v, (what, pair, sign, k, kind, u, v)


@contextlib.contextmanager
def environment(env):
    """the switches of a case, for the hierarchies made inside the block"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
