"""Operators, reference and yardsticks for the coarsest-level direct solvers (csrc/coarse.hip, dense.hip, sine_cube16.h).
CPU only: tests/test_coarse_cases_host.py checks this file against exact arithmetic, tests/test_gpu_coarse_edges.py
compares the device with it.

Reference: `refined_solve` — SuperLU with iterative refinement, the residual in double-double arithmetic (about 106
bits: with np.longdouble's 64 the corrections stall at kappa * 2^-64, above 2^-60 for kappa > 16), until the correction
is below 2^-60 max|x|; the result is the pair (hi, lo).

Unit: 2^-53 kappa_1(A) (fp32: 2^-24 kappa_1(A)) relative to max|x| — what a backward-stable solve in that precision may
lose.  `cond1` is ||A||_1 times SciPy's one-norm estimate of the inverse through the same factorisation.

Yardsticks: NumPy/SciPy restatements of the method class a path belongs to (never the library): the explicit inverse
np.linalg.inv(A) @ b for the inverse, substructuring and chain paths, a scipy.fft.dstn solve for the sine path,
np.linalg.inv(A).astype(float32) @ b32 for the fp32 products.  The device must stay within FACTOR = 8 times
max(yardstick error, one unit): the 8 is a supposition — other association and elimination order (64-lane strided sums and
a wave tree against BLAS) — not a measurement; a dropped k-step, a wrong tile or stale LDS misses by many orders more.

Extents are written x-fastest (gx, gy, gz); operators.stencil_poisson takes the reversed tuple."""
import functools
import zlib

import numpy as np
import scipy.fft
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from openmg_amd import operators

U64 = 2.0 ** -53
U32 = 2.0 ** -24
FACTOR = 8.0
LD = np.longdouble                                       # (only to subtract a candidate from the pair; the residual is double-double)


# ---- reference -----------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp's split and Dekker's product: no fused multiply-add needed)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _residual(A, b, hi, lo):
    """b - A (hi + lo) in double-double arithmetic (a mantissa of about 106 bits: products split exactly, every partial
    sum carried as a pair), rounded to double at the end.  The k-th stored entries of all rows are added in one step."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    pos = np.arange(A.nnz) - A.indptr[:-1][rows]
    order = np.argsort(pos, kind="stable")
    ends = np.cumsum(np.bincount(pos, minlength=1)) if A.nnz else np.zeros(1, dtype=np.int64)
    p, pe = _two_prod(A.data, hi[A.indices])
    q = A.data * lo[A.indices]
    s, e = b.astype(np.float64).copy(), np.zeros(n)
    start = 0
    for end in ends:
        sel = order[start:end]
        r = rows[sel]
        for term in (p[sel], pe[sel], q[sel]):
            s[r], err = _two_sum(s[r], -term)
            e[r] += err
        start = end
    return s + e


def _accumulate(hi, lo, d):
    """(hi, lo) <- hi + lo + d, renormalised"""
    s, err = _two_sum(hi, d)
    return _two_sum(s, lo + err)


def refined_solve(A, b, lu=None):
    """(hi, lo): A (hi + lo) = b to 2^-60 and better; hi is the solution rounded to double"""
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    lu = lu or spla.splu(sp.csc_matrix(A))
    hi = lu.solve(b)
    lo = np.zeros_like(hi)
    for _ in range(12):
        d = lu.solve(_residual(A, b, hi, lo))
        hi, lo = _accumulate(hi, lo, d)
        if np.abs(d).max() <= 2.0 ** -60 * np.abs(hi).max():
            return hi, lo
    raise RuntimeError("refined_solve: the corrections do not fall below 2^-60 max|x|")


def cond1(A, lu=None):
    A = sp.csc_matrix(A)
    lu = lu or spla.splu(A)
    inv = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"), dtype=np.float64)
    return float(abs(A).sum(axis=0).max()) * float(spla.onenormest(inv))


def error(x, ref):
    """max|x - (hi + lo)| / max|hi|, formed in extended precision"""
    hi, lo = ref
    d = np.abs((np.asarray(x, dtype=np.float64).astype(LD) - hi.astype(LD)) - lo.astype(LD)).max()
    return float(d / LD(np.abs(hi).max()))


# ---- operators -----------------------------------------------------------------------------------------------------
def banded_unsymmetric(n, w, rng, density=0.3):
    """tests/test_gpu_coarse.py's: strictly diagonally dominant, unsymmetric values and pattern, half-bandwidth exactly w,
    stored column order shuffled"""
    rows, cols, vals = [], [], []
    for off in range(-w, w + 1):
        if off == 0:
            continue
        keep = rng.random(n - abs(off)) < (1.0 if abs(off) == w else density)
        i = np.arange(max(0, -off), min(n, n - off))[keep]
        rows.append(i); cols.append(i + off); vals.append(rng.standard_normal(i.size))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    d = np.asarray(abs(A).sum(axis=1)).ravel() + 1.0
    A = sp.csr_matrix(A + sp.diags(d * np.where(rng.random(n) < 0.5, 1.0, -1.0)))
    for i in range(n):
        s, e = A.indptr[i], A.indptr[i + 1]
        q = rng.permutation(e - s)
        A.indices[s:e] = A.indices[s:e][q]
        A.data[s:e] = A.data[s:e][q]
    A.has_sorted_indices = False
    return A


def star(extents, coefficients=None):
    """constant-coefficient symmetric star stencil on gx x gy x gz, x fastest: (diagonal, x, y, z couplings);
    None: operators.stencil_poisson"""
    if coefficients is None:
        return operators.stencil_poisson(tuple(reversed(extents)))
    ext = tuple(extents) + (1,) * (3 - len(extents))
    T = [sp.diags([np.ones(m - 1), np.ones(m - 1)], [-1, 1], shape=(m, m)) if m > 1 else sp.csr_matrix((1, 1)) for m in ext]
    I = [sp.identity(m) for m in ext]
    n = ext[0] * ext[1] * ext[2]
    A = coefficients[0] * sp.identity(n) + coefficients[1] * sp.kron(I[2], sp.kron(I[1], T[0]))
    if ext[1] > 1:
        A = A + coefficients[2] * sp.kron(I[2], sp.kron(T[1], I[0]))
    if ext[2] > 1:
        A = A + coefficients[3] * sp.kron(T[2], sp.kron(I[1], I[0]))
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


ANISO = (5.0, -0.3, -1.1, 0.7)                           # tests/test_gpu_coarse.py sine_aniso's couplings


def dst_solve(extents, coefficients, b):
    """the sine path's yardstick: x = S (S b / lambda) with scipy's orthonormal DST-I along every axis"""
    c = coefficients or (2.0 * len(extents), -1.0, -1.0, -1.0)        # None: operators.stencil_poisson's
    shape = tuple(reversed(extents))
    lam = np.full(shape, c[0])
    for axis, m in enumerate(shape):
        coupling = c[len(shape) - axis]                  # the last axis of the C-ordered array is x
        view = [1] * len(shape)
        view[axis] = m
        lam = lam + 2.0 * coupling * np.cos(np.pi * np.arange(1, m + 1) / (m + 1)).reshape(view)
    t = scipy.fft.dstn(np.asarray(b, dtype=np.float64).reshape(shape), type=1, norm="ortho")
    return scipy.fft.dstn(t / lam, type=1, norm="ortho").reshape(-1)


def dense_dominant(n, rng):
    """dense, unsymmetric, diagonally dominant by rows"""
    M = rng.standard_normal((n, n))
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, (np.abs(M).sum(axis=1) + 1.0) * np.where(rng.random(n) < 0.5, 1.0, -1.0))
    return sp.csr_matrix(M)


def lower_plus_diagonal(n, rng):
    """dense below the diagonal, nothing above: the blocked inverse's zero tiles on one side only"""
    M = np.tril(rng.standard_normal((n, n)), -1)
    np.fill_diagonal(M, (np.abs(M).sum(axis=1) + 1.0) * np.where(rng.random(n) < 0.5, 1.0, -1.0))
    return sp.csr_matrix(M)


def block_permutation(n, rng, noise=0.05, weight=3.0, nb=64):
    """3 x (a derangement inside every 64-row diagonal block) + 0.05 noise everywhere, diagonal entries exactly zero: the
    blocked inverse must pivot INSIDE its diagonal blocks and succeeds"""
    M = noise * rng.standard_normal((n, n))
    for k0 in range(0, n, nb):
        m = min(nb, n - k0)
        while True:
            p = rng.permutation(m)
            if not np.any(p == np.arange(m)):
                break
        M[k0 + np.arange(m), k0 + p] += weight
    np.fill_diagonal(M, 0.0)
    return sp.csr_matrix(M)


def shifted_growth(n, eps, seed, nb=64):
    """3 P + eps * noise on the 64-row diagonal blocks, P the cyclic shift by 64: without pivoting across blocks every
    block step multiplies by (eps noise)^-1 * 3"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    M[np.arange(n), (np.arange(n) + nb) % n] = 3.0
    for k0 in range(0, n, nb):
        m = min(nb, n - k0)
        M[k0:k0 + m, k0:k0 + m] += eps * rng.standard_normal((m, m))
    return sp.csr_matrix(M)


def grid_laplacian(shape):
    """the grid's graph Laplacian (pure Neumann: zero row sums), C order, sorted CSR — tests/test_gpu_nullspace.py's"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols = [], []
    for ax in range(len(shape)):
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


def aggregation(shape):
    """pairwise averaging along every axis (even extents), C order: constant columns, so R A R^T keeps the constant null space
    (the oracle's restriction_list does not on extents that are no power of two)"""
    R = None
    for m in shape:
        assert m % 2 == 0
        one = sp.csr_matrix((np.full(m, 0.5), (np.arange(m) // 2, np.arange(m))), shape=(m // 2, m))
        R = one if R is None else sp.kron(R, one, format="csr")
    R = sp.csr_matrix(R)
    R.sort_indices()
    return R


@functools.lru_cache(maxsize=None)
def neumann_lists(shape):
    """(A, R): the Neumann Laplacian on `shape` and its Galerkin coarse operator under one aggregation"""
    A0 = grid_laplacian(shape)
    R = aggregation(shape)
    Ac = sp.csr_matrix((R @ A0) @ R.T)
    Ac.sort_indices()
    return [A0, Ac], [R]


def gamma_of(Ac):
    n = Ac.shape[0]
    return (float(Ac.diagonal().sum()) / n) / n


# ---- the host model of the blocked inverse (dense.hip blocked_inverse) ----------------------------------------------
def block_gauss_jordan(M, nb=64):
    """Gauss-Jordan in nb-row blocks, no pivoting across blocks (inside a block: whatever np.linalg.inv does)"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    W = np.hstack([M, np.eye(n)])
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        W[k0:k1] = np.linalg.inv(W[k0:k1, k0:k1]) @ W[k0:k1]
        C = W[:, k0:k1].copy()
        C[k0:k1] = 0.0
        W -= C @ W[k0:k1]
        W[:, k0:k1] = 0.0
        W[k0:k1, k0:k1] = np.eye(k1 - k0)
    return W[:, n:]


def acceptance_vector(n):
    i = np.arange(n)
    return np.where(i & 1, -1.0, 1.0) / (1.0 + i % 7)


def acceptance_residual(M, X):
    """the library's check of a blocked inverse: max|M (X v) - v| for its fixed v"""
    v = acceptance_vector(M.shape[0])
    return float(np.abs(M @ (X @ v) - v).max())


# ---- the library's admission rules, restated (coarse.hip CoarseSolver::build, build_chain, build_sine) -----------------
LDS_DOUBLES = 6144


def half_bandwidth(A):
    A = sp.coo_matrix(A)
    return max(1, int(np.abs(A.row.astype(np.int64) - A.col).max())) if A.nnz else 1


def admitted_blocks(n, w, forced, itemsize=8):
    """P of CoarseSolver::build for OMG_COARSE_BLOCKS=forced (0: its own choice): 1 where the rule refuses"""
    lds_cap = LDS_DOUBLES * (8 // itemsize)
    big = float(n) * n * itemsize > float(256 << 20)
    best, P = float(n) * n, 1
    if forced > 1 or (forced == 0 and big):
        for q in range(2, 65):
            gq = (q - 1) * w
            if gq >= n or gq > lds_cap or 2 * w > lds_cap:
                break
            mq = (n - gq + q - 1) // q
            if mq < 2 * w:
                break
            cost = float(q) * mq * mq + float(gq) * gq
            if forced == q or (forced == 0 and cost < best):
                best, P = cost, q
            if forced == q:
                break
    return P


def chain_blocks(n, w, forced_bs):
    """(bs, K) of build_chain for OMG_COARSE_CHAIN_BS=forced_bs (None: its own); a forced size below w is ignored"""
    bs = max((w + 63) // 64 * 64, 64)
    if forced_bs is not None and forced_bs >= w:
        bs = forced_bs
    bs = min(bs, n)
    return bs, (n + bs - 1) // bs


def sine_admitted(extents):
    n = int(np.prod(extents))
    return 2 <= n <= 8192 and extents[0] >= 2 and max(extents) <= 32


def sine_stride(extents):
    return 16 if max(extents) <= 16 else 32


def sine_lds_bytes(extents):
    g = tuple(extents) + (1,) * (3 - len(extents))
    return ((g[0] + 1) * g[1] * g[2] + 2 + (g[0] + g[1] + g[2]) * sine_stride(extents)) * 8


# ---- cases ---------------------------------------------------------------------------------------------------------
class Case:
    """name; family; make() -> CSR; env: the switches that force the path; blocks: coarse_info()['blocks'] expected;
    extents / coefficients: star stencils; yardstick: 'inverse' or 'dst'; forced: the q or bs the switches ask for;
    lists: the fine shape of a null-space case's own hierarchy (neumann_lists)"""

    def __init__(self, name, family, make, env=None, blocks=None, extents=None, coefficients=None, yardstick="inverse",
                 forced=None, lists=None):
        self.name, self.family, self.make, self.env, self.blocks = name, family, make, dict(env or {}), blocks
        self.extents, self.coefficients, self.yardstick, self.forced, self.lists = extents, coefficients, yardstick, forced, lists

    def __repr__(self):
        return self.name


def _seed(name):
    return zlib.crc32(name.encode())


def _rng(name):
    return np.random.default_rng(_seed(name))


SINE_SHAPES = [(2,), (3, 2), (5, 7, 6), (16, 16, 15), (16, 16, 16), (16, 15, 17), (17, 17, 17), (31, 16, 16), (32, 32, 8), (8, 32, 32), (32, 2)]
SINE_ABOVE_64K = {(31, 16, 16), (32, 32, 8), (8, 32, 32)}          # need the hipFuncSetAttribute branch
SINE_LEAVING = [(33, 8), (48, 48, 4)]                    # an extent above 32; n = 9216 > 8192 with blocks too short to substructure


def _shape_name(extents):
    return "x".join(str(e) for e in extents)


def sine_cases():
    out = []
    for ext in SINE_SHAPES:
        for tag, coef in (("poisson", None), ("aniso", ANISO)):
            out.append(Case("sine-%s-%s" % (tag, _shape_name(ext)), "sine", functools.partial(star, ext, coef), blocks=0,
                            extents=ext, coefficients=coef, yardstick="dst"))
    for ext in SINE_LEAVING:
        out.append(Case("sine-left-poisson-%s" % _shape_name(ext), "sine", functools.partial(star, ext, None), blocks=1,
                        extents=ext, coefficients=None, yardstick="dst"))
    return out


INVERSE_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 319, 320, 321, 1025]
INVERSE_ENV = {"OMG_COARSE_BLOCKS": "1"}


def inverse_cases():
    out = []
    for n in INVERSE_SIZES:
        name = "inverse-dense-%d" % n
        out.append(Case(name, "inverse", functools.partial(lambda n, name: dense_dominant(n, _rng(name)), n, name), INVERSE_ENV, 1, forced=1))
        for w in (5, 70):
            if n >= (63 if w == 5 else 255):             # banded_unsymmetric cannot build a band wider than n - 1
                name = "inverse-band%d-%d" % (w, n)
                out.append(Case(name, "inverse", functools.partial(lambda n, w, name: banded_unsymmetric(n, w, _rng(name)), n, w, name), INVERSE_ENV, 1, forced=1))
    out.append(Case("inverse-lower-321", "inverse", lambda: lower_plus_diagonal(321, _rng("inverse-lower-321")), INVERSE_ENV, 1, forced=1))
    for n in (320, 300):
        name = "inverse-pivot-%d" % n
        out.append(Case(name, "inverse", functools.partial(lambda n, name: block_permutation(n, _rng(name)), n, name), INVERSE_ENV, 1, forced=1))
    return out


GROWTH_SIZES = (320, 700)
GROWTH_EPS = (1.0, 0.9, 0.8, 0.7)
GROWTH_SEEDS = tuple(range(10))
GROWTH_ACCEPT = 1e-9                                     # the absolute threshold dense.hip's check had
GROWTH_WORSE = 30.0


@functools.lru_cache(maxsize=None)
def growth_candidates():
    """[(name, n, eps, seed, model's check, model's error, np.linalg.inv's error)] for every candidate"""
    out = []
    for n in GROWTH_SIZES:
        for eps in GROWTH_EPS:
            for seed in GROWTH_SEEDS:
                name = "growth-%d-eps%.1f-seed%d" % (n, eps, seed)
                A = shifted_growth(n, eps, seed)
                M = A.toarray()
                b = _rng(name).standard_normal(n)
                with np.errstate(all="ignore"):
                    X = block_gauss_jordan(M)
                    check = acceptance_residual(M, X) if np.all(np.isfinite(X)) else np.inf
                if not check <= GROWTH_ACCEPT:
                    out.append((name, n, eps, seed, check, np.inf, 0.0))
                    continue
                ref = refined_solve(A, b)
                out.append((name, n, eps, seed, check, error(X @ b, ref), error(np.linalg.inv(M) @ b, ref)))
    return out


def growth_cases():
    """the candidates the host model accepts although they are at least 30 x worse than np.linalg.inv"""
    return [Case(name, "growth", functools.partial(shifted_growth, n, eps, seed), INVERSE_ENV, 1, forced=1)
            for name, n, eps, seed, check, err, inv_err in growth_candidates() if check <= GROWTH_ACCEPT and err >= GROWTH_WORSE * inv_err]


NULLSPACE_SHAPES = [((12, 14, 14), 294), ((16, 16, 16), 512)]         # C order: the coarsest level 6 x 7 x 7 (x fastest: 7 x 7 x 6) and 8^3


def regularised(Ac):
    n = Ac.shape[0]
    return sp.csr_matrix(Ac.toarray() + gamma_of(Ac) * np.ones((n, n)))


def nullspace_cases():
    """the reference solves (Ac + gamma 1 1^T) x = b: x = pinv(Ac) b + mean(b) / (gamma n)"""
    out = []
    for shape, n in NULLSPACE_SHAPES:
        out.append(Case("nullspace-neumann-%d" % n, "nullspace", functools.partial(lambda shape: regularised(sp.csr_matrix(neumann_lists(shape)[0][-1])), shape),
                        {}, 1, lists=shape))
    return out


def poisson1d(n):
    return sp.csr_matrix(operators.poisson(n))


def substructuring_cases():
    specs = [("sub-1d-300-q2", lambda: poisson1d(300), 2), ("sub-1d-300-q64", lambda: poisson1d(300), 64),
             ("sub-1d-191-q64", lambda: poisson1d(191), 64),                 # every block exactly 2 w = 2 rows
             ("sub-2d-40x40-q2", lambda: operators.stencil_poisson((40, 40)), 2),
             ("sub-2d-40x40-q13", lambda: operators.stencil_poisson((40, 40)), 13),      # the largest the rule admits
             ("sub-band37-1200-q3", lambda: banded_unsymmetric(1200, 37, _rng("sub-band37-1200-q3")), 3)]
    return [Case(name, "substructuring", make, {"OMG_COARSE_BLOCKS": str(q)}, q, forced=q) for name, make, q in specs]


def chain_cases():
    specs = [("chain-3d-12-bs144", lambda: operators.stencil_poisson((12, 12, 12)), 144),       # bs == w
             ("chain-3d-12-bs864", lambda: operators.stencil_poisson((12, 12, 12)), 864),       # K == 2
             ("chain-1d-301-bs100", lambda: poisson1d(301), 100),                               # a last block of one row
             ("chain-1d-40-bs1", lambda: poisson1d(40), 1),
             ("chain-var27-10-bs111", lambda: operators.stencil27_variable((10, 10, 10)), 111)]  # bs == w == 111
    return [Case(name, "chain", make, {"OMG_COARSE_CHAIN": "1", "OMG_COARSE_SINE": "0", "OMG_COARSE_CHAIN_BS": str(bs)}, -1, forced=bs)
            for name, make, bs in specs]


FAMILIES = {"sine": sine_cases, "inverse": inverse_cases, "growth": growth_cases, "nullspace": nullspace_cases,
            "substructuring": substructuring_cases, "chain": chain_cases}


def all_cases():
    return [c for family in FAMILIES.values() for c in family()]


# ---- a case's numbers, computed once ---------------------------------------------------------------------------------
class Numbers:
    pass


@functools.lru_cache(maxsize=None)
def _numbers(name):
    case = {c.name: c for c in all_cases()}[name]
    out = Numbers()
    A = sp.csr_matrix(case.make())
    n = A.shape[0]
    out.A, out.n = A, n
    out.b = _rng(name + "/b").standard_normal(n)
    out.b32 = out.b.astype(np.float32).astype(np.float64)
    S = sp.csr_matrix(A, copy=True)
    S.sum_duplicates()
    lu = spla.splu(sp.csc_matrix(S))
    out.kappa = cond1(S, lu)
    out.ref = refined_solve(S, out.b, lu)
    out.ref32 = refined_solve(S, out.b32, lu)
    if case.yardstick == "dst":
        out.yard = dst_solve(case.extents, case.coefficients, out.b)
        out.yard_b32 = dst_solve(case.extents, case.coefficients, out.b32)       # the fp64 method on the rounded right-hand side
    else:
        assert n <= 2100
    out.yard32 = None
    if n <= 2100:
        inv = np.linalg.inv(S.toarray())
        if case.yardstick == "inverse":
            out.yard, out.yard_b32 = inv @ out.b, None
        out.yard32 = (inv.astype(np.float32) @ out.b.astype(np.float32)).astype(np.float64)
    out.yard_err = error(out.yard, out.ref)
    out.yard_b32_err = None if out.yard_b32 is None else error(out.yard_b32, out.ref32)
    out.yard32_err = None if out.yard32 is None else error(out.yard32, out.ref32)
    for v in (out.b, out.b32, out.ref[0], out.ref[1], out.ref32[0], out.ref32[1]):
        v.setflags(write=False)
    return out


def numbers(case):
    return _numbers(case.name)


def bound64(num):
    """relative to max|x|: FACTOR x max(yardstick error, one unit)"""
    return FACTOR * max(num.yard_err, U64 * num.kappa)


def bound32(num):
    """the fp32 products (inverse, substructuring, chain): FACTOR x max(fp32 yardstick error, 2^-24 kappa_1)"""
    return FACTOR * max(num.yard32_err or 0.0, U32 * num.kappa)          # (no fp32 yardstick above n = 2100: the unit alone)


def sine32_allowance(num):
    """the sine kernels compute in double and round once: componentwise |x32 - x_ref(b32)| <= 2^-24 |x_ref| + the fp64 bound
    (derived, not measured); the fp64 bound: FACTOR x max(the fp64 yardstick's error on b32, one unit) x max|x_ref|"""
    hi = num.ref32[0]
    return U32 * np.abs(hi) + FACTOR * max(num.yard_b32_err, U64 * num.kappa) * np.abs(hi).max()
