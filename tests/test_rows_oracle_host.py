"""The exact restatement of the row kernels (oracle/gs_oracle.c rows_*, oracle/mg_oracle.py rows_*) pinned on the
CPU: against rational arithmetic with a hand-written round-to-nearest-even, against np.int64 on integer data,
on committed rows where the association rule and the fused Jacobi update are observable, and against the older
multiply-then-add oracle within a derived bound.  tests/test_gpu_rows_bits.py then compares the kernels with this
restatement bit for bit.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import rows_cases as rc
from openmg_amd import _hip
from oracle import mg_oracle as orc

BITS = {np.float32: 24, np.float64: 53}
DTYPES = [np.float32, np.float64]
U53 = 2.0 ** -53


# ---------------------------------------------------------------- rational arithmetic, rounded by hand --
def rn(q, p):
    """Fraction q rounded to nearest, ties to even, to a p-bit significand (no overflow / underflow here)."""
    if q == 0:
        return Fraction(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    elif Fraction(2) ** (e + 1) <= q:
        e += 1                                                    # 2^e <= q < 2^(e+1)
    scale = Fraction(2) ** (p - 1 - e)
    m = q * scale                                                 # in [2^(p-1), 2^p)
    f = m.numerator // m.denominator
    rem = m - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (f & 1)):
        f += 1
    return sign * Fraction(f) / scale


def chain_sum(vals, xs, p, chains):
    """`chains` interleaved fma chains from +0 (entry e to chain e % chains), one rounding per fma, added as
    ((s0 + s1) + s2) + s3 with one rounding per addition."""
    s = [Fraction(0)] * chains
    for e, (v, x) in enumerate(zip(vals, xs)):
        s[e % chains] = rn(v * x + s[e % chains], p)
    tot = s[0]
    for q in range(1, chains):
        tot = rn(tot + s[q], p)
    return tot


def chain_diag(vals, on_diag, p, chains):
    s = [Fraction(0)] * chains
    for e, (v, d) in enumerate(zip(vals, on_diag)):
        if d:
            s[e % chains] = rn(s[e % chains] + v, p)
    tot = s[0]
    for q in range(1, chains):
        tot = rn(tot + s[q], p)
    return tot


def tree_sum(parts):
    """256 partials: wave_sum's shuffle tree inside each 64 (lane i adds lane i + off, off = 32 .. 1), the four
    waves in order from +0, every addition rounded to double."""
    tot = Fraction(0)
    for w in range(4):
        v = list(parts[64 * w:64 * w + 64])
        off = 32
        while off:
            for i in range(off):
                v[i] = rn(v[i] + v[i + off], 53)
            off >>= 1
        tot = rn(tot + v[0], 53)
    return tot


def row_by_the_rule(vals, xs, on_diag, p):
    """(sum, diagonal) of one row as common.h ASSOC_LEN and process_block's one-long-row branch state it."""
    k = len(vals)
    if k > rc.ROWBLK_NNZ:
        part, dpart = [], []
        for t in range(256):
            part.append(chain_sum(vals[t::256], xs[t::256], p, 1))
            dpart.append(chain_diag(vals[t::256], on_diag[t::256], p, 1))
        return rn(tree_sum(part), p), rn(tree_sum(dpart), p)
    chains = 4 if k > rc.ASSOC_LEN else 1
    return chain_sum(vals, xs, p, chains), chain_diag(vals, on_diag, p, chains)


def as_fraction(a):
    return [Fraction(float(v)) for v in a]


def test_round_to_nearest_even_helper():
    assert rn(Fraction(1) + Fraction(1, 2 ** 24), 24) == 1                       # tie -> even
    assert rn(Fraction(1) + Fraction(3, 2 ** 24), 24) == 1 + Fraction(4, 2 ** 24)  # tie -> even (up)
    assert rn(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60), 24) == 1 + Fraction(2, 2 ** 24)
    assert rn(-Fraction(7, 3), 53) == Fraction(float(-7.0 / 3.0))
    rng = np.random.default_rng(5)
    for a, b in rng.standard_normal((50, 2)):
        assert rn(Fraction(a) + Fraction(b), 53) == Fraction(float(a + b))
        assert rn(Fraction(a) * Fraction(b), 53) == Fraction(float(a * b))


# ---------------------------------------------------------------------------- exact rounding --
def _rounding_rows():
    """200 rows of 1..40 stored entries and one each of 2049 and 2600, columns with replacement (duplicates, stored
    diagonal entries among them), float32-representable normals."""
    rng = np.random.default_rng(20240)
    lengths = np.concatenate([np.arange(1, 41), rng.integers(1, 41, size=160), [2049, 2600]])
    n = lengths.size
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    for i in range(n):                                            # stored diagonal entries: about every fourth entry of a row
        seg = indices[indptr[i]:indptr[i + 1]]
        seg[rng.random(seg.size) < 0.25] = i
    data = rng.standard_normal(indices.size).astype(np.float32).astype(np.float64)
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    A.has_sorted_indices = False
    x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return A, x


@pytest.mark.parametrize("dtype", DTYPES)
def test_restatement_rounds_once_per_fma_and_add_in_the_stated_association(dtype):
    """Every row sum and diagonal equals the rational computation rounded once per fma and once per add in the
    association of common.h ASSOC_LEN (and, beyond 2048 entries, of the workgroup path): the rule as coded, and
    the platform's fmaf / fma rounding once."""
    A, x = _rounding_rows()
    p = BITS[dtype]
    got_s, got_d = orc.rows_sum(A, x, dtype)
    assert np.diff(A.indptr).max() == 2600 and A.shape[0] >= 202
    xf = as_fraction(x)
    for i in range(A.shape[0]):
        s, e = A.indptr[i], A.indptr[i + 1]
        cols = A.indices[s:e]
        want_s, want_d = row_by_the_rule(as_fraction(A.data[s:e]), [xf[c] for c in cols], list(cols == i), p)
        assert Fraction(float(got_s[i])) == want_s, (i, e - s)
        assert Fraction(float(got_d[i])) == want_d, (i, e - s)
    # the entry points are that sum with their epilogue: one more rounding each
    b = np.random.default_rng(3).standard_normal(A.shape[0]).astype(np.float32).astype(np.float64)
    assert np.array_equal(orc.rows_spmv(A, x, dtype), got_s)
    assert np.array_equal(orc.rows_residual(A, b, x, dtype), (b.astype(dtype) - got_s.astype(dtype)).astype(np.float64))
    assert np.array_equal(orc.rows_axpy(A, x, b, dtype), (b.astype(dtype) + got_s.astype(dtype)).astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_relaxations_are_the_row_sum_with_the_stated_epilogue(dtype):
    """gs_ordered: x_i + (b_i - sum) / diag with the NEW values of the rows already visited; jacobi:
    fma(omega, (b_i - sum) / diag, x_i) with omega rounded to the element type — each operation rounded once."""
    fam = rc.FAMILIES["block257"]
    A = rc.real_operator(fam)
    v = rc.real_vectors(fam, {})
    p, n = BITS[dtype], fam.n
    order = np.random.default_rng(8).permutation(n).astype(np.int32)
    got = orc.rows_gs_ordered(A, v["b"], v["x"], order, 1, dtype)
    x = v["x"].copy()
    for i in order[:40]:                                          # the first rows of the sweep, by hand
        s, d = orc.rows_sum(A, x, dtype)
        r = rn(Fraction(float(v["b"][i])) - Fraction(float(s[i])), p)
        x[i] = float(rn(Fraction(float(x[i])) + rn(r / Fraction(float(d[i])), p), p))
        assert x[i] == got[i]
    om = Fraction(float(dtype(0.7)))
    assert om != Fraction(0.7) or dtype is np.float64
    got = orc.rows_jacobi(A, v["b"], v["x"], 1, 0.7, dtype)
    s, d = orc.rows_sum(A, v["x"], dtype)
    for i in range(0, n, 5):
        q = rn(rn(Fraction(float(v["b"][i])) - Fraction(float(s[i])), p) / Fraction(float(d[i])), p)
        assert Fraction(float(got[i])) == rn(om * q + Fraction(float(v["x"][i])), p)
    two = orc.rows_jacobi(A, v["b"], v["x"], 2, 0.7, dtype)
    assert np.array_equal(two, orc.rows_jacobi(A, v["b"], got, 1, 0.7, dtype))


# ---------------------------------------------------------------------------------- integers --
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(rc.FAMILIES))
def test_integer_data_equals_int64_arithmetic(name, dtype):
    fam = rc.FAMILIES[name]
    A = rc.integer_operator(fam)
    Rs = {k: rc.restriction(fam, k, True) for k in rc.RESTRICTIONS}
    v = rc.integer_vectors(fam, {k: R.shape[0] for k, R in Rs.items()})
    Ai = sp.csr_matrix((A.data.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    x, b = v["x"].astype(np.int64), v["b"].astype(np.int64)
    rows = np.repeat(np.arange(fam.n), fam.lengths)
    want = np.zeros(fam.n, dtype=np.int64)
    np.add.at(want, rows, Ai.data * x[Ai.indices])
    wdiag = np.zeros(fam.n, dtype=np.int64)
    np.add.at(wdiag, rows, np.where(Ai.indices == rows, Ai.data, 0))
    assert np.abs(Ai.data * x[Ai.indices]).max() * fam.lengths.max() < 2 ** 24
    s, d = orc.rows_sum(A, v["x"], dtype)
    assert np.array_equal(s, want) and np.array_equal(d, wdiag) and np.all(wdiag != 0)
    assert np.array_equal(orc.rows_spmv(A, v["x"], dtype), want)
    assert np.array_equal(orc.rows_residual(A, v["b"], v["x"], dtype), b - want)
    assert np.array_equal(orc.rows_axpy(A, v["x"], v["b"], dtype), b + want)
    for k, R in Rs.items():
        Ri = sp.csr_matrix((R.data.astype(np.int64), R.indices, R.indptr), shape=R.shape)
        fine, coarse = v["fine"].astype(np.int64), v["coarse"][k].astype(np.int64)
        assert np.array_equal(orc.rows_spmv(R, v["fine"], dtype), Ri @ fine)
        assert np.array_equal(orc.rows_axpy(rc.transpose_stored(R), v["coarse"][k], v["fine"], dtype), fine + Ri.T @ coarse)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_relaxations_equal_rational_arithmetic(dtype):
    """Diagonal 2 and omega 0.5 make every division and product exact: the iterates are multiples of 1/2 (Gauss-Seidel)
    and 1/4 (Jacobi), compared with exact rational arithmetic."""
    rng = np.random.default_rng(77)
    n = 12
    M = rng.integers(-2, 3, size=(n, n))
    np.fill_diagonal(M, 2)
    A = sp.csr_matrix(M.astype(np.float64))
    b, x0 = rng.integers(-9, 10, size=n), rng.integers(-9, 10, size=n)
    order = rng.permutation(n).astype(np.int32)
    xs = [Fraction(int(v)) for v in x0]
    for i in order:
        xs[i] = xs[i] + (int(b[i]) - sum(int(M[i, j]) * xs[j] for j in range(n))) / 2
    got = orc.rows_gs_ordered(A, b, x0, order, 1, dtype)
    assert max(abs(v) for v in xs) * 2 ** 12 < 2 ** 24 and [Fraction(float(g)) for g in got] == xs
    wantj = [Fraction(int(x0[i])) + Fraction(1, 2) * Fraction(int(b[i]) - sum(int(M[i, j]) * int(x0[j]) for j in range(n)), 2)
             for i in range(n)]
    assert [Fraction(float(g)) for g in orc.rows_jacobi(A, b, x0, 1, 0.5, dtype)] == wantj


# ----------------------------------------------------------------------- the rule is observable --
def test_the_association_rule_is_observable_on_a_committed_row():
    v, x = rc.from_hex(rc.ROW17_V), rc.from_hex(rc.ROW17_X)
    assert np.array_equal(v, v.astype(np.float32)) and np.array_equal(x, x.astype(np.float32))
    four, one = float.fromhex(rc.ROW17_FOUR), float.fromhex(rc.ROW17_ONE)
    p_one, p_four = float.fromhex(rc.PREFIX16_ONE), float.fromhex(rc.PREFIX16_FOUR)
    assert four != one and p_one != p_four
    # the committed numbers are what the rational model gives for the two associations
    assert chain_sum(as_fraction(v), as_fraction(x), 24, 4) == Fraction(four)
    assert chain_sum(as_fraction(v), as_fraction(x), 24, 1) == Fraction(one)
    assert chain_sum(as_fraction(v[:16]), as_fraction(x[:16]), 24, 1) == Fraction(p_one)
    assert chain_sum(as_fraction(v[:16]), as_fraction(x[:16]), 24, 4) == Fraction(p_four)
    # the restatement: four chains for the 17 entries, one chain for their first 16
    cols = np.arange(17, dtype=np.int32)
    row = sp.csr_matrix((v, cols, np.array([0, 17], dtype=np.int32)), shape=(1, 17))
    assert orc.rows_spmv(row, x, np.float32)[0] == four
    prefix = sp.csr_matrix((v[:16], cols[:16], np.array([0, 16], dtype=np.int32)), shape=(1, 17))
    assert orc.rows_spmv(prefix, x, np.float32)[0] == p_one


def test_the_fused_jacobi_update_is_observable_on_a_committed_system():
    a, b, x = (float.fromhex(h) for h in (rc.JAC_A, rc.JAC_B, rc.JAC_X))
    fused, unfused = float.fromhex(rc.JAC_FUSED), float.fromhex(rc.JAC_UNFUSED)
    assert fused != unfused and all(np.float32(t) == t for t in (a, b, x))
    om = Fraction(float(np.float32(0.7)))
    q = rn(rn(Fraction(b) - rn(Fraction(a) * Fraction(x), 24), 24) / Fraction(a), 24)
    assert rn(om * q + Fraction(x), 24) == Fraction(fused)
    assert rn(rn(om * q, 24) + Fraction(x), 24) == Fraction(unfused)
    A = sp.csr_matrix(np.array([[a]]))
    assert orc.rows_jacobi(A, [b], [x], 1, 0.7, np.float32)[0] == fused


# ------------------------------------------------------------------- agreement with the older oracle --
def _double_problem(fam):
    """The family's structure with full double-precision normals (a product of two float32-representable numbers is
    exact in double, and the two oracles would agree to the bit on such data): operator with the designated diagonal
    +-(1 + the row's absolute sum), x and b."""
    rng = np.random.default_rng([fam.n, fam.nnz, 99])
    data = rng.standard_normal(fam.nnz)
    rows = np.repeat(np.arange(fam.n), fam.lengths)
    data[fam.diag_pos] = 0.0
    data[fam.diag_pos] = rng.choice([-1.0, 1.0], size=fam.n) * (1.0 + np.bincount(rows, weights=np.abs(data), minlength=fam.n))
    A = sp.csr_matrix((data, fam.indices.copy(), fam.indptr.copy()), shape=(fam.n, fam.n))
    A.has_sorted_indices = False
    return A, rng.standard_normal(fam.n), rng.standard_normal(fam.n)


def _abs_row_sums(A, x):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.bincount(rows, weights=np.abs(A.data) * np.abs(x)[A.indices], minlength=A.shape[0])


@pytest.mark.parametrize("name", ["block600", "mixed", "long", "short17", "huge300"])
def test_double_restatement_agrees_with_the_multiply_then_add_oracle_spmv(name):
    """oracle_spmv rounds every product and every addition, the restatement once per fma (and groups long rows
    differently); on a row of k stored entries the two differ by at most (k + 1) 2^-53 sum_j |a_ij| |x_j|."""
    fam = rc.FAMILIES[name]
    A, x, _ = _double_problem(fam)
    old = np.empty(fam.n)
    orc._clib().oracle_spmv(fam.n, *orc._csr(A), x, old)
    new = orc.rows_spmv(A, x, np.float64)
    bound = (fam.lengths + 1) * U53 * _abs_row_sums(A, x)
    assert np.all(np.abs(new - old) <= bound), float(np.max(np.abs(new - old) / bound))
    assert np.any(new != old)                                      # the two roundings are really different ones


@pytest.mark.parametrize("name,order", [("mixed", "lex"), ("long", "colour"), ("block600", "colour"), ("wave65", "lex")])
def test_double_restatement_agrees_with_the_multiply_then_add_oracle_sweeps(name, order):
    """Three sweeps of oracle_gs_ordered against rows_gs_ordered in double.  With u = 2^-53, E_j a bound on the
    difference of the two iterates' entry j (0 at the start), k_i the stored entries of row i, m_i its stored
    diagonal entries, S_i = sum_j |a_ij| (|x_j| + E_j) (|x_j|: the largest value entry j takes in either run) and d_i the diagonal, a visit of row i changes E_i to

        E_i + [ (k_i + 1) u S_i + sum_j |a_ij| E_j ] / |d_i|              the row sums: arithmetic, and the iterates' difference
            + 2 [ (m_i + 3) u (|b_i| + S_i) / |d_i| + u (|x_i| + E_i) ]    both sides: the diagonal's m_i - 1 additions, b - s,
                                                                          the division (<= m_i + 2 roundings on the quotient),
                                                                          and the final addition (one rounding on the result,
                                                                          <= |x_i| + the quotient, the quotient's share counted
                                                                          in m_i + 3)

    to first order in u; the accumulated E is multiplied by 1.01 for the higher orders."""
    fam = rc.FAMILIES[name]
    A, x0, b = _double_problem(fam)
    v = {"x": x0, "b": b}
    n = fam.n
    perm = np.arange(n, dtype=np.int32) if order == "lex" else orc.colour_order(orc.greedy_colouring(A))
    olds = [orc.gs_ordered(A, v["b"], v["x"].copy(), perm, k) for k in range(4)]
    news = [orc.rows_gs_ordered(A, v["b"], v["x"], perm, k, np.float64) for k in range(4)]
    # an entry changes once per sweep, so at any moment it holds one of these values: |x_j| of the recurrence
    absx = np.max(np.abs(np.array(olds + news)), axis=0)
    old = olds[3]
    E = np.zeros(n)
    absA = np.abs(A.data)
    diag = orc.rows_sum(A, v["x"], np.float64)[1]
    rows = np.repeat(np.arange(n), fam.lengths)
    m = np.bincount(rows[A.indices == rows], minlength=n)
    for sweep in range(3):
        for i in perm:
            s, e = A.indptr[i], A.indptr[i + 1]
            cols = A.indices[s:e]
            S = float(np.sum(absA[s:e] * (absx[cols] + E[cols])))
            prop = float(np.sum(absA[s:e] * E[cols]))
            d = abs(diag[i])
            E[i] = (E[i] + ((e - s + 1) * U53 * S + prop) / d
                    + 2 * ((m[i] + 3) * U53 * (abs(v["b"][i]) + S) / d + U53 * (absx[i] + E[i])))
    new = orc.rows_gs_ordered(A, v["b"], v["x"], perm, 3, np.float64)
    assert np.all(np.abs(new - old) <= 1.01 * E), float(np.max(np.abs(new - old) / E))
    assert np.max(E) < 1e-10                                       # the bound says something


# --------------------------------------------------------------- the families reach their variants --
def test_families_have_the_row_statistics_their_variants_need():
    """encode_csr's rule (rows_cases' docstring) applied to every family, and the properties the GPU tests lean on."""
    F = rc.FAMILIES
    for name in ("long", "huge300"):
        assert F[name].expected_lanes() == 4, name                   # average row above 16: four lanes per row
    for name in ("mixed", "huge1200", "block255", "block256", "block257", "block600", "short17", "band_const2304"):
        assert F[name].expected_lanes() == 1, name
    for name in ("short1to2", "short1to4", "unit", "short_one19"):
        assert F[name].expected_short(), name                        # widened row blocks: the SHORT variant
    assert set(F["long"].lengths) == {17, 18, 19, 20, 31, 32, 33, 40, 64, 65}
    assert set(F["unit"].lengths) == {1}
    assert sorted(set(F["short_one19"].lengths)) == [1, 2, 19] and np.sum(F["short_one19"].lengths == 19) == 1
    assert F["mixed"].lengths.max() > rc.ASSOC_LEN and 0.02 < np.mean(F["mixed"].lengths > rc.ASSOC_LEN) < 0.1
    for name in ("block255", "block256", "block257", "block600"):   # 256 rows hold more than a block's 2048 entries
        assert F[name].nnz / F[name].n * 256 > rc.ROWBLK_NNZ
    for name in ("huge300", "huge1200"):
        fam = F[name]
        rows = np.repeat(np.arange(fam.n), fam.lengths)
        ndiag = np.bincount(rows[fam.indices == rows], minlength=fam.n)
        big = np.flatnonzero(fam.lengths > rc.ROWBLK_NNZ)
        assert sorted(fam.lengths[big]) == [2049, 5000] and np.all(ndiag[big] >= 4)
    for name, fam in F.items():
        A, Ai = rc.real_operator(fam), rc.integer_operator(fam)
        rows = np.repeat(np.arange(fam.n), fam.lengths)
        on = fam.indices == rows
        d = np.bincount(rows[on], weights=A.data[on], minlength=fam.n)
        off = np.bincount(rows[~on], weights=np.abs(A.data[~on]), minlength=fam.n)
        assert np.all(np.abs(d) > off), name                         # strictly dominant, duplicates of the diagonal included
        assert np.array_equal(A.data, A.data.astype(np.float32)) and np.all(np.abs(A.data[A.data != 0]) > 1e-30), name
        assert np.all(np.bincount(rows[on], weights=Ai.data[on], minlength=fam.n) != 0), name
        assert np.abs(Ai.data).max() <= 8 and np.array_equal(Ai.data, np.round(Ai.data)), name
        assert orc.greedy_colouring(A).max() < 64, name              # the library's colouring stops at 64 colours
        for kind in rc.RESTRICTIONS:
            R = rc.restriction(fam, kind, False)
            per_col = np.bincount(R.indices, minlength=fam.n)
            if kind == "pair":
                assert np.all(per_col == 1)
            elif kind == "irregular":
                assert per_col.max() == 1 and np.diff(R.indptr).max() <= 7
                if fam.n >= 5:
                    assert per_col.min() == 0 and np.diff(R.indptr).min() == 0      # empty rows in R^T and in R
            elif kind in ("strided", "strided_var"):
                assert per_col.max() == 1 and (fam.n < 8 or (np.all(np.diff(R.indptr) == 8) and per_col[:8 * R.shape[0]].min() == 1))
            elif R.shape[0] >= 3:
                assert per_col.min() >= 2 and per_col.max() <= 3


def test_stencil_like_families_take_the_pattern_union_and_ell_codings(monkeypatch):
    """omg_format_selftest (host only): constant values per offset give row patterns in wide union blocks of
    OMG_UNION_ROWS x 256 rows where the operator has at least four of them, per-entry values give offset patterns with
    ELL values; OMG_COMPRESS=0 keeps plain CSR."""
    for dtype in ("float64", "float32"):
        for n in (2304, 4352):
            const, var = rc.real_operator(rc.FAMILIES["band_const%d" % n]), rc.real_operator(rc.FAMILIES["band_var%d" % n])
            for u in ("1", "2", "4"):
                monkeypatch.setenv("OMG_UNION_ROWS", u)
                f = _hip.format_selftest(const, dtype)
                assert f["pattern_rows"] == n and f["ell_blocks"] == 0
                if int(u) > 1 and n >= 4 * int(u) * 256:
                    assert f["blocks"] == -(-n // (256 * int(u))), (n, u)
                else:
                    assert f["blocks"] >= -(-n // 256), (n, u)
            monkeypatch.delenv("OMG_UNION_ROWS")
            f = _hip.format_selftest(var, dtype)
            assert f["pattern_rows"] == n and f["ell_blocks"] == f["blocks"] and f["ell_nnz"] == f["nnz"]
            monkeypatch.setenv("OMG_COMPRESS", "0")
            for M in (const, var):
                f = _hip.format_selftest(M, dtype)
                assert f["pattern_rows"] == 0 and f["coldict_nnz"] == 0 and f["valdict_nnz"] == 0 and f["ell_blocks"] == 0
            monkeypatch.delenv("OMG_COMPRESS")


def test_strided_restrictions_are_row_pattern_coded_where_the_scatter_is_expected(monkeypatch):
    """rows_cases.scatter_expected() against omg_format_selftest (host only): the prolongation runs as a scatter over R's
    rows exactly when every row of R is pattern coded; the pair, irregular and overlapping restrictions never are."""
    for name, fam in rc.FAMILIES.items():
        for kind in rc.RESTRICTIONS:
            for integers in (True, False):
                R = rc.restriction(fam, kind, integers)
                for compress, pk in (("15", None), ("15", "0"), ("7", None), ("0", None)):
                    monkeypatch.setenv("OMG_COMPRESS", compress)
                    if pk is None:
                        monkeypatch.delenv("OMG_PATTERN_KERNEL", raising=False)
                    else:
                        monkeypatch.setenv("OMG_PATTERN_KERNEL", pk)
                    for dtype in ("float64", "float32"):
                        f = _hip.format_selftest(R, dtype)
                        coded = f["rows"] > 0 and f["pattern_rows"] == f["rows"]
                        assert coded == rc.scatter_expected(fam, kind, compress, pk), (name, kind, integers, compress, pk, dtype)
                        if kind == "strided_var" and coded:
                            assert f["ell_blocks"] == f["blocks"]
                        if kind == "strided" and coded:
                            assert f["ell_blocks"] == 0
