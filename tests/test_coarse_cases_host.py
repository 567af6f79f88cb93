"""tests/coarse_cases.py on its own (no GPU): the reference against exact and 200-bit arithmetic, every yardstick inside its
own bound on every case, the growth family's cap, and every forced q, bs and shape against the library's admission rules
(restated from csrc/coarse.hip)."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as cc

CASES = cc.all_cases()


def exact_solve(A, b):
    """Gauss-Jordan in rational arithmetic"""
    n = len(b)
    W = [[Fraction(float(A[i, j])) for j in range(n)] + [Fraction(float(b[i]))] for i in range(n)]
    for k in range(n):
        p = next(i for i in range(k, n) if W[i][k] != 0)
        W[k], W[p] = W[p], W[k]
        W[k] = [v / W[k][k] for v in W[k]]
        for i in range(n):
            if i != k and W[i][k] != 0:
                W[i] = [v - W[i][k] * wk for v, wk in zip(W[i], W[k])]
    return [W[i][n] for i in range(n)]


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (5, 2), (12, 3), (12, 4)])
def test_refined_solve_equals_the_exact_solution_rounded(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) + (0.0 if seed == 4 else 3.0) * np.eye(n)        # (seed 4: not dominant, kappa in the hundreds)
    b = rng.standard_normal(n)
    hi, lo = cc.refined_solve(sp.csr_matrix(A), b)
    x = exact_solve(A, b)
    assert [float(v) for v in x] == list(hi)                                          # hi: the exact solution, rounded once
    big = max(abs(v) for v in x)
    assert max(abs(Fraction(float(h)) + Fraction(float(l)) - v) for h, l, v in zip(hi, lo, x)) <= Fraction(1, 2 ** 60) * big


def test_refined_solve_against_mpmath_at_200_bits():
    mpmath = pytest.importorskip("mpmath")
    rng = np.random.default_rng(11)
    n = 60
    A = cc.banded_unsymmetric(n, 7, rng)
    b = rng.standard_normal(n)
    hi, lo = cc.refined_solve(A, b)
    with mpmath.workprec(200):
        x = mpmath.lu_solve(mpmath.matrix(A.toarray().tolist()), mpmath.matrix(b.tolist()))
        big = max(abs(v) for v in x)
        worst = max(abs(mpmath.mpf(float(h)) + mpmath.mpf(float(l)) - v) for h, l, v in zip(hi, lo, x))
        assert worst <= big * mpmath.mpf(2) ** -60, float(worst / big)


def test_residual_is_exact_where_double_rounds():
    """b - A x with a cancellation no 64-bit mantissa survives: (1 + 2^-52) (1 - 2^-52) - 1 = -2^-104"""
    A = sp.csr_matrix(np.array([[1.0 + 2.0 ** -52]]))
    r = cc._residual(A, np.array([1.0]), np.array([1.0 - 2.0 ** -52]), np.array([0.0]))
    assert r[0] == 2.0 ** -104


def test_cond1_against_the_dense_one_norm():
    for name in ("inverse-dense-65", "sine-poisson-5x7x6", "sub-1d-191-q64", "growth-320"):
        case = next(c for c in CASES if c.name.startswith(name))
        M = cc.numbers(case).A.toarray()
        want = np.abs(M).sum(axis=0).max() * np.abs(np.linalg.inv(M)).sum(axis=0).max()
        assert 0.9 * want <= cc.numbers(case).kappa <= (1.0 + 1e-12) * want             # (an estimate from below: the unit can only come out tighter)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_yardstick_is_inside_its_own_bound(case):
    """the reference alone passes: each yardstick within FACTOR units of the refined solution"""
    num = cc.numbers(case)
    assert num.yard_err <= cc.FACTOR * cc.U64 * num.kappa
    assert num.yard_err <= cc.bound64(num)
    if num.yard_b32_err is not None:
        assert num.yard_b32_err <= cc.FACTOR * cc.U64 * num.kappa
        assert np.all(np.abs(num.yard_b32 - num.ref32[0]) <= cc.sine32_allowance(num))
    if num.yard32_err is not None:
        assert num.yard32_err <= cc.FACTOR * cc.U32 * num.kappa
        assert num.yard32_err <= cc.bound32(num)


def test_dst_yardstick_solves_the_star_stencils():
    """dst_solve is told extents and couplings, not the matrix: its answer must solve the assembled operator"""
    for case in cc.sine_cases():
        num = cc.numbers(case)
        r = num.b - num.A @ num.yard
        assert np.abs(r).max() <= 64 * cc.U64 * np.abs(num.A).sum(axis=1).max() * np.abs(num.yard).max(), case.name


def test_growth_family_cap():
    """at least four candidates are accepted by the host model of the blocked inverse (check <= 1e-9, the threshold the
    library had) although they are 30 x worse than np.linalg.inv — the family cannot silently become empty"""
    cases = cc.growth_cases()
    assert len(cases) >= 4
    rows = {name: (check, err, inv_err) for name, n, eps, seed, check, err, inv_err in cc.growth_candidates()}
    assert len(rows) == len(cc.GROWTH_SIZES) * len(cc.GROWTH_EPS) * len(cc.GROWTH_SEEDS)
    for c in cases:
        check, err, inv_err = rows[c.name]
        assert check <= cc.GROWTH_ACCEPT and err >= cc.GROWTH_WORSE * inv_err


def test_host_model_inverts_what_needs_no_pivoting_across_blocks():
    for name in ("inverse-dense-321", "inverse-band70-257", "inverse-pivot-300", "inverse-pivot-320"):
        M = cc.numbers(next(c for c in CASES if c.name == name)).A.toarray()
        X = cc.block_gauss_jordan(M)
        assert np.abs(X @ M - np.eye(M.shape[0])).max() <= 1e-13
        assert cc.acceptance_residual(M, X) <= 1e-13


def test_in_block_pivoting_cases_have_no_diagonal_and_sound_blocks():
    for case in cc.inverse_cases():
        if "pivot" in case.name:
            M = cc.numbers(case).A.toarray()
            assert not np.any(np.diag(M))
            for k0 in range(0, M.shape[0], 64):
                assert np.linalg.cond(M[k0:k0 + 64, k0:k0 + 64]) < 10.0


def test_forced_paths_are_admitted_by_the_library_rule():
    """a q the rule refuses leaves P = 1 silently, a bs below the half-bandwidth is ignored: every forced value is one the
    rule takes, in both precisions"""
    for case in CASES:
        num = cc.numbers(case)
        w = cc.half_bandwidth(num.A)
        if case.family == "substructuring":
            for itemsize in (8, 4):
                assert cc.admitted_blocks(num.n, w, case.forced, itemsize) == case.forced == case.blocks, case.name
        elif case.family == "chain":
            bs, K = cc.chain_blocks(num.n, w, case.forced)
            assert num.n >= 4 and bs == case.forced and K == -(-num.n // bs), case.name
        elif case.family in ("inverse", "growth"):
            assert cc.admitted_blocks(num.n, w, 1) == 1 and num.n <= 16384
    byname = {c.name: cc.numbers(c) for c in CASES}
    assert cc.admitted_blocks(1600, 40, 14) == 1 and cc.admitted_blocks(1600, 40, 13) == 13         # 13: the largest on 40 x 40
    assert cc.chain_blocks(1728, 144, 864)[1] == 2
    assert cc.chain_blocks(301, 1, 100) == (100, 4) and 301 - 3 * 100 == 1                           # a last block of one row
    assert cc.half_bandwidth(byname["chain-var27-10-bs111"].A) == 111 and cc.half_bandwidth(byname["chain-3d-12-bs144"].A) == 144
    n191 = byname["sub-1d-191-q64"].n
    assert (n191 - 63) // 64 == 2 and (n191 - 63) % 64 == 0                                           # every block exactly 2 w = 2 rows


def test_sine_shapes_sit_where_they_are_meant_to():
    for case in cc.sine_cases():
        ext, n = case.extents, int(np.prod(case.extents))
        if case.blocks == 0:
            assert cc.sine_admitted(ext), case.name
            assert (cc.sine_lds_bytes(ext) > 64 * 1024) == (ext in cc.SINE_ABOVE_64K), (case.name, cc.sine_lds_bytes(ext))
            assert cc.sine_lds_bytes(ext) <= 160 * 1024
        else:
            assert not cc.sine_admitted(ext), case.name
            w = ext[0] * (ext[1] if len(ext) > 2 else 1)
            for itemsize in (8, 4):
                assert cc.admitted_blocks(n, w, 0, itemsize) == 1 and n <= 16384, case.name           # the explicit inverse still takes it
    strides = {ext: cc.sine_stride(ext) for ext in cc.SINE_SHAPES}
    assert strides[(16, 16, 16)] == 16 and strides[(16, 16, 15)] == 16 and strides[(16, 15, 17)] == 32 and strides[(32, 2)] == 32
    assert int(np.prod((31, 16, 16))) > 7168 and int(np.prod((32, 32, 8))) == 8192 == int(np.prod((8, 32, 32)))
    assert 32 * 32 > 256                                                                             # 8 x 32 x 32: 1024 lines along x
    assert {len(e) for e in cc.SINE_SHAPES} == {1, 2, 3}


def test_nullspace_reference_is_the_pseudo_inverse_plus_the_constant():
    for case in cc.nullspace_cases():
        num = cc.numbers(case)
        Ac = sp.csr_matrix(cc.neumann_lists(case.lists)[0][-1])
        n = Ac.shape[0]
        assert n == num.n and n >= 256
        x = num.ref[0]
        mean = x.sum() / n
        want = np.linalg.pinv(Ac.toarray()) @ num.b
        assert np.abs((x - mean) - want).max() <= 1e-11 * np.abs(x).max()
        assert abs(mean - (num.b.sum() / n) / (cc.gamma_of(Ac) * n)) <= 1e-12 * np.abs(x).max()
