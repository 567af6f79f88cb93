"""The yardstick of tests/test_gpu_scaling.py, pinned without a GPU: the CPU oracle's own cycles are bitwise equivariant
under power-of-two rescaling — cycle(2^ka A, 2^kb b) has the bits of 2^(kb - ka) cycle(A, b) and 2^kb times its norms —
for every (operator family, smoother, scale pair) the GPU module uses and the oracle can run: 'colour', 'gs' and
'jacobi' V-cycles with the SuperLU coarse solve, and the regularised coarse solve of a constant-null-space hierarchy.
A pair for which the reference alone is not bitwise may not be asked of the device (scaling_cases.py holds the pairs for
both modules).  Also: SuperLU itself on the coarse-solver operator, and Solver's stop rule is homogeneous in ||b||."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from openmg_amd import _solver, operators
from oracle import mg_oracle as orc

import scaling_cases as sc

# (family, shape, grids, smoother): the GPU module's shapes, or smaller where the sequential oracle would be slow
ORACLE_CASES = [
    ("poisson", (16, 16, 16), 3, "colour"),
    ("poisson", (16, 24, 20), 3, "colour"),
    ("poisson", (64, 64), 3, "colour"),
    ("poisson", (64, 64), 3, "jacobi"),
    ("reference", (16, 16, 16), 3, "colour"),
    ("poisson", (16, 16, 16), 2, "gs"),
    ("rows", (16, 16, 16), 2, "gs"),
    ("line", (4096,), 2, "gs"),
    ("var7", (16, 20, 36), 2, "colour"),
    ("s27", (8, 12, 20), 2, "colour"),
    ("irregular", None, 2, "colour"),
    ("neumann", (8, 8, 8), 2, "colour"),
]


def oracle_cycles(name, A, Rs, b, x0, smoother):
    sm = orc.make_smoother(smoother, A, 2.0 / 3.0)
    out = []
    if name == "neumann":
        b = b - math.fsum(b) / b.size
    for pre, post in sc.SWEEPS:
        p = {"coarsestLevel": len(Rs), "preIterations": pre, "postIterations": post}
        for start in (x0, None):
            x, norms = None if start is None else start.copy(), []
            for _ in range(sc.CYCLES):
                x, info = orc.mg_cycle(A, b, 0, Rs, p, initial=x, smoother=sm)
                norms.append(info["norm"])
            out += [("norms", np.array(norms)), ("x", x)]
    return out


@pytest.mark.parametrize("name,shape,grids,smoother", ORACLE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_oracle_is_bitwise_equivariant(monkeypatch, name, shape, grids, smoother):
    if name == "neumann":
        monkeypatch.setattr(orc, "coarse_solve", sc.regularised_solve)
    A0, Rs, b, x0 = sc.family(name, shape, grids)
    base = oracle_cycles(name, sc.galerkin(A0, Rs), Rs, b, x0, smoother)
    assert all(np.all(np.isfinite(v)) for _, v in base)
    cases = [(p, 1) for p in sc.pairs64(sc.diagonal_of(name, shape, grids))] + [((0, 0), -1)] + [(p, 1) for p in sc.PAIRS32]
    for pair, sign in cases:
        s, t, f = sc.factors(pair, sign)
        got = oracle_cycles(name, sc.galerkin(sc.scaled(A0, s), Rs), Rs, t * b, f * x0, smoother)
        sc.assert_equivariant(base, got, pair, sign, (name, shape, smoother))


def test_superlu_is_bitwise_equivariant_on_the_coarse_solver_case():
    A = sp.csc_matrix(operators.stencil_poisson((12, 12, 12)))
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    x = spla.spsolve(A, b)
    for pair, sign in [(p, 1) for p in sc.pairs64(6.0)] + [((0, 0), -1)]:
        s, t, f = sc.factors(pair, sign)
        assert sc.same_bits(spla.spsolve(sp.csc_matrix(sc.scaled(A, s)), t * b), x * f), (pair, sign)


def test_edge_exponents_of_the_poisson_diagonal():
    """6 = 1.5 * 2^2: 6 * 2^397 = 1.5 * 2^399 is inside 2^400 and 6 * 2^398 is not; 6 * 2^-402 = 1.5 * 2^-400 is
    inside 2^-400 and 6 * 2^-403 is not (plane.hip fast_div: 0x1p-400 <= |c3| <= 0x1p400)."""
    assert sc.edge_exponents(6.0) == (397, 398, -402, -403)
    assert sc.edge_exponents(-6.0) == (397, 398, -402, -403)
    assert sc.edge_exponents(4.0) == (398, 399, -402, -403)
    assert sc.edge_exponents(2.5) == (398, 399, -401, -402)


def test_stop_target_is_homogeneous_in_the_rhs_norm():
    for cycles, threshold, rtol, rhs in ((0, 0.0, 1e-8, 3.7), (5, 1e-3, 1e-8, 3.7), (0, 0.25, 0.0, 11.0), (0, 1e-9, 1e-8, 0.3)):
        want = _solver.stop_target(cycles, threshold, rtol, rhs)
        for k in (-420, -110, -1, 1, 130, 420):
            f = math.ldexp(1.0, k)
            assert _solver.stop_target(cycles, threshold * f, rtol, rhs * f) == want * f, (cycles, threshold, rtol, rhs, k)
    assert _solver.stop_target(3, 0.0, 0.0, 5.0) == 0.0


def test_the_reference_adds_the_quotient_so_a_negative_zero_numerator_leaves_plus_zero():
    """openmg/solvers.py:68  x[i] = x[i] + (b[i] - A_i x) / A[i, i]: from a zero start and b[i] = -0.0 among zeros the
    quotient is -0.0 / c3 = -0.0 and x[i] = +0.0 + -0.0 = +0.0; from x[i] = -0.0 it stays -0.0.  What
    tests/test_gpu_scaling.py asks of the device for this input."""
    A = sp.csr_matrix(operators.stencil_poisson((8, 8, 8)))
    order = orc.colour_order(orc.parity_colouring((8, 8, 8)))
    n = A.shape[0]
    b = np.zeros(n)
    b[77] = -0.0
    x = orc.gs_ordered(A, b, np.zeros(n), order, 1)
    assert sc.same_bits(x, np.zeros(n))
    start = np.zeros(n)
    start[77] = -0.0
    x = orc.gs_ordered(A, b, start.copy(), order, 1)
    assert sc.same_bits(x, start)
    x = orc.gauss_seidel(A, b, np.zeros(n), iterations=1)
    assert sc.same_bits(x, np.zeros(n))
