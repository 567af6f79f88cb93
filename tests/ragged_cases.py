"""Shared by tests/test_ragged_host.py and tests/test_gpu_ragged.py: grids of any extent (parameters['oddExtents'] =
'merge') restated with NumPy, SciPy and the oracle, never touching the device code under test.

    aggregation(shape, f)      per coarsened axis of extent e the owner of fine index i is min(i // 2, e // 2 - 1) — an odd
                               extent's last cell joins the last pair —, one weight 1 / prod(f), columns sorted
    full_factors(shape)        2 on every axis with extent >= 4, 1 on the others
    lists(A0, shape, ...)      restriction and Galerkin lists (R A R^T by SciPy); the factors 'full' (full_factors per level),
                               'auto' (the library's exported HOST rule with OMG_ODD_MERGE on semicoarsen_cases.couplings:
                               no device) or named
    cycles_to(...)             V(1,1) cycles of oracle.mg_oracle.mg_cycle until ||r|| < 1e-8 ||b||

TABLE fixes the factor sequences, level shapes and cycle counts the GPU tests compare against: they were computed once with
the oracle (tests/test_ragged_host.py computes them again and compares).  As in semicoarsen_cases no deciding cycle's
norm, and none before it, may lie within 1 % of the threshold."""
import functools
import math

import numpy as np
import scipy.sparse as sp

from openmg_amd import _hip
from oracle import mg_oracle as orc

import semicoarsen_cases as sc
from semicoarsen_cases import TOL, aniso, couplings, rhs, smoother_of

MIN_SIZE = 1          # (the table's cases: the depth is 'restrictions' or where no axis is eligible; mgSolve's default is 8)


def aggregation(shape, factors):
    shape, factors = tuple(shape), tuple(factors)
    coarse = tuple(s // f for s, f in zip(shape, factors))
    cidx = np.arange(int(np.prod(coarse))).reshape(coarse)
    owners = [np.minimum(np.arange(s) // f, s // f - 1) for s, f in zip(shape, factors)]
    owner = cidx[tuple(np.meshgrid(*owners, indexing="ij"))].ravel()
    n = int(np.prod(shape))
    R = sp.csr_matrix((np.full(n, 1.0 / float(np.prod(factors))), (owner, np.arange(n))), shape=(cidx.size, n))
    R.sort_indices()
    return R


def full_factors(shape):
    return tuple(2 if e >= 4 else 1 for e in shape)


def lists(A0, shape, coarsening, restrictions, min_size=8, line_axis=None):
    """(A, R, factors, shapes) with at most `restrictions` restrictions; coarsening 'full', 'auto' or a list of tuples.  The
    depth rule is restrictionList's: the first restriction always, then until the coarse level would have <= min_size rows;
    the hierarchy ends where no axis has an extent >= 4."""
    A, R, factors, shapes = [sp.csr_matrix(A0)], [], [], [tuple(shape)]
    for k in range(restrictions):
        ext = shapes[-1]
        if coarsening == "auto":
            s, c, off = couplings(A[-1], ext)
            f = _hip.semicoarsen_rule(ext, s, c, off, line_axis, level=k, oddExtents="merge")
        elif coarsening == "full":
            f = full_factors(ext)
        else:
            f = tuple(coarsening[k])
        if all(v == 1 for v in f):
            break
        coarse = tuple(e // v for e, v in zip(ext, f))
        if k >= 1 and int(np.prod(coarse)) <= min_size:
            break
        Rl = aggregation(ext, f)
        Ac = sp.csr_matrix(Rl @ A[-1] @ Rl.T)
        Ac.sort_indices()
        R.append(Rl); A.append(Ac); factors.append(tuple(f)); shapes.append(coarse)
    return A, R, factors, shapes


def regularised_solve(A, b):
    """The coarse solve of a singular level with the constant null space: (A_c + gamma 1 1^T)^-1 b, gamma = (mean diagonal) / n
    — what the library documents for OMG_NULLSPACE_CONSTANT, in NumPy."""
    Ad = A.toarray() if sp.issparse(A) else np.asarray(A, dtype=np.float64)
    n = Ad.shape[0]
    gamma = (float(np.trace(Ad)) / n) / n
    return np.ravel(np.linalg.solve(Ad + gamma * np.ones((n, n)), np.asarray(b, dtype=np.float64).reshape(-1)))


def cycles_to(A, R, b, sm, pre=1, post=1, limit=400, neumann=False):
    """(cycles, norms, x): V(pre, post) cycles of the oracle until ||r|| < TOL ||b||.  neumann: b has mean 0 already, the
    coarsest level is solved on the complement of the constants (regularised_solve) and x comes out with mean 0."""
    p = {"coarsestLevel": len(R), "preIterations": pre, "postIterations": post}
    target = TOL * float(np.linalg.norm(b))
    x, norms = None, []
    kept = orc.coarse_solve
    if neumann:
        orc.coarse_solve = regularised_solve
    try:
        while len(norms) < limit:
            x, info = orc.mg_cycle(A, b, 0, R, p, initial=x, smoother=sm)
            norms.append(float(info["norm"]))
            if norms[-1] < target:
                break
    finally:
        orc.coarse_solve = kept
    x = np.ravel(x)
    if neumann:
        x = x - math.fsum(x) / x.size
    return len(norms), norms, x


def rhs_of(n, neumann=False):
    b = np.array(rhs(n))
    if neumann:
        b -= math.fsum(b) / b.size
    b.setflags(write=False)
    return b


# name: shape, c per axis (C order), smoother, line axis (an index into shape), restrictions, coarsening, pure Neumann,
#       expected factors, expected level shapes, oracle cycles to 1e-8 ||b||.  All with factor 2 wherever the extent is >= 4
#       ('full') unless the row says 'auto'; minSize 1.
def _cube(e, n):
    return [(e >> k,) * 3 for k in range(n)]


TABLE = {
    "iso15": ((15, 15, 15), (1, 1, 1), "colour", None, 3, "full", False, [(2, 2, 2)] * 2, _cube(15, 3), 38),
    "iso17": ((17, 17, 17), (1, 1, 1), "colour", None, 3, "full", False, [(2, 2, 2)] * 3, _cube(17, 4), 40),
    "box9": ((9, 14, 21), (1, 1, 1), "colour", None, 3, "full", False, [(2, 2, 2), (2, 2, 2), (1, 1, 2)],
             [(9, 14, 21), (4, 7, 10), (2, 3, 5), (2, 3, 2)], 30),
    "box5": ((5, 7, 11), (1, 1, 1), "colour", None, 3, "full", False, [(2, 2, 2), (1, 1, 2)], [(5, 7, 11), (2, 3, 5), (2, 3, 2)], 18),
    "sq13": ((13, 10), (1, 1), "colour", None, 3, "full", False, [(2, 2), (2, 2)], [(13, 10), (6, 5), (3, 2)], 26),
    "auto_yx100": ((15, 15, 15), (1, 100, 100), "colour", None, 3, "auto", False, [(1, 2, 2), (1, 2, 2), (2, 1, 1)],
                   [(15, 15, 15), (15, 7, 7), (15, 3, 3), (7, 3, 3)], 36),
    "line_x100": ((15, 15, 15), (1, 1, 100), "line", 2, 3, "full", False, [(2, 2, 2)] * 2, _cube(15, 3), 4),
    "neumann_box9": ((9, 14, 21), (1, 1, 1), "colour", None, 3, "full", True, [(2, 2, 2), (2, 2, 2), (1, 1, 2)],
                     [(9, 14, 21), (4, 7, 10), (2, 3, 5), (2, 3, 2)], 80),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The oracle's view of a TABLE row: lists, factors, shapes, b, smoother, cycles to 1e-8, every cycle's norm, the iterate."""
    shape, c, kind, line_axis, restrictions, coarsening, neumann = TABLE[name][:7]
    A0 = aniso(shape, c, neumann=neumann)
    A, R, factors, shapes = lists(A0, shape, coarsening, restrictions, min_size=MIN_SIZE, line_axis=line_axis)
    b = rhs_of(A0.shape[0], neumann)
    sm = smoother_of(kind, A, shapes, line_axis)
    count, norms, x = cycles_to(A, R, b, sm, neumann=neumann)
    return {"name": name, "shape": shape, "A0": A0, "A": A, "R": R, "factors": factors, "shapes": shapes, "b": b, "sm": sm,
            "kind": kind, "line_axis": line_axis, "cycles": count, "norms": norms, "x": x, "restrictions": restrictions,
            "coarsening": coarsening, "neumann": neumann}
