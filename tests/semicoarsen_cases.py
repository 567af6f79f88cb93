"""Shared by tests/test_semicoarsen_host.py and tests/test_gpu_semicoarsen.py: the semicoarsening cases restated with
SciPy and the oracle, never touching the device code under test.

    aniso(shape, c)            sum over the axes a of c[a] * tridiag(-1, 2, -1), Dirichlet, C order
    aggregation(shape, f)      the plain C-order aggregation by factors f (1 or 2 per axis), weight 1 / prod(f), NumPy
    couplings(A, shape)        per axis the sum of |a_ij| and the number of the stored entries at +- the axis's stride
    lists(A0, shape, ...)      restriction and Galerkin lists, the factors picked level by level by the library's exported
                               HOST rule (omg_semicoarsen_rule: no device) from couplings() — or named
    cycles_to(...)             V(1,1) cycles of oracle.mg_oracle.mg_cycle until ||r|| < 1e-8 ||b||

TABLE fixes the factor sequences and cycle counts the GPU tests compare against: they were computed once with the oracle
(tests/test_semicoarsen_host.py computes them again and compares)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from openmg_amd import _hip
from oracle import mg_oracle as orc
from stencils import stencil_constant

TOL = 1e-8
MIN_SIZE = 1          # (the table's cases: three restrictions whatever the coarse sizes; mgSolve's default is 8)


def aniso(shape, c, neumann=False):
    """Dirichlet: diagonal 2 sum(c).  neumann: the same couplings with zero row sums (the boundary rows lose the ghost)."""
    d = len(shape)
    c3 = [0.0] * (3 - d) + [float(v) for v in c]                   # (cz, cy, cx)
    A = stencil_constant(shape, (-c3[0], -c3[1], -c3[2], 2.0 * sum(c3), -c3[2], -c3[1], -c3[0]))
    if neumann:
        A = sp.csr_matrix(A - sp.diags(np.asarray(A.sum(axis=1)).ravel()))
        A.sort_indices()
    return A


def aggregation(shape, factors):
    shape, factors = tuple(shape), tuple(factors)
    coarse = tuple(s // f for s, f in zip(shape, factors))
    cidx = np.arange(int(np.prod(coarse))).reshape(coarse)
    grids = np.meshgrid(*[np.arange(s) // f for s, f in zip(shape, factors)], indexing="ij")
    owner = cidx[tuple(grids)].ravel()
    n = int(np.prod(shape))
    R = sp.csr_matrix((np.full(n, 1.0 / float(np.prod(factors))), (owner, np.arange(n))), shape=(cidx.size, n))
    R.sort_indices()
    return R


def couplings(A, shape):
    """(sums, counts, off_axis) stored entries by their column offset alone."""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    off = np.abs(A.indices.astype(np.int64) - rows)
    strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
    sums = tuple(float(np.abs(A.data[off == s]).sum()) for s in strides)
    counts = tuple(int((off == s).sum()) for s in strides)
    return sums, counts, int((off != 0).sum()) - sum(counts)


def lists(A0, shape, coarsening, restrictions, min_size=8, line_axis=None):
    """(A, R, factors, shapes) with at most `restrictions` restrictions; coarsening 'auto', 'full' or a list of tuples."""
    A, R, factors, shapes = [sp.csr_matrix(A0)], [], [], [tuple(shape)]
    for k in range(restrictions):
        ext = shapes[-1]
        if coarsening == "auto":
            s, c, off = couplings(A[-1], ext)
            f = _hip.semicoarsen_rule(ext, s, c, off, line_axis, level=k)
            if all(v == 1 for v in f):
                break
        elif coarsening == "full":
            if any(e < 4 or e % 2 for e in ext):          # (the yardstick keeps the grid's dimension too)
                break
            f = (2,) * len(ext)
        else:
            f = tuple(coarsening[k])
        if k >= 1 and int(np.prod(ext)) // int(np.prod(f)) <= min_size:
            break
        Rl = aggregation(ext, f)
        Ac = sp.csr_matrix(Rl @ A[-1] @ Rl.T)
        Ac.sort_indices()
        R.append(Rl); A.append(Ac); factors.append(tuple(f)); shapes.append(tuple(e // v for e, v in zip(ext, f)))
    return A, R, factors, shapes


def make_zebra(A_list, shapes, axis):
    """Zebra line Gauss-Seidel along `axis` for mg_cycle's smoother hook: the lines of colour 0 (the parity of the sum of a
    line's other indices), then colour 1, each solved exactly (a sparse direct solve of the entries along the axis)."""
    plans = []
    for A, shape in zip(A_list, shapes):
        A = sp.csr_matrix(A)
        n, s = A.shape[0], int(np.prod(shape[axis + 1:]))
        T = sp.diags([A.diagonal(-s), A.diagonal(), A.diagonal(s)], [-s, 0, s], format="csr")
        C = sp.csr_matrix(A - T)
        others = np.meshgrid(*[np.arange(e) if a != axis else np.zeros(e, dtype=int) for a, e in enumerate(shape)], indexing="ij")
        colour = (sum(others) % 2).ravel()
        sets = [np.flatnonzero(colour == c) for c in (0, 1)]
        plans.append((C, [(rows, spla.splu(sp.csc_matrix(T[rows][:, rows]))) for rows in sets]))

    def smooth(A, b, x, its, level):
        C, sets = plans[level]
        x = np.array(x, dtype=np.float64).ravel()
        b = np.asarray(b, dtype=np.float64).ravel()
        for _ in range(its):
            for rows, lu in sets:
                x[rows] = lu.solve((b - C @ x)[rows])
        return x
    return smooth


def smoother_of(kind, A, shapes, line_axis=None):
    return make_zebra(A, shapes, line_axis) if kind == "line" else orc.make_smoother(kind, A)


def cycles_to(A, R, b, sm, pre=1, post=1, limit=400):
    """(cycles, norms): V(pre, post) cycles of the oracle until ||r|| < TOL ||b||"""
    p = {"coarsestLevel": len(R), "preIterations": pre, "postIterations": post}
    target = TOL * float(np.linalg.norm(b))
    x, norms = None, []
    while len(norms) < limit:
        x, info = orc.mg_cycle(A, b, 0, R, p, initial=x, smoother=sm)
        norms.append(float(info["norm"]))
        if norms[-1] < target:
            break
    return len(norms), norms


def rhs(n):
    b = np.random.default_rng(12345).standard_normal(n)
    b.setflags(write=False)
    return b


# name: shape, c per axis (C order: z, y, x), smoother, line axis (an index into shape), restrictions,
#       expected factors under 'auto', oracle cycles to 1e-8 with 'auto', oracle cycles with full coarsening.
# No deciding cycle's norm may lie within 1 % of the threshold.  Zebra lines along x at 1 : 100 : 100 on (16, 16, 16) broke
# that rule — full coarsening: 84 cycles, the 84th at 0.992 of the threshold — and was REPLACED by the same operator,
# smoother and number of grids on (32, 32, 32), the next size up: 41 cycles at 0.792 (the 40th at 1.139), full coarsening
# 193 at 0.952 (the 192nd at 1.028).  (On 16^3 the oracle takes 22 cycles with 'auto', and full coarsening stands at
# 8.246e-4 ||b|| after those 22: the line smoother makes the first cycles fast there and the stall comes later.)
TABLE = {
    "iso16": ((16, 16, 16), (1, 1, 1), "colour", None, 3, [(2, 2, 2)] * 3, 35, 35),
    "yx10": ((16, 16, 16), (1, 10, 10), "colour", None, 3, [(1, 2, 2)] * 3, 31, 62),
    "yx100": ((16, 16, 16), (1, 100, 100), "colour", None, 3, [(1, 2, 2)] * 3, 32, 166),
    "x100": ((16, 16, 16), (1, 1, 100), "colour", None, 3, [(1, 1, 2)] * 3, 25, 144),
    "z100x10": ((16, 16, 16), (100, 1, 10), "colour", None, 3, [(2, 1, 1)] * 3, 27, 145),
    "box_yx10": ((8, 12, 20), (1, 10, 10), "colour", None, 3, [(1, 2, 2), (1, 2, 2), (2, 1, 1)], 25, 59),
    "box_z100x10": ((8, 12, 20), (100, 1, 10), "colour", None, 3, [(2, 1, 1), (2, 1, 1), (1, 1, 2)], 14, 59),
    "line_yx100": ((32, 32, 32), (1, 100, 100), "line", 2, 3, [(1, 2, 2)] * 3, 41, 193),
    "line_y10x100": ((16, 16, 16), (1, 10, 100), "line", 2, 3, [(1, 2, 2)] * 3, 10, 15),
    "line_x100": ((16, 16, 16), (1, 1, 100), "line", 2, 3, [(2, 2, 2)] * 3, 4, 4),
}


@functools.lru_cache(maxsize=None)
def case(name, coarsening="auto"):
    """The oracle's view of a TABLE row: lists, factors, shapes, b, smoother, cycles to 1e-8 and every cycle's norm."""
    shape, c, kind, line_axis, restrictions = TABLE[name][:5]
    A0 = aniso(shape, c)
    A, R, factors, shapes = lists(A0, shape, coarsening, restrictions, min_size=MIN_SIZE, line_axis=line_axis)
    b = rhs(A0.shape[0])
    sm = smoother_of(kind, A, shapes, line_axis)
    count, norms = cycles_to(A, R, b, sm)
    return {"name": name, "shape": shape, "A0": A0, "A": A, "R": R, "factors": factors, "shapes": shapes, "b": b, "sm": sm,
            "kind": kind, "line_axis": line_axis, "cycles": count, "norms": norms, "restrictions": restrictions}
