"""Constant-coefficient star stencils whose couplings all differ, for the tests of the constant-coefficient passes
(tests/test_gpu_plane_aniso.py, tests/test_stencils_host.py).

A set is seven constants in the library's slot order (-K, -J, -I, diagonal, +I, +J, +K) — K the slowest axis of a
C-ordered grid (nz, ny, nx), I the fastest.  A 2-D grid (ny, nx) uses slots 1..5, a 1-D grid (n,) slots 2..4.

UNSYM7, SYM7, UNSYM5 and SYM5 are dyadic (multiples of 1/4 below 16): with the plain 2 x 2 (x 2) aggregation of weight
1/4 (1/8) every sum of a Galerkin product is exact in fp64 and in fp32, so every coarse level has exactly ONE value per
offset again — what PlanePlan::build and plane_check_kernel ask of a level (openmg_amd/csrc/plane.hip).  ROUGH7 is not:
its coarse sums may round differently from row to row."""
import functools

import numpy as np
import scipy.sparse as sp

UNSYM7 = (-0.5, -1.25, -2.0, 9.5, -0.75, -1.5, -3.0)      # all seven different; off-diagonals 9.0 against 9.5
SYM7 = (-0.25, -1.0, -3.0, 8.75, -3.0, -1.0, -0.25)       # symmetric positive definite, three different axis couplings
UNSYM5 = (0.0, -1.25, -2.0, 6.0, -0.75, -1.5, 0.0)
SYM5 = (0.0, -1.0, -3.0, 8.5, -3.0, -1.0, 0.0)
ROUGH7 = (-0.3, -1.1, -1.9, 9.7, -0.7, -1.3, -2.9)        # not dyadic

SETS = {"UNSYM7": UNSYM7, "SYM7": SYM7, "UNSYM5": UNSYM5, "SYM5": SYM5, "ROUGH7": ROUGH7}


def slots_of(shape):
    """[(slot, axis, step)] of the off-diagonal slots a grid of this dimension has, in slot order."""
    d = len(shape)
    lower = [(2 - a, d - 1 - a, -1) for a in range(d)]           # -I is slot 2 on the last axis, -J slot 1, -K slot 0
    upper = [(4 + a, d - 1 - a, +1) for a in range(d)]
    return sorted(lower + upper)


def stencil_constant(shape, c):
    """The 3-, 5- or 7-point operator with the constants c on a C-ordered grid, CSR with sorted columns and no stored
    zeros: row r holds c[slot] at column r + step * stride(axis) wherever that neighbour is inside the grid."""
    shape = tuple(int(s) for s in shape)
    assert 1 <= len(shape) <= 3 and len(c) == 7
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, float(c[3]))]
    for slot, axis, step in slots_of(shape):
        here, there = [slice(None)] * len(shape), [slice(None)] * len(shape)
        here[axis] = slice(1, None) if step < 0 else slice(0, -1)
        there[axis] = slice(0, -1) if step < 0 else slice(1, None)
        r, k = idx[tuple(here)].ravel(), idx[tuple(there)].ravel()
        rows.append(r)
        cols.append(k)
        vals.append(np.full(r.size, float(c[slot])))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def aggregation(shape):
    """The plain 2 x 2 (x 2) aggregation of an even grid, weight 1/4 (1/8), sorted columns: the tests' own."""
    if len(shape) == 3:
        from test_gpu_plane import aggregation as agg
    else:
        from test_gpu_plane2d import aggregation2 as agg
    return agg(tuple(shape))


def hierarchy(shape, grids, c):
    """(A, R): the Galerkin lists of stencil_constant(shape, c) over `grids` grids with the plain aggregation."""
    A, R = [stencil_constant(shape, c)], []
    sh = tuple(shape)
    for _ in range(grids - 1):
        R.append(aggregation(sh))
        Ac = sp.csr_matrix((R[-1] @ A[-1]) @ R[-1].T)
        Ac.sort_indices()
        A.append(Ac)
        sh = tuple(s // 2 for s in sh)
    return A, R


def level_shapes(shape, grids):
    return [tuple(s >> l for s in shape) for l in range(grids)]


def values_per_offset(A, shape):
    """{slot: set of the values stored at that slot's offset} of a star-stencil CSR on a grid of `shape`; a stored entry at
    any other offset raises."""
    shape = tuple(int(s) for s in shape)
    strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
    off = {0: 3}
    for slot, axis, step in slots_of(shape):
        off[step * strides[axis]] = slot
    A = sp.csr_matrix(A)
    r = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    d = A.indices.astype(np.int64) - r
    out = {}
    for o in np.unique(d):
        if int(o) not in off:
            raise ValueError("stored entry at offset %d: not a star stencil on %r" % (int(o), shape))
        out[off[int(o)]] = set(A.data[d == o].tolist())
    return out


# ---- the cases of tests/test_gpu_plane_aniso.py (here so that tests/test_stencils_host.py sees them without the GPU tests) ----
# shape, grids, environment, forced tile (None: the plan's own choice)
MARCHING = [
    ((8, 12, 20), 2, {}, None),
    ((10, 8, 6), 2, {}, None),
    ((16, 24, 20), 3, {}, None),                                                        # the block kernel below the finest level
    ((16, 24, 20), 3, {"OMG_PLANE_BLOCK": "0"}, None),                                  # marching, two steps of look-ahead
    ((16, 24, 20), 3, {"OMG_PLANE_BLOCK": "0", "OMG_PLANE_LA2": "0"}, None),            # marching, one step
    ((24, 20, 36), 3, {"OMG_PLANE_BLOCK": "0", "OMG_PLANE_TILE": "16,6,4"}, "16,6,4"),   # several chunks, tiles overhanging the grid
    ((24, 20, 36), 3, {"OMG_PLANE_BLOCK": "0", "OMG_PLANE_TILE": "16,6,24"}, "16,6,24"),  # one chunk
]
MIRROR = [((20, 12, 24), 2), ((24, 20, 36), 3)]
TILE2D = [((10, 22), 2), ((36, 6), 2), ((64, 48), 3)]
SPMV = [("UNSYM7", (8, 12, 20)), ("UNSYM7", (12, 20, 34)), ("UNSYM7", (4, 4, 4)), ("UNSYM5", (10, 22))]
ORACLE = [("UNSYM7", (16, 24, 20), 3), ("UNSYM5", (64, 48), 3)]
SLABS = [((32, 16, 24), 3, 1), ((32, 24, 16), 4, 2)]
FCG_BOX, FCG_LARGE = ((16, 24, 32), 3), ((32, 64, 80), 4)

# every (set, shape, grids) of tests/test_gpu_plane_aniso.py: tests/test_stencils_host.py checks each of them
CASES = sorted(set([("UNSYM7", s, g) for s, g, _, _ in MARCHING] + [("UNSYM7", s, g) for s, g in MIRROR]
                   + [("UNSYM5", s, g) for s, g in TILE2D] + [(n, s, 2) for n, s in SPMV] + ORACLE
                   + [("UNSYM7", s, g) for s, g, _ in SLABS] + [("UNSYM7", (16, 16, 16), 3)]
                   + [("SYM7",) + FCG_BOX, ("UNSYM7",) + FCG_BOX, ("SYM7",) + FCG_LARGE]))
ROUGH_CASE = ((16, 24, 20), 3)


def line_aggregation(n):
    """Pairs of cells, the last aggregate of three when n is odd; weight 0.5."""
    nc = n // 2
    rows = np.minimum(np.arange(n) // 2, nc - 1)
    R = sp.csr_matrix((np.full(n, 0.5), (rows, np.arange(n))), shape=(nc, n))
    R.sort_indices()
    return R


@functools.lru_cache(maxsize=None)
def line_problem():
    """(-1.25, 3.0, -0.75) symmetrised: (-1.0, 2.5, -1.0) on 4099 cells, three grids (4099, 2049, 1024)."""
    n = 4099
    A, R = [stencil_constant((n,), (0, 0, -1.0, 2.5, -1.0, 0, 0))], []
    for _ in range(2):
        R.append(line_aggregation(A[-1].shape[0]))
        Ac = sp.csr_matrix((R[-1] @ A[-1]) @ R[-1].T)
        Ac.sort_indices()
        A.append(Ac)
    assert [M.shape[0] for M in A] == [4099, 2049, 1024]
    b = np.random.default_rng(5).standard_normal(n)
    b.setflags(write=False)
    return A, R, b
