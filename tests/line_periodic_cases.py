"""Shared by the tests of the line smoother on periodic operators ('smoother': 'line-periodic', OMG_SMOOTH_LINE* | 8): the
operators, the lists and a restatement of the zebra sweep and of the cycle that never touches the code under test.

    operators     face-coefficient stencils in 2-D and 3-D (a factor per axis, an optional random cell coefficient) with
                  any set of PERIODIC axes — the face between the last and the first cell of a line, the wrapped entry at
                  the seam rows —, Dirichlet or pure Neumann on the others; 'chan' comes from operators.stencil7_kappa
                  with tanh-clustered widths.  Restrictions: the plain aggregation; coarse operators: Galerkin products.
    sweep         T = the entries of A whose row and column lie on one grid line along the axis (the wrap included),
                  C = A - T.  Lines are coloured by the parity of the sum of their other indices; colour 0, then colour 1:
                  x_colour <- T_cc^-1 (b - C x)_colour, T_cc factorised by SuperLU in float64 — NOT the cyclic recurrence
                  of csrc/line.hip.  C couples no two lines of one colour (asserted).
    cycle         tests/test_gpu_line.py's restated_cycle: the oracle's residual, products and coarse solve.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from openmg_amd import operators
from oracle import mg_oracle as orc

CYC = dict(rtol=1e-9, atol=1e-11)
NORM_RTOL = 1e-10
U64 = 2.0 ** -53
EPS32 = float(np.finfo(np.float32).eps)
SWEEPS = [(1, 1), (2, 1), (1, 0), (0, 1)]
SHAPES = [("V", 1.0), ("F", 1.8), ("W", 1.5)]


# ------------------------------------------------------------------------------------ operators --
def face_operator(shape, factors, seed=None, dirichlet=True, periodic=(), sigma=0.0):
    """sum over the axes a of factors[a] * (differences across the faces normal to a, weighted by the mean of the two cells'
    coefficients).  A periodic axis (extent >= 3) has the face between its last and its first cell and no boundary face; on
    the others Dirichlet adds the boundary faces (a ghost value 0), otherwise the rows sum to sigma.  A factor 0.0 leaves
    STORED zeros.  C order, sorted CSR."""
    shape = tuple(shape)
    d, n = len(shape), int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    kap = np.ones(shape) if seed is None else np.random.default_rng(seed).uniform(0.5, 2.0, shape)
    diag = np.full(shape, float(sigma))
    rows, cols, vals = [], [], []
    for a, f in enumerate(factors):
        lo, hi = [slice(None)] * d, [slice(None)] * d
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        pairs = [(tuple(lo), tuple(hi))]
        if a in periodic:
            assert shape[a] >= 3
            lo[a], hi[a] = slice(-1, None), slice(0, 1)
            pairs.append((tuple(lo), tuple(hi)))
        for lo_, hi_ in pairs:
            c = f * 0.5 * (kap[lo_] + kap[hi_])
            rows += [idx[lo_].ravel(), idx[hi_].ravel()]
            cols += [idx[hi_].ravel(), idx[lo_].ravel()]
            vals += [-c.ravel(), -c.ravel()]
            diag[lo_] += c
            diag[hi_] += c
        if dirichlet and a not in periodic:
            for end in (0, -1):
                face = [slice(None)] * d
                face[a] = end
                diag[tuple(face)] += f * kap[tuple(face)]
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def aggregation(shape):
    """the plain aggregation of 2 x 2 (x 2) cells (an odd extent: the last cell alone), weight 1 / 2^d; the coarse shape"""
    shape = tuple(shape)
    d, n = len(shape), int(np.prod(shape))
    coarse = tuple((s + 1) // 2 for s in shape)
    cidx = np.arange(int(np.prod(coarse))).reshape(coarse)
    grids = np.meshgrid(*[np.arange(s) // 2 for s in shape], indexing="ij")
    owner = cidx[tuple(grids)].ravel()
    R = sp.csr_matrix((np.full(n, 1.0 / 2 ** d), (owner, np.arange(n))), shape=(cidx.size, n))
    R.sort_indices()
    return R, coarse


def lists_of(A0, shape, grids):
    A, R, shapes = [A0], [], [tuple(shape)]
    for _ in range(grids - 1):
        Rl, coarse = aggregation(shapes[-1])
        Ac = sp.csr_matrix(Rl @ A[-1] @ Rl.T)
        Ac.sort_indices()
        R.append(Rl); A.append(Ac); shapes.append(coarse)
    return A, R, shapes


def tanh_widths(n, beta):
    """n cell widths on [0, 1] clustered towards BOTH walls: faces y_f = (1 + tanh(beta (2 f / n - 1)) / tanh(beta)) / 2"""
    f = np.arange(n + 1, dtype=np.float64)
    return np.diff(0.5 * (1.0 + np.tanh(beta * (2.0 * f / n - 1.0)) / np.tanh(beta)))


def padded(widths):
    """one ghost entry at each end: the boundary cell's own width (the boundary value at the mirrored cell centre)"""
    return np.concatenate([widths[:1], widths, widths[-1:]])


CHAN_SHAPE, CHAN_BETA = (8, 32, 8), 3.0


def chan_arguments(neumann=False, seed=31):
    """the turbulent channel's operator: periodic in z and x, walls in y (Dirichlet, or Neumann: singular), y clustered by
    tanh(beta = 3) on the unit box, kappa = exp(U(-1/2, 1/2)); what operators.stencil7_kappa and Solver.from_kappa take"""
    nz, ny, nx = CHAN_SHAPE
    kappa = np.exp(np.random.default_rng(seed).uniform(-0.5, 0.5, (nz + 2, ny + 2, nx + 2)))
    wall_y = "neumann" if neumann else "dirichlet"
    walls = ("periodic", "periodic", wall_y, wall_y, "periodic", "periodic")
    spacing = (padded(np.full(nz, 1.0 / nz)), padded(tanh_widths(ny, CHAN_BETA)), padded(np.full(nx, 1.0 / nx)))
    return kappa, walls, spacing


# name: shape, periodic axes, the lines' (strong) axis, grids, factor per axis, seed, Dirichlet on the other axes, sigma
CASES = {
    "wrap": ((10, 12, 14), (0, 2), 1, 2, (1.0, 4.0, 1.0), 41, True, 0.0),       # 70 lines per colour: a full and a ragged bundle
    "ringx": ((8, 12, 16), (2,), 2, 3, (1.0, 1.0, 100.0), 42, True, 0.0),      # a unit-stride cyclic line of length 16
    "ringz": ((16, 12, 8), (0,), 0, 3, (4.0, 1.0, 1.0), 43, True, 0.0),
    "odd": ((8, 9, 12), (1,), 1, 2, (1.0, 4.0, 1.0), 44, True, 0.0),           # a cyclic line of odd length 9
    "ragged": ((4, 6, 139), (2,), 2, 2, (1.0, 1.0, 4.0), 45, True, 0.0),       # 17 groups and 3 cells: the special cells in the tail
    "tiny": ((6, 8, 3), (2,), 2, 2, (1.0, 1.0, 4.0), 46, True, 0.0),           # m = 3
    "box": ((16, 8, 8), (0, 1, 2), 0, 3, (4.0, 1.0, 1.0), 47, True, 0.375),
    "boxN": ((16, 8, 8), (0, 1, 2), 0, 3, (4.0, 1.0, 1.0), 48, False, 0.0),    # singular: nullspace='constant'
    "sqring": ((16, 24), (1,), 1, 3, (1.0, 4.0), 49, True, 0.0),
    "sqwrap": ((16, 24), (0,), 1, 3, (1.0, 4.0), 50, True, 0.0),
    # test_gpu_line's in-grid constructions
    "var1": ((8, 12, 20), (), 1, 3, (1.0, 100.0, 1.0), 12, True, 0.0),
    "sq0": ((16, 24), (), 0, 3, (100.0, 1.0), 16, True, 0.0),
    "long": ((4, 6, 136), (), 2, 2, (1.0, 1.0, 100.0), 14, True, 0.0),
    # the auto axis: z and x periodic, y a hundred times stronger
    "auto": ((8, 32, 8), (0, 2), 1, 3, (1.0, 100.0, 1.0), 51, True, 0.0),
}
PERIODIC = ["wrap", "chan", "ringx", "ringz", "odd", "ragged", "tiny", "box", "boxN", "sqring", "sqwrap"]
IN_GRID = ["var1", "sq0", "long"]


@functools.lru_cache(maxsize=None)
def problem(name):
    if name in ("chan", "chanN"):
        shape, periodic, axis, grids = CHAN_SHAPE, (0, 2), 1, 3
        kappa, walls, spacing = chan_arguments(neumann=name == "chanN")
        A0 = sp.csr_matrix(operators.stencil7_kappa(kappa, walls, None, spacing=spacing))
        A0.sort_indices()
        singular = name == "chanN"
    else:
        shape, periodic, axis, grids, factors, seed, dirichlet, sigma = CASES[name]
        A0 = face_operator(shape, factors, seed, dirichlet, periodic, sigma)
        singular = sigma == 0.0 and (not dirichlet or len(periodic) == len(shape))
    A, R, shapes = lists_of(A0, shape, grids)
    rng = np.random.default_rng(12345)
    b = rng.standard_normal(A0.shape[0]) + (0.3 if singular else 0.0)
    return {"name": name, "shape": tuple(shape), "periodic": tuple(periodic), "A0": A0, "A": A, "R": R, "shapes": shapes, "b": b,
            "axis": axis, "nullspace": "constant" if singular else None}


def periodic_on(pr, level):
    """the axes that are periodic on that level as the plan reads them: extent >= 3 and row 0 holds column (e - 1) s"""
    shape = pr["shapes"][level]
    A = sp.csr_matrix(pr["A"][level])
    row0 = set(A.indices[A.indptr[0]:A.indptr[1]].tolist())
    out = []
    for a, e in enumerate(shape):
        s = int(np.prod(shape[a + 1:]))
        if e >= 3 and (e - 1) * s in row0:
            out.append(a)
    return tuple(out)


def admissible_axes(pr):
    """the line axes the library takes: on every smoothed level every periodic axis ACROSS the lines has an even extent"""
    out = []
    for axis in range(len(pr["shape"])):
        ok = True
        for level in range(len(pr["R"])):
            for a in periodic_on(pr, level):
                if a != axis and pr["shapes"][level][a] % 2:
                    ok = False
        if ok:
            out.append(axis)
    return out


# ------------------------------------------------------------------------------ the restatement --
@functools.lru_cache(maxsize=None)
def split(name, level, axis):
    """of level `level` of problem `name`: T (same-line entries along `axis`, the wrap included), C = A - T, and per colour
    the rows and the SuperLU factorisation of T's colour block"""
    pr = problem(name)
    A, shape = sp.coo_matrix(pr["A"][level]), pr["shapes"][level]
    coords = np.array(np.unravel_index(np.arange(A.shape[0]), shape))
    others = np.delete(coords, axis, axis=0)
    line = np.ravel_multi_index(tuple(others), tuple(e for a, e in enumerate(shape) if a != axis)) if len(shape) > 1 else np.zeros(A.shape[0], int)
    colour = others.sum(axis=0) % 2
    same = line[A.row] == line[A.col]
    T = sp.csr_matrix((A.data[same], (A.row[same], A.col[same])), shape=A.shape)
    C = sp.csr_matrix((A.data[~same], (A.row[~same], A.col[~same])), shape=A.shape)
    blocks = []
    for c in (0, 1):
        rows = np.flatnonzero(colour == c)
        Ccc = C[rows][:, rows]
        assert Ccc.nnz == 0 or not np.any(Ccc.data), "C couples two lines of colour %d on level %d of %s" % (c, level, name)
        blocks.append((rows, spla.splu(sp.csc_matrix(T[rows][:, rows]))))
    return T, C, blocks


def zebra(name, level, axis, b, x, sweeps=1):
    _, C, blocks = split(name, level, axis)
    x = np.array(x, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    for _ in range(sweeps):
        for rows, lu in blocks:
            x[rows] = lu.solve((b - C @ x)[rows])
    return x


def line_condition(pr, level, axis):
    """||T||_inf ||T^-1||_inf of the lines' blocks WITH their corner entries, bounded as in tests/test_gpu_line.py: the rows
    of T stay strictly diagonally dominant (the cross couplings, the boundary faces or sigma), so ||T^-1||_inf <=
    1 / min_i (|d_i| - sum of the row's other entries of T) (Varah); ||T||_inf <= the row sum of |A|."""
    T, _, _ = split(pr["name"], level, axis)
    d = np.abs(T.diagonal())
    margin = float((d - (np.asarray(abs(T).sum(axis=1)).ravel() - d)).min())
    assert margin > 0
    return float(abs(pr["A"][level]).sum(axis=1).max()) / margin


def visits_of(shape, level, coarsest):
    if shape == "V" or level + 1 == coarsest:
        return [shape]
    return ["F", "V"] if shape == "F" else ["W", "W"]


def prolongations(R, alpha, dtype=np.float64):
    out = []
    for Rl in R:
        P = sp.csr_matrix(sp.csr_matrix(Rl).T)
        a = P.data.astype(dtype).astype(np.float64)
        P.data = (np.float64(alpha) * a).astype(dtype).astype(np.float64)
        out.append(P)
    return out


def mean_of(x):
    return math.fsum(x) / x.size


def coarse_solve(pr, b):
    Ac = pr["A"][-1]
    if pr["nullspace"] is None:
        return np.ravel(orc.coarse_solve(Ac, np.asarray(b, dtype=np.float64).reshape((-1, 1))))
    # OMG_NULLSPACE_CONSTANT: (A + gamma 1 1^T)^-1, gamma = (mean diagonal) / n  (tests/test_gpu_nullspace.py)
    n = Ac.shape[0]
    gamma = (float(Ac.diagonal().sum()) / n) / n
    return np.ravel(np.linalg.solve(Ac.toarray() + gamma * np.ones((n, n)), np.asarray(b, dtype=np.float64).ravel()))


def smoother_of(pr, kind, axis):
    if kind == "line":
        return lambda A, b, x, its, level: zebra(pr["name"], level, axis, b, x, its)
    return orc.make_smoother(kind, pr["A"])


def restated_cycle(pr, P, b, level, pre, post, shape, sm, x=None):
    A, R = pr["A"], pr["R"]
    coarsest = len(R)
    b = np.asarray(b, dtype=np.float64).ravel()
    N = b.size
    if level == coarsest:
        return coarse_solve(pr, b)
    u = np.zeros(N) if x is None else np.array(x, dtype=np.float64).ravel()
    if pre > 0:
        u = np.ravel(sm(A[level], b, u, pre, level))
    NH = R[level].shape[0]
    r = orc.get_residual(b, A[level], u, N)
    bc = np.asarray(orc.flexible_mmult(R[level], r.reshape((N, 1)))).reshape((NH,))
    e = None
    for s in visits_of(shape, level, coarsest):
        e = restated_cycle(pr, P, bc, level + 1, pre, post, s, sm, e)
    u = np.asarray(u).reshape((N,)) + np.asarray(orc.flexible_mmult(P[level], e.reshape((NH, 1)))).reshape((N,))
    if post > 0:
        u = np.ravel(sm(A[level], b, u, post, level))
    return u


def projected_b(pr):
    return pr["b"] if pr["nullspace"] is None else pr["b"] - mean_of(pr["b"])


def restated_cycles(pr, sm, shape, alpha, pre, post, n, x0=None):
    """norms and iterate of n cycles; with a null space: on the projected b, the iterate projected on the way out"""
    P = prolongations(pr["R"], alpha)
    b = projected_b(pr)
    x, norms = x0, []
    for _ in range(n):
        x = restated_cycle(pr, P, b, 0, pre, post, shape, sm, x)
        norms.append(float(np.linalg.norm(orc.get_residual(b, pr["A"][0], x, b.size))))
    return np.array(norms), (x if pr["nullspace"] is None else x - mean_of(x))


def restated_cycles_to(pr, sm, shape, alpha, pre, post, target, limit):
    """the norms of cycles until one is below target (at most `limit`)"""
    P = prolongations(pr["R"], alpha)
    b = projected_b(pr)
    x, norms = None, []
    while len(norms) < limit:
        x = restated_cycle(pr, P, b, 0, pre, post, shape, sm, x)
        norms.append(float(np.linalg.norm(orc.get_residual(b, pr["A"][0], x, b.size))))
        if norms[-1] < target:
            break
    return norms


def norm_floor(A0, b, x):
    """what fp64 itself leaves open in ||b - A0 x|| (tests/test_gpu_cycle_shapes.py norm_floor)"""
    k = int(np.diff(sp.csr_matrix(A0).indptr).max())
    return 2.0 * (k + 2) * U64 * float(np.linalg.norm(np.abs(b) + abs(A0) @ np.abs(x)))


def cyclic_solve(low, diag, up, r):
    """A NumPy transcription of the factorisation csrc/line.hip stores for a cyclic line: M = tridiag(low, diag,
    up) with M[0, m-1] = low[0] and M[m-1, 0] = up[m-1]; LU without pivoting, a fill column g and a fill row h.  Only the
    host test uses it (against dense solves): the sweep above does not."""
    m = len(diag)
    p, f, g, h, uh = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m), np.array(up, dtype=np.float64)
    p[0] = diag[0]
    for i in range(1, m - 1):
        f[i] = low[i] / p[i - 1]
        p[i] = diag[i] - f[i] * up[i - 1]
    g[0] = low[0]
    for i in range(1, m - 2):
        g[i] = -f[i] * g[i - 1]
    uh[m - 2] = up[m - 2] - f[m - 2] * g[m - 3]
    h[0] = up[m - 1] / p[0]
    for i in range(1, m - 2):
        h[i] = -h[i - 1] * up[i - 1] / p[i]
    h[m - 2] = (low[m - 1] - h[m - 3] * up[m - 3]) / p[m - 2]
    p[m - 1] = diag[m - 1] - float(np.dot(h[:m - 2], g[:m - 2])) - h[m - 2] * uh[m - 2]
    g[m - 2] = 0.0
    y = np.zeros(m)
    y[0] = r[0]
    for i in range(1, m - 1):
        y[i] = r[i] - f[i] * y[i - 1]
    y[m - 1] = r[m - 1] - float(np.dot(h[:m - 1], y[:m - 1]))
    x = np.zeros(m)
    x[m - 1] = y[m - 1] / p[m - 1]
    for i in range(m - 2, -1, -1):
        x[i] = (y[i] - uh[i] * x[i + 1] - g[i] * x[m - 1]) / p[i]
    return x
