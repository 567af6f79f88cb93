"""Hierarchy setup with the reference's names (openmg/operators.py).

restriction() and the Galerkin product run on the GPU (omg_restriction / omg_rap); the
Poisson generators are test-input builders and stay NumPy like the reference's.
"""
import numpy as np
import scipy.sparse as sp

from . import _hip, tools


def restriction(shape, dense=False, factors=None, oddExtents=None):
    """R of shape (N / 2**alpha, N): every coarse cell averages its 2**alpha fine cells
    (openmg/operators.py:15-89).  Index conventions follow the reference exactly, including
    the second-axis offset shape[0] and third-axis offset shape[0]*shape[1] (Q6).

    factors (not in the reference): 1 or 2 per axis of a 2-D / 3-D `shape` — the plain C-order aggregation that
    coarsens only the axes with factor 2 (semicoarsening), weight 1 / prod(factors); ValueError for a factor other
    than 1 or 2, all ones, or a 2 on an extent that is odd or below 4.

    oddExtents (with factors): None, or 'merge' — a 2 is taken on any extent e >= 4 and gives e // 2 coarse cells, the
    last of which holds three fine cells along an odd axis; every entry keeps the weight 1 / prod(factors)."""
    shape = tuple(int(s) for s in shape)
    if factors is not None:
        R = _hip.restriction_ex(shape, checkFactors(shape, factors, oddExtents), oddExtents)
        return R.toarray() if dense else R
    if oddExtents is not None:
        raise ValueError("restriction(): oddExtents goes with factors (the reference's restriction knows no such key)")
    alpha = len(shape)
    N = tools.product(shape)
    n = N // (2 ** alpha)
    if n in (0, 1):
        raise ValueError("New restriction matrix would have shape %s. Coarse set would have %d point(s)! "
                         "Try a larger problem or fewer gridLevels." % (str((n, N)), n))
    if alpha > 3:
        raise ValueError("restriction(): Greater than 3 dimensions is not implemented. "
                         "(shape was %s .)" % str(shape))
    R = _hip.restriction(shape)
    if any(s % 2 for s in shape) or len(set(shape)) > 1:
        # unequal / odd extents: the reference's LIL assignment stores a repeated (r, c)
        # once and zip() leaves trailing rows empty; canonicalise the same way.
        R = R.tocoo()
        key = np.unique(R.row.astype(np.int64) * N + R.col)
        R = sp.csr_matrix((np.full(key.size, 1.0 / 2 ** alpha), (key // N, key % N)), shape=(n, N))
    R.sort_indices()
    return R.toarray() if dense else R


def restrictionList(problemShape, coarsestLevel, minSize, dense=False, verbose=False):
    """One restriction per level transition (openmg/operators.py:92-141): always the first,
    then more until `coarsestLevel` exist or the next coarse size would be <= minSize."""
    if verbose:
        print("Generating restriction matrices; dense=%s" % dense)
    extents = np.array(problemShape)
    out = [restriction(tuple(extents // 1), dense=dense)]
    for level in range(1, coarsestLevel + 1):
        candidate = restriction(tuple(extents // (2 ** level)), dense=dense)
        if candidate.shape[0] <= minSize:
            break
        out.append(candidate)
    return out


def coeffecientList(A_in, R, dense=False, verbose=False):
    """[A_0, R_0 A_0 R_0^T, ...] (openmg/operators.py:144-188), each Galerkin product done on
    the device.  (Spelling as in the reference.)"""
    if verbose:
        print("Generating coefficient matrices; dense=%s ..." % dense, end=" ")
    levels = [sp.csr_matrix(A_in)]
    for Rl in R:
        levels.append(_hip.rap(sp.csr_matrix(Rl), levels[-1]))
    if dense:
        levels = [M.toarray() for M in levels]
    if verbose:
        print("made %i A matrices" % len(levels))
    return levels


# ---- semicoarsening (NOT in the reference): a factor of 1 or 2 per axis and restriction -------
def canHalve(extent, oddExtents=None):
    """May an axis of this extent take a factor 2: even and >= 4, or — oddExtents 'merge' — just >= 4."""
    return extent >= 4 and (extent % 2 == 0 or _hip.odd_code(oddExtents) == _hip.ODD_MERGE)


def fullFactors(shape, oddExtents="merge"):
    """The factors of 'full' coarsening with oddExtents 'merge' on a level's grid: 2 on every axis that can take it, 1 on
    the others; all ones where no axis can."""
    return tuple(2 if canHalve(int(s), oddExtents) else 1 for s in shape)


def checkFactors(shape, factors, oddExtents=None):
    """One restriction's factors as a tuple of ints, checked against the extents they apply to; ValueError otherwise.
    oddExtents: None (a 2 needs an even extent >= 4) or 'merge' (a 2 needs an extent >= 4)."""
    merge = _hip.odd_code(oddExtents) == _hip.ODD_MERGE
    shape = tuple(int(s) for s in shape)
    try:
        entry = tuple(factors)
    except TypeError:
        raise ValueError("a coarsening entry must be a tuple of one factor per axis of %s, not %r" % (shape, factors))
    if len(entry) != len(shape) or any(isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f not in (1, 2) for f in entry):
        raise ValueError("a coarsening entry must hold a factor of 1 or 2 for each axis of %s, not %r" % (shape, factors))
    entry = tuple(int(f) for f in entry)
    if all(f == 1 for f in entry):
        raise ValueError("a coarsening entry of all ones coarsens nothing: %r" % (factors,))
    for axis, (s, f) in enumerate(zip(shape, entry)):
        if f == 2 and not canHalve(s, oddExtents):
            raise ValueError("a factor of 2 needs an %sextent >= 4: axis %d of the level's grid %s has %d"
                             % ("" if merge else "even ", axis, shape, s))
    return entry


def coarseningOf(coarsening, problemShape=None, coarsestLevel=None, minSize=None, oddExtents=None):
    """parameters['coarsening'] checked, without any device work: None for full coarsening (None / 'full'), 'auto', or the
    list of factor tuples that will be used — the depth rule is restrictionList's: the first restriction always, then more
    until coarsestLevel + 1 exist or the next coarse level would have <= minSize rows; a sequence that ends before that
    depth is reached (while an axis can still be coarsened) raises ValueError, like every other malformed value.
    oddExtents: None or 'merge' (anything else: ValueError).  With 'merge' a 2 is accepted on any extent >= 4, and None /
    'full' is no longer the reference's hierarchy but a NAMED one, returned as such: every restriction takes fullFactors of
    its level (2 on every axis with extent >= 4), to the same depth rule, ending where no axis can be coarsened."""
    merge = _hip.odd_code(oddExtents) == _hip.ODD_MERGE
    full = coarsening is None or (isinstance(coarsening, str) and coarsening == "full")
    if full and not merge:
        return None
    try:
        shape = tuple(int(s) for s in problemShape)
    except TypeError:
        raise ValueError("parameters['coarsening'] needs a 2-D or 3-D parameters['problemShape'], not %r" % (problemShape,))
    if len(shape) not in (2, 3) or min(shape) < 2:
        raise ValueError("parameters['coarsening'] needs a 2-D or 3-D parameters['problemShape'] with extents >= 2, not %r" % (problemShape,))
    if full:
        used, ext = [], shape
        for k in range(int(coarsestLevel) + 1):
            entry = fullFactors(ext, oddExtents)
            coarse = tuple(s // f for s, f in zip(ext, entry))
            if all(f == 1 for f in entry) or (k >= 1 and tools.product(coarse) <= minSize):
                break
            used.append(entry)
            ext = coarse
        if not used:
            raise ValueError("parameters['oddExtents'] = 'merge': no axis of problemShape %s can be coarsened (it needs an extent >= 4)" % (shape,))
        return used
    if isinstance(coarsening, str):
        if coarsening == "auto":
            return "auto"
        raise ValueError("parameters['coarsening'] must be None, 'full', 'auto' or a sequence of factor tuples, not %r" % (coarsening,))
    try:
        given = list(coarsening)
    except TypeError:
        raise ValueError("parameters['coarsening'] must be None, 'full', 'auto' or a sequence of factor tuples, not %r" % (coarsening,))
    used = []
    ext = shape
    for k in range(int(coarsestLevel) + 1):
        if k >= len(given):
            if not any(canHalve(s, oddExtents) for s in ext) or (k >= 1 and tools.product(ext) // 2 <= minSize):
                break                               # (nothing left to coarsen, or whatever the factors minSize ends it here)
            raise ValueError("parameters['coarsening'] has %d entries but restriction %d is reached (gridLevels %d, minSize %d)"
                             % (len(given), k, int(coarsestLevel) + 1, minSize))
        entry = checkFactors(ext, given[k], oddExtents)
        coarse = tuple(s // f for s, f in zip(ext, entry))
        if k >= 1 and tools.product(coarse) <= minSize:
            break
        used.append(entry)
        ext = coarse
    if not used:
        raise ValueError("parameters['coarsening'] is empty")
    return used


def semicoarsenedLists(A_in, problemShape, coarsening, coarsestLevel, minSize, lineAxis=None, oddExtents=None):
    """restrictionList + coeffecientList with a factor of 1 or 2 per axis and restriction: returns (R, A, factors), every
    restriction built on the device (omg_restriction_ex), every Galerkin product too (omg_rap).  coarsening: 'auto' — per level
    the couplings of its operator (omg_axis_couplings) go through the rule (omg_semicoarsen_rule), which ends the hierarchy
    where no axis can be coarsened — or a sequence of factor tuples, consumed entry by entry.  The depth rule is
    restrictionList's.  lineAxis: the line smoother's axis (an index into problemShape) for the rule, or None.
    oddExtents: None or 'merge' (coarseningOf); with 'merge' coarsening may also be None / 'full'."""
    shape = tuple(int(s) for s in problemShape)
    named = coarseningOf(coarsening, shape, coarsestLevel, minSize, oddExtents)
    if named is None:
        raise ValueError("semicoarsenedLists needs coarsening 'auto' or a sequence of factor tuples; restrictionList does 'full'")
    A = [sp.csr_matrix(A_in)]
    if A[0].shape != (tools.product(shape),) * 2:
        raise ValueError("problemShape %s does not match the operator's shape %s" % (shape, A[0].shape))
    R, factors, ext = [], [], shape
    for k in range(int(coarsestLevel) + 1):
        if named == "auto":
            sums, counts, off_axis = _hip.axis_couplings(A[-1], ext)
            entry = _hip.semicoarsen_rule(ext, sums, counts, off_axis, lineAxis, level=k, oddExtents=oddExtents)
            if all(f == 1 for f in entry):
                if k == 0:
                    raise ValueError("coarsening 'auto': no axis of problemShape %s can be coarsened (it needs an %sextent >= 4)"
                                     % (shape, "" if oddExtents else "even "))
                break
            if k >= 1 and tools.product(s // f for s, f in zip(ext, entry)) <= minSize:
                break
        elif k >= len(named):
            break
        else:
            entry = named[k]
        R.append(_hip.restriction_ex(ext, entry, oddExtents))
        A.append(_hip.rap(R[-1], A[-1]))
        factors.append(entry)
        ext = tuple(s // f for s, f in zip(ext, entry))
    return R, A, factors


# ---- generators (test inputs; quirks of the reference kept) ----------------------
def poisson1Dsparse(N):
    """Sparse 1-D operator with 4 on the diagonal and -1 beside it (openmg/operators.py:191-203)."""
    return sp.csr_matrix(sp.diags([-np.ones(N - 1), 4.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1]))


def poisson1D(shape, sparse=False):
    """Dense 1-D operator is (2, -1) — not the sparse one's (4, -1) (openmg/operators.py:206-218)."""
    N = shape[0]
    if sparse:
        return poisson1Dsparse(N)
    return 2.0 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1)


def poisson2D(shape, sparse=False):
    """Dense only: -4 / +1 at offsets 1 and NX+1, bands not cut at grid-row ends
    (openmg/operators.py:221-243)."""
    if sparse:
        raise NotImplementedError("Sparse poisson for alpha>1 is not yet implemented.")
    NX, NY = shape
    N = NX * NY
    return (-4.0 * np.eye(N) + np.eye(N, k=1) + np.eye(N, k=-1)
            + np.eye(N, k=NX + 1) + np.eye(N, k=-(NX + 1)))


def poisson3D(shape, sparse=False):
    """Dense only: +1 at i+1, i+NX, i+NX*NY wherever that index is < N, mirrored; the
    reference sets -6 on the diagonal BEFORE `A += A.T`, so the stored diagonal is -12
    (openmg/operators.py:245-257; fixture gen_p3dense_*)."""
    if sparse:
        raise NotImplementedError("Sparse poisson for alpha>1 is not yet implemented.")
    NX, NY, NZ = shape
    N = NX * NY * NZ
    upper = np.eye(N, k=1) + np.eye(N, k=NX) + np.eye(N, k=NX * NY)
    upper = np.minimum(upper, 1.0)          # NX == 1 would stack two bands
    return -12.0 * np.eye(N) + upper + upper.T


def poissonnd(shape, sparse=False):
    """Dispatch on len(shape) (openmg/operators.py:260-279)."""
    if isinstance(shape, int):
        shape = (shape,)
    if len(shape) == 1:
        out = poisson1D(shape, sparse)
    elif len(shape) == 2:
        out = poisson2D(shape, sparse)
    elif len(shape) == 3:
        out = poisson3D(shape, sparse)
    else:
        raise ValueError("Only 1, 2 or 3 dimensions are allowed.")
    return sp.csr_matrix(out) if sparse else out


poisson = poissonnd


def stencil_poisson(shape):
    """Dirichlet 3/5/7-point Laplacian (2*dim on the diagonal, -1 off it), C-order numbering,
    sorted CSR with int32 indices, assembled directly (no Kronecker products, so 256^3 takes
    seconds).  NOT in the reference (its sparse 2-D/3-D generators raise NotImplementedError);
    these are BASELINE.json's synthetic inputs."""
    shape = tuple(int(s) for s in shape)
    dim = len(shape)
    N = int(np.prod(shape))
    strides = [int(np.prod(shape[d + 1:])) for d in range(dim)]
    coords = np.unravel_index(np.arange(N, dtype=np.int64), shape)
    # neighbours in ascending column order: -stride_0, ..., -stride_{dim-1}, 0, +stride_{dim-1}, ..., +stride_0
    offsets, valid = [], []
    for d in range(dim):
        offsets.append(-strides[d]); valid.append(coords[d] > 0)
    offsets.append(0); valid.append(np.ones(N, dtype=bool))
    for d in reversed(range(dim)):
        offsets.append(strides[d]); valid.append(coords[d] < shape[d] - 1)
    counts = np.zeros(N, dtype=np.int64)
    for v in valid:
        counts += v
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz, dtype=np.float64)
    cursor = indptr[:-1].copy()
    rows = np.arange(N, dtype=np.int64)
    for off, v in zip(offsets, valid):
        pos = cursor[v]
        indices[pos] = (rows[v] + off).astype(np.int32)
        data[pos] = 2.0 * dim if off == 0 else -1.0
        cursor += v
    out = sp.csr_matrix((data, indices, indptr.astype(np.int32)), shape=(N, N))
    out.has_sorted_indices = True
    return out


def _q1_element_stiffness():
    """8 x 8 stiffness matrix of the trilinear (Q1) element on the unit cube for -div(grad u),
    local nodes numbered (dz, dy, dx) in C order; 2-point Gauss quadrature is exact here."""
    g = np.array([0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)])
    corners = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    K = np.zeros((8, 8))
    for z in g:
        for y in g:
            for x in g:
                grads = []
                for (cz, cy, cx) in corners:
                    fz, fy, fx = (z if cz else 1 - z), (y if cy else 1 - y), (x if cx else 1 - x)
                    sz, sy, sx = (1.0 if cz else -1.0), (1.0 if cy else -1.0), (1.0 if cx else -1.0)
                    grads.append((sz * fy * fx, fz * sy * fx, fz * fy * sx))
                G = np.array(grads)
                K += G @ G.T / 8.0
    return K, corners


def stencil7_variable(shape, seed=2024):
    """7-point variable-coefficient operator (NOT in the reference; the ordinary real input of mgSolve): cell-centred
    finite volumes of -div(kappa grad u) on a box of `shape` cells, homogeneous Dirichlet boundary, kappa =
    exp(U(-1, 1) ln 10) per cell (two decades, as BASELINE configs[4] draws it) from default_rng(seed); the coupling of two
    cells is the harmonic mean of their coefficients.  Symmetric (bit for bit) positive definite.  C-order numbering,
    sorted CSR with int32 indices."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3:
        raise ValueError("stencil7_variable needs a 3-D shape")
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    kap = np.exp(rng.uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(10.0))     # cells incl. one boundary layer

    def face(a, b):
        return 2.0 * a * b / (a + b)
    c = kap[1:-1, 1:-1, 1:-1]
    w = {(0, 0, -1): face(c, kap[1:-1, 1:-1, :-2]), (0, 0, 1): face(c, kap[1:-1, 1:-1, 2:]),
         (0, -1, 0): face(c, kap[1:-1, :-2, 1:-1]), (0, 1, 0): face(c, kap[1:-1, 2:, 1:-1]),
         (-1, 0, 0): face(c, kap[:-2, 1:-1, 1:-1]), (1, 0, 0): face(c, kap[2:, 1:-1, 1:-1])}
    diag = ((((w[(-1, 0, 0)] + w[(0, -1, 0)]) + w[(0, 0, -1)]) + w[(0, 0, 1)]) + w[(0, 1, 0)]) + w[(1, 0, 0)]
    n = nx * ny * nz
    idx = np.arange(n, dtype=np.int64).reshape(nz, ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [diag.ravel()]
    for (dz, dy, dx), ww in w.items():
        sel = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
        rows.append(idx[sel].ravel())
        cols.append((idx[sel] + (dz * ny + dy) * nx + dx).ravel())
        vals.append(-ww[sel].ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


WALLS = ("dirichlet", "neumann")       # OMG_WALL_DIRICHLET, OMG_WALL_NEUMANN
WALL_CODES = {"dirichlet": 0, "neumann": 1, "periodic": 2}     # ... and OMG_WALL_PERIODIC: both walls of an axis or neither


def kappa_arguments(kappa_shape, walls=None, sigma=None, scale=(1.0, 1.0, 1.0)):
    """What stencil7_kappa, _hip.kappa_assemble and Solver.from_kappa check of their arguments besides the fields' values:
    (problemShape, wall codes -z +z -y +y -x +x, scale z y x); ValueError for a kappa that is not 3-D with a ghost layer,
    an unknown wall, 'periodic' on one wall of an axis only or on an axis of extent 1 or 2, a scale factor that is not
    finite and > 0, a scalar sigma that is not finite and >= 0, a sigma field of another shape than problemShape (a field's
    values are the caller's to check: on the host here, on the device by the kernel that reads them)."""
    kappa_shape = tuple(int(s) for s in kappa_shape)
    if len(kappa_shape) != 3 or min(kappa_shape) < 3:
        raise ValueError("kappa must be 3-D with one ghost layer, shape (nz + 2, ny + 2, nx + 2), not %r" % (kappa_shape,))
    shape = tuple(s - 2 for s in kappa_shape)
    walls = ("dirichlet",) * 6 if walls is None else tuple(walls)
    if len(walls) != 6 or any(not isinstance(w, str) or w not in WALL_CODES for w in walls):
        raise ValueError("walls must be six of 'dirichlet' / 'neumann' / 'periodic' in the order -z, +z, -y, +y, -x, +x, not %r" % (walls,))
    for axis, name in enumerate("zyx"):
        lo, hi = walls[2 * axis] == "periodic", walls[2 * axis + 1] == "periodic"
        if lo != hi:
            raise ValueError("walls: 'periodic' must be given for both walls of an axis, not for one wall of %s alone: %r" % (name, walls))
        if lo and shape[axis] < 3:
            raise ValueError("walls: a periodic axis needs an extent >= 3 (the cell and its two neighbours are three columns): "
                             "%s has %d" % (name, shape[axis]))
    try:
        scale = tuple(float(f) for f in scale)
    except (TypeError, ValueError):
        raise ValueError("scale must be three numbers (z, y, x), not %r" % (scale,))
    if len(scale) != 3 or any(not (np.isfinite(f) and f > 0.0) for f in scale):
        raise ValueError("scale must be three finite factors > 0 (z, y, x), not %r" % (scale,))
    if sigma is not None and np.ndim(sigma) == 0 and not hasattr(sigma, "__cuda_array_interface__"):
        try:
            value = float(sigma)
        except (TypeError, ValueError):
            raise ValueError("sigma must be None, a number >= 0 or an array of problemShape, not %r" % (sigma,))
        if not (np.isfinite(value) and value >= 0.0):
            raise ValueError("sigma must be finite and >= 0, not %r" % (sigma,))
    elif sigma is not None:
        s_shape = tuple(int(s) for s in (sigma.__cuda_array_interface__["shape"] if hasattr(sigma, "__cuda_array_interface__")
                                          and not isinstance(sigma, np.ndarray) else np.shape(sigma)))
        if s_shape != shape:
            raise ValueError("a sigma field must have problemShape %r, not %r" % (shape, s_shape))
    return shape, tuple(WALL_CODES[w] for w in walls), scale


def periodic_axes(walls):
    """Per axis (z, y, x) whether `walls` — six names or six codes, checked — makes it periodic."""
    return tuple(walls[2 * axis] in ("periodic", WALL_CODES["periodic"]) for axis in range(3))


def spacing_arguments(shape, spacing):
    """The cell widths of a tensor-product grid as stencil7_kappa, _hip.KappaArgs and Solver.from_kappa take them:
    spacing = (hz, hy, hx), three 1-D sequences of nz + 2, ny + 2 and nx + 2 widths — the cells' along that axis and one
    ghost entry at each end, like kappa's ghost layer.  Returns three contiguous float64 arrays.  ValueError for another
    count of sequences, other lengths, a value that is not finite, an interior width <= 0, a ghost width < 0, and for a
    device array (the widths are host arrays: the library checks them before any launch)."""
    shape = tuple(int(s) for s in shape)
    if hasattr(spacing, "__cuda_array_interface__") and not isinstance(spacing, np.ndarray):
        raise ValueError("spacing must be host arrays, not a device array: pass NumPy arrays or sequences")
    try:
        spacing = tuple(spacing)
    except TypeError:
        raise ValueError("spacing must be three sequences of cell widths (hz, hy, hx), not %r" % (spacing,))
    if len(spacing) != len(shape):
        raise ValueError("spacing must be %d sequences of cell widths, one per axis, not %d" % (len(shape), len(spacing)))
    out = []
    for name, extent, widths in zip("zyx"[-len(shape):], shape, spacing):
        if hasattr(widths, "__cuda_array_interface__") and not isinstance(widths, np.ndarray):
            raise ValueError("spacing: the widths along %s are a device array: pass host arrays (NumPy arrays or sequences)" % name)
        try:
            h = np.ascontiguousarray(widths, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("spacing: the widths along %s are not numbers" % name)
        if h.ndim != 1 or h.size != extent + 2:
            raise ValueError("spacing: the widths along %s must be a 1-D sequence of %d entries (the %d cells and one ghost "
                             "entry at each end), not shape %r" % (name, extent + 2, extent, h.shape))
        if not np.isfinite(h).all():
            raise ValueError("spacing: the widths along %s must be finite" % name)
        if not (h[1:-1] > 0.0).all():
            raise ValueError("spacing: the width of every cell along %s must be > 0" % name)
        if h[0] < 0.0 or h[-1] < 0.0:
            raise ValueError("spacing: the ghost widths along %s must be >= 0" % name)
        out.append(h)
    return tuple(out)


def cell_volumes(spacing):
    """The cell volumes (hz[k] hy[j]) hx[i] of a tensor-product grid as an (nz, ny, nx) float64 array, with the rounding
    stencil7_kappa(..., spacing=spacing) uses for sigma: that operator is the volume-integrated one, so its right-hand
    side is b = f * cell_volumes(spacing).  spacing as spacing_arguments takes it (the ghost entries are not used)."""
    try:
        shape = tuple(len(h) - 2 for h in spacing)
    except TypeError:
        raise ValueError("spacing must be three sequences of cell widths (hz, hy, hx), not %r" % (spacing,))
    if len(shape) != 3:
        raise ValueError("spacing must be three sequences of cell widths (hz, hy, hx), not %d" % len(shape))
    hz, hy, hx = spacing_arguments(shape, spacing)
    return (hz[1:-1, None, None] * hy[None, 1:-1, None]) * hx[None, None, 1:-1]


def unit_scale(scale):
    """Whether scale is the default (1, 1, 1): the only one that goes with spacing."""
    try:
        return tuple(float(f) for f in scale) == (1.0, 1.0, 1.0)
    except (TypeError, ValueError):
        return False


def stencil7_kappa(kappa, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), spacing=None, _terms=None):
    """7-point operator of -div(kappa grad u) + sigma u from a coefficient field (NOT in the reference; the definition the
    device assembly — _hip.kappa_assemble, Solver.from_kappa — is pinned to bit for bit): cell-centred finite volumes on a
    box of (nz, ny, nx) cells.  kappa: float64 (nz + 2, ny + 2, nx + 2), the cells and one ghost layer, as
    stencil7_variable draws it.  walls: six of 'dirichlet' (default) / 'neumann' / 'periodic' in the order -z, +z, -y, +y,
    -x, +x, 'periodic' for both walls of an axis or neither.
    sigma: None, a scalar or an array of problemShape, >= 0.  scale: one factor per axis (z, y, x), e.g. dt / h_axis^2.

    Every operation is rounded once in double: face(a, b) = ((2 a) b) / (a + b), c = face * scale[axis], the off-diagonal
    entry is -c, the diagonal (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K), then + sigma.  The face at a Dirichlet wall takes
    the ghost cell's kappa and enters the diagonal only; at a Neumann wall it contributes +0.0.  With the defaults and
    stencil7_variable's kappa this is stencil7_variable's matrix bit for bit.  C-order numbering, sorted CSR, int32 indices.

    spacing = (hz, hy, hx) (spacing_arguments; in place of scale): the cell widths of a stretched tensor-product grid, one
    ghost entry at each end of every axis.  The operator is then the volume-integrated one — symmetric, the right-hand side
    is f * cell_volumes(spacing).  With a, da the cell's own kappa and width along the face's axis and b, db the neighbour's:
    c = (((2 a) b) / (da b + db a)) * area[axis], area_z = hy[j] hx[i], area_y = hz[k] hx[i], area_x = hz[k] hy[j]; the
    diagonal is the same sum, then + sigma * ((hz[k] hy[j]) hx[i]).  A Dirichlet wall face takes the ghost cell's kappa and
    the ghost width: 0 puts the boundary value on the wall face itself, the boundary cell's width at the mirrored cell centre
    (what the operator without spacing does); a Neumann wall face reads neither.  Equal power-of-two widths h along every
    axis give stencil7_kappa(kappa, walls, sigma V, scale=(V / hz^2, V / hy^2, V / hx^2)), V = hz hy hx, bit for bit.

    A periodic axis (extent >= 3): every row holds both neighbours along it, the one across the seam being the cell at the
    other end of the line; its face is the inner-face expression — own a, that cell's b (and width db) —, so the matrix
    stays symmetric bit for bit; the diagonal is the same sum in the same order wherever the wrapped column lands in the
    row.  The ghost layer of kappa and the ghost entries of spacing along a periodic axis are not read (kappa's may hold
    anything; spacing_arguments checks the widths' as ever).  nnz = 7 n - 2 sum of n / extent over the axes that are not periodic.

    ValueError: kappa of another rank or without cells, not finite or <= 0 in a cell or in a ghost cell behind a
    Dirichlet wall; sigma negative or not finite; scale not finite or <= 0; an unknown wall, 'periodic' on one wall of
    an axis alone or on an extent below 3; what spacing_arguments refuses; spacing together with a scale other than (1, 1, 1)."""
    kap = np.asarray(kappa)
    if kap.dtype != np.float64:
        raise ValueError("kappa must be float64, not %s" % kap.dtype)
    shape, wall, scale = kappa_arguments(kap.shape, walls, sigma, scale)
    nz, ny, nx = shape
    if spacing is not None:
        if not unit_scale(scale):
            raise ValueError("spacing and scale exclude each other: the widths carry every factor")
        hz, hy, hx = spacing_arguments(shape, spacing)
        along = (lambda h: h[:, None, None], lambda h: h[None, :, None], lambda h: h[None, None, :])   # broadcast over the grid
        H = (hz, hy, hx)
        own = [along[a](H[a][1:-1]) for a in range(3)]
        area = (own[1] * own[2], own[0] * own[2], own[0] * own[1])
    c = kap[1:-1, 1:-1, 1:-1]
    # (dz, dy, dx) -> (neighbour's kappa, axis, wall); in the order of the diagonal's sum
    dirs = [((-1, 0, 0), kap[:-2, 1:-1, 1:-1], 0, 0), ((0, -1, 0), kap[1:-1, :-2, 1:-1], 1, 2), ((0, 0, -1), kap[1:-1, 1:-1, :-2], 2, 4),
            ((0, 0, 1), kap[1:-1, 1:-1, 2:], 2, 5), ((0, 1, 0), kap[1:-1, 2:, 1:-1], 1, 3), ((1, 0, 0), kap[2:, 1:-1, 1:-1], 0, 1)]
    periodic = periodic_axes(wall)
    # (a periodic axis: the neighbour is the cell one step round the line; no ghost cell is looked at)
    dirs = [(d, np.roll(c, -sum(d), axis) if periodic[axis] else nb, axis, f) for d, nb, axis, f in dirs]

    def ghost(d, a):                                      # the ghost cells a face of the box reads: one layer of `a`
        sel = [slice(None)] * 3
        sel[[abs(v) for v in d].index(1)] = 0 if sum(d) < 0 else -1
        return a[tuple(sel)]
    checked = [c] + [ghost(d, nb) for d, nb, _, f in dirs if wall[f] == 0]
    if any(not (np.isfinite(a).all() and (a > 0.0).all()) for a in checked):
        raise ValueError("kappa must be finite and > 0 in every cell and in the ghost cells behind Dirichlet walls")
    sig = None
    if sigma is not None:
        sig = np.asarray(sigma, dtype=np.float64)
        if not (np.isfinite(sig).all() and (sig >= 0.0).all()):
            raise ValueError("sigma must be finite and >= 0")
    w = {}
    with np.errstate(all="ignore"):                       # (ghost cells behind Neumann walls hold anything: their faces are replaced)
        for d, nb, axis, f in dirs:
            if spacing is not None:
                other = along[axis](H[axis][1 + sum(d):H[axis].size - 1 + sum(d)])     # the neighbour's width
                if periodic[axis]:
                    other = along[axis](np.roll(H[axis][1:-1], -sum(d)))
                face = ((2.0 * c) * nb) / (own[axis] * nb + other * c) * area[axis]
            else:
                face = ((2.0 * c) * nb) / (c + nb) * scale[axis]
            if wall[f] == 1:
                face = face.copy()
                ghost(d, face)[...] = 0.0
            w[d] = face
    diag = ((((w[(-1, 0, 0)] + w[(0, -1, 0)]) + w[(0, 0, -1)]) + w[(0, 0, 1)]) + w[(0, 1, 0)]) + w[(1, 0, 0)]
    if sig is not None:
        diag = diag + (sig * ((own[0] * own[1]) * own[2]) if spacing is not None else sig)
    if _terms is not None:                                # (face_coefficients_kappa: the six face terms as they entered the diagonal)
        _terms.update(w)
    return _assemble7(shape, w, diag, periodic)


def _assemble7(shape, w, diag, periodic):
    """The sorted CSR of a 7-point operator from its per-cell face terms w[(dz, dy, dx)] (problemShape arrays; the
    off-diagonal entry is -w) and its diagonal: an in-grid neighbour per face, along a periodic axis every cell's."""
    nz, ny, nx = shape
    n = nx * ny * nz
    idx = np.arange(n, dtype=np.int64).reshape(nz, ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [diag.ravel()]
    for (dz, dy, dx), ww in w.items():
        axis = (dz, dy, dx).index(dz + dy + dx)
        if periodic[axis]:                                # (every cell of the line has this neighbour: the seam's is the other end)
            rows.append(idx.ravel())
            cols.append(np.roll(idx, -(dz + dy + dx), axis).ravel())
            vals.append(-ww.ravel())
            continue
        sel = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
        rows.append(idx[sel].ravel())
        cols.append((idx[sel] + (dz * ny + dy) * nx + dx).ravel())
        vals.append(-ww[sel].ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


WALL_FACES = ((1, 2), (1, 2), (0, 2), (0, 2), (0, 1), (0, 1))     # per wall: the two axes (of z, y, x) its faces run over


def wall_values_arguments(shape, wall, values):
    """The boundary data of rhs_kappa, _hip.kappa_rhs and Solver.rhs, checked: values None, or six entries in the order of
    the walls (-z, +z, -y, +y, -x, +x), each None, a scalar or a 2-D array over that wall's faces — (ny, nx) for the z
    walls, (nz, nx) for the y walls, (nz, ny) for the x walls; shape = problemShape, wall = the six codes kappa_arguments
    returned.  Returns a tuple of six: None, a float, or the array as it came (a device array's shape is read off its
    interface; its dtype is the caller's to get right, checked where its address is taken).  ValueError for another
    count, a value on a periodic wall, another shape, an entry that is neither."""
    if values is None:
        return (None,) * 6
    try:
        values = tuple(values)
    except TypeError:
        raise ValueError("values must be None or six entries in the order -z, +z, -y, +y, -x, +x, not %r" % (values,))
    if len(values) != 6:
        raise ValueError("values must be None or six entries in the order -z, +z, -y, +y, -x, +x, not %d" % len(values))
    out = []
    for f, v in enumerate(values):
        name = ("-z", "+z", "-y", "+y", "-x", "+x")[f]
        if v is None:
            out.append(None)
            continue
        if wall[f] == WALL_CODES["periodic"]:
            raise ValueError("values: the wall %s is periodic and takes None only" % name)
        on_device = hasattr(v, "__cuda_array_interface__") and not isinstance(v, np.ndarray)
        if not on_device and np.ndim(v) == 0:
            try:
                out.append(float(v))
            except (TypeError, ValueError):
                raise ValueError("values: the entry of wall %s must be None, a number or a 2-D array, not %r" % (name, v))
            continue
        v_shape = tuple(int(s) for s in (v.__cuda_array_interface__["shape"] if on_device else np.shape(v)))
        faces = tuple(shape[a] for a in WALL_FACES[f])
        if v_shape != faces:
            raise ValueError("values: the field of wall %s must have that wall's faces %r, not %r" % (name, faces, v_shape))
        out.append(v)
    return tuple(out)


def source_argument(shape, f):
    """The source f of rhs_kappa and its device twins, checked: None, a float, or the array as it came; ValueError for an
    array of another shape than problemShape or an entry that is neither."""
    if f is None:
        return None
    on_device = hasattr(f, "__cuda_array_interface__") and not isinstance(f, np.ndarray)
    if not on_device and np.ndim(f) == 0:
        try:
            return float(f)
        except (TypeError, ValueError):
            raise ValueError("f must be None, a number or an array of problemShape, not %r" % (f,))
    f_shape = tuple(int(s) for s in (f.__cuda_array_interface__["shape"] if on_device else np.shape(f)))
    if f_shape != tuple(shape):
        raise ValueError("a source field f must have problemShape %r, not %r" % (tuple(shape), f_shape))
    return f


def rhs_kappa(kappa, f=None, walls=None, values=None, scale=(1.0, 1.0, 1.0), spacing=None):
    """The right-hand side b that goes with stencil7_kappa(kappa, walls, sigma, scale, spacing) (NOT in the reference; the
    definition the device kernel — _hip.kappa_rhs, Solver.rhs — is pinned to bit for bit): a source per cell and
    inhomogeneous boundary data, as a float64 array of problemShape.  sigma plays no part.  kappa, walls, scale, spacing:
    as stencil7_kappa takes them.  f: the source per cell — None (zero), a scalar or an array of problemShape.  values:
    None, or six entries in the order of walls (-z, +z, -y, +y, -x, +x), each None, a scalar or a 2-D float64 array over
    that wall's faces ((ny, nx) for z, (nz, nx) for y, (nz, ny) for x walls); a periodic wall takes None only.

    What a wall's value means:
      - a Dirichlet wall: the boundary value g, located where the operator puts it — with spacing, where the ghost width
        says (0: on the wall face; the boundary cell's width: at the mirrored ghost-cell centre), without spacing at the
        mirrored ghost-cell centre.  The cell gets c_wall * g, c_wall being the very face coefficient stencil7_kappa
        added to that cell's diagonal for this wall (the same expression with the ghost cell's kappa and width, the same
        rounding, times scale[axis] or the spaced area[axis]).
      - a Neumann wall: the OUTWARD flux q = kappa du/dn.  With spacing the cell gets q * area[axis].  WITHOUT spacing the
        library does not know the cell width h: the value is then q TIMES THE CELL WIDTH ALONG THAT AXIS, q h, and the
        cell gets value * scale[axis] (with scale = 1 / h_axis^2 that is q / h, the flux per cell volume).

    Every operation is rounded once in double.  The volume term is f * ((hz[k] hy[j]) hx[i]) (cell_volumes' rounding)
    with spacing, f itself without, +0.0 for f = None, and
        b = ((((((volume term + t-K) + t-J) + t-I) + t+I) + t+J) + t+K),
    the order of the diagonal's sum; an in-grid face and a wall without a value contribute +0.0.

    Only the cells at a Dirichlet wall WITH a value read kappa (their own and the ghost cell's) and the ghost width; ghost
    cells behind Neumann walls, periodic walls and Dirichlet walls without a value are never read and may hold anything.
    kappa's values are not checked here: stencil7_kappa (Solver.from_kappa, update_kappa) checked the same field.

    ValueError: what kappa_arguments and spacing_arguments refuse, spacing together with a scale other than (1, 1, 1), an f
    of another shape, values of another count, a value on a periodic wall, a value field of another shape than its wall."""
    kap = np.asarray(kappa)
    if kap.dtype != np.float64:
        raise ValueError("kappa must be float64, not %s" % kap.dtype)
    shape, wall, scale = kappa_arguments(kap.shape, walls, None, scale)
    f = source_argument(shape, f)
    values = wall_values_arguments(shape, wall, values)
    H = None
    if spacing is not None:
        if not unit_scale(scale):
            raise ValueError("spacing and scale exclude each other: the widths carry every factor")
        H = spacing_arguments(shape, spacing)
        own = (H[0][1:-1, None, None], H[1][None, 1:-1, None], H[2][None, None, 1:-1])
        area = (own[1] * own[2], own[0] * own[2], own[0] * own[1])
    if f is None:
        volume = np.zeros(shape)
    else:
        source = np.broadcast_to(np.asarray(f, dtype=np.float64), shape)
        volume = source * ((own[0] * own[1]) * own[2]) if H is not None else source.copy()
    c = kap[1:-1, 1:-1, 1:-1]
    terms = {}
    for face in range(6):
        axis, hi = face // 2, face % 2
        t = np.zeros(shape)
        terms[face] = t
        if values[face] is None:
            continue
        g = np.asarray(values[face], dtype=np.float64)
        layer = [slice(None)] * 3
        layer[axis] = -1 if hi else 0                      # the cells at this wall ...
        layer = tuple(layer)
        behind = list(layer)
        behind[axis] = -1 if hi else 0                     # ... and, in the padded field, the ghost cells behind them
        behind = tuple(slice(1, -1) if isinstance(s, slice) else s for s in behind)
        if wall[face] == WALL_CODES["neumann"]:
            t[layer] = g * (np.broadcast_to(area[axis], shape)[layer] if H is not None else scale[axis])
            continue
        a, b = c[layer], kap[behind]
        if H is not None:
            da = np.broadcast_to(own[axis], shape)[layer]
            db = H[axis][-1 if hi else 0]
            coeff = ((2.0 * a) * b) / (da * b + db * a) * np.broadcast_to(area[axis], shape)[layer]
        else:
            coeff = ((2.0 * a) * b) / (a + b) * scale[axis]
        t[layer] = coeff * g
    # faces in the order of the diagonal's sum: -K, -J, -I, +I, +J, +K = walls 0, 2, 4, 5, 3, 1
    return (((((volume + terms[0]) + terms[2]) + terms[4]) + terms[5]) + terms[3]) + terms[1]


def face_shapes(shape):
    """The shapes of the three face arrays (Fz, Fy, Fx) of a grid of problemShape (nz, ny, nx): one more along the own axis."""
    shape = tuple(int(s) for s in shape)
    return tuple(tuple(s + (1 if a == axis else 0) for a, s in enumerate(shape)) for axis in range(3))


def solution_argument(shape, u):
    """The solution u of flux_kappa and its device twins, checked: an array of problemShape or of n entries ((n,) or (n, 1),
    as solve returns it), returned as it came; ValueError for anything else."""
    on_device = hasattr(u, "__cuda_array_interface__") and not isinstance(u, np.ndarray)
    if u is None or (not on_device and np.ndim(u) == 0):
        raise ValueError("u must be an array of problemShape %r or of its n entries, not %r" % (tuple(shape), u))
    u_shape = tuple(int(s) for s in (u.__cuda_array_interface__["shape"] if on_device else np.shape(u)))
    n = int(np.prod(shape))
    if u_shape != tuple(shape) and u_shape != (n,) and u_shape != (n, 1):
        raise ValueError("u must have problemShape %r or its %d entries, not shape %r" % (tuple(shape), n, u_shape))
    return u


def flux_kappa(kappa, u, walls=None, values=None, scale=(1.0, 1.0, 1.0), spacing=None):
    """The face fluxes of a solution u under stencil7_kappa(kappa, walls, sigma, scale, spacing) with the boundary data of
    rhs_kappa(kappa, None, walls, values, scale, spacing) (NOT in the reference; the definition the device kernel —
    _hip.kappa_flux, Solver.fluxes — is pinned to bit for bit).  Returns (Fz, Fy, Fx), float64 arrays of shapes
    (nz + 1, ny, nx), (nz, ny + 1, nx), (nz, ny, nx + 1): F is the flux of -kappa grad u ALONG THE +AXIS DIRECTION through
    each face, times the operator's own factor — scale[axis] without spacing, the face area with spacing —, so that the
    differences of F are the operator's rows: for every u
        divergence_faces(*flux_kappa(kappa, u, walls, values, ...)) (+ sigma u; with spacing sigma cell_volumes u)
            = stencil7_kappa(...) @ u - rhs_kappa(kappa, None, walls, values, ...)
    up to rounding.  kappa, walls, scale, spacing, values: as stencil7_kappa and rhs_kappa take them; sigma plays no part.
    u: an array of problemShape or of n entries.

    Face m of an axis of extent e lies between cell m - 1 ("lo") and cell m ("hi").
      - an in-grid face, m = 1 .. e - 1: F = c * (u_lo - u_hi), c the face coefficient as the lo cell computes its + face
        in stencil7_kappa (a = kappa_lo, b = kappa_hi, da, db their widths, area[axis]): the bits of -A[lo, hi] = -A[hi, lo].
      - a periodic axis: faces 0 and e are the same face and hold the same bits, c * (u_{e-1} - u_0) with the inner-face
        expression of a = kappa_{e-1}, b = kappa_0 and their widths; no ghost kappa or ghost width is read.
      - a Dirichlet wall: F[0] = c_wall * (g - u_0), F[e] = c_wall * (u_{e-1} - g); c_wall is rhs_kappa's (own kappa, ghost
        kappa, own width, ghost width, the same rounding), g the wall's value, +0.0 where it has none.
      - a Neumann wall: +0.0 where it has no value, and nothing is read.  With a value v under rhs_kappa's convention (the
        OUTWARD flux q = kappa du/dn; WITHOUT spacing q times the cell width along the axis) t = v * area[axis] with
        spacing, v * scale[axis] without, and F[0] = t, F[e] = -t: the outward flux of -kappa grad u is -q.
    Every operation is rounded once in double: one subtraction and one multiplication per face, the coefficient as the
    operator rounds it.  The ghost cells of kappa behind Neumann and periodic walls are never read and may hold anything;
    behind a Dirichlet wall they are always read, with or without a value.  kappa's values are not checked, as in rhs_kappa.

    ValueError: what rhs_kappa refuses of kappa, walls, values, scale and spacing; a u of another shape."""
    kap = np.asarray(kappa)
    if kap.dtype != np.float64:
        raise ValueError("kappa must be float64, not %s" % kap.dtype)
    shape, wall, scale = kappa_arguments(kap.shape, walls, None, scale)
    values = wall_values_arguments(shape, wall, values)
    H = None
    if spacing is not None:
        if not unit_scale(scale):
            raise ValueError("spacing and scale exclude each other: the widths carry every factor")
        H = spacing_arguments(shape, spacing)
        own = (H[0][1:-1, None, None], H[1][None, 1:-1, None], H[2][None, None, 1:-1])
        area = (own[1] * own[2], own[0] * own[2], own[0] * own[1])
    u = np.asarray(solution_argument(shape, u), dtype=np.float64).reshape(shape)
    c = kap[1:-1, 1:-1, 1:-1]
    periodic = periodic_axes(wall)
    out = []
    for axis, faces in enumerate(face_shapes(shape)):
        e = shape[axis]

        def at(m, a=None):                                 # layer m (or layers m) along the axis, of `a` broadcast over the grid
            sel = [slice(None)] * 3
            sel[axis] = m
            return np.broadcast_to(c if a is None else a, shape)[tuple(sel)]

        def coefficient(a, b, da, db, lo):                 # the face between kappa a and b; area of the cells in layers `lo`
            if H is not None:
                return ((2.0 * a) * b) / (da * b + db * a) * at(lo, area[axis])
            return ((2.0 * a) * b) / (a + b) * scale[axis]
        F = np.zeros(faces)
        inner = [slice(None)] * 3
        inner[axis] = slice(1, e)
        lo, hi = slice(0, e - 1), slice(1, e)
        widths = own[axis] if H is not None else None
        F[tuple(inner)] = coefficient(at(lo), at(hi), at(lo, widths), at(hi, widths), lo) * (at(lo, u) - at(hi, u))
        first, last = [slice(None)] * 3, [slice(None)] * 3
        first[axis], last[axis] = 0, e
        first, last = tuple(first), tuple(last)
        if periodic[axis]:
            seam = coefficient(at(e - 1), at(0), at(e - 1, widths), at(0, widths), e - 1) * (at(e - 1, u) - at(0, u))
            F[first] = seam
            F[last] = seam
            out.append(F)
            continue
        for side, place, cell in ((0, first, 0), (1, last, e - 1)):
            w = 2 * axis + side
            if wall[w] == WALL_CODES["neumann"]:
                if values[w] is not None:
                    t = np.asarray(values[w], dtype=np.float64) * (at(cell, area[axis]) if H is not None else scale[axis])
                    F[place] = -t if side else t
                continue
            behind = [slice(1, -1)] * 3
            behind[axis] = -1 if side else 0               # in the padded field: the ghost cells behind the wall's cells
            g = 0.0 if values[w] is None else np.asarray(values[w], dtype=np.float64)
            c_wall = coefficient(at(cell), kap[tuple(behind)], at(cell, widths), H[axis][-1 if side else 0] if H is not None else None, cell)
            F[place] = c_wall * (at(cell, u) - g if side else g - at(cell, u))
        out.append(F)
    return tuple(out)


def divergence_faces(Fz, Fy, Fx):
    """The cell balance of three face arrays, ((Fz[k+1] - Fz[k]) + (Fy[j+1] - Fy[j])) + (Fx[i+1] - Fx[i]) in that order, as
    a float64 array of problemShape (the definition _hip.face_divergence and Solver.divergence are pinned to bit for bit).
    ValueError for shapes that are not the three face shapes (nz + 1, ny, nx), (nz, ny + 1, nx), (nz, ny, nx + 1) of one grid."""
    F = tuple(np.asarray(a, dtype=np.float64) for a in (Fz, Fy, Fx))
    grid_of_faces(tuple(a.shape for a in F))
    return ((F[0][1:] - F[0][:-1]) + (F[1][:, 1:] - F[1][:, :-1])) + (F[2][:, :, 1:] - F[2][:, :, :-1])


def grid_of_faces(shapes):
    """problemShape of the grid whose face shapes (Fz, Fy, Fx) these three are; ValueError if they are not one grid's."""
    shapes = tuple(tuple(int(s) for s in sh) for sh in shapes)
    if len(shapes) == 3 and len(shapes[0]) == 3 and shapes[0][0] >= 2:
        shape = (shapes[0][0] - 1,) + shapes[0][1:]
        if min(shape) >= 1 and shapes == face_shapes(shape):
            return shape
    raise ValueError("the face arrays must have the shapes (nz + 1, ny, nx), (nz, ny + 1, nx), (nz, ny, nx + 1) of one grid, not %r" % (shapes,))


def faces_arguments(shapes, walls=None, sigma=None):
    """What stencil7_faces, _hip.FaceArgs and Solver.from_faces check of their arguments besides the arrays' values:
    (problemShape, wall codes -z +z -y +y -x +x) from the shapes of the three coefficient arrays (Cz, Cy, Cx); ValueError
    for shapes that are not one grid's face shapes and for what kappa_arguments refuses of walls and sigma."""
    try:
        shape = grid_of_faces(shapes)
    except TypeError:
        raise ValueError("faces must be three coefficient arrays (Cz, Cy, Cx) in the face shapes of one grid")
    shape, wall, _ = kappa_arguments(tuple(s + 2 for s in shape), walls, sigma)
    return shape, wall


def _host_faces(faces):
    """(Cz, Cy, Cx) as float64 NumPy arrays, problemShape; ValueError for another count, dtype or shapes."""
    try:
        faces = tuple(faces)
    except TypeError:
        raise ValueError("faces must be three coefficient arrays (Cz, Cy, Cx), not %r" % (faces,))
    if len(faces) != 3:
        raise ValueError("faces must be three coefficient arrays (Cz, Cy, Cx), not %d" % len(faces))
    faces = tuple(np.asarray(a) for a in faces)
    for name, a in zip(("Cz", "Cy", "Cx"), faces):
        if a.dtype != np.float64:
            raise ValueError("the face coefficients %s must be float64, not %s" % (name, a.dtype))
    return faces


def _face_layer(axis, m):
    sel = [slice(None)] * 3
    sel[axis] = m
    return tuple(sel)


def stencil7_faces(faces, walls=None, sigma=None):
    """7-point operator from one coefficient per FACE (NOT in the reference; the definition the device assembly —
    _hip.faces_assemble, Solver.from_faces — is pinned to bit for bit): faces = (Cz, Cy, Cx), float64 arrays of the shapes
    face_shapes(problemShape) — (nz + 1, ny, nx), (nz, ny + 1, nx), (nz, ny, nx + 1), the arrays flux_kappa writes and
    divergence_faces reads.  Along an axis of extent e, face m lies between cell m - 1 and cell m.  The coefficients carry
    every factor (the mean of the medium, the face area over the distance, the time step): there is no scale and no spacing.
      - an in-grid face, m = 1 .. e - 1: A[lo, hi] = A[hi, lo] = -C[m].
      - a Dirichlet wall: C[0] and C[e] enter the diagonal of the cell at the wall only.
      - a Neumann wall: its face contributes +0.0; its entry of C is never read and may hold anything, NaN too.
      - a periodic axis (both walls, extent >= 3): the seam's coefficient is C[0]; C[e] is never read (flux_kappa writes the
        same bits to both, so its output can be fed back as it is).
    The diagonal is (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K), then + sigma, every operation rounded once in double; sigma:
    None, a scalar or an array of problemShape, >= 0, with no volume factor.  C-order numbering, sorted CSR with int32
    indices; the pattern is stencil7_kappa's for the same walls.  walls as stencil7_kappa takes them.
    stencil7_faces(face_coefficients_kappa(kappa, walls, scale, spacing), walls, sigma) is stencil7_kappa(kappa, walls, sigma,
    scale, spacing) bit for bit (with spacing: sigma * cell_volumes(spacing) in the former).

    ValueError: three arrays that are not one grid's face shapes or not float64; what kappa_arguments refuses of the walls; a
    coefficient on a face that is read which is not finite and > 0 (zero — a blocked face — included); a sigma that is not
    finite and >= 0."""
    F = _host_faces(faces)
    shape, wall = faces_arguments(tuple(a.shape for a in F), walls, sigma)
    periodic = periodic_axes(wall)
    w = {}
    for axis in range(3):
        e, C = shape[axis], F[axis]
        lo, hi = C[_face_layer(axis, slice(0, e))].copy(), C[_face_layer(axis, slice(1, e + 1))].copy()
        if periodic[axis]:
            hi[_face_layer(axis, e - 1)] = C[_face_layer(axis, 0)]
        if wall[2 * axis] == WALL_CODES["neumann"]:
            lo[_face_layer(axis, 0)] = 0.0
        if wall[2 * axis + 1] == WALL_CODES["neumann"]:
            hi[_face_layer(axis, e - 1)] = 0.0
        for name, a, w_face in (("low", lo, 2 * axis), ("high", hi, 2 * axis + 1)):
            read = a
            if wall[w_face] == WALL_CODES["neumann"]:      # (everything but the wall's own layer, which was replaced)
                read = a[_face_layer(axis, slice(1, e) if w_face % 2 == 0 else slice(0, e - 1))]
            if not (np.isfinite(read).all() and (read > 0.0).all()):
                raise ValueError("the face coefficients C%s must be finite and > 0 on every face that is read" % "zyx"[axis])
        d = [0, 0, 0]
        d[axis] = -1
        w[tuple(d)] = lo
        d[axis] = 1
        w[tuple(d)] = hi
    diag = ((((w[(-1, 0, 0)] + w[(0, -1, 0)]) + w[(0, 0, -1)]) + w[(0, 0, 1)]) + w[(0, 1, 0)]) + w[(1, 0, 0)]
    if sigma is not None:
        sig = np.asarray(sigma, dtype=np.float64)
        if not (np.isfinite(sig).all() and (sig >= 0.0).all()):
            raise ValueError("sigma must be finite and >= 0")
        diag = diag + sig
    # (the order of _assemble7's passes over w is stencil7_kappa's: -K, -J, -I, +I, +J, +K)
    order = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    return _assemble7(shape, {d: w[d] for d in order}, diag, periodic)


def face_coefficients_kappa(kappa, walls=None, scale=(1.0, 1.0, 1.0), spacing=None):
    """The three face arrays (Cz, Cy, Cx) of stencil7_kappa(kappa, walls, sigma, scale, spacing) (host only): every in-grid,
    seam and Dirichlet-wall coefficient as that function rounds it — the seam's in both C[0] and C[e] —, +0.0 on the faces of
    Neumann walls.  stencil7_faces of them (with the spaced sigma as sigma * cell_volumes(spacing)) is that matrix bit for
    bit: the face expression is symmetric in its two cells and a face's area is the same seen from both."""
    terms = {}
    stencil7_kappa(kappa, walls, None, scale, spacing, _terms=terms)
    shape = tuple(s - 2 for s in np.shape(kappa))
    out = []
    for axis, faces in enumerate(face_shapes(shape)):
        e = shape[axis]
        d = [0, 0, 0]
        d[axis] = -1
        lo = terms[tuple(d)]
        d[axis] = 1
        hi = terms[tuple(d)]
        C = np.zeros(faces)
        C[_face_layer(axis, slice(1, e + 1))] = hi         # (face m + 1 as its lo cell m rounds it; the last: the wall's or the seam's)
        C[_face_layer(axis, 0)] = lo[_face_layer(axis, 0)]
        out.append(C)
    return tuple(out)


def rhs_faces(faces, f=None, walls=None, values=None):
    """The right-hand side b that goes with stencil7_faces(faces, walls, sigma) (the definition _hip.faces_rhs and Solver.rhs
    of a from_faces solver are pinned to bit for bit), a float64 array of problemShape: b = ((((((f + t-K) + t-J) + t-I) +
    t+I) + t+J) + t+K), every operation rounded once.  A Dirichlet wall with the value g contributes C_wall * g to the cell at
    it (C_wall = C[0] or C[e], the coefficient the diagonal took); a Neumann wall's value is the OUTWARD flux through that
    face already integrated over it, t = value with no factor (the coefficients carry every factor, so nothing here knows an
    area); an in-grid face and a wall without a value contribute +0.0.  Only the cells at a Dirichlet wall with a value
    read a coefficient; the coefficients' values are not checked.  f, values: as rhs_kappa takes them.
    ValueError: what stencil7_faces refuses of the arrays' shapes, dtype and the walls; what wall_values_arguments and
    source_argument refuse."""
    F = _host_faces(faces)
    shape, wall = faces_arguments(tuple(a.shape for a in F), walls, None)
    f = source_argument(shape, f)
    values = wall_values_arguments(shape, wall, values)
    volume = np.zeros(shape) if f is None else np.broadcast_to(np.asarray(f, dtype=np.float64), shape).copy()
    terms = {}
    for face in range(6):
        axis, hi = face // 2, face % 2
        t = np.zeros(shape)
        terms[face] = t
        if values[face] is None:
            continue
        g = np.asarray(values[face], dtype=np.float64)
        layer = _face_layer(axis, -1 if hi else 0)
        if wall[face] == WALL_CODES["neumann"]:
            t[layer] = g
        else:
            t[layer] = F[axis][_face_layer(axis, shape[axis] if hi else 0)] * g
    return (((((volume + terms[0]) + terms[2]) + terms[4]) + terms[5]) + terms[3]) + terms[1]


def flux_faces(faces, u, walls=None, values=None):
    """The face fluxes (Fz, Fy, Fx) of u under stencil7_faces(faces, walls, sigma) with the boundary data of rhs_faces (the
    definition _hip.faces_flux and Solver.fluxes of a from_faces solver are pinned to bit for bit), one subtraction and one
    multiplication per face, each rounded once:
      - an in-grid face: F[m] = C[m] * (u_lo - u_hi).
      - a periodic axis: F[0] = F[e] = C[0] * (u_{e-1} - u_0).
      - a Dirichlet wall: F[0] = C[0] * (g - u_0), F[e] = C[e] * (u_{e-1} - g); g = +0.0 where the wall has no value.
      - a Neumann wall: +0.0 without a value, nothing read; with a value v (rhs_faces' outward flux) F[0] = v, F[e] = -v.
    For every u, to rounding: divergence_faces(*flux_faces(faces, u, walls, values)) + sigma u = stencil7_faces(faces, walls,
    sigma) @ u - rhs_faces(faces, None, walls, values).  The coefficients' values are not checked.
    ValueError: what rhs_faces refuses; a u of another shape."""
    C = _host_faces(faces)
    shape, wall = faces_arguments(tuple(a.shape for a in C), walls, None)
    values = wall_values_arguments(shape, wall, values)
    u = np.asarray(solution_argument(shape, u), dtype=np.float64).reshape(shape)
    periodic = periodic_axes(wall)
    out = []
    for axis, fshape in enumerate(face_shapes(shape)):
        e = shape[axis]
        F = np.zeros(fshape)
        inner = _face_layer(axis, slice(1, e))
        F[inner] = C[axis][inner] * (u[_face_layer(axis, slice(0, e - 1))] - u[inner])
        first, last = _face_layer(axis, 0), _face_layer(axis, e)
        if periodic[axis]:
            seam = C[axis][first] * (u[_face_layer(axis, e - 1)] - u[first])
            F[first] = seam
            F[last] = seam
            out.append(F)
            continue
        for side, place, cell in ((0, first, 0), (1, last, e - 1)):
            w = 2 * axis + side
            at = _face_layer(axis, cell)
            if wall[w] == WALL_CODES["neumann"]:
                if values[w] is not None:
                    t = np.asarray(values[w], dtype=np.float64)
                    F[place] = -t if side else t
                continue
            g = 0.0 if values[w] is None else np.asarray(values[w], dtype=np.float64)
            F[place] = C[axis][place] * (u[at] - g if side else g - u[at])
        out.append(F)
    return tuple(out)


def stencil27_variable(shape, seed=2024, rows=None):
    """27-point variable-coefficient operator of BASELINE.json configs[4] as SURVEY.md 8(d)
    specifies it (NOT in the reference): Q1 finite-element stiffness of -div(kappa grad u) on a
    box of unit cells whose unknowns are the interior nodes `shape` (homogeneous Dirichlet
    boundary), kappa = exp(U(-1, 1) ln 10) per cell from default_rng(seed).  Symmetric positive
    definite.  C-order numbering, sorted CSR with int32 indices, all 27 couplings of a node
    stored (the six along the axes cancel to ~0 only where kappa is locally constant),
    assembled directly in CSR (the 256^3 operator has 450 M entries).  rows=(lo, hi): only those
    rows, as a (hi - lo) x N matrix with global columns (one slab of a distributed run)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3:
        raise ValueError("stencil27_variable needs a 3-D shape")
    N = int(np.prod(shape))
    strides = (shape[1] * shape[2], shape[2], 1)
    K, corners = _q1_element_stiffness()
    rng = np.random.default_rng(seed)
    # one cell per (node, node + 1) interval including the two boundary layers: (n + 1)^3 cells;
    # cell c spans nodes c - 1 .. c along each axis (node -1 and node n are the Dirichlet boundary)
    kappa = np.exp(rng.uniform(-1.0, 1.0, size=tuple(s + 1 for s in shape)) * np.log(10.0))
    row_lo, row_hi = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    M = row_hi - row_lo
    cz, cy, cx = np.unravel_index(np.arange(row_lo, row_hi, dtype=np.int64), shape)
    coords = (cz, cy, cx)
    dirs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]   # ascending column offset

    def valid_of(d):
        v = np.ones(M, dtype=bool)
        for ax in range(3):
            if d[ax] < 0:
                v &= coords[ax] > 0
            elif d[ax] > 0:
                v &= coords[ax] < shape[ax] - 1
        return v
    valid = [valid_of(d) for d in dirs]
    counts = np.zeros(M, dtype=np.int64)
    for v in valid:
        counts += v
    indptr = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz, dtype=np.float64)
    cursor = indptr[:-1].copy()
    gid = np.arange(row_lo, row_hi, dtype=np.int64)
    for d, v in zip(dirs, valid):
        off = d[0] * strides[0] + d[1] * strides[1] + d[2] * strides[2]
        # A[i, i + d] = sum over the cells that contain both nodes: local node a of the cell is i,
        # local node a + d is i + d; the cell's origin node is i - a, i.e. cell index i - a + 1
        val = np.zeros(int(v.sum()))
        pz, py, px = cz[v], cy[v], cx[v]
        for ia, a in enumerate(corners):
            b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
            if min(b) < 0 or max(b) > 1:
                continue
            ib = corners.index(b)
            val += kappa[pz - a[0] + 1, py - a[1] + 1, px - a[2] + 1] * K[ia, ib]
        pos = cursor[v]
        indices[pos] = (gid[v] + off).astype(np.int32)
        data[pos] = val
        cursor += v
    out = sp.csr_matrix((data, indices, indptr.astype(np.int32)), shape=(M, N))
    out.has_sorted_indices = True
    return out
