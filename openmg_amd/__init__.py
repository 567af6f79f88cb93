"""
openmg_amd — geometric multigrid V-cycle on AMD MI355X (gfx950), presenting the public
names of tsbertalan/openmg: mgSolve, mgCycle (alias mg_cycle), defaults, smooth,
smoothToThreshold, coarseSolve, tools, operators, solvers.

All numerical work runs in hand-written HIP kernels behind libopenmg_hip.so
(include/openmg_hip.h); this package is the NumPy/SciPy-facing host side.  There is no
CPU fallback: without the library or without a GPU the calls raise.

Extra keys understood in the `parameters` dict (ignored by the reference):
    'smoother'  'gs' (default: the reference's lexicographic Gauss-Seidel iterate),
                'colour' (multi-colour GS; red-black on 5/7-point stencils) or 'jacobi'
                or 'line' (alias 'line-gs'): zebra line Gauss-Seidel for ANISOTROPIC grid operators — a stretched grid, thin
                boundary-layer cells — where every point smoother stalls whatever the 'cycle' and 'accel'.  The grid lines
                along one axis, coloured by the parity of the sum of their other two indices, are solved exactly (a
                tridiagonal solve each), colour 0 then colour 1.  Every smoothed level must be a 5-point (2-D) or 7-point
                (3-D) stencil on the lexicographically numbered grid, any coefficients, extents even or odd; a 27-point,
                periodic or 1-D operator raises HipError (ERR_UNSUPPORTED) naming the level.  It repairs ONE strong axis
                (couplings 100 : 1 : 1: 9 V-cycles where 'colour' needs hundreds); with two strong axes (one weak one) it
                is no better than 'colour' — that is what 'coarsening' (semicoarsening, below) repairs, with 'line' or
                with any point smoother; plane smoothing is not here.
                Works with every 'accel', 'dtype', 'cycle', 'overCorrection', 'nullspace', 'coarsening', device arrays
                and Solver; single GPU, the lists setup route, set-by-set launches (no fused passes)
                or 'line-periodic': 'line' for operators with PERIODIC axes (a channel periodic in x and z, a periodic
                box; Solver.from_kappa(..., walls=<'periodic' ...>) makes them).  An axis of extent >= 3 is periodic on a
                level when its seam rows hold the wrapped neighbour (columns ascending).  Across the lines the wrapped
                coupling is one more cross coupling — such an axis must have an EVEN extent on every smoothed level, or
                HipError (ERR_UNSUPPORTED) names the level and the extent: choose the depth or 'coarsening' accordingly;
                along the lines every line is cyclic and solved exactly by a factorisation of the tridiagonal block with
                its two corner entries (a singular block — no cross couplings, no shift: HipError ERR_INVALID).  On an
                operator without wrapped rows it is 'line', bit for bit; 'coarsening': 'auto' on a periodic operator
                stays ERR_UNSUPPORTED (named factors work).  'line' itself keeps refusing periodic operators
    'lineAxis'  with 'line' / 'line-periodic': None or 'auto' (default: the axis whose couplings of A_in have the largest sum of |a_ij|, ties
                to the unit-stride axis), or an index into 'problemShape' (C order: the last entry is the unit-stride
                axis).  The same axis on every level.  Anything else raises ValueError before any device work; mgSolve's
                infoDict['lineAxis'] (and Solver's info) reports the axis used
    'coarsening'  None or 'full' (default: every restriction halves every axis, the reference's hierarchy, bit for bit),
                'auto', or a sequence with one tuple per restriction holding a factor of 1 or 2 for each axis of
                'problemShape' (2-D / 3-D): SEMICOARSENING for grid-aligned anisotropic operators — only the strongly
                coupled axes are coarsened, which halves their coupling relative to the others, until the operator is
                isotropic and coarsening is full again.  It repairs what 'line' cannot (two strong axes, three different
                strengths) with any smoother, and composes with 'line'.  'auto' picks the factors level by level from
                the operator's couplings (an axis is coarsened when its mean |a_ij| is at least half the strongest
                axis's; it needs a 5- / 7-point stencil: a 27-point or periodic operator raises HipError
                (ERR_UNSUPPORTED) naming the level — name the factors for those).  A named sequence is consumed entry by
                entry; the depth rule is unchanged ('gridLevels', then 'minSize' after the first restriction).  An
                entry of all ones, a factor of 2 on an extent that is odd (see 'oddExtents') or below 4, or a sequence shorter than the
                depth reached raises ValueError before any device work.  No axis ever collapses to 1.  Works with every
                'smoother', 'accel', 'dtype', 'cycle', 'overCorrection', 'nullspace' and device arrays; single GPU.
                Semicoarsened levels run the set-by-set row kernels (no fused passes) and a V-cycle does about twice
                the finest level's work instead of 8/7 of it: a cycle costs more, the gain is in their number.
                'overCorrection' > 1 is the repair for the 2**dim aggregation and CAN DIVERGE on a hierarchy that
                coarsens one axis per level (measured: 'colour', F, 1.8 at 100 : 10 : 1); with ONE strong
                axis use 'line' (a point smoother then leaves a large coarsest level to the direct solve).
                infoDict['coarsening'] (and Solver's info) lists the factor tuples used, infoDict['levelShapes'] every
                level's grid.  Solver.update keeps the factors chosen at construction and builds a new hierarchy
    'oddExtents'  None (default: an axis is halved only where its extent is even — the behaviour above, bit for bit) or
                'merge': grids of ANY extent get a real hierarchy (100^3, 250^3, 300 x 150 x 75).  An axis of extent
                e >= 4, odd or even, can take a factor 2: it gets e // 2 coarse cells, and where e is odd the last
                aggregate along that axis holds three cells instead of two (every entry of R keeps the one weight
                1 / prod(factors), so 'nullspace': 'constant' works unchanged).  With 'coarsening' 'auto' the rule's
                eligibility becomes extent >= 4; named factor tuples may put a 2 on any extent >= 4 (below 4 still raises
                ValueError); with None / 'full' every restriction takes factor 2 on each axis with extent >= 4 and 1 on
                the others — the plain C-order aggregation, on boxes too, NOT the reference's restriction(), which is no
                aggregation on an odd extent — to the usual depth rule, ending where no axis is eligible; on a cube
                with extents m * 2^k these are the matrices of the default.  A level whose restriction has a merged
                cell runs the set-by-set row kernels (no fused passes); the even levels above and below it keep theirs.
                infoDict['coarsening'] / ['levelShapes'] report what was built.  Works with every 'smoother', 'accel',
                'dtype', 'cycle', 'overCorrection', 'nullspace', device arrays and Solver (update keeps the factors
                and the key); single GPU; 'dense' true or any other value raises ValueError before any device work
    'omega'     relaxation weight for 'jacobi' (default 2/3)
    'accel'     mgSolve only: None (default: plain V-cycles, the reference's loop) or 'cg': flexible preconditioned
                conjugate gradients (FCG(1)) on the finest level with one zero-start V-cycle as the preconditioner per
                iteration — 'cycles' then caps the CG iterations, 'threshold' is the target of the recurrence residual
                norm, infoDict['cycle'] counts iterations and infoDict['norm'] is the true ||b - A u||; a CG breakdown
                (an indefinite operator or preconditioner) raises RuntimeError.  Any other value raises ValueError
    'cycle'     'V' (default: the reference's cycle), 'F' or 'W': how often a cycle visits the coarse levels.  A cycle over
                level l visits level l + 1 once ('V', and wherever l + 1 is the coarsest level: its direct solve is exact)
                or twice, the second visit starting from the first one's result: 'F' = an F- then a V-cycle, 'W' = two
                W-cycles.  Level l >= 1 is visited l + 1 ('F') or 2**l ('W') times per cycle.  The plain aggregation's
                Galerkin operators are about twice too stiff, so a V-cycle's factor degrades with depth; F and W repair it
    'overCorrection'  a finite float > 0, default 1.0: the coarse correction is added as alpha * R^T e.  The factor is applied
                as the prolongation's weight (every entry of R^T times alpha, rounded once to the levels' precision).
                1.5 .. 1.8 with 'F' or 'W' is the standard repair for plain aggregation; with 'V' the overshoot compounds
                down the levels and alpha > 1 CAN DIVERGE.  Both keys hold for mgSolve (with every 'accel' and 'dtype') and
                mgCycle (from the level it is entered at downward); anything else raises ValueError before any device work
    'dtype'     'float64' (default, the reference's precision) or 'float32': the precision the
                levels are stored and computed in on the device (inputs / outputs stay float64).
                mgSolve only: 'mixed' — fp32 levels and V-cycles inside fp64 iterations on the finest level (its
                operator, iterate, residual and CG vectors in fp64, each cycle run on fl32(r)): with accel None every
                cycle is a defect correction x += M(fl32(b - A x)), with accel 'cg' FCG uses z = M(fl32(r)); u and
                every norm are fp64 and converge to the fp64 solution at fp32 cycle cost.  mgCycle raises ValueError
    'nullspace' None (default) or 'constant': A_in is SINGULAR with the constant null space — zero row and column sums: the
                pure-Neumann or periodic Poisson problem (the pressure equation of an incompressible flow step).  The
                coarsest operator is then inverted on the complement of the constants (as A + gamma 1 1^T, an explicit
                inverse: at most 16384 coarsest unknowns), mgSolve subtracts mean(b) from its copy of b (a b with a mean has
                no solution; the caller's array is untouched and every norm is that of the projected system) and returns
                the u with mean(u) = 0.  An operator without that null space (a Dirichlet boundary) raises HipError
                (ERR_INVALID).  Works with every 'smoother', 'accel', 'dtype', 'cycle' and 'overCorrection' and with device
                arrays.  mgCycle, the reference's recursive building block, projects nothing: only the coarse solve
                changes (b and the iterate are the caller's).  Anything else raises ValueError before any device work
    'trustOperators'  mgCycle only, default False: when the caller passes the SAME list members (object identity) it
                passed on an earlier call — e.g. infoDict['A'] / infoDict['R'] handed back unchanged — the per-call
                checksum of every byte of the lists (what recognises an operator edited in place) is skipped

`b` and `initial` may be DEVICE arrays (objects with `__cuda_array_interface__`, e.g. PyTorch-ROCm tensors: contiguous
float64): mgCycle / mgSolve then return a device array of the same kind and only the norm crosses PCIe.

Many right-hand sides with one operator (a time-stepping loop's pressure solves): `Solver(A_in, parameters)` runs
mgSolve's whole setup once; `solve(b, initial=None, out=None, **overrides)` then costs the solve alone, may start from
the previous step's u, stops below max('threshold', 'rtol' * ||b||) or after 'cycles' and returns (u, info) — from zero,
the bits of mgSolve; `apply(r)` is one zero-start cycle (a preconditioner), `update(A_new)` takes new values in the same
pattern, `close()` frees the device (openmg_amd/_solver.py).
"""
import weakref

import numpy as np
import scipy.sparse as sp

from . import _devarray, _hip
from . import operators, solvers, tools
from .solvers import coarseSolve, smooth, smoothToThreshold

__all__ = ["mgSolve", "mgCycle", "mg_cycle", "defaults", "smooth", "smoothToThreshold",
           "coarseSolve", "tools", "operators", "solvers", "clear_cache", "Solver"]

# Same keys and values as the reference (openmg/__init__.py:16-27).  Like there, this dict
# is module-global and mgSolve writes 'coarsestLevel' into it on every call.
defaults = {
    "problemShape": (200,),
    "gridLevels": 2,
    "verbose": False,
    "threshold": 0.1,
    "cycles": 0,
    "preIterations": 1,
    "postIterations": 0,
    "dense": False,
    "giveInfo": False,
    "minSize": 8,
}

_DEFAULT_OMEGA = 2.0 / 3.0


def _smoother_of(parameters):
    kind = parameters.get("smoother", "gs")
    code = _hip.smoother_code(kind)
    if _hip.is_line_smoother(code) and code & ~_hip.SMOOTH_LINE_WRAP == _hip.SMOOTH_LINE:
        # 'line' / 'line-periodic': parameters['lineAxis'] picks the code (None / 'auto': the library scans level 0)
        axis = parameters.get("lineAxis")
        shape = parameters.get("problemShape")
        if shape is None and not (axis is None or (isinstance(axis, str) and axis == "auto")):
            raise ValueError("parameters['lineAxis'] = %r is an index into parameters['problemShape'], which is missing" % (axis,))
        code = _hip.line_smoother_code(axis, () if shape is None else shape, wrap=bool(code & _hip.SMOOTH_LINE_WRAP))
    omega = float(parameters.get("omega", _DEFAULT_OMEGA if code == _hip.SMOOTH_JACOBI else 1.0))
    return code, omega


def _dtype_of(parameters):
    return _hip.dtype_code(parameters.get("dtype", "float64"))


def _cycle_of(parameters):
    """(shape, over-correction factor) of parameters['cycle'] / ['overCorrection']; ValueError for anything else."""
    shape = parameters.get("cycle", "V")
    if not isinstance(shape, str) or shape not in _hip.CYCLES:
        raise ValueError("parameters['cycle'] must be 'V', 'F' or 'W', not %r" % (shape,))
    try:
        alpha = _hip.over_correction_of(parameters.get("overCorrection", 1.0))
    except ValueError:
        raise ValueError("parameters['overCorrection'] must be a finite float > 0, not %r" % (parameters.get("overCorrection"),))
    return shape, alpha


def _nullspace_of(parameters):
    """parameters['nullspace']: None or 'constant'; ValueError for anything else."""
    kind = parameters.get("nullspace")
    if kind is not None and not (isinstance(kind, str) and kind == "constant"):
        raise ValueError("parameters['nullspace'] must be None or 'constant', not %r" % (kind,))
    return kind


# ---- device hierarchy cache for repeated mgCycle calls ---------------------------------------
# mgCycle receives the A and R lists on every call (openmg/__init__.py:151); uploading
# them each time would dominate.  A cache entry holds the device hierarchy TOGETHER WITH strong
# references to the list members it was built from, so that neither their ids nor their buffer
# addresses can be recycled for other matrices while the entry lives, and the key carries a
# checksum of the stored arrays (every byte), so that a matrix edited in place (or rebuilt into
# the same buffers) misses.  Members that are not CSR are converted once per object (cached by id
# while the object lives).
_cache = {}
_CACHE_SLOTS = 2

def _array_checksum(a):
    """Checksum of the WHOLE array — an in-place edit of a few entries of a large operator must not hit
    the stale device copy.  omg_host_checksum hashes 4 MiB chunks on all host threads (one Python thread
    with xxhash: ~5 GB/s under the interpreter lock, 0.3 s per mgCycle call for a 256^3 operator)."""
    return _hip.host_checksum(np.asarray(a))


_csr_of = {}          # id(non-CSR sparse member) -> (weak reference, checksum of its own arrays, its CSR form)


def _as_csr_cached(M):
    """CSR form of a sparse member, converted once while the member lives and keeps its content."""
    if sp.isspmatrix_csr(M):
        return M
    arrays = [getattr(M, name) for name in ("data", "indices", "indptr", "row", "col", "offsets")
              if isinstance(getattr(M, name, None), np.ndarray)]
    if not arrays or any(a.dtype.kind == "O" for a in arrays):
        # LIL (object arrays of Python lists), DOK: no flat buffers to checksum — converted on every call
        return sp.csr_matrix(M)
    src = tuple(_array_checksum(a) for a in arrays)
    entry = _csr_of.get(id(M))
    if entry is not None and entry[0]() is M and entry[1] == src:
        return entry[2]
    C = sp.csr_matrix(M)
    try:
        ref = weakref.ref(M, lambda _r, k=id(M): _csr_of.pop(k, None))
    except TypeError:                           # not weakly referenceable: convert every time
        return C
    _csr_of[id(M)] = (ref, src, C)
    return C


def _fingerprint(A, R, n_levels, code, omega, dtype, nullspace=None):
    def one(M):
        if sp.issparse(M):
            M = _as_csr_cached(M)
            return (M.shape, M.nnz, _array_checksum(M.indptr), _array_checksum(M.indices), _array_checksum(M.data))
        M = np.asarray(M)
        return (M.shape, _array_checksum(M))
    return (tuple(one(M) for M in A[:n_levels]), tuple(one(M) for M in R[:n_levels - 1]), code, omega, dtype, nullspace)


def _hierarchy_for(A, R, n_levels, code, omega, dtype=_hip.DTYPE_F64, trust=False, nullspace=None):
    if trust:
        # parameters['trustOperators']: the caller vouches that list members it has passed before are unchanged; an entry
        # built from the very same objects (identity, not equality) and the same smoother / precision is taken as it is
        for h, members, how in _cache.values():
            if (how == (code, omega, dtype, nullspace) and len(members[0]) == n_levels
                    and all(a is m for a, m in zip(A[:n_levels], members[0]))
                    and all(r is m for r, m in zip(R[:n_levels - 1], members[1]))):
                return h
    key = _fingerprint(A, R, n_levels, code, omega, dtype, nullspace)
    entry = _cache.get(key)
    if entry is None:
        while len(_cache) >= _CACHE_SLOTS:
            _cache.pop(next(iter(_cache)))[0].close()
        members = (list(A[:n_levels]), list(R[:n_levels - 1]))
        h = _hip.Hierarchy(members[0], members[1], smoother=code, omega=omega, dtype=dtype, nullspace=nullspace)
        entry = _cache[key] = (h, members, (code, omega, dtype, nullspace))
    return entry[0]


def clear_cache():
    """Free the device hierarchies kept for repeated mgCycle calls."""
    while _cache:
        _cache.popitem()[1][0].close()


# ---- the two public drivers ---------------------------------------------------------------
def mgSolve(A_in, b, parameters):
    """Solve A_in u = b by V-cycles on the GPU; same contract as openmg.mgSolve
    (openmg/__init__.py:28-148).

    parameters must hold 'problemShape' and 'gridLevels'; the optional keys and their
    defaults are those of `openmg_amd.defaults`.  gridLevels = g builds g restriction
    operators, i.e. g+1 grids, unless 'minSize' stops the coarsening earlier.  At least one
    cycle is run; cycling stops when 'cycles' (> 0) is reached or the absolute residual
    2-norm falls below 'threshold' (> 0); if both are <= 0 a ValueError is raised (after the
    first cycle, as in the reference).  The caller's dict is completed with the defaults
    and its 'coarsestLevel' is overwritten with the depth actually built.

    Returns u, or (u, infoDict) when parameters['giveInfo'] is true; infoDict holds
    'cycle', 'norm', and the hierarchies 'R' and 'A' as SciPy CSR lists.
    """
    hierarchy, R, A, accel, shape, alpha = _setup(A_in, parameters, defaults)
    verbose = parameters["verbose"]
    pre, post = parameters["preIterations"], parameters["postIterations"]
    depth = parameters["coarsestLevel"]
    b_on_device = _devarray.is_device_array(b)
    try:
        hierarchy.set_cycle(shape, alpha)
        if b_on_device:
            _devarray.synchronize()
            hierarchy.resident_load_dev(_devarray.address(b, hierarchy.sizes[0], "b"))
        else:
            hierarchy.resident_load(np.asarray(b, dtype=np.float64).reshape(-1))
        if accel == "cg":
            cycle, norm = _solve_cg(hierarchy, parameters, pre, post, depth, verbose, shape)
        else:
            cycle, norm = _solve_cycles(hierarchy, parameters, pre, post, depth, verbose, shape)
        if b_on_device:
            result = _devarray.empty_like(b, hierarchy.sizes[0])
            hierarchy.resident_fetch_dev(_devarray.address(result, hierarchy.sizes[0], "result"))
        else:
            result = hierarchy.resident_fetch()
        line_axis = hierarchy.line_axis
    finally:
        hierarchy.close()

    infoDict = {"norm": norm, "cycle": cycle, "R": R, "A": A}
    if line_axis is not None:
        infoDict["lineAxis"] = line_axis           # ('line': the axis the lines ran along, an index into problemShape)
    if hierarchy.coarsening is not None:
        # ('coarsening' 'auto' or named: the factors of every restriction built, and every level's grid)
        infoDict["coarsening"] = list(hierarchy.coarsening)
        infoDict["levelShapes"] = list(hierarchy.level_shapes)
    if verbose:
        print("Returning mgSolve after %i cycle(s) with norm %f" % (cycle, norm))
    if parameters["giveInfo"]:
        return result, infoDict
    return result


def _accel_of(parameters):
    accel = parameters.get("accel")
    if accel not in (None, "cg"):
        raise ValueError("parameters['accel'] must be None or 'cg', not %r" % (accel,))
    return accel


def _setup(A_in, parameters, completed_from):
    """mgSolve's whole setup, shared with Solver: checks the keys, completes `parameters` in place from `completed_from`
    (mgSolve: the module-global `defaults`, which gets its 'coarsestLevel' written as in the reference; Solver: a copy),
    writes the depth actually built into parameters['coarsestLevel'] and builds the device hierarchy.  Returns
    (hierarchy, R, A, accel, cycle shape, over-correction factor); R = A = None on the device route (giveInfo off)."""
    accel = _accel_of(parameters)
    shape, alpha = _cycle_of(parameters)
    nullspace = _nullspace_of(parameters)
    problemShape = parameters["problemShape"]
    gridLevels = parameters["gridLevels"]
    completed_from["coarsestLevel"] = gridLevels - 1
    tools.dictUpdateNoClobber(completed_from, parameters)
    verbose = parameters["verbose"]
    dense = parameters["dense"]
    code, omega = _smoother_of(parameters)
    coarsening = _coarsening_of(parameters)
    # (Solver.from_kappa: A_in is the coefficient field's arguments; the plain device route below assembles level 0 in HBM,
    # every other route gets the operator assembled on the device into host arrays and runs as for any A_in)
    # (Solver.from_faces: the same with the face coefficients' arguments)
    kappa = A_in if isinstance(A_in, (_hip.KappaArgs, _hip.FaceArgs)) else None
    if coarsening is not None:
        A_in = A_in if kappa is None else kappa.matrix()
        return _setup_semicoarsened(A_in, parameters, coarsening, code, omega, nullspace) + (accel, shape, alpha)

    # (the device route qualifies levels for the FUSED paths, which exist for the colour orderings and 2-D weighted Jacobi; with
    # the reference's own lexicographic smoother it would build the Galerkin chain in HBM only to fetch it again for the host's
    # orderings and codings: 1.14 s of setup at 256^3 where the lists route below takes 0.7)
    fused_smoother = code == _hip.SMOOTH_GS_COLOUR or (code == _hip.SMOOTH_JACOBI and len(tuple(problemShape)) == 2)
    n_fused = _device_setup_depth(A_in, problemShape, parameters) if fused_smoother else 0
    if n_fused:
        # nobody asked for the operator lists (giveInfo off): restrictions, Galerkin products and the levels' qualification
        # for the fused paths stay in HBM (omg_hierarchy_create_from_fine); same hierarchy, same results
        R = A = None
        parameters["coarsestLevel"] = n_fused
        if kappa is not None:
            from_field = _hip.Hierarchy.from_faces if isinstance(kappa, _hip.FaceArgs) else _hip.Hierarchy.from_kappa
            hierarchy = from_field(kappa, n_fused, smoother=code, omega=omega, dtype=_dtype_of(parameters), nullspace=nullspace)
        else:
            hierarchy = _hip.Hierarchy.from_fine(A_in, problemShape, n_fused, smoother=code, omega=omega, dtype=_dtype_of(parameters),
                                                 nullspace=nullspace)
    else:
        A_in = A_in if kappa is None else kappa.matrix()
        R = operators.restrictionList(problemShape, parameters["coarsestLevel"], parameters["minSize"],
                                      dense=dense, verbose=verbose)
        parameters["coarsestLevel"] = len(R)
        A = operators.coeffecientList(A_in, R, dense=dense, verbose=verbose)
        hierarchy = _hip.Hierarchy(A, R, smoother=code, omega=omega, dtype=_dtype_of(parameters), nullspace=nullspace)
    return hierarchy, R, A, accel, shape, alpha


def _odd_extents_of(parameters):
    """parameters['oddExtents']: None or 'merge'; ValueError for anything else."""
    value = parameters.get("oddExtents")
    _hip.odd_code(value)
    return value


def _coarsening_of(parameters):
    """parameters['coarsening'] and ['oddExtents'] checked (operators.coarseningOf): None for the reference's full
    coarsening, 'auto', or the list of factor tuples the depth rule will use (with 'oddExtents': 'merge' also for None /
    'full'); ValueError for anything else — before any device work."""
    value = parameters.get("coarsening")
    odd = _odd_extents_of(parameters)
    if odd is None and (value is None or (isinstance(value, str) and value == "full")):
        return None
    if odd is not None and parameters.get("dense", defaults["dense"]):
        raise ValueError("parameters['oddExtents'] works on sparse operators: parameters['dense'] must be false")
    levels = parameters.get("coarsestLevel", parameters.get("gridLevels", defaults["gridLevels"]) - 1)
    return operators.coarseningOf(value, parameters.get("problemShape"), levels, parameters.get("minSize", defaults["minSize"]), odd)


def _setup_semicoarsened(A_in, parameters, coarsening, code, omega, nullspace):
    """_setup with parameters['coarsening'] = 'auto' or factor tuples: (hierarchy, R, A).  The device route
    (omg_hierarchy_create_from_fine_semi) when nobody asked for the lists and the smoother is one the device route takes
    today, else operators.semicoarsenedLists; either way the same hierarchy."""
    problemShape = tuple(int(s) for s in parameters["problemShape"])
    dim = len(problemShape)
    odd = _odd_extents_of(parameters)
    if parameters["dense"]:
        raise ValueError("parameters['coarsening'] / ['oddExtents'] work on sparse operators: parameters['dense'] must be false")
    if not sp.issparse(A_in):
        A_in = sp.csr_matrix(A_in)
    if A_in.shape != (tools.product(problemShape),) * 2:
        raise ValueError("parameters['problemShape'] %s does not match the operator's shape %s" % (problemShape, A_in.shape))
    levels = parameters["coarsestLevel"] + 1
    line_axis = None
    if _hip.is_line_smoother(code) and coarsening == "auto":
        # the rule treats the line axis apart, so it must know it before the hierarchy exists: 'lineAxis' None / 'auto' is
        # resolved here as the library resolves it (the largest sum of |a_ij|, ties to the unit-stride axis) and then NAMED
        # to the library, so that both use the same axis
        wrap = bool(code & _hip.SMOOTH_LINE_WRAP)           # ('line-periodic': the flag is stripped before the axis is read)
        if code & ~_hip.SMOOTH_LINE_WRAP == _hip.SMOOTH_LINE:
            sums = _hip.axis_couplings(A_in, problemShape)[0]
            line_axis = dim - 1
            for axis in range(dim - 2, -1, -1):
                if sums[axis] > sums[line_axis]:
                    line_axis = axis
            code = _hip.line_smoother_code(line_axis, problemShape, wrap=wrap)
        else:
            line_axis = dim - 1 - ((code & ~_hip.SMOOTH_LINE_WRAP) - _hip.SMOOTH_LINE_X)
    fused_smoother = code == _hip.SMOOTH_GS_COLOUR or (code == _hip.SMOOTH_JACOBI and dim == 2)
    if fused_smoother and not (parameters["giveInfo"] or parameters["verbose"]):
        R = A = None
        named = None if coarsening == "auto" else coarsening
        hierarchy = _hip.Hierarchy.from_fine_semi(A_in, problemShape, levels if named is None else len(named), named,
                                                  min_size=parameters["minSize"], smoother=code, omega=omega, dtype=_dtype_of(parameters),
                                                  nullspace=nullspace, oddExtents=odd)
    else:
        R, A, factors = operators.semicoarsenedLists(A_in, problemShape, coarsening, parameters["coarsestLevel"], parameters["minSize"],
                                                     lineAxis=line_axis, oddExtents=odd)
        hierarchy = _hip.Hierarchy(A, R, smoother=code, omega=omega, dtype=_dtype_of(parameters), nullspace=nullspace)
        hierarchy._set_coarsening(problemShape, factors, odd)
    parameters["coarsestLevel"] = len(hierarchy.coarsening)
    return hierarchy, R, A


# CG iterations per omg_resident_pcg call when only 'threshold' stops the solve (the next call restarts from the iterate)
_CG_CHUNK = 10000


def _solve_cg(hierarchy, parameters, pre, post, depth, verbose, shape="V", observe=None):
    """mgSolve's loop with parameters['accel'] == 'cg': FCG on the resident iterate; returns (iterations, true norm).
    observe (Solver): called with (iteration, recurrence norm) for every iteration, before a breakdown is reported."""
    cycles, threshold = parameters["cycles"], parameters["threshold"]
    both_off = threshold <= 0 and cycles <= 0
    done = 0
    while True:
        max_iter = 1 if both_off else (cycles - done if cycles > 0 else _CG_CHUNK)
        its, norms, norm, breakdown = hierarchy.resident_pcg(pre, post, max_iter, threshold if threshold > 0 else 0.0)
        if observe is not None:
            for k, nk in enumerate(norms):
                observe(done + k + 1, float(nk))
        if verbose:
            for k, nk in enumerate(norms):
                _announce_descent(depth, shape)
                print("Residual norm from cycle %d is %f." % (done + k + 1, nk))
        if breakdown:
            raise RuntimeError("mgSolve accel='cg': conjugate gradients broke down in iteration %d (the operator or the "
                               "V-cycle is not positive definite)" % (done + its + 1))
        done += its
        if both_off:
            raise ValueError("Either parameters['threshold'] or parameters['cycles'] must be > 0.")
        if (cycles > 0 and done >= cycles) or (threshold > 0 and len(norms) and norms[-1] < threshold):
            return done, norm


def _solve_cycles(hierarchy, parameters, pre, post, depth, verbose, shape="V", observe=None):
    """mgSolve's loop of plain V-cycles (openmg/__init__.py:112-138); returns (cycles, norm).
    observe (Solver): called with (cycle, norm) for every cycle as soon as its norm is on the host."""
    if verbose:
        _announce_descent(depth, shape)
    norm = hierarchy.resident_cycle(pre, post)
    cycle = 1
    if observe is not None:
        observe(cycle, norm)
    if verbose:
        print("Residual norm from cycle %d is %f." % (cycle, norm))
    if parameters["threshold"] <= 0 and parameters["cycles"] <= 0:
        raise ValueError("Either parameters['threshold'] or parameters['cycles'] must be > 0.")

    def finished():
        by_count = parameters.get("cycles", 0) > 0 and cycle >= parameters["cycles"]
        by_norm = "threshold" in parameters and parameters["threshold"] > 0 and norm < parameters["threshold"]
        return by_count or by_norm

    if (not verbose and parameters.get("cycles", 0) > cycle and not parameters.get("threshold", 0) > 0):
        # stop rule = cycle count only: the remaining cycles go to the device in one call (every
        # cycle's norm is still computed; only the last one is observable here)
        batch = hierarchy.resident_cycles(pre, post, parameters["cycles"] - cycle)
        norm = batch[-1]
        if observe is not None:
            for k, nk in enumerate(batch):
                observe(cycle + k + 1, nk)
        cycle = parameters["cycles"]
    while not finished():
        if verbose:
            print("cycle %i < cycles %i" % (cycle, parameters["cycles"]))
            _announce_descent(depth, shape)
        cycle += 1
        norm = hierarchy.resident_cycle(pre, post)
        if observe is not None:
            observe(cycle, norm)
        if verbose:
            print("Residual norm from cycle %d is %f." % (cycle, norm))
    return cycle, norm


def _device_setup_depth(A_in, problemShape, parameters):
    """How many restrictions operators.restrictionList would build (openmg/operators.py:128-141) when mgSolve's whole
    setup can stay on the device — 0 when it cannot: the caller wants the lists (giveInfo), the dense path, progress
    messages, or the shape is not one whose restriction is the plain aggregation at every level (2-D / 3-D, first and
    last extent equal, extents even on every restricted level) — then the ordinary route runs (and raises what the
    reference raises)."""
    if parameters.get("giveInfo") or parameters.get("dense") or parameters.get("verbose"):
        return 0
    if not (sp.issparse(A_in) or isinstance(A_in, (_hip.KappaArgs, _hip.FaceArgs))):        # (their .shape: the operator's, as a matrix has it)
        return 0
    try:
        shape = tuple(int(s) for s in problemShape)
    except TypeError:
        return 0
    dim = len(shape)
    if dim not in (2, 3) or shape[0] != shape[-1] or min(shape) < 2:
        return 0
    if int(np.prod(shape)) != A_in.shape[0] or A_in.shape[0] != A_in.shape[1]:
        return 0

    def rows_of(level):                 # rows of restriction(shape // 2**level), or None where the reference's quirks start
        ext = [s // 2 ** level for s in shape]
        if any(e < 2 or e % 2 for e in ext):
            return None
        return int(np.prod(ext)) // 2 ** dim

    first = rows_of(0)
    if first is None or first in (0, 1):
        return 0
    n = 1
    for level in range(1, parameters["coarsestLevel"] + 1):
        rows = rows_of(level)
        if rows is None or rows in (0, 1):
            return 0                    # (the reference raises or truncates here: let the ordinary route do that)
        if rows <= parameters["minSize"]:
            break
        n += 1
    return n


def _announce_descent(depth, shape="V", level=0):
    """The reference's progress lines for one cycle of `shape` entered at `level`, in the order of the recursion."""
    if level >= depth:
        print(depth * " " + "direct solving at level %i" % depth)
        return
    print(level * " " + "calling mgCycle at level %i" % level)
    visits = [shape] if (shape == "V" or level + 1 >= depth) else (["F", "V"] if shape == "F" else ["W", "W"])
    for s in visits:
        _announce_descent(depth, s, level + 1)


def mgCycle(A, b, level, R, parameters, initial=None):
    """One cycle (parameters['cycle'], default a V-cycle) entered at `level`; same contract as openmg.mgCycle
    (openmg/__init__.py:151-236): pre-smooth, restrict the residual, recurse, prolong and
    correct, post-smooth; direct solve at parameters['coarsestLevel'].

    A, R are the lists made by operators.coeffecientList / restrictionList (any CSR lists
    of matching shapes work).  Returns (uOut, {'norm': ||b - A[level] uOut||_2}); the norm
    is 0 when `level` is the coarsest.  The device copy of the hierarchy is cached between
    calls (see clear_cache)."""
    if parameters.get("dtype", "float64") == "mixed":
        raise ValueError("parameters['dtype'] = 'mixed' is for mgSolve only (fp64 iterations around fp32 V-cycles); "
                         "mgCycle runs one cycle: use 'float32' or 'float64'")
    shape, alpha = _cycle_of(parameters)
    nullspace = _nullspace_of(parameters)
    coarsest = parameters["coarsestLevel"]
    if coarsest >= len(A) or coarsest > len(R):
        raise IndexError("parameters['coarsestLevel'] = %d but only %d operators / %d restrictions given"
                         % (coarsest, len(A), len(R)))
    code, omega = _smoother_of(parameters)
    on_device = _devarray.is_device_array(b)
    if _devarray.is_device_array(initial) and not on_device:
        raise TypeError("mgCycle: `initial` is a device array but `b` is not; pass both on the device or both on the host")
    if not on_device:
        b = np.asarray(b, dtype=np.float64).reshape(-1)
    if level >= coarsest:
        # the reference's `else` branch (:229-234): direct solve with A[level], norm 0
        if on_device:
            raise ValueError("mgCycle at the coarsest level with device arrays: use solvers.coarseSolve on host arrays")
        return solvers.coarseSolve(A[level], b), {"norm": 0}
    hierarchy = _hierarchy_for(A, R, coarsest + 1, code, omega, _dtype_of(parameters), trust=bool(parameters.get("trustOperators", False)),
                               nullspace=nullspace)
    hierarchy.set_cycle(shape, alpha)          # (the cached hierarchy may have run another setting: a no-op when unchanged)
    if parameters.get("verbose", False):
        _announce_descent(coarsest, shape, level)
    pre = parameters["preIterations"]
    if on_device:
        # b, initial, uOut in HBM: only the norm crosses PCIe (omg_vcycle_dev).  Q2 as on the host: with pre-smoothing the
        # caller's `initial` holds the pre-smoothed iterate afterwards; uOut is a new array (:220 / :224).
        n = hierarchy.sizes[level]
        _devarray.synchronize()
        x_in = None if initial is None else _devarray.address(initial, n, "initial")
        out = _devarray.empty_like(b, n)
        norm = hierarchy.vcycle_dev(_devarray.address(b, n, "b"), x_in, _devarray.address(out, n, "uOut"),
                                    x_in if (x_in is not None and pre > 0) else None, pre, parameters["postIterations"], level=level)
        return out, {"norm": norm}
    x_in = None if initial is None else np.ascontiguousarray(np.asarray(initial, dtype=np.float64).reshape(-1))
    x = np.empty(b.size)                    # uOut is a new array (openmg/__init__.py:220 / :224)
    in_place = (pre > 0 and isinstance(initial, np.ndarray) and initial.dtype == np.float64 and initial.flags.writeable
                and initial.size == b.size and np.shares_memory(initial, initial.reshape(-1)))
    if in_place and np.shares_memory(x_in, initial):
        # Q2: the reference's pre-smoother works IN PLACE on the caller's `initial`
        # (openmg/__init__.py:201 -> solvers.py:68,75): after the call it holds the pre-smoothed
        # iterate.  The device hands that iterate back from the same cycle (omg_vcycle_ex): x_in is read
        # before x_pre is written, so the two may be the caller's one buffer.
        norm = hierarchy.vcycle_ex(b, x_in, x, x_in, pre, parameters["postIterations"], level=level)
    elif in_place:
        smoothed = np.empty(b.size)
        norm = hierarchy.vcycle_ex(b, x_in, x, smoothed, pre, parameters["postIterations"], level=level)
        initial.reshape(-1)[:] = smoothed
    else:
        norm = hierarchy.vcycle_ex(b, x_in, x, None, pre, parameters["postIterations"], level=level)
    return x, {"norm": norm}


mg_cycle = mgCycle   # BASELINE.json's spelling

from ._solver import Solver  # noqa: E402  (it shares the setup and the loops above)
