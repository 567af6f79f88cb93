"""openmg_amd.Solver: mgSolve's setup once, then many right-hand sides on the hierarchy it built.

    s = openmg_amd.Solver(A_in, parameters)     # restrictions, Galerkin products, upload, qualification: once
    u, info = s.solve(b, initial=None, out=None, **overrides)
    z = s.apply(r, out=None)                    # one zero-start cycle, z = M r (a preconditioner for the caller's own iteration)
    s.update(A_new)                             # new values in the same pattern
    s = openmg_amd.Solver.from_kappa(kappa, parameters, walls, sigma, scale)    # the 7-point operator of a coefficient field,
    s.update_kappa(kappa_new, sigma=None)       # ... assembled in HBM (operators.stencil7_kappa: the definition)
    b = s.rhs(kappa, f=None, values=None)       # ... and its right-hand side: source, boundary values, fluxes (operators.rhs_kappa)
    Fz, Fy, Fx = s.fluxes(kappa, u, values=None, out=None, alpha=None)     # the face fluxes of a solution (operators.flux_kappa)
    d = s.divergence((Fz, Fy, Fx), out=None)    # ... and the cell balance of face arrays (operators.divergence_faces)
    s = openmg_amd.Solver.from_faces((Cz, Cy, Cx), parameters, walls, sigma)    # the same line from one coefficient per FACE
    s.update_faces((Cz, Cy, Cx), sigma=None)    # ... (operators.stencil7_faces); rhs and fluxes then take the three arrays
    y = s.matvec(x, out=None)                   # y = A x on the operator as the hierarchy holds it (b - A u where u lives)
    s = openmg_amd.Solver(A_in, parameters, projection=8)       # every solve starts from its projection onto up to 8 earlier
    x0 = s.project(b); s.projection_size; s.projection_basis(); s.projection_clear()      # ... solutions kept in HBM
    s.close()                                   # also a context manager

The setup and the two loops are mgSolve's own (openmg_amd._setup, _solve_cycles, _solve_cg): a solve from zero has the
bits of mgSolve(A_in, b, parameters).  What a solve leaves on the device is the resident b and x, the cycle setting and
the FCG vectors; the next solve loads b and x again, sets the cycle again and FCG starts from its own set-up, so that no
solve sees anything of an earlier one.  Not thread safe; one GPU; b is one vector.
"""
import math

import numpy as np

from . import _devarray, _hip

# the keys a solve may override: those that do not define the hierarchy ('smoother', 'lineAxis', 'coarsening', 'oddExtents', 'dtype', 'nullspace',
# the grids do, and are refused)
SOLVE_KEYS = ("cycles", "threshold", "rtol", "preIterations", "postIterations", "accel", "cycle", "overCorrection")


def stop_target(cycles, threshold, rtol, rhs_norm=None):
    """The residual norm a solve stops below: max(threshold, rtol * rhs_norm), 0.0 when neither rule is on (then only
    `cycles` stops it).  ValueError when all three rules are off or rtol is not a finite number >= 0.  rhs_norm None:
    the check alone (before any device work).  A right-hand side whose norm is not finite leaves the threshold alone:
    the first cycle's norm then reports it."""
    try:
        rtol = float(rtol)
    except (TypeError, ValueError):
        raise ValueError("rtol must be a finite number >= 0, not %r" % (rtol,))
    if not math.isfinite(rtol) or rtol < 0.0:
        raise ValueError("rtol must be a finite number >= 0, not %r" % (rtol,))
    if not (threshold > 0 or rtol > 0.0 or cycles > 0):
        raise ValueError("Either 'threshold', 'rtol' or 'cycles' must be > 0.")
    if rhs_norm is None:
        return None
    target = float(threshold) if threshold > 0 else 0.0
    relative = rtol * rhs_norm
    return relative if relative > target else target


def _host_out(out, n):
    """A new result array, or the caller's `out` checked: writeable contiguous float64 of n entries."""
    if out is None:
        return np.empty(n)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable and out.size == n):
        raise ValueError("out must be a writeable contiguous float64 array of %d entries" % n)
    return out


def _check_keys(parameters):
    """ValueError for a value mgSolve would refuse — before any device work, GPU or not."""
    from . import _accel_of, _coarsening_of, _cycle_of, _dtype_of, _nullspace_of, _smoother_of
    _accel_of(parameters)
    _coarsening_of(parameters)
    _cycle_of(parameters)
    _nullspace_of(parameters)
    _smoother_of(parameters)
    try:
        _dtype_of(parameters)
    except TypeError:
        raise ValueError("parameters['dtype'] must be 'float64', 'float32' or 'mixed', not %r" % (parameters.get("dtype"),))


PROJECTION_MAX = 64


def _projection_of(projection):
    """The capacity `projection` asks for: 0 (also for None), or an integer in 1..64; anything else: ValueError."""
    if projection is None:
        return 0
    if isinstance(projection, (bool, np.bool_)) or not isinstance(projection, (int, np.integer)) or not 0 <= projection <= PROJECTION_MAX:
        raise ValueError("projection must be None or an integer in 0..%d (the earlier solutions kept), not %r" % (PROJECTION_MAX, projection))
    return int(projection)


class Solver:
    """A hierarchy set up once for A_in and `parameters` (every key mgSolve understands, and 'rtol'), solving many
    right-hand sides.  .parameters: the solver's own completed copy (the caller's dict and openmg_amd.defaults are not
    touched); .hierarchy: the _hip.Hierarchy; .A / .R: the operator lists when parameters['giveInfo'] asked for the
    lists route, else None.

    projection = L (1..64): every solve starts from the A-best approximation of its solution in the span of up to L
    earlier solutions kept in HBM as an A-orthonormal set, and adds what it found beyond that to the set (Fischer's
    projection for successive right-hand sides; a full set restarts from the last solution).  0 or None: none is kept
    and no solve differs from before."""

    def __init__(self, A_in, parameters, *, projection=0):
        from . import _setup, defaults
        self._hierarchy = None
        given = dict(parameters)
        _check_keys(given)
        self._capacity = _projection_of(projection)
        stop_target(1, 0.0, given.get("rtol", 0.0))                 # (rtol alone: the stop rules are checked per solve)
        self._given = given
        completed = dict(given)
        self._hierarchy, self.R, self.A = _setup(A_in, completed, dict(defaults))[:3]
        completed.setdefault("rtol", 0.0)
        self.parameters = completed
        self._pattern_of(A_in)
        if self._capacity:
            try:
                self._hierarchy.projection(self._capacity)
            except Exception:
                self.close()
                raise

    _kappa = None              # from_kappa: (problemShape, walls, scale, spacing) of construction, else None
    _capacity = 0              # projection: the vectors the set may hold (0: no set) ...
    _basis = 0                 # ... and how many it holds

    @classmethod
    def from_kappa(cls, kappa, parameters, walls=None, sigma=None, scale=(1.0, 1.0, 1.0), spacing=None, *, projection=0):
        """The Solver of operators.stencil7_kappa(kappa, walls, sigma, scale, spacing) — same bits — from the coefficient
        field itself: kappa float64 (nz + 2, ny + 2, nx + 2), the cells and one ghost layer, and sigma (None, a scalar, an
        array of problemShape) as NumPy arrays or device arrays.  spacing: None, or the cell widths (hz, hy, hx) of a
        stretched tensor-product grid (operators.spacing_arguments: host arrays, in place of scale); the operator is then the
        volume-integrated one and the right-hand side f * operators.cell_volumes(spacing); the widths are kept for
        update_kappa and have no say in the route.  parameters['problemShape'] is taken from kappa; if given it
        must agree.  Where the setup takes the plain device route (the colour smoother, no giveInfo / verbose / dense, no
        'coarsening' / 'oddExtents', a shape the device setup takes) level 0 is assembled in HBM and no host matrix is ever
        made; with any other parameters the operator is assembled on the device into host arrays and the setup runs as for
        any A_in.  ValueError for bad arguments before any device work; a kappa or sigma value out of range: HipError
        (ERR_INVALID) naming the first such cell.

        walls may name 'periodic' for both walls of an axis (extent >= 3): the operator then holds the wrap-around
        couplings, assembled in HBM like every other; no fused pass takes such a level, so the hierarchy is the one
        Solver(operators.stencil7_kappa(...), parameters) builds by the ordinary route, update_kappa builds a new
        hierarchy, and update(A_new) wants A_new in the periodic pattern.  With every wall periodic or Neumann and no
        sigma the operator is singular: parameters['nullspace'] = 'constant'.  'smoother': 'line' and 'coarsening':
        'auto' read the grid off the in-grid pattern and raise HipError (ERR_UNSUPPORTED) on a periodic operator, as they
        do for a periodic matrix; named 'coarsening' factors and 'oddExtents' work."""
        _projection_of(projection)
        source = _hip.KappaArgs(kappa, walls, sigma, scale, spacing)
        given = dict(parameters)
        if given.get("problemShape") is not None:
            try:
                same = tuple(int(s) for s in given["problemShape"]) == source.grid
            except TypeError:
                same = False
            if not same:
                raise ValueError("parameters['problemShape'] = %r is not kappa's grid %r" % (given["problemShape"], source.grid))
        given["problemShape"] = source.grid
        self = cls(source, given, projection=projection)
        self._kappa = (source.grid, walls, scale, source.spacing)
        return self

    _faces = None              # from_faces: (problemShape, walls) of construction, else None

    @classmethod
    def from_faces(cls, faces, parameters, walls=None, sigma=None, *, projection=0):
        """The Solver of operators.stencil7_faces(faces, walls, sigma) — same bits — from one coefficient per FACE: faces =
        (Cz, Cy, Cx), float64 arrays of the shapes operators.face_shapes(problemShape) — the arrays fluxes() writes and
        divergence() reads —, all NumPy arrays or all device arrays; sigma None, a scalar or an array of problemShape.  For
        callers whose coefficients live on the faces: a MAC grid's 1 / rho from face fractions or an arithmetic mean,
        orthotropic media (another field per axis), metric factors.  The coefficients carry every factor (the face area over
        the distance, the time step): there is no scale and no spacing.  A Neumann wall's faces and face e of a periodic axis
        are never read.  parameters['problemShape'] is taken from the arrays; if given it must agree.  The routes are
        from_kappa's: on the plain device route level 0 is assembled in HBM and no host matrix is ever made, with any other
        parameters the operator is assembled on the device into host arrays and the setup runs as for any A_in; periodic
        walls give the ordinary route's hierarchy, and 'smoother': 'line' and 'coarsening': 'auto' raise HipError
        (ERR_UNSUPPORTED) on a periodic operator.  ValueError for bad arguments before any device work; a coefficient that is
        read and is not finite and > 0 (zero, a blocked face, included) or a sigma value out of range: HipError (ERR_INVALID)
        naming the face."""
        _projection_of(projection)
        source = _hip.FaceArgs(faces, walls, sigma)
        given = dict(parameters)
        if given.get("problemShape") is not None:
            try:
                same = tuple(int(s) for s in given["problemShape"]) == source.grid
            except TypeError:
                same = False
            if not same:
                raise ValueError("parameters['problemShape'] = %r is not the face arrays' grid %r" % (given["problemShape"], source.grid))
        given["problemShape"] = source.grid
        self = cls(source, given, projection=projection)
        self._faces = (source.grid, walls)
        return self

    def _pattern_of(self, A_in):
        if isinstance(A_in, (_hip.KappaArgs, _hip.FaceArgs)):
            # (the in-grid 7-point pattern: formed on the host when update(A_new) first asks for it)
            self._shape, self._indptr, self._indices = A_in.shape, None, None
            return
        A0 = _hip.as_csr(A_in)
        self._shape, self._indptr, self._indices = A0.shape, A0.indptr, A0.indices

    # ---- life cycle -------------------------------------------------------------------------------------------------
    @property
    def hierarchy(self):
        """The _hip.Hierarchy the solver runs on (level_flags and the other probes)."""
        return self._open()

    def _open(self):
        if self._hierarchy is None:
            raise RuntimeError("this Solver has been closed")
        return self._hierarchy

    def close(self):
        """Free the device hierarchy; a second call does nothing, any other call afterwards raises RuntimeError."""
        h, self._hierarchy = getattr(self, "_hierarchy", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        self._open()
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- solve --------------------------------------------------------------------------------------------------------
    def solve(self, b, initial=None, out=None, project=None, **overrides):
        """Solve A u = b from `initial` (None: zero).  Stops below max(threshold, rtol * ||b||) or after `cycles` (> 0)
        cycles / FCG iterations; a start that is already below the target returns at once with info['cycle'] == 0.
        overrides: SOLVE_KEYS, for this call only.  b, initial, out: host arrays, or contiguous float64 device arrays
        (then u is a device array: `out`, or a new one of b's kind).  With a null space b is projected on the device
        (rhs_norm and every norm are the projected system's), `initial` is taken as it is and u has mean 0.

        Returns (u, info): info['cycle'], ['norm'] (mgSolve's meaning: the true fp64 norm for 'cg' and 'mixed'),
        ['norms'] (one per cycle or iteration), ['rhs_norm'], ['initial_norm'].  A norm that is not finite raises
        RuntimeError naming the cycle; the solver stays usable.

        project (None: on exactly when the solver was made with projection=L > 0; True without that: ValueError): the
        solve starts from the projection of the solution onto the earlier ones — after b is loaded (and projected, with a
        null space) the iterate becomes sum_i (x_i . b) x_i over the set —, runs the same loop from there, and what it
        added to that start joins the set afterwards (nothing does when no cycle ran).  info['initial_norm'] is then the
        projected start's residual, and a start that already meets the target returns with info['cycle'] == 0.
        `initial` together with a projected start: ValueError — pass project=False for that solve, which leaves the set
        alone.  On a solver with a set info also has ['projected'], the vectors this solve started from, and ['basis'],
        the set's size afterwards."""
        from . import _accel_of, _cycle_of, _solve_cg, _solve_cycles
        h = self._open()
        if project is None:
            project = self._capacity > 0
        elif project and not self._capacity:
            raise ValueError("Solver.solve: project=True needs a solver made with projection=L (1..%d)" % PROJECTION_MAX)
        if project and initial is not None:
            raise ValueError("Solver.solve: `initial` and the projected start exclude each other: pass project=False for this solve")
        for key in overrides:
            if key not in SOLVE_KEYS:
                raise ValueError("solve() cannot override %r (it defines the hierarchy); allowed: %s" % (key, ", ".join(SOLVE_KEYS)))
        p = dict(self.parameters, **overrides)
        accel = _accel_of(p)
        shape, alpha = _cycle_of(p)
        pre, post = int(p["preIterations"]), int(p["postIterations"])
        if pre < 0 or post < 0:
            raise ValueError("preIterations and postIterations must be >= 0")
        cycles, threshold, rtol = p["cycles"], p["threshold"], p["rtol"]
        stop_target(cycles, threshold, rtol)
        n = h.sizes[0]
        on_device = _devarray.is_device_array(b)
        if _devarray.is_device_array(initial) != (on_device and initial is not None):
            raise TypeError("Solver.solve: `b` and `initial` must both be device arrays or both be host arrays")
        if out is not None and _devarray.is_device_array(out) != on_device:
            raise TypeError("Solver.solve: `out` must be a device array exactly when `b` is one")
        verbose = p["verbose"]

        h.set_cycle(shape, alpha)
        if on_device:
            if out is not None:
                _devarray.address(out, n, "out")                    # (a wrong `out` is refused before the solve, not after)
            _devarray.synchronize()
            h.resident_load_dev(_devarray.address(b, n, "b"), None if initial is None else _devarray.address(initial, n, "initial"))
        else:
            out = _host_out(out, n)
            h.resident_load(np.asarray(b, dtype=np.float64).reshape(-1), initial)
        used = h.resident_project() if project else 0
        # ||b|| as it is held, and the start's residual: from zero (no `initial`, an empty set) that is ||b|| itself (no SpMV)
        from_zero = initial is None and used == 0
        rhs_norm, initial_norm = h.resident_norms(rhs=True, residual=not from_zero)
        if from_zero:
            initial_norm = rhs_norm
        target = stop_target(cycles, threshold, rtol, rhs_norm)
        norms = []

        def observe(k, value):
            norms.append(float(value))
            if not math.isfinite(value):
                raise RuntimeError("Solver.solve: the residual norm of cycle %d is not finite (%r)" % (k, value))

        if target > 0.0 and (initial_norm < target or initial_norm == 0.0):
            cycle, norm = 0, initial_norm
        else:
            loop = dict(p, cycles=cycles, threshold=target)
            run = _solve_cg if accel == "cg" else _solve_cycles
            cycle, norm = run(h, loop, pre, post, self.parameters["coarsestLevel"], verbose, shape, observe)
            if not math.isfinite(norm):
                raise RuntimeError("Solver.solve: the residual norm after cycle %d is not finite (%r)" % (cycle, norm))
        if project and cycle > 0:
            self._basis = h.resident_project_update()[0]
        if on_device:
            u = _devarray.empty_like(b, n) if out is None else out
            h.resident_fetch_dev(_devarray.address(u, n, "out"))
        else:
            u = h.resident_fetch(out)
        info = {"cycle": cycle, "norm": norm, "norms": norms, "rhs_norm": rhs_norm, "initial_norm": initial_norm}
        if self._capacity:
            info["projected"], info["basis"] = used, self._basis
        if _hip.is_line_smoother(h.smoother):
            info["lineAxis"] = h.line_axis          # ('smoother': 'line': the axis of the lines, an index into problemShape)
        if h.coarsening is not None:
            info["coarsening"] = list(h.coarsening)   # ('coarsening': the factors of every restriction, every level's grid)
            info["levelShapes"] = list(h.level_shapes)
        return u, info

    # ---- projection ---------------------------------------------------------------------------------------------------
    def project(self, b, out=None):
        """The start a solve of b would take: sum_i (x_i . b) x_i over the set as it stands (zeros while it is empty);
        with a null space b is projected first, as solve() does.  The set is not changed.  b, out: host arrays, or device
        arrays (then the result is a device array), under apply()'s rules.  ValueError on a solver without a set."""
        h = self._open()
        if not self._capacity:
            raise ValueError("Solver.project: needs a solver made with projection=L (1..%d)" % PROJECTION_MAX)
        n = h.sizes[0]
        on_device = _devarray.is_device_array(b)
        if out is not None and _devarray.is_device_array(out) != on_device:
            raise TypeError("Solver.project: `out` must be a device array exactly when `b` is one")
        if on_device:
            x = _devarray.empty_like(b, n) if out is None else out
            b_ptr, x_ptr = _devarray.address(b, n, "b"), _devarray.address(x, n, "out")
            _devarray.synchronize()
            h.resident_load_dev(b_ptr, None)
            h.resident_project()
            h.resident_fetch_dev(x_ptr)
            return x
        x = _host_out(out, n)
        h.resident_load(np.asarray(b, dtype=np.float64).reshape(-1), None)
        h.resident_project()
        return h.resident_fetch(x)

    @property
    def projection_size(self):
        """How many earlier solutions the set holds now (0 .. the capacity; always 0 without one)."""
        self._open()
        return self._basis

    def projection_clear(self):
        """Empty the set; the capacity stays.  The next solve starts from zero, with the bits of a fresh solver's."""
        h = self._open()
        self._basis = 0
        if self._capacity:
            h.projection(self._capacity)

    def projection_basis(self):
        """The set as a list of host arrays in the caller's numbering: x_i^T A x_j = delta_ij."""
        h = self._open()
        return [h.projection_fetch(i) for i in range(self._basis)]

    # ---- apply --------------------------------------------------------------------------------------------------------
    def apply(self, r, out=None):
        """z = M r: one cycle from zero with the construction's sweep counts, cycle shape and over-correction factor —
        mgCycle(A, r, 0, R, ...)[0] without its checksum of the lists.  Nothing is projected.  r, out: host arrays, or
        device arrays (then z is a device array).  ValueError on a mixed hierarchy."""
        from . import _cycle_of
        h = self._open()
        if h.dtype == _hip.DTYPE_MIXED:
            raise ValueError("parameters['dtype'] = 'mixed' is for solve() (fp64 iterations around fp32 cycles); "
                             "apply runs one cycle: use 'float32' or 'float64'")
        p = self.parameters
        shape, alpha = _cycle_of(p)
        pre, post = int(p["preIterations"]), int(p["postIterations"])
        n = h.sizes[0]
        on_device = _devarray.is_device_array(r)
        if out is not None and _devarray.is_device_array(out) != on_device:
            raise TypeError("Solver.apply: `out` must be a device array exactly when `r` is one")
        h.set_cycle(shape, alpha)
        if on_device:
            z = _devarray.empty_like(r, n) if out is None else out
            r_ptr, z_ptr = _devarray.address(r, n, "r"), _devarray.address(z, n, "out")
            _devarray.synchronize()
            h.cycle_dev(r_ptr, z_ptr, pre, post)
            h.sync()
            return z
        z = _host_out(out, n)
        h.vcycle_ex(np.asarray(r, dtype=np.float64).reshape(-1), None, z, None, pre, post, level=0)
        return z

    # ---- matvec -------------------------------------------------------------------------------------------------------
    def matvec(self, x, out=None):
        """y = A x with the operator as the hierarchy holds it (level 0, the caller's numbering): the A p a Krylov
        iteration around apply() needs, and b - A u where u lives — on the plain device route of from_kappa no host matrix
        exists to form either with.  x, out: host arrays (Hierarchy.spmv(0, x); like every single-level host entry this
        gives up what a resident_load left on the device), or device arrays (then y is a device array, `out` may be x, and the
        resident right-hand side and iterate are not touched: omg_level_spmv_dev).  The argument rules of apply();
        ValueError on a mixed hierarchy."""
        h = self._open()
        if h.dtype == _hip.DTYPE_MIXED:
            raise ValueError("parameters['dtype'] = 'mixed' is for solve() (fp64 iterations around fp32 cycles); "
                             "matvec would apply the fp32 operator: use 'float32' or 'float64'")
        n = h.sizes[0]
        on_device = _devarray.is_device_array(x)
        if out is not None and _devarray.is_device_array(out) != on_device:
            raise TypeError("Solver.matvec: `out` must be a device array exactly when `x` is one")
        if on_device:
            y = _devarray.empty_like(x, n) if out is None else out
            x_ptr, y_ptr = _devarray.address(x, n, "x"), _devarray.address(y, n, "out")
            _devarray.synchronize()
            h.spmv_dev(0, x_ptr, y_ptr)
            return y
        y = _host_out(out, n)
        y[...] = h.spmv(0, np.asarray(x, dtype=np.float64).reshape(-1)).reshape(y.shape)
        return y

    # ---- right-hand side ----------------------------------------------------------------------------------------------
    def rhs(self, kappa, f=None, values=None, out=None):
        """The right-hand side b that goes with the operator of a Solver made by from_kappa (ValueError otherwise, like
        update_kappa): operators.rhs_kappa(kappa, f, walls, values, scale, spacing) — same bits — made on the device, with
        the walls, scale and spacing of construction; kappa's grid must be the solver's.  f: the source per cell (None, a
        scalar, an array of problemShape); values: None or six entries in the order of the walls, each None, a scalar or a
        2-D array over that wall's faces — a Dirichlet wall's boundary value, a Neumann wall's outward flux kappa du/dn
        (without spacing: times the cell width along that axis); a periodic wall takes None.  kappa, f and the value fields
        are NumPy arrays or all device arrays (then b is a device array: `out`, which may be f, or a new one).  Returns b
        flattened to n entries in the solver's numbering, ready for solve().

        Nothing is projected here.  With parameters['nullspace'] = 'constant' (every wall Neumann or periodic, no sigma)
        solve() projects b; the problem itself has a solution only if the data are compatible, sum(b) = 0 — the integral
        of f over the box plus the fluxes into it through the Neumann walls vanish —, which the caller's f and fluxes
        should meet: what solve() removes otherwise is the part of the data no u can answer.

        On a Solver made by from_faces `kappa` is the three coefficient arrays (Cz, Cy, Cx) and b has the bits of
        operators.rhs_faces(faces, f, walls, values): a Dirichlet value enters with the wall face's coefficient, a Neumann
        value is the outward flux through the face already integrated over it and enters with no factor."""
        self._open()
        if self._faces is not None:
            b = _hip.faces_rhs(self._own_faces("rhs", kappa), f, self._faces[1], values, out)
            return b.reshape(-1) if out is None else b
        if self._kappa is None:
            raise ValueError("Solver.rhs: the solver was not made by Solver.from_kappa or Solver.from_faces")
        grid, walls, scale, spacing = self._kappa
        k_shape = tuple(int(s) for s in (kappa.__cuda_array_interface__["shape"] if _devarray.is_device_array(kappa) else np.shape(kappa)))
        if k_shape != tuple(s + 2 for s in grid):
            raise ValueError("Solver.rhs: kappa's shape %r is not the solver's grid %r with one ghost layer" % (k_shape, grid))
        b = _hip.kappa_rhs(kappa, f, walls, values, scale, spacing, out)
        return b.reshape(-1) if out is None else b

    # ---- face fluxes --------------------------------------------------------------------------------------------------
    def fluxes(self, kappa, u, values=None, out=None, alpha=None):
        """The face fluxes (Fz, Fy, Fx) of u under the operator of a Solver made by from_kappa (ValueError otherwise, like
        rhs): operators.flux_kappa(kappa, u, walls, values, scale, spacing) — same bits — made on the device in one launch,
        with the walls, scale and spacing of construction; kappa's grid must be the solver's.  F is the flux of
        -kappa grad u along +z, +y, +x through every face — shapes (nz + 1, ny, nx), (nz, ny + 1, nx), (nz, ny, nx + 1) —
        with the operator's own coefficients and factor (scale[axis]; with spacing the face area), so that
        divergence(fluxes(kappa, u, values)) (+ the sigma term) = matvec(u) - rhs(kappa, None, values) to rounding.
        u: flat, as solve returns it, or in problemShape; values: the boundary data as rhs takes them (a Dirichlet wall
        without a value: 0; a Neumann wall's value: the outward flux kappa du/dn, without spacing times the cell width
        along that axis — its face gets +value area at the low wall, -value area at the high wall).  kappa, u and the value
        fields are NumPy arrays or all device arrays.  out: three arrays to write into, on the same side; alpha (needs
        out): out = out + alpha * F — the velocity correction of a projection step is fluxes(kappa, p, out=W, alpha=-1.0).
        An `out` that overlaps u or kappa is refused.  Nothing is projected, a resident solve is not disturbed and the
        hierarchy is not touched.

        On a Solver made by from_faces `kappa` is the three coefficient arrays (Cz, Cy, Cx) and the result has the bits of
        operators.flux_faces(faces, u, walls, values) — F = C (u_lo - u_hi), the coefficient loaded from the face's own
        place; an `out` that overlaps one of them is refused."""
        self._open()
        if self._faces is not None:
            return _hip.faces_flux(self._own_faces("fluxes", kappa), u, self._faces[1], values, out, alpha)
        if self._kappa is None:
            raise ValueError("Solver.fluxes: the solver was not made by Solver.from_kappa or Solver.from_faces")
        grid, walls, scale, spacing = self._kappa
        k_shape = tuple(int(s) for s in (kappa.__cuda_array_interface__["shape"] if _devarray.is_device_array(kappa) else np.shape(kappa)))
        if k_shape != tuple(s + 2 for s in grid):
            raise ValueError("Solver.fluxes: kappa's shape %r is not the solver's grid %r with one ghost layer" % (k_shape, grid))
        return _hip.kappa_flux(kappa, u, walls, values, scale, spacing, out, alpha)

    def divergence(self, faces, out=None):
        """The cell balance of three face arrays (Fz, Fy, Fx) of the solver's grid, operators.divergence_faces — same bits —
        made on the device: ((Fz[k+1] - Fz[k]) + (Fy[j+1] - Fy[j])) + (Fx[i+1] - Fx[i]) per cell.  For a Solver made by
        from_kappa or from_faces (ValueError otherwise); the arrays are NumPy arrays or all device arrays, `out` an array of n entries on
        their side.  Returns the balance flattened to n entries in the solver's numbering, ready for solve() — the
        right-hand side of a projection step is divergence(W) of the face velocities times area."""
        self._open()
        if self._kappa is None and self._faces is None:
            raise ValueError("Solver.divergence: the solver was not made by Solver.from_kappa or Solver.from_faces")
        grid = tuple((self._kappa or self._faces)[0])
        from . import operators
        try:
            shapes = tuple(tuple(int(s) for s in (a.__cuda_array_interface__["shape"] if _devarray.is_device_array(a) else np.shape(a)))
                           for a in faces)
        except TypeError:
            raise ValueError("Solver.divergence: `faces` must be three face arrays (Fz, Fy, Fx)")
        if shapes != operators.face_shapes(grid):
            raise ValueError("Solver.divergence: the face arrays' shapes %r are not those of the solver's grid %r" % (shapes, grid))
        d = _hip.face_divergence(faces, out)
        return d.reshape(-1) if out is None else d

    # ---- update -------------------------------------------------------------------------------------------------------
    def update(self, A_new):
        """New values in A_in's pattern (the same indptr and indices; anything else: ValueError, and the solver keeps
        the old operator).  Where the hierarchy takes new coefficients in place (_hip.Hierarchy.can_update_fine) that
        is update_fine; otherwise a new hierarchy is built first and the old one closed after that succeeded.  Either
        way later solves have the bits of a fresh Solver(A_new, parameters).  With parameters['coarsening'] the new
        hierarchy is built with the FACTORS CHOSEN AT CONSTRUCTION ('auto' is not asked again: sizes and patterns cannot
        change under the caller), always as a new hierarchy: a semicoarsened one takes no update in place.  The same holds
        with parameters['oddExtents'] = 'merge': the factors and the key are kept, the hierarchy is built anew."""
        h = self._open()
        A1 = _hip.as_csr(A_new)
        if self._indptr is None:
            from . import operators
            grid, walls = (self._kappa or self._faces)[:2]
            if walls is not None and "periodic" in tuple(walls):
                # (the pattern with the wrapped columns: the definition's own, of a field of ones; from_faces has the same)
                P = operators.stencil7_kappa(np.ones(tuple(s + 2 for s in grid)), walls)
            else:
                P = operators.stencil_poisson(grid)
            self._indptr, self._indices = P.indptr, P.indices
        if (A1.shape != self._shape or A1.indptr.size != self._indptr.size or A1.indices.size != self._indices.size
                or not np.array_equal(A1.indptr, self._indptr) or not np.array_equal(A1.indices, self._indices)):
            raise ValueError("Solver.update: A_new must have the pattern (indptr and indices) the solver was set up with")
        if h.can_update_fine():
            self._basis = 0                                         # (update_fine empties the set: it was A-orthonormal for the old operator)
            h.update_fine(A1.data)
            return
        self._rebuild(A_new)
        self._pattern_of(A1)

    def _rebuild(self, A_new):
        """A new hierarchy for A_new with the construction's parameters (and factors); the old one is closed after that succeeded."""
        from . import _setup, defaults
        h = self._open()
        given = dict(self._given)
        if h.coarsening is not None:
            given["coarsening"] = list(h.coarsening)
            given["gridLevels"] = len(h.coarsening)  # (the depth built: the list is consumed exactly)
            given.pop("coarsestLevel", None)
        fresh, R, A = _setup(A_new, given, dict(defaults))[:3]
        if self._capacity:
            try:
                fresh.projection(self._capacity)                    # (an empty set of the same capacity)
            except Exception:
                fresh.close()
                raise
        self._hierarchy, self.R, self.A, self._basis = fresh, R, A, 0
        h.close()

    def _own_faces(self, what, faces):
        """`faces` checked as three arrays in the face shapes of the solver's grid (a from_faces solver), as a tuple."""
        from . import operators
        grid = self._faces[0]
        try:
            faces = tuple(faces)
            shapes = tuple(tuple(int(s) for s in (a.__cuda_array_interface__["shape"] if _devarray.is_device_array(a) else np.shape(a)))
                           for a in faces)
        except TypeError:
            raise ValueError("Solver.%s: on a solver made by Solver.from_faces the coefficients are three face arrays (Cz, Cy, Cx)" % what)
        if shapes != operators.face_shapes(grid):
            raise ValueError("Solver.%s: the coefficient arrays' shapes %r are not the face shapes of the solver's grid %r" % (what, shapes, grid))
        return faces

    def update_faces(self, faces, sigma=None):
        """update() with the operator of new face coefficients (and sigma), for a Solver made by from_faces (ValueError
        otherwise); the walls are those of construction.  Where the hierarchy takes new coefficients in place the values are
        made on the device and go straight into update_fine — with device arrays nothing crosses to the host; otherwise
        (periodic walls, 'coarsening', ...) the operator is assembled into host arrays and a new hierarchy built as update()
        does.  Either way later solves have the bits of a fresh Solver.from_faces(faces, parameters, ...), and the
        projection set is emptied.  Refused coefficients leave the solver with the old operator."""
        h = self._open()
        if self._faces is None:
            raise ValueError("Solver.update_faces: the solver was not made by Solver.from_faces")
        grid, walls = self._faces
        source = _hip.FaceArgs(self._own_faces("update_faces", faces), walls, sigma)
        if h.can_update_fine():
            self._basis = 0
            h.update_faces(source)
            return
        self._rebuild(source)

    def update_kappa(self, kappa, sigma=None):
        """update() with the operator of a new coefficient field (and sigma), for a Solver made by from_kappa; walls,
        scale and spacing are those of construction.  Where the hierarchy takes new coefficients in place the values are made on the
        device and go straight into update_fine — with device arrays nothing crosses to the host; otherwise the operator
        is assembled into host arrays and a new hierarchy built as update() does.  Either way later solves have the bits of
        a fresh Solver.from_kappa(kappa, parameters, ...).  A refused field leaves the solver with the old operator."""
        h = self._open()
        if self._kappa is None:
            raise ValueError("Solver.update_kappa: the solver was not made by Solver.from_kappa")
        grid, walls, scale, spacing = self._kappa
        source = _hip.KappaArgs(kappa, walls, sigma, scale, spacing)
        if source.grid != grid:
            raise ValueError("Solver.update_kappa: kappa's grid %r is not the solver's %r" % (source.grid, grid))
        if h.can_update_fine():
            self._basis = 0
            h.update_kappa(source)
            return
        self._rebuild(source)
