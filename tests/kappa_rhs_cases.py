"""Shared inputs of tests/test_kappa_rhs_host.py and tests/test_gpu_kappa_rhs.py: tensor-product grids on the unit box
(uniform, or tanh-stretched with chosen ghost widths), a field that is linear in the coordinates with the boundary data
that belong to it, and random data for the bit comparisons.  Not a test module."""
import numpy as np

D, N, P = "dirichlet", "neumann", "periodic"
WALL_NAMES = ("-z", "+z", "-y", "+y", "-x", "+x")
WALL_AXES = ((1, 2), (1, 2), (0, 2), (0, 2), (0, 1), (0, 1))      # the two axes a wall's faces run over

ALPHA, BETA, GAMMA, DELTA = 0.7, -1.3, 0.45, 2.0                   # u = ALPHA x + BETA y + GAMMA z + DELTA


def widths(n, stretch, ghost):
    """n cell widths over [0, 1] — uniform for stretch = 0, else clustered at both ends by a tanh map — with one ghost entry
    at each end: ghost = 'mirror' (the boundary cell's width: the value sits at the mirrored cell centre), or a number."""
    s = np.linspace(-1.0, 1.0, n + 1)
    faces = s if stretch == 0 else np.tanh(stretch * s) / np.tanh(stretch)
    h = np.diff(0.5 * (faces + 1.0))
    lo, hi = (h[0], h[-1]) if ghost == "mirror" else (float(ghost), float(ghost))
    return np.concatenate([[lo], h, [hi]])


def centres(h):
    """The cell centres of the padded width array h (the first cell starts at 0)."""
    faces = np.concatenate([[0.0], np.cumsum(h[1:-1])])
    return 0.5 * (faces[:-1] + faces[1:])


def linear_problem(shape, walls, spacing=None, kappa_x=None, kappa0=1.7):
    """The linear field on `shape` cells of the unit box and the data that make it the exact discrete solution:
    returns (kappa, scale, values, u).  spacing: None (a uniform grid: scale = 1 / h_axis^2, Dirichlet values at the mirrored
    ghost-cell centres, Neumann values q h_axis) or the padded widths (hz, hy, hx).  kappa: the constant kappa0, or
    kappa_x — one value per cell along x, for a field that does not depend on x (ALPHA is then taken as 0) and walls that
    are periodic along x: every y and z face then lies between equal coefficients."""
    alpha = 0.0 if kappa_x is not None else ALPHA
    coef = (GAMMA, BETA, alpha)                                    # du/dz, du/dy, du/dx
    if spacing is None:
        H = tuple(np.full(n + 2, 1.0 / n) for n in shape)
        scale = tuple(float(n) ** 2 for n in shape)
    else:
        H, scale = tuple(np.asarray(h, dtype=np.float64) for h in spacing), (1.0, 1.0, 1.0)
    X = [centres(h) for h in H]
    u = coef[0] * X[0][:, None, None] + coef[1] * X[1][None, :, None] + coef[2] * X[2][None, None, :] + DELTA
    line = np.full(shape[2], kappa0) if kappa_x is None else np.asarray(kappa_x, dtype=np.float64)
    kappa = np.empty(tuple(n + 2 for n in shape))
    kappa[...] = np.concatenate([[line[-1]], line, [line[0]]])[None, None, :]
    values = []
    for w, kind in enumerate(walls):
        axis, hi = w // 2, w % 2
        if kind == P:
            values.append(None)
            continue
        a, b = WALL_AXES[w]
        grids = [None, None, None]
        grids[a] = X[a][:, None]
        grids[b] = X[b][None, :]
        if kind == D:
            # where the operator puts the value: half a ghost width beyond the wall face
            edge = float(np.sum(H[axis][1:-1])) if hi else 0.0
            at = edge + 0.5 * H[axis][-1] if hi else edge - 0.5 * H[axis][0]
            grids[axis] = at
            values.append(np.ascontiguousarray(np.broadcast_to(coef[0] * grids[0] + coef[1] * grids[1] + coef[2] * grids[2] + DELTA,
                                                               (shape[a], shape[b]))))
            continue
        # the outward flux kappa du/dn; without spacing times the cell width along the axis
        k_face = np.broadcast_to(line[None, :] if b == 2 else kappa0, (shape[a], shape[b]))       # (x walls: constant kappa only)
        q = k_face * (coef[axis] if hi else -coef[axis])
        values.append(np.ascontiguousarray(q if spacing is not None else q * H[axis][1]))
    return kappa, scale, values, u


def random_case(shape, walls, kinds, seed=3):
    """Random data for the bit comparisons: kappa over two decades with a ghost layer, and per wall a value of the kind
    named in `kinds` ('none' / 'scalar' / 'field'; a periodic wall gets None whatever is asked)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    kappa = np.exp(rng.uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(10.0))
    values = []
    for w, kind in enumerate(kinds):
        a, b = WALL_AXES[w]
        field = rng.standard_normal((shape[a], shape[b]))
        scalar = float(rng.standard_normal())
        values.append(None if walls[w] == P or kind == "none" else scalar if kind == "scalar" else field)
    return kappa, values


def poison_unread_ghosts(kappa, walls, values):
    """A copy of kappa with NaN in every ghost cell the right-hand side must not read: all of the ghost layer but the face
    layers behind Dirichlet walls that carry a value."""
    out = np.full_like(kappa, np.nan)
    out[1:-1, 1:-1, 1:-1] = kappa[1:-1, 1:-1, 1:-1]
    for w, kind in enumerate(walls):
        if kind != D or values is None or values[w] is None:
            continue
        sel = [slice(1, -1)] * 3
        sel[w // 2] = -1 if w % 2 else 0
        out[tuple(sel)] = kappa[tuple(sel)]
    return out
