"""Shared inputs of tests/test_faces_host.py and tests/test_gpu_faces.py: shapes, wall sets, sigma kinds, random face
coefficients over six decades with NaN on every face the operator must not read, boundary values, and the two sides of the
flux identity with the bound tests/kappa_flux_cases.py uses for the kappa twin.  Not a test module."""
import functools

import numpy as np

from openmg_amd import operators

EPS = np.finfo(np.float64).eps
D, N, P = "dirichlet", "neumann", "periodic"

SHAPES = [(4, 4, 4),        # the smallest with interior rows and every kind of boundary row
          (5, 7, 9),        # odd extents, 315 rows: a ragged last workgroup
          (2, 3, 70),       # more than one wave along x, fewer than two cells along z
          (3, 3, 70),       # ... with room for a periodic z
          (16, 16, 16)]
WALLS = {"dirichlet": (D,) * 6,
         "mixed": (N, D, D, N, D, D),
         "periodic zx": (P, P, D, N, P, P),
         "periodic": (P,) * 6}
SIGMAS = ("none", "scalar", "field")
SCALE = (4.0, 1.0, 0.25)


def takes(shape, walls):
    return all(shape[axis] >= 3 for axis in range(3) if walls[2 * axis] == P)


def assembly_cases():
    return [(shape, wname, skind) for shape in SHAPES for wname, walls in WALLS.items() if takes(shape, walls) for skind in SIGMAS]


def kappa_of(shape, seed=11):
    nz, ny, nx = shape
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(1.0e3))


def widths_of(shape, seed=13):
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(0.5, 2.0, size=n + 2) for n in shape)


def sigma_of(kind, shape, seed=12):
    if kind == "none":
        return None
    if kind == "scalar":
        return 0.375
    return np.random.default_rng(seed).uniform(0.0, 2.0, size=shape)


def unread(shape, walls):
    """Per axis the layers of C that stencil7_faces never reads: a Neumann wall's face, and face e of a periodic axis."""
    out = []
    for axis in range(3):
        layers = []
        if walls[2 * axis] == N:
            layers.append(0)
        if walls[2 * axis + 1] in (N, P):
            layers.append(shape[axis])
        out.append(layers)
    return out


def faces_of(shape, walls, seed=21, poison=True):
    """(Cz, Cy, Cx): exp(U(-1, 1) ln 10^3) per face — six decades —, NaN on every face that is not read (poison)."""
    rng = np.random.default_rng(seed)
    out = []
    for axis, fshape in enumerate(operators.face_shapes(shape)):
        C = np.exp(rng.uniform(-1.0, 1.0, size=fshape) * np.log(1.0e3))
        if poison:
            for m in unread(shape, walls)[axis]:
                sel = [slice(None)] * 3
                sel[axis] = m
                C[tuple(sel)] = np.nan
        out.append(C)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def definition(shape, wname, skind, seed=21):
    """operators.stencil7_faces of the case: computed once, shared, never written to."""
    A = operators.stencil7_faces(faces_of(shape, WALLS[wname], seed), WALLS[wname], sigma_of(skind, shape))
    for a in (A.indptr, A.indices, A.data):
        a.setflags(write=False)
    return A


VALUE_KINDS = {"none": None, "scalars": ("scalar",) * 6, "fields": ("field",) * 6,
               "mixture": ("field", "none", "scalar", "field", "none", "scalar")}


def values_of(shape, walls, kinds, seed=31):
    """Six boundary values of the kinds named (None on periodic walls); kinds None: no values at all."""
    if kinds is None:
        return None
    rng = np.random.default_rng(seed)
    out = []
    for w, kind in enumerate(kinds):
        extent = tuple(shape[a] for a in operators.WALL_FACES[w])
        scalar, field = float(rng.standard_normal()), rng.standard_normal(extent)
        out.append(None if kind == "none" or walls[w] == P else scalar if kind == "scalar" else field)
    return tuple(out)


def solution(shape, seed=41):
    """A random u with signed zeros sprinkled in."""
    u = np.random.default_rng(seed).standard_normal(shape)
    u.ravel()[::5] = 0.0
    u.ravel()[2::7] = -0.0
    return u


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def same_csr(A, B):
    return all(same_bits(getattr(A, name), getattr(B, name)) for name in ("indptr", "indices", "data"))


def identity_sides(faces, u, walls, values, sigma):
    """(left, right, bound) of  divergence_faces(flux_faces(u)) + sigma u = A u - rhs_faces(None, values), per cell; the bound
    is kappa_flux_cases.identity_sides' own, 32 eps (|A| |u| + |b|)."""
    A = operators.stencil7_faces(faces, walls, sigma)
    b = operators.rhs_faces(faces, None, walls, values)
    left = operators.divergence_faces(*operators.flux_faces(faces, u, walls, values))
    if sigma is not None:
        left = left + np.broadcast_to(np.asarray(sigma, dtype=np.float64), u.shape) * u
    right = (A @ u.ravel()).reshape(u.shape) - b
    bound = 32 * EPS * ((abs(A) @ np.abs(u.ravel())).reshape(u.shape) + np.abs(b))
    return left, right, bound
