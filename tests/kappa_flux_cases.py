"""Shared inputs of tests/test_kappa_flux_host.py and tests/test_gpu_kappa_flux.py: the shapes, wall sets, value kinds and
grid variants of the right-hand side's bit test (tests/test_gpu_kappa_rhs.py), a solution with signed zeros in it, the
poisoning of every ghost cell the fluxes must not read, and the two sides of the discrete identity with its bound.  Not a
test module."""
import numpy as np

from openmg_amd import operators

import kappa_rhs_cases as rc
from kappa_rhs_cases import D, N, P

EPS = np.finfo(np.float64).eps

SHAPES = [(1, 1, 1),
          (1, 5, 7),
          (3, 3, 3),
          (5, 6, 9),        # 270 cells: a workgroup boundary inside a line and a ragged last group
          (4, 8, 16),       # exactly two groups
          (2, 3, 257)]      # a line longer than a workgroup; face rows of nx + 1 = 258
WALLSETS = {"dirichlet": (D,) * 6, "neumann": (N,) * 6, "mixed": (N, D, D, N, D, N),
            "periodic x": (D, N, N, D, P, P), "periodic y": (N, D, P, P, D, N), "periodic z": (P, P, D, N, N, D),
            "periodic xyz": (P,) * 6}
VALUE_KINDS = {"none": None, "scalars": ("scalar",) * 6, "fields": ("field",) * 6,
               "mixture": ("field", "none", "scalar", "field", "none", "scalar")}
SCALE = (0.3, 1.7, 2.9)


def takes(shape, walls):
    return all(shape[axis] >= 3 for axis in range(3) if walls[2 * axis] == P)


def grids_of(shape):
    """scale factors; cell widths with ghost widths 0; cell widths with ghost widths that are not 0"""
    return [dict(scale=SCALE),
            dict(spacing=tuple(rc.widths(n, 1.3, 0.0) for n in shape)),
            dict(spacing=(rc.widths(shape[0], 1.3, "mirror"), rc.widths(shape[1], 0.0, 0.021), rc.widths(shape[2], 1.7, "mirror")))]


def solution(shape, seed=41):
    """A random u with signed zeros sprinkled in."""
    u = np.random.default_rng(seed).standard_normal(shape)
    u.ravel()[::5] = 0.0
    u.ravel()[2::7] = -0.0
    return u


def case(shape, walls, kinds, seed=3):
    """(kappa, values) of rc.random_case; kinds None: no values at all."""
    kappa, values = rc.random_case(shape, walls, kinds or ("none",) * 6, seed)
    return kappa, (None if kinds is None else values)


def poison(kappa, walls):
    """A copy of kappa with NaN in every ghost cell the fluxes must not read: all of the ghost layer but the face layers
    behind Dirichlet walls (read with or without a value) — what rc.poison_unread_ghosts gives for six values."""
    return rc.poison_unread_ghosts(kappa, walls, (0.0,) * 6)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def sigma_term(sigma, u, how):
    """What the operator adds to the balance of the fluxes: sigma u, with widths sigma V u."""
    if sigma is None:
        return np.zeros(u.shape)
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), u.shape)
    return s * operators.cell_volumes(how["spacing"]) * u if "spacing" in how else s * u


def identity_sides(kappa, u, walls, values, sigma, how):
    """(left, right, bound) of  divergence_faces(flux_kappa(u)) + sigma term = A u - rhs_kappa(None, values), per cell; the
    bound is 32 eps (|A| |u| + |b|): each side is at most 7 products of at most 3 roundings plus at most 7 additions."""
    A = operators.stencil7_kappa(kappa, walls, sigma, **how)
    b = operators.rhs_kappa(kappa, None, walls, values, **how)
    left = operators.divergence_faces(*operators.flux_kappa(kappa, u, walls, values, **how)) + sigma_term(sigma, u, how)
    right = (A @ u.ravel()).reshape(u.shape) - b
    bound = 32 * EPS * ((abs(A) @ np.abs(u.ravel())).reshape(u.shape) + np.abs(b))
    return left, right, bound
