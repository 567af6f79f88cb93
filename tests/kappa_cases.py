"""Shared inputs of tests/test_kappa_host.py and tests/test_gpu_kappa.py: coefficient fields over six decades, the wall,
sigma and scale settings, and the SciPy definition (operators.stencil7_kappa) computed once per case."""
import functools

import numpy as np

from openmg_amd import operators

SHAPES = [(4, 4, 4),        # the smallest with interior rows and every kind of boundary row
          (5, 7, 9),        # odd extents
          (2, 3, 70),       # more than one wave along x, fewer than two cells along z (the -K / +K logic)
          (16, 16, 16),
          (32, 32, 32)]

D, N = "dirichlet", "neumann"
WALLS = {"dirichlet": (D,) * 6,
         "neumann": (N,) * 6,                   # (always with a sigma field: the operator is singular without)
         "mixed": (N, D, D, N, D, D)}           # Neumann on -z and +y
SIGMAS = ("none", "scalar", "field")
SCALES = [(1.0, 1.0, 1.0), (4.0, 1.0, 0.25)]


def kappa_of(shape, seed=11):
    """exp(U(-1, 1) ln 10^3) per cell, ghost layer included: six decades."""
    nz, ny, nx = shape
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(1.0e3))


def sigma_of(kind, shape, seed=12):
    if kind == "none":
        return None
    if kind == "scalar":
        return 0.375
    return np.random.default_rng(seed).uniform(0.0, 2.0, size=shape)


def assembly_cases():
    """(shape, walls name, sigma kind, scale) of the assembly test: every shape x walls x sigma x scale, all-Neumann walls
    with the sigma field only."""
    out = []
    for shape in SHAPES:
        for wname in WALLS:
            for skind in SIGMAS:
                if wname == "neumann" and skind != "field":
                    continue
                for scale in SCALES:
                    out.append((shape, wname, skind, scale))
    return out


@functools.lru_cache(maxsize=None)
def definition(shape, wname="dirichlet", skind="none", scale=(1.0, 1.0, 1.0), seed=11):
    """operators.stencil7_kappa of the case: computed once, shared, never written to."""
    A = operators.stencil7_kappa(kappa_of(shape, seed), WALLS[wname], sigma_of(skind, shape), scale)
    for a in (A.indptr, A.indices, A.data):
        a.setflags(write=False)
    return A


def rhs_of(shape, seed=5):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    return rng.standard_normal(n), rng.standard_normal(n)
