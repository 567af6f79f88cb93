"""Shared inputs of tests/test_stretched_host.py and tests/test_gpu_stretched.py: random cell widths over three decades,
the tanh-clustered faces of a boundary-layer grid, and the SciPy definition (operators.stencil7_kappa with spacing=)
computed once per case.  The fields, walls and sigmas are those of kappa_cases."""
import functools

import numpy as np

from openmg_amd import operators

import kappa_cases as kc


def widths_of(shape, seed=61, zero=False):
    """exp(U(-1, 1) ln 30) per entry, ghost entries included; zero: the ghost width is 0 at +z and at -x (Dirichlet in every
    wall setting but the all-Neumann one: the value then sits on the wall face itself)."""
    rng = np.random.default_rng(seed)
    sp = [np.exp(rng.uniform(-1.0, 1.0, size=s + 2) * np.log(30.0)) for s in shape]
    if zero:
        sp[0][-1] = 0.0
        sp[2][0] = 0.0
    return tuple(sp)


def tanh_faces(n, beta):
    """n + 1 faces on [0, 1] clustered towards 0: z_f = 1 - tanh(beta (1 - m / n)) / tanh(beta)."""
    m = np.arange(n + 1, dtype=np.float64)
    return 1.0 - np.tanh(beta * (1.0 - m / n)) / np.tanh(beta)


def padded(widths, ghost="mirror"):
    """The widths with one ghost entry at each end: the boundary cell's own width ('mirror') or 0 ('wall')."""
    w = np.asarray(widths, dtype=np.float64)
    return np.concatenate(([w[0] if ghost == "mirror" else 0.0], w, [w[-1] if ghost == "mirror" else 0.0]))


def boundary_layer_spacing(shape, beta=2.0, ghost="mirror"):
    """z clustered by the tanh map, y and x uniform on the unit box."""
    nz, ny, nx = shape
    return (padded(np.diff(tanh_faces(nz, beta)), ghost), padded(np.full(ny, 1.0 / ny), ghost), padded(np.full(nx, 1.0 / nx), ghost))


def assembly_cases():
    """(shape, walls name, sigma kind, zero ghost widths) of the assembly test: all-Neumann walls with the sigma field only."""
    out = []
    for shape in [(4, 4, 4), (5, 7, 9), (2, 3, 70), (16, 16, 16)]:
        for wname in kc.WALLS:
            for skind in kc.SIGMAS:
                if wname == "neumann" and skind != "field":
                    continue
                for zero in (False, True):
                    out.append((shape, wname, skind, zero))
    return out


@functools.lru_cache(maxsize=None)
def definition(shape, wname="dirichlet", skind="none", zero=False, seed=11, wseed=61):
    """operators.stencil7_kappa(..., spacing=widths_of(...)) of the case: computed once, shared, never written to."""
    A = operators.stencil7_kappa(kc.kappa_of(shape, seed), kc.WALLS[wname], kc.sigma_of(skind, shape), spacing=widths_of(shape, wseed, zero))
    for a in (A.indptr, A.indices, A.data):
        a.setflags(write=False)
    return A
