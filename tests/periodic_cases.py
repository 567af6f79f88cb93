"""Shared inputs of tests/test_periodic_host.py and tests/test_gpu_periodic.py: the seven sets of periodic axes, the three
kinds of walls on the other axes, fields, widths, and the SciPy definition (operators.stencil7_kappa) computed once per
case and never written to."""
import functools
import itertools

import numpy as np

from openmg_amd import operators

D, N, P = "dirichlet", "neumann", "periodic"
AXIS_SETS = [axes for k in (1, 2, 3) for axes in itertools.combinations((0, 1, 2), k)]       # axes of the grid's shape: 0 = z, 2 = x
OTHERS = ("dirichlet", "neumann", "mixed")                                                     # the walls of the axes that are not periodic
ALL = (0, 1, 2)


def axes_id(axes):
    return "".join("zyx"[a] for a in axes)


def walls_of(axes, other="dirichlet"):
    """Six wall names (-z, +z, -y, +y, -x, +x): 'periodic' on both walls of every axis in `axes`; on the others Dirichlet,
    Neumann, or mixed = Neumann below and Dirichlet above."""
    pair = {"dirichlet": (D, D), "neumann": (N, N), "mixed": (N, D)}[other]
    out = []
    for axis in range(3):
        out += [P, P] if axis in axes else list(pair)
    return tuple(out)


def kappa_of(shape, seed=11, decades=3.0):
    """exp(U(-1, 1) ln 10^decades) per cell, ghost layer included."""
    nz, ny, nx = shape
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nz + 2, ny + 2, nx + 2)) * np.log(10.0 ** decades))


def nan_ghosts(kappa, axes):
    """A copy with NaN in every ghost entry along the periodic axes (both layers of each, edges and corners included)."""
    out = kappa.copy()
    for axis in axes:
        sel = [slice(None)] * 3
        for end in (0, -1):
            sel[axis] = end
            out[tuple(sel)] = np.nan
    return out


def sigma_of(kind, shape, seed=12):
    if kind == "none":
        return None
    if kind == "scalar":
        return 0.375
    return np.random.default_rng(seed).uniform(0.0, 2.0, size=shape)


def spacing_of(shape, seed=13):
    """Non-uniform widths in [0.5, 2) per axis, the ghost entries too (finite: operators.spacing_arguments checks them)."""
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(0.5, 2.0, size=s + 2) for s in shape)


SCALE = (4.0, 1.0, 0.25)
# (sigma kind, spaced): every sigma kind and both forms of the face, without the full product
FORMS = [("none", False), ("scalar", True), ("field", False), ("field", True)]


@functools.lru_cache(maxsize=None)
def definition(shape, axes, other="dirichlet", skind="none", spaced=False, seed=11):
    """operators.stencil7_kappa of the case (scale SCALE, or spacing_of(shape)): computed once, shared, never written to."""
    kw = {"spacing": spacing_of(shape)} if spaced else {"scale": SCALE}
    A = operators.stencil7_kappa(kappa_of(shape, seed), walls_of(axes, other), sigma_of(skind, shape), **kw)
    for a in (A.indptr, A.indices, A.data):
        a.setflags(write=False)
    return A


def expected_nnz(shape, axes):
    n = int(np.prod(shape))
    return 7 * n - 2 * sum(n // shape[a] for a in range(3) if a not in axes)


def rhs_of(shape, seed=5):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    return rng.standard_normal(n), rng.standard_normal(n)


def same_csr(got, want):
    """(indptr, indices, data) against a SciPy CSR, bit for bit, dtypes included."""
    indptr, indices, data = got
    return (indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
            and np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices) and np.array_equal(data, want.data))


def check_assembly(shape, axes, others=OTHERS, forms=FORMS):
    """The device assembly of every (other walls, sigma, spacing) form of one (shape, periodic axes) against the definition;
    the field is handed over with NaN in the ghost layers along the periodic axes.  Used in-process and by the child process
    that runs the unstaged store path."""
    from openmg_amd import _hip
    kappa = nan_ghosts(kappa_of(shape), axes)
    for other in others:
        for skind, spaced in forms:
            want = definition(shape, axes, other, skind, spaced)
            kw = {"spacing": spacing_of(shape)} if spaced else {"scale": SCALE}
            got = _hip.kappa_assemble(kappa, walls_of(axes, other), sigma_of(skind, shape), **kw)
            assert same_csr(got, want), (shape, axes, other, skind, spaced)
