"""Fischer's projection onto earlier solutions (P. F. Fischer, Projection techniques for iterative solution of A x = b with
successive right-hand sides, 1998) restated in NumPy / SciPy, and the problems tests/test_projection_host.py and
tests/test_gpu_projection.py share.  The restatement is the definition openmg_amd.Solver(..., projection=L) is held to: a
set of at most L vectors with x_i^T A x_j = delta_ij, a start sum_i (x_i . b) x_i, and after the solve the direction the
solve added, A-orthogonalised against the set with the operator applied twice, kept exactly when s2 = d^T A d is finite,
positive and at least 2^-26 of what it was before the orthogonalisation; a full set restarts from the whole solution."""
import functools
import math

import numpy as np

from openmg_amd import operators

KEEP = 2.0 ** -26

MODES = ((1, 1, 1), (2, 1, 3), (3, 2, 1), (1, 4, 2), (5, 1, 1), (2, 3, 4))


class Projection:
    """The set for the SciPy matrix A and a capacity; nullspace: directions lose their mean before they are measured."""

    def __init__(self, A, capacity, nullspace=False):
        assert 1 <= capacity <= 64
        self.A, self.capacity, self.nullspace = A, int(capacity), nullspace
        self.X = []
        self.restarts = 0

    def project(self, b):
        """(the start, the alphas): sum_i (x_i . b) x_i with i ascending"""
        alpha = [float(x @ b) for x in self.X]
        start = np.zeros(self.A.shape[0])
        for a, x in zip(alpha, self.X):
            start += a * x
        return start, alpha

    def update(self, x, alpha):
        """The solve that started from project()'s start ended at x.  Returns whether its direction was kept."""
        if len(self.X) == self.capacity:
            self.X, self.restarts = [], self.restarts + 1
            d = np.array(x, dtype=np.float64)
        else:
            d = np.array(x, dtype=np.float64)
            for a, v in zip(alpha, self.X):
                d -= a * v
        if self.nullspace:
            d -= d.mean()
        w = self.A @ d
        e0 = float(d @ w)
        beta = [float(v @ w) for v in self.X]
        for c, v in zip(beta, self.X):
            d -= c * v
        w = self.A @ d
        s2 = float(d @ w)
        keep = math.isfinite(s2) and s2 > 0.0 and s2 >= KEEP * e0
        if keep:
            self.X.append(d / math.sqrt(s2))
        return keep

    def solve(self, b, callback):
        """callback(b, start) -> (x, cycles run).  Returns (x, cycles, vectors used, kept)."""
        start, alpha = self.project(b)
        x, cycles = callback(b, start)
        kept = self.update(x, alpha) if cycles > 0 else False
        return x, cycles, len(alpha), kept

    def gram_error(self, X=None, A=None):
        return gram_error(self.X if X is None else X, self.A if A is None else A)


def gram_error(X, A):
    """max |x_i^T A x_j - delta_ij| over a list of vectors (0.0 for an empty one)"""
    if not len(X):
        return 0.0
    M = np.stack([np.asarray(x, dtype=np.float64) for x in X])
    return float(np.abs(M @ (A @ M.T) - np.eye(len(X))).max())


# ------------------------------------------------------------------------------------ problems --
def kappa_field(shape):
    """kappa = exp(U(-1, 1)), seed 0, on the cells and one ghost layer"""
    return np.exp(np.random.default_rng(0).uniform(-1.0, 1.0, tuple(s + 2 for s in shape)))


@functools.lru_cache(maxsize=None)
def operator(shape, walls=None):
    """operators.stencil7_kappa of kappa_field(shape): Dirichlet walls unless `walls` names others"""
    A = operators.stencil7_kappa(kappa_field(shape), walls)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def modes(shape):
    """(the six smooth modes f_m as rows, the noise g): f = sin pi(a z + 0.3) cos pi b y sin pi(c x + 0.1) with z, y, x in
    [0, 1] on the cell index grid, g standard normal with seed 0"""
    z, y, x = (np.linspace(0.0, 1.0, s) for s in shape)
    F = []
    for a, b, c in MODES:
        f = (np.sin(np.pi * (a * z + 0.3))[:, None, None] * np.cos(np.pi * b * y)[None, :, None]
             * np.sin(np.pi * (c * x + 0.1))[None, None, :])
        F.append(f.reshape(-1))
    g = np.random.default_rng(0).standard_normal(int(np.prod(shape)))
    return np.stack(F), g


def rhs(shape, t):
    """b(t) = sum_m cos(0.03 (m + 1) t + m) f_m + 0.3 cos(0.015 t) g, m = 0 .. 5"""
    F, g = modes(tuple(shape))
    amp = np.array([math.cos(0.03 * (m + 1) * t + m) for m in range(len(MODES))])
    return amp @ F + 0.3 * math.cos(0.015 * t) * g
