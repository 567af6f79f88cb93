#!/usr/bin/env python3
"""Solve a 3-D pure-Neumann Poisson problem — the pressure equation of an incompressible flow step — on one MI355X
through `mgSolve` with parameters['nullspace'] = 'constant' and accel = 'cg'.

    python examples/neumann3d_solve.py [extent] [grids]        (default 64, 4)

The operator is the grid's graph Laplacian (zero row sums: homogeneous Neumann walls), so it is singular and its null
space is the constant vector.  A right-hand side with a mean has no solution; mgSolve subtracts the mean from its copy of
b, solves on the complement of the constants and returns the u with mean(u) = 0.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402


def neumann_laplacian(shape):
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols = [], []
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [a, b]
        cols += [b, a]
    W = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A = sp.csr_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
    A.sort_indices()
    return A


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    shape = (extent,) * 3
    A = neumann_laplacian(shape)
    zz, yy, xx = np.meshgrid(*((np.arange(extent) + 0.5) / extent,) * 3, indexing="ij")
    u_exact = (np.cos(np.pi * xx) * np.cos(2 * np.pi * yy) * np.cos(3 * np.pi * zz)).ravel()
    u_exact -= u_exact.mean()
    b = A @ u_exact + 0.3                      # a source with a mean: only b - mean(b) has a solution
    target = 1e-8 * np.linalg.norm(b - b.mean())
    print("%d^3 unknowns, %d nonzeros, %d grids, pure Neumann; mean(b) = %.3f" % (extent, A.nnz, grids, b.mean()))
    print("%-28s %10s %14s %14s %12s %10s" % ("solver", "iterations", "||r||", "max |u - u*|", "|mean u|", "seconds"))
    for name, extra in (("V(1,1) + accel='cg'", {"accel": "cg"}), ("F(1,1), overCorrection 1.8", {"cycle": "F", "overCorrection": 1.8})):
        params = dict({"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "smoother": "colour",
                       "nullspace": "constant", "threshold": target, "cycles": 400, "giveInfo": True}, **extra)
        t0 = time.perf_counter()
        u, info = openmg_amd.mgSolve(A, b, params)
        print("%-28s %10d %14.6e %14.6e %12.2e %10.2f" % (name, info["cycle"], info["norm"], np.abs(u - u_exact).max(), abs(u.mean()),
                                                          time.perf_counter() - t0))


if __name__ == "__main__":
    main()
