#!/usr/bin/env python3
"""A time-stepping loop's pressure solves on one MI355X through `openmg_amd.Solver`: one operator, a new right-hand side
every step, each solve started from the previous step's pressure.

    python examples/timestep_solve.py [extent] [grids]        (default 64, 4)

The operator is the grid's graph Laplacian (homogeneous Neumann walls: singular, null space the constants), so the solver
is made with parameters['nullspace'] = 'constant': every b is projected onto the complement of the constants and every u
comes back with mean 0.  The hierarchy is set up once; a step costs one upload of b, the FCG iterations the drift of the
source makes necessary, and one download of u.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402

STEPS = 20


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
    params = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "smoother": "colour",
              "nullspace": "constant", "accel": "cg", "cycle": "F", "overCorrection": 1.8, "threshold": 0.0, "cycles": 200, "rtol": 1e-8}
    t0 = time.perf_counter()
    with openmg_amd.Solver(A, params) as solver:
        print("%d^3 unknowns, %d grids, pure Neumann; setup %.1f ms" % (extent, grids, 1e3 * (time.perf_counter() - t0)))
        print("%4s %10s %14s %14s %12s %8s" % ("step", "iterations", "||r0|| / ||b||", "||r|| / ||b||", "|mean u|", "ms"))
        u = None
        for step in range(STEPS):
            t = 0.05 * step                                    # the source moves a little every step
            b = (np.cos(np.pi * (xx + t)) * np.cos(2 * np.pi * yy) * np.cos(3 * np.pi * (zz - t))).ravel() / extent ** 2
            t0 = time.perf_counter()
            u, info = solver.solve(b, initial=u)
            ms = 1e3 * (time.perf_counter() - t0)
            print("%4d %10d %14.3e %14.3e %12.2e %8.2f" % (step, info["cycle"], info["initial_norm"] / info["rhs_norm"],
                                                           info["norm"] / info["rhs_norm"], abs(u.mean()), ms))


if __name__ == "__main__":
    main()
