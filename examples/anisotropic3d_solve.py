#!/usr/bin/env python3
"""Solve an anisotropic 3-D diffusion problem — a grid stretched along one axis, as in a boundary layer — on one MI355X
with the point smoother 'colour' and with the zebra line smoother 'line', and print cycles and milliseconds for each.

    python examples/anisotropic3d_solve.py [N] [levels] [ratio]        (default 64, 4, 100)

The operator is the 7-point finite-volume Laplacian on N^3 cells whose couplings along the unit-stride axis are `ratio`
times those along the other two (Dirichlet walls).  Point smoothing only damps the error along the strong axis, so the
cycles crawl whatever their shape; 'line' solves every grid line along that axis exactly ('lineAxis': 'auto' finds it) and
converges like multigrid on an isotropic problem.  With TWO strong axes (try ratio < 1: the unit-stride axis becomes the
one weak axis) lines along one axis are not enough — that is what 'coarsening': 'auto' (semicoarsening) repairs:
examples/semicoarsen3d_solve.py.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402


def anisotropic_laplacian(shape, factors):
    """sum over the axes of factors[a] * (second difference along a), Dirichlet walls; C order, sorted CSR"""
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 2.0 * sum(factors))]
    for ax, f in enumerate(factors):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [a, b]
        cols += [b, a]
        vals += [np.full(a.size, -f), np.full(a.size, -f)]
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    ratio = float(sys.argv[3]) if len(sys.argv) > 3 else 100.0
    shape = (extent,) * 3
    A = anisotropic_laplacian(shape, (1.0, 1.0, ratio))
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    target = 1e-8 * np.linalg.norm(b)
    limit = 400
    print("%d^3 unknowns, %d grids, couplings 1 : 1 : %g (last = unit-stride axis); to ||r|| < 1e-8 ||b||, at most %d cycles"
          % (extent, levels, ratio, limit))
    print("%-34s %8s %14s %10s %10s" % ("smoother, cycle", "cycles", "||r|| / ||b||", "ms", "line axis"))
    for smoother, extra in (("colour", {"cycle": "F", "overCorrection": 1.8}), ("line", {}), ("line", {"cycle": "F", "overCorrection": 1.8})):
        params = dict({"problemShape": shape, "gridLevels": levels - 1, "preIterations": 1, "postIterations": 1, "smoother": smoother,
                       "threshold": target, "cycles": limit, "giveInfo": True}, **extra)
        with openmg_amd.Solver(A, params) as solver:       # (the setup once: the time below is the solve alone)
            solver.solve(b, cycles=1)
            t0 = time.perf_counter()
            u, info = solver.solve(b)
            ms = 1e3 * (time.perf_counter() - t0)
        name = "'%s', %s" % (smoother, "F(1,1) x 1.8" if extra else "V(1,1)")
        reached = "" if info["norm"] < target else "  (not reached)"
        print("%-34s %8d %14.3e %10.1f %10s%s" % (name, info["cycle"], info["norm"] / np.linalg.norm(b), ms, info.get("lineAxis", "-"), reached))


if __name__ == "__main__":
    main()
