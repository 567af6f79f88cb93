#!/usr/bin/env python3
"""Solve a 3-D Poisson problem on a grid whose extents are NOT of the form m * 2^k on one MI355X, with
'oddExtents': 'merge', and print the hierarchy that was built, the cycles and the milliseconds.

    python examples/anyshape3d_solve.py [N] [levels] [NY NX]        (default 100 5; e.g. 100 5, 250 6, 300 6 150 75)

Without the key a hierarchy halves an axis only where its extent is even: 100^3 stops at 25^3, whose 15625 unknowns the
coarsest level has to solve directly, and 75 cannot be coarsened at all.  With 'merge' an axis of any extent e >= 4 gets
e // 2 coarse cells, and where e is odd the last coarse cell along that axis holds three fine cells instead of two:
100 -> 50 -> 25 -> 12 -> 6 -> 3.  The levels whose extents are even keep their fused passes; a level with a merged cell runs
the set-by-set row kernels.  `levels` is the number of restrictions asked for ('gridLevels'); the hierarchy ends earlier
where no axis has an extent >= 4 or the next level would have <= 8 rows ('minSize').
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from openmg_amd import operators  # noqa: E402


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    shape = (extent, int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (extent,) * 3
    A = operators.stencil_poisson(shape)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    target = 1e-8 * np.linalg.norm(b)
    print("%s unknowns, at most %d restrictions; to ||r|| < 1e-8 ||b||, at most 400 cycles" % (" x ".join(map(str, shape)), levels))
    print("%-14s %8s %14s %10s %10s   %s" % ("cycle", "cycles", "||r|| / ||b||", "setup s", "solve ms", "levels"))
    for extra in ({}, {"cycle": "F", "overCorrection": 1.8}, {"accel": "cg", "cycle": "F", "overCorrection": 1.8}):
        params = dict({"problemShape": shape, "gridLevels": levels, "preIterations": 1, "postIterations": 1, "smoother": "colour",
                       "oddExtents": "merge", "threshold": target, "cycles": 400}, **extra)
        t0 = time.perf_counter()
        with openmg_amd.Solver(A, params) as solver:           # (the setup once: the solve time below is the solve alone)
            solver.solve(b, cycles=1)
            setup = time.perf_counter() - t0
            t0 = time.perf_counter()
            u, info = solver.solve(b)
            ms = 1e3 * (time.perf_counter() - t0)
        name = ("FCG + " if extra.get("accel") else "") + ("F(1,1) x 1.8" if "cycle" in extra else "V(1,1)")
        print("%-14s %8d %14.3e %10.2f %10.1f   %s" % (name, info["cycle"], info["norm"] / np.linalg.norm(b), setup, ms,
                                                       " -> ".join("x".join(str(s) for s in g) for g in info["levelShapes"])))
    # (the last row is FCG: its stopping test is on the recurrence's residual, the true one may stand a little above it)
    assert np.linalg.norm(b - A @ u) < 2 * target or info["cycle"] == 400


if __name__ == "__main__":
    main()
