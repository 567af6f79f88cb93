#!/usr/bin/env python3
"""examples/timestep_solve.py's loop with `projection=8`: every solve starts from the best approximation of its solution in
the span of up to eight earlier ones (Fischer's projection for successive right-hand sides), kept in HBM.

    python examples/projected_timestep_solve.py [extent] [grids]        (default 64, 4)

The operator, the null space and the moving source are those of timestep_solve.py.  Beside each projected solve the same
step is solved from the previous step's pressure on a second solver, so that the two iteration counts stand side by side;
the step after the set has filled up (the set restarts from the last solution) costs about what the warm start costs.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from timestep_solve import STEPS, neumann_laplacian  # noqa: E402

CAPACITY = 8


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    shape = (extent,) * 3
    A = neumann_laplacian(shape)
    zz, yy, xx = np.meshgrid(*((np.arange(extent) + 0.5) / extent,) * 3, indexing="ij")
    params = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "smoother": "colour",
              "nullspace": "constant", "accel": "cg", "cycle": "F", "overCorrection": 1.8, "threshold": 0.0, "cycles": 200, "rtol": 1e-8}
    with openmg_amd.Solver(A, params, projection=CAPACITY) as solver, openmg_amd.Solver(A, params) as warm:
        print("%d^3 unknowns, %d grids, pure Neumann; a set of up to %d earlier solutions" % (extent, grids, CAPACITY))
        print("%4s | %9s %5s %14s %10s %8s | %15s %8s" % ("step", "projected", "set", "||r0|| / ||b||", "iterations", "ms",
                                                          "warm: iterations", "ms"))
        u_warm = None
        for step in range(STEPS):
            t = 0.05 * step                                    # the source moves a little every step
            b = (np.cos(np.pi * (xx + t)) * np.cos(2 * np.pi * yy) * np.cos(3 * np.pi * (zz - t))).ravel() / extent ** 2
            t0 = time.perf_counter()
            u, info = solver.solve(b)
            ms = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            u_warm, winfo = warm.solve(b, initial=u_warm)
            wms = 1e3 * (time.perf_counter() - t0)
            print("%4d | %9d %5d %14.3e %10d %8.2f | %15d %8.2f" % (step, info["projected"], info["basis"],
                                                                    info["initial_norm"] / info["rhs_norm"], info["cycle"], ms,
                                                                    winfo["cycle"], wms))


if __name__ == "__main__":
    main()
