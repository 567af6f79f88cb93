#!/usr/bin/env python3
"""Solve a grid-aligned anisotropic 3-D diffusion problem on one MI355X with full coarsening and with semicoarsening
('coarsening': 'auto'), and print the factors chosen, the levels' grids, cycles and milliseconds for each.

    python examples/semicoarsen3d_solve.py [N] [grids] [cz] [cy] [cx]        (default 64, 4, 1, 100, 100)

The operator is sum over the axes a of c_a * (second difference along a) on N^3 cells with Dirichlet walls, C order
(z, y, x: x has unit stride).  With two strong axes (the default 1 : 100 : 100) a point smoother leaves an error that is
smooth along y and x and rough along z; a grid coarsened along z too cannot represent it, and lines along one axis do not
remove it either.  'auto' coarsens only y and x until the operator is isotropic — every such step halves their coupling
relative to z — and all axes from there on.  A semicoarsened cycle costs more than a fully coarsened one (its coarse
levels are larger and run the set-by-set kernels); the gain is in the number of cycles.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from examples.anisotropic3d_solve import anisotropic_laplacian  # noqa: E402


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    c = tuple(float(v) for v in sys.argv[3:6]) if len(sys.argv) > 5 else (1.0, 100.0, 100.0)
    shape = (extent,) * 3
    A = anisotropic_laplacian(shape, c)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    target = 1e-8 * np.linalg.norm(b)
    limit = 400
    print("%d^3 unknowns, %d grids, couplings %g : %g : %g (z : y : x); to ||r|| < 1e-8 ||b||, at most %d cycles"
          % ((extent, grids) + c + (limit,)))
    print("%-10s %-10s %-14s %8s %14s %10s   %s" % ("smoother", "coarsening", "cycle", "cycles", "||r|| / ||b||", "ms", "factors -> coarsest grid"))
    for smoother in ("colour", "line"):
        for coarsening in ("full", "auto"):
            for extra in ({}, {"cycle": "F", "overCorrection": 1.8}):
                params = dict({"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1,
                               "smoother": smoother, "coarsening": coarsening, "threshold": target, "cycles": limit, "minSize": 1}, **extra)
                with openmg_amd.Solver(A, params) as solver:       # (the setup once: the time below is the solve alone)
                    solver.solve(b, cycles=1)
                    t0 = time.perf_counter()
                    u, info = solver.solve(b)
                    ms = 1e3 * (time.perf_counter() - t0)
                how = "every axis by 2"
                if "coarsening" in info:
                    how = "%s -> %s" % (" ".join("x".join(str(f) for f in entry) for entry in info["coarsening"]),
                                        "x".join(str(s) for s in info["levelShapes"][-1]))
                reached = "" if info["norm"] < target else "  (not reached)"
                print("%-10s %-10s %-14s %8d %14.3e %10.1f   %s%s" % (smoother, coarsening, "F(1,1) x 1.8" if extra else "V(1,1)", info["cycle"],
                                                                     info["norm"] / np.linalg.norm(b), ms, how, reached))


if __name__ == "__main__":
    main()
