#!/usr/bin/env python3
"""The pressure equation of a variable-density flow step in a periodic box on one MI355X, through
`openmg_amd.Solver.from_kappa(..., walls=('periodic',) * 6)`:

    -div((1 / rho) grad p) = f   on the unit box, periodic in x, y and z,

with a density that varies by a factor of `ratio` across a wavy interface (a Rayleigh-Taylor layer seen early) and a
right-hand side of zero mean, as the divergence of a periodic velocity field has.

    python examples/periodic_box_solve.py [N] [levels] [ratio]        (default 64, 4, 10.0)

The solver is made from the field itself — kappa = 1 / rho with one ghost layer, which along a periodic axis is never read
and here holds NaN to show it — and the 7-point operator with its wrap-around couplings is assembled in HBM
(operators.stencil7_kappa is the definition).  Every wall is periodic and there is no sigma, so the operator is singular
with the constants as its null space: 'nullspace': 'constant' projects the right-hand side and returns the pressure of
zero mean.  The iteration is flexible conjugate gradients around an F(1,1) cycle with an over-correction of 1.8.  Then the
interface moves a few times and the solver takes each new field with `update_kappa`, starting from the last pressure.
(No fused pass takes a periodic level: the hierarchy runs the ordinary row kernels, and update_kappa builds a new one.)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402

WALLS = ("periodic",) * 6


def fields(n, ratio):
    """kappa_at(t): 1 / rho with NaN ghost layers; f: a right-hand side of zero mean; both periodic on the cell centres."""
    x = (np.arange(n) + 0.5) / n
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")

    def kappa_at(t):
        interface = 0.5 + 0.08 * np.sin(2.0 * np.pi * (X + 0.1 * t)) * np.cos(2.0 * np.pi * Y) + 0.05 * t * np.cos(4.0 * np.pi * X)
        # heavy above the interface, light below, and back again across z = 0 = 1: smooth steps of width 2 / n
        step = 0.5 * (np.tanh((Z - interface) * n / 2.0) - np.tanh((Z - interface - 0.5) * n / 2.0))
        rho = 1.0 + (ratio - 1.0) * step
        out = np.full((n + 2,) * 3, np.nan)
        out[1:-1, 1:-1, 1:-1] = 1.0 / rho
        return out

    f = np.sin(2.0 * np.pi * X) * np.cos(4.0 * np.pi * Y) * np.sin(2.0 * np.pi * Z) + np.cos(2.0 * np.pi * (X + Y + Z))
    return kappa_at, (f - f.mean()).ravel()


def run(n, levels, ratio, steps=3, say=print):
    """Setup, a solve, `steps` new fields with a solve each.  Returns the iteration count of every solve."""
    kappa_at, f = fields(n, ratio)
    params = {"gridLevels": levels, "preIterations": 1, "postIterations": 1, "smoother": "colour", "nullspace": "constant",
              "accel": "cg", "cycle": "F", "overCorrection": 1.8, "threshold": 0.0, "cycles": 100, "rtol": 1e-8}
    scale = (float(n) ** 2,) * 3                                   # 1 / h^2 along every axis
    say("%d^3 cells, %d levels, density ratio %.1f, periodic in x, y and z; FCG around F(1,1), overCorrection 1.8" % (n, levels, ratio))
    t0 = time.perf_counter()
    with openmg_amd.Solver.from_kappa(kappa_at(0.0), params, WALLS, scale=scale) as solver:
        t1 = time.perf_counter()
        p, info = solver.solve(f)
        t2 = time.perf_counter()
        say("setup %.1f ms, updates in place: %s" % (1e3 * (t1 - t0), solver.hierarchy.can_update_fine()))
        say("    %4s %10s %14s %12s %12s %12s" % ("step", "iterations", "||r|| / ||f||", "mean(p)", "update ms", "solve ms"))
        say("    %4d %10d %14.3e %12.1e %12s %12.2f" % (0, info["cycle"], info["norm"] / info["rhs_norm"], p.mean(), "-", 1e3 * (t2 - t1)))
        counts = [info["cycle"]]
        for step in range(1, steps + 1):
            t0 = time.perf_counter()
            solver.update_kappa(kappa_at(step / steps))
            t1 = time.perf_counter()
            p, info = solver.solve(f, initial=p)
            t2 = time.perf_counter()
            say("    %4d %10d %14.3e %12.1e %12.2f %12.2f" % (step, info["cycle"], info["norm"] / info["rhs_norm"], p.mean(), 1e3 * (t1 - t0),
                                                              1e3 * (t2 - t1)))
            counts.append(info["cycle"])
    return counts


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    ratio = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0
    run(n, levels, ratio)


if __name__ == "__main__":
    main()
