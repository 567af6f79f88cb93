#!/usr/bin/env python3
"""A turbulent-channel grid on one MI355X: -div(kappa grad u) = f on the classical channel box — 2 pi long in x, pi wide in
z, 1 high in y (4 pi x 2 x 2 pi in half heights) —, PERIODIC in x and z, walls in y with the y faces clustered towards both
of them,

    y_f = (1 + tanh(beta (2 m / n - 1)) / tanh(beta)) / 2,   m = 0 .. n,

through `openmg_amd.Solver.from_kappa(kappa, parameters, walls, spacing=...)`.

    python examples/channel_solve.py [N] [levels] [beta]        (default 64, 4, 2.5)

N^3 cells, `levels` grids.  The thin wall cells couple strongly along y, which is what stalls a point smoother, and the two
periodic axes are what the plain 'line' smoother refuses: 'line-periodic' takes the wrapped neighbours across its lines
(and would solve cyclic lines along a periodic axis).  The lines run along y, the axis the library finds by itself; the
periodic extents across them stay even on every smoothed level as long as N / 2^(levels - 2) is even.  'line-periodic' and
'colour' meet the same operator, each with V cycles and with F cycles at an over-correction of 1.8: cycles to
||r|| <= 1e-8 ||b|| (at most 200) and milliseconds per cycle.  u = 0 on the walls, so the operator is regular.  (In this
box the cells are nowhere higher than wide or long, so y is the strong axis everywhere; on the unit cube with beta = 2.5
the cells in the middle of the channel are 2.5 times as high as wide, the strong axis changes across the channel and lines
along y alone gain little: 83 against 93 F(1.8) cycles at 128^3.)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from openmg_amd import operators  # noqa: E402

WALLS = ("periodic", "periodic", "dirichlet", "dirichlet", "periodic", "periodic")     # -z, +z, -y, +y, -x, +x
VARIANTS = [("line-periodic", "V", 1.0), ("line-periodic", "F", 1.8), ("colour", "V", 1.0), ("colour", "F", 1.8)]


def grid(n, beta):
    """The widths (hz, hy, hx) — ghost entries 0: the wall value sits on the wall face; the periodic axes' are never read —
    and the cell centres."""
    m = np.arange(n + 1, dtype=np.float64)
    faces = [np.pi * m / n, 0.5 * (1.0 + np.tanh(beta * (2.0 * m / n - 1.0)) / np.tanh(beta)), 2.0 * np.pi * m / n]
    spacing = tuple(np.concatenate(([0.0], np.diff(f), [0.0])) for f in faces)
    centres = [0.5 * (f[1:] + f[:-1]) for f in faces]
    return spacing, np.meshgrid(*centres, indexing="ij")


def run(n, levels, beta, limit=200, say=print):
    """Every variant: setup and one solve.  Returns {(smoother, cycle): (cycles, reached)}."""
    spacing, (Z, Y, X) = grid(n, beta)
    kappa = np.ones((n + 2,) * 3)
    kappa[1:-1, 1:-1, 1:-1] = np.exp(0.5 * np.sin(X) * np.cos(2.0 * Z) * np.sin(np.pi * Y))
    f = np.sin(X) * np.cos(4.0 * Z) * (1.0 + Y) + np.sin(3.0 * np.pi * Y)
    b = (f * operators.cell_volumes(spacing)).ravel()
    hy = spacing[1][1:-1]
    say("%d^3 cells, %d grids, beta %.2f: y cells %.2e .. %.2e (ratio %.1f), the wall cells %.1f times as wide as high"
        % (n, levels, beta, hy.min(), hy.max(), hy.max() / hy.min(), (np.pi / n) / hy[0]))
    say("%-14s %-7s %8s %14s %10s %12s %12s" % ("smoother", "cycle", "cycles", "||r|| / ||b||", "setup ms", "solve ms", "ms / cycle"))
    results = {}
    for smoother, cycle, alpha in VARIANTS:
        params = {"gridLevels": levels, "preIterations": 1, "postIterations": 1, "threshold": 0.0, "cycles": limit, "rtol": 1e-8,
                  "smoother": smoother, "cycle": cycle, "overCorrection": alpha}
        t0 = time.perf_counter()
        with openmg_amd.Solver.from_kappa(kappa, params, WALLS, spacing=spacing) as solver:
            t1 = time.perf_counter()
            solver.solve(b, cycles=2)                              # (warm: first-use formats)
            t2 = time.perf_counter()
            u, info = solver.solve(b)
            t3 = time.perf_counter()
        reached = info["norm"] <= 1e-8 * info["rhs_norm"]
        axis = info.get("lineAxis")
        say("%-14s %-7s %8s %14.3e %10.1f %12.2f %12.3f%s"
            % (smoother, "%s(%.1f)" % (cycle, alpha), "%d%s" % (info["cycle"], "" if reached else "+"), info["norm"] / info["rhs_norm"],
               1e3 * (t1 - t0), 1e3 * (t3 - t2), 1e3 * (t3 - t2) / max(info["cycle"], 1),
               "" if axis is None else "   (lines along axis %d)" % axis))
        results[(smoother, cycle)] = (info["cycle"], bool(reached))
    say("(a '+' after the cycles: not there after %d)" % limit)
    return results


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    beta = float(sys.argv[3]) if len(sys.argv) > 3 else 2.5
    run(n, levels, beta)


if __name__ == "__main__":
    main()
