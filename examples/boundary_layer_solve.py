#!/usr/bin/env python3
"""A boundary-layer grid on one MI355X through `openmg_amd.Solver.from_kappa(..., spacing=...)`: -div(kappa grad u) = 1 on
the unit box, u = 0 on every wall, with the z faces clustered towards the wall z = 0,

    z_f = 1 - tanh(beta (1 - m / n)) / tanh(beta),   m = 0 .. n,

so the cells at the wall are thin (at n = 128, beta = 2 the widest z cell is 14 times the narrowest one and the cells at
the wall are 7 times as wide as high).  y and x are uniform.

    python examples/boundary_layer_solve.py [n] [grids] [beta]        (default 64, 4, 2.0)

The solver is made from the field and the cell widths themselves — kappa with one ghost layer, three 1-D width arrays
with one ghost entry at each end, here 0: the Dirichlet value sits on the wall face — and the 7-point finite-volume
operator is assembled in HBM; no matrix is made on the host where the setup takes the device route ('colour').  The
operator is the volume-integrated one, so the right-hand side is f * operators.cell_volumes(spacing).  Three smoothers
meet the same grid: 'colour' (point Gauss-Seidel: the thin cells couple strongly along z and slow it down), 'line' (zebra
lines along z, the axis the library finds by itself) and 'line' with F-cycles and an over-correction of 1.8.  Then the
field changes a few times and every solver takes the new one with `update_kappa`; the widths are the solver's own.
('line' is set up through the host lists, so its update_kappa builds a new hierarchy, as Solver.update does.)
At 128^3 only the third arrives at 1e-8 within the 200 cycles allowed here (profiles/stretched_256.txt).
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from openmg_amd import operators  # noqa: E402


def tanh_faces(n, beta):
    return 1.0 - np.tanh(beta * (1.0 - np.arange(n + 1) / n)) / np.tanh(beta)


def grid(n, beta):
    """The widths (hz, hy, hx) with ghost entries 0, and the cell centres with the ghost centres half a cell outside."""
    faces = [tanh_faces(n, beta), np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1)]
    widths = [np.diff(f) for f in faces]
    spacing = tuple(np.concatenate(([0.0], w, [0.0])) for w in widths)
    centres = [np.concatenate(([f[0] - 0.5 * w[0]], 0.5 * (f[1:] + f[:-1]), [f[-1] + 0.5 * w[-1]])) for f, w in zip(faces, widths)]
    return spacing, np.meshgrid(*centres, indexing="ij")


VARIANTS = [("colour", {"smoother": "colour"}), ("line", {"smoother": "line"}),
            ("line, F-cycle, overCorrection 1.8", {"smoother": "line", "cycle": "F", "overCorrection": 1.8})]


def run(n, grids, beta, steps=3, say=print):
    """Every variant: setup, a solve, `steps` updates of kappa with a solve each.  Returns {variant: [cycles of every solve]}."""
    spacing, (Z, Y, X) = grid(n, beta)

    def kappa_at(t):
        return 1.0 + 0.5 * np.sin(2.0 * Z + Y + 3.0 * t) * np.cos(X)

    b = operators.cell_volumes(spacing).ravel()                   # f = 1
    hz = spacing[0][1:-1]
    say("%d^3 cells, %d grids, beta %.2f: z cells %.2e .. %.2e (ratio %.1f), the wall cells %.1f times as wide as high"
        % (n, grids, beta, hz.min(), hz.max(), hz.max() / hz.min(), (1.0 / n) / hz[0]))
    counts = {}
    for name, more in VARIANTS:
        params = dict({"gridLevels": grids, "preIterations": 1, "postIterations": 1, "threshold": 0.0, "cycles": 200, "rtol": 1e-8}, **more)
        t0 = time.perf_counter()
        with openmg_amd.Solver.from_kappa(kappa_at(0.0), params, spacing=spacing) as solver:
            t1 = time.perf_counter()
            u, info = solver.solve(b)
            t2 = time.perf_counter()
            axis = info.get("lineAxis")
            say("%s%s: setup %.1f ms, updates in place: %s" % (name, "" if axis is None else " (lines along axis %d)" % axis, 1e3 * (t1 - t0),
                                                               solver.hierarchy.can_update_fine()))
            say("    %4s %8s %14s %12s %12s" % ("step", "cycles", "||r|| / ||b||", "update ms", "solve ms"))
            say("    %4d %8d %14.3e %12s %12.2f" % (0, info["cycle"], info["norm"] / info["rhs_norm"], "-", 1e3 * (t2 - t1)))
            counts[name] = [info["cycle"]]
            for step in range(1, steps + 1):
                t0 = time.perf_counter()
                solver.update_kappa(kappa_at(step / steps))
                t1 = time.perf_counter()
                u, info = solver.solve(b, initial=u)
                t2 = time.perf_counter()
                say("    %4d %8d %14.3e %12.2f %12.2f" % (step, info["cycle"], info["norm"] / info["rhs_norm"], 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
                counts[name].append(info["cycle"])
    return counts


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    beta = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
    run(n, grids, beta)


if __name__ == "__main__":
    main()
