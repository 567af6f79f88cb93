#!/usr/bin/env python3
"""A time loop whose coefficient field changes every step, on one MI355X through `openmg_amd.Solver.from_kappa`: implicit
diffusion (1 / dt - div(kappa grad)) u = u_old / dt with a conductivity that follows a moving front.

    python examples/variable_density_solve.py [extent] [steps]        (default 128, 10)

The solver is made from the field itself — kappa with one ghost layer, Neumann walls, sigma = 1 / dt, scale = 1 / h^2 —
and every step hands it the new field with `update_kappa`: the 7-point operator is assembled in HBM and goes straight
into the hierarchy's update, no matrix is ever made on the host.  Where PyTorch sees a GPU the field, the right-hand
side and the solution are device tensors and a step moves nothing over PCIe; without it they are NumPy arrays and the
same calls upload them.  (`operators.stencil7_kappa(kappa, walls, sigma, scale)` is the matrix the solver works with.)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

try:                                   # (device arrays: PyTorch first, before the library touches the GPU)
    import torch
    ON_DEVICE = torch.cuda.is_available()
except ImportError:
    ON_DEVICE = False
import openmg_amd  # noqa: E402


def main():
    extent = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    shape = (extent,) * 3
    h, dt = 1.0 / extent, 1.0e-3
    grids = max(2, int(np.log2(extent)) - 2)
    xp = torch if ON_DEVICE else np
    kw = {"dtype": torch.float64, "device": "cuda"} if ON_DEVICE else {}
    # cell centres, ghost layer included
    c = (xp.arange(extent + 2, **kw) - 0.5) * h
    zz, yy, xx = xp.meshgrid(c, c, c, indexing="ij")

    def kappa_at(t):                   # conductivity 100 behind a front that moves along x, 1 ahead of it
        front = 0.25 + 0.5 * t
        return 1.0 + 99.0 * 0.5 * (1.0 - xp.tanh((xx + 0.1 * xp.sin(6.28 * yy) - front) / (2 * h)))

    walls = ("neumann",) * 6
    scale = (1.0 / h ** 2,) * 3
    params = {"gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg", "threshold": 0.0,
              "cycles": 200, "rtol": 1e-8}
    u = xp.exp(-((xx - 0.5) ** 2 + (yy - 0.5) ** 2 + (zz - 0.5) ** 2) / 0.02)[1:-1, 1:-1, 1:-1].reshape(-1)
    if ON_DEVICE:
        u = u.contiguous()
    t0 = time.perf_counter()
    with openmg_amd.Solver.from_kappa(kappa_at(0.0), params, walls=walls, sigma=1.0 / dt, scale=scale) as solver:
        print("%d^3 cells, %d grids, %s arrays; setup %.1f ms; updates in place: %s"
              % (extent, grids, "device" if ON_DEVICE else "host", 1e3 * (time.perf_counter() - t0), solver.hierarchy.can_update_fine()))
        print("%4s %10s %14s %12s %12s" % ("step", "iterations", "||r|| / ||b||", "update ms", "solve ms"))
        for step in range(1, steps + 1):
            t0 = time.perf_counter()
            solver.update_kappa(kappa_at(step / steps), sigma=1.0 / dt)
            t1 = time.perf_counter()
            u, info = solver.solve(u / dt, initial=u)
            t2 = time.perf_counter()
            print("%4d %10d %14.3e %12.2f %12.2f" % (step, info["cycle"], info["norm"] / info["rhs_norm"], 1e3 * (t1 - t0), 1e3 * (t2 - t1)))


if __name__ == "__main__":
    main()
