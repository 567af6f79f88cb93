#!/usr/bin/env python3
"""A heated wall on one MI355X: -div(kappa grad T) = 0 in a channel with inhomogeneous boundary data, through
`Solver.from_kappa`, `Solver.rhs` and `Solver.matvec`.

    python examples/heated_wall_solve.py [n] [grids]        (default 64, 4)

The channel is the unit box with n^3 cells: periodic along x, the hot wall T = 1 at y = 0 and the cold wall T = 0 at y = 1
(the y cells clustered towards both walls by a tanh map; ghost widths 0, so the values sit on the wall faces), a heat flux
q(x, y) INTO the box through the floor z = 0 (a Neumann wall: the value is the outward flux kappa dT/dn, so a flux into
the box is negative) and an insulated lid z = 1 (a Neumann wall without a value).  kappa varies smoothly over a factor of
six.  The operator is assembled in HBM from the field and the widths; `s.rhs(kappa, values=...)` makes the right-hand side
that belongs to it — the wall coefficients times the wall temperatures, the fluxes times the face areas — in one launch,
`s.solve` solves, and `s.matvec(T)` forms b - A T where T lives.  With a GPU visible to torch every array of the run is a
device array and nothing but the norms crosses to the host."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402

WALLS = ("neumann", "neumann", "dirichlet", "dirichlet", "periodic", "periodic")       # -z, +z, -y, +y, -x, +x


def channel(n, beta=1.5):
    """(kappa with its ghost layer, the widths (hz, hy, hx) with theirs, the six wall values)."""
    faces_y = 0.5 * (1.0 + np.tanh(beta * np.linspace(-1.0, 1.0, n + 1)) / np.tanh(beta))
    uniform = np.full(n, 1.0 / n)
    spacing = tuple(np.concatenate(([0.0], w, [0.0])) for w in (uniform, np.diff(faces_y), uniform))
    c = (np.arange(-1, n + 1) + 0.5) / n                                            # uniform centres, ghost cells included
    cy = np.concatenate(([0.0], 0.5 * (faces_y[1:] + faces_y[:-1]), [1.0]))         # (ghost width 0: the ghost "centre" is the wall)
    Z, Y, X = np.meshgrid(c, cy, c, indexing="ij")
    kappa = np.exp(np.log(6.0) * 0.5 * np.sin(2.0 * np.pi * X) * np.cos(np.pi * Y) * (1.0 - 0.5 * Z))
    y, x = np.meshgrid(cy[1:-1], c[1:-1], indexing="ij")
    floor_flux = -0.5 * np.sin(np.pi * y) * (1.0 + 0.5 * np.cos(2.0 * np.pi * x))   # outward, so negative: heat enters
    return kappa, spacing, [floor_flux, None, 1.0, 0.0, None, None]


def run(n, grids, say=print):
    """Returns the relative residual ||b - A T|| / ||b|| formed with matvec."""
    kappa, spacing, values = channel(n)
    on_device = False
    try:
        import torch
        on_device = torch.cuda.is_available()
    except ImportError:
        pass
    if on_device:
        kappa = torch.from_numpy(kappa).cuda()
        values = [torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v for v in values]
    params = {"gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg", "cycle": "F",
              "overCorrection": 1.8, "threshold": 0.0, "cycles": 200, "rtol": 1e-10}
    with openmg_amd.Solver.from_kappa(kappa, params, WALLS, spacing=spacing) as s:
        b = s.rhs(kappa, values=values)
        T, info = s.solve(b)
        r = b - s.matvec(T)
        if on_device:
            norm_r, norm_b = float(torch.linalg.norm(r)), float(torch.linalg.norm(b))
            lo, hi, mean_floor = float(T.min()), float(T.max()), float(T.reshape(n, n, n)[0].mean())
        else:
            norm_r, norm_b = float(np.linalg.norm(r)), float(np.linalg.norm(b))
            lo, hi, mean_floor = float(T.min()), float(T.max()), float(T.reshape(n, n, n)[0].mean())
    say("%d^3 cells, %d grids, %s arrays: %d FCG iterations, the solver's ||r|| / ||b|| = %.3e"
        % (n, grids, "device" if on_device else "host", info["cycle"], info["norm"] / info["rhs_norm"]))
    say("T in [%.4f, %.4f], mean over the heated floor's cells %.4f" % (lo, hi, mean_floor))
    say("||b - s.matvec(T)|| / ||b|| = %.3e" % (norm_r / norm_b))
    return norm_r / norm_b


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    run(n, grids)


if __name__ == "__main__":
    main()
