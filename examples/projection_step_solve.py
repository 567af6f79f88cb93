#!/usr/bin/env python3
"""A variable-density pressure projection on one MI355X, and the heat balance of a heated channel: what a solution drives
through the cell faces, through `Solver.divergence` and `Solver.fluxes`.

    python examples/projection_step_solve.py [n] [grids]        (default 64, 4)

The projection: the unit box with n^3 cells, periodic along x, solid walls in y and z (Neumann walls without a value: nothing
passes).  W = (Wz, Wy, Wx) holds the face velocities times the face areas, random, and 1 / rho varies over a factor of e^2.
Each step makes the field discretely divergence-free:

    b = s.divergence(W)                           the cell balance of W
    q, info = s.solve(b)                          -div((1 / rho) grad q) = b, the constants projected out
    s.fluxes(kappa, q, out=W, alpha=-1.0)         W = W - F(q), F the operator's own face fluxes of q

The balance of the corrected W is b - A q, the solve's residual, up to rounding — because the fluxes are made with the
operator's own face coefficients, their differences ARE its rows; a restatement with other roundings would leave the
truncation error of the restatement instead.  With a GPU visible to torch every array of the run is a device array and
nothing but the norms crosses to the host.

The heated channel is that of examples/heated_wall_solve.py with heat entering through the floor: the heat that leaves
through each wall is the sum of that wall's face fluxes, and in the steady state their total vanishes — what enters through
the floor leaves through the hot and the cold wall."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from openmg_amd import operators  # noqa: E402

from heated_wall_solve import WALLS as CHANNEL_WALLS, channel  # noqa: E402

WALLS = ("neumann", "neumann", "neumann", "neumann", "periodic", "periodic")       # -z, +z, -y, +y, -x, +x


def device():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except ImportError:
        return None


def norm(a):
    return float(np.linalg.norm(a)) if isinstance(a, np.ndarray) else float(a.norm())


def total(a):
    return float(a.sum())


def face_velocities(rng, shape):
    """Random face velocities (times area): none through the solid walls, the two seam faces of x equal."""
    W = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
    W[0][0] = W[0][-1] = 0.0
    W[1][:, 0] = W[1][:, -1] = 0.0
    W[2][:, :, -1] = W[2][:, :, 0]
    return W


def projection(n, grids, steps=3, say=print):
    """Returns the largest ||divergence(W)|| / ||b|| after a step."""
    torch = device()
    shape = (n,) * 3
    rng = np.random.default_rng(7)
    spacing = tuple(np.full(n + 2, 1.0 / n) for _ in range(3))
    kappa = np.exp(rng.uniform(-1.0, 1.0, size=(n + 2,) * 3))                       # 1 / rho, with a ghost layer nothing reads
    to_device = (lambda a: torch.from_numpy(a).cuda()) if torch else (lambda a: a)
    kappa = to_device(kappa)
    W = [to_device(a) for a in face_velocities(rng, shape)]
    params = {"gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg", "cycle": "F",
              "overCorrection": 1.8, "threshold": 0.0, "cycles": 200, "rtol": 1e-8, "nullspace": "constant"}
    worst = 0.0
    say("projection: %d^3 cells, %d grids, %s arrays" % (n, grids, "device" if torch else "host"))
    with openmg_amd.Solver.from_kappa(kappa, params, WALLS, spacing=spacing) as s:
        for step in range(steps):
            b = s.divergence(W)
            q, info = s.solve(b)
            s.fluxes(kappa, q, out=W, alpha=-1.0)
            after = norm(s.divergence(W)) / norm(b)
            worst = max(worst, after)
            say("step %d: %2d FCG iterations, ||divergence(W)|| / ||b|| = %.3e after the correction, the solver's ||r|| / ||b|| = %.3e"
                % (step, info["cycle"], after, info["norm"] / norm(b)))
            # the next step's forcing: new velocities on top of the divergence-free ones
            for a, more in zip(W, face_velocities(rng, shape)):
                a += 0.1 * to_device(more)
    return worst


def heat_balance(n, grids, say=print):
    """Returns |the total heat leaving| / the heat injected through the floor."""
    torch = device()
    kappa, spacing, values = channel(n)
    values[0] = -values[0]              # kappa dT/dn > 0 along the outward normal: -kappa grad T points INTO the box, heat enters
    areas = np.multiply.outer(spacing[1][1:-1], spacing[2][1:-1])
    injected = float((values[0] * areas).sum())
    if torch:
        kappa = torch.from_numpy(kappa).cuda()
        values = [torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v for v in values]
    params = {"gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg", "cycle": "F",
              "overCorrection": 1.8, "threshold": 0.0, "cycles": 200, "rtol": 1e-10}
    with openmg_amd.Solver.from_kappa(kappa, params, CHANNEL_WALLS, spacing=spacing) as s:
        b = s.rhs(kappa, values=values)
        T, info = s.solve(b)
        Fz, Fy, Fx = s.fluxes(kappa, T, values)
    # F is the flux along +axis: what LEAVES through a low wall is -F[0], through a high wall +F[e]
    leaving = {"floor (-z)": -total(Fz[0]), "lid (+z)": total(Fz[-1]), "hot wall (-y)": -total(Fy[:, 0]), "cold wall (+y)": total(Fy[:, -1])}
    say("heated channel: %d^3 cells, %d FCG iterations, ||r|| / ||b|| = %.3e; heat injected through the floor %.6e"
        % (n, info["cycle"], info["norm"] / info["rhs_norm"], injected))
    for name, heat in leaving.items():
        say("  heat leaving through the %-14s %+.6e" % (name + ":", heat))
    balance = sum(leaving.values())
    say("  total %+.3e, %.3e of the injected heat (x is periodic: what leaves through +x enters through -x, the same face)"
        % (balance, abs(balance) / injected))
    return abs(balance) / injected


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    projection(n, grids)
    heat_balance(n, grids)


if __name__ == "__main__":
    main()
