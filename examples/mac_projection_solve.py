#!/usr/bin/env python3
"""A two-fluid pressure projection on a MAC grid on one MI355X, with the coefficients where such a code holds them: on the
faces, through `Solver.from_faces`, `Solver.fluxes` and `Solver.update_faces`.

    python examples/mac_projection_solve.py [n] [grids]        (default 64, 4)

The unit box with n^3 cells and solid walls all round (Neumann walls without a value: nothing passes).  A drop of a fluid
a hundred times as heavy as its surroundings drifts along x.  The code holds beta = 1 / rho on the FACES —
here from the arithmetic mean of the two cells' densities, as a volume-of-fluid code would from its face fractions — and the
same beta has to stand in the pressure operator and in the velocity correction.  C = beta * area / distance per face are the
three coefficient arrays; W = (Wz, Wy, Wx) holds the face velocities times the face areas.  Each step:

    b = s.divergence(W)                           the cell balance of W
    q, info = s.solve(b)                          -div(beta grad q) = b, the constants projected out
    s.fluxes(C, q, out=W, alpha=-1.0)             W = W - C (q_lo - q_hi), with the operator's own coefficients
    s.update_faces(C_next)                        the operator of the next density — in place where the hierarchy takes new
                                                  coefficients (by default from 128^3 on), else a new hierarchy

The balance of the corrected W is b - A q, the solve's residual, up to rounding: the fluxes are made with the very numbers
the operator holds.  With a GPU visible to torch every array of the run is a device array — the densities, the coefficients
made from them with torch operations, W, b and q — and nothing but the norms crosses to the host."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmg_amd  # noqa: E402
from openmg_amd import operators  # noqa: E402

WALLS = ("neumann",) * 6                    # -z, +z, -y, +y, -x, +x
HEAVY = 100.0


def device():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except ImportError:
        return None


def norm(a):
    return float(np.linalg.norm(a)) if isinstance(a, np.ndarray) else float(a.norm())


def density(n, centre):
    """rho per cell: a drop of radius 0.2 around (0.5, 0.5, centre)."""
    c = (np.arange(n) + 0.5) / n
    r2 = (c[:, None, None] - 0.5) ** 2 + (c[None, :, None] - 0.5) ** 2 + (c[None, None, :] - centre) ** 2
    return np.where(r2 < 0.04, HEAVY, 1.0)


def coefficients(rho, zeros):
    """(Cz, Cy, Cx) = area / distance / (the arithmetic mean of rho over the face's two cells) = (1 / n) * 2 / (rho_lo + rho_hi),
    with slices that NumPy arrays and torch tensors share.  The faces of the solid walls keep 0: a Neumann wall's faces are
    never read."""
    n = rho.shape[0]
    h = 1.0 / n
    Cz, Cy, Cx = (zeros(s) for s in operators.face_shapes(rho.shape))
    Cz[1:-1] = 2.0 * h / (rho[:-1] + rho[1:])
    Cy[:, 1:-1] = 2.0 * h / (rho[:, :-1] + rho[:, 1:])
    Cx[:, :, 1:-1] = 2.0 * h / (rho[:, :, :-1] + rho[:, :, 1:])
    return [Cz, Cy, Cx]


def face_velocities(rng, shape):
    """Random face velocities (times area): none through the solid walls."""
    W = [rng.standard_normal(s) for s in operators.face_shapes(shape)]
    W[0][0] = W[0][-1] = 0.0
    W[1][:, 0] = W[1][:, -1] = 0.0
    W[2][:, :, 0] = W[2][:, :, -1] = 0.0
    return W


def projection(n, grids, steps=3, say=print):
    """Returns the largest ||divergence(W)|| / ||b|| after a step."""
    torch = device()
    shape = (n,) * 3
    rng = np.random.default_rng(7)
    to_device = (lambda a: torch.from_numpy(a).cuda()) if torch else (lambda a: a)
    zeros = (lambda s: torch.zeros(s, dtype=torch.float64, device="cuda")) if torch else np.zeros
    W = [to_device(a) for a in face_velocities(rng, shape)]
    params = {"gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg", "threshold": 0.0,
              "cycles": 200, "rtol": 1e-8, "nullspace": "constant"}
    worst = 0.0
    say("MAC projection: %d^3 cells, %d grids, density ratio %g, %s arrays" % (n, grids, HEAVY, "device" if torch else "host"))
    C = coefficients(to_device(density(n, 0.3)), zeros)
    with openmg_amd.Solver.from_faces(C, params, WALLS) as s:
        for step in range(steps):
            b = s.divergence(W)
            q, info = s.solve(b)
            s.fluxes(C, q, out=W, alpha=-1.0)
            after = norm(s.divergence(W)) / norm(b)
            worst = max(worst, after)
            say("step %d: %2d FCG iterations, ||divergence(W)|| / ||b|| = %.3e after the correction, the solver's ||r|| / ||b|| = %.3e"
                % (step, info["cycle"], after, info["norm"] / norm(b)))
            # the next step: the drop has moved on, new velocities on top of the divergence-free ones
            C = coefficients(to_device(density(n, 0.3 + 0.1 * (step + 1))), zeros)
            s.update_faces(C)
            for a, more in zip(W, face_velocities(rng, shape)):
                a += 0.1 * to_device(more)
    return worst


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grids = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    projection(n, grids)


if __name__ == "__main__":
    main()
