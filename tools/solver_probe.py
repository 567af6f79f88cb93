#!/usr/bin/env python3
"""What does setting up once buy a loop of solves?  One process:
    python tools/solver_probe.py [N [grids]] [--out FILE]
7-point Poisson at N^3 (default 256; grids: down to 16^3), colour V(1,1) sweeps, FCG (accel='cg') around F-cycles with
overCorrection 1.8 to 1e-8 ||b||, STEPS steps with a new right-hand side each: b_0 = A x_0, b_k = 0.97 b_{k-1} + 0.03 A x_k
(x_k seeded uniform vectors: b drifts by a few per cent per step, as the source of a pressure equation does).  Three ways,
each with host arrays and with device arrays (PyTorch tensors), on the same sequence of b:
  (a) one mgSolve call per step (threshold = 1e-8 ||b_k||): the whole setup inside every call — the yardstick;
  (b) one openmg_amd.Solver, every step from zero (rtol = 1e-8);
  (c) one Solver, every step started from the previous step's u.
Wall time per call (time.perf_counter; every call returns with its result complete): setup ms once, ms per step as
median (min - max) over the steps, iterations per step.  Written to profiles/solver_<N>.txt."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import openmg_amd
from openmg_amd import _hip, operators

STEPS = 20
RTOL = 1e-8


def spread(v, fmt="%.2f"):
    return (fmt + " (" + fmt + " - " + fmt + ")") % (statistics.median(v), min(v), max(v))


def counts(v):
    return "%d" % v[0] if min(v) == max(v) else "%d - %d (first %d)" % (min(v), max(v), v[0])


def right_hand_sides(A, steps):
    rng = np.random.default_rng(12345)
    b = A @ rng.random(A.shape[0])
    out = [b]
    for _ in range(steps - 1):
        b = 0.97 * b + 0.03 * (A @ rng.random(A.shape[0]))
        out.append(b)
    return out


def probe(size, grids, say):
    shape = (size,) * 3
    A = operators.stencil_poisson(shape)
    say("7-point Poisson %d^3, %d grids, colour V(1,1) sweeps, accel='cg' around F-cycles with overCorrection 1.8, to %.0e ||b||; "
        "%d steps, b_k = 0.97 b_(k-1) + 0.03 A x_k; one process, one MI355X (%s)" % (size, grids, RTOL, STEPS, torch.cuda.get_device_name(0)))
    say("wall ms per call, median (min - max) over the steps; iterations per step")
    say("%-52s | %-9s | %-30s | %s" % ("way", "setup ms", "ms per step", "iterations per step"))
    base = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "smoother": "colour",
            "accel": "cg", "cycle": "F", "overCorrection": 1.8, "cycles": 200, "threshold": 0.0}
    bs = right_hand_sides(A, STEPS)
    norms = [float(np.linalg.norm(b)) for b in bs]
    openmg_amd.mgSolve(A, bs[0], dict(base, threshold=RTOL * norms[0], giveInfo=False))            # warm-up: runtime, code objects, clocks
    results = {}
    for where in ("host", "device"):
        def arr(b):
            return torch.tensor(b, device="cuda") if where == "device" else b

        def host(u):
            return u.cpu().numpy() if where == "device" else u

        # (a) mgSolve per step.  giveInfo off: the setup stays on the device, the cheaper of mgSolve's two routes; the count
        # comes from a Solver run on the same b below (the same loop, the same bits)
        ms = []
        for k, b in enumerate(bs):
            bk = arr(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u = openmg_amd.mgSolve(A, bk, dict(base, threshold=RTOL * norms[k]))
            ms.append(1e3 * (time.perf_counter() - t0))
        last_a = host(u)
        say("%-52s | %-9s | %-30s | %s" % ("(a) mgSolve per step, %s arrays" % where, "in step", spread(ms), "as (b)"))
        results[("a", where)] = ms
        # (b) one Solver, cold starts
        t0 = time.perf_counter()
        s = openmg_amd.Solver(A, dict(base, rtol=RTOL))
        setup = 1e3 * (time.perf_counter() - t0)
        ms, its = [], []
        for b in bs:
            bk = arr(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u, info = s.solve(bk)
            ms.append(1e3 * (time.perf_counter() - t0))
            its.append(info["cycle"])
        same = bool(np.array_equal(host(u), last_a))
        say("%-52s | %-9.1f | %-30s | %s" % ("(b) one Solver, every step from zero, %s arrays" % where, setup, spread(ms), counts(its)))
        results[("b", where)] = ms
        # (c) warm starts
        ms, its, u = [], [], None
        for b in bs:
            bk = arr(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u, info = s.solve(bk, initial=u)
            ms.append(1e3 * (time.perf_counter() - t0))
            its.append(info["cycle"])
        final = info["norm"] / info["rhs_norm"]
        s.close()
        say("%-52s | %-9s | %-30s | %s" % ("(c) the same Solver, from the previous u, %s arrays" % where, "-", spread(ms), counts(its)))
        say("    last step: (b)'s u equals (a)'s bit for bit: %s; (c) ends at ||r|| / ||b|| = %.2e" % (same, final))
        results[("c", where)] = ms
    for where in ("host", "device"):
        a, b, c = (statistics.median(results[(w, where)]) for w in "abc")
        say("%s arrays: (a) / (b) = %.1f, (a) / (c) = %.1f, (b) / (c) = %.2f (medians)" % (where, a / b, a / c, b / c))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    size = int(args[0]) if args else 256
    grids = int(args[1]) if len(args) > 1 else max(2, int(np.log2(size)) - 3)
    out = out or os.path.join(ROOT, "profiles", "solver_%d.txt" % size)
    torch.cuda.init()
    _hip.require_gpu()
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    probe(size, grids, say)
