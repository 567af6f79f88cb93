#!/usr/bin/env python3
"""What does semicoarsening ('coarsening': 'auto') buy, and what does it cost?

    python tools/semicoarsen_probe.py N        # writes profiles/semicoarsen_N.txt (and prints it)

The operator of tools/line_probe.py — N^3 cells, a 7-point operator with per-cell coefficients — with couplings
(x : y : z) 100 : 1 : 1, 100 : 100 : 1 and 100 : 10 : 1, x the unit-stride axis.  Per operator, in one process, the
configurations alternating and the best of the rounds reported: cycles and wall milliseconds to ||r|| < 1e-8 ||b|| for the
smoothers 'colour' and 'line', coarsening 'full' and 'auto', cycle shapes V and F(1.8), V(1,1) sweeps, fp64.  Then the setup
time of 'auto' on the device route (omg_hierarchy_create_from_fine_semi) against the lists route (giveInfo) for 'colour'."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import openmg_amd
from line_probe import face_operator

ROUNDS, LIMIT = 2, 600


def cycles_to(h, b, shape, alpha, target, limit):
    h.set_cycle(shape, alpha)
    h.resident_load(b)
    h.sync()
    t0 = time.perf_counter()
    k, norm = 0, float("inf")
    while k < limit and not norm < target:
        norm = h.resident_cycle(1, 1)
        k += 1
    return k, 1e3 * (time.perf_counter() - t0), norm


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    shape = (size,) * 3
    grids = max(2, int(np.log2(size)) - 2)                     # full coarsening: down to 8^3
    out = []
    say = lambda line="": (out.append(line), print(line, flush=True))
    say("tools/semicoarsen_probe.py %d: %d^3 cells, at most %d grids, per-cell coefficients; to ||r|| < 1e-8 ||b||, V(1,1) sweeps, fp64,"
        " at most %d cycles; %d rounds alternating over the configurations, the fastest round of each" % (size, size, grids, LIMIT, ROUNDS))
    b = np.random.default_rng(1).standard_normal(size ** 3)
    nb = float(np.linalg.norm(b))
    base = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "cycles": 1, "threshold": 0.0}
    for label, factors in (("100 : 1 : 1", (1.0, 1.0, 100.0)), ("100 : 100 : 1", (1.0, 100.0, 100.0)), ("100 : 10 : 1", (1.0, 10.0, 100.0))):
        A0 = face_operator(shape, factors, seed=7)
        say()
        say("couplings x : y : z = %s" % label)
        say("| smoother | coarsening | factors (z y x per restriction) -> coarsest grid | cycle | cycles | ms | ms per cycle | final ||r|| / ||b|| |")
        say("|---|---|---|---|---|---|---|---|")
        solvers = {}
        for kind in ("colour", "line"):
            for coarsening in ("full", "auto"):
                solvers[kind, coarsening] = openmg_amd.Solver(A0, dict(base, smoother=kind, coarsening=coarsening))
        best = {}
        for rnd in range(ROUNDS + 1):                            # (round 0 warms: first-use formats, tunings)
            for key, s in solvers.items():
                for cyc, alpha in (("V", 1.0), ("F", 1.8)):
                    if rnd == 0:
                        cycles_to(s.hierarchy, b, cyc, alpha, 0.0, 2)
                        continue
                    k, ms, norm = cycles_to(s.hierarchy, b, cyc, alpha, 1e-8 * nb, LIMIT)
                    if (key, cyc) not in best or ms < best[key, cyc][1]:
                        best[key, cyc] = (k, ms, norm)
        for (kind, coarsening), s in solvers.items():
            h = s.hierarchy
            how = "every axis by 2, %d grids" % len(h.sizes)
            if h.coarsening is not None:
                how = "%s -> %s" % (" ".join("".join(str(f) for f in e) for e in h.coarsening), "x".join(str(v) for v in h.level_shapes[-1]))
            for cyc, alpha in (("V", 1.0), ("F", 1.8)):
                k, ms, norm = best[(kind, coarsening), cyc]
                say("| %s | %s | %s | %s(%.1f) | %d%s | %.1f | %.3f | %.2e |" % (kind, coarsening, how, cyc, alpha, k,
                    "" if norm < 1e-8 * nb else " (not reached)", ms, ms / k, norm / nb))
            s.close()
        if label == "100 : 100 : 1":
            say()
            say("setup of 'colour' with coarsening 'auto' on that operator, seconds, %d alternations:" % ROUNDS)
            times = {"device route": [], "lists route (giveInfo)": []}
            for _ in range(ROUNDS):
                for name, give in (("device route", False), ("lists route (giveInfo)", True)):
                    t0 = time.perf_counter()
                    s = openmg_amd.Solver(A0, dict(base, smoother="colour", coarsening="auto", giveInfo=give))
                    s.hierarchy.sync()
                    times[name].append(time.perf_counter() - t0)
                    s.close()
            for name, ts in times.items():
                say("  %-24s %s" % (name, "  ".join("%.3f" % t for t in ts)))
    path = os.path.join(ROOT, "profiles", "semicoarsen_%d.txt" % size)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
