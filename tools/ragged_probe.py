#!/usr/bin/env python3
"""What does a real hierarchy on a grid of any extent ('oddExtents': 'merge') cost, and what does it buy?

    python tools/ragged_probe.py [N ...]        # default 100 200; writes profiles/ragged_probe.txt (and prints it)

One MI355X, fp64, 'colour', V(1,1) sweeps, to ||r|| < 1e-8 ||b||.  Two operators: the constant-coefficient 7-point Poisson
operator and operators.stencil7_variable (per-row coefficients).  Per operator, in ONE process, these hierarchies are set up
side by side and then timed with the configurations alternating, the fastest round of each reported:

    N^3, 'oddExtents': 'merge'     every axis by 2 down to 3^3 (100 -> 50 -> 25 -> 12 -> 6 -> 3)
    N^3, named factors             today's best on the same grid: (2, 2, 2) down to the first odd extent (25^3), whose
                                   15625 unknowns the coarsest level solves directly
    96^3 and 128^3, full           the even grids next to 100^3, for the cost per cell

For each: V cycles and F cycles with over-correction 1.8, cycles and ms per cycle, ns per cell and cycle, setup seconds, the
levels' grids with the kind of pass each smoothed level runs, and the coarsest size."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import openmg_amd
from openmg_amd import operators

ROUNDS, LIMIT = 2, 400


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


def halvings(extent, stop):
    """restrictions of an axis by 2 (rounded down) until the extent is <= stop"""
    n = 0
    while extent > stop:
        extent //= 2
        n += 1
    return n


def configurations(sizes):
    """(label, extent, parameters beyond the common ones)"""
    out = []
    for n in sizes:
        out.append(("%d^3 merge" % n, n, {"gridLevels": halvings(n, 3), "oddExtents": "merge"}))
        even = 0
        while (n >> even) % 2 == 0 and (n >> even) >= 4:
            even += 1
        if even and (n >> even) % 2:
            out.append(("%d^3 named to %d^3" % (n, n >> even), n, {"gridLevels": even, "coarsening": [(2, 2, 2)] * even}))
    for n in (96, 128):
        out.append(("%d^3 full" % n, n, {"gridLevels": halvings(n, 4)}))
    return out


def kinds_of(h):
    names = []
    for l in range(len(h.sizes) - 1):
        f = h.level_flags(l)
        names.append("plane" if f["plane"] else "var7" if f["var7"] else "27" if f["stencil27"] else "rows")
    return names


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [100, 200]
    out = []
    say = lambda line="": (out.append(line), print(line, flush=True))
    say("tools/ragged_probe.py %s: fp64, 'colour', V(1,1) sweeps, to ||r|| < 1e-8 ||b||, at most %d cycles; per operator one process-wide set of"
        " hierarchies, %d rounds alternating over the configurations, the fastest round of each" % (" ".join(map(str, sizes)), LIMIT, ROUNDS))
    for label, make in (("constant-coefficient Poisson (stencil_poisson)", operators.stencil_poisson),
                        ("per-row coefficients (stencil7_variable)", operators.stencil7_variable)):
        say()
        say(label)
        say("| grid, coarsening | levels (pass kind of each smoothed level) | coarsest | setup s | cycle | cycles | ms | ms per cycle | ns per cell and cycle | final ||r|| / ||b|| |")
        say("|---|---|---|---|---|---|---|---|---|---|")
        solvers, rhs, setup = {}, {}, {}
        for name, n, extra in configurations(sizes):
            shape = (n,) * 3
            A0 = make(shape)
            if n not in rhs:
                rhs[n] = np.random.default_rng(1).standard_normal(n ** 3)
            p = dict({"problemShape": shape, "preIterations": 1, "postIterations": 1, "cycles": 1, "threshold": 0.0, "smoother": "colour"}, **extra)
            t0 = time.perf_counter()
            solvers[name] = (openmg_amd.Solver(A0, p), n)
            solvers[name][0].hierarchy.sync()
            setup[name] = time.perf_counter() - t0
            del A0
        best = {}
        for rnd in range(ROUNDS + 1):                            # (round 0 warms: first-use formats, tunings)
            for name, (s, n) in solvers.items():
                b = rhs[n]
                for cyc, alpha in (("V", 1.0), ("F", 1.8)):
                    if rnd == 0:
                        cycles_to(s.hierarchy, b, cyc, alpha, 0.0, 2)
                        continue
                    k, ms, norm = cycles_to(s.hierarchy, b, cyc, alpha, 1e-8 * float(np.linalg.norm(b)), LIMIT)
                    if (name, cyc) not in best or ms < best[name, cyc][1]:
                        best[name, cyc] = (k, ms, norm)
        for name, (s, n) in solvers.items():
            h = s.hierarchy
            nb = float(np.linalg.norm(rhs[n]))
            shapes = h.level_shapes if h.level_shapes is not None else [(n >> l,) * 3 for l in range(len(h.sizes))]
            levels = " ".join("%d^3%s" % (sh[0], "" if l + 1 == len(shapes) else "(" + kinds_of(h)[l] + ")") for l, sh in enumerate(shapes))
            for cyc, alpha in (("V", 1.0), ("F", 1.8)):
                k, ms, norm = best[name, cyc]
                say("| %s | %s | %d | %.2f | %s(%.1f) | %d%s | %.1f | %.3f | %.3f | %.2e |" % (name, levels, h.sizes[-1], setup[name], cyc, alpha, k,
                    "" if norm < 1e-8 * nb else " (not reached)", ms, ms / k, 1e6 * ms / k / n ** 3, norm / nb))
            s.close()
    path = os.path.join(ROOT, "profiles", "ragged_probe.txt")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
