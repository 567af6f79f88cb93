#!/usr/bin/env python3
"""What do F- and W-cycles and the over-correction factor (omg_hierarchy_set_cycle) cost and buy on the flagship problem?
    python tools/cycle_probe.py [N [grids]] [--out FILE]
7-point Poisson N^3 (default 256), `grids` grids (default 5), colour V(1,1), fp64, set up on the device, a seeded random
right-hand side.  For V / F / W with the factor in {1, 1.5, 1.8}:
  - ms per cycle: REPEATS batches of K resident cycles (omg_resident_cycles), each bracketed by hipEvents on the hierarchy's
    stream after a warm-up batch; median and range;
  - cycles and wall time (host clock around calls that end in a device synchronise; median of REPEATS solves) to
    ||r|| < 1e-8 ||b||: plain cycles (batches of 8 per device call) and accel='cg' (omg_resident_pcg);
    "diverged" = a norm above 1e6 ||b|| or not finite, "not reached" = LIMIT cycles without reaching the target.
Then dtype='mixed' once (F, 1.8, plain and cg, target 1e-8).  Everything is written to profiles/cycle_shapes_<N>.txt
(--out: somewhere else) and printed."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from openmg_amd import _hip, operators

K = 32
REPEATS = 5
LIMIT = 400
SETTINGS = [(s, a) for s in "VFW" for a in (1.0, 1.5, 1.8)]


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def plain_solve(h, b, tol, nb):
    """(cycles or None, why, seconds)"""
    h.resident_load(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    cycles = 0
    while cycles < LIMIT:
        got = h.resident_cycles(1, 1, 8)
        below = [k for k, v in enumerate(got) if v < tol]
        if below:
            return cycles + below[0] + 1, "", time.perf_counter() - t
        cycles += 8
        if not np.isfinite(got[-1]) or got[-1] > 1e6 * nb:
            return None, "diverged", time.perf_counter() - t
    return None, "not reached in %d" % LIMIT, time.perf_counter() - t


def cg_solve(h, b, tol):
    h.resident_load(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    its, norms, tn, bd = h.resident_pcg(1, 1, LIMIT, tol)
    dt = time.perf_counter() - t
    ok = (not bd) and len(norms) and norms[-1] < tol
    return (its if ok else None), ("" if ok else ("breakdown" if bd else "not reached in %d" % LIMIT)), dt, tn


def spread(v):
    return "%.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


def probe(size, grids, say):
    shape = (size,) * 3
    A0 = operators.stencil_poisson(shape)
    b = np.random.default_rng(7).standard_normal(A0.shape[0])
    nb = float(np.linalg.norm(b))
    tol = 1e-8 * nb
    stream = torch.cuda.Stream()
    say("7-point Poisson %d^3, %d grids, colour V(1,1), fp64; %s; batches of %d cycles, %d repeats: median (min - max)"
        % (size, grids, torch.cuda.get_device_name(0), K, REPEATS))
    say("%-5s %-5s | %-26s | %-32s | %-32s" % ("shape", "alpha", "ms per cycle", "plain: cycles, ms to 1e-8", "accel='cg': iterations, ms to 1e-8"))
    with _hip.Hierarchy.from_fine(A0, shape, grids - 1, smoother="colour") as h:
        h.set_stream(stream.cuda_stream)
        assert h.level_flags(0)["plane"]
        base = None
        for shape_key, alpha in SETTINGS:
            h.set_cycle(shape_key, alpha)
            h.resident_load(b)
            h.resident_cycles(1, 1, K)                                # warm-up: formats, buffers, clocks
            per = []
            for _ in range(REPEATS):
                h.resident_load(b)
                per.append(timed(stream, lambda: h.resident_cycles(1, 1, K)) / K)
            plain = [plain_solve(h, b, tol, nb) for _ in range(REPEATS)]
            cg_solve(h, b, tol)                                       # warm-up of the CG buffers
            cg = [cg_solve(h, b, tol) for _ in range(REPEATS)]
            p_txt = ("%d cycles, %s ms" % (plain[0][0], spread([1e3 * p[2] for p in plain]))) if plain[0][0] else plain[0][1]
            c_txt = ("%d iterations, %s ms" % (cg[0][0], spread([1e3 * c[2] for c in cg]))) if cg[0][0] else cg[0][1]
            say("%-5s %-5.1f | %-26s | %-32s | %-32s" % (shape_key, alpha, spread(per), p_txt, c_txt))
            if (shape_key, alpha) == ("V", 1.0):
                base = (statistics.median(per), statistics.median([p[2] for p in plain]) if plain[0][0] else None,
                        statistics.median([c[2] for c in cg]) if cg[0][0] else None)
            elif base:
                rel = ["cycle time x %.2f" % (statistics.median(per) / base[0])]
                if plain[0][0] and base[1]:
                    rel.append("plain solve time x %.2f of V's" % (statistics.median([p[2] for p in plain]) / base[1]))
                if cg[0][0] and base[2]:
                    rel.append("cg solve time x %.2f of V's cg" % (statistics.median([c[2] for c in cg]) / base[2]))
                if plain[0][0] and base[2]:
                    rel.append("plain solve / V's cg x %.2f" % (statistics.median([p[2] for p in plain]) / base[2]))
                say("              " + "; ".join(rel))
    with _hip.Hierarchy.from_fine(A0, shape, grids - 1, smoother="colour", dtype="mixed") as h:
        h.set_stream(stream.cuda_stream)
        for shape_key, alpha in (("V", 1.0), ("F", 1.8)):
            h.set_cycle(shape_key, alpha)
            plain_solve(h, b, tol, nb)
            plain = [plain_solve(h, b, tol, nb) for _ in range(REPEATS)]
            cg_solve(h, b, tol)
            cg = [cg_solve(h, b, tol) for _ in range(REPEATS)]
            p_txt = ("%d cycles, %s ms" % (plain[0][0], spread([1e3 * p[2] for p in plain]))) if plain[0][0] else plain[0][1]
            c_txt = ("%d iterations, %s ms, true residual %.2e ||b||" % (cg[0][0], spread([1e3 * c[2] for c in cg]), cg[0][3] / nb)) if cg[0][0] else cg[0][1]
            say("dtype='mixed' %s %.1f | plain (defect correction): %s | accel='cg': %s" % (shape_key, alpha, p_txt, c_txt))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    size = int(args[0]) if args else 256
    grids = int(args[1]) if len(args) > 1 else 5
    out = out or os.path.join(ROOT, "profiles", "cycle_shapes_%d.txt" % size)
    _hip.require_gpu()
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    probe(size, grids, say)
