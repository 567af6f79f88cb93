#!/usr/bin/env python3
"""What does starting each solve from a projection onto earlier solutions buy a loop of solves?  One process:
    python tools/projection_probe.py [N [grids]] [--out FILE]
tools/solver_probe.py's scenario — 7-point Poisson at N^3 (default 256; grids: down to 16^3), colour V(1,1) sweeps, FCG
(accel='cg') around F-cycles with overCorrection 1.8 to 1e-8 ||b||, STEPS steps, b_0 = A x_0, b_k = 0.97 b_{k-1} + 0.03 A x_k
(x_k seeded uniform vectors), device arrays (PyTorch tensors) — three ways, INTERLEAVED step by step in one process, each on
a Solver of its own:
  (z) every step from zero;
  (w) every step from the previous step's u (initial=u_prev);
  (p) Solver(..., projection=8): every step from the projection onto the earlier solutions.
Per step: iterations, and wall ms of the solve call (time.perf_counter; the call returns with u complete).  The project
and update parts of (p) are timed apart, between hipEvents on the hierarchy's stream, in a second pass over the same steps
driven entry by entry as solve() drives them.  Last, the inner-product launch alone
(omg_resident_projection_time: REPS launches between hipEvents after a warm-up) as GB/s on its (l + 1) n 8 bytes, beside
pcg.hip's dot_kernel on two vectors of the same n in the same run (2 n 8 bytes).
No figure is fixed in advance: the yardsticks are the other two ways of the same run and dot_kernel.
Written to profiles/projection_<N>.txt."""
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
CAPACITY = 8
REPS = 20


def spread(v, fmt="%.2f"):
    return (fmt + " - " + fmt + " - " + fmt) % (min(v), statistics.median(v), max(v))


def right_hand_sides(A, steps):
    rng = np.random.default_rng(12345)
    b = A @ rng.random(A.shape[0])
    out = [b]
    for _ in range(steps - 1):
        b = 0.97 * b + 0.03 * (A @ rng.random(A.shape[0]))
        out.append(b)
    return out


def timed(stream, fn):
    """(fn(), ms between two events on the stream)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    result = fn()
    e1.record(stream)
    e1.synchronize()
    return result, e0.elapsed_time(e1)


def probe(size, grids, say):
    shape = (size,) * 3
    A = operators.stencil_poisson(shape)
    n = A.shape[0]
    say("7-point Poisson %d^3, %d grids, colour V(1,1) sweeps, accel='cg' around F-cycles with overCorrection 1.8, to %.0e ||b||; "
        "%d steps, b_k = 0.97 b_(k-1) + 0.03 A x_k; device arrays; one process, one MI355X (%s)"
        % (size, grids, RTOL, STEPS, torch.cuda.get_device_name(0)))
    base = {"problemShape": shape, "gridLevels": grids - 1, "preIterations": 1, "postIterations": 1, "smoother": "colour",
            "accel": "cg", "cycle": "F", "overCorrection": 1.8, "cycles": 200, "threshold": 0.0, "rtol": RTOL}
    bs = right_hand_sides(A, STEPS)
    zero, warm = openmg_amd.Solver(A, base), openmg_amd.Solver(A, base)
    proj = openmg_amd.Solver(A, base, projection=CAPACITY)
    warm_up = torch.tensor(bs[0], device="cuda")
    for s in (zero, warm):
        s.solve(warm_up)                                            # warm-up: runtime, code objects, clocks
    proj.solve(warm_up, project=False)

    say("")
    say("step | iterations: zero  warm  projected (vectors used) | ms: zero    warm    projected | start's ||r|| / ||b||: warm, projected")
    its = {"z": [], "w": [], "p": []}
    ms = {"z": [], "w": [], "p": []}
    u_prev = None
    last = {}
    for k, b in enumerate(bs):
        bk = torch.tensor(b, device="cuda")
        row = {}
        for way, call in (("z", lambda: zero.solve(bk)), ("w", lambda: warm.solve(bk, initial=u_prev)), ("p", lambda: proj.solve(bk))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u, info = call()
            ms[way].append(1e3 * (time.perf_counter() - t0))
            its[way].append(info["cycle"])
            row[way] = info
            last[way] = (u, info)
            if way == "w":
                u_prev = u
        say("%4d | %16d  %4d  %9d (%d)           | %8.2f  %6.2f  %9.2f  | %.1e, %.1e"
            % (k, its["z"][-1], its["w"][-1], its["p"][-1], row["p"]["projected"], ms["z"][-1], ms["w"][-1], ms["p"][-1],
               row["w"]["initial_norm"] / row["w"]["rhs_norm"], row["p"]["initial_norm"] / row["p"]["rhs_norm"]))
    say("")
    say("over the %d steps, min - median - max (step 0 is the same solve three times: no earlier solution exists)" % STEPS)
    say("%-34s | %-22s | %-28s | %s" % ("way", "iterations per step", "ms per step", "sum of iterations, of ms"))
    for way, name in (("z", "(z) from zero"), ("w", "(w) from the previous u"), ("p", "(p) projection=%d" % CAPACITY)):
        say("%-34s | %-22s | %-28s | %d, %.1f" % (name, spread(its[way], "%d"), spread(ms[way]), sum(its[way]), sum(ms[way])))
    for way in "zwp":
        say("    %s ends at ||r|| / ||b|| = %.2e" % (way, last[way][1]["norm"] / last[way][1]["rhs_norm"]))
    # the parts of (p) apart: the same steps once more on a hierarchy of its own, driven entry by entry as solve() drives them
    # (load, project, the two norms, FCG to the target, update), the hierarchy's work on a stream the events are recorded on
    parts = {"project": [], "update": []}
    hand = []
    stream = torch.cuda.Stream()
    with openmg_amd.Solver(A, base, projection=CAPACITY) as again:
        h = again.hierarchy
        h.set_stream(stream.cuda_stream)
        h.set_cycle("F", 1.8)
        for k, b in enumerate(bs):
            bk = torch.tensor(b, device="cuda")
            torch.cuda.synchronize()
            h.resident_load_dev(bk.data_ptr(), None)
            used, t = timed(stream, h.resident_project)
            h.sync()
            parts["project"].append((used, t))
            rhs_norm, start = h.resident_norms(rhs=True, residual=used > 0)
            if used > 0 and start < RTOL * rhs_norm:
                continue                                            # (as solve(): nothing to do, nothing joins the set)
            hand.append(h.resident_pcg(1, 1, 200, RTOL * rhs_norm)[0])
            (size_after, kept), t = timed(stream, h.resident_project_update)
            parts["update"].append((size_after, t))
    say("")
    say("the parts of (p), ms between hipEvents on the hierarchy's stream (update: until its status word is back), from a second pass "
        "over the steps driven entry by entry (%d iterations in all; solve() took %d)" % (sum(hand), sum(its["p"])))
    by = {}
    for used, t in parts["project"]:
        by.setdefault(used, []).append(t)
    for used in sorted(by):
        say("    project with %d vectors: %s ms (%d calls)" % (used, spread(by[used], "%.3f"), len(by[used])))
    by = {}
    for size_after, t in parts["update"]:
        by.setdefault(size_after, []).append(t)
    for size_after in sorted(by):
        say("    update leaving %d vectors: %s ms (%d calls)" % (size_after, spread(by[size_after], "%.3f"), len(by[size_after])))
    say("    project, all calls: %s ms; update, all calls: %s ms; a step of (p) takes %s ms"
        % (spread([t for _, t in parts["project"]], "%.3f"), spread([t for _, t in parts["update"]], "%.3f"), spread(ms["p"])))
    say("")
    l = proj.projection_size
    dots, dot, comb = proj.hierarchy.projection_time(REPS)
    say("the launches alone, %d of each between hipEvents after a warm-up, n = %d doubles, the set holds l = %d vectors:" % (REPS, n, l))
    say("    inner products of b with the set (kernel + fold): %.3f ms = %.0f GB/s on (l + 1) n 8 = %.0f MB"
        % (dots, (l + 1) * n * 8 / dots / 1e6, (l + 1) * n * 8 / 1e6))
    say("    linear combination over the set:                  %.3f ms = %.0f GB/s on (l + 1) n 8 (l read, 1 written)"
        % (comb, (l + 1) * n * 8 / comb / 1e6))
    say("    pcg.hip dot_kernel on two vectors (kernel alone): %.3f ms = %.0f GB/s on 2 n 8" % (dot, 2 * n * 8 / dot / 1e6))
    for s in (zero, warm, proj):
        s.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    size = int(args[0]) if args else 256
    grids = int(args[1]) if len(args) > 1 else max(2, int(np.log2(size)) - 3)
    out = out or os.path.join(ROOT, "profiles", "projection_%d.txt" % size)
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
