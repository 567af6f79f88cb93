#!/usr/bin/env python3
"""What does nullspace='constant' cost?  One process:
    python tools/nullspace_probe.py [N [restrictions]] [--out FILE]
The zero-row-sum variable-coefficient operator of tests/test_gpu_nullspace.py (operators.stencil7_variable with its diagonal
replaced by minus the sum of its off-diagonals: pure Neumann) at N^3 (default 128), set up on the device with `restrictions`
restrictions (default: down to 8^3), colour V(1,1), fp64, a seeded right-hand side with mean 0.3 — and, in the same process,
the Dirichlet operators.stencil7_variable itself on an ordinary hierarchy:
  - ms per cycle: REPEATS batches of K resident cycles bracketed by hipEvents on the hierarchy's stream; median (min - max);
  - ms per FCG iteration: the same around omg_resident_pcg with K iterations and no threshold;
  - cycles (plain, batches of 8) and iterations (accel='cg') to 1e-8 relative — to ||b - mean b|| on the null-space hierarchy;
  - us per omg_resident_fetch_dev call (CALLS calls bracketed by hipEvents, each ending in a stream synchronise) on either
    hierarchy: the null-space one runs the projection's launches (partial sums, fold; subtraction) in front of the scatter,
    the difference is their cost in place.
Then the counts of the end-to-end test (16^3, threshold 1e-8 ||b - mean b||) through mgSolve.  OMG_VAR7_MIN defaults to 4096
here, as in the tests, so that level 0 runs the fused passes of var7.hip at every N.  Written to profiles/nullspace_<N>.txt."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMG_VAR7_MIN", "4096")
import numpy as np
import scipy.sparse as sp
import torch

import openmg_amd
from openmg_amd import _hip, operators

K = 32
REPEATS = 5
CALLS = 200
LIMIT = 400


def neumann_var(shape, seed=2024):
    A = sp.csr_matrix(operators.stencil7_variable(shape, seed))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    off = np.where(A.indices == rows, 0.0, A.data)
    diag = -np.add.reduceat(off, A.indptr[:-1])
    A.data = np.where(A.indices == rows, diag[rows], A.data)
    return A


def neumann_laplacian(shape):
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols = [], []
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [a, b]
        cols += [b, a]
    W = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A = sp.csr_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
    A.sort_indices()
    return A


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v, fmt="%.4f"):
    return (fmt + " (" + fmt + " - " + fmt + ")") % (statistics.median(v), min(v), max(v))


def measure(h, stream, b, tol, say, name):
    n = b.size
    h.resident_load(b)
    h.resident_cycles(1, 1, K)                                        # warm-up: formats, buffers, clocks
    per = []
    for _ in range(REPEATS):
        h.resident_load(b)
        per.append(timed(stream, lambda: h.resident_cycles(1, 1, K)) / K)
    h.resident_load(b)
    h.resident_pcg(1, 1, K, 0.0)
    cg = []
    for _ in range(REPEATS):
        h.resident_load(b)
        cg.append(timed(stream, lambda: h.resident_pcg(1, 1, K, 0.0)) / K)
    h.resident_load(b)
    cycles, norms = None, []
    while len(norms) < LIMIT and cycles is None:
        norms += h.resident_cycles(1, 1, 8)
        below = [k for k, v in enumerate(norms) if v < tol]
        cycles = below[0] + 1 if below else None
        if not np.isfinite(norms[-1]):
            break
    h.resident_load(b)
    its, cg_norms, true_norm, breakdown = h.resident_pcg(1, 1, LIMIT, tol)
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.resident_fetch_dev(out.data_ptr())
    fetch = [1e3 * timed(stream, lambda: [h.resident_fetch_dev(out.data_ptr()) for _ in range(CALLS)]) / CALLS for _ in range(REPEATS)]
    say("%-34s | %-28s | %-28s | %-14s | %-22s | %s"
        % (name, spread(per), spread(cg), "%s cycles" % (cycles if cycles else "> %d" % LIMIT),
           "%d iterations%s" % (its, " (breakdown)" if breakdown else ("" if len(cg_norms) and cg_norms[-1] < tol else " (not reached)")),
           spread(fetch, "%.1f")))
    return statistics.median(per), statistics.median(fetch), float(np.abs(out.cpu().numpy().mean()))


def probe(size, restrictions, say):
    shape = (size,) * 3
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(12345)
    say("7-point per-row coefficients %d^3, %d restrictions (coarsest %d^3), colour V(1,1), fp64, set up on the device; one process, one MI355X (%s)"
        % (size, restrictions, size >> restrictions, torch.cuda.get_device_name(0)))
    say("batches of %d cycles / iterations, %d repeats, %d fetch calls per repeat: median (min - max)" % (K, REPEATS, CALLS))
    say("%-34s | %-28s | %-28s | %-14s | %-22s | %s" % ("operator", "ms per cycle", "ms per FCG iteration", "to 1e-8", "accel='cg' to 1e-8", "us per fetch_dev call"))
    got = {}
    for name, A0, kind in (("pure Neumann, nullspace='constant'", neumann_var(shape), "constant"), ("Dirichlet stencil7_variable", operators.stencil7_variable(shape), None)):
        b = A0 @ rng.random(A0.shape[0]) + 0.3
        tol = 1e-8 * float(np.linalg.norm(b - b.mean() if kind else b))
        with _hip.Hierarchy.from_fine(A0, shape, restrictions, smoother="colour", nullspace=kind) as h:
            h.set_stream(stream.cuda_stream)
            flags = [k for l in range(restrictions) for k, v in h.level_flags(l).items() if v and k in ("var7", "plane", "stencil27")]
            got[kind] = measure(h, stream, b, tol, say, name) + (flags, h.coarse_info())
    for kind, (per, fetch, mean, flags, info) in got.items():
        say("  nullspace=%-10r fused levels %s; coarse solve: %s; |mean of the fetched iterate| %.2e" % (kind, flags, info, mean))
    say("projection in place (partial sums + fold + subtraction of %d doubles): %.1f us per fetch = null-space fetch - ordinary fetch"
        % (size ** 3, got["constant"][1] - got[None][1]))
    say("ms per cycle, null space / Dirichlet: %.3f (the same kernels on both; the explicit inverse of %d unknowns in place of the sine solve or inverse)"
        % (got["constant"][0] / got[None][0], got["constant"][4]["n"]))
    say("")
    say("mgSolve end to end at 16^3 (tests/test_gpu_nullspace.py case 4: b with mean 0.3, threshold 1e-8 ||b - mean b||, colour V(1,1), gridLevels 2):")
    for name, A0 in (("neumann_var((16,16,16))", neumann_var((16,) * 3)), ("Neumann Laplacian 16^3", neumann_laplacian((16,) * 3))):
        b = A0 @ np.random.default_rng(12345).random(A0.shape[0]) + 0.3
        thr = 1e-8 * float(np.linalg.norm(b - b.mean()))
        for extra in ({"accel": "cg"}, {"accel": "cg", "dtype": "mixed"}, {"cycle": "F", "overCorrection": 1.8}):
            p = dict({"problemShape": (16,) * 3, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "smoother": "colour", "minSize": 8,
                      "nullspace": "constant", "threshold": thr, "cycles": 200, "giveInfo": True}, **extra)
            u, info = openmg_amd.mgSolve(A0, b, p)
            say("  %-24s %-44s %3d %s, norm %.3e (threshold %.3e), |mean u| %.1e"
                % (name, extra, info["cycle"], "iterations" if "accel" in extra else "cycles", info["norm"], thr, abs(u.mean())))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    size = int(args[0]) if args else 128
    restrictions = int(args[1]) if len(args) > 1 else max(1, int(np.log2(size)) - 3)
    out = out or os.path.join(ROOT, "profiles", "nullspace_%d.txt" % size)
    torch.cuda.init()
    _hip.require_gpu()
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    probe(size, restrictions, say)
