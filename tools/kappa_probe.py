#!/usr/bin/env python3
"""The 7-point operator from a coefficient field in HBM (csrc/kappa.hip) at N^3, fp64, one process:
  - kappa_values alone (omg_kappa_assemble, device arrays in, the value array out in HBM): ms per call — a host clock
    around a call that ends in a synchronise, so the launch, the error word and the synchronise are in it —, the bytes
    the kernel needs (kappa once, the values once, sigma if a field) and their fraction of the 8 TB/s peak;
  - a time step: Solver.update_kappa(kappa on the device) beside Hierarchy.update_fine(values on the device) on the same
    hierarchy and stream (hipEvents, alternating), and beside the route without the feature: kappa to the host, SciPy
    assembly (operators.stencil7_kappa), Solver.update(A) — each part; then the FCG solve that follows;
  - Solver.from_kappa(kappa on the device) beside Solver(A) with the host assembly in front.
Kernel times proper (kappa_values_kernel beside var7_rap's level-0 pass) come from a rocprofv3 --kernel-trace --stats run
of `kappa_probe.py N kernels`, which only runs five update_kappa calls.  Writes profiles/kappa_N.txt.
Usage: kappa_probe.py [N] [kernels]"""
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openmg_amd  # noqa: E402
from openmg_amd import _hip, operators  # noqa: E402

PEAK = 8e12
size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kernels_only = len(sys.argv) > 2 and sys.argv[2] == "kernels"
grids = {256: 5, 128: 4}.get(size, 3)
shape = (size,) * 3
n = size ** 3
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def kappa_of(seed):
    return np.exp(np.random.default_rng(seed).uniform(-1.0, 1.0, size=(size + 2,) * 3) * np.log(10.0))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    _hip.check(_hip.lib().omg_device_synchronize())
    return 1e3 * (time.perf_counter() - t), out


def fmt(v):
    return "median %.3f, min %.3f, max %.3f" % (float(np.median(v)), min(v), max(v))


fields = [kappa_of(1), kappa_of(2)]
dev = [torch.from_numpy(k).cuda() for k in fields]
sigma = torch.full(shape, 0.125, dtype=torch.float64, device="cuda")
p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg",
     "cycles": 200, "threshold": 0.0, "rtol": 1e-8}
b = np.random.default_rng(7).standard_normal(n)
bd = torch.from_numpy(b).cuda()
say("kappa_probe %d^3, %d grids, fp64, colour, kappa = exp(U(-1, 1) ln 10), store path: %s"
    % (size, grids, "direct" if os.environ.get("OMG_KAPPA_STAGE", "1")[0] == "0" else "staged in LDS"))

if kernels_only:
    with openmg_amd.Solver.from_kappa(dev[0], p) as s:
        for k in range(5):
            s.update_kappa(dev[(k + 1) % 2])
    sys.exit(0)

# ---- kappa_values alone -----------------------------------------------------------------------------------------------
nnz = 7 * n - 6 * size * size
values = torch.empty(nnz, dtype=torch.float64, device="cuda")
for name, sg, extra in (("no sigma", None, 0), ("sigma field", sigma, n)):
    ms = [wall(lambda: _hip.kappa_assemble(dev[k % 2], sigma=sg, out=(None, None, values)))[0] for k in range(12)][2:]
    need = 8 * ((size + 2) ** 3 + nnz + extra)
    say("kappa_values, %s: %s ms per call (host clock, launch + error word + synchronise included); %.3f GB needed: "
        "%.2f TB/s = %.2f of 8 TB/s at the median" % (name, fmt(ms), need / 1e9, need / (np.median(ms) * 1e-3) / 1e12,
                                                     need / (np.median(ms) * 1e-3) / PEAK))

# ---- Solver.from_kappa beside Solver(A) ---------------------------------------------------------------------------------
t = time.perf_counter()
A = [operators.stencil7_kappa(fields[0])]
ms_assemble = 1e3 * (time.perf_counter() - t)
openmg_amd.Solver.from_kappa(dev[0], p).close()                      # warm-up: code objects, the first allocations
ms_new, ms_old = [], []
for k in range(3):                                                   # alternating
    ms, s = wall(lambda: openmg_amd.Solver.from_kappa(dev[0], p))
    ms_new.append(ms)
    s.close()
    ms, s = wall(lambda: openmg_amd.Solver(A[0], p))
    ms_old.append(ms)
    s.close()
s = openmg_amd.Solver.from_kappa(dev[0], p)
say("setup: Solver.from_kappa(kappa in HBM) %s ms; Solver(A) %s ms after %.1f ms of SciPy assembly (%.0f MB of CSR)"
    % (fmt(ms_new), fmt(ms_old), ms_assemble, (A[0].data.nbytes + A[0].indices.nbytes + A[0].indptr.nbytes) / 1e6))
h = s.hierarchy
say("levels: %s; can_update_fine %s" % (["var7" if h.level_flags(l)["var7"] else "plane" if h.level_flags(l)["plane"] else "host"
                                          for l in range(grids - 1)], h.can_update_fine()))

# ---- a time step ----------------------------------------------------------------------------------------------------------
stream = torch.cuda.Stream()
h.set_stream(stream.cuda_stream)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)


vals = []
for k in range(2):
    v = torch.empty(nnz, dtype=torch.float64, device="cuda")
    _hip.kappa_assemble(dev[k], out=(None, None, v))
    vals.append(v)
s.update_kappa(dev[1])                                               # warm-up: the value array, the products' arrays
ev_k, ev_f, wl_k, wl_f = [], [], [], []
for k in range(6):
    e, w = events(lambda: s.update_kappa(dev[k % 2]))
    ev_k.append(e)
    wl_k.append(w)
    e, w = events(lambda: h.update_fine((vals[k % 2].data_ptr(), nnz), on_device=True))
    ev_f.append(e)
    wl_f.append(w)
say("step, Solver.update_kappa(kappa in HBM):      hipEvents %s ms; host clock %s ms" % (fmt(ev_k), fmt(wl_k)))
say("step, update_fine(the same values in HBM):   hipEvents %s ms; host clock %s ms" % (fmt(ev_f), fmt(wl_f)))
say("      the price of assembling: %.3f ms at the medians, %.3f ms at the minima (update_fine alone spreads over %.1f ms)"
    % (np.median(ev_k) - np.median(ev_f), min(ev_k) - min(ev_f), max(ev_f) - min(ev_f)))
ms_solve, (u, info) = wall(lambda: s.solve(bd))
say("      the FCG solve that follows: %.1f ms, %d iterations to 1e-8" % (ms_solve, info["cycle"]))
# the route without the feature, on the same solver (update(A) forms the host pattern on its first call: once, not timed)
s.update(A[0])
for k in (1, 0):
    ms_copy, host = wall(lambda: dev[k].cpu().numpy())
    t = time.perf_counter()
    A[0] = None
    A[0] = operators.stencil7_kappa(host)
    ms_asm = 1e3 * (time.perf_counter() - t)
    ms_upd, _ = wall(lambda: s.update(A[0]))
    say("step, without the feature: kappa to the host %.1f ms + SciPy assembly %.1f ms + Solver.update(A) %.1f ms = %.1f ms"
        % (ms_copy, ms_asm, ms_upd, ms_copy + ms_asm + ms_upd))
s.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
name = "kappa_%d%s.txt" % (size, "_direct" if os.environ.get("OMG_KAPPA_STAGE", "1")[0] == "0" else "")
with open(os.path.join(ROOT, "profiles", name), "w") as f:
    f.write("\n".join(lines) + "\n")
