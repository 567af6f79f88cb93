#!/usr/bin/env python3
"""The right-hand side of a coefficient-field operator (csrc/kappa.hip kappa_rhs_kernel) at N^3, fp64, one
process: all walls carry a value (Dirichlet fields on the y and x walls, flux fields on the z walls), f is a field, the
grid is stretched (the SPACED kernel), every array a device array, b written in place of a separate output.
  - the call (_hip.kappa_rhs, device arrays in and out): hipEvents on a stream of the caller's around a call that ends in a
    synchronise, and the host clock around the same — the entry runs on a stream of its own, so both hold its stream, its
    launch and its synchronise besides the kernel;
  - the kernel alone: from a rocprofv3 --kernel-trace CSV of `kappa_rhs_probe.py N kernels` (a run of its own, which only
    makes the launches), given as the third argument; its needed bytes — 16 per cell, plus per cell at a wall with a value
    8 for the value and, at a Dirichlet wall, 16 for the two kappa — and with them the share of the 8.0 TB/s HBM peak;
  - the same b formed with torch operations on the same device arrays (what a caller could do before: slices of kappa and
    of the widths, the face expression, six in-place additions into the wall layers), hipEvents, alternating with the call.
Writes profiles/kappa_rhs_N.txt.   Usage: kappa_rhs_probe.py [N] [kernels | measure] [kernel_trace.csv]"""
import csv
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmg_amd import _hip, operators  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kernels_only = len(sys.argv) > 2 and sys.argv[2] == "kernels"
trace = sys.argv[3] if len(sys.argv) > 3 else None
shape = (size,) * 3
n = size ** 3
HBM_PEAK = 8.0e12
REPEATS = 30
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fmt(v):
    return "min %.1f, median %.1f, max %.1f" % (min(v), float(np.median(v)), max(v))


rng = np.random.default_rng(1)
walls = ("neumann", "neumann", "dirichlet", "dirichlet", "dirichlet", "dirichlet")
faces = 0.5 * (1.0 + np.tanh(1.5 * np.linspace(-1.0, 1.0, size + 1)) / np.tanh(1.5))
spacing = (np.full(size + 2, 1.0 / size), np.concatenate(([0.0], np.diff(faces), [0.0])), np.full(size + 2, 1.0 / size))
kappa = torch.from_numpy(np.exp(rng.uniform(-1.0, 1.0, size=(size + 2,) * 3) * np.log(10.0))).cuda()
f = torch.from_numpy(rng.standard_normal(shape)).cuda()
values = [torch.from_numpy(rng.standard_normal((size, size))).cuda() for _ in range(6)]
out = torch.empty(n, dtype=torch.float64, device="cuda")


def call():
    _hip.kappa_rhs(kappa, f, walls, values, spacing=spacing, out=out)


if kernels_only:
    for _ in range(REPEATS + 2):
        call()
    sys.exit(0)

# ---- the same b with torch operations ---------------------------------------------------------------------------------------
H = [torch.from_numpy(h).cuda() for h in spacing]
own = (H[0][1:-1, None, None], H[1][None, 1:-1, None], H[2][None, None, 1:-1])
area = (own[1] * own[2], own[0] * own[2], own[0] * own[1])
volume = (own[0] * own[1]) * own[2]
cells = kappa[1:-1, 1:-1, 1:-1]


def torch_rhs():
    """operators.rhs_kappa's steps with device arrays.  The additions go into the wall layers only, so the order of a
    corner cell's sum is not the definition's: equal to rounding, not bit for bit."""
    b = f * volume
    for w in range(6):
        axis, hi = w // 2, w % 2
        layer = [slice(None)] * 3
        layer[axis] = -1 if hi else 0
        layer = tuple(layer)
        behind = tuple(slice(1, -1) if isinstance(s, slice) else s for s in layer)
        face_area = area[axis].expand(shape)[layer]
        if walls[w] == "neumann":
            b[layer] += values[w] * face_area
            continue
        a, g = cells[layer], kappa[behind]
        da, db = own[axis].expand(shape)[layer], H[axis][-1 if hi else 0]
        b[layer] += ((2.0 * a) * g) / (da * g + db * a) * face_area * values[w]
    return b


stream = torch.cuda.Stream()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        e0.record(stream)
        fn()
        e1.record(stream)
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def host(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t)


say("kappa_rhs_probe %d^3, fp64, cell widths (y stretched by a tanh map), f a field, all six walls with a field of values "
    "(z Neumann, y and x Dirichlet), device arrays" % size)
want = torch_rhs().reshape(-1)
call()
scale_of = float(torch.abs(want).max())
say("the two agree to %.1e of max |b| (the torch form sums a corner cell's terms in another order)" % (float(torch.abs(out - want).max()) / scale_of))
assert float(torch.abs(out - want).max()) <= 1e-13 * scale_of

us = {"call, hipEvents": [], "call, host clock": [], "torch, hipEvents": [], "torch, host clock": []}
for k in range(REPEATS + 2):
    us["call, hipEvents"].append(events(call))
    us["torch, hipEvents"].append(events(torch_rhs))
    us["call, host clock"].append(host(call))
    us["torch, host clock"].append(host(torch_rhs))
for name in us:
    say("%-18s: %s us (%d repeats after 2 warm-ups, alternating)" % (name, fmt(us[name][2:]), REPEATS))
say("the call is %.1f times as fast as the torch operations at the medians of the hipEvents figures"
    % (np.median(us["torch, hipEvents"][2:]) / np.median(us["call, hipEvents"][2:])))

# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
wall_cells = size * size
needed = 16 * n + 2 * wall_cells * 8 + 4 * wall_cells * (8 + 16)
say("needed bytes: %d = 16 per cell (f read, b written) + %d for the values, the ghost and the own kappa of the wall cells (%.2f %% of the whole)"
    % (needed, needed - 16 * n, 100.0 * (needed - 16 * n) / needed))
if trace:
    rows = [r for r in csv.DictReader(open(trace)) if "kappa_rhs_kernel" in r["Kernel_Name"]]
    t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows][2:]
    say("kappa_rhs_kernel<SPACED>, rocprofv3 --kernel-trace (a run of its own, %d launches after 2 warm-ups): %s us" % (len(t), fmt(t)))
    med = float(np.median(t))
    say("   at the median: %.2f TB/s of needed bytes, %.1f %% of the %.1f TB/s HBM peak (bound by the stream: 16 bytes and one sum per cell)"
        % (needed / med * 1e-6, 100.0 * needed / (med * 1e-6) / HBM_PEAK, HBM_PEAK * 1e-12))
else:
    say("kappa_rhs_kernel alone: not measured (no kernel trace given)")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "kappa_rhs_%d.txt" % size), "w") as fh:
    fh.write("\n".join(lines) + "\n")
