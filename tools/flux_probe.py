#!/usr/bin/env python3
"""The face fluxes of a solution under a coefficient-field operator (csrc/kappa.hip kappa_flux_kernel and
face_divergence_kernel) at N^3, fp64, one process: cell widths (y stretched), mixed walls — x periodic, the y
walls Dirichlet with a scalar and a field of values, the floor a Neumann wall with a flux field, the lid a Neumann wall
without a value —, every array a device array.
  - the call (_hip.kappa_flux, device arrays in and out, storing and with alpha = -1 accumulating): hipEvents on a stream of
    the caller's around a call that ends in a synchronise — the entry runs on a stream of its own, so the figure holds its
    stream, its launch and its synchronise besides the kernel;
  - the same three face arrays formed with torch operations on the same device arrays (what a caller could do before:
    slices of kappa, u and the widths, the face expression per axis, the seam and wall faces written into their layers),
    first compared with the call to 1e-12, then timed with hipEvents, alternating with the call;
  - _hip.face_divergence, _hip.kappa_rhs (a source field and the same wall values) and the assembling launch
    (_hip.kappa_assemble, values alone) in the same process, the same way;
  - the kernels alone: from a rocprofv3 --kernel-trace CSV of `flux_probe.py N kernels` (a run of its own, which only makes
    the launches), given as the third argument; their needed bytes — 40 per cell storing (kappa and u read once, three faces
    written), 64 accumulating, 32 for the divergence — and with them TB/s and the share of the 8.0 TB/s HBM peak.
Writes profiles/flux_N.txt.   Usage: flux_probe.py [N] [kernels | measure] [kernel_trace.csv]"""
import csv
import os
import sys

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
REPEATS = 20
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fmt(v):
    return "min %.1f, median %.1f, max %.1f" % (min(v), float(np.median(v)), max(v))


rng = np.random.default_rng(1)
walls = ("neumann", "neumann", "dirichlet", "dirichlet", "periodic", "periodic")
edges = 0.5 * (1.0 + np.tanh(1.5 * np.linspace(-1.0, 1.0, size + 1)) / np.tanh(1.5))
spacing = (np.full(size + 2, 1.0 / size), np.concatenate(([0.0], np.diff(edges), [0.0])), np.full(size + 2, 1.0 / size))
kappa = torch.from_numpy(np.exp(rng.uniform(-1.0, 1.0, size=(size + 2,) * 3) * np.log(10.0))).cuda()
u = torch.from_numpy(rng.standard_normal(shape)).cuda()
values = [torch.from_numpy(rng.standard_normal((size, size))).cuda(), None, 1.0, torch.from_numpy(rng.standard_normal((size, size))).cuda(),
          None, None]
face_shapes = operators.face_shapes(shape)
out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in face_shapes]
acc = [torch.from_numpy(rng.standard_normal(s)).cuda() for s in face_shapes]
balance = torch.empty(n, dtype=torch.float64, device="cuda")
b = torch.empty(n, dtype=torch.float64, device="cuda")
args = _hip.KappaArgs(kappa, walls, spacing=spacing)
data = torch.empty(args.nnz, dtype=torch.float64, device="cuda")


def call():
    _hip.kappa_flux(kappa, u, walls, values, spacing=spacing, out=out)


def call_accumulate():
    _hip.kappa_flux(kappa, u, walls, values, spacing=spacing, out=acc, alpha=-1.0)


def call_divergence():
    _hip.face_divergence(out, out=balance)


def call_rhs():
    _hip.kappa_rhs(kappa, u, walls, values, spacing=spacing, out=b)          # (u as the source field: 16 bytes per cell)


def call_assemble():
    _hip.kappa_assemble(args, out=(None, None, data))


if kernels_only:
    for _ in range(REPEATS + 2):
        call()
        call_accumulate()
        call_divergence()
        call_rhs()
        call_assemble()
    sys.exit(0)

# ---- the same face arrays with torch operations ------------------------------------------------------------------------------
H = [torch.from_numpy(h).cuda() for h in spacing]
own = (H[0][1:-1, None, None], H[1][None, 1:-1, None], H[2][None, None, 1:-1])
area = (own[1] * own[2], own[0] * own[2], own[0] * own[1])
cells = kappa[1:-1, 1:-1, 1:-1]


def torch_fluxes():
    """operators.flux_kappa's steps with device arrays."""
    result = []
    for axis in range(3):
        e = shape[axis]
        F = torch.empty(face_shapes[axis], dtype=torch.float64, device="cuda")
        width = own[axis].expand(shape)
        face_area = area[axis].expand(shape)
        lo, hi = cells.narrow(axis, 0, e - 1), cells.narrow(axis, 1, e - 1)
        d_lo, d_hi = width.narrow(axis, 0, e - 1), width.narrow(axis, 1, e - 1)
        c = ((2.0 * lo) * hi) / (d_lo * hi + d_hi * lo) * face_area.narrow(axis, 0, e - 1)
        F.narrow(axis, 1, e - 1).copy_(c * (u.narrow(axis, 0, e - 1) - u.narrow(axis, 1, e - 1)))
        first, last = F.select(axis, 0), F.select(axis, e)
        if walls[2 * axis] == "periodic":
            a, g = cells.select(axis, e - 1), cells.select(axis, 0)
            c = ((2.0 * a) * g) / (width.select(axis, e - 1) * g + width.select(axis, 0) * a) * face_area.select(axis, e - 1)
            seam = c * (u.select(axis, e - 1) - u.select(axis, 0))
            first.copy_(seam)
            last.copy_(seam)
            result.append(F)
            continue
        for side, place, cell in ((0, first, 0), (1, last, e - 1)):
            w = 2 * axis + side
            if walls[w] == "neumann":
                if values[w] is None:
                    place.zero_()
                else:
                    t = values[w] * face_area.select(axis, cell)
                    place.copy_(-t if side else t)
                continue
            a, g = cells.select(axis, cell), kappa.select(axis, size + 1 if side else 0)[1:-1, 1:-1]      # the ghost cells behind
            c = ((2.0 * a) * g) / (width.select(axis, cell) * g + H[axis][-1 if side else 0] * a) * face_area.select(axis, cell)
            value = 0.0 if values[w] is None else values[w]
            place.copy_(c * (u.select(axis, cell) - value if side else value - u.select(axis, cell)))
        result.append(F)
    return result


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


say("flux_probe %d^3, fp64, cell widths (y stretched by a tanh map), x periodic, y Dirichlet (a scalar, a field), the floor a Neumann "
    "wall with a flux field, the lid one without a value, device arrays" % size)
want = torch_fluxes()
call()
torch.cuda.synchronize()
worst = max(float(torch.abs(a - w).max()) / float(torch.abs(w).max()) for a, w in zip(out, want))
say("the call and the torch operations agree to %.1e of max |F| per face array" % worst)
assert worst <= 1e-12
call_divergence()
torch.cuda.synchronize()
say("the balance of the call's faces and of the torch faces agree to %.1e of max |balance|"
    % (float(torch.abs(balance.reshape(shape) - ((want[0][1:] - want[0][:-1]) + (want[1][:, 1:] - want[1][:, :-1])
                                                 + (want[2][:, :, 1:] - want[2][:, :, :-1]))).max()) / float(torch.abs(balance).max())))
del want

us = {"fluxes, store": [], "fluxes, torch": [], "fluxes, alpha = -1": [], "face_divergence": [], "kappa_rhs": [], "kappa_assemble (values)": []}
fns = {"fluxes, store": call, "fluxes, torch": torch_fluxes, "fluxes, alpha = -1": call_accumulate, "face_divergence": call_divergence,
       "kappa_rhs": call_rhs, "kappa_assemble (values)": call_assemble}
for k in range(REPEATS + 2):
    for name in us:
        us[name].append(events(fns[name]))
for name in us:
    say("%-24s: %s us (hipEvents, %d repeats after 2 warm-ups, alternating)" % (name, fmt(us[name][2:]), REPEATS))
entry, other = us["fluxes, store"][2:], us["fluxes, torch"][2:]
say("the call's range %.1f - %.1f us lies %s the torch operations' range %.1f - %.1f us; at the medians the call is %.1f times as fast"
    % (min(entry), max(entry), "below" if max(entry) < min(other) else "NOT below", min(other), max(other), np.median(other) / np.median(entry)))

# ---- the kernels alone -------------------------------------------------------------------------------------------------------
# (name, needed bytes, what the kernel's name in the trace holds: demangled or mangled)
needed = {"kappa_flux_kernel<SPACED, PERIODIC>, store": (40 * n, ("kappa_flux_kernel<true, true, false>", "kappa_flux_kernelILb1ELb1ELb0E")),
          "kappa_flux_kernel<SPACED, PERIODIC, ACCUMULATE>": (64 * n, ("kappa_flux_kernel<true, true, true>", "kappa_flux_kernelILb1ELb1ELb1E")),
          "face_divergence_kernel": (32 * n, ("face_divergence_kernel",)),
          "kappa_rhs_kernel": (16 * n + 3 * 8 * size * size, ("kappa_rhs_kernel",)),
          "kappa_values_kernel": (8 * n + 8 * args.nnz, ("kappa_values_kernel",))}
if trace:
    rows = list(csv.DictReader(open(trace)))
    for name, (nbytes, keys) in needed.items():
        pick = [r for r in rows if any(key in r["Kernel_Name"] for key in keys)]
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in pick][2:]
        if not t:
            say("%s: not in the trace" % name)
            continue
        med = float(np.median(t))
        say("%s, rocprofv3 --kernel-trace (a run of its own, %d launches after 2 warm-ups): %s us" % (name, len(t), fmt(t)))
        say("   at the median: %.2f TB/s of its %.0f MB of needed bytes, %.1f %% of the %.1f TB/s HBM peak"
            % (nbytes / med * 1e-6, nbytes * 1e-6, 100.0 * nbytes / (med * 1e-6) / HBM_PEAK, HBM_PEAK * 1e-12))
else:
    say("the kernels alone: not measured (no kernel trace given)")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "flux_%d.txt" % size), "w") as fh:
    fh.write("\n".join(lines) + "\n")
