#!/usr/bin/env python3
"""The 7-point operator from one coefficient per face in HBM (csrc/kappa.hip faces_*_kernel) beside its
kappa twin at N^3, fp64, one process, every array a device array; tools/kappa_probe.py's and tools/flux_probe.py's methods:
  (a) the assembling call, values alone (_hip.faces_assemble beside _hip.kappa_assemble, out in HBM): a HOST CLOCK around a
      call that ends in a synchronise — the launch, the error word's copy and the synchronise are in it —, 12 calls of each,
      alternating, the first 2 dropped; the bytes each kernel needs (faces: three coefficients per row once each, 24 B, and
      7 values, 56 B; kappa: 8 B and 56 B) and with them TB/s;
  (b) a time step: Solver.update_faces beside Solver.update_kappa on two solvers of the same hierarchy shape, hipEvents on
      the hierarchies' stream, alternating; and the route update_faces replaces: the arrays to the host, SciPy assembly
      (operators.stencil7_faces), Solver.update(A) — a host clock, each part, once;
  (c) Solver.fluxes on the from_faces solver beside Solver.fluxes on the from_kappa solver and beside the same three arrays
      formed with torch operations (compared to 1e-12 first), storing and with alpha = -1: hipEvents on a stream of the
      caller's around calls that end in a synchronise, alternating; needed bytes faces 56 B per cell storing (three
      coefficients and u read, three faces written), 80 B accumulating; kappa 40 B and 64 B.
No counters and no kernel trace are taken here: every figure holds the entry's own overhead besides the kernel.
Writes profiles/faces_N.txt.   Usage: faces_probe.py [N]"""
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

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
grids = {256: 5, 128: 4}.get(size, 3)
shape = (size,) * 3
n = size ** 3
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fmt(v):
    return "median %.3f, min %.3f, max %.3f" % (float(np.median(v)), min(v), max(v))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    _hip.check(_hip.lib().omg_device_synchronize())
    return 1e3 * (time.perf_counter() - t), out


walls = ("neumann", "neumann", "dirichlet", "dirichlet", "periodic", "periodic")
plain = ("neumann", "neumann", "dirichlet", "dirichlet", "dirichlet", "dirichlet")      # (in place: no periodic wall)
face_shapes = operators.face_shapes(shape)
rng = np.random.default_rng(1)
kappas = [torch.from_numpy(np.exp(rng.uniform(-1.0, 1.0, size=(size + 2,) * 3) * np.log(10.0))).cuda() for _ in range(2)]
coeffs = [[torch.from_numpy(np.exp(rng.uniform(-1.0, 1.0, size=s) * np.log(10.0))).cuda() for s in face_shapes] for _ in range(2)]
u = torch.from_numpy(rng.standard_normal(shape)).cuda()
say("faces_probe %d^3, %d grids, fp64, colour; coefficients exp(U(-1, 1) ln 10) per face (per cell for the kappa twin), device arrays" % (size, grids))

# ---- (a) the assembling call ---------------------------------------------------------------------------------------------
nnz = 7 * n - 6 * size * size
values = torch.empty(nnz, dtype=torch.float64, device="cuda")
ms_f, ms_k = [], []
for k in range(12):
    ms_f.append(wall(lambda: _hip.faces_assemble(coeffs[k % 2], out=(None, None, values)))[0])
    ms_k.append(wall(lambda: _hip.kappa_assemble(kappas[k % 2], out=(None, None, values)))[0])
ms_f, ms_k = ms_f[2:], ms_k[2:]
need_f, need_k = 8 * (sum(int(np.prod(s)) for s in face_shapes) + nnz), 8 * ((size + 2) ** 3 + nnz)
for name, ms, need in (("faces_assemble", ms_f, need_f), ("kappa_assemble", ms_k, need_k)):
    say("(a) %s, values alone: %s ms per call (host clock; launch + error word + synchronise included); %.3f GB needed: %.2f TB/s at the median"
        % (name, fmt(ms), need / 1e9, need / (np.median(ms) * 1e-3) / 1e12))
say("(a) faces / kappa at the medians: %.2f in time, %.2f in needed bytes" % (np.median(ms_f) / np.median(ms_k), need_f / need_k))

# ---- (b) a time step -----------------------------------------------------------------------------------------------------
p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg",
     "cycles": 200, "threshold": 0.0, "rtol": 1e-8}
sf = openmg_amd.Solver.from_faces(coeffs[0], p, plain)
sk = openmg_amd.Solver.from_kappa(kappas[0], p, plain)
for name, s in (("from_faces", sf), ("from_kappa", sk)):
    h = s.hierarchy
    say("(b) %s levels: %s; can_update_fine %s" % (name, ["var7" if h.level_flags(l)["var7"] else "plane" if h.level_flags(l)["plane"] else "host"
                                                         for l in range(grids - 1)], h.can_update_fine()))
stream = torch.cuda.Stream()
sf.hierarchy.set_stream(stream.cuda_stream)
sk.hierarchy.set_stream(stream.cuda_stream)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        e0.record(stream)
        fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


sf.update_faces(coeffs[1])                                           # warm-up: the value array, the products' arrays
sk.update_kappa(kappas[1])
ev_f, ev_k = [], []
for k in range(6):
    ev_f.append(events(lambda: sf.update_faces(coeffs[k % 2])))
    ev_k.append(events(lambda: sk.update_kappa(kappas[k % 2])))
say("(b) Solver.update_faces(arrays in HBM): hipEvents %s ms" % fmt(ev_f))
say("(b) Solver.update_kappa(kappa in HBM):  hipEvents %s ms" % fmt(ev_k))
sk.close()
ms_copy, host = wall(lambda: [c.cpu().numpy() for c in coeffs[1]])
t = time.perf_counter()
A = operators.stencil7_faces(host, plain)
ms_asm = 1e3 * (time.perf_counter() - t)
sf.update(A)                                                         # (forms the host pattern on its first call: once, not timed)
ms_upd, _ = wall(lambda: sf.update(A))
say("(b) the route it replaces: arrays to the host %.1f ms + SciPy assembly %.1f ms + Solver.update(A) %.1f ms = %.1f ms"
    % (ms_copy, ms_asm, ms_upd, ms_copy + ms_asm + ms_upd))
del A, host
sf.close()

# ---- (c) fluxes ----------------------------------------------------------------------------------------------------------
values_w = [torch.from_numpy(rng.standard_normal((size, size))).cuda(), None, 1.0, torch.from_numpy(rng.standard_normal((size, size))).cuda(),
            None, None]
out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in face_shapes]
acc = [torch.from_numpy(rng.standard_normal(s)).cuda() for s in face_shapes]
C = coeffs[0]


def torch_fluxes():
    """operators.flux_faces' steps with device arrays."""
    result = []
    for axis in range(3):
        e = shape[axis]
        F = torch.empty(face_shapes[axis], dtype=torch.float64, device="cuda")
        F.narrow(axis, 1, e - 1).copy_(C[axis].narrow(axis, 1, e - 1) * (u.narrow(axis, 0, e - 1) - u.narrow(axis, 1, e - 1)))
        first, last = F.select(axis, 0), F.select(axis, e)
        if walls[2 * axis] == "periodic":
            seam = C[axis].select(axis, 0) * (u.select(axis, e - 1) - u.select(axis, 0))
            first.copy_(seam)
            last.copy_(seam)
            result.append(F)
            continue
        for side, place, cell in ((0, first, 0), (1, last, e - 1)):
            w = 2 * axis + side
            if walls[w] == "neumann":
                if values_w[w] is None:
                    place.zero_()
                else:
                    place.copy_(-values_w[w] if side else values_w[w])
                continue
            value = 0.0 if values_w[w] is None else values_w[w]
            place.copy_(C[axis].select(axis, e if side else 0) * (u.select(axis, cell) - value if side else value - u.select(axis, cell)))
        result.append(F)
    return result


def call_faces():
    _hip.faces_flux(C, u, walls, values_w, out=out)


def call_faces_acc():
    _hip.faces_flux(C, u, walls, values_w, out=acc, alpha=-1.0)


def call_kappa():
    _hip.kappa_flux(kappas[0], u, walls, values_w, out=out)


def call_kappa_acc():
    _hip.kappa_flux(kappas[0], u, walls, values_w, out=acc, alpha=-1.0)


want = torch_fluxes()
call_faces()
torch.cuda.synchronize()
worst = max(float(torch.abs(a - w).max()) / float(torch.abs(w).max()) for a, w in zip(out, want))
say("(c) the call and the torch operations agree to %.1e of max |F| per face array" % worst)
assert worst <= 1e-12
del want
fns = {"faces_flux, store": (call_faces, 56 * n), "faces_flux, alpha = -1": (call_faces_acc, 80 * n), "kappa_flux, store": (call_kappa, 40 * n),
       "kappa_flux, alpha = -1": (call_kappa_acc, 64 * n), "torch operations, store": (torch_fluxes, None)}
us = {name: [] for name in fns}
for k in range(14):
    for name in fns:
        us[name].append(1e3 * events(fns[name][0]))
for name in fns:
    t = us[name][2:]
    need = fns[name][1]
    say("(c) %-24s: median %.1f, min %.1f, max %.1f us (hipEvents around the call, 12 repeats after 2 warm-ups, alternating)%s"
        % (name, float(np.median(t)), min(t), max(t),
           "" if need is None else "; %.0f MB needed: %.2f TB/s at the median" % (need * 1e-6, need / (np.median(t) * 1e-6) / 1e12)))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "faces_%d.txt" % size), "w") as fh:
    fh.write("\n".join(lines) + "\n")
