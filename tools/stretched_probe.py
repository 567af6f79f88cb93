#!/usr/bin/env python3
"""The 7-point operator of a coefficient field on a stretched grid (csrc/kappa.hip SPACED) at N^3, fp64, one
process:
  - the assembling launch with and without cell widths (omg_kappa_assemble_spaced, device arrays in, the value array out
    in HBM), alternating, best of several.  The entry runs on a stream of its own that no caller's event can bracket, so
    the clock is the host's around a call that ends in a synchronise: the launch, the error word and the synchronise are
    in both figures alike.  The kernels' own durations come from a rocprofv3 --kernel-trace --stats run of
    `stretched_probe.py N kernels`, which only makes six launches of each;
  - a time step: Solver.update_kappa on a solver made with widths beside one made without, the same field, hipEvents on
    the solvers' stream, alternating;
  - examples/boundary_layer_solve.py's cycle counts at 128^3.
Writes profiles/stretched_N.txt.   Usage: stretched_probe.py [N] [kernels]"""
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import openmg_amd  # noqa: E402
from openmg_amd import _hip  # noqa: E402
import boundary_layer_solve as example  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kernels_only = len(sys.argv) > 2 and sys.argv[2] == "kernels"
grids = {256: 5, 128: 4}.get(size, 3)
shape = (size,) * 3
n = size ** 3
nnz = 7 * n - 6 * size * size
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fmt(v):
    return "min %.3f, median %.3f, max %.3f" % (min(v), float(np.median(v)), max(v))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    _hip.check(_hip.lib().omg_device_synchronize())
    return 1e3 * (time.perf_counter() - t)


rng = np.random.default_rng(1)
fields = [torch.from_numpy(np.exp(rng.uniform(-1.0, 1.0, size=(size + 2,) * 3) * np.log(10.0))).cuda() for _ in range(2)]
spacing, _ = example.grid(size, 2.0)
spacing = tuple(np.where(h > 0.0, h * size, h) for h in spacing)          # (widths of order one, as the scale factors are)
values = torch.empty(nnz, dtype=torch.float64, device="cuda")
say("stretched_probe %d^3, %d grids, fp64, colour, kappa = exp(U(-1, 1) ln 10), z clustered by the tanh map (beta 2), store path: %s"
    % (size, grids, "direct" if os.environ.get("OMG_KAPPA_STAGE", "1")[0] == "0" else "staged in LDS"))

if kernels_only:
    for k in range(6):
        _hip.kappa_assemble(fields[k % 2], out=(None, None, values), spacing=spacing)
        _hip.kappa_assemble(fields[k % 2], out=(None, None, values))
    sys.exit(0)

# ---- the assembling launch ----------------------------------------------------------------------------------------------
ms = {"spaced": [], "unspaced": []}
for k in range(14):
    ms["spaced"].append(wall(lambda: _hip.kappa_assemble(fields[k % 2], out=(None, None, values), spacing=spacing)))
    ms["unspaced"].append(wall(lambda: _hip.kappa_assemble(fields[k % 2], out=(None, None, values))))
for name in ("spaced", "unspaced"):
    say("kappa_values, %-8s: %s ms per call (host clock: launch + error word + synchronise included; 12 calls, alternating)"
        % (name, fmt(ms[name][2:])))
say("      the widths cost %+.3f ms at the minima, %+.3f ms at the medians"
    % (min(ms["spaced"][2:]) - min(ms["unspaced"][2:]), np.median(ms["spaced"][2:]) - np.median(ms["unspaced"][2:])))

# ---- a time step ----------------------------------------------------------------------------------------------------------
p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "accel": "cg",
     "cycles": 200, "threshold": 0.0, "rtol": 1e-8}
stream = torch.cuda.Stream()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


with openmg_amd.Solver.from_kappa(fields[0], p, spacing=spacing) as s_w, openmg_amd.Solver.from_kappa(fields[0], p) as s_u:
    for s in (s_w, s_u):
        s.hierarchy.set_stream(stream.cuda_stream)
        s.update_kappa(fields[1])                                          # warm-up: the value array, the products' arrays
    say("levels: %s; can_update_fine %s" % (["var7" if s_w.hierarchy.level_flags(l)["var7"] else "host" for l in range(grids - 1)],
                                            s_w.hierarchy.can_update_fine()))
    ev_w, ev_u = [], []
    for k in range(6):
        ev_w.append(events(lambda: s_w.update_kappa(fields[k % 2])))
        ev_u.append(events(lambda: s_u.update_kappa(fields[k % 2])))
    say("step, Solver.update_kappa with widths:    hipEvents %s ms" % fmt(ev_w))
    say("step, Solver.update_kappa without widths: hipEvents %s ms" % fmt(ev_u))

# ---- the example ------------------------------------------------------------------------------------------------------------
say("")
say("examples/boundary_layer_solve.py 128 4 2.0:")
example.run(128, 4, 2.0, say=say)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "stretched_%d.txt" % size), "w") as f:
    f.write("\n".join(lines) + "\n")
