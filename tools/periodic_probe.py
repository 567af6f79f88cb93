#!/usr/bin/env python3
"""The 7-point operator of a coefficient field with periodic axes (csrc/kappa.hip PERIODIC) at N^3, fp64, 5
grids at 256^3, one field:
  - the assembling launch with x, y and z periodic beside the in-grid launch of the same process (omg_kappa_assemble, device
    arrays in, the value array out in HBM), alternating, best of several — once with the staged store path and once, in a
    child process (OMG_KAPPA_STAGE is read once per process), with the direct one.  The entry runs on a stream of its own
    that no caller's event can bracket, so the clock is the host's around a call that ends in a synchronise: the launch,
    the error word and the synchronise are in both figures alike;
  - setup (Solver.from_kappa), ms per cycle (resident V(1,1) cycles, hipEvents on the solver's stream) and Solver.update_kappa
    for the all-periodic operator — the ordinary route: the chain in HBM, the operators fetched, host orderings; update_kappa
    builds a new hierarchy — beside the Dirichlet operator of the same field, which takes the var7 passes and is updated in
    place.
Writes profiles/periodic_N.txt.   Usage: periodic_probe.py [N] [launch]"""
import os
import subprocess
import sys
import time

import numpy as np
import torch

torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openmg_amd  # noqa: E402
from openmg_amd import _hip  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
launch_only = len(sys.argv) > 2 and sys.argv[2] == "launch"
grids = {256: 5, 128: 4}.get(size, 3)
shape = (size,) * 3
n = size ** 3
PERIODIC = ("periodic",) * 6
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
staged = os.environ.get("OMG_KAPPA_STAGE", "1")[0] != "0"


def launches():
    values = {"periodic": torch.empty(7 * n, dtype=torch.float64, device="cuda"),
              "in-grid": torch.empty(7 * n - 6 * size * size, dtype=torch.float64, device="cuda")}
    ms = {"periodic": [], "in-grid": []}
    for k in range(14):
        ms["periodic"].append(wall(lambda: _hip.kappa_assemble(fields[k % 2], PERIODIC, out=(None, None, values["periodic"]))))
        ms["in-grid"].append(wall(lambda: _hip.kappa_assemble(fields[k % 2], out=(None, None, values["in-grid"]))))
    path = "staged in LDS" if staged else "direct"
    for name in ("periodic", "in-grid"):
        say("kappa_values, %-13s %-8s: %s ms per call (host clock: launch + error word + synchronise included; 12 calls, alternating)"
            % (path + ",", name, fmt(ms[name][2:])))
    say("      the periodic axes cost %+.3f ms at the minima, %+.3f ms at the medians (%s)"
        % (min(ms["periodic"][2:]) - min(ms["in-grid"][2:]), np.median(ms["periodic"][2:]) - np.median(ms["in-grid"][2:]), path))


if launch_only:
    launches()
    sys.exit(0)

say("periodic_probe %d^3, %d grids, fp64, colour, kappa = exp(U(-1, 1) ln 10), x, y and z periodic beside all-Dirichlet walls" % (size, grids))
launches()
# the direct store path: a fresh process, its lines taken over
child = subprocess.run([sys.executable, os.path.abspath(__file__), str(size), "launch"], env=dict(os.environ, OMG_KAPPA_STAGE="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
if child.returncode != 0:
    raise SystemExit("the child process failed:\n" + child.stderr[-2000:])
for text in child.stdout.splitlines():
    say(text)

# ---- setup, cycles, a time step ---------------------------------------------------------------------------------------------
p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "cycles": 10,
     "threshold": 0.0}
stream = torch.cuda.Stream()
b = np.random.default_rng(2).standard_normal(n)
b -= b.mean()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


say("")
for name, walls, more in (("periodic", PERIODIC, {"nullspace": "constant"}), ("dirichlet", None, {})):
    setup = []
    for k in range(3):
        t = time.perf_counter()
        s = openmg_amd.Solver.from_kappa(fields[0], dict(p, **more), walls)
        _hip.check(_hip.lib().omg_device_synchronize())
        setup.append(1e3 * (time.perf_counter() - t))
        if k < 2:
            s.close()
    with s:
        h = s.hierarchy
        kinds = ["var7" if h.level_flags(l)["var7"] else "plane" if h.level_flags(l)["plane"] else "rows" for l in range(h.n_levels - 1)]
        say("%-9s levels: %s; can_update_fine %s" % (name + ":", kinds, h.can_update_fine()))
        say("%-9s setup, Solver.from_kappa: host clock %s ms (3 setups)" % (name + ":", fmt(setup)))
        h.set_stream(stream.cuda_stream)
        h.resident_load(b, None)
        for _ in range(3):
            h.resident_cycle(1, 1, want_norm=False)
        per_cycle = [events(lambda: [h.resident_cycle(1, 1, want_norm=False) for _ in range(10)]) / 10.0 for _ in range(5)]
        say("%-9s V(1,1) cycle: hipEvents %s ms per cycle (5 x 10 cycles)" % (name + ":", fmt(per_cycle)))
        s.update_kappa(fields[1])                                          # warm-up
        step = []
        for k in range(4):
            t = time.perf_counter()
            s.update_kappa(fields[k % 2])
            _hip.check(_hip.lib().omg_device_synchronize())
            step.append(1e3 * (time.perf_counter() - t))
        say("%-9s step, Solver.update_kappa: host clock %s ms (4 updates; %s)"
            % (name + ":", fmt(step), "in place" if s.hierarchy.can_update_fine() else "a new hierarchy"))

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "periodic_%d.txt" % size), "w") as f:
    f.write("\n".join(lines) + "\n")
