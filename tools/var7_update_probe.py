#!/usr/bin/env python3
"""omg_hierarchy_update_fine on the var7 bench leg's hierarchy (stencil7_variable, 256^3, 5 grids, default thresholds):
wall time of a fresh from_fine of the new operator, of an update from values in HBM, of one from host values, and of an
update + one cycle, fp64 and fp32, all in one process (a synchronise before every clock read).  With OMG_SETUP_TIMING=1
the library prints the phases.  Usage: var7_update_probe.py [size] [grids] [dtypes, comma-separated]"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmg_amd import _hip, operators  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
grids = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dtypes = sys.argv[3].split(",") if len(sys.argv) > 3 else ["float64", "float32"]
reps = 3
shape = (size,) * 3
t = time.perf_counter()
A = operators.stencil7_variable(shape, seed=1)
A2 = operators.stencil7_variable(shape, seed=2)
print("operators: %.1f s" % (time.perf_counter() - t), flush=True)
b = A @ np.random.default_rng(12345).random(A.shape[0])
hip = ctypes.CDLL("libamdhip64.so.7")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipFree.argtypes = [ctypes.c_void_p]
dev = []
for M in (A, A2):
    d = ctypes.c_void_p()
    data = np.ascontiguousarray(M.data)
    assert hip.hipMalloc(ctypes.byref(d), data.nbytes) == 0 and hip.hipMemcpy(d, data.ctypes.data, data.nbytes, 1) == 0
    dev.append((d, data.size))


def ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


for dtype in dtypes:
    print("== %d^3, %d grids, %s" % (size, grids, dtype), flush=True)
    fresh = []
    for k in range(reps):
        def make():
            global h
            h = _hip.Hierarchy.from_fine(A2 if k % 2 == 0 else A, shape, grids - 1, "colour", dtype=dtype)
            h.sync()
        if k:
            h.close()
        fresh.append(ms(make))
    print("levels:", ["var7" if h.level_flags(l)["var7"] else "host" for l in range(grids - 1)])
    h.resident_load(b)
    h.resident_cycle(1, 1)
    dv, hv, cyc = [], [], []
    for k in range(reps):
        which = dev[k % 2]

        def upd_dev():
            h.update_fine((which[0].value, which[1]), on_device=True)
            h.sync()
        dv.append(ms(upd_dev))

        def upd_host():
            h.update_fine((A, A2)[k % 2].data)
            h.sync()
        hv.append(ms(upd_host))

        def upd_cycle():
            h.update_fine((which[0].value, which[1]), on_device=True)
            h.resident_cycle(1, 1)
        cyc.append(ms(upd_cycle))
    h.close()
    fmt = lambda v: " ".join("%.1f" % x for x in v)  # noqa: E731
    print("fresh from_fine ms:        ", fmt(fresh))
    print("update, values in HBM ms:  ", fmt(dv))
    print("update, values on host ms: ", fmt(hv))
    print("update + one V(1,1) ms:    ", fmt(cyc), flush=True)
for d, _ in dev:
    hip.hipFree(d)
