#!/usr/bin/env python3
"""What does a flexible-CG iteration (omg_resident_pcg, csrc/pcg.hip) cost at 256^3 fp64, and what does it buy?
    python tools/pcg_probe.py [size]
Per operator (stencil_poisson and stencil7_variable, colour V(1,1), 5 grids, set up on the device):
  - ms per PCG iteration (32 iterations, threshold 0, bracketed by hipEvents on the hierarchy's stream), the V-cycle's
    share (32 resident V-cycles bracketed the same way) and the CG kernels' (the difference);
  - the CG kernels' bytes (13 vectors of n values per iteration) / their time, as a fraction of 8 TB/s;
  - iterations and wall time to relative residual 1e-8 next to plain V-cycles (resident cycles in batches of 8)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from openmg_amd import _hip, operators

PEAK = 8e12
K = 32


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def probe(name, A0, shape, grids=5):
    n = A0.shape[0]
    b = np.random.default_rng(7).standard_normal(n)
    tol = 1e-8 * np.linalg.norm(b)
    stream = torch.cuda.Stream()
    with _hip.Hierarchy.from_fine(A0, shape, grids - 1, smoother="colour") as h:
        h.set_stream(stream.cuda_stream)
        flags = h.level_flags(0)
        h.resident_load(b)
        h.resident_pcg(1, 1, 4)                                   # warm-up (buffers, formats)
        h.resident_cycles(1, 1, 4)
        h.resident_load(b)
        ms_pcg = timed(stream, lambda: h.resident_pcg(1, 1, K)) / K
        h.resident_load(b)
        ms_cyc = timed(stream, lambda: h.resident_cycles(1, 1, K)) / K
        ms_cg = ms_pcg - ms_cyc
        gb = 13 * n * 8
        # time to 1e-8: PCG
        h.resident_load(b)
        torch.cuda.synchronize()
        t = time.perf_counter()
        its, norms, tn, bd = h.resident_pcg(1, 1, 1000, tol)
        t_pcg = time.perf_counter() - t
        # plain cycles, 8 per device call
        h.resident_load(b)
        torch.cuda.synchronize()
        t = time.perf_counter()
        cycles, nv = 0, np.inf
        while nv >= tol and cycles < 2000:
            got = h.resident_cycles(1, 1, 8)
            below = [k for k, v in enumerate(got) if v < tol]
            cycles += below[0] + 1 if below else 8
            nv = got[below[0]] if below else got[-1]
        t_plain = time.perf_counter() - t
    print("%s %s fp64, %d grids, colour V(1,1); level 0: %s" % (name, "x".join(map(str, shape)), grids,
                                                               "plane (fused CG step)" if flags["plane"] else
                                                               "var7" if flags["var7"] else "row kernels"))
    print("  per PCG iteration: %.3f ms = V-cycle %.3f ms + CG kernels %.3f ms" % (ms_pcg, ms_cyc, ms_cg))
    print("  CG kernels: %.2f GB per iteration in %.3f ms = %.2f TB/s = %.2f of 8 TB/s" % (gb / 1e9, ms_cg, gb / (ms_cg * 1e-3) / 1e12,
                                                                                       gb / (ms_cg * 1e-3) / PEAK))
    print("  to 1e-8 relative: PCG %d iterations, %.1f ms (true residual %.3e, breakdown %s); plain %d cycles, %.1f ms; "
          "time ratio PCG / plain = %.2f" % (its, 1e3 * t_pcg, tn / np.linalg.norm(b), bd, cycles, 1e3 * t_plain, t_pcg / t_plain))
    sys.stdout.flush()


if __name__ == "__main__":
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    shape = (size,) * 3
    probe("stencil_poisson", operators.stencil_poisson(shape), shape)
    probe("stencil7_variable", operators.stencil7_variable(shape), shape)
