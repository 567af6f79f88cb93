#!/usr/bin/env python3
"""What does a mixed-precision iteration (OMG_DTYPE_MIXED: fp32 V-cycle inside fp64 FCG / defect correction) cost at
256^3, and what does it buy?
    python tools/mixed_probe.py [size]
Per operator (stencil_poisson and stencil7_variable, colour V(1,1), 5 grids, set up on the device):
  - ms per mixed PCG iteration (32 iterations, threshold 0, bracketed by hipEvents on the hierarchy's stream), the fp32
    cycle's share (32 resident cycles of the fp32 hierarchy bracketed the same way) and the fp64 CG kernels' (the
    difference); the CG kernels' bytes / their time, as a fraction of 8 TB/s;
  - iterations and wall time to relative true residual 1e-10 for fp64 PCG, mixed PCG, fp64 plain cycles and mixed plain
    cycles (resident cycles in batches of 8);
  - the fp32 hierarchy's floor: the fp64 ||b - A x|| / ||b|| of its PCG iterate after 200 iterations."""
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


def to_tol_pcg(h, b, tol):
    h.resident_load(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    its, _, tn, bd = h.resident_pcg(1, 1, 2000, tol)
    return its, time.perf_counter() - t, tn, bd


def to_tol_plain(h, b, tol, cap=3000):
    h.resident_load(b)
    torch.cuda.synchronize()
    t = time.perf_counter()
    cycles, nv = 0, np.inf
    while nv >= tol and cycles < cap:
        got = h.resident_cycles(1, 1, 8)
        below = [k for k, v in enumerate(got) if v < tol]
        cycles += below[0] + 1 if below else 8
        nv = got[below[0]] if below else got[-1]
    return cycles, time.perf_counter() - t, nv


def probe(name, A0, shape, grids=5):
    n = A0.shape[0]
    b = np.random.default_rng(7).standard_normal(n)
    nb = np.linalg.norm(b)
    tol = 1e-10 * nb
    stream = torch.cuda.Stream()
    mk = lambda dtype: _hip.Hierarchy.from_fine(A0, shape, grids - 1, smoother="colour", dtype=dtype)
    with mk("float32") as h32:
        h32.set_stream(stream.cuda_stream)
        h32.resident_load(b)
        h32.resident_cycles(1, 1, 4)
        h32.resident_load(b)
        ms_cyc32 = timed(stream, lambda: h32.resident_cycles(1, 1, K)) / K
        h32.resident_load(b)
        h32.resident_pcg(1, 1, 200, 0.0)
        floor32 = np.linalg.norm(b - A0 @ h32.resident_fetch()) / nb
    with mk("float64") as h64:
        h64.set_stream(stream.cuda_stream)
        h64.resident_load(b)
        h64.resident_pcg(1, 1, 4)
        h64.resident_load(b)
        ms_pcg64 = timed(stream, lambda: h64.resident_pcg(1, 1, K)) / K
        r64 = to_tol_pcg(h64, b, tol)
        p64 = to_tol_plain(h64, b, tol)
    with mk("mixed") as hm:
        hm.set_stream(stream.cuda_stream)
        flags = hm.level_flags(0)
        hm.resident_load(b)
        hm.resident_pcg(1, 1, 4)                                  # warm-up (buffers, formats)
        hm.resident_cycles(1, 1, 4)
        hm.resident_load(b)
        ms_pcg = timed(stream, lambda: hm.resident_pcg(1, 1, K)) / K
        hm.resident_load(b)
        ms_plain = timed(stream, lambda: hm.resident_cycles(1, 1, K)) / K
        rm = to_tol_pcg(hm, b, tol)
        pm = to_tol_plain(hm, b, tol)
        xm = hm.resident_fetch()
    ms_cg = ms_pcg - ms_cyc32
    if flags["plane"]:
        per_cell = 20 + 28 + 52                                   # dots, fused step, update (+ fl32(r))
    else:
        per_cell = 20 + 20 + (12 * A0.nnz / n + 4 + 16) + 16 + 52  # dots, p update, fp64 CSR SpMV, dot, update
    gb = per_cell * n
    print("%s %s mixed (fp32 levels, fp64 outer), %d grids, colour V(1,1); level 0: %s" % (
        name, "x".join(map(str, shape)), grids,
        "plane (fused CG step)" if flags["plane"] else "var7 (fp64 CSR SpMV outside)" if flags["var7"] else "row kernels"))
    print("  per mixed PCG iteration: %.3f ms = fp32 cycle %.3f ms + fp64 CG kernels %.3f ms  (fp64 PCG: %.3f ms)" % (
        ms_pcg, ms_cyc32, ms_cg, ms_pcg64))
    print("  CG kernels: %.2f GB per iteration (%.0f B/cell) in %.3f ms = %.2f TB/s = %.2f of 8 TB/s" % (
        gb / 1e9, per_cell, ms_cg, gb / (ms_cg * 1e-3) / 1e12, gb / (ms_cg * 1e-3) / PEAK))
    print("  per mixed plain cycle (defect correction): %.3f ms" % ms_plain)
    print("  to 1e-10 relative: fp64 PCG %d its, %.1f ms | mixed PCG %d its, %.1f ms (true %.3e, breakdown %s) | "
          "fp64 plain %d cycles, %.1f ms | mixed plain %d cycles, %.1f ms" % (
              r64[0], 1e3 * r64[1], rm[0], 1e3 * rm[1], rm[2] / nb, rm[3], p64[0], 1e3 * p64[1], pm[0], 1e3 * pm[1]))
    print("  mixed PCG / fp64 PCG time = %.2f; host fp64 residual of the mixed plain iterate %.3e; fp32 hierarchy floor "
          "(200 PCG its) %.3e" % (rm[1] / r64[1], np.linalg.norm(b - A0 @ xm) / nb, floor32))
    sys.stdout.flush()


if __name__ == "__main__":
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    shape = (size,) * 3
    probe("stencil_poisson", operators.stencil_poisson(shape), shape)
    probe("stencil7_variable", operators.stencil7_variable(shape), shape)
