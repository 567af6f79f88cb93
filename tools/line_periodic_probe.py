#!/usr/bin/env python3
"""What do periodic levels cost the zebra line smoother ('smoother': 'line-periodic', csrc/line.hip)?

    python tools/line_periodic_probe.py N        # writes profiles/line_periodic_N.txt (and prints it)

N^3 cells, a 7-point operator with per-cell coefficients and couplings 100 : 1 : 1 along the lines' axis — the unit-stride
one, then the slowest —, fp64 and fp32 levels.  Four hierarchies per axis and precision, in one process: the in-grid operator
under 'line' (what tools/line_probe.py measures), the same operator with the two axes ACROSS the lines periodic (wrapped
neighbours: the same kernel, other neighbour ranks), with the lines' own axis periodic (cyclic lines: the CYCLIC kernel, two
more streams) and with all three periodic (plus a shift of the diagonal).  Microseconds per sweep of level 0 by hipEvents
around the sweeps' launches (omg_profile_*), the four alternating; every timing is printed, the ratio is formed from the
best of each."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
from openmg_amd import _hip, operators

HBM_PEAK = 8000.0e9          # bytes / s, the peak bench.py's roofline uses
SWEEPS, ROUNDS = 10, 5


def face_operator(shape, factors, seed, periodic=(), sigma=0.0):
    """factors[a] * (face-weighted differences along axis a), cell coefficients uniform in [0.5, 2]; a periodic axis has the
    face between its last and its first cell, the others Dirichlet walls; sorted CSR"""
    d, n = len(shape), int(np.prod(shape))
    idx = np.arange(n, dtype=np.int32).reshape(shape)
    kap = np.random.default_rng(seed).uniform(0.5, 2.0, shape)
    diag = np.full(shape, float(sigma))
    rows, cols, vals = [], [], []
    for a, f in enumerate(factors):
        lo, hi = [slice(None)] * d, [slice(None)] * d
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        pairs = [(tuple(lo), tuple(hi))]
        if a in periodic:
            lo[a], hi[a] = slice(-1, None), slice(0, 1)
            pairs.append((tuple(lo), tuple(hi)))
        for lo_, hi_ in pairs:
            c = f * 0.5 * (kap[lo_] + kap[hi_])
            rows += [idx[lo_].ravel(), idx[hi_].ravel()]
            cols += [idx[hi_].ravel(), idx[lo_].ravel()]
            vals += [-c.ravel(), -c.ravel()]
            diag[lo_] += c
            diag[hi_] += c
        if a not in periodic:
            for end in (0, -1):
                face = [slice(None)] * d
                face[a] = end
                diag[tuple(face)] += f * kap[tuple(face)]
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def sweep_us(h, b, x):
    """microseconds per sweep of level 0: SWEEPS sweeps through omg_level_smooth, the events around the sweeps' launches"""
    before = h.profile_read()["smoother_set_sweep"]
    h.smooth(0, b, x.copy(), SWEEPS)
    after = h.profile_read()["smoother_set_sweep"]
    assert after[0] - before[0] == SWEEPS, (before, after)
    return 1e3 * (after[1] - before[1]) / SWEEPS


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    shape = (size,) * 3
    n = size ** 3
    grids = max(2, int(np.log2(size)) - 2)                     # down to 8^3
    out = []
    say = lambda line="": (out.append(line), print(line, flush=True))
    say("tools/line_periodic_probe.py %d: %d^3 cells, %d grids, per-cell coefficients, couplings 100 : 1 : 1 along the lines; %d sweeps"
        " per timing, %d alternations; HBM peak %.0f GB/s" % (size, size, grids, SWEEPS, ROUNDS, HBM_PEAK / 1e9))
    say("values per cell and sweep — tridiagonal lines: 12 (forward: b, 4 cross couplings, the other colour's x, f read, y written;"
        " back: y, u, 1/p read, x written); cyclic lines: 14 (+ the fill row forward, the fill column backward)")
    say()
    say("| lines along | dtype | in-grid 'line' us | wrapped neighbours us | ratio | cyclic lines us | ratio | cyclic + wrapped us | ratio |"
        " cyclic GB/s | of peak | every timing: in-grid; wrapped; cyclic; cyclic + wrapped |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    R = operators.restrictionList(shape, grids - 2, 8)
    rng = np.random.default_rng(1)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    for axis in (2, 0):
        factors = [1.0, 1.0, 1.0]
        factors[axis] = 100.0
        across = tuple(a for a in range(3) if a != axis)
        kinds = [("in-grid", (), 0.0), ("wrapped", across, 0.0), ("cyclic", (axis,), 0.0), ("cyclic + wrapped", (0, 1, 2), 0.5)]
        lists = [operators.coeffecientList(face_operator(shape, factors, 7, per, sigma), R) for _, per, sigma in kinds]
        for dtype, vb in (("float64", 8), ("float32", 4)):
            hs = []
            try:
                for k, A in enumerate(lists):
                    code = _hip.line_smoother_code(axis, shape, wrap=k > 0)
                    h = _hip.Hierarchy(A, R, smoother=code, dtype=dtype)
                    hs.append(h)
                    assert h.level_flags(0)["line"] and h.line_axis == axis
                    h.profile_enable(["smoother_set_sweep"])
                t = [[] for _ in hs]
                for _ in range(ROUNDS):
                    for k, h in enumerate(hs):
                        t[k].append(sweep_us(h, b, x))
            finally:
                for h in hs:
                    h.close()
            best = [min(v) for v in t]
            gbs = 14 * n * vb / (best[2] * 1e-6)
            say("| %s | %s | %.1f | %.1f | %.3f | %.1f | %.3f | %.1f | %.3f | %.0f | %.3f | %s |"
                % ("xyz"[2 - axis] + " (problemShape[%d])" % axis, dtype, best[0], best[1], best[1] / best[0], best[2], best[2] / best[0],
                   best[3], best[3] / best[0], gbs / 1e9, gbs / HBM_PEAK, "; ".join(" ".join("%.1f" % v for v in row) for row in t)))
    say()
    say("lines per colour %d, cells per line %d: one thread per line, %d waves per launch, two launches per sweep"
        % (size * size // 2, size, size * size // 128))
    path = os.path.join(ROOT, "profiles", "line_periodic_%d.txt" % size)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
