#!/usr/bin/env python3
"""What does the zebra line smoother ('smoother': 'line', csrc/line.hip) cost, and what does it buy?

    python tools/line_probe.py N        # writes profiles/line_N.txt (and prints it)

N^3 cells, a 7-point operator with per-cell coefficients and couplings 100 : 1 : 1 — the strong axis each of the three in
turn —, fp64 and fp32 levels.  Per axis and precision: microseconds per line sweep (lines along the strong axis) beside the
set-schedule red-black sweep ('colour', omg_hierarchy_use_plane(0)) on the same operator in the same process, the two
alternating, timed by hipEvents around the sweeps' launches (omg_profile_*); the bytes a sweep has to move and what
fraction of the HBM peak that is.  Then, for the operator whose strong axis is the unit-stride one, cycles and wall time to
||r|| < 1e-8 ||b|| with 'colour' F(1.8) (fused passes on: the best the point smoothers offer), 'line' V and 'line' F(1.8)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
from openmg_amd import _hip, operators

HBM_PEAK = 8000.0e9          # bytes / s, the peak bench.py's roofline uses
SWEEPS, ROUNDS = 10, 4


def face_operator(shape, factors, seed):
    """factors[a] * (face-weighted differences along axis a), cell coefficients uniform in [0.5, 2], Dirichlet; sorted CSR"""
    d, n = len(shape), int(np.prod(shape))
    idx = np.arange(n, dtype=np.int32).reshape(shape)
    kap = np.random.default_rng(seed).uniform(0.5, 2.0, shape)
    diag = np.zeros(shape)
    rows, cols, vals = [], [], []
    for a, f in enumerate(factors):
        lo, hi = [slice(None)] * d, [slice(None)] * d
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        c = f * 0.5 * (kap[lo] + kap[hi])
        rows += [idx[lo].ravel(), idx[hi].ravel()]
        cols += [idx[hi].ravel(), idx[lo].ravel()]
        vals += [-c.ravel(), -c.ravel()]
        diag[lo] += c
        diag[hi] += c
        for end in (0, -1):
            face = [slice(None)] * d
            face[a] = end
            diag[tuple(face)] += f * kap[tuple(face)]
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def sweep_us(h, b, x, launches_per_sweep):
    """microseconds per sweep of level 0: SWEEPS sweeps through omg_level_smooth, the events around the sweeps' launches"""
    before = h.profile_read()["smoother_set_sweep"]
    h.smooth(0, b, x.copy(), SWEEPS)
    after = h.profile_read()["smoother_set_sweep"]
    assert after[0] - before[0] == SWEEPS * launches_per_sweep, (before, after)
    return 1e3 * (after[1] - before[1]) / SWEEPS


def cycles_to(h, b, shape, alpha, target, limit):
    h.set_cycle(shape, alpha)
    h.resident_load(b)
    h.sync()
    t0 = time.perf_counter()
    k, norm = 0, float("inf")
    while k < limit and not norm < target:
        norm = h.resident_cycle(1, 1)
        k += 1
    return k, 1e3 * (time.perf_counter() - t0), norm


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    shape = (size,) * 3
    n = size ** 3
    grids = max(2, int(np.log2(size)) - 2)                     # down to 8^3
    out = []
    say = lambda line="": (out.append(line), print(line, flush=True))
    say("tools/line_probe.py %d: %d^3 cells, %d grids, per-cell coefficients, couplings 100 : 1 : 1; %d sweeps per timing, %d"
        " alternations, the best of them; HBM peak %.0f GB/s" % (size, size, grids, SWEEPS, ROUNDS, HBM_PEAK / 1e9))
    say("bytes per sweep — line: 12 values per cell (forward: b, 4 cross couplings, the other colour's x, f read, y written;"
        " back: y, u, 1/p read, x written); colour: the two sets' operator bytes as held (omg_hierarchy_format_info) + 3 values"
        " per cell (b, x read, x written)")
    say()
    say("| strong axis (lines along it) | dtype | line sweep us | GB/s | of peak | colour set-schedule sweep us | GB/s | of peak | line / colour | every timing: line; colour |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    R = operators.restrictionList(shape, grids - 2, 8)
    rng = np.random.default_rng(1)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    keep = None
    for axis in (2, 1, 0):
        factors = [1.0, 1.0, 1.0]
        factors[axis] = 100.0
        A0 = face_operator(shape, factors, seed=7)
        A = operators.coeffecientList(A0, R)
        if axis == 2:
            keep = (A0, A)
        for dtype, vb in (("float64", 8), ("float32", 4)):
            with _hip.Hierarchy(A, R, smoother=_hip.line_smoother_code(axis, shape), dtype=dtype) as hl, \
                    _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as hc:
                assert hl.level_flags(0)["line"] and hl.line_axis == axis
                hc.use_plane(False)
                hl.profile_enable(["smoother_set_sweep"])
                hc.profile_enable(["smoother_set_sweep"])
                sets = hc.level_sets(0)
                tl, tc = [], []
                for _ in range(ROUNDS):
                    tl.append(sweep_us(hl, b, x, 1))
                    tc.append(sweep_us(hc, b, x, sets))
                bytes_line = 12 * n * vb
                bytes_colour = sum(hc.format_info(0, "A", s)["format_bytes"] for s in range(sets)) + 3 * n * vb
                ul, uc = min(tl), min(tc)
                gl, gc = bytes_line / (ul * 1e-6), bytes_colour / (uc * 1e-6)
                say("| %s | %s | %.1f | %.0f | %.3f | %.1f | %.0f | %.3f | %.2f | %s; %s |"
                    % ("xyz"[2 - axis] + " (problemShape[%d])" % axis, dtype, ul, gl / 1e9, gl / HBM_PEAK, uc, gc / 1e9, gc / HBM_PEAK, ul / uc,
                       " ".join("%.1f" % t for t in tl), " ".join("%.1f" % t for t in tc)))
    say()
    say("lines per colour %d, cells per line %d: one thread per line, %d waves per launch" % (size * size // 2, size, size * size // 128))
    say()
    A0, A = keep
    nb = float(np.linalg.norm(b))
    say("to ||r|| < 1e-8 ||b||, strong axis = the unit-stride one, fp64, V(1,1) sweeps, at most 600 cycles:")
    say("| smoother | cycle | cycles | ms | final ||r|| / ||b|| |")
    say("|---|---|---|---|---|")
    for kind, cyc, alpha in (("colour", "F", 1.8), ("line", "V", 1.0), ("line", "F", 1.8)):
        with _hip.Hierarchy(A, R, smoother=kind) as h:
            cycles_to(h, b, cyc, alpha, 0.0, 2)                  # (warm: first-use formats, tunings)
            k, ms, norm = cycles_to(h, b, cyc, alpha, 1e-8 * nb, 600)
            say("| %s | %s(%.1f) | %d%s | %.1f | %.2e |" % (kind, cyc, alpha, k, "" if norm < 1e-8 * nb else " (not reached)", ms, norm / nb))
    path = os.path.join(ROOT, "profiles", "line_%d.txt" % size)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
