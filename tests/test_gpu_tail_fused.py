"""The fused tail of the V-cycle (openmg_amd/csrc/plane.hip tail_up_kernel; OMG_TAIL_FUSE=0|1|2 when a hierarchy is made):
the 16^3 sine solve and the up passes of the one or two block levels above it in one launch.  It must leave the bits of
the launches it replaces, so every comparison here is array_equal — on resident_fetch() and on every returned norm against
the same hierarchy made with OMG_TAIL_FUSE=0, and on the iterate against the set-by-set schedule (use_plane(False)).

The norms of the set-by-set schedule are compared to 1e-12 relative (fp32 levels: 1e-6), not bit for bit: that schedule
adds the squares of the residual in another order than the plane passes (include/openmg_hip.h at omg_hierarchy_use_plane:
"same iterate, bit for bit; the norm's partial sums are associated differently"), with or without this launch; the
tolerances are the ones tests/test_gpu_cycle_shapes.py and tests/poison_worker.py use for the same pair.

Whether the launch RAN is read from Hierarchy.tail_info() (omg_hierarchy_tail_info: launches put on the stream, and how many
of them by a graph replay), not only from level_flags: one per cycle where it must run, none where it must step aside.

Shapes: 64^3 with three grids (depth 1: 32^3 is the block level above the solve) and 128^3 with four (depth 2: 64^3 and
32^3) are the smallest hierarchies that reach either depth — the solve is 16^3 by definition and a block level is twice
the level below; the hierarchies that must NOT take the launch are 64^3-sized too (64 x 64 x 32 from host lists: the
device set-up wants the first and last extent equal).  Needs an MI355X: run with -m gpu."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators
from oracle import mg_oracle as orc

import stencils

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEPS = [(1, 1), (1, 0), (0, 1), (2, 2)]
BATCH, SINGLES = 5, 3


@functools.lru_cache(maxsize=None)
def poisson(shape, dtype="float64"):
    A0 = operators.stencil_poisson(shape)
    rng = np.random.default_rng(12345)
    b = A0 @ rng.random(A0.shape[0])
    x0 = rng.standard_normal(A0.shape[0])
    if dtype == "float32":
        b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
    b.setflags(write=False)
    x0.setflags(write=False)
    return A0, b, x0


class switch:
    """OMG_TAIL_FUSE for the hierarchies made inside the block"""

    def __init__(self, value):
        self.value = str(value)

    def __enter__(self):
        self.old = os.environ.get("OMG_TAIL_FUSE")
        os.environ["OMG_TAIL_FUSE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["OMG_TAIL_FUSE"]
        else:
            os.environ["OMG_TAIL_FUSE"] = self.old


def make(shape, grids, dtype, fuse):
    with switch(fuse):
        return _hip.Hierarchy.from_fine(poisson(shape, dtype)[0], shape, grids - 1, "colour", dtype=dtype)


def cycles(h, b, x0, pre, post):
    """a batch of cycles from x0 and single calls from zero: every norm, both iterates"""
    h.resident_load(b, x0)
    norms = h.resident_cycles(pre, post, BATCH)
    xs = [h.resident_fetch()]
    h.resident_load(b)
    norms += [h.resident_cycle(pre, post) for _ in range(SINGLES)]
    xs.append(h.resident_fetch())
    return np.array(norms), xs


@functools.lru_cache(maxsize=None)
def separate(shape, grids, dtype, setting=("V", 1.0), sweeps=tuple(SWEEPS)):
    """{sweeps: (cycles() of the separate launches, cycles() of the set-by-set schedule)} of a hierarchy made with the switch off"""
    _, b, x0 = poisson(shape, dtype)
    out = {}
    with make(shape, grids, dtype, 0) as h:
        h.set_cycle(*setting)
        assert not any(h.level_flags(l)["tail_fused"] for l in range(grids - 1))
        for pre, post in sweeps:
            h.use_plane(True)
            planes = cycles(h, b, x0, pre, post)
            h.use_plane(False)
            out[(pre, post)] = (planes, cycles(h, b, x0, pre, post))
    return out


def assert_same(got, want, sets, dtype, what):
    for k, (x, y) in enumerate(zip(got[1], want[1])):
        assert np.array_equal(x, y), (what, "separate launches", k, int(np.sum(x != y)))
    assert np.array_equal(got[0], want[0]), (what, "norms", got[0], want[0])
    for k, (x, y) in enumerate(zip(got[1], sets[1])):
        assert np.array_equal(x, y), (what, "set-by-set schedule", k, int(np.sum(x != y)))
    np.testing.assert_allclose(got[0], sets[0], rtol=1e-12 if dtype == "float64" else 1e-6)
    assert np.all(np.isfinite(got[0]))


def launches(h, run):
    """run() and the fused tail launches it put on the stream"""
    before = h.tail_info()[0]
    out = run()
    return out, h.tail_info()[0] - before


def check_all_sweeps(h, shape, grids, dtype, setting=("V", 1.0), sweeps=SWEEPS):
    """every cycle of a V hierarchy with at most one post-smoothing sweep holds the launch once; nothing else holds it"""
    _, b, x0 = poisson(shape, dtype)
    ref = separate(shape, grids, dtype, setting, tuple(sweeps))
    for pre, post in sweeps:
        got, ran = launches(h, lambda: cycles(h, b, x0, pre, post))
        assert ran == (BATCH + SINGLES if setting[0] == "V" and post <= 1 else 0), (shape, dtype, setting, pre, post, ran)
        assert_same(got, ref[(pre, post)][0], ref[(pre, post)][1], dtype, (shape, dtype, setting, pre, post))


# ------------------------------------------------------------------------------------- depth 1 --
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fuse", [1, 2])
def test_solve_and_one_up_pass_64(fuse, dtype):
    """64^3, three grids: 32^3 is the one block level between the entry level and the solve"""
    shape = (64, 64, 64)
    with make(shape, 3, dtype, fuse) as h:
        assert h.level_flags(1)["plane"] and h.level_flags(1)["tail_fused"]
        check_all_sweeps(h, shape, 3, dtype)


# ------------------------------------------------------------------------------------- depth 2 --
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fuse", [1, 2])
def test_solve_and_two_up_passes_128(fuse, dtype):
    """128^3, four grids: 64^3 and 32^3; V(2,2) runs the separate launches (more than one post-smoothing sweep)"""
    shape = (128, 128, 128)
    with make(shape, 4, dtype, fuse) as h:
        assert not h.level_flags(0)["tail_fused"]
        assert h.level_flags(1)["tail_fused"] == (fuse == 2) and h.level_flags(2)["tail_fused"]
        check_all_sweeps(h, shape, 4, dtype)


def test_over_correction_128():
    shape = (128, 128, 128)
    with make(shape, 4, "float64", 2) as h:
        h.set_cycle("V", 1.5)
        assert h.level_flags(1)["tail_fused"] and h.level_flags(2)["tail_fused"]
        check_all_sweeps(h, shape, 4, "float64", ("V", 1.5), [(1, 1), (1, 0)])


def test_replayed_from_a_graph_128():
    shape = (128, 128, 128)
    _, b, x0 = poisson(shape)
    want = separate(shape, 4, "float64", ("V", 1.0), tuple(SWEEPS))[(1, 1)][0]            # (shared with test_solve_and_two_up_passes_128)
    with make(shape, 4, "float64", 2) as h:
        h.use_graph(True)
        before = h.tail_info()
        got = cycles(h, b, x0, 1, 1)
        after = h.tail_info()
        h.use_graph(False)
    assert after[0] - before[0] == BATCH + SINGLES and after[1] - before[1] >= SINGLES, (before, after)
    assert np.array_equal(got[0], want[0])
    for x, y in zip(got[1], want[1]):
        assert np.array_equal(x, y)


# -------------------------------------------------------------------------------------- guards --
@pytest.mark.parametrize("setting", [("F", 1.0), ("W", 1.0)])
def test_f_and_w_cycles_keep_the_separate_launches(setting):
    shape = (128, 128, 128)
    with make(shape, 4, "float64", 2) as h:
        assert h.level_flags(1)["tail_fused"]
        h.set_cycle(*setting)
        assert not any(h.level_flags(l)["tail_fused"] for l in range(3))
        check_all_sweeps(h, shape, 4, "float64", setting, [(1, 1)])


def separate_launches_with_the_bits_of_the_sets(A, R):
    """a hierarchy made with the switch at 2 that must not take the fused launch: its flags, and its cycles both ways"""
    rng = np.random.default_rng(7)
    b, x0 = A[0] @ rng.random(A[0].shape[0]), rng.standard_normal(A[0].shape[0])
    with switch(2):
        h = _hip.Hierarchy(A, R, smoother="colour")
    with h:
        assert h.level_flags(0)["plane"] and h.level_flags(1)["plane"]
        assert not any(h.level_flags(l)["tail_fused"] for l in range(2))
        planes = cycles(h, b, x0, 1, 1)
        h.use_plane(False)
        sets = cycles(h, b, x0, 1, 1)
        assert h.tail_info() == (0, 0)
    for x, y in zip(planes[1], sets[1]):
        assert np.array_equal(x, y)
    np.testing.assert_allclose(planes[0], sets[0], rtol=1e-12)


def test_the_general_sine_kernel_keeps_the_separate_launches():
    """64 x 64 x 32, three grids: the coarsest grid is 16 x 16 x 8"""
    A, R = stencils.hierarchy((32, 64, 64), 3, (-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0))
    assert A[-1].shape[0] == 16 * 16 * 8
    separate_launches_with_the_bits_of_the_sets(A, R)


def test_another_coarse_solver_keeps_the_separate_launches():
    """seven pairwise different couplings at 64^3, three grids: the coarsest operator is not symmetric, no sine solve"""
    separate_launches_with_the_bits_of_the_sets(*stencils.hierarchy((64, 64, 64), 3, stencils.UNSYM7))


# ------------------------------------------------------------------------- unwritten memory --
POISONED = """
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_tail_fused as t
shape = (128, 128, 128)
_, b, x0 = t.poisson(shape)
with t.make(shape, 4, "float64", 2) as h:
    assert h.level_flags(1)["tail_fused"] and h.level_flags(2)["tail_fused"]
    out = {}
    for pre, post in ((1, 1), (0, 1), (1, 0)):
        h.use_plane(True)
        got = t.cycles(h, b, x0, pre, post)
        h.use_plane(False)
        sets = t.cycles(h, b, x0, pre, post)
        out["%d%d" % (pre, post)] = {"finite": bool(np.all(np.isfinite(got[0])) and all(np.all(np.isfinite(x)) for x in got[1])),
                                     "same_bits": bool(all(np.array_equal(x, y) for x, y in zip(got[1], sets[1]))),
                                     "norm_rel": float(np.max(np.abs(got[0] - sets[0]) / np.abs(sets[0])))}
    out["launches"] = h.tail_info()[0]
print(json.dumps(out))
"""


def test_reads_no_unwritten_memory():
    """every fresh device allocation filled with NaN patterns (OMG_POISON=1, read once per process: a process of its own)"""
    env = dict(os.environ, OMG_POISON="1")
    run = subprocess.run([sys.executable, "-c", POISONED, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    report = json.loads(run.stdout.strip().splitlines()[-1])
    assert report.pop("launches") == 3 * (BATCH + SINGLES)
    assert len(report) == 3
    for key, c in report.items():
        assert c["finite"] and c["same_bits"] and c["norm_rel"] <= 1e-12, (key, c)


# --------------------------------------------------------------------- the accelerated entries --
@pytest.mark.parametrize("kw", [{"accel": "cg"}, {"dtype": "mixed"}, {"accel": "cg", "dtype": "mixed"}])
def test_mgsolve_with_cg_and_mixed_precision_64(monkeypatch, kw):
    shape = (64, 64, 64)
    A0, _, _ = poisson(shape)
    b = np.random.default_rng(7).standard_normal(A0.shape[0])
    p = {"problemShape": shape, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "cycles": 6, "threshold": 0.0,
         "giveInfo": True, "smoother": "colour", "minSize": 1}
    res = {}
    for fuse in ("0", "1", "2"):
        monkeypatch.setenv("OMG_TAIL_FUSE", fuse)
        openmg_amd.clear_cache()
        res[fuse] = openmg_amd.mgSolve(A0, b, dict(p, **kw))
    openmg_amd.clear_cache()
    for fuse in ("1", "2"):
        assert np.array_equal(res[fuse][0], res["0"][0]), (kw, fuse)
        assert res[fuse][1]["norm"] == res["0"][1]["norm"] and res[fuse][1]["cycle"] == res["0"][1]["cycle"]
    assert np.all(np.isfinite(res["2"][0]))


@pytest.mark.parametrize("dtype", ["float64", "mixed"])
def test_pcg_and_mixed_entries_take_the_launch_64(dtype):
    """the entries mgSolve's accel='cg' and dtype='mixed' run (resident_pcg; resident cycles of a mixed hierarchy), on the
    hierarchy itself so that the launches can be counted: they take the fused launch, and leave the bits they leave without it"""
    shape = (64, 64, 64)
    b = np.random.default_rng(7).standard_normal(64 ** 3)
    res = {}
    for fuse in (0, 2):
        with make(shape, 3, dtype, fuse) as h:
            h.resident_load(b)
            its, norms, tn, bd = h.resident_pcg(1, 1, 6, 0.0)
            x_pcg, ran_pcg = h.resident_fetch(), h.tail_info()[0]
            h.resident_load(b)
            n = [h.resident_cycle(1, 1) for _ in range(3)]
            res[fuse] = (its, np.array(norms), tn, x_pcg, np.array(n), h.resident_fetch())
            ran_cycles = h.tail_info()[0] - ran_pcg
        assert not bd
        assert (ran_pcg >= its and ran_cycles >= 3) if fuse else (ran_pcg == 0 and ran_cycles == 0), (dtype, fuse, ran_pcg, ran_cycles)
    assert res[0][0] == res[2][0] and res[0][2] == res[2][2]
    for k in (1, 3, 4, 5):
        assert np.array_equal(res[0][k], res[2][k]), (dtype, k)


# ---------------------------------------------------------------------------------- the oracle --
def test_against_the_cpu_oracle_64():
    """two V(1,1) cycles at 64^3, three grids, from zero, against the CPU oracle on its own Galerkin lists: the 1e-10 of
    the other cycle tests (the hierarchy is the one mgSolve sets up: its products are exact for this operator)"""
    shape = (64, 64, 64)
    A0, b, _ = poisson(shape)
    R = orc.restriction_list(shape, 1, 1)
    A = orc.coefficient_list(A0, R)
    assert len(A) == 3 and A[-1].shape[0] == 16 ** 3
    po = {"problemShape": shape, "gridLevels": 2, "preIterations": 1, "postIterations": 1, "cycles": 2, "threshold": 0,
          "giveInfo": True, "smoother": "colour", "coarsestLevel": len(R)}
    sm = orc.make_smoother("colour", A)
    xo, want = None, []
    for _ in range(2):
        xo, inf = orc.mg_cycle(A, b, 0, R, po, initial=xo, smoother=sm)
        want.append(inf["norm"])
    with make(shape, 3, "float64", 2) as h:
        assert h.level_flags(1)["tail_fused"]
        h.resident_load(b)
        got = [h.resident_cycle(1, 1) for _ in range(2)]
        x = h.resident_fetch()
        assert h.tail_info()[0] == 2
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-10 * w, (g, w)
    assert np.allclose(x, np.asarray(xo).ravel(), rtol=1e-9, atol=1e-11)
