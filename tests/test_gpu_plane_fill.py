"""The fill and drain steps of a plane pass's chunks (openmg_amd/csrc/plane.hip, plane_kernel's `step`: a chunk [z0, z1)
marches from step z0 - 2 to z1 + 1) run only the stages whose results reach an owned plane, a coarse slot or a square
(the live-step table).  Whatever the chunk geometry, the sweep counts, the number format, the marching
direction and the way the cycles are issued: the iterate has the bits of the set-by-set schedule of the same hierarchy
(OMG_PLANE=0), the norms agree to rounding as in tests/test_gpu_plane.py.

Every hierarchy here has three grids and is built with OMG_PLANE_BLOCK=0, so that the level below the finest marches too:
its down pass starts from a zero iterate, its up pass forms no norm — the instantiations whose red sweeps are skipped.

Run as a script (`test_gpu_plane_fill.py worker`) it prints a JSON report of a subset of the cases: the poison test
starts it with OMG_POISON=1 in a process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from openmg_amd import _hip, operators

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEPS = ((1, 1), (1, 0), (0, 1), (0, 0), (2, 1))
DTYPES = ("float64", "float32")
CYCLES = 3
# (nz, ny, nx): three grids with even extents on the two that are relaxed; tiles of 16 x 6 divide neither 36 nor 20 (nor 18, 10)
SHAPE_A = (24, 20, 36)
SHAPE_B = (44, 20, 36)
# tile, shape, what the chunks of level 0 / level 1 look like
GEOMETRIES = [
    ("16,6,2", SHAPE_A),     # chunks of two planes: fill and drain steps outnumber the chunk's own
    ("16,6,4", SHAPE_A),     # six chunks / three
    ("16,6,6", SHAPE_A),     # four chunks / two
    ("16,6,10", SHAPE_A),    # a last chunk shorter than LZ: 10 + 10 + 4 / 10 + 2
    ("16,6,12", SHAPE_A),    # two chunks / one
    ("16,6,24", SHAPE_A),    # one chunk covering all of nz
    ("16,6,6", SHAPE_B),     # nz = 44: seven chunks and one of two planes / three and one of four
    ("16,6,22", SHAPE_B),    # two chunks / one
    ("16,6,44", SHAPE_B),    # one chunk
    ("12,10,4", SHAPE_B),    # another ring: eleven chunks / five and one of two planes
]


def aggregation(shape):
    """2x2x2 cell aggregation with weight 1/8 for any even shape (as tests/test_gpu_plane.py)."""
    mats = []
    for s in shape:
        m = sp.lil_matrix((s // 2, s))
        for i in range(s // 2):
            m[i, 2 * i] = 0.5
            m[i, 2 * i + 1] = 0.5
        mats.append(sp.csr_matrix(m))
    R = mats[0]
    for m in mats[1:]:
        R = sp.kron(R, m, format="csr")
    R = sp.csr_matrix(R)
    R.sort_indices()
    return R


_problems = {}


def problem(shape):
    """Galerkin hierarchy over three grids, a right-hand side and a first iterate (both exact in fp32 too)."""
    if shape not in _problems:
        A = [sp.csr_matrix(operators.stencil_poisson(shape) * 0.37)]
        R = []
        sh = tuple(shape)
        for _ in range(2):
            R.append(aggregation(sh))
            Ac = sp.csr_matrix((R[-1] @ A[-1]) @ R[-1].T)
            Ac.sort_indices()
            A.append(Ac)
            sh = tuple(s // 2 for s in sh)
        rng = np.random.default_rng(8)
        b = rng.standard_normal(A[0].shape[0]).astype(np.float32).astype(np.float64)
        x0 = rng.standard_normal(A[0].shape[0]).astype(np.float32).astype(np.float64)
        _problems[shape] = (A, R, b, x0)
    return _problems[shape]


def singles(h, b, x0, pre, post):
    h.resident_load(b, x0)
    norms = [h.resident_cycle(pre, post) for _ in range(CYCLES)]
    return norms, h.resident_fetch()


def batches(h, b, x0, pre, post):
    h.resident_load(b, x0)
    norms = h.resident_cycles(pre, post, 1) + h.resident_cycles(pre, post, CYCLES - 1)
    return norms, h.resident_fetch()


def set_env(env):
    for k in ("OMG_PLANE", "OMG_PLANE_TILE", "OMG_PLANE_BLOCK", "OMG_PLANE_LA2", "OMG_PLANE_MIRROR"):
        os.environ.pop(k, None)
    os.environ.update(env)


_references = {}


def reference(shape, dtype):
    """{(pre, post): (norms, x)} of the set-by-set schedule (OMG_PLANE=0; a process's poison fill does not change it)."""
    if (shape, dtype) not in _references:
        A, R, b, x0 = problem(shape)
        set_env({"OMG_PLANE": "0", "OMG_PLANE_BLOCK": "0"})
        with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype) as h:
            assert not h.level_flags(0)["plane"] and not h.level_flags(1)["plane"]
            _references[(shape, dtype)] = {sw: singles(h, b, x0, *sw) for sw in SWEEPS}
    return _references[(shape, dtype)]


def marching(shape, dtype, tile, la2=True):
    """The hierarchy with both relaxed levels on the marching kernel under the given tiling."""
    A, R, _, _ = problem(shape)
    set_env({"OMG_PLANE": "1", "OMG_PLANE_BLOCK": "0", "OMG_PLANE_TILE": tile, "OMG_PLANE_LA2": "1" if la2 else "0"})
    h = _hip.Hierarchy(A, R, smoother="colour", dtype=dtype)
    want = [int(v) for v in tile.split(",")]
    for level in (0, 1):
        assert h.level_flags(level)["plane"], (shape, level)
        info = h.plane_info(level)
        assert [info["tile_x"], info["tile_y"], info["tile_z"]] == want, (level, info)
    return h


def differences(got, ref, dtype):
    """None, or what differs: the iterate bit for bit, the norms as tests/test_gpu_plane.py compares them."""
    tol = 1e-13 if dtype == "float64" else 1e-12
    if not np.all(np.isfinite(got[1])) or not np.all(np.isfinite(got[0])):
        return "not finite"
    if not np.array_equal(got[1], ref[1]):
        return "%d entries of the iterate differ" % int(np.sum(got[1] != ref[1]))
    if not all(abs(u - v) <= tol * abs(v) for u, v in zip(got[0], ref[0])):
        return "norms %r against %r" % (got[0], ref[0])
    return None


@pytest.fixture(autouse=True)
def restore_environment():
    saved = dict(os.environ)
    yield
    os.environ.clear()
    os.environ.update(saved)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", GEOMETRIES)
def test_chunk_geometries_sweep_counts_and_directions(tile, shape, dtype):
    """Single resident_cycle calls: every chunk geometry x sweep count x number format, the up pass marching down
    (default) and up (OMG_PLANE_MIRROR=0, read per call)."""
    _, _, b, x0 = problem(shape)
    ref = reference(shape, dtype)
    with marching(shape, dtype, tile) as h:
        for mirror in ("1", "0"):
            os.environ["OMG_PLANE_MIRROR"] = mirror
            for sw in SWEEPS:
                bad = differences(singles(h, b, x0, *sw), ref[sw], dtype)
                assert bad is None, (tile, shape, dtype, mirror, sw, bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", [GEOMETRIES[0], GEOMETRIES[3], GEOMETRIES[5], GEOMETRIES[6], GEOMETRIES[7]])
def test_batches_and_graph_replay(tile, shape, dtype):
    """resident_cycles batches (1 + 2 cycles) and single calls replayed from a captured graph."""
    _, _, b, x0 = problem(shape)
    ref = reference(shape, dtype)
    with marching(shape, dtype, tile) as h:
        for sw in SWEEPS:
            bad = differences(batches(h, b, x0, *sw), ref[sw], dtype)
            assert bad is None, ("batch", tile, shape, dtype, sw, bad)
        h.use_graph(True)
        for sw in SWEEPS:
            bad = differences(singles(h, b, x0, *sw), ref[sw], dtype)
            assert bad is None, ("graph", tile, shape, dtype, sw, bad)
        h.use_graph(False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_step_of_lookahead_below_the_finest_level(dtype):
    """OMG_PLANE_LA2=0: the level below the finest with the finest level's one-step form of the loop."""
    _, _, b, x0 = problem(SHAPE_B)
    ref = reference(SHAPE_B, dtype)
    for tile in ("16,6,6", "16,6,22"):
        with marching(SHAPE_B, dtype, tile, la2=False) as h:
            for sw in SWEEPS:
                bad = differences(singles(h, b, x0, *sw), ref[sw], dtype)
                assert bad is None, (tile, dtype, sw, bad)


WORKER_GEOMETRIES = [GEOMETRIES[0], GEOMETRIES[3], GEOMETRIES[5], GEOMETRIES[6], GEOMETRIES[8]]


def worker():
    report = []
    for tile, shape in WORKER_GEOMETRIES:
        _, _, b, x0 = problem(shape)
        for dtype in DTYPES:
            ref = reference(shape, dtype)
            with marching(shape, dtype, tile) as h:
                for mirror in ("1", "0"):
                    os.environ["OMG_PLANE_MIRROR"] = mirror
                    for sw in SWEEPS:
                        for name, how in (("singles", singles), ("batches", batches)):
                            report.append({"case": [tile, list(shape), dtype, mirror, list(sw), name],
                                           "bad": differences(how(h, b, x0, *sw), ref[sw], dtype)})
    print(json.dumps(report))


def test_skipped_stages_leave_no_path_from_unwritten_memory():
    """The same comparison in a process whose every fresh device allocation holds NaN patterns (OMG_POISON=1, as
    tests/test_gpu_poison.py): a stage skipped in a fill step must not let a value nobody wrote reach a stored one."""
    env = dict(os.environ, OMG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "worker"], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    report = json.loads(run.stdout.strip().splitlines()[-1])
    assert len(report) == len(WORKER_GEOMETRIES) * len(DTYPES) * 2 * len(SWEEPS) * 2
    for c in report:
        assert c["bad"] is None, c


if __name__ == "__main__":
    if sys.argv[1:] == ["worker"]:
        worker()
