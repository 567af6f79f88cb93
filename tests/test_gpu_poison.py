"""Nothing the fused passes compute may depend on what freshly allocated device memory happens to hold (zeros in a young
process, arbitrary bits later: the 27-point sweeps once multiplied a zero coefficient with such bits and a long test run
turned its iterate into NaNs).  tests/poison_worker.py runs the fused paths beside the set-by-set schedule of the same
hierarchy in a process whose every device allocation starts as NaN patterns (OMG_POISON=1)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slab27_in_a_process_of_its_own(out, shape, world, n_levels, grids, dtype, p2p, **env):
    """tests/poison_worker.py slab27 ... with `env` added to the environment; the saved arrays"""
    import numpy as np
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "poison_worker.py"), "slab27", str(out), "x".join(map(str, shape)),
                          str(world), str(n_levels), str(grids), dtype, str(p2p)], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return dict(np.load(str(out)))


def test_peer_stores_into_a_pooled_level_stay_inside_their_vectors(tmp_path):
    """Two 27-point slabs of (8, 512, 256), fp64, whose level 0 keeps x, b and tmp in one allocation, peer stores between
    them (loopback): with every fresh allocation filled with NaN patterns — the pool's slack and the gaps between its three
    spans stay that way — the iterates and norms are finite and have the bits of a run without the fill.  A store or a load
    that strays out of a vector shows as a NaN or a changed bit.  (MI355X: 4.9 s for the two processes.)"""
    import numpy as np
    from test_gpu_dist27 import POOLED_SMALL, assert_pooled
    shape, grids, world, n_levels = POOLED_SMALL
    plain = slab27_in_a_process_of_its_own(tmp_path / "plain.npz", shape, world, n_levels, grids, "float64", 1)
    poisoned = slab27_in_a_process_of_its_own(tmp_path / "poison.npz", shape, world, n_levels, grids, "float64", 1, OMG_POISON="1")
    assert_pooled(json.loads(str(poisoned["layouts"])), shape, world, n_levels, "float64")
    for key in ("x11", "x10", "x21", "norms"):
        assert np.all(np.isfinite(poisoned[key])), key
        assert np.array_equal(poisoned[key], plain[key]), (key, int(np.sum(poisoned[key] != plain[key])))


def test_fused_passes_do_not_read_unwritten_memory():
    env = dict(os.environ, OMG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "poison_worker.py")], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    report = json.loads(run.stdout.strip().splitlines()[-1])
    assert len(report) == 12
    for name, cases in report.items():
        for c in cases:
            assert c["finite"] and c["same_bits"], (name, c)
            assert c["norm_rel"] <= 1e-6 if "float32" in name else c["norm_rel"] <= 1e-12, (name, c)
