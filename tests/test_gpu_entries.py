"""The entries of the C ABI that are one operation with several transports, pinned to each other bit for bit:
omg_vcycle / omg_vcycle_ex / omg_vcycle_dev; omg_resident_load[_dev] + omg_resident_cycle + omg_resident_fetch[_dev] /
omg_resident_cycles / omg_solve; omg_resident_pcg from host and from device arrays, and omg_resident_norms after it; what
the entries refuse.  Every comparison is np.array_equal on iterates and == on norms: there is no tolerance in this file.

The problems are the seven of tests/test_gpu_solver.py (one per kind of level 0: plane, wavefront, var7, 27-point, 2-D
Jacobi, line, null space) and a single-level hierarchy, in float64, float32 and — where the entry takes it — mixed.
Device arrays are torch tensors, so those comparisons run in a child process (one per problem) that calls the same
functions with a `dev`.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openmg_amd import _hip, operators
from test_gpu_cycle_shapes import EPS32
from test_gpu_nullspace import mean_of
from test_gpu_solver import NAMES, get, open_lists, check_flag, setenv

pytestmark = pytest.mark.gpu

ALL = NAMES + ["single"]
SWEEPS = [(1, 1), (2, 1), (0, 1)]


def problem_of(name):
    """test_gpu_solver.get(name); 'single': one level (len(R) == 0), whose every cycle is the direct solve"""
    if name != "single":
        return get(name)
    A0 = operators.stencil_poisson((8, 8, 8))
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    return {"name": name, "shape": (8, 8, 8), "A0": A0, "A": [A0], "R": [], "b": b, "kw": {"smoother": "colour"},
            "kind": "colour", "env": {}, "flag": None, "nullspace": None}


def rhs_of(pr):
    """level 0's right-hand side; with the null space one that has a mean, so that the projection has something to remove"""
    return pr["b"] + 0.3 if pr["nullspace"] else pr["b"]


def same_result(got, want):
    """two (norm(s), iterate) results, bit for bit"""
    return got[0] == want[0] and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------ 1. cycle entries --
def cycle_entries(pr, h, dev=None):
    """every case of omg_vcycle_ex against omg_vcycle, against what x_pre must hold, and — with dev — against omg_vcycle_dev"""
    last = len(pr["R"])
    rng = np.random.default_rng(21)
    for level in sorted({0, min(1, last), last}):
        n = h.sizes[level]
        b = rhs_of(pr) if level == 0 else rng.standard_normal(n)
        x0 = rng.standard_normal(n)
        zeros = np.zeros(n)
        direct = h.coarse_solve(b) if level == last else None
        for pre, post in SWEEPS:
            for start in (x0, None):
                first = zeros if start is None else start
                x = first.copy()
                want = (h.vcycle(b, x, pre, post, level), x)
                if level < last and pre > 0:
                    want_pre = h.smooth(level, b, first.copy(), pre)       # the iterate after the pre-smoothing
                else:
                    want_pre = first                                       # the input's copy; zeros with no input
                if level == last:
                    assert want[0] == 0.0 and np.array_equal(want[1], direct), (pr["name"], level)
                for x_pre in ("absent", "separate") + (() if start is None else ("x_in",)):
                    case = (pr["name"], level, pre, post, start is not None, x_pre)
                    x_in = None if start is None else start.copy()
                    x_out = np.full(n, np.nan)
                    pre_out = {"absent": None, "separate": np.full(n, np.nan), "x_in": x_in}[x_pre]
                    norm = h.vcycle_ex(b, x_in, x_out, pre_out, pre, post, level)
                    assert same_result((norm, x_out), want), case
                    assert pre_out is None or np.array_equal(pre_out, want_pre), case
                    if x_in is not None and x_pre != "x_in":
                        assert np.array_equal(x_in, start), case
                    if dev is None:
                        continue
                    bd, out_d = dev.put(b), dev.put(np.full(n, np.nan))
                    in_d = None if start is None else dev.put(start)
                    pre_d = {"absent": None, "separate": dev.put(np.full(n, np.nan)), "x_in": in_d}[x_pre]
                    norm = h.vcycle_dev(dev.addr(bd), dev.addr(in_d), dev.addr(out_d), dev.addr(pre_d), pre, post, level)
                    assert same_result((norm, dev.get(out_d)), want), case
                    assert pre_d is None or np.array_equal(dev.get(pre_d), want_pre), case
                    assert np.array_equal(dev.get(bd), b), case
                    if in_d is not None and x_pre != "x_in":
                        assert np.array_equal(dev.get(in_d), start), case


# --------------------------------------------------------------------------- 2. resident entries --
def resident_entries(pr, h, dtype, dev=None):
    """load + three omg_resident_cycle + fetch, against omg_resident_cycles, omg_solve and — with dev — the _dev load and fetch"""
    b = rhs_of(pr)
    n = b.size
    for x0 in (None, np.random.default_rng(5).standard_normal(n)):
        for graph in (False, True):
            case = (pr["name"], dtype, x0 is not None, graph)
            h.use_graph(graph)
            h.resident_load(b, x0)
            want = ([h.resident_cycle(1, 1) for _ in range(3)], h.resident_fetch())
            h.resident_load(b, x0)
            assert same_result((h.resident_cycles(1, 1, 3), h.resident_fetch()), want), case
            if dtype != "mixed":
                x = np.zeros(n) if x0 is None else x0.copy()
                assert h.solve(b, x, 1, 1, 3, 0.0) == (3, want[0][-1]) and np.array_equal(x, want[1]), case
            if pr["nullspace"]:
                # (the gates of tests/test_gpu_nullspace.py: the projection's own rounding, in the precision it runs in)
                gate = 64 * EPS32 if dtype == "float32" else 1e-13
                assert abs(mean_of(b)) > 0.29 and abs(mean_of(want[1])) <= gate * np.abs(want[1]).max(), case
            if len(pr["R"]) == 0 and dtype != "mixed":
                # (a mixed hierarchy's cycle corrects the fp64 iterate by the fp32 direct solve: its norm is a true residual's)
                assert want[0] == [0.0, 0.0, 0.0] and np.array_equal(want[1], h.coarse_solve(b)), case
            if dev is None:
                continue
            bd, out_d = dev.put(b), dev.put(np.full(n, np.nan))
            xd = None if x0 is None else dev.put(x0)
            for batched in (False, True):
                h.resident_load_dev(dev.addr(bd), dev.addr(xd))
                norms = h.resident_cycles(1, 1, 3) if batched else [h.resident_cycle(1, 1) for _ in range(3)]
                h.resident_fetch_dev(dev.addr(out_d))
                assert same_result((norms, dev.get(out_d)), want), case + (batched,)
            assert np.array_equal(dev.get(bd), b) and (xd is None or np.array_equal(dev.get(xd), x0)), case
    h.use_graph(False)


# ------------------------------------------------------------------------------------- 3. FCG --
def fcg_entries(pr, h, dtype, dev=None):
    """omg_resident_pcg twice from one state, omg_resident_norms behind it, and — with dev — from the _dev load and fetch"""
    b = rhs_of(pr)
    n = b.size
    x0 = np.random.default_rng(5).standard_normal(n)

    def run(load, fetch):
        load()
        its, norms, true_norm, breakdown = h.resident_pcg(1, 1, 4)
        after = h.resident_norms()[1]                   # (before the fetch, which projects the iterate where there is a null space)
        return (its, list(norms), true_norm, breakdown, after), fetch()

    want = run(lambda: h.resident_load(b, x0), h.resident_fetch)
    case = (pr["name"], dtype)
    assert want[0][0] == 4 and len(want[0][1]) == 4 and not want[0][3], case
    # the true norm and omg_resident_norms are the same launches on the same resident b and x
    assert want[0][4] == want[0][2], case
    assert same_result(run(lambda: h.resident_load(b, x0), h.resident_fetch), want), case
    if dev is None:
        return
    bd, xd, out_d = dev.put(b), dev.put(x0), dev.put(np.full(n, np.nan))

    def fetch_dev():
        h.resident_fetch_dev(dev.addr(out_d))
        return dev.get(out_d)

    assert same_result(run(lambda: h.resident_load_dev(dev.addr(bd), dev.addr(xd)), fetch_dev), want), case
    assert np.array_equal(dev.get(bd), b) and np.array_equal(dev.get(xd), x0), case


def dtypes_of(entries):
    return ("float64", "float32") if entries is cycle_entries else ("float64", "float32", "mixed")


def every_entry(pr, dev=None):
    """what the child process runs: all three groups in every precision on one problem"""
    for entries in (cycle_entries, resident_entries, fcg_entries):
        if entries is fcg_entries and len(pr["R"]) == 0:
            continue                                    # (nothing to accelerate: refused, test_what_the_entries_refuse)
        for dtype in dtypes_of(entries):
            with open_lists(pr, dtype=dtype) as h:
                check_flag(pr, h)
                if entries is cycle_entries:
                    entries(pr, h, dev)
                else:
                    entries(pr, h, dtype, dev)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ALL)
def test_the_three_cycle_entries_are_one_cycle(monkeypatch, name, dtype):
    pr = problem_of(name)
    setenv(pr, monkeypatch)
    with open_lists(pr, dtype=dtype) as h:
        check_flag(pr, h)
        cycle_entries(pr, h)


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("name", ALL)
def test_single_batched_and_solved_cycles_are_the_same_cycles(monkeypatch, name, dtype):
    pr = problem_of(name)
    setenv(pr, monkeypatch)
    with open_lists(pr, dtype=dtype) as h:
        check_flag(pr, h)
        resident_entries(pr, h, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("name", NAMES)
def test_fcg_repeats_itself_and_its_true_norm_is_resident_norms(monkeypatch, name, dtype):
    pr = problem_of(name)
    setenv(pr, monkeypatch)
    with open_lists(pr, dtype=dtype) as h:
        check_flag(pr, h)
        fcg_entries(pr, h, dtype)


# ----------------------------------------------------------------------------- 4. device arrays --
# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as in tests/test_gpu_solver.py)
DEVICE_ARRAYS = """
import os
import sys
import torch
torch.cuda.init()
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import test_gpu_entries as t


class Dev:
    def put(self, a):
        return torch.tensor(a, dtype=torch.float64, device="cuda")

    def addr(self, tensor):
        return None if tensor is None else tensor.data_ptr()

    def get(self, tensor):
        return tensor.cpu().numpy()


pr = t.problem_of(sys.argv[2])
os.environ.update(pr["env"])
t.every_entry(pr, Dev())
print("device arrays ok")
"""


@pytest.mark.parametrize("name", ALL)
def test_device_arrays_have_the_bits_of_the_host_entries(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, root, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0 and "device arrays ok" in p.stdout, p.stderr[-3000:]


# ---------------------------------------------------------------------------------- 5. refusals --
def test_what_the_entries_refuse():
    pr = problem_of("poisson32")
    b = pr["b"]
    x = np.zeros(b.size)
    fake = b.ctypes.data                                # (an address the refusing entries never follow)
    with open_lists(pr, dtype="mixed") as h:
        refused = {"omg_vcycle": lambda: h.vcycle(b, x, 1, 1),
                   "omg_vcycle_ex": lambda: h.vcycle_ex(b, None, x, None, 1, 1),
                   "omg_vcycle_dev": lambda: h.vcycle_dev(fake, None, fake, None, 1, 1),
                   "omg_solve": lambda: h.solve(b, x, 1, 1, 2, 0.0),
                   "omg_hierarchy_cycle_dev": lambda: h.cycle_dev(fake, fake, 1, 1)}
        for entry, call in refused.items():
            with pytest.raises(_hip.HipError) as e:
                call()
            assert e.value.code == _hip.ERR_UNSUPPORTED and (" " + entry + ": ") in str(e.value), (entry, str(e.value))
    for dtype in ("float64", "mixed"):
        with open_lists(pr, dtype=dtype) as h:
            for call in (lambda: h.resident_cycle(1, 1), lambda: h.resident_cycles(1, 1, 2), h.resident_fetch,
                         lambda: h.resident_fetch_dev(fake), lambda: h.resident_pcg(1, 1, 2), h.resident_norms):
                with pytest.raises(_hip.HipError) as e:
                    call()
                assert e.value.code == _hip.ERR_INVALID, (dtype, str(e.value))
    with open_lists(problem_of("single")) as h:
        h.resident_load(problem_of("single")["b"])
        with pytest.raises(_hip.HipError) as e:
            h.resident_pcg(1, 1, 2)
        assert e.value.code == _hip.ERR_INVALID
