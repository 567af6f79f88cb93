"""The 7-point operator of a coefficient field, assembled in HBM (csrc/kappa.hip), and the routes built on it:
omg_kappa_assemble against the SciPy definition operators.stencil7_kappa, Hierarchy.from_kappa / update_kappa against
from_fine / update_fine of that definition, Solver.from_kappa / update_kappa against Solver(A) / update(A).  Every
comparison is bit for bit and with the existing routes, never with the code under test.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import kappa_cases as kc
from kappa_gpu import DeviceArray, flags, params, run, run_pcg, same, same_solve, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- assembly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wname,skind,scale", kc.assembly_cases())
def test_assembly_is_the_scipy_definition_bit_for_bit(shape, wname, skind, scale):
    want = kc.definition(shape, wname, skind, scale)
    kappa, sigma = kc.kappa_of(shape), kc.sigma_of(skind, shape)
    n, nnz = want.shape[0], want.nnz

    def check(indptr, indices, data, where):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
        assert np.array_equal(indptr, want.indptr), where
        assert np.array_equal(indices, want.indices), where
        assert np.array_equal(data, want.data), where              # (bit for bit: no NaN, no -0.0 in the definition)
        assert not np.signbit(data[data == 0.0]).any()
    # host arrays in, host arrays out; the values alone
    check(*_hip.kappa_assemble(kappa, kc.WALLS[wname], sigma, scale), "host")
    none_p, none_i, data = _hip.kappa_assemble(kappa, kc.WALLS[wname], sigma, scale, pattern=False)
    assert none_p is None and none_i is None and np.array_equal(data, want.data)
    # device arrays in, device arrays out (poisoned first: every entry is written)
    d_kappa = DeviceArray(kappa)
    d_sigma = DeviceArray(sigma) if skind == "field" else sigma
    out = (DeviceArray(np.full(n + 1, -7, dtype=np.int32)), DeviceArray(np.full(nnz, -7, dtype=np.int32)), DeviceArray(np.full(nnz, np.nan)))
    got = _hip.kappa_assemble(d_kappa, kc.WALLS[wname], d_sigma, scale, out=out)
    assert got is out
    check(out[0].numpy(), out[1].numpy(), out[2].numpy(), "device")
    # device in, host out; host in, device values alone
    check(*_hip.kappa_assemble(d_kappa, kc.WALLS[wname], d_sigma, scale), "device in, host out")
    only = DeviceArray(np.full(nnz, np.nan))
    _hip.kappa_assemble(kappa, kc.WALLS[wname], sigma, scale, out=(None, None, only))
    assert np.array_equal(only.numpy(), want.data)


def test_both_store_paths_write_the_same_array():
    # OMG_KAPPA_STAGE is read once per process: the other path in a child
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, kappa_cases as kc\nfrom openmg_amd import _hip\n"
            "for shape in kc.SHAPES:\n"
            "    want = kc.definition(shape, 'mixed', 'field', (4.0, 1.0, 0.25))\n"
            "    p, i, d = _hip.kappa_assemble(kc.kappa_of(shape), kc.WALLS['mixed'], kc.sigma_of('field', shape), (4.0, 1.0, 0.25))\n"
            "    assert np.array_equal(d, want.data) and np.array_equal(p, want.indptr) and np.array_equal(i, want.indices)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    for stage in ("0", "1"):
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMG_KAPPA_STAGE=stage), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-4000:]


# ---- refusal --------------------------------------------------------------------------------------------------------------
def test_a_bad_value_is_refused_naming_the_first_cell_and_the_next_call_works():
    shape = (5, 7, 9)
    kappa, sigma = kc.kappa_of(shape), kc.sigma_of("field", shape)
    want = kc.definition(shape, "dirichlet", "field")

    def refused(k, s, text, walls=None):
        with pytest.raises(_hip.HipError) as e:
            _hip.kappa_assemble(k, walls, s)
        assert e.value.code == _hip.ERR_INVALID and text in str(e.value), str(e.value)
        p, i, d = _hip.kappa_assemble(kappa, None, sigma)            # the same process, the next call
        assert np.array_equal(d, want.data)
    for value in (np.nan, 0.0, -2.0, np.inf):
        k = kappa.copy()
        k[3, 2, 5] = value                                           # cell (2, 1, 4)
        k[4, 1, 1] = value                                           # a later cell: the first one is named
        refused(k, sigma, "kappa at cell (2, 1, 4)")
    k = kappa.copy()
    k[0, 3, 3] = np.nan                                              # the ghost cell behind -z of cell (0, 2, 2)
    refused(k, sigma, "kappa at cell (-1, 2, 2)")
    k[2, 3, 10] = 0.0                                                # ... and one behind +x, later in the field
    refused(k, sigma, "kappa at cell (-1, 2, 2)")
    # behind a Neumann wall nothing is read: the same field assembles, as the definition does
    walls = ("neumann",) + ("dirichlet",) * 5
    k = kappa.copy()
    k[0, 3, 3] = np.nan
    k[0, 0, 0] = -1.0                                                # (a corner ghost cell: no face reads it)
    p, i, d = _hip.kappa_assemble(k, walls, sigma)
    assert np.array_equal(d, operators.stencil7_kappa(k, walls, sigma).data)
    s = sigma.copy()
    s[1, 0, 8] = -0.25
    s[4, 6, 8] = np.nan
    refused(kappa, s, "sigma at cell (1, 0, 8)")
    k = kappa.copy()
    k[2, 1, 9] = np.nan                                              # cell (1, 0, 8): kappa before sigma in the same cell
    refused(k, s, "kappa at cell (1, 0, 8)")
    refused(DeviceArray(kappa), DeviceArray(s), "sigma at cell (1, 0, 8)")


# ---- creation and update ----------------------------------------------------------------------------------------------------
VAR7 = [((16, 16, 16), 3, ["var7", "host"]), ((32, 32, 32), 4, ["var7", "var7", "host"])]
SETTINGS = [("dirichlet", "none", (1.0, 1.0, 1.0)), ("mixed", "field", (4.0, 1.0, 0.25))]


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("wname,skind,scale", SETTINGS)
@pytest.mark.parametrize("shape,grids,kinds", VAR7)
def test_from_kappa_and_update_kappa_against_from_fine_and_update_fine(monkeypatch, shape, grids, kinds, wname, skind, scale, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")               # (by default only levels of 128^3 and more take the var7 passes)
    walls, sigma = kc.WALLS[wname], kc.sigma_of(skind, shape)
    k1, k2 = kc.kappa_of(shape, seed=11), kc.kappa_of(shape, seed=21)
    A1, A2 = kc.definition(shape, wname, skind, scale, 11), kc.definition(shape, wname, skind, scale, 21)
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour", dtype=dtype) as ref, \
            _hip.Hierarchy.from_kappa(k1, grids - 1, walls, sigma, scale, smoother="colour", dtype=dtype) as h:
        assert flags(h) == flags(ref)
        assert ["var7" if f["var7"] else "host" for f in flags(h)] == kinds
        assert h.can_update_fine() and ref.can_update_fine()
        assert h.sizes == ref.sizes and h.device_dtype() == ref.device_dtype()
        first = go(ref, b, x0, 5)
        assert same(go(h, b, x0, 5), first)
        # update: against a fresh from_kappa of the new field and against update_fine of the definition's values
        h.update_kappa(k2, walls, sigma, scale)
        ref.update_fine(A2.data)
        second = go(ref, b, x0, 5)
        assert not np.array_equal(second[1], first[1])
        assert same(go(h, b, x0, 5), second)
        with _hip.Hierarchy.from_kappa(k2, grids - 1, walls, sigma, scale, smoother="colour", dtype=dtype) as fresh:
            assert flags(fresh) == flags(ref)
            assert same(go(fresh, b, x0, 5), second)
        # back again (the value array of the hierarchy is reused), the resident b and x stay across an update
        h.resident_load(b, x0)
        h.update_kappa(k1, walls, sigma, scale)
        ref.resident_load(b, x0)
        ref.update_fine(A1.data)
        assert np.array_equal(h.resident_fetch(), ref.resident_fetch())
        assert h.resident_cycle(1, 1) == ref.resident_cycle(1, 1)
        assert same(go(h, b, x0, 5), first)
        # a refused field leaves the hierarchy as it is; so does a field of another grid
        bad = k2.copy()
        bad[5, 5, 5] = np.nan
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(bad, walls, sigma, scale)
        assert e.value.code == _hip.ERR_INVALID and "kappa at cell (4, 4, 4)" in str(e.value)
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(kc.kappa_of((8, 8, 8)), walls, None, scale)
        assert e.value.code == _hip.ERR_INVALID
        assert same(go(h, b, x0, 5), first)


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
def test_constant_kappa_gives_the_plane_hierarchy_and_update_kappa_refuses_it(dtype):
    shape, grids = (16, 16, 16), 3
    kappa = np.full((18, 18, 18), 1.5)
    A = operators.stencil7_kappa(kappa)
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy.from_fine(A, shape, grids - 1, "colour", dtype=dtype) as ref, \
            _hip.Hierarchy.from_kappa(kappa, grids - 1, smoother="colour", dtype=dtype) as h:
        assert flags(h) == flags(ref) and all(f["plane"] for f in flags(h))
        assert h.can_update_fine() == ref.can_update_fine() and not h.can_update_fine()
        want = go(ref, b, x0, 5)
        assert same(go(h, b, x0, 5), want)
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(kc.kappa_of(shape))
        assert e.value.code == _hip.ERR_INVALID
        assert same(go(h, b, x0, 5), want)                               # still cycles as before


def test_a_hierarchy_made_from_lists_is_refused_by_update_kappa():
    shape = (8, 8, 8)
    A0 = kc.definition(shape)
    R = operators.restrictionList(shape, 1, 8)
    A = operators.coeffecientList(A0, R)
    with _hip.Hierarchy(A, R, smoother="colour") as h:
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(kc.kappa_of(shape))
        assert e.value.code == _hip.ERR_INVALID


# ---- Solver ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", [{}, {"accel": "cg"}, {"cycle": "F", "overCorrection": 1.8}, {"dtype": "mixed", "accel": "cg"}],
                         ids=["plain", "cg", "F-1.8", "mixed-cg"])
def test_solver_from_kappa_and_three_time_steps(monkeypatch, more):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (16, 16, 16), 3
    walls, scale = kc.WALLS["mixed"], (4.0, 1.0, 0.25)
    sigma = kc.sigma_of("field", shape)
    b = kc.rhs_of(shape)[0]
    p = params(shape, grids, 6, **more)
    fields = [kc.kappa_of(shape, seed=30 + step) for step in range(4)]
    matrices = [operators.stencil7_kappa(k, walls, sigma, scale) for k in fields]
    with openmg_amd.Solver(matrices[0], p) as ref, openmg_amd.Solver.from_kappa(fields[0], p, walls, sigma, scale) as s:
        assert s.A is None and s.R is None and s.parameters["problemShape"] == shape
        assert s.hierarchy.can_update_fine() and flags(s.hierarchy) == flags(ref.hierarchy) and s.hierarchy.level_flags(0)["var7"]
        assert same_solve(s.solve(b), ref.solve(b))
        for step in (1, 2, 3):
            s.update_kappa(fields[step], sigma=sigma)
            ref.update(matrices[step])
            assert same_solve(s.solve(b), ref.solve(b)), step
        # the solver keeps working with update(A_new): the host pattern is formed on this first call
        s.update(matrices[0])
        ref.update(matrices[0])
        assert same_solve(s.solve(b), ref.solve(b))
        with pytest.raises(ValueError):
            s.update(operators.stencil27_variable(shape))
        with pytest.raises(ValueError):
            s.update_kappa(kc.kappa_of((8, 8, 8)))
        with pytest.raises(ValueError):
            ref.update_kappa(fields[1])                               # (not made by from_kappa)


def test_solver_from_kappa_on_the_singular_all_neumann_operator(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (16, 16, 16), 3
    kappa, walls = kc.kappa_of(shape, seed=40), kc.WALLS["neumann"]
    A = operators.stencil7_kappa(kappa, walls)                        # sigma = 0: the constants are its null space
    b = kc.rhs_of(shape)[0]
    b -= b.mean()
    for more in ({}, {"accel": "cg"}):
        p = params(shape, grids, 6, nullspace="constant", **more)
        with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls) as s:
            got, want = s.solve(b), ref.solve(b)
            assert same_solve(got, want) and abs(got[0].mean()) < 1e-10 * np.abs(got[0]).max()


@pytest.mark.parametrize("more", [{"smoother": "line"}, {"oddExtents": "merge"}, {"giveInfo": True}, {"coarsening": "auto"}],
                         ids=["line", "merge", "giveInfo", "semi"])
def test_solver_from_kappa_with_parameters_of_the_ordinary_route(more):
    shape = (10, 10, 10)
    walls, scale, sigma = kc.WALLS["mixed"], (4.0, 1.0, 0.25), 0.375
    kappa, kappa2 = kc.kappa_of(shape, seed=50), kc.kappa_of(shape, seed=51)
    A, A2 = operators.stencil7_kappa(kappa, walls, sigma, scale), operators.stencil7_kappa(kappa2, walls, sigma, scale)
    b = kc.rhs_of(shape)[0]
    p = params(shape, 2, 6, **more)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls, sigma, scale) as s:
        assert not s.hierarchy.can_update_fine()
        assert same_solve(s.solve(b), ref.solve(b))
        s.update_kappa(kappa2, sigma=sigma)                           # (a new hierarchy, as Solver.update builds one)
        ref.update(A2)
        assert same_solve(s.solve(b), ref.solve(b))
        s.update(A)
        ref.update(A)
        assert same_solve(s.solve(b), ref.solve(b))


# ---- device arrays ----------------------------------------------------------------------------------------------------------
# (PyTorch-ROCm brings its own copy of the HIP runtime and must initialise it before this package's library touches the GPU:
# a process of its own, as tests/devarray_worker.py does)
DEVICE_ARRAYS = """
import os
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import openmg_amd
from openmg_amd import _hip, operators
import kappa_cases as kc

shape, grids = (16, 16, 16), 3
walls, scale = kc.WALLS["mixed"], (4.0, 1.0, 0.25)
sigma = kc.sigma_of("field", shape)
k1, k2 = kc.kappa_of(shape, seed=11), kc.kappa_of(shape, seed=21)
d1, d2, ds = torch.from_numpy(k1).cuda(), torch.from_numpy(k2).cuda(), torch.from_numpy(sigma).cuda()
b, x0 = kc.rhs_of(shape)

def run(h):
    h.resident_load(b, x0)
    return [h.resident_cycle(1, 1) for _ in range(5)], h.resident_fetch()

def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])

# the assembly itself, into tensors
A = kc.definition(shape, "mixed", "field", scale)
out = (torch.full((A.shape[0] + 1,), -7, dtype=torch.int32, device="cuda"), torch.full((A.nnz,), -7, dtype=torch.int32, device="cuda"),
       torch.full((A.nnz,), float("nan"), dtype=torch.float64, device="cuda"))
_hip.kappa_assemble(d1, walls, ds, scale, out=out)
torch.cuda.synchronize()
assert np.array_equal(out[0].cpu().numpy(), A.indptr) and np.array_equal(out[1].cpu().numpy(), A.indices)
assert np.array_equal(out[2].cpu().numpy(), A.data)
for bad in (d1.float(), d1[:, :, 1:], d1.reshape(-1)):
    try:
        _hip.kappa_assemble(bad, walls, ds, scale)
    except (TypeError, ValueError):
        continue
    raise AssertionError("expected a refusal")

with _hip.Hierarchy.from_kappa(k1, grids - 1, walls, sigma, scale, smoother="colour") as host, \\
        _hip.Hierarchy.from_kappa(d1, grids - 1, walls, ds, scale, smoother="colour") as dev:
    assert dev.can_update_fine() and dev.level_flags(0)["var7"]
    assert same(run(dev), run(host))
    host.update_kappa(k2, walls, sigma, scale)
    dev.update_kappa(d2, walls, ds, scale)
    assert same(run(dev), run(host))

p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "cycles": 5,
     "threshold": 0.0, "minSize": 8, "accel": "cg"}
bd = torch.from_numpy(b).cuda()
with openmg_amd.Solver.from_kappa(k1, p, walls, sigma, scale) as host, openmg_amd.Solver.from_kappa(d1, p, walls, ds, scale) as dev:
    u, info = dev.solve(bd)
    uh, infoh = host.solve(b)
    assert u.is_cuda and np.array_equal(u.cpu().numpy(), uh) and info["norms"] == infoh["norms"]
    for kh, kd in ((k2, d2), (k1, d1)):
        host.update_kappa(kh, sigma=sigma)
        dev.update_kappa(kd * 1.0, sigma=ds)               # (a tensor made by a kernel still in flight on torch's stream)
        u, info = dev.solve(bd)
        uh, infoh = host.solve(b)
        assert np.array_equal(u.cpu().numpy(), uh) and info["norms"] == infoh["norms"]
print("ok")
"""


def test_device_arrays_give_the_bits_of_the_host_array_calls():
    p = subprocess.run([sys.executable, "-c", DEVICE_ARRAYS, ROOT], env=dict(os.environ, OMG_VAR7_MIN="4096"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-4000:]
