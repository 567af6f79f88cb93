"""The 7-point operator of a coefficient field on a stretched tensor-product grid, assembled in HBM (csrc/kappa.hip, the
SPACED kernels), and the routes built on it: omg_kappa_assemble_spaced against the SciPy definition
operators.stencil7_kappa(..., spacing=...), Hierarchy.from_kappa / update_kappa against from_fine / update_fine of that
definition, Solver.from_kappa / update_kappa against Solver(A) / update(A).  Every comparison is bit for bit and with an
existing route fed the host definition's matrix, never with the code under test.  Needs an MI355X: run with -m gpu."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import openmg_amd
from openmg_amd import _hip, operators

import kappa_cases as kc
import stretched_cases as sc
from kappa_gpu import DeviceArray, flags, params, run, run_pcg, same, same_solve, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- assembly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wname,skind,zero", sc.assembly_cases())
def test_assembly_is_the_scipy_definition_bit_for_bit(shape, wname, skind, zero):
    want = sc.definition(shape, wname, skind, zero)
    kappa, sigma, sp = kc.kappa_of(shape), kc.sigma_of(skind, shape), sc.widths_of(shape, zero=zero)
    walls = kc.WALLS[wname]
    n, nnz = want.shape[0], want.nnz

    def check(indptr, indices, data, where):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float64
        assert np.array_equal(indptr, want.indptr), where
        assert np.array_equal(indices, want.indices), where
        assert np.array_equal(data, want.data), where              # (bit for bit: no NaN, no -0.0 in the definition)
        assert not np.signbit(data[data == 0.0]).any()
    # host arrays in, host arrays out; the values alone
    check(*_hip.kappa_assemble(kappa, walls, sigma, spacing=sp), "host")
    none_p, none_i, data = _hip.kappa_assemble(kappa, walls, sigma, pattern=False, spacing=sp)
    assert none_p is None and none_i is None and np.array_equal(data, want.data)
    # device arrays in, device arrays out (poisoned first: every entry is written); the widths stay host arrays
    d_kappa = DeviceArray(kappa)
    d_sigma = DeviceArray(sigma) if skind == "field" else sigma
    out = (DeviceArray(np.full(n + 1, -7, dtype=np.int32)), DeviceArray(np.full(nnz, -7, dtype=np.int32)), DeviceArray(np.full(nnz, np.nan)))
    got = _hip.kappa_assemble(d_kappa, walls, d_sigma, out=out, spacing=sp)
    assert got is out
    check(out[0].numpy(), out[1].numpy(), out[2].numpy(), "device")
    # device in, host out; host in, device values alone
    check(*_hip.kappa_assemble(d_kappa, walls, d_sigma, spacing=sp), "device in, host out")
    only = DeviceArray(np.full(nnz, np.nan))
    _hip.kappa_assemble(kappa, walls, sigma, out=(None, None, only), spacing=sp)
    assert np.array_equal(only.numpy(), want.data)
    # without widths the same call still gives the operator without them
    plain = _hip.kappa_assemble(kappa, walls, sigma, pattern=False)[2]
    assert np.array_equal(plain, kc.definition(shape, wname, skind).data)


STORE_PATHS = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
               "import numpy as np, kappa_cases as kc, stretched_cases as sc\nfrom openmg_amd import _hip\n"
               "for shape in [(4, 4, 4), (5, 7, 9), (2, 3, 70), (16, 16, 16)]:\n"
               "    for zero in (False, True):\n"
               "        want = sc.definition(shape, 'mixed', 'field', zero)\n"
               "        p, i, d = _hip.kappa_assemble(kc.kappa_of(shape), kc.WALLS['mixed'], kc.sigma_of('field', shape),\n"
               "                                      spacing=sc.widths_of(shape, zero=zero))\n"
               "        assert np.array_equal(d, want.data) and np.array_equal(p, want.indptr) and np.array_equal(i, want.indices)\n"
               "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("env", [{"OMG_KAPPA_STAGE": "0"}, {"OMG_KAPPA_STAGE": "1"}, {"OMG_POISON": "1"}], ids=["straight", "staged", "poison"])
def test_both_store_paths_write_the_same_array_and_read_nothing_unwritten(env):
    # OMG_KAPPA_STAGE and OMG_POISON are read once per process: a child each
    p = subprocess.run([sys.executable, "-c", STORE_PATHS], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-4000:]


# ---- validity -------------------------------------------------------------------------------------------------------------
def test_bad_values_and_bad_widths_are_refused_and_the_next_call_works():
    shape = (5, 7, 9)
    kappa, sigma, sp = kc.kappa_of(shape), kc.sigma_of("field", shape), sc.widths_of(shape, zero=True)
    want = sc.definition(shape, "dirichlet", "field", True)

    def works():
        assert np.array_equal(_hip.kappa_assemble(kappa, None, sigma, spacing=sp)[2], want.data)       # the same process, the next call

    def refused(k, text):
        with pytest.raises(_hip.HipError) as e:
            _hip.kappa_assemble(k, None, sigma, spacing=sp)
        assert e.value.code == _hip.ERR_INVALID and text in str(e.value), str(e.value)
        works()
    k = kappa.copy()
    k[3, 2, 5] = np.nan                                              # cell (2, 1, 4)
    k[4, 1, 1] = np.nan                                              # a later cell: the first one is named
    refused(k, "kappa at cell (2, 1, 4)")
    k = kappa.copy()
    k[0, 3, 3] = np.nan                                              # the ghost cell behind the Dirichlet wall -z of cell (0, 2, 2)
    refused(k, "kappa at cell (-1, 2, 2)")
    k = kappa.copy()
    k[6, 3, 3] = np.nan                                              # ... and behind +z, where the ghost width is 0
    refused(k, "kappa at cell (5, 2, 2)")
    # behind a Neumann wall neither the ghost kappa nor the ghost width is read
    walls = ("neumann",) + ("dirichlet",) * 5
    k = kappa.copy()
    k[0, 3, 3] = np.nan
    assert np.array_equal(_hip.kappa_assemble(k, walls, sigma, spacing=sp)[2], operators.stencil7_kappa(k, walls, sigma, spacing=sp).data)

    # a bad width straight to the C entry (the Python entries refuse it themselves): named by axis and index
    lib = _hip.lib()
    grid = (ctypes.c_int64 * 3)(*shape)
    data = np.empty(want.nnz)

    def c_entry(widths, scale=None):
        hz, hy, hx = (None if w is None else np.ascontiguousarray(w, dtype=np.float64) for w in widths)
        ptr = [None if w is None else ctypes.c_void_p(w.ctypes.data) for w in (hz, hy, hx)]
        return lib.omg_kappa_assemble_spaced(grid, ctypes.c_void_p(kappa.ctypes.data), 0, None, ctypes.c_void_p(sigma.ctypes.data), _hip.SIGMA_FIELD, 0,
                                             None if scale is None else (ctypes.c_double * 3)(*scale), ptr[0], ptr[1], ptr[2], None, None,
                                             ctypes.c_void_p(data.ctypes.data), 0)

    def put(axis, index, value):
        w = [h.copy() for h in sp]
        w[axis][index] = value
        return w
    for widths, text in ((put(0, 3, np.nan), "along z at index 2"), (put(1, 1, 0.0), "along y at index 0"), (put(2, 9, -1.0), "along x at index 8"),
                         (put(2, 10, np.inf), "along x at index 9"), (put(0, 0, -0.5), "along z at index -1"), (put(1, 8, np.nan), "along y at index 7")):
        assert c_entry(widths) == _hip.ERR_INVALID
        assert text in lib.omg_last_error().decode(), lib.omg_last_error()
        works()
    assert c_entry((sp[0], None, sp[2])) == _hip.ERR_INVALID         # some but not all
    assert c_entry(sp, scale=(4.0, 1.0, 0.25)) == _hip.ERR_INVALID   # widths and a scale
    assert c_entry(sp, scale=(1.0, 1.0, 1.0)) == 0 and np.array_equal(data, want.data)
    assert c_entry(sp) == 0 and np.array_equal(data, want.data)
    assert c_entry((None, None, None), scale=(4.0, 1.0, 0.25)) == 0  # all NULL: the entry without widths
    assert np.array_equal(data, kc.definition(shape, "dirichlet", "field", (4.0, 1.0, 0.25)).data)


# ---- creation and update ----------------------------------------------------------------------------------------------------
VAR7 = [((16, 16, 16), 3, ["var7", "host"]), ((32, 32, 32), 4, ["var7", "var7", "host"])]
SETTINGS = [("dirichlet", "none", False), ("mixed", "field", True)]


@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("wname,skind,zero", SETTINGS)
@pytest.mark.parametrize("shape,grids,kinds", VAR7)
def test_from_kappa_and_update_kappa_against_from_fine_and_update_fine(monkeypatch, shape, grids, kinds, wname, skind, zero, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")               # (by default only levels of 128^3 and more take the var7 passes)
    walls, sigma, sp = kc.WALLS[wname], kc.sigma_of(skind, shape), sc.widths_of(shape, zero=zero)
    k1, k2 = kc.kappa_of(shape, seed=11), kc.kappa_of(shape, seed=21)
    A1, A2 = operators.stencil7_kappa(k1, walls, sigma, spacing=sp), operators.stencil7_kappa(k2, walls, sigma, spacing=sp)
    b, x0 = vectors(shape, dtype)
    go = run_pcg if dtype == "mixed" else run
    with _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour", dtype=dtype) as ref, \
            _hip.Hierarchy.from_kappa(k1, grids - 1, walls, sigma, smoother="colour", dtype=dtype, spacing=sp) as h:
        assert flags(h) == flags(ref)
        assert ["var7" if f["var7"] else "host" for f in flags(h)] == kinds
        assert h.can_update_fine() and ref.can_update_fine()
        assert h.sizes == ref.sizes and h.device_dtype() == ref.device_dtype()
        first = go(ref, b, x0, 5)
        assert same(go(h, b, x0, 5), first)
        # update: against update_fine of the definition's values
        h.update_kappa(k2, walls, sigma, spacing=sp)
        ref.update_fine(A2.data)
        second = go(ref, b, x0, 5)
        assert not np.array_equal(second[1], first[1])
        assert same(go(h, b, x0, 5), second)
        # back again (the value array of the hierarchy is reused), the resident b and x stay across an update
        h.resident_load(b, x0)
        h.update_kappa(k1, walls, sigma, spacing=sp)
        ref.resident_load(b, x0)
        ref.update_fine(A1.data)
        assert np.array_equal(h.resident_fetch(), ref.resident_fetch())
        assert h.resident_cycle(1, 1) == ref.resident_cycle(1, 1)
        assert same(go(h, b, x0, 5), first)
        # a refused field leaves the hierarchy as it is
        bad = k2.copy()
        bad[5, 5, 5] = np.nan
        with pytest.raises(_hip.HipError) as e:
            h.update_kappa(bad, walls, sigma, spacing=sp)
        assert e.value.code == _hip.ERR_INVALID and "kappa at cell (4, 4, 4)" in str(e.value)
        assert same(go(h, b, x0, 5), first)


# ---- Solver ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", [{}, {"accel": "cg"}, {"cycle": "F", "overCorrection": 1.8}, {"dtype": "mixed", "accel": "cg"}],
                         ids=["plain", "cg", "F-1.8", "mixed-cg"])
def test_solver_from_kappa_and_three_time_steps(monkeypatch, more):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (16, 16, 16), 3
    walls, sp = kc.WALLS["mixed"], sc.widths_of(shape, zero=True)
    sigma = kc.sigma_of("field", shape)
    b = kc.rhs_of(shape)[0]
    p = params(shape, grids, 6, **more)
    fields = [kc.kappa_of(shape, seed=30 + step) for step in range(4)]
    matrices = [operators.stencil7_kappa(k, walls, sigma, spacing=sp) for k in fields]
    with openmg_amd.Solver(matrices[0], p) as ref, openmg_amd.Solver.from_kappa(fields[0], p, walls, sigma, spacing=sp) as s:
        assert s.A is None and s.R is None and s.parameters["problemShape"] == shape
        assert s.hierarchy.can_update_fine() and flags(s.hierarchy) == flags(ref.hierarchy) and s.hierarchy.level_flags(0)["var7"]
        assert same_solve(s.solve(b), ref.solve(b))
        for step in (1, 2, 3):
            s.update_kappa(fields[step], sigma=sigma)                  # (the widths are the solver's)
            ref.update(matrices[step])
            assert same_solve(s.solve(b), ref.solve(b)), step
        s.update(matrices[0])
        ref.update(matrices[0])
        assert same_solve(s.solve(b), ref.solve(b))


def test_solver_from_kappa_on_the_singular_all_neumann_operator(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (16, 16, 16), 3
    kappa, walls, sp = kc.kappa_of(shape, seed=40), kc.WALLS["neumann"], sc.widths_of(shape)
    A = operators.stencil7_kappa(kappa, walls, spacing=sp)           # sigma none: the constants are its null space
    b = kc.rhs_of(shape)[0]
    b -= b.mean()
    for more in ({}, {"accel": "cg"}):
        p = params(shape, grids, 6, nullspace="constant", **more)
        with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls, spacing=sp) as s:
            assert same_solve(s.solve(b), ref.solve(b))


def smooth_kappa(shape, spacing, shift=0.0):
    """1 + 0.5 sin(2 z + y + shift) cos(x) at the cell centres of the grid, the ghost centres mirrored."""
    centres = []
    for h in spacing:
        w = np.concatenate(([h[1]], h[1:-1], [h[-2]]))
        faces = np.concatenate(([0.0], np.cumsum(h[1:-1])))
        centres.append(np.concatenate(([-0.5 * w[0]], 0.5 * (faces[1:] + faces[:-1]), [faces[-1] + 0.5 * w[-1]])))
    Z, Y, X = np.meshgrid(*centres, indexing="ij")
    return 1.0 + 0.5 * np.sin(2.0 * Z + Y + shift) * np.cos(X)


@pytest.mark.parametrize("more", [{"smoother": "line"}, {"coarsening": "auto"}, {"oddExtents": "merge"}, {"giveInfo": True}],
                         ids=["line", "semi", "merge", "giveInfo"])
def test_solver_from_kappa_with_parameters_of_the_ordinary_route(more):
    shape = (10, 10, 10)
    walls, sigma = kc.WALLS["mixed"], 0.375
    sp = sc.boundary_layer_spacing(shape, beta=2.0)                   # thin cells at z = 0: the z couplings are the strong ones
    kappa, kappa2 = smooth_kappa(shape, sp), smooth_kappa(shape, sp, shift=0.7)
    A, A2 = operators.stencil7_kappa(kappa, walls, sigma, spacing=sp), operators.stencil7_kappa(kappa2, walls, sigma, spacing=sp)
    b = kc.rhs_of(shape)[0]
    p = params(shape, 2, 6, **more)
    with openmg_amd.Solver(A, p) as ref, openmg_amd.Solver.from_kappa(kappa, p, walls, sigma, spacing=sp) as s:
        assert not s.hierarchy.can_update_fine()
        got, want = s.solve(b), ref.solve(b)
        assert same_solve(got, want)
        assert s.hierarchy.line_axis == ref.hierarchy.line_axis and got[1].get("lineAxis") == want[1].get("lineAxis")
        assert got[1].get("coarsening") == want[1].get("coarsening")
        if "smoother" in more:
            assert got[1]["lineAxis"] == 0 and s.hierarchy.line_axis == 0          # the z axis, an index into problemShape
        s.update_kappa(kappa2, sigma=sigma)                           # (a new hierarchy, as Solver.update builds one: with the widths)
        ref.update(A2)
        assert same_solve(s.solve(b), ref.solve(b))
        assert s.hierarchy.line_axis == ref.hierarchy.line_axis
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
from openmg_amd import operators
import kappa_cases as kc
import stretched_cases as sc
from kappa_gpu import DeviceArray, flags, params, run, run_pcg, same, same_solve, vectors

shape, grids = (16, 16, 16), 3
walls = kc.WALLS["mixed"]
sp = sc.widths_of(shape, zero=True)
sigma = kc.sigma_of("field", shape)
k1, k2 = kc.kappa_of(shape, seed=11), kc.kappa_of(shape, seed=21)
d1, d2, ds = torch.from_numpy(k1).cuda(), torch.from_numpy(k2).cuda(), torch.from_numpy(sigma).cuda()
b = kc.rhs_of(shape)[0]
bd = torch.from_numpy(b).cuda()

try:
    openmg_amd.Solver.from_kappa(d1, {"gridLevels": grids}, walls, ds, spacing=[torch.from_numpy(h).cuda() for h in sp])
except ValueError as e:
    assert "host" in str(e), e
else:
    raise AssertionError("device widths were taken")

p = {"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour", "cycles": 5,
     "threshold": 0.0, "minSize": 8, "accel": "cg"}
A1 = operators.stencil7_kappa(k1, walls, sigma, spacing=sp)
with openmg_amd.Solver(A1, p) as ref, openmg_amd.Solver.from_kappa(k1, p, walls, sigma, spacing=sp) as host, \\
        openmg_amd.Solver.from_kappa(d1, p, walls, ds, spacing=sp) as dev:
    u, info = dev.solve(bd)
    uh, infoh = host.solve(b)
    ur, infor = ref.solve(b)
    assert u.is_cuda and np.array_equal(u.cpu().numpy(), uh) and info["norms"] == infoh["norms"]
    assert np.array_equal(ur, uh) and infor["norms"] == infoh["norms"]
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
