"""omg_hierarchy_update_fine on a hierarchy of 7-point per-row-coefficient levels (var7, csrc/var7.hip) set up on the
device: every Galerkin product re-formed by the closed-form streaming kernel var7_rap_kernel, the small host-coded levels
below the var7 levels rebuilt from their new products, the coarsest operator factorised anew.  The updated hierarchy must
be the hierarchy a fresh from_fine of the new operator gives: the same norms and iterate bit for bit, cycle after cycle —
which holds only if every product of the chain came out with the bits of the SciPy-order setup kernel."""
import ctypes

import numpy as np
import pytest

from openmg_amd import _hip, operators

pytestmark = pytest.mark.gpu


def run(h, b, x0, pre, post, cycles):
    h.resident_load(b, x0)
    return [h.resident_cycle(pre, post) for _ in range(cycles)], h.resident_fetch()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


def problem(shape, dtype, seed=3):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    if dtype == "float32":
        b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
    return b, x0


class DeviceValues:
    """A CSR value array copied to HBM (hipMalloc / hipFree through the HIP runtime)."""

    def __init__(self, data):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        data = np.ascontiguousarray(data, dtype=np.float64)
        self.size = data.size
        self.d = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.d), data.nbytes) == 0
        assert self.hip.hipMemcpy(self.d, data.ctypes.data, data.nbytes, 1) == 0

    def __enter__(self):
        return (self.d.value, self.size)

    def __exit__(self, *exc):
        self.hip.hipFree(self.d)


def level_kinds(h, grids):
    kinds = []
    for l in range(grids - 1):
        f = h.level_flags(l)
        assert not f["plane"] and not f["stencil27"]
        kinds.append("var7" if f["var7"] else "host")
    return kinds


CASES = [((16, 16, 16), 3, 4096, ["var7", "host"]),
         ((32, 32, 32), 4, 4096, ["var7", "var7", "host"]),
         ((16, 24, 16), 3, 4096, ["var7", "host"]),
         ((40, 24, 40), 2, 4096, ["var7"]),                           # ragged tiles
         ((64, 64, 64), 4, 32768, ["var7", "var7", "host"])]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,grids,var7_min,kinds", CASES)
def test_updated_hierarchy_is_the_freshly_built_one(monkeypatch, shape, grids, var7_min, kinds, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", str(var7_min))
    A1 = operators.stencil7_variable(shape, seed=1)
    A2 = operators.stencil7_variable(shape, seed=2)
    assert np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices)
    b, x0 = problem(shape, dtype)
    with _hip.Hierarchy.from_fine(A2, shape, grids - 1, "colour", dtype=dtype) as fresh, \
            _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour", dtype=dtype) as h:
        assert level_kinds(h, grids) == kinds and level_kinds(fresh, grids) == kinds
        want = run(fresh, b, x0, 1, 1, 3)
        old = run(h, b, x0, 1, 1, 3)
        assert not np.array_equal(old[1], want[1])
        h.update_fine(A2.data)
        assert same(run(h, b, x0, 1, 1, 3), want), (shape, dtype)
        # the row-kernel schedule of the updated hierarchy is built from the NEW operator too
        h.use_plane(False)
        fresh.use_plane(False)
        assert same(run(h, b, x0, 1, 1, 3), run(fresh, b, x0, 1, 1, 3))
        h.use_plane(True)
        fresh.use_plane(True)
        # back again, from device-resident values; then a third update in a row (the products' arrays are reused)
        with DeviceValues(A1.data) as dv:
            h.update_fine(dv, on_device=True)
        assert same(run(h, b, x0, 1, 1, 3), old)
        h.update_fine(A2.data)
        assert same(run(h, b, x0, 1, 1, 3), want)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_coupling_that_cancels_on_a_host_level(monkeypatch, dtype):
    # level 1 of a 16^3 hierarchy is host-coded; the four fine couplings across the +x face of its aggregate (2, 2, 2) are
    # -1, 1, -1, 1: the Galerkin coupling is ((0 - 1/64) + 1/64 - 1/64) + 1/64 = 0.0 exactly, and SciPy's order drops it
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (16, 16, 16)
    A1 = operators.stencil7_variable(shape, seed=1)
    A2 = operators.stencil7_variable(shape, seed=2)
    data = A2.data.copy()
    for (y, z), v in zip([(4, 4), (5, 4), (4, 5), (5, 5)], [-1.0, 1.0, -1.0, 1.0]):
        row = (z * 16 + y) * 16 + 5
        p = A2.indptr[row] + int(np.flatnonzero(A2.indices[A2.indptr[row]:A2.indptr[row + 1]] == row + 1)[0])
        data[p] = v
    A3 = A2.copy()
    A3.data = data
    b, x0 = problem(shape, dtype)
    with _hip.Hierarchy.from_fine(A3, shape, 2, "colour", dtype=dtype) as fresh, \
            _hip.Hierarchy.from_fine(A2, shape, 2, "colour", dtype=dtype) as plain, \
            _hip.Hierarchy.from_fine(A1, shape, 2, "colour", dtype=dtype) as h:
        assert level_kinds(fresh, 3) == ["var7", "host"]
        assert fresh.format_info(1)["nnz"] == plain.format_info(1)["nnz"] - 1
        want = run(fresh, b, x0, 1, 1, 3)
        h.update_fine(A3.data)
        assert h.format_info(1)["nnz"] == fresh.format_info(1)["nnz"]
        assert same(run(h, b, x0, 1, 1, 3), want)
        h.update_fine(A2.data)                                    # and the entry comes back
        assert h.format_info(1)["nnz"] == plain.format_info(1)["nnz"]
        assert same(run(h, b, x0, 1, 1, 3), run(plain, b, x0, 1, 1, 3))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_other_cycles_cg_and_graphs_after_an_update(monkeypatch, dtype):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape, grids = (32, 32, 32), 4
    A1 = operators.stencil7_variable(shape, seed=1)
    A2 = operators.stencil7_variable(shape, seed=2)
    b, x0 = problem(shape, dtype)
    with _hip.Hierarchy.from_fine(A2, shape, grids - 1, "colour", dtype=dtype) as fresh, \
            _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour", dtype=dtype) as h:
        # a captured cycle and the zero-start first relaxation's diagonal exist before the update: neither may survive it
        h.use_graph(True)
        run(h, b, x0, 1, 1, 2)
        h.use_graph(False)
        h.resident_load(b)
        h.resident_pcg(2, 1, 2)
        h.update_fine(A2.data)
        for pre, post in [(2, 1), (0, 1)]:
            assert same(run(h, b, x0, pre, post, 2), run(fresh, b, x0, pre, post, 2)), (pre, post)
        for pre, post in [(1, 1), (2, 1)]:
            got, want = [], []
            for hh, out in ((h, got), (fresh, want)):
                hh.resident_load(b, x0)
                its, norms, tn, bd = hh.resident_pcg(pre, post, 4)
                out.extend([its, norms, tn, bd, hh.resident_fetch()])
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3]
            assert np.array_equal(got[4], want[4]), (pre, post)
        h.use_graph(True)
        fresh.use_graph(True)
        assert same(run(h, b, x0, 1, 1, 3), run(fresh, b, x0, 1, 1, 3))
        h.use_graph(False)
        fresh.use_graph(False)


def test_update_is_refused_where_it_does_not_apply(monkeypatch):
    monkeypatch.setenv("OMG_VAR7_MIN", "4096")
    shape = (16, 16, 16)
    A1 = operators.stencil7_variable(shape, seed=1)
    A2 = operators.stencil7_variable(shape, seed=2)
    b, x0 = problem(shape, "float64")
    with _hip.Hierarchy.from_fine(A2, shape, 2, "colour") as fresh, _hip.Hierarchy.from_fine(A1, shape, 2, "colour") as h:
        want = run(fresh, b, x0, 1, 1, 3)
        with pytest.raises(_hip.HipError):
            h.update_fine(A2.data[:-1])                           # not the pattern's number of entries
        h.update_fine(A2.data)
        assert same(run(h, b, x0, 1, 1, 3), want)
        bad = A2.data.copy()
        interior = (5 * 16 + 5) * 16 + 5                          # cell (5, 5, 5): all six neighbours, the diagonal is entry 3
        bad[A2.indptr[interior] + 3] = 0.0
        with pytest.raises(_hip.HipError) as e:
            h.update_fine(bad)
        assert e.value.code == _hip.ERR_NO_DIAGONAL
        h.update_fine(A2.data)
        assert same(run(h, b, x0, 1, 1, 3), want)
    # the ordinary route (host-built levels) and the lexicographic smoother: nothing to update in place
    R = [operators.restriction(shape)]
    with _hip.Hierarchy([A1, (R[0] @ A1 @ R[0].T).tocsr()], R, "colour") as h:
        with pytest.raises(_hip.HipError):
            h.update_fine(A2.data)
    with _hip.Hierarchy.from_fine(A1, shape, 2, "gs") as h:
        assert not h.level_flags(0)["var7"]
        with pytest.raises(_hip.HipError):
            h.update_fine(A2.data)


def test_full_size(monkeypatch):
    # the var7 bench leg's hierarchy: 256^3, 5 grids, default thresholds (256^3 and 128^3 var7, 64^3 and 32^3 host-coded)
    monkeypatch.delenv("OMG_VAR7_MIN", raising=False)
    free, _ = _hip.device_mem_info()
    if free < (40 << 30):
        pytest.skip("needs 40 GiB of free device memory")
    shape, grids = (256, 256, 256), 5
    A1 = operators.stencil7_variable(shape, seed=1)
    # new values: the off-diagonal couplings scaled row by row, the diagonal kept (still diagonally dominant)
    rows = np.repeat(np.arange(A1.shape[0]), np.diff(A1.indptr))
    off = A1.indices != rows
    d2 = A1.data.copy()
    d2[off] *= 0.5 + 0.5 * ((rows[off] * 2654435761) % 1024) / 1024.0
    del rows, off
    b, x0 = problem(shape, "float64")
    with _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour") as h:
        assert level_kinds(h, grids) == ["var7", "var7", "host", "host"]
        h.update_fine(d2)
        got = run(h, b, x0, 1, 1, 3)
    A1.data = d2
    with _hip.Hierarchy.from_fine(A1, shape, grids - 1, "colour") as fresh:
        assert same(got, run(fresh, b, x0, 1, 1, 3))
