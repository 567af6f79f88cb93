"""BASELINE configs[4] on slabs (openmg_amd/csrc/dist27.hip): the 27-point octant-layout kernels on a rank's extended
slab — ghost aggregate planes, colours 0 .. 3 of the upper ghost plane relaxed redundantly, one exchange per sweep, the
Galerkin products per rank on the device — as LOOPBACK groups of 1, 2, 4 and 8 slabs on one GPU: the iterate bit for bit
the single-GPU hierarchy's (which runs the same kernels on the whole grid: no OMG_STENCIL27=0), the coarse operators
bit for bit the global products', and against the CPU oracle (openmg/__init__.py:151-236) at BASELINE's 1e-10."""
import numpy as np
import pytest
import scipy.sparse as sp

from openmg_amd import _hip, _hip_dist, dist, operators
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu


def restrictions(shape, grids):
    """operators.restrictionList keeps the reference's index quirk (its second axis strides by shape[0]), which is the plain
    2 x 2 x 2 aggregation of the grid — what the slabs and the 27-point kernels restrict with — only where shape[0] ==
    shape[2]; for the other shapes the same aggregation, weight 1/8, is written down directly."""
    if shape[0] == shape[2]:
        return operators.restrictionList(shape, grids - 2, 1)
    from poison_worker import aggregation
    return [aggregation(tuple(s >> l for s in shape)) for l in range(grids - 1)]


def make_tail(coarse, tshape, n_grids, dtype):
    """dist.make_tail, whose restrictions are operators.restriction's, where those are the plain aggregation; otherwise the
    same hierarchy below the slabs with restrictions()'s"""
    if tshape[0] == tshape[2]:
        return dist.make_tail(coarse, tshape, n_grids, smoother="colour", dtype=dtype)
    R = restrictions(tshape, n_grids)
    return _hip.Hierarchy(operators.coeffecientList(sp.csr_matrix(coarse), R), R, smoother="colour", dtype=dtype)


_OPERATORS = {}


def single_gpu_operators(shape, grids):
    """(the last problem's operators are kept: the pooled cases share their 1 M- and 2 M-row hierarchies)"""
    if (shape, grids) not in _OPERATORS:
        _OPERATORS.clear()
        A0 = operators.stencil27_variable(shape)
        R = restrictions(shape, grids)
        assert len(R) == grids - 1
        _OPERATORS[(shape, grids)] = (operators.coeffecientList(A0, R), R)
    return _OPERATORS[(shape, grids)]


def single_gpu(shape, grids, dtype):
    A, R = single_gpu_operators(shape, grids)
    return A, R, _hip.Hierarchy(A, R, smoother="colour", dtype=dtype)


def slab_group(shape, world, n_levels, grids, dtype, p2p=0):
    plane = shape[1] * shape[2]
    per = shape[0] // world
    ranks = [_hip_dist.Slab27Rank(r, world, shape, dist.stencil27_variable_rows(shape, r * per * plane, (r + 1) * per * plane), n_levels,
                                  dtype=dtype) for r in range(world)]
    coarse = dist.assemble_coarse([r.coarse_rows() for r in ranks])
    tshape = tuple(s >> n_levels for s in shape)
    tails = [make_tail(coarse, tshape, grids - n_levels, dtype) for _ in ranks]
    for r, t in zip(ranks, tails):
        r.set_tail(t)
    return _hip_dist.Slab27Group(ranks, p2p=p2p), tails, coarse


def close(a, b, tol=1e-12):
    return all(abs(u - v) <= tol * abs(v) for u, v in zip(a, b))


# Slabs whose level 0 keeps x, b and tmp in ONE allocation (dist27.hip: nx * ny * (planes per rank + 4) >= 2^20 values)
# above a level that does not; nx = 256 is the widest line the fp64 kernels take.  POOLED: four ranks of four planes, level
# 0 exactly at the threshold, two ranks with a neighbour on both sides; POOLED_SMALL: two ranks, half the rows.
POOLED = ((16, 512, 256), 5, 4, 2)
POOLED_SMALL = ((8, 512, 256), 4, 2, 2)


def assert_pooled(layouts, shape, world, n_levels, dtype):
    """The ranks' p2p_layout(): level 0 really is pooled (x, tmp, b share one allocation), the last level is not, and the
    layout rule holds on every level (tests/test_gpu_plane_dist.py assert_export_layout)."""
    from test_gpu_plane_dist import assert_export_layout
    item = 8 if dtype == "float64" else 4
    nbytes = [item * (shape[1] >> l) * (shape[2] >> l) * ((shape[0] >> l) // world + 4) for l in range(n_levels)]
    pooled = [b // item >= 1 << 20 for b in nbytes]
    assert pooled[0] and not pooled[-1], (nbytes, "the case no longer has a pooled level above an unpooled one")
    assert assert_export_layout(layouts, 1, nbytes, pooled) == 1 + sum(pooled) + 3 * (len(pooled) - sum(pooled))


def slab_problem(shape, world, dtype):
    """b and x0 of the pooled cases from the ranks' own rows (tests/poison_worker.py makes them without the whole operator)"""
    n = int(np.prod(shape))
    per = n // world
    u = np.random.default_rng(11).random(n)
    b = np.concatenate([dist.stencil27_variable_rows(shape, r * per, (r + 1) * per) @ u for r in range(world)])
    x0 = np.random.default_rng(12).standard_normal(n)
    if dtype == "float32":
        b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
    return b, x0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pooled_slab_groups_have_the_bits_of_the_single_gpu_hierarchy(dtype):
    """Four slabs of (16, 512, 256) whose level 0 is pooled, with copies (p2p = 0, the six sweep-count pairs of the first test)
    and with peer stores (p2p = 1, the four of the second): the iterate bit for bit the single-GPU hierarchy's, the norms at
    1e-12 / 1e-6, the layout asserted through p2p_layout().  (MI355X: 7.0 s in fp64, with the operators' construction, 5.0 s in fp32.)"""
    shape, grids, world, n_levels = POOLED
    A, R, h = single_gpu(shape, grids, dtype)
    want = {}
    groups = []
    try:
        assert all(h.level_flags(l)["stencil27"] for l in range(n_levels + 1)), [h.level_flags(l) for l in range(grids - 1)]
        b, x0 = slab_problem(shape, world, dtype)
        per = b.size // world
        for p2p, pairs in ((0, ((1, 1), (1, 0), (2, 1), (0, 1), (0, 0), (2, 2))), (1, ((1, 1), (1, 0), (2, 1), (0, 0)))):
            g, tails, _ = slab_group(shape, world, n_levels, grids, dtype, p2p=p2p)
            groups.append((g, tails))
            assert_pooled([r.p2p_layout() for r in g.ranks], shape, world, n_levels, dtype)
            for pre, post in pairs:
                if (pre, post) not in want:
                    h.resident_load(b, x0)
                    want[(pre, post)] = (h.resident_cycles(pre, post, 3), h.resident_fetch())
                want_norms, want_x = want[(pre, post)]
                for r in g.ranks:
                    r.load(b[r.rank * per:(r.rank + 1) * per], x0[r.rank * per:(r.rank + 1) * per])
                norms = g.cycles(pre, post, 3)
                x = np.concatenate([r.fetch() for r in g.ranks])
                assert np.array_equal(x, want_x), (p2p, dtype, pre, post, int(np.sum(x != want_x)))
                assert close(norms, want_norms, 1e-12 if dtype == "float64" else 1e-6), (p2p, pre, post, norms, want_norms)
                assert g.ranks[1].info()["exchanges_last_call"] == 3 * ((pre + post) + (n_levels - 1) * (1 + pre + post))
            groups.pop()
            g.close()
            for t in tails:
                t.close()
    finally:
        for g, tails in groups:
            g.close()
            for t in tails:
                t.close()
        h.close()


def test_pooled_peer_store_slabs_against_the_oracle_and_without_the_pool(tmp_path):
    """Two slabs of (8, 512, 256), 4 grids, fp64, level 0 pooled, peer stores: every cycle's norm within BASELINE's 1e-10 of
    the CPU oracle's for V(1,1) (the oracle's greedy colouring of 1 M rows is most of this test's time) — the chain pooled slabs -> single-GPU hierarchy -> oracle closed at this size —,
    the bits of the single-GPU hierarchy, and the same bits from a process with OMG_VEC_POOL=0 (three allocations per level
    against one; the switch is read once per process).  (MI355X: 9.5 s; the norms agree with the oracle's to 8e-16, 2e-15 and 3e-15.)"""
    import json
    from test_gpu_poison import slab27_in_a_process_of_its_own
    shape, grids, world, n_levels = POOLED_SMALL
    A, R, h = single_gpu(shape, grids, "float64")
    g, tails, _ = slab_group(shape, world, n_levels, grids, "float64", p2p=1)
    try:
        assert all(h.level_flags(l)["stencil27"] for l in range(n_levels + 1)), [h.level_flags(l) for l in range(grids - 1)]
        assert_pooled([r.p2p_layout() for r in g.ranks], shape, world, n_levels, "float64")
        b, x0 = slab_problem(shape, world, "float64")
        per = b.size // world
        got = {}
        norms = []
        for pre, post in ((1, 1), (1, 0), (2, 1)):
            h.resident_load(b, x0)
            want_norms = h.resident_cycles(pre, post, 3)
            want_x = h.resident_fetch()
            for r in g.ranks:
                r.load(b[r.rank * per:(r.rank + 1) * per], x0[r.rank * per:(r.rank + 1) * per])
            norms += g.cycles(pre, post, 3)
            got["x%d%d" % (pre, post)] = np.concatenate([r.fetch() for r in g.ranks])
            assert np.array_equal(got["x%d%d" % (pre, post)], want_x), (pre, post)
            assert close(norms[-3:], want_norms, 1e-12), (pre, post, norms[-3:], want_norms)
        # three allocations per level: the same bits
        apart = slab27_in_a_process_of_its_own(tmp_path / "apart.npz", shape, world, n_levels, grids, "float64", 1, OMG_VEC_POOL="0")
        lay = json.loads(str(apart["layouts"]))
        assert all(len({t["alloc"] for t in rank["buffers"][1:4]}) == 3 and all(t["base_delta"] == 0 for t in rank["buffers"]) for rank in lay), lay
        for key, x in got.items():
            assert np.array_equal(apart[key], x), (key, int(np.sum(apart[key] != x)))
        assert np.array_equal(apart["norms"], np.array(norms))
        # the oracle, from a zero start as test_eight_slabs_against_the_oracle
        Ro = R                                               # (the plain aggregation, as the slabs have it: restrictions())
        Ao = orc.coefficient_list(A[0], Ro)
        sm = orc.make_smoother("colour", Ao)
        for pre, post in ((1, 1),):
            for r in g.ranks:
                r.load(b[r.rank * per:(r.rank + 1) * per])
            norms = g.cycles(pre, post, 3)
            p = {"preIterations": pre, "postIterations": post, "coarsestLevel": len(Ro)}
            xo = None
            for k in range(3):
                xo, info = orc.mg_cycle(Ao, b, 0, Ro, p, initial=xo, smoother=sm)
                rel = abs(norms[k] - info["norm"]) / info["norm"]
                print("pooled slabs against the oracle: V(%d,%d) cycle %d norm %.15e oracle %.15e rel %.2e" % (pre, post, k, norms[k], info["norm"], rel))
                assert rel <= 1e-10, (pre, post, k, norms[k], info["norm"])
            x = np.concatenate([r.fetch() for r in g.ranks])
            np.testing.assert_allclose(x, xo, rtol=1e-9, atol=1e-12)
    finally:
        g.close()
        for t in tails:
            t.close()
        h.close()


CASES = [((16, 16, 16), 3, 1, 2), ((16, 16, 16), 3, 2, 2), ((16, 16, 16), 3, 4, 2), ((16, 16, 16), 3, 8, 1),
         ((32, 16, 32), 4, 4, 3), ((32, 16, 32), 4, 8, 2), ((32, 24, 32), 3, 2, 2)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,grids,world,n_levels", CASES)
def test_slab_groups_have_the_bits_of_the_single_gpu_hierarchy(shape, grids, world, n_levels, dtype):
    A, R, h = single_gpu(shape, grids, dtype)
    assert all(h.level_flags(l)["stencil27"] for l in range(grids - 1))
    g, tails, coarse = slab_group(shape, world, n_levels, grids, dtype)
    try:
        # the operator below the slabs, made from the ranks' own rows on the device: the bits of the global product
        want = sp.csr_matrix(A[n_levels])
        want.sort_indices()
        got = sp.csr_matrix(coarse)
        got.sort_indices()
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data, want.data)
        rng = np.random.default_rng(11)
        b = A[0] @ rng.random(A[0].shape[0])
        x0 = rng.standard_normal(A[0].shape[0])
        if dtype == "float32":
            b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
        per = b.size // world
        for pre, post in ((1, 1), (1, 0), (2, 1), (0, 1), (0, 0), (2, 2)):
            h.resident_load(b, x0)
            want_norms = h.resident_cycles(pre, post, 3)
            want_x = h.resident_fetch()
            for r in g.ranks:
                r.load(b[r.rank * per:(r.rank + 1) * per], x0[r.rank * per:(r.rank + 1) * per])
            norms = g.cycles(pre, post, 3)
            x = np.concatenate([r.fetch() for r in g.ranks])
            assert np.array_equal(x, want_x), (shape, world, dtype, pre, post, int(np.sum(x != want_x)))
            assert close(norms, want_norms, 1e-12 if dtype == "float64" else 1e-6), (pre, post, norms, want_norms)
            if world > 1:
                assert g.ranks[1].info()["exchanges_last_call"] == 3 * ((pre + post) + (n_levels - 1) * (1 + pre + post))
    finally:
        g.close()
        for t in tails:
            t.close()
        h.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,grids,world,n_levels", [((16, 16, 16), 3, 2, 2), ((32, 16, 32), 4, 4, 3), ((32, 16, 32), 4, 8, 2), ((32, 24, 32), 3, 2, 2)])
def test_peer_store_exchanges_have_the_bits_of_the_single_gpu_hierarchy(shape, grids, world, n_levels, dtype):
    """Round 6 ("also give dist27 the peer-store exchange PlaneDist has"): the halo exchanges as stores into
    the neighbours' ghost planes ordered by flags — permission, push, landed — instead of copies / grouped send-recv; the
    same planes, the same bits, the same number of exchanges."""
    A, R, h = single_gpu(shape, grids, dtype)
    g, tails, _ = slab_group(shape, world, n_levels, grids, dtype, p2p=1)
    try:
        rng = np.random.default_rng(11)
        b = A[0] @ rng.random(A[0].shape[0])
        x0 = rng.standard_normal(A[0].shape[0])
        if dtype == "float32":
            b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
        per = b.size // world
        for pre, post in ((1, 1), (1, 0), (2, 1), (0, 0)):
            h.resident_load(b, x0)
            want_norms = h.resident_cycles(pre, post, 3)
            want_x = h.resident_fetch()
            for r in g.ranks:
                r.load(b[r.rank * per:(r.rank + 1) * per], x0[r.rank * per:(r.rank + 1) * per])
            norms = g.cycles(pre, post, 3)
            x = np.concatenate([r.fetch() for r in g.ranks])
            assert np.array_equal(x, want_x), (shape, world, dtype, pre, post, int(np.sum(x != want_x)))
            assert close(norms, want_norms, 1e-12 if dtype == "float64" else 1e-6)
            assert g.ranks[1].info()["exchanges_last_call"] == 3 * ((pre + post) + (n_levels - 1) * (1 + pre + post))
    finally:
        g.close()
        for t in tails:
            t.close()
        h.close()


def test_a_peer_store_wait_gives_up_instead_of_hanging(monkeypatch):
    """A neighbour that never answers (its buffers mapped, peer mode on, but it does not run the cycle): the bounded wait
    (OMG_P2P_SPIN polls) ends, the call raises."""
    monkeypatch.setenv("OMG_P2P_SPIN", "2000")
    shape, world = (16, 16, 16), 2
    plane, per = 256, 8
    ranks = [_hip_dist.Slab27Rank(r, world, shape, dist.stencil27_variable_rows(shape, r * per * plane, (r + 1) * per * plane), 1) for r in range(world)]
    coarse = dist.assemble_coarse([r.coarse_rows() for r in ranks])
    tails = [dist.make_tail(coarse, (8, 8, 8), 2, smoother="colour") for _ in ranks]
    for r, t in zip(ranks, tails):
        r.set_tail(t)
    g = _hip_dist.Slab27Group(ranks, p2p=1)                 # (neighbour rows exchanged, buffers mapped)
    try:
        b = np.random.default_rng(2).random(shape[0] * plane)
        for r in ranks:
            r.load(b[r.rank * per * plane:(r.rank + 1) * per * plane])
        with pytest.raises((RuntimeError, _hip.HipError)):
            ranks[0].cycles(1, 1, 1)                        # rank 1 does not take part
    finally:
        g.close()
        for t in tails:
            t.close()


@pytest.mark.parametrize("pre,post", [(1, 1), (1, 0)])
def test_eight_slabs_against_the_oracle(pre, post):
    """16^3, 3 grids, fp64, 8 slabs of two planes: every cycle's norm within BASELINE's 1e-10 of the oracle's."""
    shape, grids, world, n_levels = (16, 16, 16), 3, 8, 1
    A0 = operators.stencil27_variable(shape)
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    Ro = orc.restriction_list(shape, grids - 2, 1)
    Ao = orc.coefficient_list(A0, Ro)
    sm = orc.make_smoother("colour", Ao)
    p = {"preIterations": pre, "postIterations": post, "coarsestLevel": len(Ro)}
    g, tails, _ = slab_group(shape, world, n_levels, grids, "float64")
    try:
        per = b.size // world
        for r in g.ranks:
            r.load(b[r.rank * per:(r.rank + 1) * per])
        norms = g.cycles(pre, post, 3)
        xo = None
        for k in range(3):
            xo, info = orc.mg_cycle(Ao, b, 0, Ro, p, initial=xo, smoother=sm)
            assert abs(norms[k] - info["norm"]) <= 1e-10 * info["norm"], (k, norms[k], info["norm"])
        x = np.concatenate([r.fetch() for r in g.ranks])
        np.testing.assert_allclose(x, xo, rtol=1e-9, atol=1e-12)
    finally:
        g.close()
        for t in tails:
            t.close()


def test_rows_that_are_not_the_stencil_are_refused():
    shape = (16, 16, 16)
    rows = dist.stencil27_variable_rows(shape, 0, 8 * 256).tolil()
    rows[300, 301] = 0.0
    bad = sp.csr_matrix(rows)
    bad.eliminate_zeros()
    with pytest.raises(_hip.HipError):
        _hip_dist.Slab27Rank(0, 2, shape, bad, 1)
    with pytest.raises(_hip.HipError):                           # six planes per rank, then three: an aggregate would straddle the ranks
        _hip_dist.Slab27Rank(0, 2, (12, 16, 16), dist.stencil27_variable_rows((12, 16, 16), 0, 6 * 256), 2)
