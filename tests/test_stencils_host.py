"""tests/stencils.py without a GPU: for every (set, shape, grids) tests/test_gpu_plane_aniso.py uses, each level of the
Galerkin hierarchy has ONE value per offset — in fp64, and again after a round trip through fp32 — which is what
PlanePlan::build and plane_check_kernel ask of a level (openmg_amd/csrc/plane.hip: data[p] != c[e] disqualifies it).  Under
that condition 'level l must carry the plane flag' is a fair assertion there.  Also: the seven values of an UNSYM set are
pairwise different on every level (a test built on them can tell any two slots apart), and every operator is strictly
diagonally dominant."""
import numpy as np
import pytest
import scipy.sparse as sp

from stencils import (CASES, ROUGH7, ROUGH_CASE, SETS, SYM5, SYM7, UNSYM5, UNSYM7, hierarchy, level_shapes, line_problem, slots_of,
                      stencil_constant, values_per_offset)


def dominance(A):
    """min over the rows of |diagonal| - sum of |off-diagonals|"""
    A = sp.csr_matrix(A)
    d = np.abs(A.diagonal())
    return float((d - (np.asarray(abs(A).sum(axis=1)).ravel() - d)).min())


def test_the_cases_cover_every_set_and_kind_of_grid():
    assert {c[0] for c in CASES} == {"UNSYM7", "SYM7", "UNSYM5"}
    assert {len(c[1]) for c in CASES} == {2, 3}
    assert any(len(set(c[1])) == 3 for c in CASES)


@pytest.mark.parametrize("name,shape,grids", CASES)
def test_one_value_per_offset_on_every_level(name, shape, grids):
    c = SETS[name]
    A, R = hierarchy(shape, grids, c)
    slots = [3] + [s for s, _, _ in slots_of(shape)]
    assert values_per_offset(A[0], shape) == {s: {float(c[s])} for s in slots}
    for l, sh in enumerate(level_shapes(shape, grids)):
        assert A[l].shape[0] == int(np.prod(sh)) and A[l].has_sorted_indices
        if l < grids - 1:
            assert np.all(R[l].data == R[l].data[0]) and R[l].shape == (A[l + 1].shape[0], A[l].shape[0])
        present = [3] + [s for s, axis, _ in slots_of(sh) if sh[axis] > 1]
        for M in (A[l], sp.csr_matrix((A[l].data.astype(np.float32).astype(np.float64), A[l].indices, A[l].indptr), shape=A[l].shape)):
            v = values_per_offset(M, sh)
            assert sorted(v) == sorted(present), (l, sorted(v))
            assert all(len(s) == 1 for s in v.values()), (name, shape, l, v)
            if name.startswith("UNSYM"):
                assert len({next(iter(s)) for s in v.values()}) == len(present), (name, shape, l, v)
        assert np.array_equal(A[l].data.astype(np.float32).astype(np.float64), A[l].data), (name, shape, l)   # exact in fp32
        assert dominance(A[l]) > 0.0, (name, shape, l, dominance(A[l]))


def test_the_sets():
    for c in (UNSYM7, UNSYM5):
        nz = [v for v in c if v != 0.0]
        assert len(set(nz)) == len(nz)
    assert len(set(UNSYM7)) == 7 and len(set(ROUGH7)) == 7
    for c in (SYM7, SYM5):
        assert c[:3] == c[:3:-1] and len({c[0], c[1], c[2]}) == 3
    for c in SETS.values():
        assert c[3] > sum(abs(v) for v in c[:3] + c[4:])
    for c in (UNSYM7, SYM7, UNSYM5, SYM5):
        assert all(float(4 * v).is_integer() and abs(v) < 16 for v in c)          # dyadic
    assert not all(float(4 * v).is_integer() for v in ROUGH7)
    # symmetric sets give symmetric operators, the others do not
    S, U = stencil_constant((4, 6, 8), SYM7), stencil_constant((4, 6, 8), UNSYM7)
    assert abs(S - S.T).max() == 0.0 and abs(U - U.T).max() > 0.0


def test_stencil_constant_against_a_dense_loop():
    for shape, c in (((3, 4, 5), UNSYM7), ((4, 3), UNSYM5), ((6,), (0, 0, -1.25, 3.0, -0.75, 0, 0))):
        A = stencil_constant(shape, c)
        n = int(np.prod(shape))
        D = np.zeros((n, n))
        full = (1,) * (3 - len(shape)) + tuple(shape)
        nz, ny, nx = full
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    r = (k * ny + j) * nx + i
                    for s, (dk, dj, di) in enumerate(((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0))):
                        kk, jj, ii = k + dk, j + dj, i + di
                        if 0 <= kk < nz and 0 <= jj < ny and 0 <= ii < nx and c[s] != 0:
                            D[r, (kk * ny + jj) * nx + ii] = c[s]
        assert np.array_equal(A.toarray(), D), shape
        assert A.has_sorted_indices and A.nnz == np.count_nonzero(D)


def test_rough_constants_stay_dominant_and_the_line_operator_is_what_the_gpu_test_says():
    shape, grids = ROUGH_CASE
    A, _ = hierarchy(shape, grids, ROUGH7)
    assert all(dominance(M) > 0.0 for M in A)
    A, R, _ = line_problem()
    assert [M.shape[0] for M in A] == [4099, 2049, 1024] and abs(A[0] - A[0].T).max() == 0.0
    assert values_per_offset(A[0], (4099,)) == {2: {-1.0}, 3: {2.5}, 4: {-1.0}}
    assert all(np.all(Rl.data == 0.5) for Rl in R)
    assert list(np.diff(R[0].indptr)[-2:]) == [2, 3] and list(np.diff(R[1].indptr)[-2:]) == [2, 3]
    assert all(dominance(M) > 0.0 for M in A)
