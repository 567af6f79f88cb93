"""A setup whose coarse factorisation fails: omg_hierarchy_create factorises the coarsest operator on a helper thread with a
stream of its own while the calling thread sets up the smoothed levels (hierarchy.hip, CoarseThread); the helper's error
is raised after the calling thread's work.  The constructor must return it as an ordinary error and leave nothing behind —
no thread, no stream, no state: the next hierarchy of the same process is the one a fresh process builds.

The input: 8^3 7-point Poisson, two levels; the coarsest operator (4^3 = 64 rows) is the Galerkin product with its last
row and last column emptied (a stored 0.0 on the diagonal keeps the CSR valid).  An all-zero column has no pivot at any
stage of the elimination and zeros stay exactly zero, so the factorisation's flag is set deterministically: ERR_SINGULAR
(dense.hip)."""
import numpy as np
import pytest
import scipy.sparse as sp

from openmg_amd import _hip, operators

pytestmark = pytest.mark.gpu

SHAPE = (8, 8, 8)


def lists():
    A0 = operators.stencil_poisson(SHAPE)
    R = operators.restrictionList(SHAPE, 1, 8)
    A = operators.coeffecientList(A0, R)
    assert len(A) == 2 and A[1].shape == (64, 64)
    D = A[1].toarray()
    D[63, :] = 0.0
    D[:, 63] = 0.0
    C = sp.coo_matrix(D)
    bad = sp.csr_matrix((np.append(C.data, 0.0), (np.append(C.row, 63), np.append(C.col, 63))), shape=D.shape)
    bad.sort_indices()
    assert bad.nnz == C.nnz + 1 and bad.indptr[64] - bad.indptr[63] == 1 and bad.data[-1] == 0.0      # (the stored zero is kept)
    assert not (bad.toarray()[:, 63] != 0).any() and not (bad.toarray()[63, :] != 0).any()
    return A, [A[0], bad], R


def three_cycles(A, R, smoother, dtype, b):
    with _hip.Hierarchy(A, R, smoother=smoother, dtype=dtype) as h:
        h.resident_load(b)
        norms = h.resident_cycles(1, 1, 3)
        return norms, h.resident_fetch()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("smoother", ["colour", "gs"])                   # (colour: a plane level above the coarsest)
def test_a_failed_coarse_factorisation_is_an_error_and_leaves_nothing_behind(smoother, dtype):
    A, A_bad, R = lists()
    b = A[0] @ np.random.default_rng(5).random(A[0].shape[0])
    want = three_cycles(A, R, smoother, dtype, b)                         # a fresh handle, before the failed one
    assert all(np.isfinite(want[0])) and want[0][2] < want[0][0]
    with pytest.raises(_hip.HipError) as e:
        _hip.Hierarchy(A_bad, R, smoother=smoother, dtype=dtype)
    assert e.value.code == _hip.ERR_SINGULAR, str(e.value)
    got = three_cycles(A, R, smoother, dtype, b)                          # the same lists with the intact A[1], same process
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])
