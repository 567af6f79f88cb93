"""The coarsest-level solve of a tests/coarse_cases.py case on the device (tests/test_gpu_coarse_edges.py), and, run as a
program, the same in a process of its own:

`coarse_edges_worker.py CASE [CASE ...]` prints one JSON line {case: {dtype: {"info": coarse_info(), "x": [...]}}}.  The
parent sets OMG_DENSE_BLOCKED=0, which like every such switch is read once per process: the pivoted column-by-column
elimination at sizes the blocked one would take."""
import contextlib
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

from openmg_amd import _hip

DTYPES = ("float64", "float32")


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def solve_on_device(case, num, dtype, rhs):
    """(coarse_info(), x) of a hierarchy whose coarsest operator is the case's: two levels, [block_diag(A, A), A] with a
    selection for R (not a Galerkin pair: only the coarse solver is used), in `dtype`; the case's switches set while it is
    built.  A null-space case: its own Neumann hierarchy with nullspace='constant'."""
    import coarse_cases as cc
    with environment(case.env):
        if case.lists is not None:
            A, R = cc.neumann_lists(case.lists)
            with _hip.Hierarchy(A, R, smoother="colour", dtype=dtype, nullspace="constant") as h:
                return h.coarse_info(), h.coarse_solve(rhs)
        A, n = num.A, num.n
        A1 = sp.block_diag([A, A], format="csr")
        if not np.all(A1.diagonal()):                        # (the fine level is smoothed: it needs a diagonal; the coarsest does not)
            A1 = sp.csr_matrix(A1 + sp.identity(2 * n))
        Rsel = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n))), shape=(n, 2 * n))
        with _hip.Hierarchy([A1, A], [Rsel], smoother="jacobi", dtype=dtype) as h:
            return h.coarse_info(), h.coarse_solve(rhs)


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import coarse_cases as cc
    cases = {c.name: c for c in cc.all_cases()}
    out = {}
    for name in sys.argv[1:]:
        num = cc.numbers(cases[name])
        out[name] = {}
        for dtype in DTYPES:
            info, x = solve_on_device(cases[name], num, dtype, num.b if dtype == "float64" else num.b32)
            out[name][dtype] = {"info": info, "x": [float(v) for v in x]}
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
