"""The row kernels of csrc/csr_kernels.hip (rows_kernel, rows_pattern_kernel, rows_union_kernel, rows_serial_kernel)
against the exact CPU restatement oracle/mg_oracle.py rows_* — np.array_equal, float64 and float32 — on irregular
operators: every family of tests/rows_cases.py, under plain CSR and the full coding, with and without the pattern
kernel, and for the stencil-like families with 1, 2 and 4 rows per thread of the union walk.  The restatement itself
is pinned to exact rational arithmetic in tests/test_rows_oracle_host.py.

Each case is a two-level hierarchy [A0, A1], [R] (A1 a small dominant matrix: the lists route does not ask for the
Galerkin product) and uses the level entries spmv, residual(want_norm=True), restrict, prolong_add and smooth.  Which
kernel variant a family reaches follows encode_csr's rule (rows_cases' docstring, checked on the host in
tests/test_rows_oracle_host.py); where the library reports the path (format_info, level_flags) it is asserted here.

The only tolerance in this file is the norm's: sqrt of a sum of n non-negative doubles added in any order, against
math.fsum: (n + 2) 2^-53 relative.  Needs an MI355X: run with -m gpu."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import rows_cases as rc
from openmg_amd import _hip
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
# (OMG_COMPRESS, OMG_PATTERN_KERNEL, OMG_UNION_ROWS); None = unset
PLAIN_CODINGS = [("0", None, None), ("15", None, None), ("0", "0", None), ("15", "0", None)]
STENCIL_CODINGS = [("0", None, None), ("0", "0", None), ("15", "0", None), ("15", None, "1"), ("15", None, "2"), ("15", None, "4")]
CASES = [(name, c) for name, fam in rc.FAMILIES.items() for c in (STENCIL_CODINGS if fam.stencil else PLAIN_CODINGS)]
CASE_IDS = ["%s-c%s-pk%s-u%s" % (name, c[0], c[1] or "d", c[2] or "d") for name, c in CASES]
GS_MAX_N = 1200                       # lexicographic sweeps: one launch per dependency level


def set_coding(monkeypatch, coding):
    for key, val in zip(("OMG_COMPRESS", "OMG_PATTERN_KERNEL", "OMG_UNION_ROWS"), coding):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)
    for key in ("OMG_UNION_KERNEL", "OMG_NO_FUSE", "OMG_PROLONG_SCATTER", "OMG_MARCH"):
        monkeypatch.delenv(key, raising=False)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def problem(name, regime):
    """Operator, the three restrictions with their coarsest operators, and the vectors of one family and regime."""
    fam = rc.FAMILIES[name]
    integers = regime == "integers"
    A = rc.integer_operator(fam) if integers else rc.real_operator(fam)
    Rs = {k: rc.restriction(fam, k, integers) for k in rc.RESTRICTIONS}
    nc = {k: R.shape[0] for k, R in Rs.items()}
    vec = (rc.integer_vectors if integers else rc.real_vectors)(fam, nc)
    for v in (*(a for a in vec.values() if isinstance(a, np.ndarray)), *vec["coarse"].values()):
        v.setflags(write=False)
    return {"fam": fam, "A": A, "R": Rs, "Ac": {k: rc.coarse_operator(m) for k, m in nc.items()}, "vec": vec}


@functools.lru_cache(maxsize=None)
def colouring_of(name):
    return frozen(orc.greedy_colouring(problem(name, "reals")["A"]))


def colour_order_of(name):
    return orc.colour_order(colouring_of(name))


@functools.lru_cache(maxsize=None)
def expected_integers(name):
    """np.int64 arithmetic (the same for both precisions and any association)."""
    p = problem(name, "integers")
    A, v = p["A"], p["vec"]
    x, b, fine = (v[k].astype(np.int64) for k in ("x", "b", "fine"))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], dtype=np.int64)
    np.add.at(Ax, rows, A.data.astype(np.int64) * x[A.indices])
    out = {"spmv": frozen(Ax), "residual": frozen(b - Ax)}
    for k, R in p["R"].items():
        Ri = sp.csr_matrix((R.data.astype(np.int64), R.indices, R.indptr), shape=R.shape)
        out["restrict", k] = frozen(Ri @ fine)
        out["prolong", k] = frozen(fine + Ri.T @ v["coarse"][k].astype(np.int64))
    return out


@functools.lru_cache(maxsize=None)
def expected_reals(name, dtype):
    p = problem(name, "reals")
    A, v = p["A"], p["vec"]
    out = {"spmv": frozen(orc.rows_spmv(A, v["x"], dtype)), "residual": frozen(orc.rows_residual(A, v["b"], v["x"], dtype))}
    out["spmv_d"] = frozen(orc.rows_spmv(A, v["xd"], dtype))          # operands that float32 does not hold
    out["residual_d"] = frozen(orc.rows_residual(A, v["bd"], v["xd"], dtype))
    for k, R in p["R"].items():
        out["restrict", k] = frozen(orc.rows_spmv(R, v["fine"], dtype))
        out["restrict_d", k] = frozen(orc.rows_spmv(R, v["xd"], dtype))
        if k != "overlap":                   # one entry per row of R^T: one product rounded, then one addition
            out["prolong", k] = frozen(orc.rows_axpy(rc.transpose_stored(R), v["coarse"][k], v["fine"], dtype))
    return out


@functools.lru_cache(maxsize=None)
def expected_sweeps(name, dtype, smoother, sweeps):
    p = problem(name, "reals")
    A, v = p["A"], p["vec"]
    if smoother == "jacobi":
        return frozen(orc.rows_jacobi(A, v["b"], v["x"], sweeps, 0.7, dtype))
    order = None if smoother == "gs" else colour_order_of(name)
    return frozen(orc.rows_gs_ordered(A, v["b"], v["x"], order, sweeps, dtype))


def check_norm(norm, residual, exact):
    """The reported norm against math.fsum of the squares of the (restated) residual: n non-negative double additions
    in any order and the square root, (n + 2) 2^-53 relative."""
    sq = math.fsum(float(r) * float(r) for r in residual)
    if exact:
        assert sq < 2.0 ** 53                                    # integers: the squares and their sum are exact
    want = math.sqrt(sq)
    assert abs(norm - want) <= (len(residual) + 2) * 2.0 ** -53 * want, (norm, want)


def check_paths(h, fam, coding, kind, nc, smoother, constant_values):
    """What the library tells about the path that ran."""
    compress, pk, ur = coding
    flags, info = h.level_flags(0), h.format_info(0)
    for other in ("march", "plane", "stencil27", "var7", "line"):
        assert not flags[other], other                           # the row kernels, not a structured path
    assert info["rows"] == fam.n and info["nnz"] == fam.nnz
    if kind == "overlap" and nc >= 3:
        assert not flags["scatter_prolong"]                      # shared columns: the explicit transpose and ROW_AXPY
    if smoother == "jacobi":
        # natural order on both levels: R is coded as the caller stored it, and rows_cases.scatter_expected() (checked
        # against the host-side coding in tests/test_rows_oracle_host.py) says whether prolong_add is ROW_SCATTER over
        # R's rows — the strided restrictions under a pattern coding — or ROW_AXPY over the explicit transpose
        scatter = rc.scatter_expected(fam, kind, compress, pk)
        assert flags["scatter_prolong"] == scatter, (kind, coding)
        rinfo = h.format_info(0, "R")
        assert (rinfo["pattern_rows"] == rinfo["rows"]) == scatter
        if scatter:
            assert (rinfo["ell_blocks"] == rinfo["blocks"]) == (kind == "strided_var")
    if compress == "0":
        assert info["pattern_rows"] == 0 and info["coldict_nnz"] == 0 and info["valdict_nnz"] == 0 and info["ell_blocks"] == 0
        assert not flags["scatter_prolong"] and not flags["union_walk"]
    if pk == "0":
        assert info["ell_blocks"] == 0 and not flags["union_walk"]
    if not fam.stencil:
        assert not flags["union_walk"]
        if smoother == "jacobi":
            # natural order, one set: the row-block partition shows encode_csr's choice (rows_cases' docstring) —
            # four lanes per row: blocks of at most 64 rows; widened blocks (the SHORT variant): more than 256 rows
            # per block; else at most 256 rows
            if fam.expected_lanes() == 4:
                assert info["blocks"] >= -(-fam.n // 64)
            elif fam.expected_short() and fam.n >= 1024:
                assert info["blocks"] < -(-fam.n // 256)
            else:
                assert info["blocks"] >= -(-fam.n // 256)
    if fam.stencil and compress == "15" and pk is None and smoother == "jacobi":    # natural order: the host-side check applies
        assert info["pattern_rows"] == fam.n
        if constant_values:
            u = int(ur)
            if u > 1 and fam.n >= 4 * u * 256:                   # wide union blocks, U rows per thread
                assert flags["union_walk"] and info["blocks"] == -(-fam.n // (256 * u))
        else:
            assert info["ell_blocks"] == info["blocks"] and info["ell_nnz"] == fam.nnz


# three orderings of the same operator; the strided restrictions keep the natural order, in which they are pattern coded
SMOOTHER_OF_KIND = {"pair": "jacobi", "irregular": "colour", "overlap": "gs", "strided": "jacobi", "strided_var": "jacobi"}


def smoother_for(kind, n):
    s = SMOOTHER_OF_KIND[kind]
    return "colour" if s == "gs" and n > GS_MAX_N else s


def level_operations(p, kind, dtype, coding, constant_values):
    fam, v = p["fam"], p["vec"]
    smoother = smoother_for(kind, fam.n)
    with _hip.Hierarchy([p["A"], p["Ac"][kind]], [p["R"][kind]], smoother=smoother, omega=0.7, dtype=dtype) as h:
        check_paths(h, fam, coding, kind, p["R"][kind].shape[0], smoother, constant_values)
        y = h.spmv(0, v["x"])
        r, norm = h.residual(0, v["b"], v["x"], want_norm=True)
        coarse = h.restrict(0, v["fine"])
        fine = h.prolong_add(0, v["coarse"][kind], v["fine"])
        extra = (h.spmv(0, v["xd"]), h.residual(0, v["bd"], v["xd"]), h.restrict(0, v["xd"])) if "xd" in v else None
    return y, r, norm, coarse, fine, extra


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,coding", CASES, ids=CASE_IDS)
def test_integer_operators_equal_int64_arithmetic(monkeypatch, name, coding, dtype):
    """Entries in [-8, 8], x in [-64, 64], b in [-1000, 1000], restriction weights 1, 2, 4: every partial sum is an
    integer below 2^24, exact in both precisions under any association — spmv, residual (and its norm), restrict and
    prolong_add, the overlapping restriction's internal transpose and the scatter over the strided restrictions' rows
    included, equal np.int64 arithmetic."""
    set_coding(monkeypatch, coding)
    p, want = problem(name, "integers"), expected_integers(name)
    for kind in rc.RESTRICTIONS:
        y, r, norm, coarse, fine, _ = level_operations(p, kind, dtype, coding, p["fam"].constant is not None)
        assert np.array_equal(y, want["spmv"]), kind
        assert np.array_equal(r, want["residual"]), kind
        check_norm(norm, want["residual"], exact=True)
        assert np.array_equal(coarse, want["restrict", kind]), kind
        assert np.array_equal(fine, want["prolong", kind]), kind


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,coding", CASES, ids=CASE_IDS)
def test_real_operators_equal_the_restatement(monkeypatch, name, coding, dtype):
    """float32-representable normals: spmv, residual and restrict have the restatement's bits in both precisions under
    three orderings of the operator — also with vectors that float32 does not hold (in float64 a fused and an unfused
    row sum differ only then) —; prolong_add with the four aggregation restrictions too (one product rounded, one
    addition): through the explicit transpose (pair, irregular) and, where check_paths has seen scatter_prolong, as
    ROW_SCATTER over the rows of the strided restrictions, with pattern values and with ELL values."""
    set_coding(monkeypatch, coding)
    p, want = problem(name, "reals"), expected_reals(name, dtype)
    for kind in rc.RESTRICTIONS:
        y, r, norm, coarse, fine, (yd, rd, cd) = level_operations(p, kind, dtype, coding, p["fam"].constant is not None)
        assert np.array_equal(y, want["spmv"]), kind
        assert np.array_equal(r, want["residual"]), kind
        check_norm(norm, want["residual"], exact=False)
        assert np.array_equal(coarse, want["restrict", kind]), kind
        assert np.array_equal(yd, want["spmv_d"]) and np.array_equal(rd, want["residual_d"]), kind
        assert np.array_equal(cd, want["restrict_d", kind]), kind
        if kind != "overlap":
            assert np.array_equal(fine, want["prolong", kind]), kind


RELAX_CASES = [(name, c, s) for name, c in CASES for s in ("gs", "colour", "jacobi")
               if s != "gs" or rc.FAMILIES[name].n <= GS_MAX_N]      # lexicographic sweeps: families of at most 1200 rows
RELAX_IDS = ["%s-c%s-pk%s-u%s-%s" % (name, c[0], c[1] or "d", c[2] or "d", s) for name, c, s in RELAX_CASES]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,coding,smoother", RELAX_CASES, ids=RELAX_IDS)
def test_relaxations_equal_the_restatement(monkeypatch, name, coding, dtype, smoother):
    """1 and 3 sweeps on the strictly dominant operators: lexicographic Gauss-Seidel (level schedule, serial kernel for
    runs of one-block sets; families of at most 1200 rows), greedy multi-colour Gauss-Seidel and Jacobi with
    omega = 0.7 (not representable: its rounding to the element type is part of the statement)."""
    p = problem(name, "reals")
    fam, v = p["fam"], p["vec"]
    set_coding(monkeypatch, coding)
    with _hip.Hierarchy([p["A"], p["Ac"]["pair"]], [p["R"]["pair"]], smoother=smoother, omega=0.7, dtype=dtype) as h:
        check_paths(h, fam, coding, "pair", p["R"]["pair"].shape[0], smoother, fam.constant is not None)
        for sweeps in (1, 3):
            x = v["x"].copy()
            h.smooth(0, v["b"], x, sweeps)
            assert np.array_equal(x, expected_sweeps(name, dtype, smoother, sweeps)), sweeps


# The greedy colouring of a random operator ends in colours of a handful of rows — single-block sets, one serial launch,
# nothing to fuse — so the random families run this test on rows_cases.bipartite_operator(): the family's rows with two
# colours of n / 2 rows.  FUSING: the families whose half then spans several row blocks (encode_csr's partition,
# rows_cases' docstring), the one-row and the diagonal operator (a single set), and the banded family whose own last
# colour does; in the others the fused modes cannot run (two single-block sets) and only the comparison is made.
FUSING = {"tiny1", "unit", "block600", "short1to2", "short1to4", "short17", "short_one19", "long", "mixed", "huge300",
          "huge1200", "band_const2304"}


@functools.lru_cache(maxsize=None)
def fused_problem(name):
    fam = rc.FAMILIES[name]
    A = problem(name, "reals")["A"] if fam.stencil else rc.bipartite_operator(fam)
    return A, int(orc.greedy_colouring(A).max()) + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(rc.FAMILIES))
def test_fused_last_set_sweeps_leave_the_same_bits(monkeypatch, name, dtype):
    """Two V(1,1) cycles with the last colour's sweep fused with the residual / norm launch (ROW_GS_RES, ROW_GS_NORM)
    and with OMG_NO_FUSE=1: the same iterate and the same norms.  Whether a level fuses is can_fuse's rule
    (hierarchy.hip, with build_plan): the last step of the sweep must be an ordinary set launch, and runs of two or
    more consecutive single-block sets are one serial launch — so the level fuses exactly when its last two sets are
    not both single-block.  Asserted both ways from the block counts the library reports per set; FUSING lists the
    families in which the fused modes run."""
    p = problem(name, "reals")
    fam, v = p["fam"], p["vec"]
    A, colours = fused_problem(name)
    coupled = bool(np.any(A.indices != np.repeat(np.arange(fam.n), fam.lengths)))
    assert fam.stencil or colours == (2 if coupled else 1)      # (the diagonal operator and the one-row one: a single set)
    set_coding(monkeypatch, ("15", None, None))
    out = {}
    for no_fuse in ("1", "0"):
        monkeypatch.setenv("OMG_NO_FUSE", no_fuse)
        with _hip.Hierarchy([A, p["Ac"]["pair"]], [p["R"]["pair"]], smoother="colour", dtype=dtype) as h:
            blocks = [h.format_info(0, "A", q)["blocks"] for q in range(h.level_sets(0))]
            assert len(blocks) == colours and min(blocks) >= 1
            fuses = not (len(blocks) >= 2 and blocks[-1] == 1 and blocks[-2] == 1)
            assert h.level_flags(0)["fused_last_set"] == (fuses and no_fuse == "0"), blocks
            assert fuses == (name in FUSING), blocks
            h.resident_load(v["b"], v["x"])
            norms = [h.resident_cycle(1, 1) for _ in range(2)]
            out[no_fuse] = (h.resident_fetch(), norms)
    assert np.array_equal(out["0"][0], out["1"][0])
    assert out["0"][1] == out["1"][1]
    # ... and the sweeps are the restatement's: with a restriction of zero weights a cycle is its two sweeps (see below)
    R0 = p["R"]["pair"].copy()
    R0.data[:] = 0.0
    monkeypatch.setenv("OMG_NO_FUSE", "0")
    with _hip.Hierarchy([A, p["Ac"]["pair"]], [R0], smoother="colour", dtype=dtype) as h:
        h.resident_load(v["b"], v["x"])
        norm = h.resident_cycle(1, 1)
        x = h.resident_fetch()
    want = orc.rows_gs_ordered(A, v["b"], v["x"], orc.colour_order(orc.greedy_colouring(A)), 2, dtype)
    assert np.array_equal(x, want)
    check_norm(norm, orc.rows_residual(A, v["b"], want, dtype), exact=False)


JACOBI_CYCLE_FAMILIES = ["mixed", "long", "short1to2", "huge1200", "band_const2304", "band_var2304"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", JACOBI_CYCLE_FAMILIES)
def test_resident_jacobi_cycles_equal_the_restatement(monkeypatch, name, dtype):
    """ROW_JACOBI_PRENORM: in a batch of resident cycles a Jacobi level's first launch of cycle k + 1 also forms the
    squares of cycle k's residual (can_prenorm: any Jacobi level with a pre-sweep).  With a restriction whose stored
    weights are all zero the coarse correction is exactly zero (R r = 0, the coarsest solve of 0, x + 0 * e), so three
    V(1,1) cycles are six Jacobi sweeps: the iterate has the restatement's bits — the fused epilogue
    fma(omega, q, x) in the PRENORM instantiations too — and every cycle's norm is the restated residual's."""
    p = problem(name, "reals")
    fam, v = p["fam"], p["vec"]
    set_coding(monkeypatch, ("15", None, None))
    R = p["R"]["pair"].copy()
    R.data[:] = 0.0
    with _hip.Hierarchy([p["A"], p["Ac"]["pair"]], [R], smoother="jacobi", omega=0.7, dtype=dtype) as h:
        h.resident_load(v["b"], v["x"])
        norms = h.resident_cycles(1, 1, 3)
        x = h.resident_fetch()
    assert np.array_equal(x, orc.rows_jacobi(p["A"], v["b"], v["x"], 6, 0.7, dtype))
    for k, norm in enumerate(norms):
        xk = orc.rows_jacobi(p["A"], v["b"], v["x"], 2 * (k + 1), 0.7, dtype)
        check_norm(norm, orc.rows_residual(p["A"], v["b"], xk, dtype), exact=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_committed_association_row_on_the_device(dtype):
    """The committed 17-entry float32 row of tests/rows_cases.py whose one-chain and four-chain sums differ, as a row
    of a device operator — among short rows (one lane per row, the LONG instantiation) and among long ones (four lanes
    per row) — and its 16-entry prefix: four chains above ASSOC_LEN, one chain at it."""
    v17, x17 = rc.from_hex(rc.ROW17_V), rc.from_hex(rc.ROW17_X)
    four, one = float.fromhex(rc.ROW17_FOUR), float.fromhex(rc.PREFIX16_ONE)
    for filler in (2, 24):                                       # the other rows' length: average below / above 16
        n = 64
        lengths = np.full(n, filler)
        lengths[5], lengths[9] = 17, 16
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        indices = (np.arange(indptr[-1]) % 17).astype(np.int32)
        data = np.ones(indptr[-1])
        indices[indptr[:-1]] = np.arange(n)                      # a diagonal entry in every row
        data[indptr[:-1]] = 40.0
        x = np.zeros(n)
        x[:17] = x17
        # the two rows: entries in the committed order, columns 0..16 holding the committed x; the diagonal column's
        # entry keeps its place in the chain (row 5: entry 5, row 9: entry 9)
        indices[indptr[5]:indptr[6]] = np.arange(17)
        data[indptr[5]:indptr[6]] = v17
        indices[indptr[9]:indptr[10]] = np.arange(16)
        data[indptr[9]:indptr[10]] = v17[:16]
        A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
        A.has_sorted_indices = False
        R = sp.csr_matrix((np.ones(n), (np.arange(n) // 2, np.arange(n))), shape=(n // 2, n))
        with _hip.Hierarchy([A, rc.coarse_operator(n // 2)], [R], smoother="jacobi", dtype=dtype) as h:
            y = h.spmv(0, x)
        assert np.array_equal(y, orc.rows_spmv(A, x, dtype)), filler
        if dtype == "float32":
            assert y[5] == four and y[9] == one, filler


def test_load_and_fetch_round_once_to_float32():
    """gather_kernel / scatter_kernel<double, float> through a colour ordering: resident_load followed by resident_fetch
    returns the iterate rounded once to float32, to nearest even — ties at 1 + 2^-24 and 1 + 3 2^-24, doubles on both
    sides of FLT_MAX (the tie FLT_MAX + half an ulp goes to infinity, anything below it to FLT_MAX), signed zeros.
    (Subnormals are left out: nothing in the kernels states how they are kept.)"""
    p = problem("block257", "reals")
    n = p["fam"].n
    fmax = float(np.finfo(np.float32).max)
    half_ulp = 2.0 ** 103                                        # FLT_MAX = (2 - 2^-23) 2^127: ulp 2^104
    special = np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50,
                        np.nextafter(fmax, 0.0), fmax, np.nextafter(fmax, np.inf), fmax + half_ulp / 2,
                        np.nextafter(fmax + half_ulp, 0.0), fmax + half_ulp, -(fmax + half_ulp), -np.nextafter(fmax + half_ulp, 0.0),
                        0.0, -0.0, 2.0 ** -100, 1.0 / 3.0])
    x0 = np.random.default_rng(41).standard_normal(n)
    where = np.random.default_rng(42).choice(n, size=special.size, replace=False)
    x0[where] = special
    with np.errstate(over="ignore"):
        want = x0.astype(np.float32).astype(np.float64)
    assert want[where[0]] == 1.0 and want[where[1]] == 1.0 + 2.0 ** -22 and want[where[3]] == 1.0 + 2.0 ** -23
    assert want[where[8]] == fmax and want[where[9]] == np.inf and want[where[10]] == -np.inf and want[where[11]] == -fmax
    with _hip.Hierarchy([p["A"], p["Ac"]["pair"]], [p["R"]["pair"]], smoother="colour", dtype="float32") as h:
        assert h.level_sets(0) > 1                               # a colour ordering: the index maps are in use
        h.resident_load(p["vec"]["b"], x0)
        got = h.resident_fetch()
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))
