"""Operators, restrictions and vectors for tests/test_gpu_rows_bits.py (the row kernels against the exact
restatement oracle/mg_oracle.py rows_*) and for the host-side checks of the generators themselves in
tests/test_rows_oracle_host.py.  Everything is made from fixed seeds; nothing here needs a GPU.

A family fixes the STRUCTURE of a square operator: row lengths, stored columns (drawn with replacement, so
duplicates stay stored; stored order random).  A hierarchy refuses an operator row without a nonzero diagonal
(OMG_ERR_NO_DIAGONAL), so every row of an operator holds one designated diagonal entry at a random position and a
drawn length of 0 becomes that single entry; EMPTY rows live in the restrictions and their transposes instead
(restriction(), kind 'irregular': one coarse row and a few fine columns without entries).

Two value regimes fill a structure:
  integers  entries in [-8, 8], x in [-64, 64], b in [-1000, 1000], restriction weights in {1, 2, 4}: every partial
            sum of a row of at most 5000 entries is an integer below 5000 * 8 * 64 < 2^24, exact in float32 and
            float64 under ANY association, so the statement is np.int64 arithmetic;
  reals     standard normals rounded to float32 first (both precisions see the same numbers, the float32
            narrowing is exact), the designated diagonal +-(1 + the row's absolute sum): strictly dominant, so
            the relaxations are well defined.  Magnitudes stay far from the float32 subnormals.

Which kernel variant a family reaches follows encode_csr's rule (openmg_amd/csrc/setup_host.cpp): an average row
of more than 16 stored entries gives four lanes per row; average * 2 * rows <= 2048 widens the row blocks to 512 /
1024 / 2048 rows and picks rows_kernel's SHORT variant; a block ends at 256 rows (64 with four lanes) or at 2048
stored entries, whichever comes first; a row of more than 2048 entries is a block of its own and takes the
workgroup path.  expected_lanes() / expected_short() restate the two averages for the tests' assertions."""
import numpy as np
import scipy.sparse as sp

ASSOC_LEN = 16
ROWBLK_NNZ = 2048


class Family:
    def __init__(self, name, n, indptr, indices, diag_pos, stencil=False, constant=None):
        self.name, self.n = name, n
        self.indptr, self.indices, self.diag_pos = indptr, indices, diag_pos
        self.stencil = stencil                 # banded: the union walk / pattern codings are in reach
        self.constant = constant               # banded with one value per offset: index of each entry's offset, else None

    @property
    def nnz(self):
        return int(self.indptr[-1])

    @property
    def lengths(self):
        return np.diff(self.indptr)

    def expected_lanes(self):
        """encode_csr: four lanes share a row when the average row holds more than 16 stored entries."""
        return 4 if self.nnz / self.n > 16.0 else 1

    def expected_short(self):
        """encode_csr: the row blocks widen (rows_kernel's SHORT variant) while average * 2 * rows <= 2048."""
        return self.nnz / self.n * 512 <= ROWBLK_NNZ


def _random_family(name, n, lengths, rng):
    """Rows of the given stored lengths (0 -> 1: the diagonal alone); columns with replacement, order random."""
    lengths = np.maximum(np.asarray(lengths, dtype=np.int64), 1)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    diag_pos = (indptr[:-1] + rng.integers(0, lengths)).astype(np.int64)
    indices[diag_pos] = np.arange(n)
    return Family(name, n, indptr, indices, diag_pos)


def _huge_family(name, n, other_lengths, rng):
    """One row of 2049 and one of 5000 stored entries (the workgroup path), each with at least three further stored
    diagonal entries, among rows of the given lengths."""
    lengths = np.asarray(other_lengths(n), dtype=np.int64)
    big = {int(n // 3): 2049, int(2 * n // 3 + 1): 5000}
    for i, L in big.items():
        lengths[i] = L
    fam = _random_family(name, n, lengths, rng)
    for i in big:
        s, e = int(fam.indptr[i]), int(fam.indptr[i + 1])
        free = np.setdiff1d(np.arange(s, e), [fam.diag_pos[i]])
        fam.indices[rng.choice(free, size=3, replace=False)] = i
    return fam


def _banded_family(name, n, n_offsets, constant, rng):
    """Stencil-like: every row holds the same (column - row) offsets in the same shuffled stored order, entries that
    would leave the matrix dropped (boundary rows are subsequences of the interior row)."""
    reach = 60
    offs = np.concatenate([[0], rng.choice(np.setdiff1d(np.arange(-reach, reach + 1), [0]), size=n_offsets - 1, replace=False)])
    rng.shuffle(offs)
    i = np.arange(n)
    rows, cols, which = [], [], []
    for k, o in enumerate(offs):
        keep = (i + o >= 0) & (i + o < n)
        rows.append(i[keep]); cols.append(i[keep] + o); which.append(np.full(int(keep.sum()), k))
    rows, cols, which = np.concatenate(rows), np.concatenate(cols), np.concatenate(which)
    perm = np.argsort(rows, kind="stable")                      # row-major, offsets in the shuffled order
    indptr = np.searchsorted(rows[perm], np.arange(n + 1)).astype(np.int32)
    indices = cols[perm].astype(np.int32)
    diag_pos = np.flatnonzero(indices == np.repeat(i, np.diff(indptr))).astype(np.int64)
    return Family(name, n, indptr, indices, diag_pos, stencil=True, constant=which[perm] if constant else None)


def _make_families():
    fams = []
    seed = [7000]

    def rng():
        seed[0] += 1
        return np.random.default_rng(seed[0])

    def draw(n, choices, r):
        return r.choice(np.asarray(choices), size=n)

    for n in (1, 2, 3, 5):                                                              # tiny
        r = rng(); fams.append(_random_family("tiny%d" % n, n, r.integers(0, 6, size=n), r))
    for n in (63, 64, 65):                                                              # wave edges
        r = rng(); fams.append(_random_family("wave%d" % n, n, r.integers(0, 9, size=n), r))
    for n in (255, 256, 257, 600):                                                      # block edges: ~12 per row, the 2048-entry cap cuts blocks too
        r = rng(); fams.append(_random_family("block%d" % n, n, r.integers(8, 17, size=n), r))
    n = 3000                                                                            # short rows
    # (drawn lengths {0, 1, 2} and {0..4}; a drawn 0 is stored as 1, the diagonal alone — the module docstring —, so the
    # operators hold rows of 1..2 and 1..4 entries and no empty row: the names say what is stored)
    r = rng(); fams.append(_random_family("short1to2", n, draw(n, [0, 1, 2], r), r))
    r = rng(); fams.append(_random_family("short1to4", n, draw(n, [0, 1, 2, 3, 4], r), r))
    r = rng(); fams.append(_random_family("short17", n, draw(n, [1, 2, 3, 4, 5, 6, 7], r), r))
    r = rng(); fams.append(_random_family("unit", n, np.ones(n, dtype=np.int64), r))     # exactly one entry per row
    r = rng(); L = draw(n, [0, 1, 2], r); L[1717] = 19                                  # one long row among rows of 1..2 (drawn 0 -> 1)
    fams.append(_random_family("short_one19", n, L, r))
    n = 300                                                                             # long rows: four lanes per row
    r = rng(); fams.append(_random_family("long", n, draw(n, [17, 18, 19, 20, 31, 32, 33, 40, 64, 65], r), r))
    n = 700                                                                             # mixed: one lane per row, LONG instantiation
    r = rng(); L = r.integers(3, 16, size=n); m = r.random(n) < 0.05; L[m] = r.integers(17, 41, size=int(m.sum()))
    fams.append(_random_family("mixed", n, L, r))
    r = rng(); fams.append(_huge_family("huge300", 300, lambda n: r.integers(3, 10, size=n), r))     # average above 16
    r = rng(); fams.append(_huge_family("huge1200", 1200, lambda n: r.integers(3, 10, size=n), r))   # average below 16
    for n, k in ((2304, 7), (4352, 9)):                                                 # stencil-like
        r = rng(); fams.append(_banded_family("band_const%d" % n, n, k, True, r))
        r = rng(); fams.append(_banded_family("band_var%d" % n, n, k - 2, False, r))
    return fams


FAMILIES = {f.name: f for f in _make_families()}
RESTRICTIONS = ("pair", "irregular", "overlap", "strided", "strided_var")


def _seed_of(fam, salt):
    return [sum(ord(c) for c in fam.name) * 131 + fam.n, salt]


def integer_operator(fam):
    """Entries in [-8, 8] (no stored zero), every row's diagonal sum nonzero."""
    rng = np.random.default_rng(_seed_of(fam, 1))
    if fam.constant is not None:
        per = rng.integers(1, 9, size=int(fam.constant.max()) + 1) * rng.choice([-1, 1], size=int(fam.constant.max()) + 1)
        data = per[fam.constant].astype(np.float64)
    else:
        data = (rng.integers(1, 9, size=fam.nnz) * rng.choice([-1, 1], size=fam.nnz)).astype(np.float64)
    rows = np.repeat(np.arange(fam.n), fam.lengths)
    on_diag = fam.indices == rows
    dsum = np.bincount(rows[on_diag], weights=data[on_diag], minlength=fam.n)
    if fam.constant is None:
        for i in np.flatnonzero(dsum == 0):                      # duplicates cancelled the designated entry: move it by one
            p = fam.diag_pos[i]
            data[p] += 2.0 if data[p] == -1.0 else -1.0 if data[p] == 8.0 else 1.0     # stays in [-8, 8], not zero
    A = sp.csr_matrix((data, fam.indices.copy(), fam.indptr.copy()), shape=(fam.n, fam.n))
    A.has_sorted_indices = False
    return A


def real_operator(fam):
    """Standard normals rounded to float32; the designated diagonal +-(1 + the row's absolute sum), rounded to float32
    (banded with constant values: the largest row's, one value for the offset)."""
    rng = np.random.default_rng(_seed_of(fam, 2))
    if fam.constant is not None:
        per = rng.standard_normal(int(fam.constant.max()) + 1).astype(np.float32).astype(np.float64)
        data = per[fam.constant]
    else:
        data = rng.standard_normal(fam.nnz).astype(np.float32).astype(np.float64)
    rows = np.repeat(np.arange(fam.n), fam.lengths)
    data[fam.diag_pos] = 0.0
    absum = np.bincount(rows, weights=np.abs(data), minlength=fam.n)
    sign = rng.choice([-1.0, 1.0], size=fam.n)
    if fam.constant is not None:
        data[fam.diag_pos] = np.float64(np.float32(sign[0] * (1.0 + absum.max())))
    else:
        data[fam.diag_pos] = (sign * (1.0 + absum)).astype(np.float32).astype(np.float64)
    A = sp.csr_matrix((data, fam.indices.copy(), fam.indptr.copy()), shape=(fam.n, fam.n))
    A.has_sorted_indices = False
    return A


def bipartite_operator(fam):
    """real_operator(fam) with every off-diagonal column moved, where needed, into the other half of the unknowns: rows
    of the first half couple only to the second half and back, so the greedy colouring has two colours of n / 2 rows
    each (one for n = 1) instead of a tail of colours with a handful of rows.  Row lengths, stored order, values and
    the stored diagonal entries are the family's.  For the fused last-set sweeps, which run only where the sweep does
    not end in a run of single-block sets (tests/test_gpu_rows_bits.py)."""
    A = real_operator(fam)
    n, half = fam.n, fam.n // 2
    if half:
        rows = np.repeat(np.arange(n), fam.lengths)
        cols = A.indices.astype(np.int64)
        same = (cols != rows) & ((cols < half) == (rows < half))
        cols[same] = np.where(cols[same] < half, cols[same] + half, (cols[same] - half) % half)
        A.indices[:] = cols
    return A


def restriction(fam, kind, integers):
    """R (coarse x fine), stored order shuffled inside the rows.
    pair       aggregates {2k, 2k+1}: every fine column once;
    irregular  aggregates of 1..7 random fine unknowns; from 5 unknowns up a few fine columns belong to no aggregate
               and one coarse row is empty (empty rows in R and in its transpose);
    overlap    every fine column in 2 or 3 coarse rows: no scatter, the explicit transpose and ROW_AXPY;
    strided    aggregates {r, r + nc, ..., r + 7 nc} with nc = n // 8: every row has the same eight (column - row)
               offsets in the same stored order and one weight per offset, so R is row-pattern coded and the
               prolongation runs as a scatter over R's rows (ROW_SCATTER) — scatter_expected();
    strided_var  the same aggregates with a weight per entry: offset patterns with the values in the ELL array.
    Weights: integers {1, 2, 4}; reals standard normals rounded to float32."""
    n = fam.n
    rng = np.random.default_rng(_seed_of(fam, 10 + RESTRICTIONS.index(kind)))
    if kind == "pair":
        rows, cols = np.arange(n) // 2, np.arange(n)
        nc = (n + 1) // 2
    elif kind == "irregular":
        members = rng.permutation(n)
        if n >= 5:
            members = members[: n - max(1, n // 50)]            # the rest: fine unknowns without a parent
        sizes = []
        while sum(sizes) < members.size:
            sizes.append(min(int(rng.integers(1, 8)), members.size - sum(sizes)))
        rows = np.repeat(np.arange(len(sizes)), sizes)
        cols = members
        nc = len(sizes)
        if n >= 5:                                               # an empty coarse row in the middle
            gap = nc // 2
            rows = rows + (rows >= gap)
            nc += 1
    elif kind in ("strided", "strided_var"):
        nc = max(1, n // 8)
        js = rng.permutation(8)                                  # one stored order of the offsets for every row
        rows = np.repeat(np.arange(nc), 8)
        cols = rows + np.tile(js, nc) * nc
        which = np.tile(js, nc)
        rows, cols, which = rows[cols < n], cols[cols < n], which[cols < n]
        if integers:
            w = rng.choice([1.0, 2.0, 4.0], size=8 if kind == "strided" else rows.size)
        else:
            w = rng.standard_normal(8 if kind == "strided" else rows.size).astype(np.float32).astype(np.float64)
            w[w == 0.0] = 1.0
        if kind == "strided":
            w = w[which]
        R = sp.csr_matrix((w, cols.astype(np.int32), np.searchsorted(rows, np.arange(nc + 1)).astype(np.int32)), shape=(nc, n))
        R.has_sorted_indices = False
        return R
    else:
        nc = max(1, (n + 2) // 3)
        times = rng.integers(2, 4, size=n) if nc >= 3 else np.full(n, min(nc, 2))
        cols = np.repeat(np.arange(n), times)
        rows = np.concatenate([rng.choice(nc, size=int(t), replace=False) for t in times])
    order = rng.permutation(rows.size)                           # stored order inside a row: random
    order = order[np.argsort(rows[order], kind="stable")]
    rows, cols = rows[order], cols[order]
    if integers:
        w = rng.choice([1.0, 2.0, 4.0], size=rows.size)
    else:
        w = rng.standard_normal(rows.size).astype(np.float32).astype(np.float64)
        w[w == 0.0] = 1.0
    indptr = np.searchsorted(rows, np.arange(nc + 1)).astype(np.int32)
    R = sp.csr_matrix((w, cols.astype(np.int32), indptr), shape=(nc, n))
    R.has_sorted_indices = False
    return R


def scatter_expected(fam, kind, compress, pattern_kernel):
    """Does prolong_add over this restriction run as a scatter over R's rows?  hierarchy.hip build_format: when every
    block of R is row-pattern coded (and no fine column has two parents).  encode_csr codes a block so when the
    operator's average row exceeds 4 entries (256-row blocks), the block holds at least 64 entries, and its rows share
    a dictionary: the strided restrictions from 64 fine unknowns up, whose last block of nc % 256 rows has at least 8
    rows.  One weight per offset: patterns with values, walked by either kernel; a weight per entry: offset patterns
    with ELL values, which need OMG_COMPRESS's bit 8 and the pattern kernel on."""
    nc = max(1, fam.n // 8)
    bits = int(compress)                                         # OMG_COMPRESS: 4 = row patterns, 8 = offset patterns + ELL values
    if kind not in ("strided", "strided_var") or not bits & 4 or nc < 8 or 0 < nc % 256 < 8:
        return False
    return kind == "strided" or (bool(bits & 8) and pattern_kernel != "0")


def coarse_operator(nc):
    """A small strictly dominant coarsest operator (the lists route does not ask for the Galerkin product)."""
    return sp.csr_matrix(sp.diags([-np.ones(max(nc - 1, 0)), 4.0 * np.ones(nc), -np.ones(max(nc - 1, 0))], [-1, 0, 1]))


def integer_vectors(fam, nc):
    rng = np.random.default_rng(_seed_of(fam, 3))
    draw = lambda lo, hi, m: rng.integers(lo, hi + 1, size=m).astype(np.float64)
    return {"x": draw(-64, 64, fam.n), "b": draw(-1000, 1000, fam.n), "fine": draw(-64, 64, fam.n),
            "coarse": {k: draw(-64, 64, m) for k, m in nc.items()}}


def real_vectors(fam, nc):
    rng = np.random.default_rng(_seed_of(fam, 4))
    draw = lambda m: rng.standard_normal(m).astype(np.float32).astype(np.float64)
    out = {"x": draw(fam.n), "b": draw(fam.n), "fine": draw(fam.n), "coarse": {k: draw(m) for k, m in nc.items()}}
    # ... and a pair that is NOT float32-representable: a product of two float32-representable numbers is exact in double,
    # where a fused and an unfused row sum then agree; with these, float64 tells them apart too (float32 rounds them to
    # nearest at upload, on the device and in the restatement alike)
    out["xd"], out["bd"] = rng.standard_normal(fam.n), rng.standard_normal(fam.n)
    return out


def transpose_stored(R):
    """R^T as CSR (the order inside its rows is SciPy's, not necessarily the library's: use it where a row of the
    transpose holds one entry, or where the arithmetic is exact)."""
    return sp.csr_matrix(R.T)


# ----------------------------------------------------------- committed rows: the rule is observable --
# Found by search over float32 standard normals (the search compared the rational model's one-chain and four-chain
# sums) and committed as numbers.  ROW17: 17 stored entries whose one-chain and four-chain float32 sums differ, while
# the first 16 of them also differ between the two associations — so a kernel that ignored ASSOC_LEN on either side
# of the threshold gives other bits on this row.
ROW17_V = ["-0x1.529f56p+1", "-0x1.de873ap+0", "0x1.3756a4p-1", "0x1.68203cp+0", "0x1.a36630p-1", "0x1.c37366p-1",
           "0x1.8d3bb8p-6", "-0x1.53f70ap-1", "-0x1.286f5cp-3", "0x1.ce61a0p-1", "-0x1.3087d2p-1", "-0x1.2f0180p-2",
           "0x1.ab5deap+0", "-0x1.cc7326p-1", "-0x1.26a994p+0", "-0x1.3fb702p+0", "0x1.8985d8p-4"]
ROW17_X = ["-0x1.b7b620p-2", "-0x1.cbfbfap-1", "-0x1.e251b8p-1", "-0x1.073b88p-2", "-0x1.76d33ap-2", "-0x1.d76f50p-2",
           "0x1.f14202p-4", "-0x1.3ae534p+0", "-0x1.05fac4p+0", "-0x1.a81a0cp-1", "-0x1.b7dc92p+0", "0x1.fad902p-3",
           "0x1.044308p+1", "-0x1.0a4616p-4", "0x1.62b954p-1", "-0x1.843c28p-1", "0x1.2ccbb6p+0"]
ROW17_FOUR = "0x1.83c4d4p+2"      # the row's sum: four chains (17 > ASSOC_LEN)
ROW17_ONE = "0x1.83c4d2p+2"       # what one chain would give
PREFIX16_ONE = "0x1.7c8b4ap+2"    # the first 16 entries: one chain (16 <= ASSOC_LEN)
PREFIX16_FOUR = "0x1.7c8b4cp+2"   # what four chains would give
# JAC: a 1 x 1 system a x = b for which fma(omega, q, x) and x + fl(omega * q) differ in float32, omega = float32(0.7)
JAC_A, JAC_B, JAC_X = "-0x1.39d584p+0", "0x1.e10aa6p-6", "0x1.8f6c8ap+0"
JAC_FUSED, JAC_UNFUSED = "0x1.ce243cp-2", "0x1.ce2438p-2"


def from_hex(a):
    return np.array([float.fromhex(h) for h in a])
