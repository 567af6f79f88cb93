// Zebra line smoother for 5- / 7-point grid stencils with any coefficients (common.h LinePlan).  The grid lines along one
// axis are coloured by the parity of the sum of their other two indices; a sweep solves every line of colour 0, then every
// line of colour 1, exactly:  x_line <- T^-1 (b_line - sum of the cross couplings times x of the neighbouring lines),
// T the line's own tridiagonal block.  In a star stencil every neighbouring line has the other colour, so the lines of a
// colour are independent and the update is in place.  One launch per colour; no launch waits on anything.
//
// Layout.  The plan WRITES the level's ordering (two sets, one per colour), and it writes it in bundles of 64 lines with
// the lines of a bundle interleaved: cell i of the k-th line of colour c sits in slot
//     base[c] + (k / 64) * 64 * len + i * w + k % 64,      w = 64 (the last bundle: the lines that are left).
// Whatever axis the lines run along in the grid — the unit-stride one included —, in the level's numbering the 64 lines a
// wave holds lie side by side and their cells follow each other: one thread per line, adjacent lanes on adjacent lines,
// every access of the sweep (iterate, right-hand side, the per-cell arrays below, all indexed by slot) unit-stride across
// the wave, and the wave's whole walk one contiguous stream of len * w values per array.  (Interleaving ALL lines of a
// colour, stride nl[c], was measured first: at 128^3 every cell of a line then lies 64 KiB from the last one and a sweep
// took 350 us, latency after latency.)  The transposition a unit-stride line would otherwise need in every sweep — a pass
// through LDS — is made once, by the permutation at the host boundary; the row kernels (residual, restriction,
// prolongation) take the ordering like any other.
//
// Per cell, by slot: the cross couplings (4 in 3-D, 2 in 2-D; an absent neighbour: coefficient 0 on a valid slot), the
// line's super-diagonal u, and the factorisation of T computed once in double and rounded once to V — the pivots
// p_0 = d_0, p_i = d_i - l_i u_{i-1} / p_{i-1}, stored as 1 / p_i and f_i = l_i / p_{i-1} (f_0 = 0).
//   forward:  y_i = r_i - f_i y_{i-1}          (y kept in x)
//   back:     x_i = (y_i - u_i x_{i+1}) (1 / p_i)
// Only the one-fma recurrence is serial: the loads run a group of eight cells ahead of it (line_sweep_kernel).
//
// Periodic levels (OMG_SMOOTH_LINE_WRAP).  Across the lines a periodic axis only adds a wrapped coupling to the cross arrays
// and the seam lines to each other's nbr: the kernel is the same.  ALONG the lines the block is cyclic, M = tridiag(l, d, u)
// with M[0, m-1] = l_0 and M[m-1, 0] = u_{m-1}; its LU without pivoting has one fill column g (above the last pivot) and one
// fill row h (left of it), both per cell (LinePlan::fill_col, fill_row):
//   forward:  y_i = r_i - f_i y_{i-1},  S += h_i y_i   (i <= m-2);   y_{m-1} = r_{m-1} - S
//   back:     x_{m-1} = y_{m-1} / p_{m-1};   x_i = (y_i - u^_i x_{i+1} - g_i x_{m-1}) (1 / p_i)
// The arrays are written so that the two special cells need no branch: f_{m-1} = h_{m-1} = 0 (the walk leaves r_{m-1} in
// y and S complete, one subtraction follows it), upper holds u^ (u^_{m-2} with the fill merged, u^_{m-1} = 0), g_{m-2} =
// g_{m-1} = 0 — wherever cells m-2 and m-1 fall, in a whole group or in the ragged tail.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"

namespace omg {
namespace {

constexpr int LINE_BUNDLE = 64;       // lines whose cells lie side by side in the level's numbering: one wave's
constexpr int LINE_THREADS = 64;      // one wave per workgroup: a level has few lines (128^3: 8192 per colour), spread them over the CUs
constexpr int LINE_AHEAD = 8;         // cells per group: their loads and cross sums are formed a group ahead of the recurrence

template <typename V>
struct LineArgs {
    V *xs;                    // the iterate's slots of this colour: [len][nl]
    const V *xo;              // ... of the other colour: [len][onl] (only read)
    const V *b;               // right-hand side, this colour's slots
    const V *cross;           // [ncross][n]; offset to this colour's slots
    const V *upper, *inv_pivot, *factor;
    const int32_t *nbr;       // [ncross][nl]: the neighbouring line's rank among the other colour's lines
    size_t n;                 // stride between the cross-coupling arrays
    int nl, onl, len;
};

// ... of a cyclic line (CYCLIC = true): the fill row and the fill column follow.  The tridiagonal kernels keep LineArgs.
template <typename V>
struct LineArgsCyclic : LineArgs<V> {
    const V *fill_row, *fill_col;
};
template <typename V, bool CYCLIC>
using line_args_t = typename std::conditional<CYCLIC, LineArgsCyclic<V>, LineArgs<V>>::type;

__device__ __forceinline__ double line_fma(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float line_fma(float a, float b, float c) { return fmaf(a, b, c); }

// Where line k of a colour with nl lines starts and the stride between its cells (LinePlan: bundles of LINE_BUNDLE lines,
// [bundle][cell][lane]; the last bundle is as wide as the lines that are left)
__host__ __device__ __forceinline__ void line_place(int64_t k, int64_t nl, int64_t len, int64_t &first, int64_t &stride) {
    const int64_t bundle = k / LINE_BUNDLE;
    stride = nl - bundle * LINE_BUNDLE < LINE_BUNDLE ? nl - bundle * LINE_BUNDLE : LINE_BUNDLE;
    first = bundle * LINE_BUNDLE * len + k % LINE_BUNDLE;
}

// One thread per line.  Both passes run in groups of LINE_AHEAD cells, software-pipelined: every load of the NEXT group is
// issued (into registers of its own) before the recurrence walks the current group, and folded into right-hand sides after
// it, so the wave waits for memory once per group with the recurrence in between.  __builtin_amdgcn_sched_barrier keeps the
// three phases apart (left alone, the scheduler interleaves loads, waits and fmas to save registers — a wave has a CU to
// itself at these line counts: registers are free).
// CYCLIC: one more stream per pass (fill_row forward, fill_col backward) and one more fma per cell in each — the running
// sum S of h_i y_i, the term g_i x_{m-1}; the last cell's y and x are formed between the passes.
template <typename V, int NC, bool CYCLIC>
__global__ __launch_bounds__(LINE_THREADS) void line_sweep_kernel(const line_args_t<V, CYCLIC> a) {
    const int k = int(blockIdx.x) * LINE_THREADS + int(threadIdx.x);
    if (k >= a.nl) return;                                   // (a line count that is no multiple of the workgroup)
    int64_t first = 0, stride = 0;
    line_place(k, a.nl, a.len, first, stride);
    const size_t w = size_t(stride);
    V *const xs = a.xs + first;
    const V *const b = a.b + first, *const fac = a.factor + first, *const upper = a.upper + first, *const invp = a.inv_pivot + first;
    const V *cr[NC], *xo[NC];
    size_t wo[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        int64_t fo = 0, so = 0;
        line_place(a.nbr[size_t(m) * size_t(a.nl) + size_t(k)], a.onl, a.len, fo, so);
        xo[m] = a.xo + fo;
        wo[m] = size_t(so);
        cr[m] = a.cross + size_t(m) * a.n + first;
    }
    const V *frow = nullptr, *fcol = nullptr;
    if constexpr (CYCLIC) { frow = a.fill_row + first; fcol = a.fill_col + first; }
    const int groups = a.len / LINE_AHEAD;                    // whole groups; the rest (a ragged line length) cell by cell
    // r = b - sum_m cross_m x(neighbouring line m) of cell i
    auto rhs = [&](int i) {
        V acc = b[size_t(i) * w];
#pragma unroll
        for (int m = 0; m < NC; ++m) acc = line_fma(-cr[m][size_t(i) * w], xo[m][size_t(i) * wo[m]], acc);
        return acc;
    };
    // forward substitution
    V y = V(0);
    [[maybe_unused]] V fsum = V(0);                           // CYCLIC: S = sum of h_i y_i
    {
        V r[LINE_AHEAD], f[LINE_AHEAD];
        [[maybe_unused]] V h[LINE_AHEAD];
        if (groups > 0) {
#pragma unroll
            for (int u = 0; u < LINE_AHEAD; ++u) {
                r[u] = rhs(u); f[u] = fac[size_t(u) * w];
                if constexpr (CYCLIC) h[u] = frow[size_t(u) * w];
            }
        }
        for (int g = 0; g < groups; ++g) {
            V bn[LINE_AHEAD], fn[LINE_AHEAD], cn[LINE_AHEAD][NC], xn[LINE_AHEAD][NC];
            [[maybe_unused]] V hn[LINE_AHEAD];
            const bool more = g + 1 < groups;
            if (more) {
#pragma unroll
                for (int u = 0; u < LINE_AHEAD; ++u) {
                    const size_t i = size_t((g + 1) * LINE_AHEAD + u);
                    bn[u] = b[i * w];
                    fn[u] = fac[i * w];
                    if constexpr (CYCLIC) hn[u] = frow[i * w];
#pragma unroll
                    for (int m = 0; m < NC; ++m) { cn[u][m] = cr[m][i * w]; xn[u][m] = xo[m][i * wo[m]]; }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < LINE_AHEAD; ++u) {
                y = line_fma(-f[u], y, r[u]);
                if constexpr (CYCLIC) fsum = line_fma(h[u], y, fsum);
                xs[size_t(g * LINE_AHEAD + u) * w] = y;
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
#pragma unroll
                for (int u = 0; u < LINE_AHEAD; ++u) {
                    V acc = bn[u];
#pragma unroll
                    for (int m = 0; m < NC; ++m) acc = line_fma(-cn[u][m], xn[u][m], acc);
                    r[u] = acc;
                    f[u] = fn[u];
                    if constexpr (CYCLIC) h[u] = hn[u];
                }
            }
        }
        for (int i = groups * LINE_AHEAD; i < a.len; ++i) {
            y = line_fma(-fac[size_t(i) * w], y, rhs(i));
            if constexpr (CYCLIC) fsum = line_fma(frow[size_t(i) * w], y, fsum);
            xs[size_t(i) * w] = y;
        }
    }
    // CYCLIC: f and h of the last cell are zero, so the walk left y = r_{m-1} and S whole: y_{m-1} = r_{m-1} - S, and
    // x_{m-1}, which every cell of the back substitution needs
    [[maybe_unused]] V xlast = V(0);
    if constexpr (CYCLIC) {
        const size_t s = size_t(a.len - 1) * w;
        y -= fsum;
        xs[s] = y;
        xlast = y * invp[s];
    }
    // back substitution: the ragged cells first (they are the line's last), then the whole groups downwards
    V xv = V(0);
    for (int i = a.len; i > groups * LINE_AHEAD; --i) {
        const size_t s = size_t(i - 1) * w;
        if constexpr (CYCLIC) xv = line_fma(-upper[s], xv, line_fma(-fcol[s], xlast, xs[s])) * invp[s];
        else xv = line_fma(-upper[s], xv, xs[s]) * invp[s];
        xs[s] = xv;
    }
    {
        V yy[LINE_AHEAD], up[LINE_AHEAD], ip[LINE_AHEAD];
        [[maybe_unused]] V gc[LINE_AHEAD];
        if (groups > 0) {
#pragma unroll
            for (int u = 0; u < LINE_AHEAD; ++u) {
                const size_t s = size_t(groups * LINE_AHEAD - 1 - u) * w;
                yy[u] = xs[s]; up[u] = upper[s]; ip[u] = invp[s];
                if constexpr (CYCLIC) gc[u] = fcol[s];
            }
        }
        for (int g = groups; g > 0; --g) {
            V yn[LINE_AHEAD], un[LINE_AHEAD], pn[LINE_AHEAD];
            [[maybe_unused]] V gn[LINE_AHEAD];
            const bool more = g > 1;
            if (more) {
#pragma unroll
                for (int u = 0; u < LINE_AHEAD; ++u) {
                    const size_t s = size_t((g - 1) * LINE_AHEAD - 1 - u) * w;
                    yn[u] = xs[s]; un[u] = upper[s]; pn[u] = invp[s];
                    if constexpr (CYCLIC) gn[u] = fcol[s];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < LINE_AHEAD; ++u) {
                if constexpr (CYCLIC) xv = line_fma(-up[u], xv, line_fma(-gc[u], xlast, yy[u])) * ip[u];   // (the inner fma is off the serial chain)
                else xv = line_fma(-up[u], xv, yy[u]) * ip[u];
                xs[size_t(g * LINE_AHEAD - 1 - u) * w] = xv;
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
#pragma unroll
                for (int u = 0; u < LINE_AHEAD; ++u) {
                    yy[u] = yn[u]; up[u] = un[u]; ip[u] = pn[u];
                    if constexpr (CYCLIC) gc[u] = gn[u];
                }
            }
        }
    }
}

[[noreturn]] void line_unsupported(const std::string &why) {
    throw Error(OMG_ERR_UNSUPPORTED, "the line smoother needs a 5-point (2-D) or 7-point (3-D) stencil on a lexicographically numbered "
                                     "grid, every row holding exactly its in-grid neighbours in ascending column order: " + why);
}

// The grid of a star stencil, read off the couplings: the first row not coupled to its predecessor starts the second
// line, the first line not coupled to the previous one the second plane.
void line_grid(const omg_csr &A, int64_t &nx, int64_t &ny, int64_t &nz) {
    const int64_t n = A.n_rows;
    auto has = [&](int64_t r, int64_t c) {
        for (int64_t p = A.indptr[r]; p < A.indptr[r + 1]; ++p)
            if (A.indices[p] == c) return true;
        return false;
    };
    if (n < 4 || n != A.n_cols || n >= (int64_t(1) << 31)) line_unsupported("the level has " + std::to_string(n) + " rows");
    nx = n;
    for (int64_t r = 1; r < n; ++r)
        if (!has(r, r - 1)) { nx = r; break; }
    if (nx == n) line_unsupported("a 1-D grid (one line)");
    if (nx < 2 || n % nx) line_unsupported("no grid found (line length " + std::to_string(nx) + ")");
    const int64_t lines = n / nx;
    ny = lines;
    for (int64_t q = 1; q < lines; ++q)
        if (!has(q * nx, (q - 1) * nx)) { ny = q; break; }
    if (ny < 2 || lines % ny) line_unsupported("no grid found (" + std::to_string(ny) + " lines per plane)");
    nz = lines / ny;
}

// OMG_SMOOTH_LINE_WRAP: which axes of the grid are periodic on this level — axis a of extent e >= 3 and stride s is, if and
// only if row 0 holds column (e - 1) s.  (With e = 2 the two couplings are one in-grid entry: a coarse level's axis that
// was periodic above is an ordinary one.)  The scan of line_grid finds nx and ny on such a pattern as on any other: row nx
// holds nx - 1 and row ny nx holds (ny - 1) nx in neither.
void line_periodic(const omg_csr &A, int64_t nx, int64_t ny, int64_t nz, bool per[3]) {
    const int64_t ext[3] = {nx, ny, nz}, str[3] = {1, nx, nx * ny};
    for (int a = 0; a < 3; ++a) {
        per[a] = false;
        if (ext[a] < 3) continue;
        const int64_t c = (ext[a] - 1) * str[a];
        for (int64_t p = A.indptr[0]; p < A.indptr[1]; ++p)
            if (int64_t(A.indices[p]) == c) per[a] = true;
    }
}

}  // namespace

// The axis whose couplings of A have the largest sum of |a_ij| (0 = unit stride, 1, 2 = slowest); ties go to the smaller
// stride.  A is a grid stencil (line_grid), anything else: OMG_ERR_UNSUPPORTED.  wrap: a periodic axis' wrapped entries,
// |offset| = (e - 1) s, count towards it (1, nx - 1 < nx <= (ny - 1) nx < nx ny: the three ranges are disjoint).
int line_auto_axis(const omg_csr &A, bool wrap) {
    int64_t nx = 0, ny = 0, nz = 0;
    line_grid(A, nx, ny, nz);
    bool per[3] = {false, false, false};
    if (wrap) line_periodic(A, nx, ny, nz, per);
    double sum[3] = {0.0, 0.0, 0.0};
    const int64_t sj = nx, sk = nx * ny;
    for (int64_t r = 0; r < A.n_rows; ++r)
        for (int64_t p = A.indptr[r]; p < A.indptr[r + 1]; ++p) {
            const int64_t off = std::llabs(int64_t(A.indices[p]) - r);
            if (off == 1 || (per[0] && off == nx - 1)) sum[0] += std::fabs(A.data[p]);
            else if (off == sj || (per[1] && off == (ny - 1) * sj)) sum[1] += std::fabs(A.data[p]);
            else if ((off == sk || (per[2] && off == (nz - 1) * sk)) && nz > 1) sum[2] += std::fabs(A.data[p]);
        }
    int best = 0;
    for (int a = 1; a < (nz > 1 ? 3 : 2); ++a)
        if (sum[a] > sum[best]) best = a;
    return best;
}

template <typename V>
void LinePlan<V>::build(const omg_csr &A, int axis, Ordering &ord, hipStream_t s, bool wrap) {
    int64_t nx = 0, ny = 0, nz = 0;
    line_grid(A, nx, ny, nz);
    OMG_REQUIRE(axis >= 0 && axis <= 2, "line smoother: unknown axis");
    if (axis == 2 && nz == 1) throw Error(OMG_ERR_INVALID, "line smoother: lines along Z on a 2-D grid");
    const int64_t n = A.n_rows;
    const int64_t ext[3] = {nx, ny, nz}, str[3] = {1, nx, nx * ny};
    // the line's axis a, and the other two: q the faster, p the slower (2-D: p has one value)
    const int aq = axis == 0 ? 1 : 0, ap = axis == 2 ? 1 : 2;
    const int64_t len = ext[axis], Q = ext[aq], P = ext[ap];
    const int nc = P > 1 ? 4 : 2;
    g.nx = int(nx); g.ny = int(ny); g.nz = int(nz); g.axis = axis; g.len = int(len); g.ncross = nc;
    // OMG_SMOOTH_LINE_WRAP: the level's periodic axes.  Across the lines the seam lines q = 0 and q = Q - 1 are neighbours:
    // they must differ in colour, or the in-place sweep of that colour would race
    bool per[3] = {false, false, false};
    if (wrap) line_periodic(A, nx, ny, nz, per);
    for (int ax : {aq, ap})
        if (per[ax] && ext[ax] % 2)
            throw Error(OMG_ERR_UNSUPPORTED, std::string("line smoother: the periodic axis ") + "XYZ"[ax] + " across the lines has the odd extent " +
                                             std::to_string(ext[ax]) + " on this level (its two seam lines would have one colour): the depth or "
                                             "'coarsening' must keep periodic extents across the lines even on smoothed levels");
    g.cyclic = per[axis];
    // the lines' ranks within their colour, in the natural order of (p, q)
    std::vector<int32_t> rank(size_t(P * Q));
    int64_t cnt[2] = {0, 0};
    for (int64_t p = 0; p < P; ++p)
        for (int64_t q = 0; q < Q; ++q) rank[size_t(p * Q + q)] = int32_t(cnt[(p + q) & 1]++);
    g.nl[0] = cnt[0]; g.nl[1] = cnt[1];
    g.base[0] = 0; g.base[1] = len * cnt[0];
    OMG_REQUIRE(cnt[0] > 0 && cnt[1] > 0, "line smoother: internal: a colour without lines");
    // every row: exactly its in-grid neighbours, ascending columns; its coefficients into the slot arrays
    ord = Ordering();
    ord.identity = false;
    ord.perm.assign(size_t(n), 0);
    ord.inv.assign(size_t(n), 0);
    ord.sets = {0, g.base[1], n};
    std::vector<double> lower(size_t(n), 0.0), diag(size_t(n), 0.0), upper(size_t(n), 0.0), cross(size_t(nc) * size_t(n), 0.0);
    std::vector<int32_t> nbr(size_t(nc) * size_t(P * Q), 0);
    // the thirteen offsets a row can hold, ascending: the seven of the grid and, next to each off-diagonal one, the wrapped
    // neighbour of the other side ((e - 1) s lies between s and the next axis' stride).  A cell at the top of a periodic axis
    // holds its PLUS neighbour at -(e - 1) s, a cell at the bottom its MINUS neighbour at +(e - 1) s.
    const int64_t wr[3] = {(nx - 1) * str[0], (ny - 1) * str[1], (nz - 1) * str[2]};
    const int64_t off13[13] = {-wr[2], -str[2], -wr[1], -str[1], -wr[0], -1, 0, 1, wr[0], str[1], wr[1], str[2], wr[2]};
    // which slot of (lower, cross q-, cross q+, cross p-, cross p+, upper) each offset feeds: T_DIAG the diagonal
    enum { T_LOW = 0, T_UP = 1, T_Q0 = 2, T_Q1 = 3, T_P0 = 4, T_P1 = 5, T_DIAG = 6 };
    int role[13], ax13[13];
    bool wrapped[13], plus13[13];
    for (int e = 0; e < 13; ++e) {
        if (e == 6) { role[e] = T_DIAG; ax13[e] = -1; wrapped[e] = plus13[e] = false; continue; }
        const int ax = e < 6 ? 2 - e / 2 : (e - 7) / 2;    // the axis of offset e
        wrapped[e] = e % 2 == 0;                           // (0, 2, 4 and 8, 10, 12)
        const bool plus = (e > 6) != wrapped[e];           // the neighbour's side: a wrapped entry is the other side's
        ax13[e] = ax; plus13[e] = plus;
        role[e] = ax == axis ? (plus ? T_UP : T_LOW) : ax == aq ? (plus ? T_Q1 : T_Q0) : (plus ? T_P1 : T_P0);
    }
    const char *const held = wrap ? " grid does not hold exactly its in-grid neighbours (and, at a periodic axis' seam, the wrapped one)"
                                  : " grid does not hold exactly its in-grid neighbours";
    for (int64_t r = 0; r < n; ++r) {
        const int64_t c3[3] = {r % nx, (r / nx) % ny, r / (nx * ny)};
        const int64_t i = c3[axis], q = c3[aq], p = c3[ap];
        const int col = int((p + q) & 1);
        const int64_t k = rank[size_t(p * Q + q)];
        int64_t first = 0, stride = 0;
        line_place(k, g.nl[col], len, first, stride);
        const int64_t slot = g.base[col] + first + i * stride;
        ord.perm[size_t(slot)] = int32_t(r);
        ord.inv[size_t(r)] = int32_t(slot);
        int64_t e_p = A.indptr[r];
        const int64_t e_end = A.indptr[r + 1];
        for (int e = 0; e < 13; ++e) {
            if (e != 6) {
                const int64_t c = c3[ax13[e]], top = ext[ax13[e]] - 1;
                const bool present = wrapped[e] ? per[ax13[e]] && (plus13[e] ? c == top : c == 0) : (plus13[e] ? c < top : c > 0);
                if (!present) continue;
            }
            if (e_p >= e_end || int64_t(A.indices[e_p]) != r + off13[e])
                line_unsupported("row " + std::to_string(r) + " of a " + std::to_string(nx) + " x " + std::to_string(ny) + " x " +
                                 std::to_string(nz) + held);
            const double v = A.data[e_p++];
            switch (role[e]) {
                case T_DIAG: diag[size_t(slot)] = v; break;
                case T_LOW: lower[size_t(slot)] = v; break;
                case T_UP: upper[size_t(slot)] = v; break;
                default: cross[size_t(role[e] - T_Q0) * size_t(n) + size_t(slot)] = v; break;
            }
        }
        if (e_p != e_end)
            line_unsupported("row " + std::to_string(r) + " of a " + std::to_string(nx) + " x " + std::to_string(ny) + " x " +
                             std::to_string(nz) + " grid holds more than its in-grid neighbours");
        if (i == 0) {
            // the neighbouring lines' ranks (an absent one: rank 0 under a zero coefficient), by colour then [cross][line]
            const int64_t t = p * Q + q;
            const int64_t lo = col == 0 ? 0 : int64_t(nc) * g.nl[0];
            int32_t *const out = nbr.data() + lo;
            // (a periodic axis across the lines: the seam lines are each other's neighbours)
            out[0 * g.nl[col] + k] = q > 0 ? rank[size_t(t - 1)] : per[aq] ? rank[size_t(t + Q - 1)] : 0;
            out[1 * g.nl[col] + k] = q + 1 < Q ? rank[size_t(t + 1)] : per[aq] ? rank[size_t(t - (Q - 1))] : 0;
            if (nc == 4) {
                out[2 * g.nl[col] + k] = p > 0 ? rank[size_t(t - Q)] : per[ap] ? rank[size_t(t + (P - 1) * Q)] : 0;
                out[3 * g.nl[col] + k] = p + 1 < P ? rank[size_t(t + Q)] : per[ap] ? rank[size_t(t - (P - 1) * Q)] : 0;
            }
        }
    }
    // the factorisation of every line, in double
    std::vector<double> inv_p(lower.size(), 0.0), fac(lower.size(), 0.0);
    // cyclic lines: M = tridiag(l, d, u) with M[0, m-1] = l_0 and M[m-1, 0] = u_{m-1} (m >= 3).  LU without pivoting: rows
    // 1 .. m-2 as for the tridiagonal block; the corner l_0 fills column m-1 downwards (g), the corner u_{m-1} row m-1
    // rightwards (h), and both merge into the last 2 x 2: u^_{m-2}, h_{m-2}, p_{m-1}.  The arrays as the kernel wants them:
    // upper <- u^ with u^_{m-1} = 0, f_{m-1} = h_{m-1} = 0, g_{m-2} = g_{m-1} = 0.
    std::vector<double> frow, fcol, pv, gg, hh;
    if (g.cyclic) {
        OMG_REQUIRE(len >= 3, "line smoother: internal: a cyclic line of fewer than three cells");
        frow.assign(lower.size(), 0.0);
        fcol.assign(lower.size(), 0.0);
        pv.assign(size_t(len), 0.0); gg.assign(size_t(len), 0.0); hh.assign(size_t(len), 0.0);
    }
    for (int col = 0; g.cyclic && col < 2; ++col)
        for (int64_t k = 0; k < g.nl[col]; ++k) {
            int64_t first = 0, stride = 0;
            line_place(k, g.nl[col], len, first, stride);
            const int64_t m = len;
            auto sl = [&](int64_t i) { return size_t(g.base[col] + first + i * stride); };
            auto bad = [&](double piv) { return !(std::fabs(piv) > 0.0) || !std::isfinite(piv) || !std::isfinite(1.0 / piv); };
            auto refuse = [&](int64_t i) {
                throw Error(OMG_ERR_INVALID, "line smoother: zero or non-finite pivot in the cyclic line through row " + std::to_string(ord.perm[sl(i)]));
            };
            pv[0] = diag[sl(0)];
            if (bad(pv[0])) refuse(0);
            for (int64_t i = 1; i + 1 < m; ++i) {
                const double f = lower[sl(i)] / pv[size_t(i - 1)];
                pv[size_t(i)] = diag[sl(i)] - f * upper[sl(i - 1)];
                if (bad(pv[size_t(i)])) refuse(i);
                fac[sl(i)] = f;
            }
            gg[0] = lower[sl(0)];
            for (int64_t i = 1; i + 2 < m; ++i) gg[size_t(i)] = -fac[sl(i)] * gg[size_t(i - 1)];
            const double u_hat = upper[sl(m - 2)] - fac[sl(m - 2)] * gg[size_t(m - 3)];
            hh[0] = upper[sl(m - 1)] / pv[0];
            for (int64_t i = 1; i + 2 < m; ++i) hh[size_t(i)] = -hh[size_t(i - 1)] * upper[sl(i - 1)] / pv[size_t(i)];
            hh[size_t(m - 2)] = (lower[sl(m - 1)] - hh[size_t(m - 3)] * upper[sl(m - 3)]) / pv[size_t(m - 2)];
            double last = diag[sl(m - 1)], scale = std::fabs(last);
            for (int64_t i = 0; i + 2 < m; ++i) {
                last -= hh[size_t(i)] * gg[size_t(i)];
                scale += std::fabs(hh[size_t(i)] * gg[size_t(i)]);
            }
            last -= hh[size_t(m - 2)] * u_hat;
            scale += std::fabs(hh[size_t(m - 2)] * u_hat);
            // (a block that is singular — every cross coupling of the line zero and no shift — leaves here what rounding
            // left of zero: a last pivot below the rounding error of its own sum is no pivot)
            if (bad(last) || !(std::fabs(last) > 8.0 * double(m) * 2.220446049250313e-16 * scale)) refuse(m - 1);
            pv[size_t(m - 1)] = last;
            for (int64_t i = 0; i < m; ++i) {
                inv_p[sl(i)] = 1.0 / pv[size_t(i)];
                frow[sl(i)] = i + 1 < m ? hh[size_t(i)] : 0.0;
                fcol[sl(i)] = i + 2 < m ? gg[size_t(i)] : 0.0;
            }
            upper[sl(m - 2)] = u_hat;
            upper[sl(m - 1)] = 0.0;
            fac[sl(0)] = fac[sl(m - 1)] = 0.0;
        }
    for (int col = 0; !g.cyclic && col < 2; ++col)
        for (int64_t k = 0; k < g.nl[col]; ++k) {
            double piv = 0.0, u_prev = 0.0;
            int64_t first = 0, stride = 0;
            line_place(k, g.nl[col], len, first, stride);
            for (int64_t i = 0; i < len; ++i) {
                const size_t sl = size_t(g.base[col] + first + i * stride);
                const double f = i ? lower[sl] / piv : 0.0;
                piv = i ? diag[sl] - f * u_prev : diag[sl];
                if (!(std::fabs(piv) > 0.0) || !std::isfinite(piv) || !std::isfinite(1.0 / piv))
                    throw Error(OMG_ERR_INVALID, "line smoother: zero or non-finite pivot in the line through row " + std::to_string(ord.perm[sl]));
                fac[sl] = f;
                inv_p[sl] = 1.0 / piv;
                u_prev = upper[sl];
            }
        }
    auto put = [&](DevBuf<V> &dst, const std::vector<double> &src) {
        std::vector<V> tmp(src.size());
        for (size_t e = 0; e < src.size(); ++e) tmp[e] = V(src[e]);
        dst.alloc(src.size());
        dst.upload(tmp.data(), tmp.size(), s);
        OMG_HIP(hipStreamSynchronize(s));                     // (tmp dies here)
    };
    put(this->cross, cross);
    put(this->upper, upper);
    put(this->inv_pivot, inv_p);
    put(this->factor, fac);
    if (g.cyclic) {
        put(this->fill_row, frow);
        put(this->fill_col, fcol);
    }
    this->nbr.alloc(nbr.size());
    this->nbr.upload(nbr.data(), nbr.size(), s);
    OMG_HIP(hipStreamSynchronize(s));
}

template <typename V>
void LinePlan<V>::sweep(V *x, const V *b, hipStream_t s) const {
    const size_t n = size_t(g.base[1]) + size_t(g.len) * size_t(g.nl[1]);
    for (int col = 0; col < 2; ++col) {
        LineArgsCyclic<V> a;                                  // (the tridiagonal kernels take its base, LineArgs<V>)
        const size_t base = size_t(g.base[col]), obase = size_t(g.base[1 - col]);
        a.xs = x + base;
        a.xo = x + obase;
        a.b = b + base;
        a.cross = cross.p + base;
        a.upper = upper.p + base;
        a.inv_pivot = inv_pivot.p + base;
        a.factor = factor.p + base;
        a.nbr = nbr.p + (col == 0 ? size_t(0) : size_t(g.ncross) * size_t(g.nl[0]));
        a.n = n;
        a.nl = int(g.nl[col]);
        a.onl = int(g.nl[1 - col]);
        a.len = g.len;
        const unsigned blocks = unsigned((g.nl[col] + LINE_THREADS - 1) / LINE_THREADS);
        a.fill_row = g.cyclic ? fill_row.p + base : nullptr;
        a.fill_col = g.cyclic ? fill_col.p + base : nullptr;
        const LineArgs<V> &t = a;
        if (g.cyclic) {
            if (g.ncross == 4) hipLaunchKernelGGL((line_sweep_kernel<V, 4, true>), dim3(blocks), dim3(LINE_THREADS), 0, s, a);
            else hipLaunchKernelGGL((line_sweep_kernel<V, 2, true>), dim3(blocks), dim3(LINE_THREADS), 0, s, a);
        } else if (g.ncross == 4) hipLaunchKernelGGL((line_sweep_kernel<V, 4, false>), dim3(blocks), dim3(LINE_THREADS), 0, s, t);
        else hipLaunchKernelGGL((line_sweep_kernel<V, 2, false>), dim3(blocks), dim3(LINE_THREADS), 0, s, t);
        OMG_HIP(hipGetLastError());
    }
}

template struct LinePlan<double>;
template struct LinePlan<float>;

}  // namespace omg
