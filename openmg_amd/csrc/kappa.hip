// The 7-point operator of -div(kappa grad u) + sigma u from a cell-centred coefficient field in HBM:
// cell-centred finite volumes on a box of nz x ny x nx cells, kappa given with one ghost layer, (nz + 2)(ny + 2)(nx + 2)
// doubles in C order.  What the kernels write is the sorted CSR operators.stencil7_kappa assembles with SciPy, bit for bit
// — the in-grid neighbours of every row in ascending column order (-K, -J, -I, D, +I, +J, +K) — and with it the input of
// create_from_fine and omg_hierarchy_update_fine.
//
// Arithmetic (every operation rounded once in double; __dadd_rn / __dmul_rn / __ddiv_rn are never contracted):
//     face(a, b) = ((2 a) b) / (a + b)         c = face scale[axis]        off-diagonal: -c
//     diagonal   = (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K) (+ sigma)
// A Dirichlet wall face takes the ghost cell's kappa and enters the diagonal only; a Neumann wall face contributes +0.0.
//
// With per-axis cell widths (SPACED, DESIGN.md §5r: a tensor-product grid, the widths hz, hy, hx with one ghost entry at each
// end like kappa's ghost layer) the operator is the volume-integrated one; a, da the cell's own kappa and width along the
// face's axis, b, db the neighbour's:
//     c = (((2 a) b) / (da b + db a)) area[axis]       area_z = hy[j] hx[i], area_y = hz[k] hx[i], area_x = hz[k] hy[j]
//     diagonal = the same sum, then + sigma ((hz[k] hy[j]) hx[i])
// The widths are three small arrays in HBM, checked on the host before any launch; a workgroup is 256 consecutive rows, so
// hy[j], hz[k] and with them area_x are nearly wave-uniform and only hx varies per lane.  A Neumann wall face reads
// neither the ghost kappa nor the ghost width.
//
// The row start is a closed form — 7 r minus the absent neighbours of the rows before r —, so neither kernel scans and
// kappa_values needs no row pointers.  One thread per row, adjacent lanes on adjacent cells along x: kappa is read once
// per cell by its own thread, the six neighbours come through the cache (the +-I neighbours are the adjacent lanes' own
// loads, the +-J / +-K rows were or will be some other workgroup's).  Stores: a row holds 4 - 7 values, so a thread's own
// stores are 32 - 56 bytes apart from its neighbour's; the staged variant collects the workgroup's rows — one contiguous
// piece of the value array — in LDS and writes it out at unit stride.
//
// Periodic axes (PERIODIC, DESIGN.md §5s: both walls of an axis OMG_WALL_PERIODIC, extent >= 3): every row holds both
// neighbours along such an axis, the one across the seam being the cell at the other end of the line — the same face
// expression with that cell's kappa (and width), its address a select (i == 0 ? +(nx - 1) : -1), no ghost cell read.  The
// wrapped column is out of face order (at i = 0 the -I neighbour is column r + nx - 1, between +I and +J); since the
// offsets of the x, y and z neighbours lie in disjoint ranges (|x| <= nx - 1 < nx <= |y| <= (ny - 1) nx < nx ny <= |z|),
// the thirteen possible entries have ONE ascending order
//     +K wrapped, -K, +J wrapped, -J, +I wrapped, -I, D, +I, -I wrapped, +J, -J wrapped, +K, -K wrapped
// and an entry's slot is the number of present entries before it in that list: a running count over predicated stores.
// The row start stays a closed form: the "absent neighbour" terms of the periodic axes drop out.  These are instantiations
// of their own with the flags behind the arguments; the kernels without them keep their argument blocks and their code.
#include "common.h"

#include <cstring>
#include <map>
#include <mutex>

// (This file is compiled with -ffp-contract=off, the Makefile's rule for kappa.hip.o: __dmul_rn / __dadd_rn are plain
// operators defined in the compiler's header, out of a pragma's reach, and without the flag a product that feeds a sum
// — da b + db a, the diagonal plus sigma vol — becomes one fused operation, rounded once instead of twice.)

namespace omg {

namespace {

constexpr int KAPPA_BLOCK = 256;                      // rows per workgroup: at most 7 * 256 staged values (14 KiB of LDS)

struct KappaGrid { int nx, ny, nz; };

// entries of the rows before r = (k ny + j) nx + i: seven each, minus every neighbour that lies outside the grid
__device__ __forceinline__ int64_t row_start(const KappaGrid &g, int64_t r, int i, int j, int k) {
    const int64_t plane = int64_t(g.nx) * g.ny, in_plane = int64_t(j) * g.nx + i, lines = int64_t(k) * g.ny + j;
    int64_t absent = (r < plane ? r : plane);                                                  // -K: the rows of plane 0
    const int64_t top = r - int64_t(g.nz - 1) * plane;
    absent += top > 0 ? top : 0;                                                               // +K: the rows of the last plane
    absent += int64_t(k) * g.nx + (in_plane < g.nx ? in_plane : g.nx);                         // -J: the first line of every plane
    const int64_t lastj = in_plane - int64_t(g.ny - 1) * g.nx;
    absent += int64_t(k) * g.nx + (lastj > 0 ? lastj : 0);                                     // +J: the last line of every plane
    absent += lines + (i > 0 ? 1 : 0);                                                         // -I: the first cell of every line
    absent += lines;                                                                           // +I: the last cell of every line
    return 7 * r - absent;
}

// PERIODIC: per axis, whether its walls are periodic; row_start without the absent-neighbour terms of those axes
struct KappaWrap { int z, y, x; };

__device__ __forceinline__ int64_t row_start_wrap(const KappaGrid &g, const KappaWrap &wr, int64_t r, int i, int j, int k) {
    const int64_t plane = int64_t(g.nx) * g.ny, in_plane = int64_t(j) * g.nx + i, lines = int64_t(k) * g.ny + j;
    int64_t absent = 0;
    if (!wr.z) {
        const int64_t top = r - int64_t(g.nz - 1) * plane;
        absent += (r < plane ? r : plane) + (top > 0 ? top : 0);
    }
    if (!wr.y) {
        const int64_t lastj = in_plane - int64_t(g.ny - 1) * g.nx;
        absent += 2 * int64_t(k) * g.nx + (in_plane < g.nx ? in_plane : g.nx) + (lastj > 0 ? lastj : 0);
    }
    if (!wr.x) absent += 2 * lines + (i > 0 ? 1 : 0);
    return 7 * r - absent;
}

__device__ __forceinline__ int64_t nnz_wrap(const KappaGrid &g, const KappaWrap &wr) {
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    return 7 * n - 2 * ((wr.z ? 0 : int64_t(g.nx) * g.ny) + (wr.y ? 0 : int64_t(g.nx) * g.nz) + (wr.x ? 0 : int64_t(g.ny) * g.nz));
}

__device__ __forceinline__ void cell_of(const KappaGrid &g, int64_t r, int &i, int &j, int &k) {
    // (r < n < 2^31 / 7, KappaField::prepare: two 32-bit divisions instead of three 64-bit ones)
    const uint32_t line = uint32_t(r) / uint32_t(g.nx);
    i = int(uint32_t(r) - line * uint32_t(g.nx));
    k = int(line / uint32_t(g.ny));
    j = int(line - uint32_t(k) * uint32_t(g.ny));
}

// row pointers and columns; thread n writes indptr[n] = nnz
__global__ void __launch_bounds__(KAPPA_BLOCK) kappa_pattern_kernel(KappaGrid g, int32_t *indptr, int32_t *indices) {
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        indptr[n] = int32_t(7 * n - 2 * (int64_t(g.nx) * g.ny + int64_t(g.nx) * g.nz + int64_t(g.ny) * g.nz));
        return;
    }
    int i, j, k;
    cell_of(g, r, i, j, k);
    int64_t p = row_start(g, r, i, j, k);
    indptr[r] = int32_t(p);
    const int64_t sj = g.nx, sk = int64_t(g.nx) * g.ny;
    if (k > 0) indices[p++] = int32_t(r - sk);
    if (j > 0) indices[p++] = int32_t(r - sj);
    if (i > 0) indices[p++] = int32_t(r - 1);
    indices[p++] = int32_t(r);
    if (i + 1 < g.nx) indices[p++] = int32_t(r + 1);
    if (j + 1 < g.ny) indices[p++] = int32_t(r + sj);
    if (k + 1 < g.nz) indices[p++] = int32_t(r + sk);
}

// the same with periodic axes: the thirteen possible entries in ascending column order (the head of this file)
__global__ void __launch_bounds__(KAPPA_BLOCK) kappa_pattern_wrap_kernel(KappaGrid g, KappaWrap wr, int32_t *indptr, int32_t *indices) {
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        indptr[n] = int32_t(nnz_wrap(g, wr));
        return;
    }
    int i, j, k;
    cell_of(g, r, i, j, k);
    int64_t p = row_start_wrap(g, wr, r, i, j, k);
    indptr[r] = int32_t(p);
    const int64_t sj = g.nx, sk = int64_t(g.nx) * g.ny;
    const bool lo_i = i > 0, hi_i = i + 1 < g.nx, lo_j = j > 0, hi_j = j + 1 < g.ny, lo_k = k > 0, hi_k = k + 1 < g.nz;
    if (!hi_k && wr.z) indices[p++] = int32_t(r - (g.nz - 1) * sk);
    if (lo_k) indices[p++] = int32_t(r - sk);
    if (!hi_j && wr.y) indices[p++] = int32_t(r - (g.ny - 1) * sj);
    if (lo_j) indices[p++] = int32_t(r - sj);
    if (!hi_i && wr.x) indices[p++] = int32_t(r - (g.nx - 1));
    if (lo_i) indices[p++] = int32_t(r - 1);
    indices[p++] = int32_t(r);
    if (hi_i) indices[p++] = int32_t(r + 1);
    if (!lo_i && wr.x) indices[p++] = int32_t(r + (g.nx - 1));
    if (hi_j) indices[p++] = int32_t(r + sj);
    if (!lo_j && wr.y) indices[p++] = int32_t(r + (g.ny - 1) * sj);
    if (hi_k) indices[p++] = int32_t(r + sk);
    if (!lo_k && wr.z) indices[p++] = int32_t(r + (g.nz - 1) * sk);
}

struct KappaValuesArgs {
    KappaGrid g;
    const double *kappa;          // (nz + 2)(ny + 2)(nx + 2)
    const double *sigma;          // null: sigma_value (sigma_kind != 0); else one double (kind 1) or one per cell (kind 2)
    double sigma_value;
    int sigma_kind;               // OMG_SIGMA_*
    int neumann[6];               // -z, +z, -y, +y, -x, +x
    double scale[3];              // z, y, x
    double *data;
    unsigned long long *err;      // the smallest key of an offending value: 2 * (index in the padded field) + (1: sigma)
};

__device__ __forceinline__ bool kappa_ok(double v) { return v > 0.0 && v < HUGE_VAL; }
__device__ __forceinline__ bool sigma_ok(double v) { return v >= 0.0 && v < HUGE_VAL; }

__device__ __forceinline__ double face_of(double a, double b, double scale) {
    return __dmul_rn(__ddiv_rn(__dmul_rn(__dmul_rn(2.0, a), b), __dadd_rn(a, b)), scale);
}

// SPACED: the padded width arrays behind the unspaced arguments (whose kernels keep their argument block as it is)
struct KappaSpacedArgs : KappaValuesArgs {
    const double *hz, *hy, *hx;   // nz + 2, ny + 2, nx + 2
};
template <bool SPACED> using kappa_args_t = std::conditional_t<SPACED, KappaSpacedArgs, KappaValuesArgs>;

// PERIODIC: the per-axis flags behind either block
template <bool SPACED> struct KappaWrapArgs : kappa_args_t<SPACED> { KappaWrap wrap; };
template <bool SPACED, bool PERIODIC> using kappa_kernel_args_t = std::conditional_t<PERIODIC, KappaWrapArgs<SPACED>, kappa_args_t<SPACED>>;

__device__ __forceinline__ double face_spaced(double a, double b, double da, double db, double area) {
    const double den = __dadd_rn(__dmul_rn(da, b), __dmul_rn(db, a));
    return __dmul_rn(__ddiv_rn(__dmul_rn(__dmul_rn(2.0, a), b), den), area);
}

// the row of cell r: its values in CSR order to out[0 .. count), count returned
template <bool STAGED, bool SPACED, bool PERIODIC>
__global__ void __launch_bounds__(KAPPA_BLOCK) kappa_values_kernel(kappa_kernel_args_t<SPACED, PERIODIC> a) {
    __shared__ double stage[STAGED ? 7 * KAPPA_BLOCK : 1];
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r0 = blockIdx.x * int64_t(KAPPA_BLOCK);
    const int64_t r = r0 + threadIdx.x;
    int64_t base = 0;
    if (STAGED) {
        int i0, j0, k0;
        cell_of(g, r0, i0, j0, k0);
        if constexpr (PERIODIC) base = row_start_wrap(g, a.wrap, r0, i0, j0, k0);
        else base = row_start(g, r0, i0, j0, k0);
    }
    if (r < n) {
        int i, j, k;
        cell_of(g, r, i, j, k);
        const int64_t px = g.nx + 2, pxy = px * (g.ny + 2);
        const int64_t c = int64_t(k + 1) * pxy + int64_t(j + 1) * px + (i + 1);
        const double kc = a.kappa[c];
        unsigned long long bad = ~0ull;
        if (!kappa_ok(kc)) bad = 2ull * (unsigned long long)c;
        // the six faces in the order of the diagonal's sum: -K, -J, -I, +I, +J, +K
        const int64_t off[6] = {-pxy, -px, -1, 1, px, pxy};
        const bool inside[6] = {k > 0, j > 0, i > 0, i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
        const int wall[6] = {0, 2, 4, 5, 3, 1};
        const int axis[6] = {0, 1, 2, 2, 1, 0};
        // SPACED: the cell's own widths (z, y, x), the areas of its faces by axis, and its neighbours' widths by face
        const double *hp[3] = {nullptr, nullptr, nullptr};
        double own[3] = {0.0, 0.0, 0.0}, area[3] = {0.0, 0.0, 0.0};
        if constexpr (SPACED) {
            hp[0] = a.hz + (k + 1); hp[1] = a.hy + (j + 1); hp[2] = a.hx + (i + 1);
            own[0] = *hp[0]; own[1] = *hp[1]; own[2] = *hp[2];
            area[0] = __dmul_rn(own[1], own[2]); area[1] = __dmul_rn(own[0], own[2]); area[2] = __dmul_rn(own[0], own[1]);
        }
        const int step[6] = {-1, -1, -1, 1, 1, 1};
        // PERIODIC: a face on a periodic wall takes the cell at the other end of its line, `across` cells away (a select of
        // the offset; never a ghost)
        bool wrapped[6] = {false, false, false, false, false, false};
        int across[3] = {0, 0, 0};
        if constexpr (PERIODIC) {
            const int periodic[3] = {a.wrap.z, a.wrap.y, a.wrap.x};
#pragma unroll
            for (int e = 0; e < 6; ++e) wrapped[e] = !inside[e] && periodic[axis[e]];
            across[0] = g.nz - 1; across[1] = g.ny - 1; across[2] = g.nx - 1;
        }
        double w[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            if constexpr (PERIODIC) {
                const bool ghost = !inside[e] && !wrapped[e];
                if (ghost && a.neumann[wall[e]]) { w[e] = 0.0; continue; }
                const int st = wrapped[e] ? -step[e] * across[axis[e]] : step[e];
                const int64_t at = c + (wrapped[e] ? -off[e] * across[axis[e]] : off[e]);
                const double kn = a.kappa[at];
                if (ghost && !kappa_ok(kn)) {
                    const unsigned long long key = 2ull * (unsigned long long)at;
                    bad = key < bad ? key : bad;
                }
                if constexpr (SPACED) w[e] = face_spaced(kc, kn, own[axis[e]], hp[axis[e]][st], area[axis[e]]);
                else w[e] = face_of(kc, kn, a.scale[axis[e]]);
            } else {
                if (!inside[e] && a.neumann[wall[e]]) { w[e] = 0.0; continue; }
                const double kn = a.kappa[c + off[e]];
                // (an inner neighbour is checked by its own thread; a ghost cell by the thread of the cell it bounds)
                if (!inside[e] && !kappa_ok(kn)) {
                    const unsigned long long key = 2ull * (unsigned long long)(c + off[e]);
                    bad = key < bad ? key : bad;
                }
                if constexpr (SPACED) w[e] = face_spaced(kc, kn, own[axis[e]], hp[axis[e]][step[e]], area[axis[e]]);
                else w[e] = face_of(kc, kn, a.scale[axis[e]]);
            }
        }
        double d = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(w[0], w[1]), w[2]), w[3]), w[4]), w[5]);
        if (a.sigma_kind != OMG_SIGMA_NONE) {
            const double s = a.sigma ? a.sigma[a.sigma_kind == OMG_SIGMA_FIELD ? r : 0] : a.sigma_value;
            if (!sigma_ok(s)) {
                const unsigned long long key = 2ull * (unsigned long long)c + 1ull;
                bad = key < bad ? key : bad;
            }
            if constexpr (SPACED) d = __dadd_rn(d, __dmul_rn(s, __dmul_rn(__dmul_rn(own[0], own[1]), own[2])));
            else d = __dadd_rn(d, s);
        }
        if (bad != ~0ull) atomicMin(a.err, bad);
        int64_t p;
        if constexpr (PERIODIC) p = row_start_wrap(g, a.wrap, r, i, j, k);
        else p = row_start(g, r, i, j, k);
        double *out = STAGED ? stage + (p - base) : a.data + p;
        int q = 0;
        // (PERIODIC: before an inner entry comes the wrapped one of the opposite face, whose column lies further down; after it, further up)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if constexpr (PERIODIC)
                if (wrapped[5 - e]) out[q++] = -w[5 - e];
            if (inside[e]) out[q++] = -w[e];
        }
        out[q++] = d;
#pragma unroll
        for (int e = 3; e < 6; ++e) {
            if (inside[e]) out[q++] = -w[e];
            if constexpr (PERIODIC)
                if (wrapped[5 - e]) out[q++] = -w[5 - e];
        }
    }
    if (STAGED) {
        __syncthreads();
        const int64_t r1 = r0 + KAPPA_BLOCK < n ? r0 + KAPPA_BLOCK : n;
        int64_t end;
        if (r1 == n) {
            if constexpr (PERIODIC) end = nnz_wrap(g, a.wrap);
            else end = 7 * n - 2 * (int64_t(g.nx) * g.ny + int64_t(g.nx) * g.nz + int64_t(g.ny) * g.nz);
        } else {
            int i1, j1, k1;
            cell_of(g, r1, i1, j1, k1);
            if constexpr (PERIODIC) end = row_start_wrap(g, a.wrap, r1, i1, j1, k1);
            else end = row_start(g, r1, i1, j1, k1);
        }
        const int count = int(end - base);                      // <= 7 * KAPPA_BLOCK
        for (int t = threadIdx.x; t < count; t += KAPPA_BLOCK) a.data[base + t] = stage[t];
    }
}

// OMG_KAPPA_STAGE=0|1: the workgroup's values straight from the threads, or through LDS at unit stride (the default: DESIGN.md §5q)
bool kappa_staged() {
    static const bool v = [] { const char *e = getenv("OMG_KAPPA_STAGE"); return !(e && e[0] == '0'); }();
    return v;
}

bool finite_pos(double v) { return v > 0.0 && v < HUGE_VAL; }

}  // namespace

int64_t KappaField::nnz() const {
    return 7 * rows() - 2 * ((periodic[0] ? 0 : int64_t(nx) * ny) + (periodic[1] ? 0 : int64_t(nx) * nz) + (periodic[2] ? 0 : int64_t(ny) * nz));
}

void KappaField::prepare(const KappaInput &in, hipStream_t s) {
    const int64_t *const shape = in.shape;
    const int *const walls = in.walls;
    const double *const kappa = in.kappa, *const sigma = in.sigma, *const hz = in.hz, *const hy = in.hy, *const hx = in.hx;
    const int kind = in.sigma_kind;
    OMG_REQUIRE(shape && kappa, "kappa: null argument");
    for (int d = 0; d < 3; ++d)
        OMG_REQUIRE(shape[d] >= 1 && shape[d] < (int64_t(1) << 30), "kappa: every extent of the shape must be >= 1");
    nz = int(shape[0]); ny = int(shape[1]); nx = int(shape[2]);
    const int64_t padded = int64_t(nz + 2) * (ny + 2) * (nx + 2);
    OMG_REQUIRE(7 * int64_t(nx) * ny * nz < (int64_t(1) << 31) - 1 && padded < (int64_t(1) << 31) - 1,
                "kappa: operator too large for int32 indices");
    for (int f = 0; f < 6; ++f) {
        const int wv = walls ? walls[f] : OMG_WALL_DIRICHLET;
        OMG_REQUIRE(wv == OMG_WALL_DIRICHLET || wv == OMG_WALL_NEUMANN || wv == OMG_WALL_PERIODIC,
                    "kappa: a wall must be OMG_WALL_DIRICHLET or OMG_WALL_NEUMANN, or OMG_WALL_PERIODIC on both walls of an axis");
        neumann[f] = wv == OMG_WALL_NEUMANN;
    }
    // a periodic axis: both of its walls, and three distinct columns (the cell and its two neighbours) in every row
    for (int d = 0; d < 3; ++d) {
        static const char *const axis_name[3] = {"z", "y", "x"};
        const bool lo = walls && walls[2 * d] == OMG_WALL_PERIODIC, hi = walls && walls[2 * d + 1] == OMG_WALL_PERIODIC;
        periodic[d] = lo && hi;
        if (lo != hi)
            throw Error(OMG_ERR_INVALID, std::string("kappa: OMG_WALL_PERIODIC must be given for both walls of an axis: only one wall of axis ") +
                                             axis_name[d] + " has it");
        if (periodic[d] && shape[d] < 3)
            throw Error(OMG_ERR_INVALID, std::string("kappa: a periodic axis needs an extent >= 3: axis ") + axis_name[d] + " has " +
                                             std::to_string((long long)shape[d]));
    }
    for (int d = 0; d < 3; ++d) {
        scale[d] = in.scale ? in.scale[d] : 1.0;
        OMG_REQUIRE(finite_pos(scale[d]), "kappa: every scale factor must be finite and > 0");
    }
    // the cell widths: all three axes or none, in place of the scale factors; checked here, before any launch
    OMG_REQUIRE((!hz && !hy && !hx) || (hz && hy && hx), "kappa: the widths hz, hy, hx are given together or not at all");
    spaced = hz != nullptr;
    if (spaced) {
        OMG_REQUIRE(scale[0] == 1.0 && scale[1] == 1.0 && scale[2] == 1.0, "kappa: widths and scale factors exclude each other");
        const double *const h[3] = {hz, hy, hx};
        const int extent[3] = {nz, ny, nx};
        static const char *const axis_name[3] = {"z", "y", "x"};
        for (int d = 0; d < 3; ++d)
            for (int m = 0; m < extent[d] + 2; ++m) {
                const double v = h[d][m];
                const bool ghost = m == 0 || m == extent[d] + 1;
                if (v < HUGE_VAL && (ghost ? v >= 0.0 : v > 0.0)) continue;
                throw Error(OMG_ERR_INVALID, std::string("kappa: the width along ") + axis_name[d] + " at index " + std::to_string(m - 1) +
                                                 (ghost ? " (a ghost entry) is not finite and >= 0" : " is not finite and > 0"));
            }
        widths.alloc(size_t(nz) + ny + nx + 6);
        size_t at = 0;
        for (int d = 0; d < 3; ++d) {
            OMG_HIP(hipMemcpyAsync(widths.p + at, h[d], size_t(extent[d] + 2) * sizeof(double), hipMemcpyHostToDevice, s));
            at += size_t(extent[d] + 2);
        }
    }
    OMG_REQUIRE(kind == OMG_SIGMA_NONE || kind == OMG_SIGMA_SCALAR || kind == OMG_SIGMA_FIELD, "kappa: sigma_kind must be one of OMG_SIGMA_*");
    OMG_REQUIRE(kind == OMG_SIGMA_NONE || sigma, "kappa: sigma is null");
    sigma_kind = kind;
    sigma_dev = nullptr;
    sigma_value = 0.0;
    if (kind == OMG_SIGMA_SCALAR && !in.sigma_on_device) {
        sigma_value = sigma[0];
        OMG_REQUIRE(sigma_value >= 0.0 && sigma_value < HUGE_VAL, "kappa: sigma must be finite and >= 0");
    } else if (kind != OMG_SIGMA_NONE) {
        if (in.sigma_on_device) {
            sigma_dev = sigma;
        } else {
            own_sigma.alloc(size_t(nx) * ny * nz);
            own_sigma.upload(sigma, size_t(nx) * ny * nz, s);
            sigma_dev = own_sigma.p;
        }
    }
    if (in.kappa_on_device) {
        kappa_dev = kappa;
    } else {
        own_kappa.alloc(size_t(padded));
        own_kappa.upload(kappa, size_t(padded), s);
        kappa_dev = own_kappa.p;
    }
    if (!err.p) err.alloc(1);
}

namespace {

// the launch of one instantiation: its argument block filled from the field
template <bool STAGED, bool SPACED, bool PERIODIC>
void launch_values(const KappaField &F, double *data, hipStream_t s) {
    kappa_kernel_args_t<SPACED, PERIODIC> a;
    a.g = {F.nx, F.ny, F.nz};
    a.kappa = F.kappa_dev;
    a.sigma = F.sigma_dev;
    a.sigma_value = F.sigma_value;
    a.sigma_kind = F.sigma_kind;
    for (int f = 0; f < 6; ++f) a.neumann[f] = F.neumann[f];
    for (int d = 0; d < 3; ++d) a.scale[d] = F.scale[d];
    a.data = data;
    a.err = F.err.p;
    if constexpr (SPACED) {
        a.hz = F.widths.p;
        a.hy = F.widths.p + (F.nz + 2);
        a.hx = F.widths.p + (F.nz + 2) + (F.ny + 2);
    }
    if constexpr (PERIODIC) a.wrap = {F.periodic[0], F.periodic[1], F.periodic[2]};
    const dim3 grid((unsigned)((F.rows() + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    hipLaunchKernelGGL((kappa_values_kernel<STAGED, SPACED, PERIODIC>), grid, dim3(KAPPA_BLOCK), 0, s, a);
}

// f(std::true_type) or f(std::false_type): a run-time flag as a compile-time constant
template <typename F>
void as_constant(bool flag, F &&f) {
    if (flag) f(std::true_type());
    else f(std::false_type());
}

}  // namespace

void KappaField::values(double *data, hipStream_t s, const char *entry) {
    OMG_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(unsigned long long), s));
    as_constant(kappa_staged(), [&](auto staged) {
        as_constant(spaced, [&](auto sp) {
            as_constant(any_periodic(), [&](auto wrap) { launch_values<decltype(staged)::value, decltype(sp)::value, decltype(wrap)::value>(*this, data, s); });
        });
    });
    OMG_HIP(hipGetLastError());
    unsigned long long e = ~0ull;
    OMG_HIP(hipMemcpyAsync(&e, err.p, sizeof(e), hipMemcpyDeviceToHost, s));
    OMG_HIP(hipStreamSynchronize(s));
    if (e == ~0ull) return;
    // the key names a cell of the padded field: as a cell of the grid, a ghost cell has a coordinate of -1 or the extent
    const int64_t c = int64_t(e >> 1), px = nx + 2, pxy = px * (ny + 2);
    const long long z = (long long)(c / pxy) - 1, y = (long long)((c / px) % (ny + 2)) - 1, x = (long long)(c % px) - 1;
    const std::string cell = "cell (" + std::to_string(z) + ", " + std::to_string(y) + ", " + std::to_string(x) + ")";
    if (e & 1) throw Error(OMG_ERR_INVALID, std::string(entry) + ": sigma at " + cell + " is not finite and >= 0");
    throw Error(OMG_ERR_INVALID, std::string(entry) + ": kappa at " + cell + " is not finite and > 0");
}

namespace {

// row pointers and columns of the 7-point pattern on a grid, with the wrapped columns of its periodic axes (z, y, x)
void launch_pattern(const KappaGrid &g, const int *periodic, int32_t *indptr, int32_t *indices, hipStream_t s) {
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const dim3 grid((unsigned)((n + 1 + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    if (periodic[0] || periodic[1] || periodic[2]) {
        const KappaWrap wr = {periodic[0], periodic[1], periodic[2]};
        hipLaunchKernelGGL(kappa_pattern_wrap_kernel, grid, dim3(KAPPA_BLOCK), 0, s, g, wr, indptr, indices);
    } else {
        hipLaunchKernelGGL(kappa_pattern_kernel, grid, dim3(KAPPA_BLOCK), 0, s, g, indptr, indices);
    }
    OMG_HIP(hipGetLastError());
}

}  // namespace

void KappaField::assemble(int32_t *indptr, int32_t *indices, double *data, hipStream_t s, const char *entry) {
    if (indptr) launch_pattern({nx, ny, nz}, periodic, indptr, indices, s);
    values(data, s, entry);
}

void KappaField::assemble(DevCsrPlain &A, hipStream_t s, const char *entry) {
    A.n_rows = A.n_cols = rows();
    A.nnz = nnz();
    A.indptr.alloc(size_t(A.n_rows) + 1);
    A.indices.alloc(size_t(A.nnz));
    A.data.alloc(size_t(A.nnz));
    assemble(A.indptr.p, A.indices.p, A.data.p, s, entry);
}

// ---- the right-hand side that goes with the operator (operators.rhs_kappa is the definition) ---------------
// b = ((((((volume term + t-K) + t-J) + t-I) + t+I) + t+J) + t+K): the source f (times the cell volume when SPACED) and, for
// a cell at a wall that carries a value, c_wall g (Dirichlet: c_wall the face coefficient kappa_values_kernel added to the
// diagonal, the same expression) or q area / q scale (Neumann: the outward flux).  One thread per cell, 256 consecutive cells
// per workgroup as above: f is read and b written at unit stride, 16 bytes per cell; a lane that is not on a wall with a value
// reads nothing else (the widths only where the volume needs them).  Lanes on such a wall read their own and the ghost kappa,
// the ghost width and the value: whole workgroups of them on the z walls, one lane per line on the x walls — the branch is
// short (one division) and the launch is bound by the stream, not by it.  b may be f: each thread reads its own f first.
namespace {

struct KappaRhsArgs {
    KappaGrid g;
    const double *__restrict__ kappa;   // (nz + 2)(ny + 2)(nx + 2); read only at Dirichlet walls with a value
    double f_value;
    int f_kind;                         // OMG_VALUE_*
    int kind[6];                        // per wall -z, +z, -y, +y, -x, +x: OMG_VALUE_* (a periodic wall: NONE)
    int neumann[6];
    double value[6];
    const double *__restrict__ field[6];   // one per face of the wall: (ny, nx), (nz, nx), (nz, ny)
    double scale[3];                    // z, y, x
};
struct KappaRhsSpacedArgs : KappaRhsArgs {
    const double *__restrict__ hz, *__restrict__ hy, *__restrict__ hx;   // nz + 2, ny + 2, nx + 2
};
template <bool SPACED> using kappa_rhs_args_t = std::conditional_t<SPACED, KappaRhsSpacedArgs, KappaRhsArgs>;

// f (F_FIELD: one per cell; else null) and b are arguments of their own — the two streams of the launch, plain global
// pointers that may be one array — and the thread's f is asked for before anything else, so that the index arithmetic runs
// under the load.  (F_FIELD is a template flag, not a test of a.f_kind: the compiler turns `kind == FIELD ? f[r] : f_value`
// into ONE load through a select of the two addresses — global memory and the argument block —, a flat load.)
template <bool SPACED, bool F_FIELD>
__global__ void __launch_bounds__(KAPPA_BLOCK) kappa_rhs_kernel(kappa_rhs_args_t<SPACED> a, const double *f, double *b) {
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r >= n) return;
    double v;
    if constexpr (F_FIELD) v = f[r];
    else v = a.f_value;                                // (the scalar; +0.0 for no f)
    int i, j, k;
    cell_of(g, r, i, j, k);
    // the six faces in the order of the sum: -K, -J, -I, +I, +J, +K
    const bool inside[6] = {k > 0, j > 0, i > 0, i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
    const int wall[6] = {0, 2, 4, 5, 3, 1};
    const int axis[6] = {0, 1, 2, 2, 1, 0};
    bool valued[6], on_wall = false;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        valued[e] = !inside[e] && a.kind[wall[e]] != OMG_VALUE_NONE;
        on_wall = on_wall || valued[e];
    }
    double own[3] = {0.0, 0.0, 0.0}, area[3] = {0.0, 0.0, 0.0};
    if constexpr (SPACED) {
        if (on_wall || a.f_kind != OMG_VALUE_NONE) {
            own[0] = a.hz[k + 1]; own[1] = a.hy[j + 1]; own[2] = a.hx[i + 1];
        }
    }
    if constexpr (SPACED) {
        if (a.f_kind != OMG_VALUE_NONE) v = __dmul_rn(v, __dmul_rn(__dmul_rn(own[0], own[1]), own[2]));
    }
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (on_wall) {
        if constexpr (SPACED) {
            area[0] = __dmul_rn(own[1], own[2]); area[1] = __dmul_rn(own[0], own[2]); area[2] = __dmul_rn(own[0], own[1]);
        }
        const int64_t px = g.nx + 2, pxy = px * (g.ny + 2);
        const int64_t c = int64_t(k + 1) * pxy + int64_t(j + 1) * px + (i + 1);
        const int64_t off[6] = {-pxy, -px, -1, 1, px, pxy};
        // the cell's face on a z, y, x wall: (j, i) of (ny, nx), (k, i) of (nz, nx), (k, j) of (nz, ny)
        const int64_t at[3] = {int64_t(j) * g.nx + i, int64_t(k) * g.nx + i, int64_t(k) * g.ny + j};
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            if (!valued[e]) continue;
            const int w = wall[e], ax = axis[e];
            double val = a.value[w];
            if (a.kind[w] == OMG_VALUE_FIELD) val = a.field[w][at[ax]];
            if (a.neumann[w]) {
                t[e] = __dmul_rn(val, SPACED ? area[ax] : a.scale[ax]);
                continue;
            }
            const double kc = a.kappa[c], kn = a.kappa[c + off[e]];
            double coeff;
            if constexpr (SPACED) {
                const double *const h = ax == 0 ? a.hz + (k + 1) : ax == 1 ? a.hy + (j + 1) : a.hx + (i + 1);
                coeff = face_spaced(kc, kn, own[ax], h[e < 3 ? -1 : 1], area[ax]);
            } else {
                coeff = face_of(kc, kn, a.scale[ax]);
            }
            t[e] = __dmul_rn(coeff, val);
        }
    }
    b[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(v, t[0]), t[1]), t[2]), t[3]), t[4]), t[5]);
}

// ---- the face fluxes of a solution (operators.flux_kappa is the definition) --------------------------------
// F = the flux of -kappa grad u along the +axis through every face, with the operator's own factor (scale[axis], or the face
// area with widths): Fz (nz + 1, ny, nx), Fy (nz, ny + 1, nx), Fx (nz, ny, nx + 1) in C order.  Face m of an axis of extent e
// lies between cell m - 1 (lo) and cell m (hi):
//     in the grid       F = c (u_lo - u_hi)      c = face(kappa_lo, kappa_hi[, d_lo, d_hi, area]): the bits of -A[lo, hi]
//     a periodic seam   faces 0 and e, both   c (u_{e-1} - u_0)   with c of the cells e - 1 and 0; no ghost is read
//     a Dirichlet wall  F[0] = c_wall (g - u_0),  F[e] = c_wall (u_{e-1} - g)     c_wall kappa_rhs_kernel's, g = +0.0 without a value
//     a Neumann wall    +0.0 without a value and nothing read; else t = value area[axis] (value scale[axis]): F[0] = t, F[e] = -t
// One thread per cell, 256 consecutive cells per workgroup as above.  The thread owns the three LOW faces of its cell, so
// every face is computed once; the cells of the last layer along an axis write that axis's high face too (a wall face), and
// at a periodic seam the thread of cell 0 writes face e with the value of face 0.  With r the cell's number the low faces
// are Fz[r], Fy[r + k nx], Fx[r + k ny + j]: three streams written at unit stride along x; a high face lies nx ny, nx or 1
// further on, the seam's face e extent times that.  Read: the thread's own kappa and u, and those of its three lower
// neighbours — the -I neighbour is the adjacent lane's own load, the -J and -K neighbours' lines were some other lane's own
// loads nx and nx ny cells ago and come out of the caches (as the six neighbours of kappa_values_kernel do; no LDS, no
// barrier: a workgroup is a piece of a LINE, not a tile, and a tile's halo would be read through the same caches).
// ACCUMULATE: out = out + alpha F, one multiplication and one addition per face, every place with its own old value.
struct KappaFluxArgs {
    KappaGrid g;
    KappaWrap wrap;                        // per axis z, y, x: periodic (read by the PERIODIC instantiations)
    const double *__restrict__ kappa;      // (nz + 2)(ny + 2)(nx + 2)
    const double *__restrict__ u;          // nz ny nx
    int kind[6];                           // per wall -z, +z, -y, +y, -x, +x: OMG_VALUE_* (a periodic wall: NONE)
    int neumann[6];
    double value[6];
    const double *__restrict__ field[6];   // one per face of the wall: (ny, nx), (nz, nx), (nz, ny)
    double scale[3];                       // z, y, x
    double alpha;                          // ACCUMULATE
    double *fz, *fy, *fx;
};
struct KappaFluxSpacedArgs : KappaFluxArgs {
    const double *__restrict__ hz, *__restrict__ hy, *__restrict__ hx;   // nz + 2, ny + 2, nx + 2
};
template <bool SPACED> using kappa_flux_args_t = std::conditional_t<SPACED, KappaFluxSpacedArgs, KappaFluxArgs>;

template <bool ACCUMULATE>
__device__ __forceinline__ void put_face(double *out, int64_t at, double v, double alpha) {
    if constexpr (ACCUMULATE) out[at] = __dadd_rn(out[at], __dmul_rn(alpha, v));
    else out[at] = v;
}

template <bool SPACED, bool PERIODIC, bool ACCUMULATE>
__global__ void __launch_bounds__(KAPPA_BLOCK) kappa_flux_kernel(kappa_flux_args_t<SPACED> a) {
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r >= n) return;
    const double uc = a.u[r];
    int i, j, k;
    cell_of(g, r, i, j, k);
    const int64_t px = g.nx + 2, pxy = px * (g.ny + 2);
    const int64_t c = int64_t(k + 1) * pxy + int64_t(j + 1) * px + (i + 1);
    const double kc = a.kappa[c];
    // by axis z, y, x: the cell's coordinate, the extent, the step to the next cell in kappa, and in u — which is the step
    // to the next face of that axis in its face array too
    const int coord[3] = {k, j, i}, extent[3] = {g.nz, g.ny, g.nx};
    const int64_t kstep[3] = {pxy, px, 1}, ustep[3] = {int64_t(g.nx) * g.ny, g.nx, 1};
    const int64_t low[3] = {r, r + int64_t(k) * g.nx, r + int64_t(k) * g.ny + j};
    double *const out[3] = {a.fz, a.fy, a.fx};
    // the cell's face on a z, y, x wall: (j, i) of (ny, nx), (k, i) of (nz, nx), (k, j) of (nz, ny)
    const int64_t at[3] = {int64_t(j) * g.nx + i, int64_t(k) * g.nx + i, int64_t(k) * g.ny + j};
    const double *hp[3] = {nullptr, nullptr, nullptr};
    double own[3] = {0.0, 0.0, 0.0}, area[3] = {0.0, 0.0, 0.0};
    if constexpr (SPACED) {
        hp[0] = a.hz + (k + 1); hp[1] = a.hy + (j + 1); hp[2] = a.hx + (i + 1);
        own[0] = *hp[0]; own[1] = *hp[1]; own[2] = *hp[2];
        area[0] = __dmul_rn(own[1], own[2]); area[1] = __dmul_rn(own[0], own[2]); area[2] = __dmul_rn(own[0], own[1]);
    }
    int periodic[3] = {0, 0, 0};
    if constexpr (PERIODIC) { periodic[0] = a.wrap.z; periodic[1] = a.wrap.y; periodic[2] = a.wrap.x; }
    // a wall face of the cell: hi = 0 the low wall of the axis, 1 the high wall
    auto wall_face = [&](int ax, int hi) __attribute__((always_inline)) -> double {
        const int w = 2 * ax + hi;
        const int kind = a.kind[w];
        double val = a.value[w];                           // (+0.0 without a value)
        if (kind == OMG_VALUE_FIELD) val = a.field[w][at[ax]];
        if (a.neumann[w]) {
            if (kind == OMG_VALUE_NONE) return 0.0;
            const double t = __dmul_rn(val, SPACED ? area[ax] : a.scale[ax]);
            return hi ? -t : t;
        }
        const double kn = a.kappa[hi ? c + kstep[ax] : c - kstep[ax]];
        double coeff;
        if constexpr (SPACED) coeff = face_spaced(kc, kn, own[ax], hp[ax][hi ? 1 : -1], area[ax]);
        else coeff = face_of(kc, kn, a.scale[ax]);
        return __dmul_rn(coeff, hi ? __dsub_rn(uc, val) : __dsub_rn(val, uc));
    };
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int m = coord[ax], e = extent[ax];
        const bool wraps = PERIODIC && periodic[ax];
        if (m > 0 || wraps) {
            // the lo cell: one step back, or e - 1 steps on across the seam
            const int back = m > 0 ? 1 : -(e - 1);
            const double kl = a.kappa[c - back * kstep[ax]], ul = a.u[r - back * ustep[ax]];
            double coeff;
            if constexpr (SPACED) coeff = face_spaced(kl, kc, hp[ax][-back], own[ax], area[ax]);
            else coeff = face_of(kl, kc, a.scale[ax]);
            const double F = __dmul_rn(coeff, __dsub_rn(ul, uc));
            put_face<ACCUMULATE>(out[ax], low[ax], F, a.alpha);
            if (m == 0) put_face<ACCUMULATE>(out[ax], low[ax] + e * ustep[ax], F, a.alpha);
        } else {
            put_face<ACCUMULATE>(out[ax], low[ax], wall_face(ax, 0), a.alpha);
        }
        if (m == e - 1 && !wraps) put_face<ACCUMULATE>(out[ax], low[ax] + ustep[ax], wall_face(ax, 1), a.alpha);
    }
}

// the cell balance of three face arrays: ((Fz[k + 1] - Fz[k]) + (Fy[j + 1] - Fy[j])) + (Fx[i + 1] - Fx[i]), one thread per
// cell; the low face indices are the flux kernel's.  32 bytes per cell: every face is read by the two cells it lies between
// (the second time out of the caches) and the balance written once.
__global__ void __launch_bounds__(KAPPA_BLOCK) face_divergence_kernel(KappaGrid g, const double *__restrict__ fz, const double *__restrict__ fy,
                                                                       const double *__restrict__ fx, double *__restrict__ out) {
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r >= n) return;
    int i, j, k;
    cell_of(g, r, i, j, k);
    const int64_t ly = r + int64_t(k) * g.nx, lx = r + int64_t(k) * g.ny + j;
    const double dz = __dsub_rn(fz[r + int64_t(g.nx) * g.ny], fz[r]);
    const double dy = __dsub_rn(fy[ly + g.nx], fy[ly]);
    const double dx = __dsub_rn(fx[lx + 1], fx[lx]);
    out[r] = __dadd_rn(__dadd_rn(dz, dy), dx);
}

// What a call keeps per DEVICE from one call to the next (a right-hand side is made every time step, and the launch itself
// takes a tenth of a millisecond at 256^3): the stream, and the widths in HBM with the host copy they were made from — the same
// widths again cost a comparison, not an allocation and three copies.  Made on first use and kept for the life of the
// process, like download_staged's pinned buffers; one call at a time per device.
struct RhsDevice {
    std::mutex mu;
    hipStream_t s = nullptr;
    double *widths = nullptr;
    size_t capacity = 0;
    std::vector<double> held;
};

RhsDevice &rhs_device() {
    static std::mutex table_mu;
    static std::map<int, RhsDevice *> table;
    int device = 0;
    OMG_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(table_mu);
    RhsDevice *&slot = table[device];
    if (!slot) slot = new RhsDevice;
    return *slot;
}

// What omg_kappa_rhs and omg_kappa_flux check alike of the grid they are given — shape, walls, scale factors, widths —, with
// the widths in HBM behind it: the device's held copy where they are the same as the call before.
struct CallGrid {
    int nz, ny, nx;
    int64_t n, padded;
    bool periodic[6];
    bool spaced;
    const double *hz, *hy, *hx;         // in HBM (spaced)
};

// fills a.g, a.neumann and a.scale; `entry` in front of every refusal
template <typename Args>
CallGrid call_grid(RhsDevice &dev, hipStream_t s, const std::string &entry, const int64_t *shape, const int *walls, const double *scale,
                   const double *hz, const double *hy, const double *hx, Args &a) {
    CallGrid cg = {};
    for (int d = 0; d < 3; ++d)
        OMG_REQUIRE(shape[d] >= 1 && shape[d] < (int64_t(1) << 30), entry + ": every extent of the shape must be >= 1");
    const int nz = cg.nz = int(shape[0]), ny = cg.ny = int(shape[1]), nx = cg.nx = int(shape[2]);
    cg.n = int64_t(nx) * ny * nz;
    cg.padded = int64_t(nz + 2) * (ny + 2) * (nx + 2);
    OMG_REQUIRE(cg.n < (int64_t(1) << 31) - 1 && cg.padded < (int64_t(1) << 31) - 1, entry + ": grid too large for int32 indices");
    a.g = {nx, ny, nz};
    for (int w = 0; w < 6; ++w) {
        const int wv = walls ? walls[w] : OMG_WALL_DIRICHLET;
        OMG_REQUIRE(wv == OMG_WALL_DIRICHLET || wv == OMG_WALL_NEUMANN || wv == OMG_WALL_PERIODIC,
                    entry + ": a wall must be OMG_WALL_DIRICHLET or OMG_WALL_NEUMANN, or OMG_WALL_PERIODIC on both walls of an axis");
        a.neumann[w] = wv == OMG_WALL_NEUMANN;
        cg.periodic[w] = wv == OMG_WALL_PERIODIC;
    }
    for (int d = 0; d < 3; ++d) {
        OMG_REQUIRE(cg.periodic[2 * d] == cg.periodic[2 * d + 1], entry + ": OMG_WALL_PERIODIC must be given for both walls of an axis");
        OMG_REQUIRE(!cg.periodic[2 * d] || shape[d] >= 3, entry + ": a periodic axis needs an extent >= 3");
        a.scale[d] = scale ? scale[d] : 1.0;
        OMG_REQUIRE(finite_pos(a.scale[d]), entry + ": every scale factor must be finite and > 0");
    }
    OMG_REQUIRE((!hz && !hy && !hx) || (hz && hy && hx), entry + ": the widths hz, hy, hx are given together or not at all");
    cg.spaced = hz != nullptr;
    if (!cg.spaced) return cg;
    const int extent[3] = {nz, ny, nx};
    OMG_REQUIRE(a.scale[0] == 1.0 && a.scale[1] == 1.0 && a.scale[2] == 1.0, entry + ": widths and scale factors exclude each other");
    const double *const h[3] = {hz, hy, hx};
    std::vector<double> all;
    all.reserve(size_t(nz) + ny + nx + 6);
    for (int d = 0; d < 3; ++d)
        for (int m = 0; m < extent[d] + 2; ++m) {
            const double v = h[d][m];
            const bool ghost = m == 0 || m == extent[d] + 1;
            OMG_REQUIRE(v < HUGE_VAL && (ghost ? v >= 0.0 : v > 0.0),
                        entry + ": a cell width must be finite and > 0, a ghost width finite and >= 0");
            all.push_back(v);
        }
    // (hz, hy, hx one after the other; compared as bytes: what is held is what the kernel reads)
    if (all.size() != dev.held.size() || std::memcmp(all.data(), dev.held.data(), all.size() * sizeof(double)) != 0) {
        dev.held.clear();
        if (dev.capacity < all.size()) {
            if (dev.widths) OMG_HIP(hipFree(dev.widths));
            dev.widths = nullptr;
            dev.capacity = 0;
            OMG_HIP(hipMalloc(reinterpret_cast<void **>(&dev.widths), all.size() * sizeof(double)));
            dev.capacity = all.size();
        }
        OMG_HIP(hipMemcpyAsync(dev.widths, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice, s));
        OMG_HIP(hipStreamSynchronize(s));               // (`all` is this call's: the copy has left it)
        dev.held = std::move(all);
    }
    cg.hz = dev.widths;
    cg.hy = dev.widths + (nz + 2);
    cg.hx = dev.widths + (nz + 2) + (ny + 2);
    return cg;
}

// the walls' values into a.kind, a.value and a.field, host fields staged one after the other in own_fields; whether a
// Dirichlet wall carries one
template <typename Args>
bool call_values(hipStream_t s, const std::string &entry, const CallGrid &cg, const int *value_kinds, const double *value_scalars,
                 const double *const *value_fields, int values_on_device, Args &a, DevBuf<double> &own_fields) {
    const int64_t faces[3] = {int64_t(cg.ny) * cg.nx, int64_t(cg.nz) * cg.nx, int64_t(cg.nz) * cg.ny};
    bool dirichlet_value = false;
    size_t staged = 0;
    for (int w = 0; w < 6; ++w) {
        const int kind = value_kinds ? value_kinds[w] : OMG_VALUE_NONE;
        OMG_REQUIRE(kind == OMG_VALUE_NONE || kind == OMG_VALUE_SCALAR || kind == OMG_VALUE_FIELD, entry + ": a value kind must be one of OMG_VALUE_*");
        OMG_REQUIRE(kind == OMG_VALUE_NONE || !cg.periodic[w], entry + ": a periodic wall takes no value");
        OMG_REQUIRE(kind != OMG_VALUE_SCALAR || value_scalars, entry + ": value_scalars is null");
        OMG_REQUIRE(kind != OMG_VALUE_FIELD || (value_fields && value_fields[w]), entry + ": a value field is announced and null");
        a.kind[w] = kind;
        a.value[w] = kind == OMG_VALUE_SCALAR ? value_scalars[w] : 0.0;
        a.field[w] = kind == OMG_VALUE_FIELD ? value_fields[w] : nullptr;
        dirichlet_value = dirichlet_value || (kind != OMG_VALUE_NONE && !a.neumann[w]);
        if (kind == OMG_VALUE_FIELD && !values_on_device) staged += size_t(faces[w / 2]);
    }
    if (staged) {                                       // host fields: one after the other in one array
        own_fields.alloc(staged);
        size_t at = 0;
        for (int w = 0; w < 6; ++w) {
            if (a.kind[w] != OMG_VALUE_FIELD) continue;
            OMG_HIP(hipMemcpyAsync(own_fields.p + at, value_fields[w], size_t(faces[w / 2]) * sizeof(double), hipMemcpyHostToDevice, s));
            a.field[w] = own_fields.p + at;
            at += size_t(faces[w / 2]);
        }
    }
    return dirichlet_value;
}

}  // namespace

void kappa_rhs(const KappaRhsInput &in) {
    RhsDevice &dev = rhs_device();
    std::lock_guard<std::mutex> lock(dev.mu);
    if (!dev.s) OMG_HIP(hipStreamCreateWithFlags(&dev.s, hipStreamNonBlocking));
    const hipStream_t s = dev.s;
    const std::string entry = "omg_kappa_rhs";
    OMG_REQUIRE(in.shape && in.b, "omg_kappa_rhs: null argument");
    kappa_rhs_args_t<true> a;
    const CallGrid cg = call_grid(dev, s, entry, in.shape, in.walls, in.scale, in.hz, in.hy, in.hx, a);
    const int64_t n = cg.n, padded = cg.padded;
    const bool spaced = cg.spaced;
    a.hz = cg.hz; a.hy = cg.hy; a.hx = cg.hx;
    // the source
    OMG_REQUIRE(in.f_kind == OMG_VALUE_NONE || in.f_kind == OMG_VALUE_SCALAR || in.f_kind == OMG_VALUE_FIELD, "omg_kappa_rhs: f_kind must be one of OMG_VALUE_*");
    OMG_REQUIRE(in.f_kind == OMG_VALUE_NONE || in.f, "omg_kappa_rhs: f is null");
    OMG_REQUIRE(in.f_kind != OMG_VALUE_SCALAR || !in.f_on_device, "omg_kappa_rhs: a scalar f is one double in host memory");
    DevBuf<double> own_f, own_b, own_kappa, own_fields;
    a.f_kind = in.f_kind;
    const double *f_dev = nullptr;
    double *b_dev = nullptr;
    a.f_value = in.f_kind == OMG_VALUE_SCALAR ? in.f[0] : 0.0;
    if (in.b_on_device) {
        b_dev = in.b;
    } else {
        own_b.alloc(size_t(n));
        b_dev = own_b.p;
    }
    if (in.f_kind == OMG_VALUE_FIELD) {
        if (in.f_on_device) {
            f_dev = in.f;
        } else if (!in.b_on_device) {
            own_b.upload(in.f, size_t(n), s);          // (a host f and a host b: staged in one array, in place)
            f_dev = own_b.p;
        } else {
            own_f.alloc(size_t(n));
            own_f.upload(in.f, size_t(n), s);
            f_dev = own_f.p;
        }
    }
    // the walls' values
    const bool reads_kappa = call_values(s, entry, cg, in.value_kinds, in.value_scalars, in.value_fields, in.values_on_device, a, own_fields);
    a.kappa = nullptr;
    if (reads_kappa) {
        OMG_REQUIRE(in.kappa, "omg_kappa_rhs: kappa is null");
        if (in.kappa_on_device) {
            a.kappa = in.kappa;
        } else {
            own_kappa.alloc(size_t(padded));
            own_kappa.upload(in.kappa, size_t(padded), s);
            a.kappa = own_kappa.p;
        }
    }
    const dim3 grid((unsigned)((n + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    as_constant(f_dev != nullptr, [&](auto field) {
        constexpr bool F = decltype(field)::value;
        if (spaced) hipLaunchKernelGGL((kappa_rhs_kernel<true, F>), grid, dim3(KAPPA_BLOCK), 0, s, a, f_dev, b_dev);
        else hipLaunchKernelGGL((kappa_rhs_kernel<false, F>), grid, dim3(KAPPA_BLOCK), 0, s, static_cast<const KappaRhsArgs &>(a), f_dev, b_dev);
    });
    OMG_HIP(hipGetLastError());
    if (!in.b_on_device) download_staged(in.b, own_b.p, size_t(n) * sizeof(double), s);
    OMG_HIP(hipStreamSynchronize(s));
}

namespace {

// do [p, p + np) and [q, q + nq) doubles share a byte (addresses of one side: both host or both HBM)
bool overlaps(const double *p, int64_t np, const double *q, int64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + uintptr_t(nq) * sizeof(double) && b < a + uintptr_t(np) * sizeof(double);
}

}  // namespace

void kappa_flux(const KappaFluxInput &in) {
    RhsDevice &dev = rhs_device();
    std::lock_guard<std::mutex> lock(dev.mu);
    if (!dev.s) OMG_HIP(hipStreamCreateWithFlags(&dev.s, hipStreamNonBlocking));
    const hipStream_t s = dev.s;
    const std::string entry = "omg_kappa_flux";
    OMG_REQUIRE(in.shape && in.kappa && in.u && in.fz && in.fy && in.fx, "omg_kappa_flux: null argument");
    OMG_REQUIRE(!in.alpha || (*in.alpha - *in.alpha == 0.0), "omg_kappa_flux: alpha must be finite");
    kappa_flux_args_t<true> a;
    const CallGrid cg = call_grid(dev, s, entry, in.shape, in.walls, in.scale, in.hz, in.hy, in.hx, a);
    a.hz = cg.hz; a.hy = cg.hy; a.hx = cg.hx;
    const int64_t n = cg.n, padded = cg.padded;
    const int64_t count[3] = {n + int64_t(cg.ny) * cg.nx, n + int64_t(cg.nz) * cg.nx, n + int64_t(cg.nz) * cg.ny};
    for (int d = 0; d < 3; ++d) OMG_REQUIRE(count[d] < (int64_t(1) << 31) - 1, "omg_kappa_flux: face arrays too large for int32 indices");
    // threads read their neighbours' u and kappa: the flux cannot be made in place
    double *const out[3] = {in.fz, in.fy, in.fx};
    for (int d = 0; d < 3; ++d) {
        OMG_REQUIRE(!(!!in.out_on_device == !!in.u_on_device && overlaps(out[d], count[d], in.u, n)), "omg_kappa_flux: an output overlaps u");
        OMG_REQUIRE(!(!!in.out_on_device == !!in.kappa_on_device && overlaps(out[d], count[d], in.kappa, padded)),
                    "omg_kappa_flux: an output overlaps kappa");
        for (int e = 0; e < d; ++e) OMG_REQUIRE(!overlaps(out[d], count[d], out[e], count[e]), "omg_kappa_flux: the outputs overlap each other");
    }
    a.wrap = {cg.periodic[0], cg.periodic[2], cg.periodic[4]};
    const bool any_periodic = cg.periodic[0] || cg.periodic[2] || cg.periodic[4];
    a.alpha = in.alpha ? *in.alpha : 0.0;
    DevBuf<double> own_u, own_kappa, own_fields, own_out;
    call_values(s, entry, cg, in.value_kinds, in.value_scalars, in.value_fields, in.values_on_device, a, own_fields);
    a.kappa = in.kappa;
    if (!in.kappa_on_device) {
        own_kappa.alloc(size_t(padded));
        own_kappa.upload(in.kappa, size_t(padded), s);
        a.kappa = own_kappa.p;
    }
    a.u = in.u;
    if (!in.u_on_device) {
        own_u.alloc(size_t(n));
        own_u.upload(in.u, size_t(n), s);
        a.u = own_u.p;
    }
    double *face[3] = {in.fz, in.fy, in.fx};
    if (!in.out_on_device) {                            // host outputs: one after the other in one array, with alpha their old values
        own_out.alloc(size_t(count[0] + count[1] + count[2]));
        size_t at = 0;
        for (int d = 0; d < 3; ++d) {
            face[d] = own_out.p + at;
            if (in.alpha) OMG_HIP(hipMemcpyAsync(face[d], out[d], size_t(count[d]) * sizeof(double), hipMemcpyHostToDevice, s));
            at += size_t(count[d]);
        }
    }
    a.fz = face[0]; a.fy = face[1]; a.fx = face[2];
    const dim3 grid((unsigned)((n + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    as_constant(any_periodic, [&](auto wrap) {
        as_constant(in.alpha != nullptr, [&](auto acc) {
            constexpr bool P = decltype(wrap)::value, A = decltype(acc)::value;
            if (cg.spaced) hipLaunchKernelGGL((kappa_flux_kernel<true, P, A>), grid, dim3(KAPPA_BLOCK), 0, s, a);
            else hipLaunchKernelGGL((kappa_flux_kernel<false, P, A>), grid, dim3(KAPPA_BLOCK), 0, s, static_cast<const KappaFluxArgs &>(a));
        });
    });
    OMG_HIP(hipGetLastError());
    if (!in.out_on_device)
        for (int d = 0; d < 3; ++d) download_staged(out[d], face[d], size_t(count[d]) * sizeof(double), s);
    OMG_HIP(hipStreamSynchronize(s));
}

void face_divergence(const int64_t *shape, const double *fz, const double *fy, const double *fx, int faces_on_device, double *out,
                     int out_on_device) {
    RhsDevice &dev = rhs_device();
    std::lock_guard<std::mutex> lock(dev.mu);
    if (!dev.s) OMG_HIP(hipStreamCreateWithFlags(&dev.s, hipStreamNonBlocking));
    const hipStream_t s = dev.s;
    OMG_REQUIRE(shape && fz && fy && fx && out, "omg_face_divergence: null argument");
    for (int d = 0; d < 3; ++d)
        OMG_REQUIRE(shape[d] >= 1 && shape[d] < (int64_t(1) << 30), "omg_face_divergence: every extent of the shape must be >= 1");
    const int nz = int(shape[0]), ny = int(shape[1]), nx = int(shape[2]);
    const int64_t n = int64_t(nx) * ny * nz;
    const int64_t count[3] = {n + int64_t(ny) * nx, n + int64_t(nz) * nx, n + int64_t(nz) * ny};
    for (int d = 0; d < 3; ++d) OMG_REQUIRE(count[d] < (int64_t(1) << 31) - 1, "omg_face_divergence: face arrays too large for int32 indices");
    const double *const given[3] = {fz, fy, fx};
    if (!!faces_on_device == !!out_on_device)
        for (int d = 0; d < 3; ++d) OMG_REQUIRE(!overlaps(out, n, given[d], count[d]), "omg_face_divergence: the output overlaps a face array");
    DevBuf<double> own_faces, own_out;
    const double *face[3] = {fz, fy, fx};
    if (!faces_on_device) {
        own_faces.alloc(size_t(count[0] + count[1] + count[2]));
        size_t at = 0;
        for (int d = 0; d < 3; ++d) {
            OMG_HIP(hipMemcpyAsync(own_faces.p + at, given[d], size_t(count[d]) * sizeof(double), hipMemcpyHostToDevice, s));
            face[d] = own_faces.p + at;
            at += size_t(count[d]);
        }
    }
    double *out_dev = out;
    if (!out_on_device) {
        own_out.alloc(size_t(n));
        out_dev = own_out.p;
    }
    const KappaGrid g = {nx, ny, nz};
    const dim3 grid((unsigned)((n + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    hipLaunchKernelGGL(face_divergence_kernel, grid, dim3(KAPPA_BLOCK), 0, s, g, face[0], face[1], face[2], out_dev);
    OMG_HIP(hipGetLastError());
    if (!out_on_device) download_staged(out, own_out.p, size_t(n) * sizeof(double), s);
    OMG_HIP(hipStreamSynchronize(s));
}

// ---- the 7-point operator of one coefficient per FACE (operators.stencil7_faces is the definition) ----------
// Cz (nz + 1, ny, nx), Cy (nz, ny + 1, nx), Cx (nz, ny, nx + 1) in C order — the arrays the flux kernels write and
// face_divergence_kernel reads; face m of an axis lies between cell m - 1 and cell m.  The row of cell r = (k ny + j) nx + i
// loads its six coefficients, the low faces at Cz[r], Cy[r + k nx], Cx[r + k ny + j] (the flux kernel's indices), the high
// ones nx ny, nx and 1 further on: -C off the diagonal, (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K) (+ sigma) on it.  No
// division and no product: the launch is loads, one sum chain and the stores.  Every face is loaded by the two rows it
// couples — lane l's +I is lane l + 1's -I in the same line, the J and K partners some other workgroup's —, so HBM gives
// each coefficient once and the caches the second time.  A Dirichlet wall's face enters the diagonal only; a Neumann wall's
// face is +0.0 and not read; on a periodic axis the seam's coefficient is C[0], read by the cells at both ends of the line,
// and C[e] is not read.  Row starts, the slot rule of wrapped columns and the staged store are kappa_values_kernel's; the
// pattern kernels are used as they are.
// Validation: every coefficient a thread reads is checked by it (each twice, at no further load); the error word takes the
// smallest key (array << 40) | flat index with the arrays in the order Cz, Cy, Cx, sigma.
namespace {

struct FacesValuesArgs {
    KappaGrid g;
    const double *c[3];           // Cz, Cy, Cx
    const double *sigma;          // null: sigma_value (sigma_kind != 0); else one double (kind 1) or one per cell (kind 2)
    double sigma_value;
    int sigma_kind;               // OMG_SIGMA_*
    int neumann[6];               // -z, +z, -y, +y, -x, +x
    double *data;
    unsigned long long *err;
};
struct FacesWrapArgs : FacesValuesArgs { KappaWrap wrap; };
template <bool PERIODIC> using faces_args_t = std::conditional_t<PERIODIC, FacesWrapArgs, FacesValuesArgs>;

constexpr int FACES_KEY_SHIFT = 40;                   // (a flat index is below 2^31)

template <bool STAGED, bool PERIODIC>
__global__ void __launch_bounds__(KAPPA_BLOCK) faces_values_kernel(faces_args_t<PERIODIC> a) {
    __shared__ double stage[STAGED ? 7 * KAPPA_BLOCK : 1];
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r0 = blockIdx.x * int64_t(KAPPA_BLOCK);
    const int64_t r = r0 + threadIdx.x;
    int64_t base = 0;
    if (STAGED) {
        int i0, j0, k0;
        cell_of(g, r0, i0, j0, k0);
        if constexpr (PERIODIC) base = row_start_wrap(g, a.wrap, r0, i0, j0, k0);
        else base = row_start(g, r0, i0, j0, k0);
    }
    if (r < n) {
        int i, j, k;
        cell_of(g, r, i, j, k);
        // by axis z, y, x: the cell's low face in that axis's array, the step to its high face, the extent
        const int64_t low[3] = {r, r + int64_t(k) * g.nx, r + int64_t(k) * g.ny + j};
        const int64_t step[3] = {int64_t(g.nx) * g.ny, g.nx, 1};
        const int extent[3] = {g.nz, g.ny, g.nx};
        // the six faces in the order of the diagonal's sum: -K, -J, -I, +I, +J, +K
        const bool inside[6] = {k > 0, j > 0, i > 0, i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
        const int wall[6] = {0, 2, 4, 5, 3, 1};
        const int axis[6] = {0, 1, 2, 2, 1, 0};
        const bool high[6] = {false, false, false, true, true, true};
        bool wrapped[6] = {false, false, false, false, false, false};
        if constexpr (PERIODIC) {
            const int periodic[3] = {a.wrap.z, a.wrap.y, a.wrap.x};
#pragma unroll
            for (int e = 0; e < 6; ++e) wrapped[e] = !inside[e] && periodic[axis[e]];
        }
        unsigned long long bad = ~0ull;
        double w[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int ax = axis[e];
            if (!inside[e] && !wrapped[e] && a.neumann[wall[e]]) { w[e] = 0.0; continue; }
            int64_t at = low[ax] + (high[e] ? step[ax] : 0);
            // (PERIODIC: the seam's coefficient is C[0] — the low face of the line's first cell, `extent` faces back from C[e])
            if constexpr (PERIODIC)
                if (wrapped[e] && high[e]) at -= extent[ax] * step[ax];
            const double c = a.c[ax][at];
            if (!kappa_ok(c)) {
                const unsigned long long key = ((unsigned long long)ax << FACES_KEY_SHIFT) | (unsigned long long)at;
                bad = key < bad ? key : bad;
            }
            w[e] = c;
        }
        double d = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(w[0], w[1]), w[2]), w[3]), w[4]), w[5]);
        if (a.sigma_kind != OMG_SIGMA_NONE) {
            const double s = a.sigma ? a.sigma[a.sigma_kind == OMG_SIGMA_FIELD ? r : 0] : a.sigma_value;
            if (!sigma_ok(s)) {
                const unsigned long long key = (3ull << FACES_KEY_SHIFT) | (unsigned long long)(a.sigma_kind == OMG_SIGMA_FIELD ? r : 0);
                bad = key < bad ? key : bad;
            }
            d = __dadd_rn(d, s);
        }
        if (bad != ~0ull) atomicMin(a.err, bad);
        int64_t p;
        if constexpr (PERIODIC) p = row_start_wrap(g, a.wrap, r, i, j, k);
        else p = row_start(g, r, i, j, k);
        double *out = STAGED ? stage + (p - base) : a.data + p;
        int q = 0;
        // (PERIODIC: before an inner entry comes the wrapped one of the opposite face, whose column lies further down; after it, further up)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if constexpr (PERIODIC)
                if (wrapped[5 - e]) out[q++] = -w[5 - e];
            if (inside[e]) out[q++] = -w[e];
        }
        out[q++] = d;
#pragma unroll
        for (int e = 3; e < 6; ++e) {
            if (inside[e]) out[q++] = -w[e];
            if constexpr (PERIODIC)
                if (wrapped[5 - e]) out[q++] = -w[5 - e];
        }
    }
    if (STAGED) {
        __syncthreads();
        const int64_t r1 = r0 + KAPPA_BLOCK < n ? r0 + KAPPA_BLOCK : n;
        int64_t end;
        if (r1 == n) {
            if constexpr (PERIODIC) end = nnz_wrap(g, a.wrap);
            else end = 7 * n - 2 * (int64_t(g.nx) * g.ny + int64_t(g.nx) * g.nz + int64_t(g.ny) * g.nz);
        } else {
            int i1, j1, k1;
            cell_of(g, r1, i1, j1, k1);
            if constexpr (PERIODIC) end = row_start_wrap(g, a.wrap, r1, i1, j1, k1);
            else end = row_start(g, r1, i1, j1, k1);
        }
        const int count = int(end - base);                      // <= 7 * KAPPA_BLOCK
        for (int t = threadIdx.x; t < count; t += KAPPA_BLOCK) a.data[base + t] = stage[t];
    }
}

// the entries of the three face arrays of a grid
void face_counts(int nz, int ny, int nx, int64_t count[3]) {
    const int64_t n = int64_t(nx) * ny * nz;
    count[0] = n + int64_t(ny) * nx;
    count[1] = n + int64_t(nz) * nx;
    count[2] = n + int64_t(nz) * ny;
}

}  // namespace

int64_t FaceField::nnz() const {
    return 7 * rows() - 2 * ((periodic[0] ? 0 : int64_t(nx) * ny) + (periodic[1] ? 0 : int64_t(nx) * nz) + (periodic[2] ? 0 : int64_t(ny) * nz));
}

void FaceField::prepare(const FacesInput &in, hipStream_t s) {
    const int64_t *const shape = in.shape;
    const int *const walls = in.walls;
    OMG_REQUIRE(shape && in.cz && in.cy && in.cx, "faces: null argument");
    for (int d = 0; d < 3; ++d)
        OMG_REQUIRE(shape[d] >= 1 && shape[d] < (int64_t(1) << 30), "faces: every extent of the shape must be >= 1");
    nz = int(shape[0]); ny = int(shape[1]); nx = int(shape[2]);
    int64_t count[3];
    face_counts(nz, ny, nx, count);
    OMG_REQUIRE(7 * int64_t(nx) * ny * nz < (int64_t(1) << 31) - 1 && count[0] < (int64_t(1) << 31) - 1 && count[1] < (int64_t(1) << 31) - 1 &&
                    count[2] < (int64_t(1) << 31) - 1,
                "faces: operator too large for int32 indices");
    for (int f = 0; f < 6; ++f) {
        const int wv = walls ? walls[f] : OMG_WALL_DIRICHLET;
        OMG_REQUIRE(wv == OMG_WALL_DIRICHLET || wv == OMG_WALL_NEUMANN || wv == OMG_WALL_PERIODIC,
                    "faces: a wall must be OMG_WALL_DIRICHLET or OMG_WALL_NEUMANN, or OMG_WALL_PERIODIC on both walls of an axis");
        neumann[f] = wv == OMG_WALL_NEUMANN;
    }
    for (int d = 0; d < 3; ++d) {
        static const char *const axis_name[3] = {"z", "y", "x"};
        const bool lo = walls && walls[2 * d] == OMG_WALL_PERIODIC, hi = walls && walls[2 * d + 1] == OMG_WALL_PERIODIC;
        periodic[d] = lo && hi;
        if (lo != hi)
            throw Error(OMG_ERR_INVALID, std::string("faces: OMG_WALL_PERIODIC must be given for both walls of an axis: only one wall of axis ") +
                                             axis_name[d] + " has it");
        if (periodic[d] && shape[d] < 3)
            throw Error(OMG_ERR_INVALID, std::string("faces: a periodic axis needs an extent >= 3: axis ") + axis_name[d] + " has " +
                                             std::to_string((long long)shape[d]));
    }
    const int kind = in.sigma_kind;
    OMG_REQUIRE(kind == OMG_SIGMA_NONE || kind == OMG_SIGMA_SCALAR || kind == OMG_SIGMA_FIELD, "faces: sigma_kind must be one of OMG_SIGMA_*");
    OMG_REQUIRE(kind == OMG_SIGMA_NONE || in.sigma, "faces: sigma is null");
    sigma_kind = kind;
    sigma_dev = nullptr;
    sigma_value = 0.0;
    if (kind == OMG_SIGMA_SCALAR && !in.sigma_on_device) {
        sigma_value = in.sigma[0];
        OMG_REQUIRE(sigma_value >= 0.0 && sigma_value < HUGE_VAL, "faces: sigma must be finite and >= 0");
    } else if (kind != OMG_SIGMA_NONE) {
        if (in.sigma_on_device) {
            sigma_dev = in.sigma;
        } else {
            own_sigma.alloc(size_t(nx) * ny * nz);
            own_sigma.upload(in.sigma, size_t(nx) * ny * nz, s);
            sigma_dev = own_sigma.p;
        }
    }
    const double *const given[3] = {in.cz, in.cy, in.cx};
    if (in.faces_on_device) {
        for (int d = 0; d < 3; ++d) c_dev[d] = given[d];
    } else {                                            // host arrays: one after the other in one array
        own_faces.alloc(size_t(count[0] + count[1] + count[2]));
        size_t at = 0;
        for (int d = 0; d < 3; ++d) {
            OMG_HIP(hipMemcpyAsync(own_faces.p + at, given[d], size_t(count[d]) * sizeof(double), hipMemcpyHostToDevice, s));
            c_dev[d] = own_faces.p + at;
            at += size_t(count[d]);
        }
    }
    if (!err.p) err.alloc(1);
}

namespace {

template <bool STAGED, bool PERIODIC>
void launch_face_values(const FaceField &F, double *data, hipStream_t s) {
    faces_args_t<PERIODIC> a;
    a.g = {F.nx, F.ny, F.nz};
    for (int d = 0; d < 3; ++d) a.c[d] = F.c_dev[d];
    a.sigma = F.sigma_dev;
    a.sigma_value = F.sigma_value;
    a.sigma_kind = F.sigma_kind;
    for (int f = 0; f < 6; ++f) a.neumann[f] = F.neumann[f];
    a.data = data;
    a.err = F.err.p;
    if constexpr (PERIODIC) a.wrap = {F.periodic[0], F.periodic[1], F.periodic[2]};
    const dim3 grid((unsigned)((F.rows() + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    hipLaunchKernelGGL((faces_values_kernel<STAGED, PERIODIC>), grid, dim3(KAPPA_BLOCK), 0, s, a);
}

}  // namespace

void FaceField::values(double *data, hipStream_t s, const char *entry) {
    OMG_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(unsigned long long), s));
    as_constant(kappa_staged(), [&](auto staged) {
        as_constant(any_periodic(), [&](auto wrap) { launch_face_values<decltype(staged)::value, decltype(wrap)::value>(*this, data, s); });
    });
    OMG_HIP(hipGetLastError());
    unsigned long long e = ~0ull;
    OMG_HIP(hipMemcpyAsync(&e, err.p, sizeof(e), hipMemcpyDeviceToHost, s));
    OMG_HIP(hipStreamSynchronize(s));
    if (e == ~0ull) return;
    // the key names an array and a flat index in it: as (k, j, i) of that array's own shape
    const int which = int(e >> FACES_KEY_SHIFT);
    const int64_t flat = int64_t(e & ((1ull << FACES_KEY_SHIFT) - 1));
    const int64_t ex = nx + (which == 2 ? 1 : 0), ey = ny + (which == 1 ? 1 : 0);
    const std::string at = "(" + std::to_string((long long)(flat / (ex * ey))) + ", " + std::to_string((long long)((flat / ex) % ey)) + ", " +
                           std::to_string((long long)(flat % ex)) + ")";
    if (which == 3) throw Error(OMG_ERR_INVALID, std::string(entry) + ": sigma at cell " + at + " is not finite and >= 0");
    static const char *const name[3] = {"Cz", "Cy", "Cx"};
    throw Error(OMG_ERR_INVALID, std::string(entry) + ": the coefficient " + name[which] + " at face " + at + " is not finite and > 0");
}

void FaceField::assemble(int32_t *indptr, int32_t *indices, double *data, hipStream_t s, const char *entry) {
    if (indptr) launch_pattern({nx, ny, nz}, periodic, indptr, indices, s);
    values(data, s, entry);
}

void FaceField::assemble(DevCsrPlain &A, hipStream_t s, const char *entry) {
    A.n_rows = A.n_cols = rows();
    A.nnz = nnz();
    A.indptr.alloc(size_t(A.n_rows) + 1);
    A.indices.alloc(size_t(A.nnz));
    A.data.alloc(size_t(A.nnz));
    assemble(A.indptr.p, A.indices.p, A.data.p, s, entry);
}

// ---- its right-hand side and its face fluxes (operators.rhs_faces, operators.flux_faces) -----------------------------------
// faces_rhs_kernel: b = ((((((f + t-K) + t-J) + t-I) + t+I) + t+J) + t+K), one thread per cell, f read and b written at unit
// stride (b may be f: each thread reads its own f first).  t = C_wall g at a Dirichlet wall with a value — the only lanes that
// read a coefficient —, the value itself at a Neumann wall (the outward flux through the face, already integrated), +0.0 else.
// faces_flux_kernel: kappa_flux_kernel's thread-to-face mapping — the thread owns the three low faces of its cell, the last
// layer's cells their high wall face too, cell 0 of a periodic line face e with the bits of face 0 — with the coefficient
// LOADED from the face's own place instead of computed: F = C (u_lo - u_hi), one subtraction and one multiplication; the
// coefficient arrays are read and the outputs written at unit stride along x.  ACCUMULATE: out = out + alpha F.
namespace {

struct FacesRhsArgs {
    KappaGrid g;
    const double *__restrict__ c[3];       // Cz, Cy, Cx; read only at Dirichlet walls with a value
    double f_value;
    int kind[6];                           // per wall -z, +z, -y, +y, -x, +x: OMG_VALUE_* (a periodic wall: NONE)
    int neumann[6];
    double value[6];
    const double *__restrict__ field[6];   // one per face of the wall: (ny, nx), (nz, nx), (nz, ny)
};

template <bool F_FIELD>
__global__ void __launch_bounds__(KAPPA_BLOCK) faces_rhs_kernel(FacesRhsArgs a, const double *f, double *b) {
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r >= n) return;
    double v;
    if constexpr (F_FIELD) v = f[r];
    else v = a.f_value;                                // (the scalar; +0.0 for no f)
    int i, j, k;
    cell_of(g, r, i, j, k);
    // the six faces in the order of the sum: -K, -J, -I, +I, +J, +K
    const bool inside[6] = {k > 0, j > 0, i > 0, i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
    const int wall[6] = {0, 2, 4, 5, 3, 1};
    const int axis[6] = {0, 1, 2, 2, 1, 0};
    const bool high[6] = {false, false, false, true, true, true};
    bool valued[6], on_wall = false;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        valued[e] = !inside[e] && a.kind[wall[e]] != OMG_VALUE_NONE;
        on_wall = on_wall || valued[e];
    }
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (on_wall) {
        const int64_t low[3] = {r, r + int64_t(k) * g.nx, r + int64_t(k) * g.ny + j};
        const int64_t step[3] = {int64_t(g.nx) * g.ny, g.nx, 1};
        // the cell's face on a z, y, x wall: (j, i) of (ny, nx), (k, i) of (nz, nx), (k, j) of (nz, ny)
        const int64_t at[3] = {int64_t(j) * g.nx + i, int64_t(k) * g.nx + i, int64_t(k) * g.ny + j};
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            if (!valued[e]) continue;
            const int w = wall[e], ax = axis[e];
            double val = a.value[w];
            if (a.kind[w] == OMG_VALUE_FIELD) val = a.field[w][at[ax]];
            if (a.neumann[w]) {
                t[e] = val;
                continue;
            }
            t[e] = __dmul_rn(a.c[ax][low[ax] + (high[e] ? step[ax] : 0)], val);
        }
    }
    b[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(v, t[0]), t[1]), t[2]), t[3]), t[4]), t[5]);
}

struct FacesFluxArgs {
    KappaGrid g;
    KappaWrap wrap;                        // per axis z, y, x: periodic (read by the PERIODIC instantiations)
    const double *__restrict__ c[3];       // Cz, Cy, Cx
    const double *__restrict__ u;          // nz ny nx
    int kind[6];                           // per wall -z, +z, -y, +y, -x, +x: OMG_VALUE_* (a periodic wall: NONE)
    int neumann[6];
    double value[6];
    const double *__restrict__ field[6];
    double alpha;                          // ACCUMULATE
    double *fz, *fy, *fx;
};

template <bool PERIODIC, bool ACCUMULATE>
__global__ void __launch_bounds__(KAPPA_BLOCK) faces_flux_kernel(FacesFluxArgs a) {
    const KappaGrid g = a.g;
    const int64_t n = int64_t(g.nx) * g.ny * g.nz;
    const int64_t r = blockIdx.x * int64_t(KAPPA_BLOCK) + threadIdx.x;
    if (r >= n) return;
    const double uc = a.u[r];
    int i, j, k;
    cell_of(g, r, i, j, k);
    // by axis z, y, x: the cell's coordinate, the extent, the step to the next cell in u — the step to the next face of that
    // axis in its face array too —, and the cell's low face
    const int coord[3] = {k, j, i}, extent[3] = {g.nz, g.ny, g.nx};
    const int64_t ustep[3] = {int64_t(g.nx) * g.ny, g.nx, 1};
    const int64_t low[3] = {r, r + int64_t(k) * g.nx, r + int64_t(k) * g.ny + j};
    double *const out[3] = {a.fz, a.fy, a.fx};
    const int64_t at[3] = {int64_t(j) * g.nx + i, int64_t(k) * g.nx + i, int64_t(k) * g.ny + j};
    int periodic[3] = {0, 0, 0};
    if constexpr (PERIODIC) { periodic[0] = a.wrap.z; periodic[1] = a.wrap.y; periodic[2] = a.wrap.x; }
    // a wall face of the cell: hi = 0 the low wall of the axis, 1 the high wall
    auto wall_face = [&](int ax, int hi) __attribute__((always_inline)) -> double {
        const int w = 2 * ax + hi;
        const int kind = a.kind[w];
        double val = a.value[w];                           // (+0.0 without a value)
        if (kind == OMG_VALUE_FIELD) val = a.field[w][at[ax]];
        if (a.neumann[w]) {
            if (kind == OMG_VALUE_NONE) return 0.0;
            return hi ? -val : val;
        }
        const double coeff = a.c[ax][hi ? low[ax] + ustep[ax] : low[ax]];
        return __dmul_rn(coeff, hi ? __dsub_rn(uc, val) : __dsub_rn(val, uc));
    };
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int m = coord[ax], e = extent[ax];
        const bool wraps = PERIODIC && periodic[ax];
        if (m > 0 || wraps) {
            // the lo cell: one step back, or e - 1 steps on across the seam (whose coefficient is C[0], this cell's low face)
            const int back = m > 0 ? 1 : -(e - 1);
            const double ul = a.u[r - back * ustep[ax]];
            const double F = __dmul_rn(a.c[ax][low[ax]], __dsub_rn(ul, uc));
            put_face<ACCUMULATE>(out[ax], low[ax], F, a.alpha);
            if (m == 0) put_face<ACCUMULATE>(out[ax], low[ax] + e * ustep[ax], F, a.alpha);
        } else {
            put_face<ACCUMULATE>(out[ax], low[ax], wall_face(ax, 0), a.alpha);
        }
        if (m == e - 1 && !wraps) put_face<ACCUMULATE>(out[ax], low[ax] + ustep[ax], wall_face(ax, 1), a.alpha);
    }
}

// what omg_faces_rhs and omg_faces_flux check of shape and walls (call_grid's checks, no scale and no widths), the three
// coefficient arrays in HBM behind it: `given` where they lie there, else staged one after the other in own_faces (`stage`)
struct FaceGridOnly {
    KappaGrid g;
    int neumann[6];
    double scale[3];
};

template <typename Args>
CallGrid face_call_grid(RhsDevice &dev, hipStream_t s, const std::string &entry, const int64_t *shape, const int *walls, Args &a) {
    FaceGridOnly only;
    const CallGrid cg = call_grid(dev, s, entry, shape, walls, nullptr, nullptr, nullptr, nullptr, only);
    a.g = only.g;
    for (int w = 0; w < 6; ++w) a.neumann[w] = only.neumann[w];
    int64_t count[3];
    face_counts(cg.nz, cg.ny, cg.nx, count);
    for (int d = 0; d < 3; ++d) OMG_REQUIRE(count[d] < (int64_t(1) << 31) - 1, entry + ": face arrays too large for int32 indices");
    return cg;
}

void stage_faces(hipStream_t s, const CallGrid &cg, const double *const given[3], int on_device, bool stage, const double *out[3],
                 DevBuf<double> &own_faces) {
    int64_t count[3];
    face_counts(cg.nz, cg.ny, cg.nx, count);
    size_t at = 0;
    if (!on_device && stage) own_faces.alloc(size_t(count[0] + count[1] + count[2]));
    for (int d = 0; d < 3; ++d) {
        out[d] = on_device ? given[d] : nullptr;
        if (on_device || !stage) continue;
        OMG_HIP(hipMemcpyAsync(own_faces.p + at, given[d], size_t(count[d]) * sizeof(double), hipMemcpyHostToDevice, s));
        out[d] = own_faces.p + at;
        at += size_t(count[d]);
    }
}

}  // namespace

void faces_rhs(const FacesRhsInput &in) {
    RhsDevice &dev = rhs_device();
    std::lock_guard<std::mutex> lock(dev.mu);
    if (!dev.s) OMG_HIP(hipStreamCreateWithFlags(&dev.s, hipStreamNonBlocking));
    const hipStream_t s = dev.s;
    const std::string entry = "omg_faces_rhs";
    OMG_REQUIRE(in.shape && in.b, "omg_faces_rhs: null argument");
    FacesRhsArgs a;
    const CallGrid cg = face_call_grid(dev, s, entry, in.shape, in.walls, a);
    const int64_t n = cg.n;
    OMG_REQUIRE(in.f_kind == OMG_VALUE_NONE || in.f_kind == OMG_VALUE_SCALAR || in.f_kind == OMG_VALUE_FIELD, "omg_faces_rhs: f_kind must be one of OMG_VALUE_*");
    OMG_REQUIRE(in.f_kind == OMG_VALUE_NONE || in.f, "omg_faces_rhs: f is null");
    OMG_REQUIRE(in.f_kind != OMG_VALUE_SCALAR || !in.f_on_device, "omg_faces_rhs: a scalar f is one double in host memory");
    DevBuf<double> own_f, own_b, own_faces, own_fields;
    const double *f_dev = nullptr;
    double *b_dev = nullptr;
    a.f_value = in.f_kind == OMG_VALUE_SCALAR ? in.f[0] : 0.0;
    if (in.b_on_device) {
        b_dev = in.b;
    } else {
        own_b.alloc(size_t(n));
        b_dev = own_b.p;
    }
    if (in.f_kind == OMG_VALUE_FIELD) {
        if (in.f_on_device) {
            f_dev = in.f;
        } else if (!in.b_on_device) {
            own_b.upload(in.f, size_t(n), s);          // (a host f and a host b: staged in one array, in place)
            f_dev = own_b.p;
        } else {
            own_f.alloc(size_t(n));
            own_f.upload(in.f, size_t(n), s);
            f_dev = own_f.p;
        }
    }
    const bool reads_faces = call_values(s, entry, cg, in.value_kinds, in.value_scalars, in.value_fields, in.values_on_device, a, own_fields);
    OMG_REQUIRE(!reads_faces || (in.cz && in.cy && in.cx), "omg_faces_rhs: a coefficient array is null");
    const double *const given[3] = {in.cz, in.cy, in.cx};
    const double *c[3];
    stage_faces(s, cg, given, in.faces_on_device, reads_faces, c, own_faces);
    for (int d = 0; d < 3; ++d) a.c[d] = reads_faces ? c[d] : nullptr;
    const dim3 grid((unsigned)((n + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    as_constant(f_dev != nullptr, [&](auto field) {
        hipLaunchKernelGGL((faces_rhs_kernel<decltype(field)::value>), grid, dim3(KAPPA_BLOCK), 0, s, a, f_dev, b_dev);
    });
    OMG_HIP(hipGetLastError());
    if (!in.b_on_device) download_staged(in.b, own_b.p, size_t(n) * sizeof(double), s);
    OMG_HIP(hipStreamSynchronize(s));
}

void faces_flux(const FacesFluxInput &in) {
    RhsDevice &dev = rhs_device();
    std::lock_guard<std::mutex> lock(dev.mu);
    if (!dev.s) OMG_HIP(hipStreamCreateWithFlags(&dev.s, hipStreamNonBlocking));
    const hipStream_t s = dev.s;
    const std::string entry = "omg_faces_flux";
    OMG_REQUIRE(in.shape && in.cz && in.cy && in.cx && in.u && in.fz && in.fy && in.fx, "omg_faces_flux: null argument");
    OMG_REQUIRE(!in.alpha || (*in.alpha - *in.alpha == 0.0), "omg_faces_flux: alpha must be finite");
    FacesFluxArgs a;
    const CallGrid cg = face_call_grid(dev, s, entry, in.shape, in.walls, a);
    const int64_t n = cg.n;
    int64_t count[3];
    face_counts(cg.nz, cg.ny, cg.nx, count);
    // threads read their neighbours' u, and a coefficient is read by the thread of another face's output: nothing in place
    double *const out[3] = {in.fz, in.fy, in.fx};
    const double *const given[3] = {in.cz, in.cy, in.cx};
    for (int d = 0; d < 3; ++d) {
        OMG_REQUIRE(!(!!in.out_on_device == !!in.u_on_device && overlaps(out[d], count[d], in.u, n)), "omg_faces_flux: an output overlaps u");
        for (int e = 0; e < 3; ++e)
            OMG_REQUIRE(!(!!in.out_on_device == !!in.faces_on_device && overlaps(out[d], count[d], given[e], count[e])),
                        "omg_faces_flux: an output overlaps a coefficient array");
        for (int e = 0; e < d; ++e) OMG_REQUIRE(!overlaps(out[d], count[d], out[e], count[e]), "omg_faces_flux: the outputs overlap each other");
    }
    a.wrap = {cg.periodic[0], cg.periodic[2], cg.periodic[4]};
    const bool any_periodic = cg.periodic[0] || cg.periodic[2] || cg.periodic[4];
    a.alpha = in.alpha ? *in.alpha : 0.0;
    DevBuf<double> own_u, own_faces, own_fields, own_out;
    call_values(s, entry, cg, in.value_kinds, in.value_scalars, in.value_fields, in.values_on_device, a, own_fields);
    const double *c[3];
    stage_faces(s, cg, given, in.faces_on_device, true, c, own_faces);
    for (int d = 0; d < 3; ++d) a.c[d] = c[d];
    a.u = in.u;
    if (!in.u_on_device) {
        own_u.alloc(size_t(n));
        own_u.upload(in.u, size_t(n), s);
        a.u = own_u.p;
    }
    double *face[3] = {in.fz, in.fy, in.fx};
    if (!in.out_on_device) {                            // host outputs: one after the other in one array, with alpha their old values
        own_out.alloc(size_t(count[0] + count[1] + count[2]));
        size_t at = 0;
        for (int d = 0; d < 3; ++d) {
            face[d] = own_out.p + at;
            if (in.alpha) OMG_HIP(hipMemcpyAsync(face[d], out[d], size_t(count[d]) * sizeof(double), hipMemcpyHostToDevice, s));
            at += size_t(count[d]);
        }
    }
    a.fz = face[0]; a.fy = face[1]; a.fx = face[2];
    const dim3 grid((unsigned)((n + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
    as_constant(any_periodic, [&](auto wrap) {
        as_constant(in.alpha != nullptr, [&](auto acc) {
            hipLaunchKernelGGL((faces_flux_kernel<decltype(wrap)::value, decltype(acc)::value>), grid, dim3(KAPPA_BLOCK), 0, s, a);
        });
    });
    OMG_HIP(hipGetLastError());
    if (!in.out_on_device)
        for (int d = 0; d < 3; ++d) download_staged(out[d], face[d], size_t(count[d]) * sizeof(double), s);
    OMG_HIP(hipStreamSynchronize(s));
}

}  // namespace omg
