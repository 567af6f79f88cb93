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

void KappaField::assemble(int32_t *indptr, int32_t *indices, double *data, hipStream_t s, const char *entry) {
    if (indptr) {
        const KappaGrid g = {nx, ny, nz};
        const dim3 grid((unsigned)((rows() + 1 + KAPPA_BLOCK - 1) / KAPPA_BLOCK));
        if (any_periodic()) {
            const KappaWrap wr = {periodic[0], periodic[1], periodic[2]};
            hipLaunchKernelGGL(kappa_pattern_wrap_kernel, grid, dim3(KAPPA_BLOCK), 0, s, g, wr, indptr, indices);
        } else {
            hipLaunchKernelGGL(kappa_pattern_kernel, grid, dim3(KAPPA_BLOCK), 0, s, g, indptr, indices);
        }
        OMG_HIP(hipGetLastError());
    }
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

}  // namespace omg
