// Device-resident level hierarchy and the V-cycle driver (openmg/__init__.py:151-236),
// plus the extern "C" surface declared in include/openmg_hip.h.
//
// The implementation is a template on the value type V the levels are stored and computed
// in (double: the reference's precision; float: BASELINE configs[4]).  The C handle holds
// one of the two instantiations; the host boundary is double either way.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <array>
#include <map>
#include <mutex>
#include <thread>
#include <type_traits>

#include "common.h"

namespace omg {

// ---- scattered device memory (common.h) -------------------------------------------------------------------------------
std::vector<ScatteredBlock> &scattered_registry() {
    static std::vector<ScatteredBlock> r;
    return r;
}
static std::mutex &scattered_mutex() {
    static std::mutex m;
    return m;
}
// Tear a block down the way it was put up: ONE hipMemUnmap per hipMemMap (the runtime unmaps per mapping — a single call over
// a range of many mappings need not undo any of them, and releasing the handles would then leave the pages mapped: a leak
// of the whole block for the life of the process), then the handles, then the address range.  Every failure is reported.
static void scattered_release(ScatteredBlock &blk, size_t mapped) {
    auto report = [](const char *what, hipError_t e) {
        if (e == hipSuccess) return;
        (void)hipGetLastError();
        fprintf(stderr, "libopenmg_hip: scattered block: %s failed: %s (device memory may stay allocated)\n", what, hipGetErrorString(e));
    };
    for (size_t i = 0; i < mapped; ++i) report("hipMemUnmap", hipMemUnmap(static_cast<char *>(blk.va) + i * blk.chunk, blk.chunk));
    for (auto h : blk.handles) report("hipMemRelease", hipMemRelease(h));
    blk.handles.clear();
    if (blk.va) report("hipMemAddressFree", hipMemAddressFree(blk.va, blk.total));
    blk.va = nullptr;
}
void *scattered_alloc(size_t bytes, size_t chunk_bytes) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return nullptr;
    hipMemAllocationProp prop;
    std::memset(&prop, 0, sizeof(prop));
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0) { (void)hipGetLastError(); return nullptr; }
    const size_t chunk = (std::max(chunk_bytes, gran) + gran - 1) / gran * gran;
    const size_t n = (bytes + chunk - 1) / chunk;
    ScatteredBlock blk;
    blk.total = n * chunk;
    blk.chunk = chunk;
    auto undo = [&](size_t mapped) { scattered_release(blk, mapped); };
    if (hipMemAddressReserve(&blk.va, blk.total, chunk, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    blk.handles.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) { undo(0); return nullptr; }
        blk.handles.push_back(h);
    }
    // piece i of the virtual range <- the perm(i)-th allocation: a fixed pseudo-random permutation (Fisher-Yates over an LCG)
    std::vector<size_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = i;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (size_t i = n; i > 1; --i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(perm[i - 1], perm[size_t((state >> 33) % i)]);
    }
    for (size_t i = 0; i < n; ++i)
        if (hipMemMap(static_cast<char *>(blk.va) + i * chunk, chunk, 0, blk.handles[perm[i]], 0) != hipSuccess) { undo(i); return nullptr; }
    hipMemAccessDesc acc;
    std::memset(&acc, 0, sizeof(acc));
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if (hipMemSetAccess(blk.va, blk.total, &acc, 1) != hipSuccess) { undo(n); return nullptr; }
    void *const va = blk.va;
    std::lock_guard<std::mutex> lock(scattered_mutex());
    scattered_registry().push_back(std::move(blk));
    return va;
}
bool scattered_free(void *va) {
    ScatteredBlock blk;
    {
        std::lock_guard<std::mutex> lock(scattered_mutex());
        auto &r = scattered_registry();
        size_t i = 0;
        while (i < r.size() && r[i].va != va) ++i;
        if (i == r.size()) return false;
        blk = std::move(r[i]);
        r.erase(r.begin() + long(i));
    }
    // unlike hipFree, unmapping does not wait for work that still uses the range
    if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
    scattered_release(blk, blk.handles.size());
    return true;
}

static thread_local std::string g_last_error;
void set_last_error(const std::string &m) { g_last_error = m; }

double SetupTimer::now() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        throw Error(OMG_ERR_NO_DEVICE,
                    "no HIP device visible: libopenmg_hip.so has no CPU fallback "
                    "(hipGetDeviceCount: " + std::string(hipGetErrorString(e)) + ")");
}

namespace {

inline bool getenv_flag(const char *name) { const char *e = getenv(name); return e && e[0] == '1'; }
inline bool getenv_flag0(const char *name) { const char *e = getenv(name); return e && e[0] == '0'; }   // switched OFF

struct SweepStep {
    int set_begin, set_end;   // [begin, end)
    bool serial;              // run of single-block sets -> one workgroup
};

template <typename V>
struct Level {
    int64_t n = 0;
    DevCsrT<V> A;             // P A P^T in this level's smoother ordering
    DevCsrT<V> R;             // to level+1: rows in next ordering, columns in this ordering
    DevCsrT<V> P;             // R^T: rows in this ordering, columns in next ordering
    Ordering ord;
    DevBuf<int32_t> perm;     // new -> old (empty when identity)
    DevBuf<int32_t> r_out;    // restriction row (natural coarse numbering) -> slot in the next level's ordering
    DevBuf<V> x, b, r, tmp;
    DevBuf<V> diag;           // diagonal of A in this level's ordering (levels entered with a zero iterate: restrict_level)
    DevBuf<double> partials;
    DevBuf<double> nat;       // natural-order (double) staging for host I/O at this level
    V *xp = nullptr, *tp = nullptr;   // current iterate / Jacobi scratch (swap)
    std::vector<SweepStep> plan;
    // prolongation as a scatter over R's row patterns (ROW_SCATTER) instead of a pass over the
    // explicit transpose P: possible when no two rows of R share a column (aggregation) and R
    // is row-pattern coded; reads 1 byte per COARSE row instead of ~9 per fine row
    bool scatter_prolong = false;
    // over-correction (Hier::over != 1) on the row-kernel path: the prolongation operator's stored values (R's under
    // scatter_prolong, P's otherwise) times the factor, each rounded once — a second edition of its value arrays, made by
    // prolong_add_level on first use for the factor pw_factor (0: none made)
    DevBuf<V> pw_data, pw_vdict, pw_pval, pw_vell;
    RowValues<V> pw;
    double pw_factor = 0.0;
    // lexicographic Gauss-Seidel of a grid star stencil: one launch per sweep (common.h MarchPlan);
    // the level then keeps its natural ordering (one "set") for every other kernel
    std::unique_ptr<MarchPlan<V>> march;
    // red-black sweeps of a constant-coefficient grid star stencil under the 2x2x2 aggregation: each half
    // of a V(pre >= 1, post >= 1) cycle is one plane-pipelined launch (common.h PlanePlan), out of place
    // between x and tmp
    std::unique_ptr<PlanePlan<V>> plane;
    // 27-point grid stencil with per-row coefficients under the 2x2x2 aggregation, 8-colour Gauss-Seidel (BASELINE
    // configs[4]): the cycle over this level runs the octant-layout kernels of stencil27.hip (common.h Stencil27Plan)
    std::unique_ptr<Stencil27Plan<V>> s27;
    // 7-point grid stencil with per-row coefficients, red-black (the ordinary variable-coefficient input): each half of the
    // cycle over this level is one launch of var7.hip (common.h Var7Plan); the row-kernel format exists beside it
    std::unique_ptr<Var7Plan<V>> var7;
    // zebra line smoother (OMG_SMOOTH_LINE*; common.h LinePlan): the level's ordering is the plan's, a sweep is its two
    // launches; everything else of the cycle runs the row kernels, set by set, with nothing fused into the sweeps
    std::unique_ptr<LinePlan<V>> line;
    DevBuf<char> pool;               // OMG_VEC_POOL=1: x, tmp, b of a large plane level as three views into ONE allocation
    size_t pool_span = 0, pool_off1 = 0, pool_off2 = 0;      // ... its layout (pool_views)
    // where the matrix-free SpMV of a plane level leaves its product: an allocation of its OWN, made on first use.  Written
    // into the level's scratch vector — which shares an allocation with x, two spans further on — the same launch takes
    // 57-62 us at 256^3 where it takes 45 into any separate allocation (profiles/r05_spmv_placement.txt: one process, the
    // destinations in turn): read and write streams a fixed physical distance apart meet on the same banks
    DevBuf<V> spmv_y;
    // A plane level's cycle never touches the row-kernel format of A and R (nor r, the block partials, the
    // sweep plan): they are built on first use — by a cycle with pre = 0 or post = 0, a single-level
    // operation, a format query — from the operator the plan describes (ensure_format; OMG_PLANE_LAZY=0: at creation)
    bool format_pending = false;
};

struct ProfEvent {
    int cls;
    hipEvent_t a, b;
};

template <typename V>
struct Hier {
    using value_type = V;
    std::vector<Level<V>> lv;
    CoarseSolver<V> coarse;   // direct solve of the coarsest operator (common.h)
    DevBuf<double> norm_dev;
    DevBuf<uint32_t> plane_status; // PlanePlan::status of every plane level: bit 1 = a wave gave up waiting for its neighbour wave
    // omg_vcycle_ex: cycle_body leaves a copy of level pre_level's iterate after its pre-smoothing here (-1: nowhere)
    DevBuf<V> pre_buf;
    int pre_level = -1;
    DevBuf<double> norms_dev;      // omg_resident_cycles: one norm per cycle of the batch
    DevBuf<double> batch_partials; // ... and the block partials of up to 64 deferred norms
    // omg_resident_pcg (level 0, its numbering): a copy of b, the iterate x, the search direction p and its successor p2, q = A p;
    // the scalars (PCG_NSC, then PCG_NSC zeros: beta = 0, not done), the workgroup partials, one norm per iteration
    DevBuf<V> pcg_b, pcg_x, pcg_p, pcg_p2, pcg_q;
    DevBuf<double> pcg_sc, pcg_part, pcg_norms;
    DevBuf<double> norms2;         // omg_resident_norms: ||b||, ||b - A x|| (resident_norms; made on first use)
    // mean projection (nullspace.hip; project_vec below): the workgroup partials and, behind them, the folded sum
    DevBuf<double> proj_scratch;
    // OMG_DTYPE_MIXED (a float hierarchy): the levels as for OMG_DTYPE_F32, and level 0's outer state in double — what the
    // resident entries iterate on (mixed_* below), in the level's numbering.  The operator: on a plane level (pcg_fused_plane)
    // its seven constants taken from the caller's double CSR; otherwise the caller's CSR renumbered into the level's ordering,
    // columns ascending, plain int32 CSR (src: entry e came from the caller's entry src[e] — omg_hierarchy_update_fine).
    // x / x2: the iterate and the out-of-place target of the plane defect correction (swapped); r, p, p2, q: FCG's
    bool mixed = false;
    struct Mixed {
        bool plane = false;
        PcgPlane pg{};
        DevCsrT<double> A;
        DevBuf<int32_t> src;
        DevBuf<double> b, x, x2, r, p, p2, q;
        DevBuf<double> load_sc;          // PCG_NSC scalars: the exponent of ||b|| in PCG_E_USED and PCG_E_NEXT, since resident_load
    } mx;
    int smoother = OMG_SMOOTH_GS_LEX;
    double omega = 1.0;
    // OMG_SMOOTH_LINE*: the axis every smoothed level's lines follow (LineGeom::axis; -1: no line smoother) and the grid's dimension
    int line_axis = -1, line_dim = 0;
    // omg_hierarchy_set_cycle: the shape of every cycle run on this hierarchy (cycle_body) and the over-correction factor —
    // the prolongation's weight is over * (the restriction's weight), rounded once to V; the restriction keeps its own
    int cycle_shape = OMG_CYCLE_V;
    double over = 1.0;
    hipStream_t own = nullptr, stream = nullptr;
    // omg_hierarchy_update_fine (a hierarchy set up on the device whose smoothed levels all run the 27-point kernels): the
    // fine operator's row pointers (the values come with every update), its grid, and per level >= 1 the Galerkin
    // operator as a dense [row][27] double array — the next product's input
    DevBuf<int32_t> indptr0;
    int64_t nnz0 = 0;
    std::vector<DevBuf<double>> dense27;
    // ... or a hierarchy from create_from_fine whose level 0 runs the 7-point per-row-coefficient passes (var7) and whose
    // smoothed levels are each var7 or coded by the host (its small levels): indptr0 / nnz0 as above (a var7 level 0 holds
    // exactly the in-grid neighbours, columns ascending: the row pointers place every value), the fine grid (nx, ny, nz), and
    // per level >= 1 the Galerkin operator as a dense [row][7] double array (made at the first update) — the next product's
    // input, and the operator of a host level or the coarsest level
    bool upd7 = false;
    int g7[3] = {0, 0, 0};
    std::vector<DevBuf<double>> dense7;
    // omg_hierarchy_update_kappa: the value array kappa_values writes, nnz0 doubles (made at the first such update)
    DevBuf<double> kappa_vals;
    // omg_level_spmv_dev: the operand and the product in the level's numbering and precision, apart from every vector a
    // cycle or the resident entries use (made at the first such call, grown to the largest level asked for)
    DevBuf<V> mv_x, mv_y;
    // omg_resident_projection (project.hip): cap + 1 vectors of the resident iterate's type (double on a mixed hierarchy, else
    // V) in level 0's numbering, `stride` values apart — the first `size` A-orthonormal, the one behind them free for the next
    // direction; the scalars, the workgroup partials, the status word.  projected: omg_resident_project has run since the
    // last load, so the alphas are this right-hand side's
    struct Projection {
        int cap = 0, size = 0;
        bool projected = false;
        int64_t stride = 0;
        DevBuf<char> vecs;
        DevBuf<double> sc, part;
        DevBuf<int32_t> status;
    } pj;
    // resident state
    bool resident = false;
    // OMG_NO_FUSE=1: never fuse the last smoother set with the residual / norm (A/B switch;
    // results are bit-identical either way, tests/test_gpu_parity.py checks that)
    bool no_fuse = [] { const char *e = getenv("OMG_NO_FUSE"); return e && e[0] == '1'; }();
    // OMG_PLANE=0 (at creation): no plane-pipelined passes; set by omg_hierarchy_use_plane afterwards
    bool no_plane = false;
    // OMG_TAIL_FUSE=0|1|2 (at creation): the coarsest solve and the small levels' up passes in one launch (tail_fuse_depth)
    // omg_hierarchy_tail_info: fused tail launches put on the stream so far, and how many of them by replaying a graph
    int64_t tail_launches = 0, tail_replayed = 0;
    int tail_fuse = [] { const char *e = getenv("OMG_TAIL_FUSE"); return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 2; }();
    // graph: a captured cycle bakes the levels' current / scratch vector pointers in, and a cycle may leave them
    // swapped (out-of-place sweeps: Jacobi, the 27-point pair launches, the plane passes) — so a graph is keyed by the
    // pointer state it was captured FROM and records the state it leaves; a cycle with an odd number of swaps gets a
    // second graph for the other phase (one graph replayed from the wrong phase recomputed cycle 1 forever)
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        int pre = -1, post = -1;
        std::vector<V *> before, after;      // xp, tp of every level
        int64_t tail = 0;                    // fused tail launches (tail_up_kernel) the captured cycle holds
    };
    bool want_graph = false;
    std::vector<GraphSlot> graphs;
    // profile
    unsigned profiling = 0;   // bit c set: time level-0 launches of class c
    std::vector<ProfEvent> events;
    int64_t prof_n[OMG_PROFILE_CLASSES] = {0};
    double prof_ms[OMG_PROFILE_CLASSES] = {0};
    std::vector<hipEvent_t> event_pool;

    Hier() = default;
    Hier(const Hier &) = delete;
    Hier &operator=(const Hier &) = delete;
    ~Hier() {
        for (auto &g : graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        for (auto &e : events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        for (auto &e : event_pool) (void)hipEventDestroy(e);
        if (own) (void)hipStreamDestroy(own);
    }
};

}  // namespace
}  // namespace omg

struct omg_hierarchy {
    std::unique_ptr<omg::Hier<double>> d;
    std::unique_ptr<omg::Hier<float>> f;
    // omg_hierarchy_create_from_fine_semi: the factors of every restriction it built, semi_dim per restriction in the grid's C order
    std::vector<int> semi_factors;
    int semi_dim = 0;
};

namespace omg {
namespace {

void check_diagonal(const omg_csr &A, int level) {
    const int64_t bad = first_row_without_diagonal(A);
    if (bad >= 0)
        throw Error(OMG_ERR_NO_DIAGONAL, "level " + std::to_string(level) + ": row " +
                                             std::to_string(bad) + " has no nonzero diagonal entry");
}

omg_csr view(const HostCsr &A) {
    return omg_csr{A.n_rows, A.n_cols, A.nnz, A.indptr.data(), A.indices.data(), A.data.data()};
}

// The smoother ordering of a level.  The reference's lexicographic sweep first tries the
// one-launch wavefront of march.hip (OMG_MARCH=0: always the level schedule; same bits, tested).
template <typename V>
void order_level(Level<V> &L, const omg_csr &A, int smoother, hipStream_t s) {
    L.march.reset();
    if (smoother == OMG_SMOOTH_GS_LEX && !getenv_flag0("OMG_MARCH")) {
        std::unique_ptr<MarchPlan<V>> plan(new MarchPlan<V>);
        if (plan->build(A, s)) {
            L.march = std::move(plan);
            L.ord = Ordering();
            L.ord.identity = true;
            L.ord.sets = {0, A.n_rows};
            return;
        }
    }
    L.ord = make_ordering(A, smoother);
}

template <typename V>
void build_plan(Level<V> &L) {
    L.plan.clear();
    const int ns = (int)L.A.n_sets();
    int s = 0;
    while (s < ns) {
        auto one_block = [&](int k) { return L.A.set_blk[k + 1] - L.A.set_blk[k] == 1; };
        if (one_block(s)) {
            int e = s + 1;
            while (e < ns && one_block(e)) ++e;
            L.plan.push_back({s, e, e - s >= 2});
            s = e;
        } else {
            L.plan.push_back({s, s + 1, false});
            ++s;
        }
    }
}

template <typename V>
struct Prof {
    Hier<V> *h;
    int idx = -1;
    Prof(Hier<V> *hh, int level, int cls) : h(hh) {
        if (level != 0 || !((h->profiling >> cls) & 1u)) return;
        ProfEvent e;
        e.cls = cls;
        auto get = [&]() {
            hipEvent_t ev;
            if (!h->event_pool.empty()) { ev = h->event_pool.back(); h->event_pool.pop_back(); }
            else OMG_HIP(hipEventCreate(&ev));
            return ev;
        };
        e.a = get();
        e.b = get();
        OMG_HIP(hipEventRecord(e.a, h->stream));
        h->events.push_back(e);
        idx = (int)h->events.size() - 1;
    }
    ~Prof() {
        if (idx >= 0) (void)hipEventRecord(h->events[idx].b, h->stream);
    }
};

template <typename V>
void ensure_format(Hier<V> *h, int l);            // (a plane level's row-kernel side is built on first use: below)

// ---- level operations (device vectors in the level's ordering) ---------------------------
// What the LAST set launch of a Gauss-Seidel smoothing call also produces for its own rows
// (RowMode ROW_GS_RES / ROW_GS_NORM): the residual pass that follows then skips that set.
enum Fuse { FUSE_NONE = 0, FUSE_RESIDUAL = 1, FUSE_NORM = 2 };

// Fusion needs a Gauss-Seidel ordering whose final step is an ordinary set launch.
template <typename V>
bool can_fuse(const Hier<V> *h, const Level<V> &L) {
    if (h->smoother == OMG_SMOOTH_JACOBI || L.plan.empty() || h->no_fuse || L.march || L.line) return false;
    return !L.plan.back().serial;
}

// Can the FIRST launch of a cycle entered at this level also finish the previous cycle's residual
// norm (RowMode ROW_GS_PRENORM / ROW_JACOBI_PRENORM)?  Jacobi: its one launch sees the iterate
// the previous cycle left, for every row.  Gauss-Seidel: only the first set does, so the other
// sets' share must already be there — two sets, the second one's squares left by the fused
// post-smoothing launch (ROW_GS_NORM).
template <typename V>
bool can_prenorm(const Hier<V> *h, const Level<V> &L, int pre, int post) {
    if (pre <= 0 || L.plan.empty() || L.march || L.line) return false;
    if (h->smoother == OMG_SMOOTH_JACOBI) return true;
    return L.A.n_sets() == 2 && post > 0 && can_fuse(h, L) && !L.plan.front().serial && L.plan.size() == 2;
}

// Returns true when the last set launch was fused (its rows' residual / norm is done).
// pre_slot (block-partials array, nullable): the first launch runs in the PRENORM mode and leaves
// the squares of ITS rows' residuals — the previous cycle's — there (caller checked can_prenorm;
// the other set's were put there by that cycle's fused post-smoothing launch, post_slot).
// post_slot (nullable = the level's own partials): where a FUSE_NORM launch puts its squares.
// first_done: the first launch of the first sweep has already been applied (restrict_level wrote
// its result for a zero iterate): skip it.
template <typename V>
bool smooth_level(Hier<V> *h, int l, int iterations, Fuse fuse = FUSE_NONE, double *pre_slot = nullptr,
                  bool first_done = false, double *post_slot = nullptr) {
    ensure_format(h, l);
    Level<V> &L = h->lv[l];
    bool fused = false;
    for (int it = 0; it < iterations; ++it) {
        if (h->smoother == OMG_SMOOTH_JACOBI) {
            if (it == 0 && first_done) continue;
            Prof<V> p(h, l, 0);
            RowArgsT<V> a;
            a.x = L.xp; a.b = L.b.p; a.y = L.tp; a.omega = h->omega;
            if (it == 0 && pre_slot) {
                a.partials = pre_slot;
                launch_rows(L.A, ROW_JACOBI_PRENORM, -1, a, h->stream);
            } else {
                launch_rows(L.A, ROW_JACOBI, -1, a, h->stream);
            }
            std::swap(L.xp, L.tp);
        } else if (L.march) {
            Prof<V> p(h, l, 0);
            L.march->sweep(L.xp, L.b.p, h->stream);
        } else if (L.line) {
            // (a line solve reads nothing of its own line's iterate: no first launch to skip, nothing to fuse — the callers
            // ask can_fuse / can_prenorm / first_sweep_in_restrict, all false for such a level)
            Prof<V> p(h, l, 0);
            L.line->sweep(L.xp, L.b.p, h->stream);
        } else {
            RowArgsT<V> a;
            a.x = L.xp; a.b = L.b.p; a.y = L.xp;
            const bool last_it = it + 1 == iterations;
            for (size_t k = 0; k < L.plan.size(); ++k) {
                const SweepStep &st = L.plan[k];
                if (it == 0 && k == 0 && first_done) continue;
                Prof<V> p(h, l, 0);
                if (st.serial) {
                    launch_gs_serial(L.A, st.set_begin, st.set_end, a, h->stream);
                } else if (last_it && k + 1 == L.plan.size() && fuse != FUSE_NONE && can_fuse(h, L)) {
                    RowArgsT<V> f = a;
                    f.zero = L.r.p;
                    f.partials = (fuse == FUSE_NORM && post_slot) ? post_slot : L.partials.p;
                    launch_rows(L.A, fuse == FUSE_RESIDUAL ? ROW_GS_RES : ROW_GS_NORM, st.set_begin, f, h->stream);
                    fused = true;
                } else if (it == 0 && k == 0 && pre_slot) {
                    RowArgsT<V> f = a;
                    f.partials = pre_slot;                // the first set's blocks; the last set's are in place (ROW_GS_NORM)
                    launch_rows(L.A, ROW_GS_PRENORM, st.set_begin, f, h->stream);
                } else {
                    launch_rows(L.A, ROW_GS, st.set_begin, a, h->stream);
                }
            }
        }
    }
    return fused;
}

// r = b - A x over all sets, or over all but the last one when the smoother has already
// produced the last set's residual.
template <typename V>
void residual_level(Hier<V> *h, int l, V *r_out, bool last_set_done = false) {
    ensure_format(h, l);
    Level<V> &L = h->lv[l];
    Prof<V> p(h, l, 1);
    RowArgsT<V> a;
    a.x = L.xp; a.b = L.b.p; a.y = r_out;
    const int ns = (int)L.A.n_sets();
    launch_rows_range(L.A, ROW_RESIDUAL, 0, last_set_done ? ns - 1 : ns, a, h->stream);
}

// ||b - A x||_2 of level l into h->norm_dev (device scalar); r_out optional.  With
// last_set_done the last set's block partials are already in place.
template <typename V>
void norm_level(Hier<V> *h, int l, V *r_out, bool last_set_done = false, double *out = nullptr) {
    ensure_format(h, l);
    Level<V> &L = h->lv[l];
    {
        Prof<V> p(h, l, 4);
        RowArgsT<V> a;
        a.x = L.xp; a.b = L.b.p; a.y = r_out; a.partials = L.partials.p;
        const int ns = (int)L.A.n_sets();
        launch_rows_range(L.A, r_out ? ROW_RESNORM : ROW_NORM_ONLY, 0, last_set_done ? ns - 1 : ns, a, h->stream);
    }
    launch_sum_sqrt(L.partials.p, L.A.n_blocks(), out ? out : h->norm_dev.p, h->stream);
}

// Can the restriction INTO level C also apply C's first smoothing launch?  A cycle enters C with
// a zero iterate, so that launch — the first set of a Gauss-Seidel sweep, or a whole Jacobi sweep
// — computes x_i = 0 + (b_i - 0) / a_ii (every term of the row sum is v * 0): no gather needed, and
// the restriction's thread holds b_i (RowArgsT::first_diag).  OMG_NO_FIRST_SWEEP=1 switches it off.
template <typename V>
bool first_sweep_in_restrict(const Hier<V> *h, const Level<V> &C, int pre) {
    if (pre <= 0 || !C.diag.p || C.plan.empty() || C.march || C.line || getenv_flag("OMG_NO_FIRST_SWEEP")) return false;
    // (a captured graph bakes the Jacobi ping-pong pointers in: keep two swaps per V(1,1) level there)
    if (h->smoother == OMG_SMOOTH_JACOBI) return !h->want_graph;
    const SweepStep &st = C.plan.front();
    return !st.serial && st.set_begin == 0 && st.set_end == 1;
}

// coarse = R fine; `clear` (nullable, coarse-sized) is zeroed by the same launch — or, with
// first_sweep, set to what the coarse level's first smoothing launch makes of a zero iterate.
template <typename V>
void restrict_level(Hier<V> *h, int l, const V *fine, V *coarse, V *clear = nullptr, bool first_sweep = false) {
    ensure_format(h, l);
    if (first_sweep) ensure_format(h, l + 1);
    Level<V> &L = h->lv[l];
    Prof<V> p(h, l, 2);
    RowArgsT<V> a;
    a.x = fine; a.y = coarse; a.zero = clear; a.ymap = L.r_out.p;
    if (first_sweep && clear) {
        const Level<V> &C = h->lv[l + 1];
        a.first_diag = C.diag.p;
        a.first_jacobi = h->smoother == OMG_SMOOTH_JACOBI;
        a.first_end = int(a.first_jacobi ? C.n : C.A.sets[1]);
        a.omega = h->omega;
    }
    launch_rows(L.R, ROW_SPMV, -1, a, h->stream);
}

// fine += R^T coarse with every stored entry of R times `factor`, rounded once (1: the entries themselves)
template <typename V>
void ensure_prolong_values(Hier<V> *h, int l, double factor) {
    Level<V> &L = h->lv[l];
    if (factor != 1.0 && L.pw_factor != factor) {
        const DevCsrT<V> &T = L.scatter_prolong ? L.R : L.P;
        auto scaled = [&](const DevBuf<V> &src, DevBuf<V> &dst) -> const V * {
            if (!src.p || !src.n) return src.p;
            if (dst.n != src.n) dst.alloc(src.n);
            launch_scale_values<V>(src.p, dst.p, int64_t(src.n), factor, h->stream);
            return dst.p;
        };
        L.pw.data = scaled(T.data, L.pw_data);
        L.pw.vdict = scaled(T.vdict, L.pw_vdict);
        L.pw.pval = scaled(T.pval, L.pw_pval);
        L.pw.vell = scaled(T.vell, L.pw_vell);
        L.pw_factor = factor;
    }
}

template <typename V>
void prolong_add_level(Hier<V> *h, int l, const V *coarse, V *fine, double factor) {
    ensure_format(h, l);
    Level<V> &L = h->lv[l];
    ensure_prolong_values(h, l, factor);
    Prof<V> p(h, l, 3);
    RowArgsT<V> a;
    a.x = coarse; a.y = fine;
    if (factor != 1.0) a.values = &L.pw;
    if (L.scatter_prolong) {
        a.ymap = L.r_out.p;                   // R's rows are in natural coarse order (create())
        launch_rows(L.R, ROW_SCATTER, -1, a, h->stream);
    } else {
        launch_rows(L.P, ROW_AXPY, -1, a, h->stream);
    }
}

template <typename V>
void coarse_solve_level(Hier<V> *h) {
    Level<V> &L = h->lv.back();
    h->coarse.solve(L.b.p, L.xp, h->stream);
}

// What a cycle leaves of the entry level's residual norm (openmg/__init__.py:227)
enum NormState { NORM_NONE = 0, NORM_LAST_SET = 1, NORM_PASS = 2, NORM_S27 = 3 };

// Does the cycle over this level run the 27-point kernels of stencil27.hip?  (Switched with the plane passes.)
// The three vectors a large fused level's passes stream side by side (x, its out-of-place twin, b) come out of ONE
// allocation, each starting 2 MiB-aligned + its stagger (common.h vector_stagger): one request to the driver instead of
// three.  Measured at 256^3 over seven alternating processes (tools/ab_libs.py): 0.2758 against 0.2832 ms per cycle, and
// the spread between processes shrinks from 1.3 % to 0.7 % — where three separate allocations land relative to each
// other is what made a process "fast" or "slow".  OMG_VEC_POOL=0: three allocations.
template <typename V>
void pool_views(Level<V> &L, char *base, size_t span, size_t off1, size_t off2);
struct PoolLayout { size_t span, off1, off2; };
template <typename V>
PoolLayout pool_layout(int64_t n) {
    auto env = [](const char *name, size_t dflt) { const char *e = getenv(name); return e && e[0] ? (size_t(atoll(e)) < 64 ? size_t(atoll(e)) : size_t(atoll(e)) / 64 * 64) : dflt; };
    const size_t off1 = env("OMG_POOL_OFF1", vector_stagger(1)), off2 = env("OMG_POOL_OFF2", vector_stagger(2)), pad = env("OMG_POOL_PAD", 0);
    const size_t MB2 = size_t(2) << 20, bytes = size_t(n) * sizeof(V);
    return {(bytes + 2 * DEVBUF_SLACK + std::max(off1, off2) + MB2 - 1) / MB2 * MB2 + pad, off1, off2};
}
constexpr int64_t POOL_TRIAL_MIN = int64_t(1) << 23;       // levels from 8 M unknowns: the placement of their pool is timed (place_finest_pool)
template <typename V>
bool pooled_vectors(Level<V> &L) {
    static const bool on = [] { const char *e = getenv("OMG_VEC_POOL"); return !(e && e[0] == '0'); }();
    if (!on || !(L.plane || L.s27) || L.n < (int64_t(1) << 20)) return false;
    if (L.pool.p || L.x.p) return true;
    const PoolLayout q = pool_layout<V>(L.n);
    // (every pooled level of a hierarchy out of ONE allocation — OMG_POOL_ARENA, round 4 — measured no different: removed)
    L.pool.alloc(3 * q.span);
    pool_views(L, L.pool.p, q.span, q.off1, q.off2);
    return true;
}

template <typename V>
void pool_views(Level<V> &L, char *base, size_t span, size_t off1, size_t off2) {
    auto env = [](const char *name, size_t dflt) { const char *e = getenv(name); return e && e[0] ? size_t(atoll(e)) : dflt; };
    // order: x, b, x's twin (OMG_POOL_ORDER=0: x, twin, b).  With b in the middle four of four processes ran 0.260 ms per
    // cycle where the other order gave 0.266-0.274 on the same box; on a second box both orders fell into two populations
    // (0.260 / 0.273) from process to process: where the allocation lands physically still matters, and is not ours to choose
    const bool b_mid = env("OMG_POOL_ORDER", 1) != 0;
    L.x.borrow(reinterpret_cast<V *>(base + DEVBUF_SLACK), size_t(L.n));
    // OMG_POOL_TMP_OWN=1 (experiment): x and b from the pool, x's twin an allocation of its own
    static const bool tmp_own = [] { const char *e = experiment_env("OMG_POOL_TMP_OWN"); return e && e[0] == '1'; }();
    if (tmp_own) L.tmp.alloc(size_t(L.n), off1);
    else
    L.tmp.borrow(reinterpret_cast<V *>(base + (b_mid ? 2 : 1) * span + DEVBUF_SLACK + off1), size_t(L.n));
    L.b.borrow(reinterpret_cast<V *>(base + (b_mid ? 1 : 2) * span + DEVBUF_SLACK + off2), size_t(L.n));
    L.pool_span = span; L.pool_off1 = off1; L.pool_off2 = off2;
}

// WHERE the finest level's pool lands in HBM decides the speed of its passes: at 256^3 fp64 a down + up pass takes 174-179 us
// on some allocations and 187-197 us on others — the "two populations of processes" of rounds 3 and 4, in truth a
// property of each allocation (tools/population_probe.py: three hierarchies made in turn by one process: slow, fast, fast;
// neither the virtual addresses nor the clocks say anything; re-placing the level's other arrays changes nothing; a
// physically CONTIGUOUS pool is the slowest of all, 210-220 us; pieces of 2 / 8 / 32 MiB mapped in a shuffled order are
// fast on some boxes every time and on others no better than hipMalloc: profiles/r05_pool_placement.txt).  Nothing a
// process can ask for decides it, so the placement is MEASURED like the tiling: candidates are allocated one after another
// (ordinary and scattered ones in turn, all held until the end so that each is different memory), the level's own down +
// up pass is timed on each, and the search ends when a candidate is good (the passes at 4.5 TB/s of needed bytes), or as fast
// as the best this process has ever had for the shape, or 7 % faster than the slowest of three or more, or after
// OMG_POOL_TRIALS (8); then, where none was good, vector by vector (below).
template <typename V>
void place_finest_pool(Hier<V> *h) {
    // (read at every call, like OMG_PLACE_KEEP_LAST=1 — tests: the newest candidate is kept whatever its time, no early stop)
    const char *env_trials = getenv("OMG_POOL_TRIALS");
    const int trials = env_trials && env_trials[0] ? atoi(env_trials) : 8;
    const bool keep_last = getenv("OMG_PLACE_KEEP_LAST") != nullptr;
    if ((trials < 2 && !getenv("OMG_POOL_REFINE")) || h->lv.size() < 2) return;
    Level<V> &L = h->lv[0], &C = h->lv[1];
    if (!L.plane || !L.pool.p || !L.pool_span || L.n < POOL_TRIAL_MIN || L.tmp.owned) return;
    SetupTimer tm("placement of the finest level's vectors (timed)");
    typename PlanePlan<V>::Coarse c;
    c.map = L.r_out.p;
    c.b = C.b.p;
    c.e = C.xp;
    auto timed = [&]() -> float {
        L.x.zero(h->stream); L.tmp.zero(h->stream); L.b.zero(h->stream); C.x.zero(h->stream);
        return L.plane->time_pair(L.x.p, L.tmp.p, L.b.p, c, h->stream, true, 4);
    };
    static std::mutex mu;
    static std::map<std::array<int64_t, 2>, float> best_ever;       // (unknowns, bytes per value) -> us
    const std::array<int64_t, 2> key = {L.n, int64_t(sizeof(V))};
    float known = 0.0f;
    {
        std::lock_guard<std::mutex> lock(mu);
        const auto it = best_ever.find(key);
        if (it != best_ever.end()) known = it->second;
    }
    // (the candidates are held together: no more than 16 GB of them — five for a 512^3 level)
    const int max_trials = int(std::min<size_t>(size_t(trials), std::max<size_t>(2, (size_t(16) << 30) / (3 * L.pool_span))));
    // "good": the pair of passes moves its 6 w n bytes at 4.5 TB/s or more (179 us at 256^3 fp64: what all three vectors on the
    // fast kind of memory give; one of them elsewhere: 180-186 us) — where a level's shape never reaches that, every candidate is tried
    const double pair_bytes = 6.0 * double(sizeof(V)) * double(L.n);
    auto good = [&](float us) { return pair_bytes / (double(us) * 1e-6) >= 4.5e12; };
    // Round 6: the level's OTHER stream over x — the matrix-free fine-grid SpMV of the metric (omg_resident_spmv_time) — has
    // its own opinion of where x lies: from a pool in 2 or 4 MiB pieces it takes 68 - 72 us whatever its destination, from
    // one in 8 MiB pieces 44 or 60 - 70 (a property of the process: all of its 8 MiB pools or none), from 32 MiB pieces or an
    // ordinary allocation 44 (profiles/r06_pool_piece_size.txt) — while the passes want the small pieces.  So a candidate
    // that is good for the passes is also asked for its SpMV time (into an ordinary allocation), and the search goes on
    // while the best pool is not good for both; between two pools within 2 % of each other for the passes the one the SpMV
    // likes wins.  (OMG_POOL_SPMV=0: the passes alone decide, as before.)
    DevBuf<V> spmv_probe_y;
    hipEvent_t se0 = nullptr, se1 = nullptr;
    const bool ask_spmv = !L.plane->g.jacobi && !getenv_flag0("OMG_POOL_SPMV");
    const bool debug = SetupTimer::on();
    auto spmv_ok = [&]() -> bool {
        if (!ask_spmv) return true;
        if (!spmv_probe_y.p) {
            try { spmv_probe_y.alloc(size_t(L.n)); } catch (const Error &) { (void)hipGetLastError(); return true; }
            OMG_HIP(hipEventCreate(&se0));
            OMG_HIP(hipEventCreate(&se1));
        }
        L.plane->spmv(L.x.p, spmv_probe_y.p, h->stream);
        OMG_HIP(hipEventRecord(se0, h->stream));
        for (int r = 0; r < 6; ++r) L.plane->spmv(L.x.p, spmv_probe_y.p, h->stream);
        OMG_HIP(hipEventRecord(se1, h->stream));
        OMG_HIP(hipEventSynchronize(se1));
        float ms = 0.0f;
        OMG_HIP(hipEventElapsedTime(&ms, se0, se1));
        const double us = 1e3 * double(ms) / 6.0;
        if (debug) fprintf(stderr, "[omg setup]   ... its matrix-free SpMV: %.1f us per launch\n", us);
        return 2.0 * double(sizeof(V)) * double(L.n) / (us * 1e-6) >= 5.15e12;        // (ensure_spmv_y's line: 52 us at 256^3 fp64)
    };
    float best = timed(), worst = best;
    std::vector<DevBuf<char>> held;                       // (the losers: kept until the end, so that a candidate is not the memory just given back)
    if (debug) fprintf(stderr, "[omg setup] finest level's pool, candidate 0 (hipMalloc): %.1f us per down + up\n", best);
    bool best_spmv = true;
    auto settled = [&](int k) { return good(best) || (k >= 3 && best <= 0.93f * worst) || (known > 0.0f && best <= 1.02f * known); };
    if (!keep_last && settled(1)) best_spmv = spmv_ok();
    for (int k = 1; k < max_trials; ++k) {
        if (!keep_last && settled(k) && best_spmv) break;
        DevBuf<char> alt;
        try { alt.alloc(3 * L.pool_span, 0, pool_placement(k)); } catch (const Error &) { (void)hipGetLastError(); break; }       // (no memory for another candidate: what there is stays)
        std::swap(L.pool, alt);                           // L.pool: the candidate, alt: the best so far
        pool_views(L, L.pool.p, L.pool_span, L.pool_off1, L.pool_off2);
        const float t = timed();
        if (debug) fprintf(stderr, "[omg setup] finest level's pool, candidate %d (placement %d): %.1f us per down + up\n", k, pool_placement(k), t);
        worst = std::max(worst, t);
        // (the SpMV is asked only where the passes' answer alone does not decide)
        bool take = keep_last || t < 0.98f * best;
        bool cand_spmv = true;
        if (!keep_last && t <= 1.02f * best) {
            cand_spmv = spmv_ok();
            take = (cand_spmv && !best_spmv) || (t < best && (cand_spmv || !best_spmv)) || t < 0.98f * best;
        }
        if (take) { best = keep_last ? std::min(best, t) : t; best_spmv = cand_spmv; }
        else std::swap(L.pool, alt);                      // the candidate lost
        held.push_back(std::move(alt));
    }
    if (se0) { (void)hipEventDestroy(se0); (void)hipEventDestroy(se1); }
    {
        std::lock_guard<std::mutex> lock(mu);
        float &e = best_ever[key];
        if (e == 0.0f || best < e) e = best;
    }
    pool_views(L, L.pool.p, L.pool_span, L.pool_off1, L.pool_off2);
    // Where no candidate was good, the search goes on vector by vector: an allocation
    // of its own for one of the three (OMG_POOL_REFINE = candidates per vector, default 4), kept where the passes get 1.5 %
    // faster.  (The times BETWEEN the two kinds are steps: 174 us with all three vectors on the fast kind of memory, + 6 us
    // for each one that is not — profiles/r05_pool_placement.txt, section 10.)
    {
        const char *e = getenv("OMG_POOL_REFINE");
        const bool established = good(best) || (known > 0.0f && best <= 1.02f * known);
        const int K = e && e[0] ? atoi(e) : ((keep_last || trials < 2 || established) ? 0 : 4);
        DevBuf<V> *vecs[3] = {&L.tmp, &L.b, &L.x};
        const size_t shifts[3] = {L.pool_off1, L.pool_off2, 0};
        std::vector<DevBuf<V>> losers;
        for (int v = 0; v < 3 && K > 0; ++v) {
            for (int k = 1; k <= K; ++k) {
                DevBuf<V> alt;
                try { alt.alloc(size_t(L.n), shifts[v], pool_placement(k + v)); } catch (const Error &) { (void)hipGetLastError(); break; }
                std::swap(*vecs[v], alt);
                const float t = timed();
                if (debug) fprintf(stderr, "[omg setup] finest level's vector %d, candidate %d (placement %d): %.1f us (best so far %.1f)\n", v, k, pool_placement(k + v), t, best);
                if (t <= 0.985f * best) { best = t; losers.push_back(std::move(alt)); break; }
                std::swap(*vecs[v], alt);
                losers.push_back(std::move(alt));
            }
        }
    }
    L.x.zero(h->stream); L.tmp.zero(h->stream); L.b.zero(h->stream); C.x.zero(h->stream);
    L.xp = L.x.p;
    L.tp = L.tmp.p;
    OMG_HIP(hipStreamSynchronize(h->stream));
}

// The same for a large 27-point level's coefficient tiles (Stencil27Plan::place_tiles, stencil27.hip)
template <typename V>
void place_s27_tiles(Hier<V> *h) {
    if (h->lv.size() < 2) return;
    Level<V> &L = h->lv[0];
    if (!L.s27 || !L.tmp.p || L.n < POOL_TRIAL_MIN) return;
    L.s27->place_tiles(L.x.p, L.tmp.p, L.b.p, h->stream);
    L.x.zero(h->stream); L.tmp.zero(h->stream); L.b.zero(h->stream);
    OMG_HIP(hipStreamSynchronize(h->stream));
}

// The matrix-free SpMV's destination (an allocation of its own: DESIGN.md section 4) is placed like the level's pool — by
// timing: 45 us per launch on some allocations, 57-69 on others at 256^3 fp64.
template <typename V>
void ensure_spmv_y(Hier<V> *h, Level<V> &L) {
    if (L.spmv_y.p) return;
    L.spmv_y.alloc(size_t(L.n));
    // (16 candidates, 0.5 ms each: the first ones a fresh hipMalloc hands out are what the pool's search has just given back —
    // its losers, the slow kind; a bench process whose eight candidates were all of them ran the SpMV at 68 us, round 6)
    static const int trials = [] { const char *e = getenv("OMG_SPMV_TRIALS"); return e && e[0] ? atoi(e) : 16; }();
    if (trials < 2 || !L.plane || L.n < POOL_TRIAL_MIN) return;
    hipEvent_t e0, e1;
    OMG_HIP(hipEventCreate(&e0));
    OMG_HIP(hipEventCreate(&e1));
    auto timed = [&]() -> float {
        L.plane->spmv(L.xp, L.spmv_y.p, h->stream);
        OMG_HIP(hipEventRecord(e0, h->stream));
        for (int r = 0; r < 8; ++r) L.plane->spmv(L.xp, L.spmv_y.p, h->stream);
        OMG_HIP(hipEventRecord(e1, h->stream));
        OMG_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        OMG_HIP(hipEventElapsedTime(&ms, e0, e1));
        return 1e3f * ms / 8.0f;
    };
    float best = timed(), worst = best;
    const bool debug = SetupTimer::on();
    if (debug) fprintf(stderr, "[omg setup] SpMV destination, candidate 0: %.1f us per launch\n", best);
    std::vector<DevBuf<V>> held;
    for (int k = 1; k < trials; ++k) {
        if (2.0 * double(sizeof(V)) * double(L.n) / (double(best) * 1e-6) >= 5.15e12) break;     // good: x read and y written at 5.15 TB/s (52 us at 256^3 fp64; the fast kind 43-45 — 47-50 in these short timings —, the others 57-70)
        DevBuf<V> alt;
        try { alt.alloc(size_t(L.n), 0, pool_placement(k)); } catch (const Error &) { (void)hipGetLastError(); break; }
        std::swap(L.spmv_y, alt);
        const float t = timed();
        if (debug) fprintf(stderr, "[omg setup] SpMV destination, candidate %d (placement %d): %.1f us per launch\n", k, pool_placement(k), t);
        worst = std::max(worst, t);
        if (t < best) best = t;
        else std::swap(L.spmv_y, alt);
        held.push_back(std::move(alt));
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

template <typename V>
bool use_s27(const Hier<V> *h, const Level<V> &L) {
    return L.s27 && !h->no_plane;
}

template <typename V>
bool use_var7(const Hier<V> *h, const Level<V> &L) {
    return L.var7 && !h->no_plane;
}

// Do both halves of a cycle over this level run as plane-pipelined launches?  (Any sweep counts: with
// pre = 0 or post = 0 — the reference's default is V(1,0), openmg/__init__.py:22-23 — the pass runs
// without its relaxation.)
template <typename V>
bool use_plane(const Hier<V> *h, const Level<V> &L) {
    return L.plane && !h->no_plane;
}

// The arm of cycle_body a level takes; PLANE and VAR7 are the "pass" kinds: each half of the cycle is one launch
enum LevelKind { KIND_ROWS, KIND_PLANE, KIND_VAR7, KIND_S27 };
template <typename V>
LevelKind level_kind(const Hier<V> *h, const Level<V> &L) {
    return use_s27(h, L) ? KIND_S27 : use_plane(h, L) ? KIND_PLANE : use_var7(h, L) ? KIND_VAR7 : KIND_ROWS;
}

// The two columns of the table above cycle_body.  x_zero: does the level's first launch NOT read the iterate?  A pass
// level's down pass when it IS the one pre-smoothing sweep (with more, smooth_level runs before it on the iterate as
// stored; with none it forms the iterate's residual), a 27-point level's first sweep, the row kernels never.
template <typename V>
bool enters_without_iterate(const Hier<V> *h, const Level<V> &L, int pre) {
    const LevelKind k = level_kind(h, L);
    return k == KIND_S27 ? pre >= 1 : k != KIND_ROWS && pre == 1;
}
// first_done: does the arm skip (or harmlessly repeat) the first relaxation launch of a zero iterate?
template <typename V>
bool honours_first_done(const Hier<V> *h, const Level<V> &L, int pre) {
    const LevelKind k = level_kind(h, L);
    return k == KIND_ROWS || k == KIND_PLANE || (k == KIND_VAR7 && pre > 1);
}

// openmg/__init__.py:199-234 with the dead work removed: R[l]*b (:205-206) is computed by the
// reference only for its length, and the norm at levels > entry (:227) is discarded by the
// caller (:213 takes [0]); neither changes any returned value.
//
// want_norm: the caller will ask for ||b - A x|| of THIS level right after the cycle.  Returns what
// is already there of it: NORM_LAST_SET — the post-smoother's last set launch has left that set's
// share in the block partials (norm_level(..., last_set_done = true) finishes it); NORM_PASS — the
// up pass of a plane or var7 level has left ALL of it in its workgroup partials (post_slot, or the plan's own
// array); NORM_S27 — the last sweep has left the share of the rows it made final (finish_norm).
// shape: OMG_CYCLE_V / F / W from this level downward (-1, what every entry passes: the hierarchy's setting).
//
// x_zero, first_done: what the caller has made of a zero iterate — enter_child() for the level below, zero_start_cycle()
// for level 0.  One table says when each may arrive, and cycle_body refuses them anywhere else (an internal error):
//
//   level's kind | x_zero: the iterate is zero and has NOT been written | first_done: the first relaxation launch of the
//                | (enters_without_iterate)                             | zero iterate is applied (honours_first_done)
//   -------------+------------------------------------------------------+------------------------------------------------
//   plane        | pre = 1 (pre = 0 from a plane parent, which then     | pre >= 1: smooth_level skips the launch; with
//                | writes the zeros itself: the up pass reads them)     | pre = 1 the down pass relaxes on what it finds
//   var7         | pre = 1                                              | pre > 1 only (smooth_level): the down pass is a
//                |                                                      | whole sweep and cannot skip a launch
//   27-point     | pre >= 1                                             | never
//   row kernels  | never                                                | pre >= 1 (smooth_level)
template <typename V>
int cycle_body(Hier<V> *h, int l, int pre, int post, bool want_norm = false, double *pre_slot = nullptr,
               bool first_done = false, double *post_slot = nullptr, bool x_zero = false, int shape = -1);

// The coarse-grid correction of a cycle of `shape` over level l: level l + 1 is visited once (V; or it is the coarsest
// level, whose direct solve is exact), or twice — F: an F-cycle, then a V-cycle; W: two W-cycles.  The first visit is the
// one a V-cycle makes, with its shortcuts (first_done, x_zero: what the parent has made of the child's zero iterate).  The
// second enters the child with its iterate as the first left it and its right-hand side untouched: nothing cleared, no
// launch skipped, and every path of cycle_body builds the format it needs itself.
template <typename V>
void cycle_children(Hier<V> *h, int l, int pre, int post, int shape, bool first_done, bool x_zero) {
    cycle_body(h, l + 1, pre, post, false, nullptr, first_done, nullptr, x_zero, shape);
    if (shape != OMG_CYCLE_V && l + 1 < (int)h->lv.size() - 1)
        cycle_body(h, l + 1, pre, post, false, nullptr, false, nullptr, false, shape == OMG_CYCLE_F ? OMG_CYCLE_V : OMG_CYCLE_W);
}

// How the first visit of a cycle over level l enters level l + 1 (openmg/__init__.py:191-192: from zeros), for every kind
// of parent.  zero / first: what the child is told (x_zero / first_done).  write: the child's iterate, for the parent's
// restricting launch to clear or, with `first`, to set to the first relaxation of zeros (first_sweep_in_restrict); null:
// nothing to write — the child does not read it, or is the coarsest level (the solve reads b only), or the zeros were
// written by a memset here.  Builds the child's row-kernel format where the child or `first` uses it: a pending format
// launches its build kernels, so WHERE this is called is part of the cycle's dispatch sequence.
template <typename V>
struct ChildEntry { bool zero = false, first = false; V *write = nullptr; };
template <typename V>
ChildEntry<V> enter_child(Hier<V> *h, int l, int pre) {
    ChildEntry<V> e;
    if (l + 1 >= (int)h->lv.size() - 1) return e;
    Level<V> &L = h->lv[l], &C = h->lv[l + 1];
    const LevelKind pk = level_kind(h, L), ck = level_kind(h, C);
    // what the parent's restricting launch can do: rows — clear or first-relax (restrict_level); plane — the same through
    // Coarse::x / diag, no first relaxation out of a 2-D level; var7 and 27-point — neither
    const bool in_launch = pk == KIND_ROWS || pk == KIND_PLANE, may_first = pk == KIND_ROWS || (pk == KIND_PLANE && !L.plane->g.dim2);
    e.zero = enters_without_iterate(h, C, pre);
    // Where a parent knows less or more than that rule (each line is the behaviour as it was, kept launch for launch):
    // a plane parent skips the clear for a plane child only — at pre = 0 too, where the child's down pass does not write
    // the iterate either and its up pass reads it: zeros by a memset
    if (pk == KIND_PLANE) e.zero = ck == KIND_PLANE && pre <= 1;
    // a rows parent clears a var7 child in its restriction launch, a 27-point parent by a memset
    if (ck == KIND_VAR7 && (pk == KIND_ROWS || pk == KIND_S27)) e.zero = false;
    // (a 27-point child runs no row kernel and a 27-point parent builds for no child; a plane parent builds for any)
    if (!e.zero && (pk == KIND_PLANE || (pk != KIND_S27 && ck != KIND_S27))) ensure_format(h, l + 1);
    if (e.zero ? pre == 0 : !in_launch) OMG_HIP(hipMemsetAsync(C.xp, 0, size_t(C.n) * sizeof(V), h->stream));
    if (e.zero || !in_launch) return e;
    e.write = C.xp;
    // (only for a child that skips the launch again; a rows parent never for a var7 child)
    e.first = may_first && honours_first_done(h, C, pre) && !(ck == KIND_VAR7 && pk == KIND_ROWS) && first_sweep_in_restrict(h, C, pre);
    return e;
}

// A pass level's plan: plane (plane.hip) or var7 (var7.hip)
template <typename V, typename Plan>
constexpr bool is_plane_plan = std::is_same<Plan, PlanePlan<V>>::value;
template <typename V, typename Plan>
Plan &pass_plan(Level<V> &L) { if constexpr (is_plane_plan<V, Plan>) return *L.plane; else return *L.var7; }

// The way down over a pass level: all but the last pre-smoothing sweep set by set (in place), then the down pass — the
// last sweep, the residual and the restriction (openmg/__init__.py:201, :209, :210).  c: what the pass was given of the
// child level (the up pass takes the same).  Returns how the child is entered.
template <typename V, typename Plan>
ChildEntry<V> pass_down(Hier<V> *h, int l, int pre, bool x_zero, bool first_done, typename Plan::Coarse &c) {
    Level<V> &L = h->lv[l], &C = h->lv[l + 1];
    Plan &P = pass_plan<V, Plan>(L);
    if (pre > 1) smooth_level(h, l, pre - 1, FUSE_NONE, nullptr, first_done);          // :201
    const ChildEntry<V> e = enter_child(h, l, pre);
    c.map = L.r_out.p;
    c.b = C.b.p;
    if constexpr (is_plane_plan<V, Plan>) {
        c.x = e.write;
        c.diag = e.first ? C.diag.p : nullptr;
        c.first_end = e.first ? int(C.A.sets[1]) : 0;
    }
    {
        Prof<V> p(h, l, 5);                                                             // :201 (last sweep), :209, :210
        if constexpr (is_plane_plan<V, Plan>) P.down(L.xp, L.tp, L.b.p, x_zero, c, h->stream, nullptr, pre >= 1);
        else P.down(L.xp, L.tp, L.b.p, x_zero, c, h->stream, pre >= 1);
    }
    if (pre >= 1) std::swap(L.xp, L.tp);
    if (l == h->pre_level) OMG_HIP(hipMemcpyAsync(h->pre_buf.p, L.xp, size_t(L.n) * sizeof(V), hipMemcpyDeviceToDevice, h->stream));
    return e;
}

// Does the cycle from plane level l downward end in the fused tail launch (plane.hip tail_up_kernel), and with how many
// up passes in it?  2: l is level last - 2 — its child's down pass runs as ever, then ONE launch holds the coarsest solve
// and both up passes; 1: l is level last - 1 — the solve and its up pass; 0: the separate launches.  Only V shapes (F and W
// come back to the level), only post <= 1 (further sweeps run set by set behind the up pass of each level), only block
// levels of a red-black 7-point hierarchy above the 16 x 16 x 16 sine solve, and never for an up pass that leaves a norm.
// The shape that counts is the HIERARCHY's: the second visit of a level in an F-cycle is a V-cycle from there down
// (cycle_children), but an F hierarchy keeps the separate launches on every visit, as omg_hierarchy_level_flags reports.
// OMG_TAIL_FUSE=0|1|2 when the hierarchy is made: never / depth 1 only / depth 2 where it applies (the default).
template <typename V>
int tail_fuse_depth(const Hier<V> *h, int l, int post, int shape) {
    const int last = (int)h->lv.size() - 1;
    if (h->tail_fuse <= 0 || shape != OMG_CYCLE_V || h->cycle_shape != OMG_CYCLE_V || post > 1 || l < 0 || l >= last || !h->coarse.cube16()) return 0;
    auto fits = [&](int k) {
        const Level<V> &K = h->lv[k];
        if (!use_plane(h, K)) return false;
        const Level<V> &D = h->lv[k + 1];
        if (k + 1 == last) return tail_up_level(K.plane->g, 16, 16, 16);
        return use_plane(h, D) && tail_up_level(K.plane->g, D.plane->g.nx, D.plane->g.ny, D.plane->g.nz);
    };
    if (l == last - 1) return fits(l) ? 1 : 0;
    if (l == last - 2 && h->tail_fuse >= 2) return fits(l) && fits(l + 1) ? 2 : 0;
    return 0;
}

// The cycle over a pass level: the down half, the levels below, then the up pass — the prolongation, the first
// post-smoothing sweep and, where asked for and post <= 1, the norm's squares (:214, :220/:224, :216-222, :227) — and the
// further post-smoothing sweeps set by set.
template <typename V, typename Plan>
int pass_cycle(Hier<V> *h, int l, int pre, int post, bool want_norm, bool first_done, double *post_slot, bool x_zero, int shape) {
    Level<V> &L = h->lv[l], &C = h->lv[l + 1];
    Plan &P = pass_plan<V, Plan>(L);
    typename Plan::Coarse c;
    const ChildEntry<V> e = pass_down<V, Plan>(h, l, pre, x_zero, first_done, c);
    double *out = (want_norm && post <= 1) ? (post_slot ? post_slot : P.partials.p) : nullptr;
    if constexpr (is_plane_plan<V, Plan>) if (const int fuse = !out ? tail_fuse_depth(h, l, post, shape) : 0) {
        // plane levels only: the rest of the cycle below this level in one launch — (depth 2: the child's down pass as ever,
        // then) the coarsest solve and the up passes of the levels above it (plane.hip tail_up_kernel)
        TailUp<V> u;
        u.top = &P.g; u.x_old = L.xp; u.x_new = L.tp; u.b = L.b.p;
        u.cmap = L.r_out.p;
        if (fuse == 2) {
            typename Plan::Coarse cc;
            pass_down<V, Plan>(h, l + 1, pre, e.zero, e.first, cc);
            u.mid = &C.plane->g; u.mid_x_old = C.xp; u.mid_x_new = C.tp; u.mid_b = C.b.p;
            u.cmap = C.r_out.p;
        }
        Level<V> &Z = h->lv.back();
        u.cb = Z.b.p; u.cx = Z.xp; u.tables = h->coarse.sine.p; u.lambda = h->coarse.lambda.p;
        u.sweep = post >= 1;
        {
            Prof<V> p(h, l, 6);
            launch_tail_up<V>(u, h->stream);
            ++h->tail_launches;
        }
        if (fuse == 2) std::swap(C.xp, C.tp);
        std::swap(L.xp, L.tp);
        return NORM_NONE;
    }
    cycle_children(h, l, pre, post, shape, e.first, e.zero);                              // :213
    c.e = C.xp;
    {
        Prof<V> p(h, l, 6);
        if constexpr (is_plane_plan<V, Plan>) P.up(L.xp, L.tp, L.b.p, c, out, h->stream, nullptr, post >= 1);
        else P.up(L.xp, L.tp, L.b.p, c, out, h->stream, post >= 1);
    }
    std::swap(L.xp, L.tp);
    if (post > 1)
        return smooth_level(h, l, post - 1, want_norm ? FUSE_NORM : FUSE_NONE, nullptr, false, post_slot) ? NORM_LAST_SET : NORM_NONE;
    return out ? NORM_PASS : NORM_NONE;
}

template <typename V>
int cycle_body(Hier<V> *h, int l, int pre, int post, bool want_norm, double *pre_slot, bool first_done, double *post_slot, bool x_zero,
               int shape) {
    if (shape < 0) shape = h->cycle_shape;
    const int last = (int)h->lv.size() - 1;
    if (l >= last) {
        coarse_solve_level(h);
        return NORM_NONE;
    }
    Level<V> &L = h->lv[l];
    Level<V> &C = h->lv[l + 1];
    const LevelKind kind = level_kind(h, L);
    // (a plane level also takes x_zero at pre = 0, from a plane parent that has written the zeros)
    OMG_REQUIRE(!x_zero || enters_without_iterate(h, L, pre) || (kind == KIND_PLANE && pre == 0),
                "internal: x_zero for a level whose first launch reads the iterate");
    OMG_REQUIRE(!first_done || honours_first_done(h, L, pre), "internal: first_done for a level that cannot skip its first relaxation");
    if (kind == KIND_PLANE) return pass_cycle<V, PlanePlan<V>>(h, l, pre, post, want_norm, first_done, post_slot, x_zero, shape);
    if (kind == KIND_VAR7) return pass_cycle<V, Var7Plan<V>>(h, l, pre, post, want_norm, first_done, post_slot, x_zero, shape);
    if (kind == KIND_S27) {
        // 27-point per-row-coefficient level (stencil27.hip): sweeps as four pair launches, out of place; the last
        // pre-smoothing sweep leaves the residuals of its final rows, the others' are formed inside the restriction
        Stencil27Plan<V> &P = *L.s27;
        bool zero_now = x_zero;
        for (int it = 0; it < pre; ++it) {                      // :201
            Prof<V> p(h, l, 0);
            P.sweep(L.xp, L.tp, L.b.p, zero_now, (it == 0 && !zero_now) ? pre_slot : nullptr, it + 1 == pre, nullptr, h->stream);
            std::swap(L.xp, L.tp);
            zero_now = false;
        }
        if (l == h->pre_level) OMG_HIP(hipMemcpyAsync(h->pre_buf.p, L.xp, size_t(L.n) * sizeof(V), hipMemcpyDeviceToDevice, h->stream));
        const ChildEntry<V> e = enter_child(h, l, pre);                                // :191-192
        {
            Prof<V> p(h, l, 1);
            P.residual_restrict(L.xp, L.b.p, pre >= 1, L.r_out.p, C.b.p, h->stream);                  // :209, :210
        }
        cycle_children(h, l, pre, post, shape, false, e.zero);                                         // :213
        {
            Prof<V> p(h, l, 3);
            P.prolong(L.xp, C.xp, L.r_out.p, h->stream);                                               // :214, :220 / :224
        }
        double *nslot = want_norm ? (post_slot ? post_slot : P.partials.p) : nullptr;
        for (int it = 0; it < post; ++it) {                     // :216-222
            Prof<V> p(h, l, 0);
            const bool fin = it + 1 == post && want_norm;
            P.sweep(L.xp, L.tp, L.b.p, false, nullptr, fin, fin ? nslot : nullptr, h->stream);
            std::swap(L.xp, L.tp);
        }
        return want_norm ? NORM_S27 : NORM_NONE;
    }
    const bool res_done = smooth_level(h, l, pre, FUSE_RESIDUAL, pre_slot, first_done);   // :201 (+ last set's share of :209)
    if (l == h->pre_level) OMG_HIP(hipMemcpyAsync(h->pre_buf.p, L.xp, size_t(L.n) * sizeof(V), hipMemcpyDeviceToDevice, h->stream));
    residual_level(h, l, L.r.p, res_done);                          // :209
    // :210, and the coarse cycle's initial=None -> zeros (:191-192) cleared by the same launch —
    // or already relaxed once (first_sweep_in_restrict)
    const ChildEntry<V> e = enter_child(h, l, pre);
    restrict_level<V>(h, l, L.r.p, C.b.p, e.write, e.first);
    cycle_children(h, l, pre, post, shape, e.first, e.zero);                             // :213
    prolong_add_level<V>(h, l, C.xp, L.xp, h->over);                // :214, :220/:224
    if (post > 0)
        return smooth_level(h, l, post, want_norm ? FUSE_NORM : FUSE_NONE, nullptr, false, post_slot) ? NORM_LAST_SET : NORM_NONE;   // :216-222
    return NORM_NONE;
}

// ||b - A x|| of level l into out (device scalar; null: h->norm_dev) after a cycle that returned `state`
template <typename V>
void finish_norm(Hier<V> *h, int l, int state, double *out = nullptr) {
    if (state == NORM_PASS) {
        Level<V> &L = h->lv[l];
        const bool plane = level_kind(h, L) == KIND_PLANE;
        launch_sum_sqrt(plane ? L.plane->partials.p : L.var7->partials.p, plane ? L.plane->g.n_wg : L.var7->n_wg,
                        out ? out : h->norm_dev.p, h->stream);
    } else if (state == NORM_S27) {
        // the rows the last post-smoothing launch made final have left their squares (segment 3); the others' now
        Level<V> &L = h->lv[l];
        Stencil27Plan<V> &P = *L.s27;
        {
            Prof<V> p(h, l, 4);
            P.norm(L.xp, L.b.p, P.have67, P.partials.p, h->stream);
        }
        launch_sum_sqrt(P.partials.p, int64_t(4) * P.g.n_wg, out ? out : h->norm_dev.p, h->stream);
    } else {
        norm_level<V>(h, l, nullptr, state == NORM_LAST_SET, out);
    }
}

// Host vectors are double for either V.  A double level in its natural ordering copies
// straight through; otherwise the vector is staged in `nat` and permuted / converted by one
// gather (idx == NULL: conversion only).
template <typename V>
constexpr bool direct_io(const Level<V> &L) { return std::is_same<V, double>::value && L.ord.identity; }

template <typename V>
void ensure_nat(Hier<V> *h, int l) {
    Level<V> &L = h->lv[l];
    if (!direct_io(L) && L.nat.n < size_t(std::max<int64_t>(L.n, 1))) L.nat.alloc(std::max<int64_t>(L.n, 1));
}

template <typename V>
void load_vec(Hier<V> *h, int l, const double *host, V *dst) {
    Level<V> &L = h->lv[l];
    if (direct_io(L)) {
        OMG_HIP(hipMemcpyAsync(dst, host, L.n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        ensure_nat(h, l);
        L.nat.upload(host, L.n, h->stream);
        launch_gather<double, V>(L.nat.p, L.ord.identity ? nullptr : L.perm.p, dst, L.n, h->stream);
    }
}

// The wavefront sweeps give up waiting for a face after a bounded number of polls instead of
// hanging the device; whoever reads results back asks whether that has happened.
template <typename V>
void check_plane_status(Hier<V> *h, uint32_t st) {
    if (!st) return;
    OMG_HIP(hipMemsetAsync(h->plane_status.p, 0, sizeof(st), h->stream));
    throw Error(OMG_ERR_HIP, "a plane-pipelined pass gave up waiting for a neighbouring wave of its workgroup (status " +
                             std::to_string(st) + "): the results since the last read-back are not valid");
}

// (have_plane_status: the caller has already copied the plane passes' status word back with its own results)
template <typename V>
void check_march(Hier<V> *h, bool have_plane_status = false, uint32_t plane_st = 0) {
    for (Level<V> &L : h->lv)
        if (L.march && L.march->timed_out(h->stream))
            throw Error(OMG_ERR_HIP, "lexicographic wavefront sweep timed out waiting for a neighbouring tile's face; the iterate and "
                                     "the hand-over slots of this hierarchy are no longer consistent: destroy it and build a new one");
    // the plane passes' waves wait for their neighbour waves a bounded number of polls (plane.hip WAVE_SYNC_SPIN)
    if (h->plane_status.p && !have_plane_status) {
        OMG_HIP(hipMemcpyAsync(&plane_st, h->plane_status.p, sizeof(plane_st), hipMemcpyDeviceToHost, h->stream));
        OMG_HIP(hipStreamSynchronize(h->stream));
    }
    check_plane_status(h, plane_st);
}

template <typename V>
void fetch_vec(Hier<V> *h, int l, const V *src, double *host) {
    Level<V> &L = h->lv[l];
    // (large vectors through the pinned staging buffers of download_staged: the runtime's own copy into a pageable
    // NumPy array ran at ~10 GB/s)
    if (direct_io(L)) {
        download_staged(host, src, size_t(L.n) * sizeof(double), h->stream);
    } else {
        ensure_nat(h, l);
        launch_scatter<V, double>(src, L.ord.identity ? nullptr : L.perm.p, L.nat.p, L.n, h->stream);
        download_staged(host, L.nat.p, size_t(L.n) * sizeof(double), h->stream);
    }
    check_march(h);
}

// The same two for a caller whose vectors already live in HBM (double, natural numbering): device-to-device
template <typename V>
void load_vec_dev(Hier<V> *h, int l, const double *dev, V *dst) {
    Level<V> &L = h->lv[l];
    if (direct_io(L)) OMG_HIP(hipMemcpyAsync(dst, dev, L.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else launch_gather<double, V>(dev, L.ord.identity ? nullptr : L.perm.p, dst, L.n, h->stream);
}
template <typename V>
void fetch_vec_dev(Hier<V> *h, int l, const V *src, double *dev) {
    Level<V> &L = h->lv[l];
    if (direct_io(L)) OMG_HIP(hipMemcpyAsync(dev, src, L.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else launch_scatter<V, double>(src, L.ord.identity ? nullptr : L.perm.p, dev, L.n, h->stream);
}

template <typename V>
double read_norm(Hier<V> *h) {
    double v = 0.0;
    uint32_t st = 0;
    OMG_HIP(hipMemcpyAsync(&v, h->norm_dev.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (h->plane_status.p) OMG_HIP(hipMemcpyAsync(&st, h->plane_status.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    OMG_HIP(hipStreamSynchronize(h->stream));
    check_march(h, true, st);
    return v;
}

template <typename V>
void drop_graph(Hier<V> *h) {
    for (auto &g : h->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

template <typename V>
std::vector<V *> pointer_state(const Hier<V> *h) {
    std::vector<V *> s;
    s.reserve(2 * h->lv.size());
    for (const Level<V> &L : h->lv) { s.push_back(L.xp); s.push_back(L.tp); }
    return s;
}

// One level-0 cycle + residual norm into norm_dev; optionally replayed from a hipGraph.
template <typename V>
void run_cycle0(Hier<V> *h, int pre, int post) {
    const bool single = h->lv.size() == 1;
    auto body = [&]() {
        const int part = cycle_body(h, 0, pre, post, !single);
        if (!single) finish_norm(h, 0, part);                 // :227
        else OMG_HIP(hipMemsetAsync(h->norm_dev.p, 0, sizeof(double), h->stream));   // :232
    };
    if (!h->want_graph || h->profiling) {
        body();
        return;
    }
    const std::vector<V *> cur = pointer_state(h);
    auto restore = [&](const std::vector<V *> &st) {
        for (size_t l = 0; l < h->lv.size(); ++l) { h->lv[l].xp = st[2 * l]; h->lv[l].tp = st[2 * l + 1]; }
    };
    typename Hier<V>::GraphSlot *slot = nullptr;
    for (auto &g : h->graphs)
        if (g.pre == pre && g.post == post && g.before == cur) slot = &g;
    if (!slot) {
        // (two phases of one (pre, post) at most: anything else — other sweep counts, a state no captured cycle
        // leaves — starts over)
        if (h->graphs.size() >= 2 || (!h->graphs.empty() && (h->graphs[0].pre != pre || h->graphs[0].post != post))) drop_graph(h);
        hipGraph_t g = nullptr;
        const int64_t tail_before = h->tail_launches;
        OMG_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        try {
            body();
        } catch (...) {
            (void)hipStreamEndCapture(h->stream, &g);
            if (g) (void)hipGraphDestroy(g);
            restore(cur);
            throw;
        }
        OMG_HIP(hipStreamEndCapture(h->stream, &g));
        typename Hier<V>::GraphSlot ns;
        ns.pre = pre;
        ns.post = post;
        ns.before = cur;
        ns.after = pointer_state(h);               // (the capture ran the host side of the cycle: the swaps are made)
        ns.tail = h->tail_launches - tail_before;  // (captured, not run: counted with every replay)
        h->tail_launches = tail_before;
        hipError_t e = hipGraphInstantiate(&ns.exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) {
            restore(cur);
            throw Error(OMG_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        }
        h->graphs.push_back(std::move(ns));
        slot = &h->graphs.back();
    }
    OMG_HIP(hipGraphLaunch(slot->exec, h->stream));
    h->tail_launches += slot->tail;
    h->tail_replayed += slot->tail;
    restore(slot->after);
}

template <typename V>
void check_level(const Hier<V> *h, int level) {
    OMG_REQUIRE(level >= 0 && level < (int)h->lv.size(), "level out of range");
}

// omg_vcycle, omg_vcycle_ex, omg_vcycle_dev: one cycle entered at `level` from x_in (null: zeros) into x_out; x_pre (nullable,
// may be x_in) receives the iterate after the pre-smoothing — the input's copy, or zeros, where none ran.  Returns the
// residual norm (0 at the coarsest level, whose solve is direct).  The vectors are double in natural numbering: host
// arrays, read back once the norm is (fetch_vec synchronises), or — dev — arrays in HBM, everything enqueued and the
// norm's read-back the one synchronisation at the end: the outputs are complete on return either way.
template <typename V>
double level_cycle(Hier<V> *hh, bool dev, int level, const double *b, const double *x_in, double *x_out, double *x_pre, int pre, int post) {
    Level<V> &L = hh->lv[level];
    const int last = (int)hh->lv.size() - 1;
    const size_t bytes = size_t(L.n) * sizeof(double);
    auto load = [&](const double *src, V *dst) { dev ? load_vec_dev(hh, level, src, dst) : load_vec(hh, level, src, dst); };
    auto fetch = [&](const V *src, double *dst) { dev ? fetch_vec_dev<V>(hh, level, src, dst) : fetch_vec<V>(hh, level, src, dst); };
    hh->resident = false;
    load(b, L.b.p);
    if (x_in) load(x_in, L.xp);
    else OMG_HIP(hipMemsetAsync(L.xp, 0, size_t(L.n) * sizeof(V), hh->stream));
    const bool want_pre = x_pre && level < last && pre > 0;
    int part = NORM_NONE;
    {
        struct Reset { int &v; ~Reset() { v = -1; } } reset{hh->pre_level};      // (cycle_body copies to pre_buf at pre_level)
        if (want_pre) {
            if (hh->pre_buf.n < size_t(L.n)) hh->pre_buf.alloc(size_t(L.n));
            hh->pre_level = level;
        }
        part = cycle_body(hh, level, pre, post, level < last);
    }
    double nv = 0.0;
    if (level < last) {
        finish_norm(hh, level, part);
        if (!dev) nv = read_norm(hh);
    }
    fetch(L.xp, x_out);
    if (want_pre) fetch(hh->pre_buf.p, x_pre);
    else if (x_pre && x_in && x_pre != x_in) {
        if (dev) OMG_HIP(hipMemcpyAsync(x_pre, x_in, bytes, hipMemcpyDeviceToDevice, hh->stream));
        else std::memcpy(x_pre, x_in, bytes);
    } else if (x_pre && !x_in) {
        if (dev) OMG_HIP(hipMemsetAsync(x_pre, 0, bytes, hh->stream));
        else std::memset(x_pre, 0, bytes);
    }
    if (dev) {
        if (level < last) nv = read_norm(hh);
        else { OMG_HIP(hipStreamSynchronize(hh->stream)); check_march(hh); }
    }
    return nv;
}

// A hierarchy made with OMG_NULLSPACE_CONSTANT: the resident right-hand side is projected when it is loaded, the resident
// iterate when it is fetched (include/openmg_hip.h); the cycle entries in between do not project.
template <typename V>
bool has_nullspace(const Hier<V> *h) { return h->coarse.nullspace == OMG_NULLSPACE_CONSTANT; }
// x <- x - mean(x) over n values of T on the hierarchy's stream; the sum that was removed stays in proj_scratch[PROJECT_MAX_WG]
template <typename V, typename T>
void project_vec(Hier<V> *h, T *x, int64_t n) {
    if (h->proj_scratch.n < size_t(PROJECT_SCRATCH)) h->proj_scratch.alloc(size_t(PROJECT_SCRATCH));
    launch_project_mean<T>(x, n, h->proj_scratch.p, h->stream);
}


// The row-kernel side of a smoothed level: A and R (and P where the prolongation cannot scatter over R) in
// the device format of common.h, the residual vector, the block partials, the sweep plan.  A, R: natural
// numbering (the caller's, or — for a plane level, later — what its plan describes).
template <typename V>
void build_format(Hier<V> *h, int l, const omg_csr &A, const omg_csr &R) {
    Level<V> &L = h->lv[l];
    const bool id = L.ord.identity;
    {
        HostCsr Ap;
        { SetupTimer tm("permute A"); Ap = permute_csr(A, id ? nullptr : L.ord.perm.data(), id ? nullptr : L.ord.inv.data()); }
        SetupTimer tm("encode + upload A");
        L.A.upload(Ap, L.ord.sets, h->stream);
        // the diagonal as the sweeps form it: restrict_level / omg_hierarchy_cycle_dev apply this
        // level's first relaxation of a zero iterate with it (level 0: only when it is needed)
        if (l >= 1) {
            L.diag.alloc(std::max<int64_t>(L.n, 1));
            launch_diagonal(L.A, L.diag.p, h->stream);
        }
    }
    const Ordering &co = h->lv[l + 1].ord;
    SetupTimer tm("R (and P): permute, encode, upload");
    HostCsr Rp, Rn;
    const HostCsr *r_used = &Rp;
    if (co.identity) {
        Rp = permute_csr(R, nullptr, id ? nullptr : L.ord.inv.data());
        L.R.upload(Rp, {}, h->stream);
    } else {
        // Restriction rows stay in NATURAL coarse order and write through a map (r_out) into the
        // coarse level's ordering: consecutive rows are then consecutive aggregates,
        // whose fine unknowns are consecutive inside each colour segment (dense
        // gathers).  In the coarse COLOUR order consecutive rows are every other
        // aggregate and each gather used half of every cache line (measured: 480 MB
        // read for 343 MB algorithmic).
        Rn = permute_csr(R, nullptr, id ? nullptr : L.ord.inv.data());
        r_used = &Rn;
        L.R.upload(Rn, {}, h->stream);
    }
    {   // OMG_PROLONG_SCATTER=0: always the explicit transpose (identical bits, tested)
        const char *e = getenv("OMG_PROLONG_SCATTER");
        bool ok = !(e && e[0] == '0') && L.R.all_pattern();
        if (ok) {
            std::vector<char> seen(size_t(L.n), 0);
            for (int32_t c : r_used->indices) {
                if (seen[c]) { ok = false; break; }
                seen[c] = 1;
            }
        }
        L.scatter_prolong = ok;
    }
    if (!L.scatter_prolong) {
        // the explicit transpose P = R^T (rows in this level's ordering, columns in the next
        // level's) is only built where the prolongation cannot run as a scatter over R's rows
        if (!co.identity) Rp = permute_csr(R, co.perm.data(), id ? nullptr : L.ord.inv.data());
        HostCsr Pt = transpose_csr(Rp);
        L.P.upload(Pt, {}, h->stream);
    }
    L.pw_factor = 0.0;                                             // (a second edition of the prolongation's values belongs to the arrays just replaced)
    L.r.alloc(L.n);
    if (h->smoother == OMG_SMOOTH_JACOBI && !L.tmp.p) { L.tmp.alloc(L.n); L.tp = L.tmp.p; }
    L.partials.alloc(L.A.n_blocks() + SUM_FOLD);
    build_plan(L);
    OMG_HIP(hipStreamSynchronize(h->stream));
}

// A plane level's row-kernel side, on first use.
template <typename V>
void ensure_format(Hier<V> *h, int l) {
    if (l < 0 || l >= (int)h->lv.size() || !h->lv[l].format_pending) return;
    Level<V> &L = h->lv[l];
    SetupTimer tm("plane / 27-point level: row-kernel format on first use");
    materialise_ordering(L.ord);                                   // (a hierarchy set up on the device keeps its closed-form
    if (l + 1 < (int)h->lv.size()) materialise_ordering(h->lv[l + 1].ord);   //  orderings as device arrays only until here)
    // (a 27-point level: from the operator PADDED to 27 entries per row, so that the row kernels associate every row's
    // sum as the kernels of stencil27.hip do)
    const HostCsr A = L.s27 ? L.s27->operator_csr(h->stream) : L.var7 ? L.var7->operator_csr(h->stream) : L.plane->operator_csr();
    const HostCsr R = L.s27 ? L.s27->restriction_csr() : L.var7 ? L.var7->restriction_csr() : L.plane->restriction_csr();
    L.format_pending = false;
    build_format(h, l, view(A), view(R));
}
template <typename V>
void ensure_format(const Hier<V> *h, int l) { ensure_format(const_cast<Hier<V> *>(h), l); }


// ---- The steps of setup that create() and create_from_fine() share, in the order both take them ----

// A new handle: its stream and the norm's slot.
template <typename V>
std::unique_ptr<Hier<V>> new_handle(int smoother, double omega, int nullspace) {
    std::unique_ptr<Hier<V>> h(new Hier<V>);
    h->smoother = smoother;
    h->omega = omega;
    h->coarse.nullspace = nullspace;       // (every build() of this hierarchy's coarse solver honours it: at setup and in update_fine)
    OMG_HIP(hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
    h->stream = h->own;
    h->norm_dev.alloc(1);
    return h;
}

// The coarsest level: n rows in their natural order, one set.
template <typename V>
void coarsest_level(Level<V> &L, int64_t n) {
    L.n = n;
    L.ord.identity = true;
    L.ord.sets = {0, L.n};
}

// The coarsest operator on the device and its factorisation (at setup: on the helper thread's stream; in an update: on the handle's)
template <typename V>
void factorise_coarsest(Hier<V> *h, const HostCsr &Ac, hipStream_t s) {
    Level<V> &L = h->lv.back();
    L.A.upload(Ac, L.ord.sets, s);
    h->coarse.build(Ac, s);                // factors in double, stored in V
}

// The coarsest operator is factored once (reference: SuperLU factorisation on every
// cycle; here: explicit inverse or substructuring along the band, common.h CoarseSolver).
// That is thousands of tiny dependent launches, so it runs on a helper thread with its own
// stream while the calling thread does the index work of the smoothed levels.  The factors are
// always computed in double; a float hierarchy stores their rounding.
// An error of the work is kept until rethrow().  Declared AFTER the handle and whatever else the work reads: the destructor
// joins, so an exception on the calling thread ends the helper before any of that dies.
struct CoarseThread {
    int code = OMG_OK;
    std::string msg;
    std::thread t;                         // (last: code and msg exist when it starts)
    static int current_device() { int device = 0; OMG_HIP(hipGetDevice(&device)); return device; }
    void run(int device, const std::function<void(hipStream_t)> &work) {
        hipStream_t s = nullptr;
        SetupTimer tm("coarse factorisation (helper thread)");
        try {
            OMG_HIP(hipSetDevice(device));
            OMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            work(s);
        } catch (const Error &e) {
            code = e.code;
            msg = e.what();
        } catch (const std::exception &e) {
            code = OMG_ERR_HIP;
            msg = e.what();
        }
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    }
    explicit CoarseThread(std::function<void(hipStream_t)> work) : t(&CoarseThread::run, this, current_device(), std::move(work)) {}
    CoarseThread(const CoarseThread &) = delete;
    CoarseThread &operator=(const CoarseThread &) = delete;
    ~CoarseThread() { finish(); }
    void finish() { if (t.joinable()) t.join(); }
    void rethrow() const { if (code != OMG_OK) throw Error(code, msg); }        // (after finish())
};

// OMG_PLANE_CHECK_ORDER=1 (tests): a fused level's closed-form ordering is the greedy colouring's (a Jacobi plane level keeps
// its natural ordering: nothing to compare)
void check_closed_form(const omg_csr &A, int smoother, const Ordering &ord, const char *what) {
    if (!getenv_flag("OMG_PLANE_CHECK_ORDER") || smoother != OMG_SMOOTH_GS_COLOUR) return;
    const Ordering g = make_ordering(A, smoother);
    OMG_REQUIRE(g.sets == ord.sets && g.perm == ord.perm && g.inv == ord.inv, what);
}

// The ordering maps of level l on the device: perm (slot -> natural row, for the gathers at the host boundary) and, for the
// level above the coarsest, r_out — restriction rows are in NATURAL coarse order and write through this map into the coarse
// level's ordering (build_format; the plane passes use it too).  closed_form_by_kernel: a closed-form ordering's maps are
// written by a kernel (create_from_fine: nothing of it is on the host); otherwise, and for every other ordering, the host's
// arrays are uploaded, each upload waited for.
template <typename V>
void level_maps(Hier<V> *h, int l, bool closed_form_by_kernel) {
    Level<V> &L = h->lv[size_t(l)];
    if (!L.ord.identity) {
        L.perm.alloc(L.n);
        if (closed_form_by_kernel && L.ord.closed_form) {
            fill_ordering_device(L.ord.closed_form, L.ord.cf_nx, L.ord.cf_ny, L.ord.cf_nz, L.perm.p, nullptr, h->stream);
        } else {
            L.perm.upload(L.ord.perm.data(), L.n, h->stream);
            OMG_HIP(hipStreamSynchronize(h->stream));
        }
    }
    if (size_t(l) + 1 >= h->lv.size()) return;
    const Level<V> &C = h->lv[size_t(l) + 1];
    const Ordering &co = C.ord;
    if (co.identity) return;
    L.r_out.alloc(size_t(C.n));
    if (closed_form_by_kernel && co.closed_form) {
        fill_ordering_device(co.closed_form, co.cf_nx, co.cf_ny, co.cf_nz, nullptr, L.r_out.p, h->stream);
    } else {
        L.r_out.upload(co.inv.data(), co.inv.size(), h->stream);
        OMG_HIP(hipStreamSynchronize(h->stream));
    }
}

// The scratch vector of a smoothed level that runs a fused path.  (Apart from level_vectors: the level's format is made
// between the two, and the order of the allocations decides where the large vectors land — place_finest_pool.)
template <typename V>
void level_scratch(Hier<V> *h, int l) {
    Level<V> &L = h->lv[size_t(l)];
    if (L.plane && !pooled_vectors(L)) L.tmp.alloc(L.n, vector_stagger(1));
    if (L.s27 && !pooled_vectors(L)) L.tmp.alloc(L.n);
    if (L.var7 && !L.tmp.p) L.tmp.alloc(L.n);
}

// The iterate and the right-hand side of level l, and what the cycle starts from.
template <typename V>
void level_vectors(Hier<V> *h, int l) {
    Level<V> &L = h->lv[size_t(l)];
    if (!L.x.p) {
        L.x.alloc(std::max<int64_t>(L.n, 1));
        L.b.alloc(std::max<int64_t>(L.n, 1), L.plane ? vector_stagger(2) : 0);
    }
    // (finite from the start: the 27-point sweeps multiply the slot of a neighbour that does not exist — a zero
    // coefficient — with whatever the vectors hold at the index the slot's shift lands on)
    L.x.zero(h->stream);
    L.tmp.zero(h->stream);
    L.xp = L.x.p;
    L.tp = L.tmp.p;
    if (SetupTimer::on() && l == 0) fprintf(stderr, "[omg setup] level 0 vectors at x %p  tmp %p  b %p\n", (void *)L.x.p, (void *)L.tmp.p, (void *)L.b.p);
}

// The end of setup: the large levels' tilings, the wait for the helper thread, the placements, the helper's error.
template <typename V>
void finish_setup(const std::unique_ptr<Hier<V>> &h, CoarseThread &inverter) {
    for (size_t l = 0; l + 1 < h->lv.size(); ++l) {
        // the large levels' tilings: measured, not modelled (plane.hip choose_tiles; tune() skips the small ones)
        if (!h->lv[l].plane || !h->lv[l].tmp.p) continue;
        SetupTimer tm("plane tiling of a large level");
        Level<V> &L = h->lv[l], &C = h->lv[l + 1];
        L.x.zero(h->stream); L.tmp.zero(h->stream); L.b.zero(h->stream); C.x.zero(h->stream);
        typename PlanePlan<V>::Coarse c;
        c.map = L.r_out.p;
        c.b = C.b.p;
        c.e = C.xp;
        L.plane->tune(L.xp, L.tp, L.b.p, c, h->stream, l == 0);
        OMG_HIP(hipStreamSynchronize(h->stream));
    }
    // (first: the coarse factorisation's kernels on their own stream beside the timed passes would make a candidate look slow
    // and the decision depend on the overlap)
    { SetupTimer tm("wait for the coarse factorisation"); inverter.finish(); }
    place_finest_pool(h.get());
    place_s27_tiles(h.get());
    inverter.rethrow();                    // (an error of the calling thread has propagated before this one)
    OMG_HIP(hipStreamSynchronize(h->stream));
}


// Which fused path a smoothed level runs, decided once for both constructors: the plane passes, else the 27-point kernels,
// else the 7-point passes with per-row coefficients; the first plan whose build takes the level is moved into it.  The three
// callables build a plan from what the caller holds of the level (host CSRs: build; operators in HBM: build_device) and
// say whether the level qualifies, leaving its closed-form ordering in L.ord.  beyond_plane: may the level take the two
// kinds after the plane passes (create_from_fine: 3-D grids only).  none: the caller orders the level itself.
enum class Fused { none, plane, s27, var7 };
template <typename V, typename Plane, typename S27, typename Var7>
Fused fused_level(Hier<V> *h, Level<V> &L, bool beyond_plane, Plane &&plane, S27 &&s27, Var7 &&var7) {
    const int smoother = h->smoother;
    if (smoother == OMG_SMOOTH_GS_COLOUR || smoother == OMG_SMOOTH_JACOBI) {
        SetupTimer tp("plane-pipelined passes: does the level qualify (+ its parity ordering)");
        std::unique_ptr<PlanePlan<V>> plan(new PlanePlan<V>);
        L.march.reset();
        // (weighted Jacobi: 2-D levels only — BASELINE configs[1] — in their natural ordering)
        if (plane(*plan)) {
            if (!h->plane_status.p) { h->plane_status.alloc(1); h->plane_status.zero(h->stream); }
            plan->status = h->plane_status.p;
            L.plane = std::move(plan);
            return Fused::plane;
        }
        std::unique_ptr<Stencil27Plan<V>> p27(new Stencil27Plan<V>);
        if (smoother == OMG_SMOOTH_GS_COLOUR && beyond_plane && s27(*p27)) {
            L.s27 = std::move(p27);
            return Fused::s27;
        }
    }
    // (OMG_PLANE=0 asks for the set-by-set schedule: no fused path of any kind)
    if (smoother == OMG_SMOOTH_GS_COLOUR && beyond_plane && !getenv_flag0("OMG_VAR7") && !getenv_flag0("OMG_PLANE")) {
        SetupTimer tv("7-point level with per-row coefficients: does it qualify (+ its coefficient arrays, its parity ordering)");
        std::unique_ptr<Var7Plan<V>> v7(new Var7Plan<V>);
        if (var7(*v7)) {
            L.var7 = std::move(v7);
            return Fused::var7;
        }
    }
    return Fused::none;
}

template <typename V>
std::unique_ptr<Hier<V>> create(int n_levels, const omg_csr *A, const omg_csr *R, int smoother,
                                double omega, int nullspace = OMG_NULLSPACE_NONE) {
    using H = Hier<V>;
    using Lv = Level<V>;
    OMG_REQUIRE(n_levels >= 1, "n_levels must be >= 1");
    OMG_REQUIRE(A != nullptr && (n_levels == 1 || R != nullptr), "A / R array is null");
    // (OMG_SMOOTH_LINE_WRAP is a flag on the four line codes alone: 11 .. 14)
    OMG_REQUIRE((smoother >= OMG_SMOOTH_GS_LEX && smoother <= OMG_SMOOTH_LINE_Z) || is_line_smoother(smoother), "unknown smoother");
    const bool line_wrap = is_line_smoother(smoother) && (smoother & OMG_SMOOTH_LINE_WRAP) != 0;
    const int line_code = smoother & ~OMG_SMOOTH_LINE_WRAP;
    for (int l = 0; l < n_levels; ++l) {
        validate_csr(A[l], ("A[" + std::to_string(l) + "]").c_str());
        OMG_REQUIRE(A[l].n_rows == A[l].n_cols, "A[l] must be square");
        if (l + 1 < n_levels) {
            validate_csr(R[l], ("R[" + std::to_string(l) + "]").c_str());
            OMG_REQUIRE(R[l].n_cols == A[l].n_rows && R[l].n_rows == A[l + 1].n_rows,
                        "R[l] shape does not match A[l], A[l+1]");
            check_diagonal(A[l], l);
        }
    }
    require_device();
    std::unique_ptr<H> h = new_handle<V>(smoother, omega, nullspace);
    h->lv.resize(n_levels);
    // (the line smoother's axis: the caller's, or the strongest of level 0 — before the helper thread starts: a refusal costs nothing)
    if (is_line_smoother(smoother) && n_levels > 1) {
        try {
            h->line_axis = line_code == OMG_SMOOTH_LINE ? line_auto_axis(A[0], line_wrap) : line_code - OMG_SMOOTH_LINE_X;
        } catch (const Error &e) {
            throw Error(e.code, std::string("level 0: ") + e.what());
        }
    }
    coarsest_level(h->lv.back(), A[n_levels - 1].n_rows);
    // (the copy of the caller's coarsest operator is made on the helper thread too)
    CoarseThread inverter([&](hipStream_t s) { factorise_coarsest(h.get(), permute_csr(A[n_levels - 1], nullptr, nullptr), s); });
    // orderings first (restrictions need both neighbours')
    for (int l = 0; l + 1 < n_levels; ++l) {
        Lv &L = h->lv[l];
        L.n = A[l].n_rows;
        if (is_line_smoother(smoother)) {
            SetupTimer tl("line smoother: the level's grid, its ordering, the lines' factorisations");
            std::unique_ptr<LinePlan<V>> plan(new LinePlan<V>);
            try {
                plan->build(A[l], h->line_axis, L.ord, h->stream, line_wrap);
            } catch (const Error &e) {
                throw Error(e.code, "level " + std::to_string(l) + ": " + e.what());
            }
            const int dim = plan->g.nz > 1 ? 3 : 2;
            if (l == 0) h->line_dim = dim;
            else if (dim != h->line_dim)
                throw Error(OMG_ERR_UNSUPPORTED, "level " + std::to_string(l) + ": the line smoother needs a grid of the dimension of level 0's on every smoothed level");
            L.line = std::move(plan);
            continue;
        }
        const Fused kind = fused_level(h.get(), L, true,
                                       [&](PlanePlan<V> &p) { return p.build(A[l], R[l], L.ord, smoother == OMG_SMOOTH_JACOBI, omega); },
                                       [&](Stencil27Plan<V> &p) { return p.build(A[l], R[l], L.ord, h->stream); },
                                       [&](Var7Plan<V> &p) { return p.build(A[l], R[l], L.ord, h->stream); });
        if (kind != Fused::none) {
            check_closed_form(A[l], smoother, L.ord, kind == Fused::s27 ? "internal: the octant ordering differs from the greedy colouring"
                                                                        : "internal: the parity ordering differs from the greedy colouring");
            continue;
        }
        SetupTimer tm("ordering (colouring / level schedule / wavefront plan)");
        order_level(L, A[l], smoother, h->stream);
    }
    for (int l = 0; l < n_levels; ++l) {
        Lv &L = h->lv[l];
        // (every ordering is on the host here, a closed-form one too — the host builds write it out —, and is uploaded)
        level_maps(h.get(), l, false);
        if (l + 1 < n_levels) {
            level_scratch(h.get(), l);
            // (OMG_PLANE_LAZY=0, the format at creation, is this route's switch alone: the device route always leaves a fused level's to its first use)
            if ((L.plane || L.s27 || L.var7) && !experiment_flag0("OMG_PLANE_LAZY")) L.format_pending = true;
            else if (L.s27) { L.format_pending = true; ensure_format(h.get(), l); }      // (from the padded operator)
            else build_format(h.get(), l, A[l], R[l]);
        }
        level_vectors(h.get(), l);
    }
    finish_setup(h, inverter);
    return h;
}

// mgSolve's setup (openmg/__init__.py:103-109) without the host in between: restrictionList + coeffecientList on the
// device (galerkin_chain_device), every smoothed level qualified THERE for a fused path (plane passes / 2-D tile passes /
// 27-point kernels) — the grid is the caller's problemShape —, orderings and slot maps written by kernels.  What comes
// back to the host: the coarsest operator (a few thousand entries) for its factorisation.  A hierarchy with a level
// that does not qualify takes the ordinary route (its operators are fetched once): the result is the same object.
// dev0 (omg_hierarchy_create_from_kappa): the fine operator is this device CSR — sorted, square, written by kappa.hip —
// and A0 is not looked at; the chain takes it over, everything after that is the one sequence.
template <typename V>
std::unique_ptr<Hier<V>> create_from_fine(const omg_csr &A0, int dim, const int64_t *shape, int n_restrictions, int smoother, double omega,
                                          int nullspace = OMG_NULLSPACE_NONE, DevCsrPlain *dev0 = nullptr) {
    using H = Hier<V>;
    using Lv = Level<V>;
    refuse_line_smoother(smoother, dev0 ? "omg_hierarchy_create_from_kappa" : "omg_hierarchy_create_from_fine");
    OMG_REQUIRE(dim >= 2 && dim <= 3 && shape && n_restrictions >= 1, "device setup: 2-D / 3-D grids, at least one restriction");
    OMG_REQUIRE(smoother >= OMG_SMOOTH_GS_LEX && smoother <= OMG_SMOOTH_JACOBI, "unknown smoother");
    if (!dev0) {
        validate_csr(A0, "A_in");
        OMG_REQUIRE(A0.n_rows == A0.n_cols, "A_in must be square");
    }
    // the reference's restriction is the plain aggregation when its quirky second-axis offset shape[0] (Q6) equals the
    // true one: first and last extent equal
    OMG_REQUIRE(shape[0] == shape[dim - 1], "device setup: first and last extent must be equal");
    require_device();
    std::unique_ptr<H> h = new_handle<V>(smoother, omega, nullspace);
    std::vector<DevCsrPlain> dA, dR;
    if (dev0) galerkin_chain_device(std::move(*dev0), dim, shape, n_restrictions, dA, dR, h->stream);
    else galerkin_chain_device(A0, dim, shape, n_restrictions, dA, dR, h->stream);
    const int n_levels = n_restrictions + 1;
    h->lv.resize(size_t(n_levels));
    const double w = 1.0 / double(1 << dim);
    auto dims = [&](int l, int &nx, int &ny, int &nz) {
        nx = int(shape[dim - 1] >> l);
        ny = int(shape[dim - 2] >> l);
        nz = dim == 3 ? int(shape[0] >> l) : 1;
    };
    bool all = smoother == OMG_SMOOTH_GS_COLOUR || (smoother == OMG_SMOOTH_JACOBI && dim == 2);
    // Round 6: a hierarchy whose LARGE levels qualify (7-point levels with per-row coefficients take the fused passes from
    // 128^3 up) keeps them on the device; the small levels below — a few hundred thousand rows — are fetched and ordered / coded
    // by the host as the ordinary route would (host_level), each a few milliseconds.
    constexpr int64_t HOST_LEVEL_MAX = int64_t(1) << 19;
    std::vector<char> host_level((size_t)(n_levels), 0);
    std::vector<HostCsr> hostA((size_t)(n_levels)), hostR((size_t)(n_levels));
    bool any_var7 = false;
    for (int l = 0; all && l + 1 < n_levels; ++l) {
        Lv &L = h->lv[size_t(l)];
        L.n = dA[size_t(l)].n_rows;
        int nx, ny, nz;
        dims(l, nx, ny, nz);
        SetupTimer tp("device setup: does the level qualify for a fused path");
        const DevCsrPlain &M = dA[size_t(l)];
        // (the 27-point and the per-row-coefficient kernels are 3-D ones)
        const Fused kind = fused_level(h.get(), L, dim == 3,
                                       [&](PlanePlan<V> &p) { return p.build_device(M, nx, ny, nz, w, L.ord, smoother == OMG_SMOOTH_JACOBI, omega, h->stream); },
                                       [&](Stencil27Plan<V> &p) { return p.build_device(M, nx, ny, nz, w, L.ord, h->stream); },
                                       [&](Var7Plan<V> &p) { return p.build_device(M, nx, ny, nz, w, L.ord, h->stream); });
        any_var7 = any_var7 || kind == Fused::var7;
        if (kind != Fused::none) continue;
        if (any_var7 && L.n <= HOST_LEVEL_MAX) {
            host_level[size_t(l)] = 1;
            hostA[size_t(l)] = download_csr(dA[size_t(l)], h->stream);
            hostR[size_t(l)] = download_csr(dR[size_t(l)], h->stream);
            check_diagonal(view(hostA[size_t(l)]), l);
            SetupTimer tm("ordering (colouring / level schedule / wavefront plan)");
            order_level(L, view(hostA[size_t(l)]), smoother, h->stream);
            continue;
        }
        all = false;
    }
    if (!all) {
        // some level needs the host's orderings and codings: fetch the operators once, then the ordinary route
        SetupTimer tm("device setup: a level does not qualify: operators fetched, ordinary route");
        std::vector<HostCsr> hA, hR;
        for (auto &M : dA) hA.push_back(download_csr(M, h->stream));
        for (auto &M : dR) hR.push_back(download_csr(M, h->stream));
        dA.clear();
        dR.clear();
        std::vector<omg_csr> vA, vR;
        for (auto &M : hA) vA.push_back(view(M));
        for (auto &M : hR) vR.push_back(view(M));
        h.reset();
        return create<V>(n_levels, vA.data(), vR.data(), smoother, omega, nullspace);
    }
    // the coarsest operator: to the host for its factorisation
    const HostCsr Ac = download_csr(dA.back(), h->stream);
    coarsest_level(h->lv.back(), Ac.n_rows);
    check_diagonal(view(Ac), n_levels - 1);
    CoarseThread inverter([&](hipStream_t s) { factorise_coarsest(h.get(), Ac, s); });
    {
        // (new coefficients later: omg_hierarchy_update_fine needs the fine pattern's row pointers, nothing else of the operators;
        // 27-point levels throughout, or 7-point var7 levels with host-coded levels below them)
        bool all27 = dim == 3;
        for (int l = 0; l + 1 < n_levels; ++l) all27 = all27 && bool(h->lv[size_t(l)].s27);
        bool all7 = dim == 3 && bool(h->lv[0].var7);
        for (int l = 0; l + 1 < n_levels; ++l) all7 = all7 && (h->lv[size_t(l)].var7 || host_level[size_t(l)]);
        if (all27 || all7) {
            h->indptr0 = std::move(dA[0].indptr);
            h->nnz0 = dA[0].nnz;
        }
        if (all7) {
            h->upd7 = true;
            h->g7[0] = int(shape[2]); h->g7[1] = int(shape[1]); h->g7[2] = int(shape[0]);
        }
    }
    dA.clear();                                                    // (the fused paths hold what they need of the operators)
    dR.clear();
    for (int l = 0; l < n_levels; ++l) {
        Lv &L = h->lv[size_t(l)];
        // (a closed-form ordering exists on the device only: a kernel writes its maps; a level the host ordered is uploaded)
        level_maps(h.get(), l, true);
        if (l + 1 < n_levels) {
            level_scratch(h.get(), l);
            if (host_level[size_t(l)]) {
                // (the restriction's rows land in the coarse level's ordering: a closed-form one is written out for that)
                materialise_ordering(h->lv[size_t(l) + 1].ord);
                build_format(h.get(), l, view(hostA[size_t(l)]), view(hostR[size_t(l)]));
            } else {
                L.format_pending = true;
            }
        }
        level_vectors(h.get(), l);
    }
    // (this route's alone: create() has never waited here.  No result can depend on it, the stream orders the work; what the
    // tuning passes of finish_setup measure might, so each route keeps what it had)
    OMG_HIP(hipStreamSynchronize(h->stream));
    finish_setup(h, inverter);
    return h;
}

// mgSolve's setup with a coarsening factor of 1 or 2 per axis and restriction: the chain of restrictions and
// Galerkin products — under 'auto' with the couplings kernel and the rule between them — is made in HBM
// (galerkin_chain_semi_device), fetched once and handed to create(): a level whose restriction is not the full 2^dim
// aggregation runs the set-by-set row kernels (the fused passes bake that aggregate into their LDS images), a level further
// down whose restriction is full again qualifies for them there as in every hierarchy made from lists.  The result is the
// object create() makes from the same lists.  odd = OMG_ODD_MERGE: a restriction with a three-cell
// aggregate is one more restriction that is not the 2^dim aggregation — its level fails every fused plan's check of R.
template <typename V>
std::unique_ptr<Hier<V>> create_from_fine_semi(const omg_csr &A0, int dim, const int64_t *shape, int n_restrictions, const int *factors,
                                               int64_t min_size, int odd, int smoother, double omega, int nullspace, std::vector<int> &used) {
    refuse_line_smoother(smoother, "omg_hierarchy_create_from_fine_semi");
    OMG_REQUIRE(smoother >= OMG_SMOOTH_GS_LEX && smoother <= OMG_SMOOTH_JACOBI, "unknown smoother");
    validate_csr(A0, "A_in");
    OMG_REQUIRE(A0.n_rows == A0.n_cols, "A_in must be square");
    require_device();
    std::vector<HostCsr> hA, hR;
    {
        hipStream_t s = nullptr;
        OMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        try {
            std::vector<DevCsrPlain> dA, dR;
            galerkin_chain_semi_device(A0, dim, shape, n_restrictions, factors, min_size, odd, dA, dR, used, s);
            SetupTimer tm("device setup: semicoarsened operators fetched, ordinary route");
            // (level 0 is the caller's own operator: not fetched)
            for (size_t l = 1; l < dA.size(); ++l) hA.push_back(download_csr(dA[l], s));
            for (auto &M : dR) hR.push_back(download_csr(M, s));
        } catch (...) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
            throw;
        }
        OMG_HIP(hipStreamSynchronize(s));
        OMG_HIP(hipStreamDestroy(s));
    }
    std::vector<omg_csr> vA = {A0}, vR;
    for (auto &M : hA) vA.push_back(view(M));
    for (auto &M : hR) vR.push_back(view(M));
    return create<V>(int(vA.size()), vA.data(), vR.data(), smoother, omega, nullspace);
}

// A grid level's operator from its dense [row][S] form on the device, slot e the neighbour at offset slots[e] (ascending in
// column): the in-grid neighbours whose value is not exactly zero, columns ascending — what the Galerkin chain hands
// create_from_fine (SciPy's csr_matmat drops exact zeros).
struct SlotOffset { int dx, dy, dz; };
// 7-point levels: -K, -J, -I, D, +I, +J, +K
std::vector<SlotOffset> slots7() { return {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}}; }
// 27-point levels: x fastest
std::vector<SlotOffset> slots27() {
    std::vector<SlotOffset> s;
    for (int sl = 0; sl < 27; ++sl) s.push_back({sl % 3 - 1, (sl / 3) % 3 - 1, sl / 9 - 1});
    return s;
}
template <typename V>
HostCsr csr_from_dense(Hier<V> *h, const DevBuf<double> &dense, const std::vector<SlotOffset> &slots, int nx, int ny, int nz) {
    const int64_t n = int64_t(nx) * ny * nz;
    const size_t S = slots.size();
    std::vector<double> d(size_t(n) * S);
    OMG_HIP(hipMemcpyAsync(d.data(), dense.p, d.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    OMG_HIP(hipStreamSynchronize(h->stream));
    HostCsr A;
    A.n_rows = A.n_cols = n;
    A.indptr.resize(size_t(n) + 1);
    A.indices.reserve(d.size());
    A.data.reserve(d.size());
    for (int64_t r = 0; r < n; ++r) {
        A.indptr[size_t(r)] = int32_t(A.indices.size());
        const int64_t i = r % nx, j = (r / nx) % ny, k = r / (int64_t(nx) * ny);
        for (size_t e = 0; e < S; ++e) {
            const SlotOffset &o = slots[e];
            const bool present = i + o.dx >= 0 && i + o.dx < nx && j + o.dy >= 0 && j + o.dy < ny && k + o.dz >= 0 && k + o.dz < nz;
            const double v = d[size_t(r) * S + e];
            if (!present || v == 0.0) continue;
            A.indices.push_back(int32_t(r + (int64_t(o.dz) * ny + o.dy) * nx + o.dx));
            A.data.push_back(v);
        }
    }
    A.indptr[size_t(n)] = int32_t(A.indices.size());
    A.nnz = int64_t(A.indices.size());
    return A;
}

// The opening of an update: the value array checked, the handle idle, no captured cycle of the old operator, the new values
// on the device (up: the owner of a host array's copy).  Returns the device array.
template <typename V>
const double *update_values(Hier<V> *h, const double *vals, int64_t nnz, bool on_device, DevBuf<double> &up) {
    OMG_REQUIRE(vals && nnz == h->nnz0, "omg_hierarchy_update_fine: the value array must have the fine operator's number of entries");
    OMG_HIP(hipStreamSynchronize(h->stream));
    drop_graph(h);
    if (on_device) return vals;
    SetupTimer tm("update: upload the new values");
    up.alloc(size_t(nnz));
    OMG_HIP(hipMemcpyAsync(up.p, vals, size_t(nnz) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return up.p;
}

// The close of an update: the coarsest operator factorised anew.
template <typename V>
void refactorise_coarsest(Hier<V> *h, const HostCsr &Ac) {
    {
        SetupTimer tm("update: coarse factorisation");
        h->coarse.retain_workspace = true;                          // (a hierarchy that is updated once is updated again)
        factorise_coarsest(h, Ac, h->stream);
    }
    OMG_HIP(hipStreamSynchronize(h->stream));
}

// The plain 2 x 2 x 2 aggregation of an nx x ny x nz grid, weight 1/8, columns ascending (setup_device.hip restriction_kernel
// for a grid whose first and last extents are equal)
HostCsr aggregation_csr(int nx, int ny, int nz) {
    const int64_t n = int64_t(nx) * ny * nz, hx = nx / 2, hy = ny / 2, nc = n / 8;
    HostCsr R;
    R.n_rows = nc;
    R.n_cols = n;
    R.nnz = n;
    R.indptr.resize(size_t(nc) + 1);
    R.indices.resize(size_t(n));
    R.data.assign(size_t(n), 1.0 / 8);
    for (int64_t cr = 0; cr <= nc; ++cr) R.indptr[size_t(cr)] = int32_t(8 * cr);
    for (int64_t cr = 0; cr < nc; ++cr) {
        const int64_t I = cr % hx, J = (cr / hx) % hy, K = cr / (hx * hy);
        int64_t p = 8 * cr;
        for (int dk = 0; dk < 2; ++dk)
            for (int dj = 0; dj < 2; ++dj)
                for (int di = 0; di < 2; ++di, ++p) R.indices[size_t(p)] = int32_t(((2 * K + dk) * ny + 2 * J + dj) * nx + 2 * I + di);
    }
    (void)nz;
    return R;
}

// New coefficients for the fine operator of a hierarchy that create_from_fine set up with a var7 level 0 (Hier::upd7): every
// Galerkin product re-formed in HBM by var7_rap — level 0's seven arrays written in the same pass that reads the new values,
// each var7 level's arrays as the coarse side of the pass above it, every product in double as a dense [row][7] array —; a
// host-coded level is then rebuilt in full from its product, as create_from_fine codes it: its greedy colouring (and with it
// its ordering, its format, the slot map of the level above) follows the pattern, and an exact zero of the new product
// changes the pattern.  The coarsest operator is factorised anew.  The result is the hierarchy a fresh setup of the new
// operator gives, bit for bit.
template <typename V>
void update_fine_var7(Hier<V> *h, const double *vals, int64_t nnz, bool on_device) {
    const int last = (int)h->lv.size() - 1;
    DevBuf<double> up;
    vals = update_values(h, vals, nnz, on_device, up);
    if (h->dense7.size() != h->lv.size()) h->dense7.resize(h->lv.size());
    DevBuf<unsigned long long> d_err(size_t(2 * last));
    std::vector<unsigned long long> err(size_t(2 * last));
    {
        SetupTimer tm("update: Galerkin products of the 7-point chain (one pass per level)");
        OMG_HIP(hipMemsetAsync(d_err.p, 0xFF, err.size() * sizeof(unsigned long long), h->stream));
        for (int l = 0; l < last; ++l) {
            Level<V> &L = h->lv[size_t(l)];
            DevBuf<double> &out = h->dense7[size_t(l) + 1];
            const size_t need = size_t(h->lv[size_t(l) + 1].n) * 7;
            if (out.n < need) out.alloc(need);
            Var7Plan<V> *C = l + 1 < last ? h->lv[size_t(l) + 1].var7.get() : nullptr;
            var7_rap<V>(l == 0 ? h->indptr0.p : nullptr, l == 0 ? vals : h->dense7[size_t(l)].p, h->g7[0] >> l, h->g7[1] >> l, h->g7[2] >> l,
                        1.0 / 8, l == 0 ? L.var7.get() : nullptr, C, out.p, d_err.p + 2 * l, h->stream);
            if (L.var7) L.format_pending = true;                   // (its row-kernel side, if it was ever built, is of the old operator)
        }
        OMG_HIP(hipMemcpyAsync(err.data(), d_err.p, err.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        OMG_HIP(hipStreamSynchronize(h->stream));
    }
    h->lv[0].diag.release();                                       // (made from the row-kernel format on first use: of the old operator)
    for (int l = 0; l < last; ++l)
        for (int q = 0; q < 2; ++q) {
            const unsigned long long e = err[size_t(2 * l + q)];
            if (e == ~0ull) continue;
            const int lev = (e >> 62) ? l + 1 : l;
            const std::string where = "omg_hierarchy_update_fine: level " + std::to_string(lev) + ": row " + std::to_string((e & ~(3ull << 62)) - 1);
            // (what a fresh setup of this operator raises: a zero diagonal is a missing one; any other value a var7 level does
            // not take makes the level one of another kind, which an update cannot turn this one into)
            if (q == 0) throw Error(OMG_ERR_NO_DIAGONAL, where + " has no nonzero diagonal entry");
            throw Error(OMG_ERR_INVALID, where + ": a value that is not finite in the level's precision, a diagonal that rounds to zero "
                                                 "there, or a coupling that is exactly zero (a fresh setup would not run this level as var7)");
        }
    std::vector<HostCsr> hA(size_t(last) + 1);
    {
        SetupTimer tm("update: host-coded levels' and the coarsest operators, from their products");
        for (int l = 1; l <= last; ++l) {
            if (l < last && h->lv[size_t(l)].var7) continue;
            hA[size_t(l)] = csr_from_dense(h, h->dense7[size_t(l)], slots7(), h->g7[0] >> l, h->g7[1] >> l, h->g7[2] >> l);
            check_diagonal(view(hA[size_t(l)]), l);
        }
    }
    for (int l = 1; l < last; ++l) {
        Level<V> &L = h->lv[size_t(l)], &U = h->lv[size_t(l) - 1];
        if (L.var7) continue;
        SetupTimer tm("update: a host-coded level's ordering");
        order_level(L, view(hA[size_t(l)]), h->smoother, h->stream);
        if (L.ord.identity) {
            L.perm.release();
            U.r_out.release();
        } else {
            if (L.perm.n != size_t(L.n)) L.perm.alloc(size_t(L.n));
            L.perm.upload(L.ord.perm.data(), size_t(L.n), h->stream);
            if (U.r_out.n != size_t(L.n)) U.r_out.alloc(size_t(L.n));
            U.r_out.upload(L.ord.inv.data(), size_t(L.n), h->stream);          // (the restriction of the level above writes through it)
        }
        OMG_HIP(hipStreamSynchronize(h->stream));
    }
    for (int l = 1; l < last; ++l) {
        if (h->lv[size_t(l)].var7) continue;
        SetupTimer tm("update: a host-coded level's format");
        const HostCsr R = aggregation_csr(h->g7[0] >> l, h->g7[1] >> l, h->g7[2] >> l);
        materialise_ordering(h->lv[size_t(l) + 1].ord);
        build_format(h, l, view(hA[size_t(l)]), view(R));
    }
    refactorise_coarsest(h, hA[size_t(last)]);
}

// New coefficients for the fine operator of a hierarchy that create_from_fine set up with 27-point levels throughout (same
// pattern, new values: BASELINE configs[4]'s "Galerkin RAP rebuilt on-device"; openmg/operators.py:144-188 is what the
// reference would run again): level 0 is re-tiled and every Galerkin product re-formed in HBM by s27_rap_kernel — each
// operator of the chain read once —, the coarsest operator factorised anew.  vals: the CSR's data array, host or device.
template <typename V>
void update_fine(Hier<V> *h, const double *vals, int64_t nnz, bool on_device) {
    if (h->upd7) { update_fine_var7(h, vals, nnz, on_device); return; }
    OMG_REQUIRE(h->indptr0.p, "omg_hierarchy_update_fine: needs a hierarchy made by omg_hierarchy_create_from_fine whose smoothed levels all run the 27-point kernels, or whose level 0 runs the 7-point var7 passes and whose smoothed levels are var7 or host-coded");
    const int last = (int)h->lv.size() - 1;
    DevBuf<double> up;
    vals = update_values(h, vals, nnz, on_device, up);
    if (h->dense27.size() != h->lv.size()) h->dense27.resize(h->lv.size());
    for (int l = 0; l < last; ++l) {
        SetupTimer tm("update: tiles + Galerkin product of a level (one pass)");
        Level<V> &L = h->lv[size_t(l)];
        DevBuf<double> &out = h->dense27[size_t(l) + 1];
        const size_t need = size_t(h->lv[size_t(l) + 1].n) * 27;
        if (out.n < need) out.alloc(need);
        Stencil27Plan<V> *C = l + 1 < last ? h->lv[size_t(l) + 1].s27.get() : nullptr;
        // (a level's tiles below the finest were written as the `coarse` of the level above)
        L.s27->rap_from(l == 0 ? h->indptr0.p : nullptr, l == 0 ? vals : h->dense27[size_t(l)].p, l == 0, out.p, C, h->stream);
        L.format_pending = true;                                   // (its row-kernel side, if it was ever built, is of the old operator)
    }
    // the coarsest operator: its present, nonzero entries as CSR (what the Galerkin chain hands create_from_fine), factorised anew
    const Stencil27Plan<V> &P = *h->lv[size_t(last) - 1].s27;
    const HostCsr Ac = csr_from_dense(h, h->dense27[size_t(last)], slots27(), P.g.hx, P.g.hy, P.g.hz);
    check_diagonal(view(Ac), last);
    refactorise_coarsest(h, Ac);
}

// A throw-away single operator for the standalone entry points.
struct OneShot {
    DevCsr A;
    hipStream_t s = nullptr;
    OneShot() { require_device(); OMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~OneShot() { if (s) (void)hipStreamDestroy(s); }
};

// Runs f(Hier<V> *) on whichever instantiation the handle holds.
template <typename H, typename F>
void with(H *h, F &&f) { omg::with(h, "null hierarchy", std::forward<F>(f)); }

// One level-0 V-cycle from a zero iterate: the right-hand side in L.b, the result left in L.xp (openmg/__init__.py:191-192;
// omg_hierarchy_cycle_dev, and the preconditioner of omg_resident_pcg)
template <typename V>
void zero_start_cycle(Hier<V> *hh, int pre, int post) {
    Level<V> &L = hh->lv[0];
    bool first = false, zero_in = false;
    if (hh->lv.size() > 1) {
        zero_in = enters_without_iterate(hh, L, pre);
        if (!zero_in) {
            // x starts from zero: the first relaxation launch is a pointwise b / diag (restrict_level).  The
            // diagonal comes from the row-kernel format, which a plane level builds on first use: BEFORE it
            // (with the format still pending the diagonal stayed uninitialised)
            if (pre > 0) {
                ensure_format(hh, 0);
                if (!L.diag.p && !getenv_flag("OMG_NO_FIRST_SWEEP")) {
                    L.diag.alloc(std::max<int64_t>(L.n, 1));
                    launch_diagonal(L.A, L.diag.p, hh->stream);
                }
            }
            first = pre > 0 && first_sweep_in_restrict(hh, L, pre);
            if (first) {
                const bool jac = hh->smoother == OMG_SMOOTH_JACOBI;
                launch_first_relaxation<V>(L.b.p, L.diag.p, L.xp, L.n, jac ? L.n : L.A.sets[1], jac, hh->omega, hh->stream);
            } else {
                OMG_HIP(hipMemsetAsync(L.xp, 0, L.n * sizeof(V), hh->stream));
            }
        }
    }
    cycle_body(hh, 0, pre, post, false, nullptr, first, nullptr, zero_in);
}

// ---- omg_resident_pcg: flexible CG on level 0 with the zero-start V-cycle as its preconditioner (pcg.hip) ---------------
// r lives where the cycle reads its right-hand side (L.b), z where it leaves its iterate (L.xp); x, p, p2, q and a copy
// of b are the hierarchy's own.  A plane level (red-black, whole grid) forms p2 = z + beta p, q = A p2 and (p2, q) in one
// launch; any other level updates p, runs the level's SpMV and the dot as three.
template <typename V>
bool pcg_fused_plane(const Hier<V> *hh, const Level<V> &L) {
    return hh->lv.size() > 1 && use_plane(hh, L) && !L.plane->g.jacobi && L.plane->g.z_base == 0 && L.plane->g.z_end == L.plane->g.nz;
}

template <typename V>
PcgPlane pcg_plane_of(const Level<V> &L) {
    const PlaneGeom &g = L.plane->g;
    PcgPlane pg;
    pg.nx = g.nx; pg.ny = g.ny; pg.nz = g.nz; pg.hx = g.hx;
    pg.nr = L.n / 2;
    for (int i = 0; i < 7; ++i) pg.c[i] = g.c[i];
    return pg;
}

// FCG's outer state on level 0, in the level's numbering, in T: V itself, or double around the fp32 cycle of a mixed
// hierarchy.  q = A v is one fused launch on a plane level (pg) and the row kernels over A anywhere else; rlo (nullable):
// where pcg_update and pcg_residual also leave fl32(2^-e r) — the cycle's right-hand side when r itself is not
template <typename T, typename V>
struct Outer {
    T *b, *x, *r, *p, *p2, *q;
    bool plane;
    PcgPlane pg;
    const DevCsrT<T> *A;
    V *rlo;
};

// the hierarchy's own copies of b and x (the cycle overwrites the level's), p, p2, q; r is the cycle's right-hand side itself
template <typename V>
Outer<V, V> plain_outer(Hier<V> *hh) {
    Level<V> &L = hh->lv[0];
    const bool plane = pcg_fused_plane(hh, L);
    return {hh->pcg_b.p, hh->pcg_x.p, L.b.p, hh->pcg_p.p, hh->pcg_p2.p, hh->pcg_q.p, plane, plane ? pcg_plane_of(L) : PcgPlane{}, &L.A, nullptr};
}
// OMG_DTYPE_MIXED (below): the resident fp64 b and x, the operator in double
template <typename V>
Outer<double, V> mixed_outer(Hier<V> *hh) {
    auto &m = hh->mx;
    return {m.b.p, m.x.p, m.r.p, m.p.p, m.p2.p, m.q.p, m.plane, m.pg, &m.A, hh->lv[0].b.p};
}

// q = A v; sc0: the zero scalars (the fused launch with beta = 0 and nothing done; scratch: its p2)
template <typename T, typename V>
void outer_apply(Hier<V> *hh, const Outer<T, V> &w, const T *v, T *q, T *scratch, const double *sc0) {
    if (w.plane) {
        pcg_plane_step<T, T>(w.pg, v, v, scratch, q, hh->pcg_part.p, sc0, hh->stream);
        return;
    }
    RowArgsT<T> a;
    a.x = const_cast<T *>(v);
    a.y = q;
    launch_rows(*w.A, ROW_SPMV, -1, a, hh->stream);
}

// r = b - A x (r nullable); ||r||^2 partials (pcg_wgs<T>(n) of them).  Uses q and p2.  start (a mixed hierarchy): the
// iteration begins here (the scalars are zero) — the exponent of ||b|| from the load becomes both of the scalars'
// exponents (pcg.hip), fl32(2^-e r) goes to the cycle's right-hand side in the same pass, and only a start whose norm is
// far from ||b|| makes pcg_lower write it again.
template <typename T, typename V>
void outer_residual(Hier<V> *hh, const Outer<T, V> &w, T *r, bool start = false) {
    const int64_t n = hh->lv[0].n;
    double *sc = hh->pcg_sc.p;
    if constexpr (!std::is_same<T, V>::value) {
        if (start && w.rlo) {
            OMG_HIP(hipMemcpyAsync(sc + PCG_E_USED, hh->mx.load_sc.p + PCG_E_USED, 2 * sizeof(double), hipMemcpyDeviceToDevice, hh->stream));
            outer_apply(hh, w, w.x, w.q, w.p2, sc + PCG_NSC);
            pcg_residual<T, V>(w.b, w.q, r, w.rlo, n, hh->pcg_part.p, sc, hh->stream);
            pcg_fold_start(hh->pcg_part.p, pcg_wgs<T>(n), sc, hh->stream);
            pcg_lower<T, V>(w.b, w.q, w.rlo, n, sc, hh->stream);
            return;
        }
    }
    outer_apply(hh, w, w.x, w.q, w.p2, sc + PCG_NSC);
    pcg_residual<T, V>(w.b, w.q, r, static_cast<V *>(nullptr), n, hh->pcg_part.p, nullptr, hh->stream);
}

// The iterations from r = b - A x0 (in w.r, and in the cycle's right-hand side) and p = 0, then the true residual of the
// x they leave.  restore: what puts the resident state back before that (a plain hierarchy's cycle has overwritten it).
template <typename T, typename V, typename Restore>
void fcg(Hier<V> *hh, Outer<T, V> w, int pre, int post, int max_iter, double threshold, int *iterations, double *norms, double *true_norm,
         int *breakdown, Restore &&restore) {
    Level<V> &L = hh->lv[0];
    const int64_t n = L.n;
    hipStream_t s = hh->stream;
    double *sc = hh->pcg_sc.p, *sc0 = hh->pcg_sc.p + PCG_NSC, *part = hh->pcg_part.p;
    const int nwg = pcg_wgs<T>(n);
    constexpr int BATCH = 16;
    double hs[PCG_NSC] = {0};
    int k = 0;
    while (k < max_iter) {
        const int cnt = std::min(BATCH, max_iter - k);
        for (int j = 0; j < cnt; ++j, ++k) {
            zero_start_cycle(hh, pre, post);                       // z = M(r), of a mixed hierarchy M(fl32(r)), in L.xp
            const V *Z = L.xp;
            pcg_dots<T, V>(w.r, Z, w.q, n, part, sc, s);
            pcg_fold_beta(part, nwg, sc, k == 0, s);
            int nwg2 = nwg;
            if (w.plane) {
                nwg2 = pcg_plane_step<T, V>(w.pg, Z, w.p, w.p2, w.q, part, sc, s);
            } else {
                pcg_pupdate<T, V>(Z, w.p, w.p2, n, sc, s);
                RowArgsT<T> a;
                a.x = w.p2;
                a.y = w.q;
                launch_rows(*w.A, ROW_SPMV, -1, a, s);
                pcg_dot<T>(w.p2, w.q, n, part, sc, s);
            }
            std::swap(w.p, w.p2);
            pcg_fold_alpha(part, nwg2, sc, s);
            pcg_update<T, V>(w.x, w.p, w.r, w.q, w.rlo, n, part, sc, s);
            pcg_fold_norm(part, nwg, sc, hh->pcg_norms.p, k, threshold, s);
        }
        OMG_HIP(hipMemcpyAsync(hs, sc, sizeof(hs), hipMemcpyDeviceToHost, s));
        OMG_HIP(hipStreamSynchronize(s));
        check_march(hh);
        if (hs[PCG_DONE] != 0.0) break;
    }
    const int iters = int(hs[PCG_ITERS]);
    if (norms && iters > 0) OMG_HIP(hipMemcpyAsync(norms, hh->pcg_norms.p, size_t(iters) * sizeof(double), hipMemcpyDeviceToHost, s));
    restore();
    outer_residual(hh, w, static_cast<T *>(nullptr));              // the true residual once
    pcg_fold_sqrt(part, nwg, sc0 + PCG_ITERS, s);
    double tn = 0.0;
    OMG_HIP(hipMemcpyAsync(&tn, sc0 + PCG_ITERS, sizeof(double), hipMemcpyDeviceToHost, s));
    OMG_HIP(hipStreamSynchronize(s));
    check_march(hh);
    if (iterations) *iterations = iters;
    if (true_norm) *true_norm = tn;
    if (breakdown) *breakdown = hs[PCG_BREAK] != 0.0 ? 1 : 0;
}

template <typename V>
void resident_pcg(Hier<V> *hh, int pre, int post, int max_iter, double threshold, int *iterations, double *norms, double *true_norm,
                  int *breakdown) {
    Level<V> &L = hh->lv[0];
    const int64_t n = L.n;
    hipStream_t s = hh->stream;
    if (hh->pcg_sc.n < size_t(2 * PCG_NSC)) hh->pcg_sc.alloc(2 * PCG_NSC);
    if (hh->pcg_part.n < size_t(2 * PCG_MAX_WG)) hh->pcg_part.alloc(2 * PCG_MAX_WG);
    if (hh->pcg_norms.n < size_t(max_iter)) hh->pcg_norms.alloc(size_t(max_iter));
    if (hh->mixed) {
        // x, r, p, p2, q, b in double and z = M(fl32(r)) in float (OMG_DTYPE_MIXED below): the resident state is FCG's own
        const Outer<double, V> w = mixed_outer(hh);
        OMG_HIP(hipMemsetAsync(hh->pcg_sc.p, 0, 2 * PCG_NSC * sizeof(double), s));
        outer_residual(hh, w, w.r, true);                          // r = b - A x0, fl32(2^-e r) -> L.b
        OMG_HIP(hipMemsetAsync(w.p, 0, size_t(n) * sizeof(double), s));      // (beta = 0 in the first iteration multiplies it)
        fcg(hh, w, pre, post, max_iter, threshold, iterations, norms, true_norm, breakdown, [] {});
        return;
    }
    const size_t vn = size_t(std::max<int64_t>(n, 1));
    for (DevBuf<V> *b : {&hh->pcg_b, &hh->pcg_x, &hh->pcg_p, &hh->pcg_p2, &hh->pcg_q})
        if (b->n < vn) b->alloc(vn);
    const Outer<V, V> w = plain_outer(hh);
    if (!w.plane) ensure_format(hh, 0);
    OMG_HIP(hipMemsetAsync(hh->pcg_sc.p, 0, 2 * PCG_NSC * sizeof(double), s));
    OMG_HIP(hipMemcpyAsync(w.b, L.b.p, size_t(n) * sizeof(V), hipMemcpyDeviceToDevice, s));
    OMG_HIP(hipMemcpyAsync(w.x, L.xp, size_t(n) * sizeof(V), hipMemcpyDeviceToDevice, s));
    OMG_HIP(hipMemsetAsync(w.p, 0, size_t(n) * sizeof(V), s));     // (beta = 0 in the first iteration multiplies it)
    outer_residual(hh, w, w.r);                                    // r = b - A x0
    fcg(hh, w, pre, post, max_iter, threshold, iterations, norms, true_norm, breakdown, [&] {
        // the resident state: x as the iterate, b as the right-hand side
        OMG_HIP(hipMemcpyAsync(L.xp, w.x, size_t(n) * sizeof(V), hipMemcpyDeviceToDevice, s));
        OMG_HIP(hipMemcpyAsync(L.b.p, w.b, size_t(n) * sizeof(V), hipMemcpyDeviceToDevice, s));
    });
}

// ---- OMG_DTYPE_MIXED: fp64 iterations around the fp32 zero-start V-cycle (pcg.hip kernels with Z = float) --------------
// Every iteration crosses the precision boundary once each way: the cycle reads fl32(r) from L.b and leaves z in L.xp
// (float); x, r, p, q, b, the operator and every norm stay double.  Plain cycles are defect correction
// (x += M(fl32(b - A x)), the norm that of b - A x after the correction), PCG is the FCG of resident_pcg.  The fp64 x and
// b are the resident state; L.b is formed again from them at the start of every call.  Neither runs from a hipGraph.

// the seven constants of a plane level 0 (-K, -J, -I, diagonal, +I, +J, +K) in double from the caller's CSR (natural
// numbering: r = (k ny + j) nx + i): for each direction the value at that offset in the row of the first cell that has
// such a neighbour — the plan checked that every row agrees; an absent direction (2-D: K) is 0
void plane_constants(const omg_csr &A, PcgPlane &g) {
    const int64_t nx = g.nx, ny = g.ny, nz = g.nz, sj = nx, sk = nx * ny;
    const int64_t off[7] = {-sk, -sj, -1, 0, 1, sj, sk};
    const int64_t ext[7] = {nz, ny, nx, 1, nx, ny, nz};
    for (int e = 0; e < 7; ++e) {
        g.c[e] = 0.0;
        if (e != 3 && ext[e] < 2) continue;
        const int64_t r = e == 0 ? sk : e == 1 ? sj : e == 2 ? 1 : 0;     // minus directions: the cell one step in
        const int64_t c = r + off[e];
        for (int64_t p = A.indptr[r]; p < A.indptr[r + 1]; ++p)
            if (A.indices[p] == c) g.c[e] = A.data[p];
    }
}

template <typename V>
void build_mixed(Hier<V> *h, const omg_csr &A0) {
    Level<V> &L = h->lv[0];
    auto &m = h->mx;
    OMG_REQUIRE(A0.n_rows == L.n, "internal: the mixed outer operator has the wrong size");
    SetupTimer tm("mixed precision: level 0's fp64 outer operator and vectors");
    m.plane = pcg_fused_plane(h, L);
    if (m.plane) {
        m.pg = pcg_plane_of(L);
        plane_constants(A0, m.pg);
    } else {
        materialise_ordering(L.ord);
        const bool id = L.ord.identity;
        std::vector<int32_t> src;
        HostCsr Ap = renumber_sorted(A0, id ? nullptr : L.ord.perm.data(), id ? nullptr : L.ord.inv.data(), src);
        m.A.upload(Ap, {0, L.n}, h->stream, true);
        m.src.alloc(std::max<size_t>(src.size(), 1));
        m.src.upload(src.data(), src.size(), h->stream);
    }
    const size_t vn = size_t(std::max<int64_t>(L.n, 1));
    for (DevBuf<double> *b : {&m.b, &m.x, &m.r, &m.p, &m.p2, &m.q}) { b->alloc(vn); b->zero(h->stream); }
    if (m.plane) { m.x2.alloc(vn); m.x2.zero(h->stream); }
    m.load_sc.alloc(PCG_NSC);
    m.load_sc.zero(h->stream);
    if (h->pcg_sc.n < size_t(2 * PCG_NSC)) h->pcg_sc.alloc(2 * PCG_NSC);
    if (h->pcg_part.n < size_t(2 * PCG_MAX_WG)) h->pcg_part.alloc(2 * PCG_MAX_WG);
    OMG_HIP(hipStreamSynchronize(h->stream));
    h->mixed = true;
}

// the entries that would hand back an fp32-accurate answer refuse a mixed hierarchy
template <typename V>
void refuse_mixed(const Hier<V> *h, const char *entry) {
    if (h->mixed)
        throw Error(OMG_ERR_UNSUPPORTED, std::string(entry) + ": a mixed-precision hierarchy solves through the resident entries "
                                         "(omg_resident_load[_dev], omg_resident_cycle[s], omg_resident_pcg, omg_resident_fetch[_dev])");
}

// n_cycles defect-correction cycles; the norm of cycle k to out[k] (device)
template <typename V>
void mixed_cycles(Hier<V> *h, int pre, int post, int n_cycles, double *out) {
    auto &m = h->mx;
    Level<V> &L = h->lv[0];
    const int64_t n = L.n;
    hipStream_t s = h->stream;
    double *part = h->pcg_part.p;
    OMG_HIP(hipMemsetAsync(h->pcg_sc.p, 0, 2 * PCG_NSC * sizeof(double), s));
    outer_residual(h, mixed_outer(h), static_cast<double *>(nullptr), true);        // fl32(2^-e (b - A x)) -> L.b
    for (int k = 0; k < n_cycles; ++k) {
        zero_start_cycle(h, pre, post);                            // z = M(fl32(r)) in L.xp
        int nwg;
        if (m.plane) {
            nwg = pcg_defect_plane<double, V>(m.pg, m.x.p, L.xp, m.x2.p, m.b.p, L.b.p, part, h->pcg_sc.p, s);
            std::swap(m.x, m.x2);
        } else {
            pcg_defect_add<double, V>(m.x.p, L.xp, n, h->pcg_sc.p, s);
            RowArgsT<double> a;
            a.x = m.x.p;
            a.y = m.q.p;
            launch_rows(m.A, ROW_SPMV, -1, a, s);
            pcg_residual<double, V>(m.b.p, m.q.p, static_cast<double *>(nullptr), L.b.p, n, part, h->pcg_sc.p, s);
            nwg = pcg_wgs<double>(n);
        }
        pcg_fold_sqrt(part, nwg, out + k, s, h->pcg_sc.p);
    }
}

// omg_resident_load[_dev], omg_solve: the resident right-hand side and iterate (x0 null: zeros) from double arrays in natural
// numbering, on the host or — dev — in HBM; b minus its mean where the hierarchy has the constant null space (the initial
// iterate stays).  A mixed hierarchy's resident state is its fp64 outer b and x, always through the gather kernel.
// Enqueued only: the load entries synchronise.
template <typename V>
void resident_load(Hier<V> *h, const double *b, const double *x0, bool dev) {
    Level<V> &L = h->lv[0];
    h->pj.projected = false;                                       // (the alphas were another right-hand side's)
    auto load = [&](auto *b_dst, auto *x_dst, auto &&put) {
        put(b, b_dst);
        if (has_nullspace(h)) project_vec(h, b_dst, L.n);
        if (x0) put(x0, x_dst);
        else OMG_HIP(hipMemsetAsync(x_dst, 0, size_t(L.n) * sizeof(*x_dst), h->stream));
    };
    if (h->mixed) {
        load(h->mx.b.p, h->mx.x.p, [&](const double *src, double *dst) {
            if (!dev) {
                ensure_nat(h, 0);
                L.nat.upload(src, L.n, h->stream);
                src = L.nat.p;
            }
            launch_gather<double, double>(src, L.ord.identity ? nullptr : L.perm.p, dst, L.n, h->stream);
        });
        // ||b||'s exponent, once per load: what the first residual of every iteration on this b is scaled by (pcg.hip)
        double *sc0 = h->pcg_sc.p + PCG_NSC;
        OMG_HIP(hipMemsetAsync(sc0, 0, PCG_NSC * sizeof(double), h->stream));
        pcg_dot<double>(h->mx.b.p, h->mx.b.p, L.n, h->pcg_part.p, sc0, h->stream);
        pcg_fold_sqrt(h->pcg_part.p, pcg_wgs<double>(L.n), nullptr, h->stream, h->mx.load_sc.p, true);
    } else
        load(L.b.p, L.xp, [&](const double *src, V *dst) { dev ? load_vec_dev(h, 0, src, dst) : load_vec(h, 0, src, dst); });
}

// omg_resident_fetch[_dev], omg_solve: the resident iterate — minus its mean, in place, where the hierarchy has the constant
// null space — to a double array in natural numbering; complete on return
template <typename V>
void resident_fetch(Hier<V> *h, double *x, bool dev) {
    Level<V> &L = h->lv[0];
    auto fetch = [&](auto *src, auto &&get) {
        if (has_nullspace(h)) project_vec(h, src, L.n);
        get(src);
        if (dev) OMG_HIP(hipStreamSynchronize(h->stream));
    };
    if (h->mixed) {
        fetch(h->mx.x.p, [&](const double *src) {
            if (!dev) ensure_nat(h, 0);
            launch_scatter<double, double>(src, L.ord.identity ? nullptr : L.perm.p, dev ? x : L.nat.p, L.n, h->stream);
            if (!dev) download_staged(x, L.nat.p, size_t(L.n) * sizeof(double), h->stream);
        });
        check_march(h);
    } else {
        fetch(L.xp, [&](const V *src) { dev ? fetch_vec_dev<V>(h, 0, src, x) : fetch_vec<V>(h, 0, src, x); });
        if (dev) check_march(h);                                    // (fetch_vec has asked already)
    }
}

// omg_hierarchy_update_fine on a mixed hierarchy, after the fp32 levels: the outer operator's values gathered from the new
// ones through src (its pattern is the caller's operator's, renumbered)
template <typename V>
void mixed_update_values(Hier<V> *h, const double *vals_dev, int64_t nnz) {
    auto &m = h->mx;
    OMG_REQUIRE(!m.plane && m.A.nnz == nnz, "internal: the mixed outer operator does not match the update");
    launch_gather<double, double>(vals_dev, m.src.p, m.A.data.p, nnz, h->stream);
    OMG_HIP(hipStreamSynchronize(h->stream));
}

// ---- omg_resident_cycles: n cycles back to back, the norm of cycle k to out[k] (device) -------------------------------------
template <typename V>
void batched_cycles(Hier<V> *hh, int pre, int post, int n_cycles, double *out) {
    auto &L0 = hh->lv[0];
    const bool single = hh->lv.size() == 1;
    // What a cycle leaves of its norm goes to a slot of nb partials in the batch buffer, and one launch per chunk adds
    // the slots up (the additions of launch_sum_sqrt: the same bits as omg_resident_cycle).  Level 0 decides nb, what
    // a cycle does with its slots, and how many slots of a chunk of cnt that launch adds:
    //  plane (post <= 1): the up pass leaves its workgroup partials in the cycle's slot; cnt
    //  s27: with pre >= 1 the first sweep of cycle j + 1 also squares the residuals with respect to the iterate it starts
    //    from — cycle j's norm (openmg/__init__.py:227) without another pass over the operator; the last cycle of a
    //    chunk (and every cycle when pre = 0) runs the norm kernel; cnt
    //  rows, where can_prenorm() holds: the last set's block partials by the cycle's fused post-smoothing launch, the
    //    first set's by cycle j + 1's first launch; the last cycle of a chunk has no successor in it and takes the
    //    usual norm launch; cnt - 1
    //  anything else (nb = 0): every cycle the usual norm launch — of a single level, whose solve is direct, a zero; none
    enum { PLANE, S27, ROWS } kind = ROWS;
    int64_t nb = 0;
    if (!single && use_plane(hh, L0) && post <= 1) {
        kind = PLANE;
        nb = L0.plane->g.n_wg;
    } else if (!single && use_s27(hh, L0)) {
        kind = S27;
        nb = int64_t(4) * L0.s27->g.n_wg;
    } else if (!single && !use_var7(hh, L0)) {                 // (a var7 cycle never touches the row-kernel format)
        ensure_format(hh, 0);
        // (a plane-pipelined cycle with post > 1 ends set by set: its first launch is no PRENORM launch)
        if (!getenv_flag("OMG_NO_PRENORM") && can_prenorm(hh, L0, pre, post) && !use_plane(hh, L0)) nb = L0.A.n_blocks();
    }
    constexpr int CHUNK = 64;
    if (hh->batch_partials.n < size_t(CHUNK) * size_t(nb)) hh->batch_partials.alloc(size_t(CHUNK) * size_t(nb));
    auto slot = [&](int j) { return hh->batch_partials.p + size_t(j) * size_t(nb); };
    for (int k0 = 0; k0 < n_cycles; k0 += CHUNK) {
        const int cnt = std::min(CHUNK, n_cycles - k0);
        for (int j = 0; j < cnt; ++j) {
            const bool last_of_chunk = j + 1 == cnt;
            if (single) {
                cycle_body(hh, 0, pre, post);
                OMG_HIP(hipMemsetAsync(out + k0 + j, 0, sizeof(double), hh->stream));   // :232
            } else if (kind == PLANE) {
                const int st = cycle_body(hh, 0, pre, post, true, nullptr, false, slot(j));
                OMG_REQUIRE(st == NORM_PASS, "internal: plane-pipelined cycle without its norm partials");
            } else if (kind == S27) {
                const bool own_norm = last_of_chunk || pre == 0;
                cycle_body(hh, 0, pre, post, own_norm, (pre >= 1 && j > 0) ? slot(j - 1) : nullptr, false, own_norm ? slot(j) : nullptr);
                if (own_norm) {
                    Prof<V> p(hh, 0, 4);
                    L0.s27->norm(L0.xp, L0.b.p, L0.s27->have67, slot(j), hh->stream);
                }
            } else {
                const bool defer = nb > 0;
                const int part = cycle_body(hh, 0, pre, post, true, (defer && j > 0) ? slot(j - 1) : nullptr, false,
                                            (defer && !last_of_chunk) ? slot(j) : nullptr);
                if (!defer || last_of_chunk) {
                    finish_norm(hh, 0, part, out + k0 + j);                            // :227
                } else {
                    OMG_REQUIRE(part || hh->smoother == OMG_SMOOTH_JACOBI, "internal: deferred norm without the fused post-smoothing launch");
                }
            }
        }
        const int sums = kind == ROWS ? (nb > 0 ? cnt - 1 : 0) : cnt;
        if (sums > 0) launch_sum_batch(hh->batch_partials.p, nb, nb, sums, out + k0, true, hh->stream);
    }
}

// ---- omg_resident_norms: ||b|| and ||b - A x|| of the resident state without a cycle --------------------------------------
// The launches are FCG's own: (b, b) by pcg_dot, q = A x by the level's SpMV (outer_apply: one fused launch on
// a plane level, the row kernels anywhere else), ||b - q||^2 by pcg_residual with no r to write, each folded by one
// workgroup (pcg_fold_sqrt).  They write q, p2, the partials and norms2 — scratch that every resident entry fills again
// before it reads it — and nothing of b, x, the levels' vectors or their pointer state: a cycle, an FCG run or a replayed
// graph afterwards has the bits it would have had.
template <typename T, typename V>
void outer_norms(Hier<V> *hh, const Outer<T, V> &w, bool rhs, bool residual, double *out) {
    const int64_t n = hh->lv[0].n;
    double *sc0 = hh->pcg_sc.p + PCG_NSC, *part = hh->pcg_part.p;
    const int nwg = pcg_wgs<T>(n);
    if (rhs) {
        pcg_dot<T>(w.b, w.b, n, part, sc0, hh->stream);
        pcg_fold_sqrt(part, nwg, out, hh->stream);
    }
    if (residual) {
        outer_residual(hh, w, static_cast<T *>(nullptr));
        pcg_fold_sqrt(part, nwg, out + 1, hh->stream);
    }
}

// The view the resident entries that only read the state take of level 0 (omg_resident_norms, the projection entries): the
// resident b and x themselves (not FCG's copies), the operator, the zero scalars; apply: the operator will be applied
// (outer_apply), so q and p2 exist as its product and scratch and the row-kernel format where no fused launch does it
template <typename V, typename F>
void with_resident_outer(Hier<V> *hh, bool apply, F &&f) {
    Level<V> &L = hh->lv[0];
    if (hh->pcg_sc.n < size_t(2 * PCG_NSC)) hh->pcg_sc.alloc(2 * PCG_NSC);
    if (hh->pcg_part.n < size_t(2 * PCG_MAX_WG)) hh->pcg_part.alloc(2 * PCG_MAX_WG);
    OMG_HIP(hipMemsetAsync(hh->pcg_sc.p + PCG_NSC, 0, PCG_NSC * sizeof(double), hh->stream));   // (beta = 0, nothing done)
    if (hh->mixed) {
        Outer<double, V> w = mixed_outer(hh);
        w.rlo = nullptr;                                           // (the cycle's right-hand side stays as it is)
        f(w);
        return;
    }
    if (apply) {
        OMG_REQUIRE(hh->lv.size() > 1, "omg_resident_norms: a single-level hierarchy has no smoothed operator to form a residual with");
        const size_t vn = size_t(std::max<int64_t>(L.n, 1));
        for (DevBuf<V> *b : {&hh->pcg_p2, &hh->pcg_q})
            if (b->n < vn) b->alloc(vn);
    }
    Outer<V, V> w = plain_outer(hh);
    w.b = L.b.p;
    w.x = L.xp;
    if (apply && !w.plane) ensure_format(hh, 0);
    f(w);
}

template <typename V>
void resident_norms(Hier<V> *hh, double *rhs_norm, double *residual_norm) {
    hipStream_t s = hh->stream;
    if (hh->norms2.n < 2) hh->norms2.alloc(2);
    double *out = hh->norms2.p;
    with_resident_outer(hh, residual_norm != nullptr, [&](auto &w) { outer_norms(hh, w, rhs_norm != nullptr, residual_norm != nullptr, out); });
    double host[2] = {0.0, 0.0};
    OMG_HIP(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, s));
    OMG_HIP(hipStreamSynchronize(s));
    if (rhs_norm) *rhs_norm = host[0];
    if (residual_norm) *residual_norm = host[1];
}

// ---- omg_resident_projection / _project / _project_update: Fischer's projection onto earlier solutions (project.hip) --------
// The set X_0 ... X_{l-1} is A-orthonormal for level 0's operator as omg_resident_norms applies it (outer_apply on the
// Outer view: the fp64 outer operator of a mixed hierarchy), in that view's type T and the level's numbering.  Everything
// is enqueued on the hierarchy's stream; the alphas, betas and s2 stay on the device and the keep-or-drop decision is taken
// there (project_keep_scale); update reads one status word back.  w = A d goes to the view's q (p2 the plane launch's
// scratch): vectors every resident entry fills again before it reads them.
template <typename V>
void projection_clear(Hier<V> *hh) {
    hh->pj.size = 0;
    hh->pj.projected = false;
}

template <typename V>
void projection_alloc(Hier<V> *hh, int capacity) {
    auto &P = hh->pj;
    OMG_REQUIRE(capacity >= 0 && capacity <= PROJECTION_MAX, "omg_resident_projection: the capacity must lie in 0 .. 64");
    OMG_HIP(hipStreamSynchronize(hh->stream));
    projection_clear(hh);
    if (capacity == P.cap) return;                                 // (the same room: emptied, nothing allocated anew)
    P.vecs.release();
    P.cap = 0;
    if (capacity == 0) return;
    OMG_REQUIRE(hh->lv.size() > 1, "omg_resident_projection: a single-level hierarchy solves directly: nothing to start from");
    const size_t elem = hh->mixed ? sizeof(double) : sizeof(V);
    // (a multiple of 16 bytes apart, so that every vector takes the 16-byte accesses)
    P.stride = (std::max<int64_t>(hh->lv[0].n, 1) + 15) & ~int64_t(15);
    P.vecs.alloc(size_t(capacity + 1) * size_t(P.stride) * elem);      // (out of memory: the hierarchy stays as it was, without a set)
    P.vecs.zero(hh->stream);
    if (P.sc.n < size_t(PJ_NSC)) P.sc.alloc(PJ_NSC);
    if (P.part.n < PROJECTION_PARTIALS) P.part.alloc(PROJECTION_PARTIALS);
    if (P.status.n < 2) P.status.alloc(2);
    P.sc.zero(hh->stream);
    OMG_HIP(hipStreamSynchronize(hh->stream));
    P.cap = capacity;
}

// x <- sum_i (X_i, b) X_i; an empty set launches nothing (x stays what the load made it)
template <typename V>
void projection_project(Hier<V> *hh, int *used) {
    auto &P = hh->pj;
    OMG_REQUIRE(P.cap > 0, "omg_resident_project: the hierarchy has no set (omg_resident_projection)");
    const int l = P.size;
    if (l > 0)
        with_resident_outer(hh, true, [&](auto &w) {
            using T = typename std::remove_pointer<decltype(w.x)>::type;
            const T *X = reinterpret_cast<const T *>(P.vecs.p);
            const int64_t n = hh->lv[0].n;
            project_dots<T>(X, P.stride, l, w.b, n, P.part.p, P.sc.p + PJ_ALPHA, hh->stream);
            project_lincomb<T>(nullptr, X, P.stride, l, P.sc.p + PJ_ALPHA, false, w.x, n, hh->stream);
        });
    P.projected = true;
    if (used) *used = l;
}

template <typename V>
void projection_update(Hier<V> *hh, int *size, int *kept) {
    auto &P = hh->pj;
    OMG_REQUIRE(P.cap > 0, "omg_resident_project_update: the hierarchy has no set (omg_resident_projection)");
    OMG_REQUIRE(P.projected, "omg_resident_project_update: omg_resident_project has not run on this right-hand side");
    int32_t status[2] = {0, 0};
    with_resident_outer(hh, true, [&](auto &w) {
        using T = typename std::remove_pointer<decltype(w.x)>::type;
        T *X = reinterpret_cast<T *>(P.vecs.p);
        const int64_t n = hh->lv[0].n;
        hipStream_t s = hh->stream;
        double *sc = P.sc.p, *sc0 = hh->pcg_sc.p + PCG_NSC;
        int l = P.size;                                            // (P.size itself changes with the status word alone)
        if (l == P.cap) {
            l = 0;                                                 // Fischer's restart: the whole solution is the first vector
            OMG_HIP(hipMemcpyAsync(X, w.x, size_t(n) * sizeof(T), hipMemcpyDeviceToDevice, s));
        } else {
            project_lincomb<T>(w.x, X, P.stride, l, sc + PJ_ALPHA, true, X + int64_t(l) * P.stride, n, s);
        }
        T *d = X + int64_t(l) * P.stride;
        if (has_nullspace(hh)) project_vec(hh, d, n);
        outer_apply(hh, w, d, w.q, w.p2, sc0);                     // w = A d
        project_dots<T>(X, P.stride, l + 1, w.q, n, P.part.p, sc + PJ_BETA, s);      // beta_i, and e0 = (d, w) behind them
        if (l > 0) project_lincomb<T>(d, X, P.stride, l, sc + PJ_BETA, true, d, n, s);
        outer_apply(hh, w, d, w.q, w.p2, sc0);                     // the operator once more: no e0 - sum beta^2
        project_dots<T>(d, P.stride, 1, w.q, n, P.part.p, sc + PJ_S2, s);
        project_keep_scale<T>(d, n, sc + PJ_S2, sc + PJ_BETA + l, l, P.status.p, s);
        OMG_HIP(hipMemcpyAsync(status, P.status.p, sizeof(status), hipMemcpyDeviceToHost, s));
        OMG_HIP(hipStreamSynchronize(s));
    });
    check_march(hh);
    P.size = int(status[0]);
    P.projected = false;
    if (size) *size = P.size;
    if (kept) *kept = int(status[1]);
}

// vector `index` of the set in the caller's numbering, on the host
template <typename V>
void projection_fetch(Hier<V> *hh, int index, double *v) {
    auto &P = hh->pj;
    Level<V> &L = hh->lv[0];
    OMG_REQUIRE(v && index >= 0 && index < P.size, "omg_resident_projection_fetch: no such vector / v is null");
    if (hh->mixed) {
        const double *src = reinterpret_cast<const double *>(P.vecs.p) + int64_t(index) * P.stride;
        ensure_nat(hh, 0);
        launch_scatter<double, double>(src, L.ord.identity ? nullptr : L.perm.p, L.nat.p, L.n, hh->stream);
        download_staged(v, L.nat.p, size_t(L.n) * sizeof(double), hh->stream);
    } else {
        fetch_vec<V>(hh, 0, reinterpret_cast<const V *>(P.vecs.p) + int64_t(index) * P.stride, v);
    }
}

// omg_resident_projection_time: `reps` launches each of the set's inner products with the resident b (the l + 1 vectors of
// omg_resident_project: kernel and fold), of the linear combination behind them (written to the scratch vector q) and of
// pcg.hip's single inner product (b, q) on the same n, each bracketed by hipEvents on the hierarchy's stream after one
// warm-up launch.  The alphas it leaves are those omg_resident_project would leave.
template <typename V>
void projection_time(Hier<V> *hh, int reps, double *dots_ms, double *dot_ms, double *lincomb_ms) {
    auto &P = hh->pj;
    OMG_REQUIRE(P.cap > 0 && P.size > 0 && reps > 0, "omg_resident_projection_time: needs a set that holds a vector / reps > 0");
    hipStream_t s = hh->stream;
    hipEvent_t e0, e1;
    OMG_HIP(hipEventCreate(&e0));
    OMG_HIP(hipEventCreate(&e1));
    auto timed = [&](auto &&once) {
        once();
        OMG_HIP(hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) once();
        OMG_HIP(hipEventRecord(e1, s));
        OMG_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        OMG_HIP(hipEventElapsedTime(&ms, e0, e1));
        return double(ms) / reps;
    };
    try {
        with_resident_outer(hh, true, [&](auto &w) {
            using T = typename std::remove_pointer<decltype(w.x)>::type;
            const T *X = reinterpret_cast<const T *>(P.vecs.p);
            const int64_t n = hh->lv[0].n;
            const double d = timed([&] { project_dots<T>(X, P.stride, P.size, w.b, n, P.part.p, P.sc.p + PJ_ALPHA, s); });
            const double c = timed([&] { project_lincomb<T>(nullptr, X, P.stride, P.size, P.sc.p + PJ_ALPHA, false, w.q, n, s); });
            const double o = timed([&] { pcg_dot<T>(w.b, w.q, n, hh->pcg_part.p, hh->pcg_sc.p + PCG_NSC, s); });
            if (dots_ms) *dots_ms = d;
            if (lincomb_ms) *lincomb_ms = c;
            if (dot_ms) *dot_ms = o;
        });
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

// What every creating entry does around its own builder: the options are checked — before the builder, which asks for the
// device —, the handle made, build(V(), handle) run in the options' precision, a mixed hierarchy given its fp64 outer
// operator from *fine (read after the builder: it may be the builder that fills it in), the handle handed out.
template <typename Build>
void create_handle(const omg_hierarchy_options *opt, omg_hierarchy **out, const omg_csr *fine, Build &&build) {
    OMG_REQUIRE(out, "out is null");
    *out = nullptr;
    OMG_REQUIRE(opt, "options are null");
    const int dtype = opt->dtype;
    OMG_REQUIRE(dtype == OMG_DTYPE_F64 || dtype == OMG_DTYPE_F32 || dtype == OMG_DTYPE_MIXED, "unknown dtype");
    OMG_REQUIRE(opt->nullspace == OMG_NULLSPACE_NONE || opt->nullspace == OMG_NULLSPACE_CONSTANT, "unknown nullspace kind");
    std::unique_ptr<omg_hierarchy> h(new omg_hierarchy);
    if (dtype != OMG_DTYPE_F64) h->f = build(float(), *h);
    else h->d = build(double(), *h);
    if (dtype == OMG_DTYPE_MIXED) build_mixed(h->f.get(), *fine);
    *out = h.release();
}

}  // namespace
}  // namespace omg

using namespace omg;

extern "C" {

const char *omg_last_error(void) { return g_last_error.c_str(); }
const char *omg_version(void) { return "openmg_hip 0.2 (gfx950; f64, f32, mixed)"; }

int omg_device_count(int *count) {
    return guarded([&] {
        OMG_REQUIRE(count, "count is null");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = (e == hipSuccess) ? n : 0;
    });
}

int omg_set_device(int device) {
    return guarded([&] { require_device(); OMG_HIP(hipSetDevice(device)); });
}

int omg_device_mem_info(int64_t *free_bytes, int64_t *total_bytes) {
    return guarded([&] {
        OMG_REQUIRE(free_bytes && total_bytes, "null argument");
        require_device();
        size_t f = 0, t = 0;
        OMG_HIP(hipMemGetInfo(&f, &t));
        *free_bytes = int64_t(f);
        *total_bytes = int64_t(t);
    });
}

int omg_device_synchronize(void) {
    return guarded([&] { require_device(); OMG_HIP(hipDeviceSynchronize()); });
}

int omg_hierarchy_create_opt(int n_levels, const omg_csr *A, const omg_csr *R, const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return guarded([&] {
        create_handle(opt, out, A, [&](auto v, omg_hierarchy &) {
            return create<decltype(v)>(n_levels, A, R, opt->smoother, opt->omega, opt->nullspace);
        });
    });
}

int omg_hierarchy_create_ex(int n_levels, const omg_csr *A, const omg_csr *R, int smoother,
                            double omega, int dtype, omg_hierarchy **out) {
    const omg_hierarchy_options opt = {smoother, omega, dtype, OMG_NULLSPACE_NONE};
    return omg_hierarchy_create_opt(n_levels, A, R, &opt, out);
}

int omg_hierarchy_create(int n_levels, const omg_csr *A, const omg_csr *R, int smoother,
                         double omega, omg_hierarchy **out) {
    return omg_hierarchy_create_ex(n_levels, A, R, smoother, omega, OMG_DTYPE_F64, out);
}

int omg_hierarchy_create_from_fine_opt(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions,
                                       const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return guarded([&] {
        OMG_REQUIRE(out && A_in, "null argument");
        create_handle(opt, out, A_in, [&](auto v, omg_hierarchy &) {
            return create_from_fine<decltype(v)>(*A_in, dim, shape, n_restrictions, opt->smoother, opt->omega, opt->nullspace);
        });
    });
}

int omg_hierarchy_create_from_fine(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, int smoother, double omega,
                                   int dtype, omg_hierarchy **out) {
    const omg_hierarchy_options opt = {smoother, omega, dtype, OMG_NULLSPACE_NONE};
    return omg_hierarchy_create_from_fine_opt(A_in, dim, shape, n_restrictions, &opt, out);
}

int omg_hierarchy_create_from_fine_semi(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, const int *factors,
                                        int64_t min_size, const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return omg_hierarchy_create_from_fine_ragged(A_in, dim, shape, n_restrictions, factors, min_size, OMG_ODD_REFUSE, opt, out);
}

int omg_hierarchy_create_from_fine_ragged(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, const int *factors,
                                          int64_t min_size, int odd, const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return guarded([&] {
        OMG_REQUIRE(out && A_in, "null argument");
        *out = nullptr;
        // (between the options' presence and their contents, where this entry has always checked it)
        OMG_REQUIRE(!opt || odd == OMG_ODD_REFUSE || odd == OMG_ODD_MERGE, "odd must be OMG_ODD_REFUSE or OMG_ODD_MERGE");
        create_handle(opt, out, A_in, [&](auto v, omg_hierarchy &h) {
            h.semi_dim = dim;
            return create_from_fine_semi<decltype(v)>(*A_in, dim, shape, n_restrictions, factors, min_size, odd, opt->smoother, opt->omega,
                                                      opt->nullspace, h.semi_factors);
        });
    });
}

int omg_hierarchy_coarsening(const omg_hierarchy *h, int level, int *factors3) {
    return guarded([&] {
        OMG_REQUIRE(h && (h->d || h->f) && factors3, "null argument");
        OMG_REQUIRE(h->semi_dim > 0, "omg_hierarchy_coarsening: the hierarchy was not made by omg_hierarchy_create_from_fine_semi (the restrictions "
                                     "of every other hierarchy are the caller's, or the full 2^dim aggregation)");
        OMG_REQUIRE(level >= 0 && size_t(level + 1) * size_t(h->semi_dim) <= h->semi_factors.size(), "omg_hierarchy_coarsening: no such restriction");
        for (int d = 0; d < 3; ++d) factors3[d] = d < h->semi_dim ? h->semi_factors[size_t(level) * size_t(h->semi_dim) + d] : 1;
    });
}

int omg_hierarchy_nullspace(const omg_hierarchy *h, int *kind) {
    return guarded([&] {
        OMG_REQUIRE(kind, "null argument");
        with(h, [&](auto *hh) { *kind = hh->coarse.nullspace; });
    });
}

int omg_hierarchy_update_fine(omg_hierarchy *h, const double *data, int64_t nnz, int on_device) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            projection_clear(hh);                                  // (the set is A-orthonormal for the old operator only)
            if (!hh->mixed) {
                update_fine(hh, data, nnz, on_device != 0);
                return;
            }
            // (the new values once in HBM for both the fp32 levels and the fp64 outer operator)
            DevBuf<double> up;
            const double *dev = data;
            if (!on_device && data && nnz > 0) {
                up.alloc(size_t(nnz));
                OMG_HIP(hipMemcpyAsync(up.p, data, size_t(nnz) * sizeof(double), hipMemcpyHostToDevice, hh->stream));
                dev = up.p;
            }
            update_fine(hh, dev, nnz, true);
            mixed_update_values(hh, dev, nnz);
        });
    });
}

// (the three entries without widths are the *_spaced ones with hz = hy = hx = NULL)
int omg_kappa_assemble(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *sigma, int sigma_kind,
                       int sigma_on_device, const double *scale, int32_t *indptr, int32_t *indices, double *data, int out_on_device) {
    return omg_kappa_assemble_spaced(shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, nullptr, nullptr, nullptr,
                                     indptr, indices, data, out_on_device);
}

int omg_kappa_assemble_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *sigma,
                              int sigma_kind, int sigma_on_device, const double *scale, const double *hz, const double *hy, const double *hx,
                              int32_t *indptr, int32_t *indices, double *data, int out_on_device) {
    return guarded([&] {
        OMG_REQUIRE(data, "omg_kappa_assemble: data is null");
        OMG_REQUIRE(!indptr == !indices, "omg_kappa_assemble: indptr and indices are given together or not at all");
        OneShot one;
        KappaField F;
        F.prepare({shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, hz, hy, hx}, one.s);
        // (host outputs: assembled into staging arrays in HBM, fetched once the values are known to be good)
        const size_t n = size_t(F.rows()), nnz = size_t(F.nnz());
        DevBuf<double> dv;
        DevBuf<int32_t> dp, di;
        if (!out_on_device) {
            dv.alloc(nnz);
            if (indptr) { dp.alloc(n + 1); di.alloc(nnz); }
        }
        F.assemble(out_on_device ? indptr : dp.p, out_on_device ? indices : di.p, out_on_device ? data : dv.p, one.s, "omg_kappa_assemble");
        if (!out_on_device) {
            if (indptr) {
                download_staged(indptr, dp.p, (n + 1) * sizeof(int32_t), one.s);
                download_staged(indices, di.p, nnz * sizeof(int32_t), one.s);
            }
            download_staged(data, dv.p, nnz * sizeof(double), one.s);
        }
        OMG_HIP(hipStreamSynchronize(one.s));
    });
}

int omg_kappa_rhs(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale, const double *f,
                  int f_kind, int f_on_device, const int *value_kinds, const double *value_scalars, const double *const *value_fields,
                  int values_on_device, double *b, int b_on_device) {
    return omg_kappa_rhs_spaced(shape, kappa, kappa_on_device, walls, scale, nullptr, nullptr, nullptr, f, f_kind, f_on_device, value_kinds,
                                value_scalars, value_fields, values_on_device, b, b_on_device);
}

int omg_kappa_rhs_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                         const double *hz, const double *hy, const double *hx, const double *f, int f_kind, int f_on_device,
                         const int *value_kinds, const double *value_scalars, const double *const *value_fields, int values_on_device,
                         double *b, int b_on_device) {
    return guarded([&] {
        require_device();
        kappa_rhs({shape, kappa, kappa_on_device, walls, scale, hz, hy, hx, f, f_kind, f_on_device, value_kinds, value_scalars, value_fields,
                   values_on_device, b, b_on_device});
    });
}

int omg_kappa_flux(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale, const double *u,
                   int u_on_device, const int *value_kinds, const double *value_scalars, const double *const *value_fields,
                   int values_on_device, const double *alpha, double *fz, double *fy, double *fx, int out_on_device) {
    return omg_kappa_flux_spaced(shape, kappa, kappa_on_device, walls, scale, nullptr, nullptr, nullptr, u, u_on_device, value_kinds,
                                 value_scalars, value_fields, values_on_device, alpha, fz, fy, fx, out_on_device);
}

int omg_kappa_flux_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                          const double *hz, const double *hy, const double *hx, const double *u, int u_on_device, const int *value_kinds,
                          const double *value_scalars, const double *const *value_fields, int values_on_device, const double *alpha,
                          double *fz, double *fy, double *fx, int out_on_device) {
    return guarded([&] {
        require_device();
        kappa_flux({shape, kappa, kappa_on_device, walls, scale, hz, hy, hx, u, u_on_device, value_kinds, value_scalars, value_fields,
                    values_on_device, alpha, fz, fy, fx, out_on_device});
    });
}

int omg_face_divergence(const int64_t *shape, const double *fz, const double *fy, const double *fx, int faces_on_device, double *out,
                        int out_on_device) {
    return guarded([&] {
        require_device();
        face_divergence(shape, fz, fy, fx, faces_on_device, out, out_on_device);
    });
}

int omg_hierarchy_create_from_kappa(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *sigma,
                                    int sigma_kind, int sigma_on_device, const double *scale, int n_restrictions,
                                    const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return omg_hierarchy_create_from_kappa_spaced(shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, nullptr,
                                                  nullptr, nullptr, n_restrictions, opt, out);
}

int omg_hierarchy_create_from_kappa_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                                           const double *sigma, int sigma_kind, int sigma_on_device, const double *scale, const double *hz,
                                           const double *hy, const double *hx, int n_restrictions, const omg_hierarchy_options *opt,
                                           omg_hierarchy **out) {
    return guarded([&] {
        HostCsr hostA0;
        omg_csr fine = {};
        create_handle(opt, out, &fine, [&](auto v, omg_hierarchy &) {
            // level 0 in HBM: the pattern and the values, on a stream of this call's own (the hierarchy's does not exist yet)
            DevCsrPlain A0;
            {
                OneShot one;
                KappaField F;
                F.prepare({shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, hz, hy, hx}, one.s);
                SetupTimer tm("device setup: the fine operator from kappa");
                F.assemble(A0, one.s, "omg_hierarchy_create_from_kappa");
                // (the fp64 outer operator of a mixed hierarchy is coded by the host: the one download of this route besides the
                // fall-back of create_from_fine, which fetches the whole chain when a level does not qualify)
                if (opt->dtype == OMG_DTYPE_MIXED) {
                    hostA0 = download_csr(A0, one.s);
                    fine = view(hostA0);
                }
            }
            return create_from_fine<decltype(v)>(omg_csr(), 3, shape, n_restrictions, opt->smoother, opt->omega, opt->nullspace, &A0);
        });
    });
}

int omg_hierarchy_update_kappa(omg_hierarchy *h, const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                               const double *sigma, int sigma_kind, int sigma_on_device, const double *scale) {
    return omg_hierarchy_update_kappa_spaced(h, shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, nullptr, nullptr,
                                             nullptr);
}

int omg_hierarchy_update_kappa_spaced(omg_hierarchy *h, const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                                      const double *sigma, int sigma_kind, int sigma_on_device, const double *scale, const double *hz,
                                      const double *hy, const double *hx) {
    return guarded([&] {
        const double *vals = nullptr;
        int64_t nnz = 0;
        with(h, [&](auto *hh) {
            OMG_REQUIRE(shape, "omg_hierarchy_update_kappa: shape is null");
            OMG_REQUIRE(hh->upd7 && shape[0] == hh->g7[2] && shape[1] == hh->g7[1] && shape[2] == hh->g7[0],
                        "omg_hierarchy_update_kappa: needs a hierarchy that omg_hierarchy_update_fine takes (omg_hierarchy_can_update_fine) "
                        "whose level 0 is the 7-point operator on the grid `shape`");
            KappaField F;
            F.prepare({shape, kappa, kappa_on_device, walls, sigma, sigma_kind, sigma_on_device, scale, hz, hy, hx}, hh->stream);
            // (a hierarchy this entry takes has the in-grid pattern on level 0: no fused path holds a wrap-around row)
            OMG_REQUIRE(!F.any_periodic(), "omg_hierarchy_update_kappa: the hierarchy's fine operator has the in-grid pattern, the walls name a periodic axis");
            nnz = F.nnz();
            OMG_REQUIRE(nnz == hh->nnz0, "internal: the fine pattern is not the in-grid 7-point pattern");
            if (hh->kappa_vals.n != size_t(nnz)) hh->kappa_vals.alloc(size_t(nnz));
            F.values(hh->kappa_vals.p, hh->stream, "omg_hierarchy_update_kappa");
            vals = hh->kappa_vals.p;
        });
        // (the one update path: the values are in HBM)
        const int rc = omg_hierarchy_update_fine(h, vals, nnz, 1);
        if (rc != OMG_OK) throw Error(rc, g_last_error);
    });
}

// ---- the same from one coefficient per face (FaceField, kappa.hip): the kappa entries' sequences with the other assembly
int omg_faces_assemble(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                       const double *sigma, int sigma_kind, int sigma_on_device, int32_t *indptr, int32_t *indices, double *data,
                       int out_on_device) {
    return guarded([&] {
        OMG_REQUIRE(data, "omg_faces_assemble: data is null");
        OMG_REQUIRE(!indptr == !indices, "omg_faces_assemble: indptr and indices are given together or not at all");
        OneShot one;
        FaceField F;
        F.prepare({shape, cz, cy, cx, faces_on_device, walls, sigma, sigma_kind, sigma_on_device}, one.s);
        const size_t n = size_t(F.rows()), nnz = size_t(F.nnz());
        DevBuf<double> dv;
        DevBuf<int32_t> dp, di;
        if (!out_on_device) {
            dv.alloc(nnz);
            if (indptr) { dp.alloc(n + 1); di.alloc(nnz); }
        }
        F.assemble(out_on_device ? indptr : dp.p, out_on_device ? indices : di.p, out_on_device ? data : dv.p, one.s, "omg_faces_assemble");
        if (!out_on_device) {
            if (indptr) {
                download_staged(indptr, dp.p, (n + 1) * sizeof(int32_t), one.s);
                download_staged(indices, di.p, nnz * sizeof(int32_t), one.s);
            }
            download_staged(data, dv.p, nnz * sizeof(double), one.s);
        }
        OMG_HIP(hipStreamSynchronize(one.s));
    });
}

int omg_faces_rhs(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                  const double *f, int f_kind, int f_on_device, const int *value_kinds, const double *value_scalars,
                  const double *const *value_fields, int values_on_device, double *b, int b_on_device) {
    return guarded([&] {
        require_device();
        faces_rhs({shape, cz, cy, cx, faces_on_device, walls, f, f_kind, f_on_device, value_kinds, value_scalars, value_fields, values_on_device, b,
                   b_on_device});
    });
}

int omg_faces_flux(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                   const double *u, int u_on_device, const int *value_kinds, const double *value_scalars, const double *const *value_fields,
                   int values_on_device, const double *alpha, double *fz, double *fy, double *fx, int out_on_device) {
    return guarded([&] {
        require_device();
        faces_flux({shape, cz, cy, cx, faces_on_device, walls, u, u_on_device, value_kinds, value_scalars, value_fields, values_on_device, alpha, fz,
                    fy, fx, out_on_device});
    });
}

int omg_hierarchy_create_from_faces(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device,
                                    const int *walls, const double *sigma, int sigma_kind, int sigma_on_device, int n_restrictions,
                                    const omg_hierarchy_options *opt, omg_hierarchy **out) {
    return guarded([&] {
        HostCsr hostA0;
        omg_csr fine = {};
        create_handle(opt, out, &fine, [&](auto v, omg_hierarchy &) {
            DevCsrPlain A0;
            {
                OneShot one;
                FaceField F;
                F.prepare({shape, cz, cy, cx, faces_on_device, walls, sigma, sigma_kind, sigma_on_device}, one.s);
                SetupTimer tm("device setup: the fine operator from face coefficients");
                F.assemble(A0, one.s, "omg_hierarchy_create_from_faces");
                // (the fp64 outer operator of a mixed hierarchy is coded by the host, as in omg_hierarchy_create_from_kappa)
                if (opt->dtype == OMG_DTYPE_MIXED) {
                    hostA0 = download_csr(A0, one.s);
                    fine = view(hostA0);
                }
            }
            return create_from_fine<decltype(v)>(omg_csr(), 3, shape, n_restrictions, opt->smoother, opt->omega, opt->nullspace, &A0);
        });
    });
}

int omg_hierarchy_update_faces(omg_hierarchy *h, const int64_t *shape, const double *cz, const double *cy, const double *cx,
                               int faces_on_device, const int *walls, const double *sigma, int sigma_kind, int sigma_on_device) {
    return guarded([&] {
        const double *vals = nullptr;
        int64_t nnz = 0;
        with(h, [&](auto *hh) {
            OMG_REQUIRE(shape, "omg_hierarchy_update_faces: shape is null");
            OMG_REQUIRE(hh->upd7 && shape[0] == hh->g7[2] && shape[1] == hh->g7[1] && shape[2] == hh->g7[0],
                        "omg_hierarchy_update_faces: needs a hierarchy that omg_hierarchy_update_fine takes (omg_hierarchy_can_update_fine) "
                        "whose level 0 is the 7-point operator on the grid `shape`");
            FaceField F;
            F.prepare({shape, cz, cy, cx, faces_on_device, walls, sigma, sigma_kind, sigma_on_device}, hh->stream);
            OMG_REQUIRE(!F.any_periodic(), "omg_hierarchy_update_faces: the hierarchy's fine operator has the in-grid pattern, the walls name a periodic axis");
            nnz = F.nnz();
            OMG_REQUIRE(nnz == hh->nnz0, "internal: the fine pattern is not the in-grid 7-point pattern");
            if (hh->kappa_vals.n != size_t(nnz)) hh->kappa_vals.alloc(size_t(nnz));
            F.values(hh->kappa_vals.p, hh->stream, "omg_hierarchy_update_faces");
            vals = hh->kappa_vals.p;
        });
        // (the one update path: the values are in HBM)
        const int rc = omg_hierarchy_update_fine(h, vals, nnz, 1);
        if (rc != OMG_OK) throw Error(rc, g_last_error);
    });
}

int omg_hierarchy_can_update_fine(const omg_hierarchy *h, int *yes) {
    return guarded([&] {
        OMG_REQUIRE(yes, "null argument");
        with(h, [&](auto *hh) { *yes = (hh->upd7 || hh->indptr0.p) ? 1 : 0; });      // (update_fine's own test)
    });
}

int omg_hierarchy_dtype(const omg_hierarchy *h, int *dtype) {
    return guarded([&] {
        OMG_REQUIRE(h && dtype, "null argument");
        *dtype = h->f ? (h->f->mixed ? OMG_DTYPE_MIXED : OMG_DTYPE_F32) : OMG_DTYPE_F64;
    });
}

int omg_hierarchy_destroy(omg_hierarchy *h) {
    return guarded([&] {
        if (!h) return;
        if (h->d || h->f) with(h, [&](auto *hh) { (void)hipStreamSynchronize(hh->stream); });
        delete h;
    });
}

int omg_hierarchy_set_stream(omg_hierarchy *h, void *hip_stream) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            OMG_HIP(hipStreamSynchronize(hh->stream));
            drop_graph(hh);
            hh->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : hh->own;
        });
    });
}

int omg_hierarchy_sync(omg_hierarchy *h) {
    return guarded([&] { with(h, [&](auto *hh) { OMG_HIP(hipStreamSynchronize(hh->stream)); }); });
}

int omg_hierarchy_level_rows(const omg_hierarchy *h, int level, int64_t *n_rows) {
    return guarded([&] {
        with(h, [&](auto *hh) { check_level(hh, level); OMG_REQUIRE(n_rows, "null"); *n_rows = hh->lv[level].n; });
    });
}

int omg_hierarchy_level_sets(const omg_hierarchy *h, int level, int64_t *n_sets) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            OMG_REQUIRE(n_sets, "null");
            *n_sets = (int64_t)hh->lv[level].ord.sets.size() - 1;      // (of the ordering: the format may not be built yet)
        });
    });
}

int omg_hierarchy_level_fused(const omg_hierarchy *h, int level, int *fused) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            OMG_REQUIRE(fused, "null");
            ensure_format(hh, level);
            *fused = (level + 1 < (int)hh->lv.size() && can_fuse(hh, hh->lv[level])) ? 1 : 0;
        });
    });
}

int omg_hierarchy_level_flags(const omg_hierarchy *h, int level, int *flags) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            OMG_REQUIRE(flags, "null");
            ensure_format(hh, level);
            const bool smoothed = level + 1 < (int)hh->lv.size();
            *flags = ((smoothed && can_fuse(hh, hh->lv[level])) ? OMG_LEVEL_FUSED_LAST_SET : 0) |
                     ((smoothed && hh->lv[level].scatter_prolong) ? OMG_LEVEL_SCATTER_PROLONG : 0) |
                     ((smoothed && hh->lv[level].A.all_union()) ? OMG_LEVEL_UNION_WALK : 0) |
                     ((smoothed && hh->lv[level].march) ? OMG_LEVEL_MARCH : 0) |
                     ((smoothed && hh->lv[level].march && hh->lv[level].march->line_scan) ? OMG_LEVEL_MARCH_SCAN : 0) |
                     ((smoothed && hh->lv[level].plane && !hh->no_plane) ? OMG_LEVEL_PLANE : 0) |
                     ((smoothed && hh->lv[level].s27 && !hh->no_plane) ? OMG_LEVEL_STENCIL27 : 0) |
                     ((smoothed && hh->lv[level].var7 && !hh->no_plane) ? OMG_LEVEL_VAR7 : 0) |
                     ((smoothed && hh->lv[level].line) ? OMG_LEVEL_LINE : 0) |
                     ((tail_fuse_depth(hh, level, 1, hh->cycle_shape) || tail_fuse_depth(hh, level - 1, 1, hh->cycle_shape) == 2)
                          ? OMG_LEVEL_TAIL_FUSED : 0);
        });
    });
}

int omg_hierarchy_line_axis(const omg_hierarchy *h, int *axis, int *dim) {
    return guarded([&] {
        OMG_REQUIRE(axis && dim, "null argument");
        with(h, [&](auto *hh) { *axis = hh->line_axis; *dim = hh->line_dim; });
    });
}

int omg_hierarchy_use_plane(omg_hierarchy *h, int enable) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            OMG_HIP(hipStreamSynchronize(hh->stream));
            drop_graph(hh);
            hh->no_plane = enable == 0;
        });
    });
}

int omg_hierarchy_set_cycle(omg_hierarchy *h, int shape, double over_correction) {
    return guarded([&] {
        OMG_REQUIRE(shape == OMG_CYCLE_V || shape == OMG_CYCLE_F || shape == OMG_CYCLE_W, "unknown cycle shape");
        OMG_REQUIRE(std::isfinite(over_correction) && over_correction > 0.0, "the over-correction factor must be finite and positive");
        with(h, [&](auto *hh) {
            if (hh->cycle_shape == shape && hh->over == over_correction) return;
            OMG_HIP(hipStreamSynchronize(hh->stream));
            drop_graph(hh);                                        // (a captured cycle has the shape's launches and the weight baked in)
            hh->cycle_shape = shape;
            hh->over = over_correction;
            for (int l = 0; l + 1 < (int)hh->lv.size(); ++l) {
                auto &L = hh->lv[l];
                if (L.plane) L.plane->g.over = over_correction;
                if (L.var7) L.var7->over = over_correction;
                if (L.s27) L.s27->g.over = over_correction;
                // (the row kernels' edition of the prolongation's values: now where the format exists, else when it is built)
                if (!L.format_pending) ensure_prolong_values(hh, l, over_correction);
            }
        });
    });
}

int omg_hierarchy_get_cycle(const omg_hierarchy *h, int *shape, double *over_correction) {
    return guarded([&] {
        OMG_REQUIRE(shape && over_correction, "null argument");
        with(h, [&](auto *hh) { *shape = hh->cycle_shape; *over_correction = hh->over; });
    });
}

int omg_hierarchy_tail_info(const omg_hierarchy *h, int64_t *out2) {
    return guarded([&] {
        OMG_REQUIRE(out2, "null");
        with(h, [&](auto *hh) { out2[0] = hh->tail_launches; out2[1] = hh->tail_replayed; });
    });
}

int omg_hierarchy_plane_info(const omg_hierarchy *h, int level, int64_t *out8) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            OMG_REQUIRE(out8, "null");
            for (int i = 0; i < 8; ++i) out8[i] = 0;
            const auto &L = hh->lv[level];
            if (!L.plane) return;
            const PlaneGeom &g = L.plane->g;
            const int64_t v[8] = {g.nx, g.ny, g.nz, g.TX, g.TY, g.LZ, g.n_wg, g.threads};
            for (int i = 0; i < 8; ++i) out8[i] = v[i];
        });
    });
}

int omg_hierarchy_set_info(const omg_hierarchy *h, int level, int set, int64_t *rows, int64_t *nnz) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            ensure_format(hh, level);
            const auto &A = hh->lv[level].A;
            OMG_REQUIRE(set >= 0 && size_t(set) < A.n_sets() && rows && nnz, "set out of range / null");
            *rows = A.sets[set + 1] - A.sets[set];
            *nnz = A.set_nnz[set];
        });
    });
}

int omg_hierarchy_format_info(const omg_hierarchy *h, int level, int op, int set, int64_t *out) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, level);
            OMG_REQUIRE(out && op >= 0 && op <= 2, "null / unknown operator");
            OMG_REQUIRE(op == 0 || level + 1 < (int)hh->lv.size(), "the coarsest level has no restriction");
            ensure_format(hh, level);
            const auto &L = hh->lv[level];
            (op == 0 ? L.A : op == 1 ? L.R : L.P).format_info(set, out);
        });
    });
}

int omg_format_selftest(const omg_csr *A, int dtype, int64_t *out) {
    return guarded([&] {
        OMG_REQUIRE(A && out, "null argument");
        OMG_REQUIRE(dtype == OMG_DTYPE_F64 || dtype == OMG_DTYPE_F32, "unknown dtype");
        validate_csr(*A, "A");
        if (dtype == OMG_DTYPE_F32) format_selftest<float>(*A, out);
        else format_selftest<double>(*A, out);
    });
}

int omg_vcycle(omg_hierarchy *h, int level, const double *b, double *x, int pre, int post,
               double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_vcycle");
            check_level(hh, level);
            OMG_REQUIRE(b && x, "b / x is null");
            OMG_REQUIRE(pre >= 0 && post >= 0, "negative sweep count");
            const double nv = level_cycle(hh, false, level, b, x, x, nullptr, pre, post);
            if (norm) *norm = nv;
        });
    });
}

int omg_vcycle_ex(omg_hierarchy *h, int level, const double *b, const double *x_in, double *x_out, double *x_pre,
                  int pre, int post, double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_vcycle_ex");
            check_level(hh, level);
            OMG_REQUIRE(b && x_out, "b / x_out is null");
            OMG_REQUIRE(pre >= 0 && post >= 0, "negative sweep count");
            const double nv = level_cycle(hh, false, level, b, x_in, x_out, x_pre, pre, post);
            if (norm) *norm = nv;
        });
    });
}

// omg_vcycle_ex for a caller whose b / initial / uOut are DEVICE arrays (double, natural numbering): openmg.mgCycle
// (openmg/__init__.py:151-236) chained on the GPU — nothing but the norm (8 bytes) crosses PCIe.  x_in_dev NULL: zeros;
// x_pre_dev (may be x_in_dev): the iterate after the pre-smoothing (Q2), the input's copy / zeros where none ran.
int omg_vcycle_dev(omg_hierarchy *h, int level, const double *b_dev, const double *x_in_dev, double *x_out_dev, double *x_pre_dev,
                   int pre, int post, double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_vcycle_dev");
            check_level(hh, level);
            OMG_REQUIRE(b_dev && x_out_dev, "b / x_out is null");
            OMG_REQUIRE(pre >= 0 && post >= 0, "negative sweep count");
            const double nv = level_cycle(hh, true, level, b_dev, x_in_dev, x_out_dev, x_pre_dev, pre, post);
            if (norm) *norm = nv;
        });
    });
}

// omg_resident_load / omg_resident_fetch with device arrays (double, natural numbering): mgSolve for a caller on the GPU
int omg_resident_load_dev(omg_hierarchy *h, const double *b_dev, const double *x0_dev) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(b_dev, "b is null");
            resident_load(hh, b_dev, x0_dev, true);
            OMG_HIP(hipStreamSynchronize(hh->stream));
            hh->resident = true;
        });
    });
}

int omg_resident_fetch_dev(omg_hierarchy *h, double *x_dev) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident && x_dev, "nothing resident / x is null");
            resident_fetch(hh, x_dev, true);
        });
    });
}

// Device-pointer V-cycle for callers that already live on the GPU (the multi-GPU runner uses
// a replicated hierarchy as its coarse solver): b_dev, x_dev are level-0 DOUBLE vectors in
// natural numbering; x starts from zero (openmg/__init__.py:191-192); enqueued on
// `hip_stream`, no host synchronisation.
int omg_hierarchy_cycle_dev(omg_hierarchy *h, const double *b_dev, double *x_dev, int pre, int post,
                            void *hip_stream) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_hierarchy_cycle_dev");
            using V = value_of<decltype(hh)>;
            check_level(hh, 0);
            OMG_REQUIRE(b_dev && x_dev && pre >= 0 && post >= 0, "bad argument");
            auto &L = hh->lv[0];
            hipStream_t keep = hh->stream;
            hh->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : hh->own;
            hh->resident = false;
            try {
                const int32_t *perm = L.ord.identity ? nullptr : L.perm.p;
                if (direct_io(L)) OMG_HIP(hipMemcpyAsync(L.b.p, b_dev, L.n * sizeof(double), hipMemcpyDeviceToDevice, hh->stream));
                else launch_gather<double, V>(b_dev, perm, L.b.p, L.n, hh->stream);
                zero_start_cycle(hh, pre, post);
                if (direct_io(L)) OMG_HIP(hipMemcpyAsync(x_dev, L.xp, L.n * sizeof(double), hipMemcpyDeviceToDevice, hh->stream));
                else launch_scatter<V, double>(L.xp, perm, x_dev, L.n, hh->stream);
            } catch (...) {
                hh->stream = keep;
                throw;
            }
            hh->stream = keep;
        });
    });
}

int omg_resident_load(omg_hierarchy *h, const double *b, const double *x0) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(b, "b is null");
            resident_load(hh, b, x0, false);
            OMG_HIP(hipStreamSynchronize(hh->stream));
            hh->resident = true;
        });
    });
}

int omg_resident_cycle(omg_hierarchy *h, int pre, int post, double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            OMG_REQUIRE(pre >= 0 && post >= 0, "negative sweep count");
            if (hh->mixed) {
                mixed_cycles(hh, pre, post, 1, hh->norm_dev.p);
                const double nv = read_norm(hh);
                if (norm) *norm = nv;
                return;
            }
            run_cycle0(hh, pre, post);
            if (norm) *norm = read_norm(hh);
        });
    });
}

// n cycles back to back, EVERY cycle's residual norm computed and returned (norms[n], host).  Where
// can_prenorm() holds, the norm of cycle k is finished inside cycle k + 1's first launch instead of
// by a launch of its own (same partial sums, same order: the same bits as n omg_resident_cycle
// calls); the last cycle's by the usual norm launch.  One host synchronisation at the end.
int omg_resident_cycles(omg_hierarchy *h, int pre, int post, int n_cycles, double *norms) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            OMG_REQUIRE(pre >= 0 && post >= 0 && n_cycles >= 0, "negative argument");
            if (n_cycles == 0) return;
            if (hh->norms_dev.n < size_t(n_cycles)) hh->norms_dev.alloc(size_t(n_cycles));
            if (hh->mixed) mixed_cycles(hh, pre, post, n_cycles, hh->norms_dev.p);
            else batched_cycles(hh, pre, post, n_cycles, hh->norms_dev.p);
            if (norms) OMG_HIP(hipMemcpyAsync(norms, hh->norms_dev.p, size_t(n_cycles) * sizeof(double), hipMemcpyDeviceToHost, hh->stream));
            OMG_HIP(hipStreamSynchronize(hh->stream));
            check_march(hh);       // (the batched entry returned norms of a sweep that had given up)
        });
    });
}

// Plain fine-grid SpMV y = A_0 x over the WHOLE operator (x: the resident iterate, y: the
// level's residual buffer, which every cycle overwrites anyway), `reps` launches timed as one
// hipEvent bracket on the hierarchy's stream: the "fine-grid SpMV GB/s" of BASELINE.json's
// metric, measured on the operator as it sits in HBM inside the V-cycle.
int omg_resident_spmv_time(omg_hierarchy *h, int reps, double *avg_ms) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident && reps > 0 && avg_ms, "nothing resident / bad argument");
            OMG_REQUIRE(hh->lv.size() > 1, "single-level hierarchy has no smoothed operator");
            auto &L = hh->lv[0];
            // a plane level (red-black ordered constant-coefficient stencil): matrix-free, like its cycle; y = the level's
            // scratch vector.  Anything else: the row kernels on the operator as it sits in HBM.
            const bool mf = use_plane(hh, L) && !L.plane->g.jacobi;
            if (!mf) ensure_format(hh, 0);
            RowArgsT<V> a;
            a.x = L.xp; a.y = mf ? L.tp : L.r.p;
            // (OMG_SPMV_Y=b / own, read at every call — placement experiments: the product written over the right-hand side, or
            // into an allocation of its own, instead of the level's scratch vector)
            if (mf) ensure_spmv_y(hh, L);
            V *ymf = L.spmv_y.p;
            DevBuf<V> own_y;
            if (const char *e = getenv("OMG_SPMV_Y")) {
                if (e[0] == 'b') ymf = L.b.p;
                else if (e[0] == 't') ymf = L.tp;
                else if (e[0] == 'o') { own_y.alloc(size_t(L.n), size_t(atoi(e + 1)) * 64); ymf = own_y.p; }
            }
            auto once = [&] {
                if (mf) L.plane->spmv(L.xp, ymf, hh->stream);
                else launch_rows(L.A, ROW_SPMV, -1, a, hh->stream);
            };
            once();                                                     // warm-up
            hipEvent_t e0, e1;
            OMG_HIP(hipEventCreate(&e0));
            OMG_HIP(hipEventCreate(&e1));
            OMG_HIP(hipEventRecord(e0, hh->stream));
            for (int i = 0; i < reps; ++i) once();
            OMG_HIP(hipEventRecord(e1, hh->stream));
            OMG_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            OMG_HIP(hipEventElapsedTime(&ms, e0, e1));
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            *avg_ms = double(ms) / reps;
        });
    });
}

int omg_resident_fetch(omg_hierarchy *h, double *x) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident && x, "nothing resident / x is null");
            resident_fetch(hh, x, false);
        });
    });
}

int omg_resident_pcg(omg_hierarchy *h, int pre, int post, int max_iter, double threshold, int *iterations, double *norms,
                     double *true_norm, int *breakdown) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            OMG_REQUIRE(pre >= 0 && post >= 0 && max_iter >= 1, "negative sweep count / max_iter < 1");
            OMG_REQUIRE(hh->lv.size() > 1, "a single-level hierarchy solves directly: nothing to accelerate");
            resident_pcg(hh, pre, post, max_iter, threshold, iterations, norms, true_norm, breakdown);
        });
    });
}

int omg_resident_norms(omg_hierarchy *h, double *rhs_norm, double *residual_norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            if (rhs_norm || residual_norm) resident_norms(hh, rhs_norm, residual_norm);
        });
    });
}

int omg_resident_projection(omg_hierarchy *h, int capacity) {
    return guarded([&] { with(h, [&](auto *hh) { projection_alloc(hh, capacity); }); });
}

int omg_resident_project(omg_hierarchy *h, int *used) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            projection_project(hh, used);
        });
    });
}

int omg_resident_project_update(omg_hierarchy *h, int *size, int *kept) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            projection_update(hh, size, kept);
        });
    });
}

int omg_resident_projection_fetch(omg_hierarchy *h, int index, double *v) {
    return guarded([&] { with(h, [&](auto *hh) { projection_fetch(hh, index, v); }); });
}

int omg_resident_projection_time(omg_hierarchy *h, int reps, double *dots_ms, double *dot_ms, double *lincomb_ms) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            check_level(hh, 0);
            OMG_REQUIRE(hh->resident, "omg_resident_load has not been called");
            projection_time(hh, reps, dots_ms, dot_ms, lincomb_ms);
        });
    });
}

int omg_resident_use_graph(omg_hierarchy *h, int enable) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            OMG_HIP(hipStreamSynchronize(hh->stream));
            hh->want_graph = enable != 0;
            if (!enable) drop_graph(hh);
        });
    });
}

int omg_solve(omg_hierarchy *h, const double *b, double *x, int pre, int post, int max_cycles,
              double threshold, int *cycles_done, double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_solve");
            check_level(hh, 0);
            OMG_REQUIRE(b && x, "b / x is null");
            OMG_REQUIRE(max_cycles > 0 || threshold > 0.0,
                        "Either threshold or cycles must be > 0");   // openmg/__init__.py:118-119
            resident_load(hh, b, x, false);                           // (load, cycles, fetch: as the resident entries)
            hh->resident = true;
            int cycle = 0;
            double nv = 0.0;
            for (;;) {                                                // :112, :132-138
                run_cycle0(hh, pre, post);
                nv = read_norm(hh);
                ++cycle;
                const bool by_cycles = max_cycles > 0 && cycle >= max_cycles;
                const bool by_norm = threshold > 0.0 && nv < threshold;
                if (by_cycles || by_norm) break;
            }
            resident_fetch(hh, x, false);
            if (cycles_done) *cycles_done = cycle;
            if (norm) *norm = nv;
        });
    });
}

int omg_profile_enable(omg_hierarchy *h, int enable) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            OMG_HIP(hipStreamSynchronize(hh->stream));
            for (auto &e : hh->events) { hh->event_pool.push_back(e.a); hh->event_pool.push_back(e.b); }
            hh->events.clear();
            std::memset(hh->prof_n, 0, sizeof(hh->prof_n));
            std::memset(hh->prof_ms, 0, sizeof(hh->prof_ms));
            hh->profiling = (unsigned)enable;   // bit c = class c; -1 = all classes
        });
    });
}

int omg_profile_read(omg_hierarchy *h, int64_t *launches, double *total_ms) {
    return guarded([&] {
        OMG_REQUIRE(launches && total_ms, "null argument");
        with(h, [&](auto *hh) {
            OMG_HIP(hipStreamSynchronize(hh->stream));
            for (auto &e : hh->events) {
                float ms = 0.f;
                OMG_HIP(hipEventElapsedTime(&ms, e.a, e.b));
                hh->prof_n[e.cls] += 1;
                hh->prof_ms[e.cls] += ms;
                hh->event_pool.push_back(e.a);
                hh->event_pool.push_back(e.b);
            }
            hh->events.clear();
            for (int c = 0; c < OMG_PROFILE_CLASSES; ++c) { launches[c] = hh->prof_n[c]; total_ms[c] = hh->prof_ms[c]; }
        });
    });
}

// ---- single level operations ------------------------------------------------------------
int omg_level_smooth(omg_hierarchy *h, int level, const double *b, double *x, int iterations) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "the coarsest level has no smoother");
            OMG_REQUIRE(b && x && iterations >= 0, "bad argument");
            auto &L = hh->lv[level];
            hh->resident = false;
            load_vec(hh, level, b, L.b.p);
            load_vec(hh, level, x, L.xp);
            smooth_level(hh, level, iterations);
            fetch_vec<V>(hh, level, L.xp, x);
        });
    });
}

int omg_level_project(omg_hierarchy *h, int level, double *x_inout, double *mean) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(x_inout, "x is null");
            auto &L = hh->lv[level];
            hh->resident = false;
            load_vec(hh, level, x_inout, L.xp);
            project_vec(hh, L.xp, L.n);
            double sum = 0.0;
            OMG_HIP(hipMemcpyAsync(&sum, hh->proj_scratch.p + PROJECT_MAX_WG, sizeof(double), hipMemcpyDeviceToHost, hh->stream));
            fetch_vec<V>(hh, level, L.xp, x_inout);                   // (synchronises)
            if (mean) *mean = L.n > 0 ? sum / double(L.n) : 0.0;
        });
    });
}

int omg_level_residual(omg_hierarchy *h, int level, const double *b, const double *x, double *r,
                       double *norm) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "use omg_residual for the coarsest operator");
            OMG_REQUIRE(b && x && r, "null vector");
            auto &L = hh->lv[level];
            hh->resident = false;
            load_vec(hh, level, b, L.b.p);
            load_vec(hh, level, x, L.xp);
            if (norm) {
                norm_level<V>(hh, level, L.r.p);
                *norm = read_norm(hh);
            } else {
                residual_level<V>(hh, level, L.r.p);
            }
            fetch_vec<V>(hh, level, L.r.p, r);
        });
    });
}

int omg_level_spmv(omg_hierarchy *h, int level, const double *x, double *y) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "use omg_spmv for the coarsest operator");
            OMG_REQUIRE(x && y, "null vector");
            auto &L = hh->lv[level];
            hh->resident = false;
            load_vec(hh, level, x, L.xp);
            const bool mf = use_plane(hh, L) && !L.plane->g.jacobi;
            if (mf) {
                ensure_spmv_y(hh, L);
                L.plane->spmv(L.xp, L.spmv_y.p, hh->stream);
                fetch_vec<V>(hh, level, L.spmv_y.p, y);
            } else {
                ensure_format(hh, level);
                RowArgsT<V> a;
                a.x = L.xp; a.y = L.r.p;
                launch_rows(L.A, ROW_SPMV, -1, a, hh->stream);
                fetch_vec<V>(hh, level, L.r.p, y);
            }
        });
    });
}

// omg_level_spmv for a caller whose vectors live in HBM (double, the caller's numbering): permuted in and out as
// omg_hierarchy_cycle_dev does, on the hierarchy's stream, through two vectors of its own — the resident right-hand side and
// iterate, and with them a solve in progress, are not touched (the kernels read and write the library's own allocations
// only, as everywhere; y_dev may be x_dev).  Waits for the stream.
int omg_level_spmv_dev(omg_hierarchy *h, int level, const double *x_dev, double *y_dev) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            refuse_mixed(hh, "omg_level_spmv_dev");
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "use omg_spmv for the coarsest operator");
            OMG_REQUIRE(x_dev && y_dev, "null vector");
            auto &L = hh->lv[level];
            const bool mf = use_plane(hh, L) && !L.plane->g.jacobi;
            if (!mf) ensure_format(hh, level);
            if (hh->mv_x.n < size_t(L.n)) { hh->mv_x.alloc(size_t(L.n)); hh->mv_y.alloc(size_t(L.n)); }
            load_vec_dev(hh, level, x_dev, hh->mv_x.p);
            if (mf) {
                L.plane->spmv(hh->mv_x.p, hh->mv_y.p, hh->stream);
            } else {
                RowArgsT<V> a;
                a.x = hh->mv_x.p; a.y = hh->mv_y.p;
                launch_rows(L.A, ROW_SPMV, -1, a, hh->stream);
            }
            fetch_vec_dev(hh, level, hh->mv_y.p, y_dev);
            OMG_HIP(hipStreamSynchronize(hh->stream));
        });
    });
}

int omg_level_restrict(omg_hierarchy *h, int level, const double *fine, double *coarse) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "no restriction below the coarsest level");
            OMG_REQUIRE(fine && coarse, "null vector");
            auto &L = hh->lv[level];
            auto &C = hh->lv[level + 1];
            hh->resident = false;
            load_vec(hh, level, fine, L.r.p);
            restrict_level<V>(hh, level, L.r.p, C.b.p);
            fetch_vec<V>(hh, level + 1, C.b.p, coarse);
        });
    });
}

int omg_level_prolong_add(omg_hierarchy *h, int level, const double *coarse, double *fine_inout) {
    return guarded([&] {
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            check_level(hh, level);
            OMG_REQUIRE(level < (int)hh->lv.size() - 1, "no prolongation below the coarsest level");
            OMG_REQUIRE(coarse && fine_inout, "null vector");
            auto &L = hh->lv[level];
            auto &C = hh->lv[level + 1];
            hh->resident = false;
            load_vec(hh, level + 1, coarse, C.xp);
            load_vec(hh, level, fine_inout, L.xp);
            prolong_add_level<V>(hh, level, C.xp, L.xp, 1.0);      // (the operator R^T itself: no over-correction)
            fetch_vec<V>(hh, level, L.xp, fine_inout);
        });
    });
}

int omg_coarse_solve(omg_hierarchy *h, const double *b, double *x) {
    return guarded([&] {
        OMG_REQUIRE(b && x, "null argument");
        with(h, [&](auto *hh) {
            using V = value_of<decltype(hh)>;
            const int last = (int)hh->lv.size() - 1;
            auto &L = hh->lv[last];
            hh->resident = last != 0 ? hh->resident : false;
            load_vec(hh, last, b, L.b.p);
            coarse_solve_level(hh);
            fetch_vec<V>(hh, last, L.xp, x);
        });
    });
}

int omg_hierarchy_coarse_info(const omg_hierarchy *h, int64_t *out4) {
    return guarded([&] {
        OMG_REQUIRE(out4, "null argument");
        with(h, [&](auto *hh) {
            out4[0] = hh->coarse.P;
            out4[1] = hh->coarse.n;
            out4[2] = hh->coarse.w;
            out4[3] = int64_t(hh->coarse.bytes);
        });
    });
}

// ---- standalone (double only: these mirror the reference's fp64 operators one to one) -------
static void standalone_rows(const omg_csr *A, int mode, const double *x, const double *b,
                            double *y, double *norm) {
    OMG_REQUIRE(A && x && y, "null argument");
    validate_csr(*A, "A");
    OneShot os;
    HostCsr Ah = permute_csr(*A, nullptr, nullptr);
    os.A.upload(Ah, {}, os.s);
    DevBuf<double> dx(std::max<int64_t>(A->n_cols, 1)), dy(std::max<int64_t>(A->n_rows, 1)), db, part, nrm;
    dx.upload(x, A->n_cols, os.s);
    RowArgs a;
    a.x = dx.p; a.y = dy.p;
    if (b) { db.alloc(std::max<int64_t>(A->n_rows, 1)); db.upload(b, A->n_rows, os.s); a.b = db.p; }
    if (norm) { part.alloc(os.A.n_blocks() + SUM_FOLD); nrm.alloc(1); a.partials = part.p; }
    launch_rows(os.A, mode, -1, a, os.s);
    if (norm) {
        launch_sum_sqrt(part.p, os.A.n_blocks(), nrm.p, os.s);
        nrm.download(norm, 1, os.s);
    }
    dy.download(y, A->n_rows, os.s);
    OMG_HIP(hipStreamSynchronize(os.s));
}

int omg_spmv(const omg_csr *A, const double *x, double *y) {
    return guarded([&] { standalone_rows(A, ROW_SPMV, x, nullptr, y, nullptr); });
}

int omg_residual(const omg_csr *A, const double *b, const double *x, double *r, double *norm) {
    return guarded([&] {
        OMG_REQUIRE(b, "b is null");
        OMG_REQUIRE(A && A->n_rows == A->n_cols, "residual needs a square operator");
        standalone_rows(A, norm ? ROW_RESNORM : ROW_RESIDUAL, x, b, r, norm);
    });
}

int omg_gauss_seidel(const omg_csr *A, const double *b, double *x, int smoother, double omega,
                     int iterations, double threshold, int *sweeps_done) {
    return guarded([&] {
        using H = Hier<double>;
        OMG_REQUIRE(A && b && x, "null argument");
        refuse_line_smoother(smoother, "omg_gauss_seidel");
        OMG_REQUIRE(A->n_rows == A->n_cols, "smoother needs a square operator");
        validate_csr(*A, "A");
        check_diagonal(*A, 0);
        if (iterations < 0 && threshold < 0.0) iterations = 1;      // openmg/solvers.py:39-40
        // a two-"level" shell so that the level machinery (ordering, plan) is reused
        require_device();
        std::unique_ptr<H> h(new H);
        h->smoother = smoother;
        h->omega = omega;
        OMG_HIP(hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
        h->stream = h->own;
        h->lv.resize(2);           // level 1 is a dummy so that level 0 counts as "smoothed"
        h->norm_dev.alloc(1);
        Level<double> &L = h->lv[0];
        L.n = A->n_rows;
        order_level(L, *A, smoother, h->stream);
        const bool id = L.ord.identity;
        {
            HostCsr Ap = permute_csr(*A, id ? nullptr : L.ord.perm.data(), id ? nullptr : L.ord.inv.data());
            L.A.upload(Ap, L.ord.sets, h->stream);
        }
        if (!id) { L.perm.alloc(L.n); L.perm.upload(L.ord.perm.data(), L.n, h->stream); }
        L.x.alloc(std::max<int64_t>(L.n, 1));
        L.b.alloc(std::max<int64_t>(L.n, 1));
        if (smoother == OMG_SMOOTH_JACOBI) L.tmp.alloc(std::max<int64_t>(L.n, 1));
        L.partials.alloc(L.A.n_blocks() + SUM_FOLD);
        L.xp = L.x.p;
        L.tp = L.tmp.p;
        build_plan(L);
        load_vec(h.get(), 0, b, L.b.p);
        load_vec(h.get(), 0, x, L.xp);
        int it = 0;
        auto stop = [&]() {                                          // openmg/solvers.py:43-50
            const bool by_iter = iterations >= 0 && it >= iterations;
            bool by_norm = false;
            if (threshold >= 0.0) {
                norm_level<double>(h.get(), 0, nullptr);
                by_norm = read_norm(h.get()) < threshold;
            }
            return by_iter || by_norm;
        };
        while (!stop()) {                                            // :52-54, :72-74
            smooth_level(h.get(), 0, 1);
            ++it;
        }
        fetch_vec<double>(h.get(), 0, L.xp, x);
        if (sweeps_done) *sweeps_done = it;
    });
}

int omg_direct_solve(const omg_csr *A, const double *b, double *x) {
    return guarded([&] {
        OMG_REQUIRE(A && b && x, "null argument");
        OMG_REQUIRE(A->n_rows == A->n_cols, "direct solve needs a square operator");
        validate_csr(*A, "A");
        OneShot os;
        HostCsr Ah = permute_csr(*A, nullptr, nullptr);
        os.A.upload(Ah, {}, os.s);
        const int64_t n = A->n_rows;
        DevBuf<double> db(std::max<int64_t>(n, 1)), dx(std::max<int64_t>(n, 1));
        CoarseSolver<double> cs;
        cs.build(Ah, os.s);
        db.upload(b, n, os.s);
        cs.solve(db.p, dx.p, os.s);
        dx.download(x, n, os.s);
        OMG_HIP(hipStreamSynchronize(os.s));
    });
}

}  // extern "C"
