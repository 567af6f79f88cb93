/*
 * openmg_hip.h — C ABI of libopenmg_hip.so, the MI355X (gfx950) implementation of the
 * multigrid V-cycle hot path of tsbertalan/openmg.
 *
 * The reference is pure Python and has no FFI of its own, so every entry
 * point below is defined by the reference CALL SITE it replaces; the citation after
 * "replaces:" is a path under the reference root.  The host side (openmg_amd/, Python,
 * ctypes) keeps the reference's function names and dict semantics and forwards here.
 *
 * Conventions
 *   - every pointer is a HOST pointer borrowed for the duration of the call unless the
 *     name ends in _dev; nothing is retained except inside an omg_hierarchy;
 *   - matrices are CSR: int32 indptr[n_rows+1], int32 indices[nnz], float64 data[nnz];
 *     column order inside a row is free (SciPy's SpGEMM leaves it unsorted) and row sums
 *     run in STORED order like the reference's (openmg/solvers.py:63-65);
 *   - vectors are float64;
 *   - every function returns OMG_OK (0) or an OMG_ERR_* code; omg_last_error() gives text;
 *   - there is NO CPU fallback: without a usable GPU every compute call returns
 *     OMG_ERR_NO_DEVICE;
 *   - what the device keeps of an operator is a LOSSLESS recoding of the caller's CSR (row
 *     patterns, dictionaries, block-transposed values; csrc/common.h):
 *     a storage choice per row block that never changes a result bit
 *     (omg_hierarchy_format_info reports it, env OMG_COMPRESS=0 turns it off).
 */
#ifndef OPENMG_HIP_H
#define OPENMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMG_OK                0
#define OMG_ERR_INVALID       1   /* bad argument / shape mismatch                         */
#define OMG_ERR_NO_DEVICE     2   /* no HIP device visible                                 */
#define OMG_ERR_HIP           3   /* a HIP runtime call failed                             */
#define OMG_ERR_SINGULAR      4   /* coarse matrix is singular (reference: SuperLU error)  */
#define OMG_ERR_NO_DIAGONAL   5   /* a row has no stored diagonal (reference: divide by 0) */
#define OMG_ERR_ALLOC         6
#define OMG_ERR_UNSUPPORTED   7

/* Smoother orderings.  The reference has exactly one smoother: lexicographic in-place
 * Gauss-Seidel (openmg/solvers.py:34-75).
 *   GS_LEX    the same iterate as the reference: rows are level-scheduled (row i runs after
 *             every coupled row j<i and before every coupled row j>i), so a sweep is a
 *             sequence of independent row sets — identical arithmetic per row.
 *   GS_COLOUR greedy multi-colour Gauss-Seidel (red-black on 5/7-point stencils, 8 colours
 *             on 27-point); equals the reference's sweep on the colour-permuted system.
 *   JACOBI    weighted Jacobi, x += omega D^-1 (b - A x); no reference counterpart.      */
#define OMG_SMOOTH_GS_LEX     0
#define OMG_SMOOTH_GS_COLOUR  1
#define OMG_SMOOTH_JACOBI     2
/*   LINE      zebra line Gauss-Seidel for anisotropic grid operators (csrc/line.hip; no reference counterpart): the grid
 *             lines along one axis, coloured by the parity of the sum of their other two indices (2-D: of the other
 *             index), are solved exactly — x_line <- T^-1 (b_line - cross couplings * x of the neighbouring lines), T the
 *             line's tridiagonal block of A — colour 0 first, then colour 1, in place.  Axes are named by stride: X is the
 *             unit-stride axis, Z the slowest.  OMG_SMOOTH_LINE takes the axis whose couplings of A[0] have the largest
 *             sum of |a_ij| (ties: the smaller stride); the same axis on every level.  Every smoothed level must be a 3-D
 *             7-point or 2-D 5-point stencil on a lexicographically numbered grid, every row holding exactly its in-grid
 *             neighbours in ascending column order with any coefficients (extents even or odd): otherwise hierarchy
 *             creation returns OMG_ERR_UNSUPPORTED and names the level (27-point, periodic wrap, 1-D, unsorted columns);
 *             OMG_SMOOTH_LINE_Z on a 2-D grid, or a zero / non-finite pivot of a line: OMG_ERR_INVALID.  omega is ignored.
 *             Taken by omg_hierarchy_create, _create_ex and _create_opt.  omg_hierarchy_create_from_fine[_opt],
 *             omg_gauss_seidel, omg_dist_create[_ex] and the omg_*dist_set_tail entries (for a tail made with it)
 *             return OMG_ERR_UNSUPPORTED.  The cycle over such a level runs set by set: two launches per sweep, the full
 *             residual / norm launches, no fused passes.                                                            */
#define OMG_SMOOTH_LINE       3
#define OMG_SMOOTH_LINE_X     4
#define OMG_SMOOTH_LINE_Y     5
#define OMG_SMOOTH_LINE_Z     6
/*   LINE_WRAP a flag OR-ed onto one of the four LINE codes (11 .. 14): the smoothed levels may be PERIODIC.  An axis of
 *             extent e >= 3 and stride s is periodic on a level when row 0 holds column (e - 1) s; its seam rows then hold
 *             the wrapped neighbour as well, columns ascending.  Across the lines the wrapped coupling is one more cross
 *             coupling (the extent must be even there, or the two seam lines had one colour: OMG_ERR_UNSUPPORTED); along the
 *             lines every line is CYCLIC: its block is tridiagonal with two corner entries, factorised once without
 *             pivoting (a fill row and a fill column; a zero, non-finite or vanishing pivot: OMG_ERR_INVALID).  On operators
 *             without wrapped rows the flag changes nothing, bit for bit.  The flag on any other code, and code 7, are
 *             OMG_ERR_INVALID; the entries that refuse the LINE codes refuse these the same way.                       */
#define OMG_SMOOTH_LINE_WRAP  8

typedef struct {
    int64_t n_rows, n_cols, nnz;
    const int32_t *indptr;
    const int32_t *indices;
    const double  *data;
} omg_csr;

typedef struct omg_hierarchy omg_hierarchy;   /* device-resident level hierarchy            */
typedef struct omg_csr_result omg_csr_result; /* device-built CSR waiting to be fetched     */

const char *omg_last_error(void);
int omg_device_count(int *count);
int omg_set_device(int device);
/* free / total memory of the current device (hipMemGetInfo): what a caller sizes its problem by; tests check that
 * destroying a hierarchy gives everything back */
int omg_device_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* every stream of the current device idle (before device arrays another library produced are handed to omg_vcycle_dev) */
int omg_device_synchronize(void);
/* Build identification (git-independent): returns a static string. */
const char *omg_version(void);

/* ---- hierarchy --------------------------------------------------------------------
 * replaces: the A and R lists built by openmg/__init__.py:103-109 and carried through
 * every mgCycle call (openmg/__init__.py:151).  A[0..n_levels-1] are the level operators,
 * R[0..n_levels-2] the restrictions (R[l]: level l -> l+1); prolongation is R[l]^T
 * (openmg/__init__.py:214).  The coarsest operator A[n_levels-1] is factorised once here
 * (the reference refactorises it on every cycle, openmg/solvers.py:23).
 * n_levels == 1 is allowed (direct solve only).                                          */
int omg_hierarchy_create(int n_levels, const omg_csr *A, const omg_csr *R,
                         int smoother, double omega, omg_hierarchy **out);
/* Same, choosing the precision the levels are STORED and COMPUTED in on the device
 * (BASELINE.json configs[4] is fp32).  OMG_DTYPE_F64 is omg_hierarchy_create.  With
 * OMG_DTYPE_F32 the operators are rounded to float once at upload, every vector lives in HBM
 * as float, row sums run in float fma; residual norms are still accumulated in double, and
 * the coarsest operator is inverted in double and then rounded.  Every entry point keeps its
 * double host (and omg_hierarchy_cycle_dev device) vectors: the conversion happens on the
 * device.  The reference has no such switch (it is fp64 throughout); parity for fp32 is
 * "within single-precision rounding of the fp64 iterate", stated per test.               */
#define OMG_DTYPE_F64 0
#define OMG_DTYPE_F32 1
/* Mixed precision: the levels exactly as OMG_DTYPE_F32, plus level 0's outer state in double — its operator taken from
 * the caller's double A[0] (never the float copy), the resident b and iterate, the CG vectors.  The resident entries then
 * iterate in double around the fp32 V-cycle: omg_resident_cycle[s] run defect correction (r = b - A x in double, one
 * zero-start fp32 V-cycle on fl32(r), x += its result; the norm is ||b - A x|| in double after the correction) and
 * omg_resident_pcg runs FCG with z = M(fl32(r)), everything else double — answers to fp64 accuracy with fp32 cycles.
 * omg_vcycle, omg_vcycle_ex, omg_vcycle_dev, omg_solve and omg_hierarchy_cycle_dev return OMG_ERR_UNSUPPORTED on such a
 * hierarchy; the per-level operations act on its fp32 levels.  omg_hierarchy_dtype reports it. */
#define OMG_DTYPE_MIXED 2
int omg_hierarchy_create_ex(int n_levels, const omg_csr *A, const omg_csr *R, int smoother,
                            double omega, int dtype, omg_hierarchy **out);
/* replaces: the setup of openmg.mgSolve — operators.restrictionList(problemShape, ...) + operators.coeffecientList(A_in, R)
 * (openmg/__init__.py:103-109) — and omg_hierarchy_create_ex in ONE call that keeps everything on the device: A_in is
 * uploaded once, every R[l] is built and every Galerkin product (R A) R^T formed in HBM, every smoothed level is
 * qualified there for a fused path (plane passes, 2-D tile passes, 27-point kernels; the grid is the caller's
 * problemShape = shape[0..dim-1], dim 2 or 3, shape[0] == shape[dim-1], extents divisible by 2^n_restrictions), and only
 * the coarsest operator visits the host (its factorisation).  n_restrictions: len(restrictionList(...)) by the
 * reference's depth rule (the caller applies it: it needs the shapes only).  If some level does not qualify its operators
 * are fetched and the hierarchy is built the ordinary way: the same object either way.  The lists mgSolve returns in
 * infoDict['A'], ['R'] are NOT kept: a caller with giveInfo takes the ordinary route.                                  */
int omg_hierarchy_create_from_fine(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, int smoother, double omega,
                                   int dtype, omg_hierarchy **out);
/* Singular operators whose null space is the constant vector (zero row and column sums: the pure-Neumann or periodic
 * Poisson problem; no reference counterpart — openmg/solvers.py:16-26 hands such a coarsest operator to SuperLU, which
 * raises or returns 1e18).  With OMG_NULLSPACE_CONSTANT
 *   - the coarsest operator must have the null space itself: every row sum and every column sum at most 1e-10 times the
 *     sum of the row's / column's absolute entries (Galerkin products of such an operator keep it to rounding), otherwise
 *     OMG_ERR_INVALID; it is inverted as A + gamma 1 1^T, gamma = (mean diagonal) / n, in double, as one explicit inverse
 *     (n > 16384: OMG_ERR_UNSUPPORTED; OMG_COARSE_BLOCKS / OMG_COARSE_CHAIN are ignored):
 *     (A + gamma 1 1^T)^-1 b = pinv(A) b + mean(b) / (gamma n) 1 — the minimum-norm solution for a right-hand side free of
 *     constants, and a rounding-level mean mapped to a rounding-level constant;
 *   - omg_resident_load[_dev] subtract its mean from the resident right-hand side after loading it (the fp64 outer b of an
 *     OMG_DTYPE_MIXED hierarchy; the caller's array and the initial iterate stay as they are: every norm reported
 *     afterwards is that of the projected system), omg_resident_fetch[_dev] subtract its mean from the resident iterate,
 *     in place, before copying it out (the null component of x does not enter the residual: a later cycle continues
 *     unchanged to rounding), omg_solve is load, cycles, fetch;
 *   - omg_vcycle, omg_vcycle_ex, omg_vcycle_dev and omg_hierarchy_cycle_dev do NOT project: they are the reference's
 *     recursive building block, entered at any level with the caller's b;
 *   - the multi-GPU runners refuse such a hierarchy as their tail (omg_*dist_set_tail: OMG_ERR_UNSUPPORTED).
 * The sums of the projection are deterministic (fixed slots, fixed order: csrc/nullspace.hip).  omg_hierarchy_update_fine
 * keeps the setting.  nullspace = OMG_NULLSPACE_NONE is omg_hierarchy_create_ex / omg_hierarchy_create_from_fine, bit for
 * bit; any other value: OMG_ERR_INVALID. */
#define OMG_NULLSPACE_NONE     0
#define OMG_NULLSPACE_CONSTANT 1
typedef struct { int smoother; double omega; int dtype; int nullspace; } omg_hierarchy_options;
int omg_hierarchy_create_opt(int n_levels, const omg_csr *A, const omg_csr *R,
                             const omg_hierarchy_options *opt, omg_hierarchy **out);
int omg_hierarchy_create_from_fine_opt(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions,
                                       const omg_hierarchy_options *opt, omg_hierarchy **out);
int omg_hierarchy_nullspace(const omg_hierarchy *h, int *kind);
/* x <- x - mean(x) on one level's vector (host doubles in natural numbering, through the level's
 * precision and ordering like omg_level_smooth); *mean (nullable) = the mean that was removed.
 * Works on any hierarchy, whatever its nullspace setting. */
int omg_level_project(omg_hierarchy *h, int level, double *x_inout, double *mean);

/* New values for the fine operator of a hierarchy made by omg_hierarchy_create_from_fine whose smoothed levels all run the
 * 27-point kernels (BASELINE configs[4]: "Galerkin RAP rebuilt on-device"; what the reference would do is run
 * operators.coeffecientList again, openmg/operators.py:144-188): data = the CSR's value array in the SAME pattern, nnz
 * doubles, in host memory or — on_device != 0 — already in HBM.  Level 0 is re-tiled, every Galerkin product re-formed
 * on the device in one pass per level (closed form of the aggregation on a grid, SciPy's accumulation order: the bits of
 * a fresh setup), the coarsest operator factorised anew.  The resident right-hand side and iterate stay.  It also takes
 * such a hierarchy whose level 0 runs the 7-point per-row-coefficient passes (var7) and whose smoothed levels are each var7
 * or one of the small host-coded levels below them: the products are re-formed the same way, the host-coded levels
 * rebuilt from theirs.  Any other hierarchy: OMG_ERR_INVALID. */
int omg_hierarchy_update_fine(omg_hierarchy *h, const double *data, int64_t nnz, int on_device);
/* *yes = 1 exactly when omg_hierarchy_update_fine takes this hierarchy (the two kinds named above), else 0: a caller
 * that holds one hierarchy for many solves asks before it decides between an update and a new setup. */
int omg_hierarchy_can_update_fine(const omg_hierarchy *h, int *yes);

/* ---- the 7-point operator of a coefficient field --------------------------------------------------------
 * -div(kappa grad u) + sigma u by cell-centred finite volumes on a box of shape = (nz, ny, nx) cells, C-order numbering.
 * kappa: (nz + 2)(ny + 2)(nx + 2) doubles in C order, the cells and one ghost layer; walls: six flags in the order
 * -z, +z, -y, +y, -x, +x (NULL: all OMG_WALL_DIRICHLET); sigma: NULL (OMG_SIGMA_NONE), one double (OMG_SIGMA_SCALAR) or one per
 * cell (OMG_SIGMA_FIELD); scale: one factor per axis z, y, x (NULL: 1).  kappa and sigma lie in host memory or — *_on_device
 * != 0 — in HBM.  Every operation is rounded once in double, nothing is contracted:
 *     face(a, b) = ((2 a) b) / (a + b),  c = face * scale[axis],  off-diagonal entry -c,
 *     diagonal (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K), then + sigma.
 * The face at a Dirichlet wall takes the ghost cell's kappa and enters the diagonal only; at a Neumann wall it is +0.0.
 * The result is operators.stencil7_kappa's matrix bit for bit: the in-grid neighbours of every row, columns ascending.
 * A kappa that is not finite and > 0 (cells, and the ghost cells behind Dirichlet walls), a sigma that is not finite and
 * >= 0, a scale factor that is not finite and > 0, an unknown wall or sigma kind: OMG_ERR_INVALID — for a value of a field
 * the text names the first such cell (z, y, x), a ghost cell with -1 or the extent; nothing faults, the next call works.
 * Periodic axes: OMG_WALL_PERIODIC on BOTH walls of an axis whose extent is >= 3 (on one wall only, or on a
 * smaller extent: OMG_ERR_INVALID naming the axis).  Every row then holds both neighbours along that axis; the one across
 * the seam is the cell at the other end of the line, its face the inner-face expression with that cell's kappa (and width),
 * its column at its own place in the ascending order; the diagonal is the same sum in the same order.  The ghost layer of
 * kappa along a periodic axis is never read.  omg_hierarchy_create_from_kappa sets such an operator up by the ordinary
 * route (no fused path takes a wrap-around row), so omg_hierarchy_update_kappa answers OMG_ERR_INVALID on the result. */
#define OMG_WALL_DIRICHLET 0
#define OMG_WALL_NEUMANN   1
#define OMG_WALL_PERIODIC  2
#define OMG_SIGMA_NONE   0
#define OMG_SIGMA_SCALAR 1
#define OMG_SIGMA_FIELD  2
/* The CSR arrays: indptr (n + 1), indices and data (nnz = 7 n - 2 (nx ny + nx nz + ny nz), each of the three products
 * counted only where the axis it leaves out — z, y, x in this order — is not periodic), all in host memory or
 * — out_on_device != 0 — all in HBM.  indptr and indices may both be NULL: the values alone. */
int omg_kappa_assemble(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *sigma,
                       int sigma_kind, int sigma_on_device, const double *scale, int32_t *indptr, int32_t *indices, double *data,
                       int out_on_device);
/* omg_hierarchy_create_from_fine_opt of that operator without the operator ever being on the host: level 0 is assembled
 * in HBM, the Galerkin chain starts from it, everything after that is omg_hierarchy_create_from_fine_opt's own sequence
 * — the result is the object it builds from operators.stencil7_kappa's matrix (the same level kinds, the same answer of
 * omg_hierarchy_can_update_fine, the same bits).  The assembled operator is fetched to the host once in two cases: for
 * OMG_DTYPE_MIXED (the fp64 outer operator of level 0 is coded by the host), and — with the whole chain — where a level
 * does not qualify for a fused path and the ordinary route sets the hierarchy up. */
int omg_hierarchy_create_from_kappa(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                                    const double *sigma, int sigma_kind, int sigma_on_device, const double *scale,
                                    int n_restrictions, const omg_hierarchy_options *opt, omg_hierarchy **out);
/* omg_hierarchy_update_fine with the new values made from a coefficient field: they are written into a value array the
 * hierarchy holds in HBM (nnz doubles, allocated at the first call) and take the device path of that entry; with kappa
 * and sigma in HBM nothing crosses to the host but the error word.  Takes exactly the hierarchies for which
 * omg_hierarchy_can_update_fine says 1 and whose level 0 is the 7-point operator on the grid `shape`; any other:
 * OMG_ERR_INVALID, and the hierarchy is as before.  So it is after a refused kappa or sigma.  The resident right-hand side
 * and iterate stay. */
int omg_hierarchy_update_kappa(omg_hierarchy *h, const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                               const double *sigma, int sigma_kind, int sigma_on_device, const double *scale);
/* The same three on a stretched tensor-product grid: hz, hy, hx — HOST memory, nz + 2, ny + 2 and nx + 2
 * doubles — are the cell widths along each axis with one ghost entry at each end, like kappa's ghost layer.  The operator is
 * the volume-integrated one (symmetric; the right-hand side is f times the cell volume); with a, da the cell's own kappa and
 * width along the face's axis and b, db the neighbour's, every operation rounded once in double and nothing contracted:
 *     c = (((2 a) b) / (da b + db a)) area[axis],  area_z = hy[j] hx[i], area_y = hz[k] hx[i], area_x = hz[k] hy[j],
 *     off-diagonal entry -c,  diagonal (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K), then + sigma ((hz[k] hy[j]) hx[i]).
 * A Dirichlet wall face takes the ghost cell's kappa and the ghost width (0: the value sits on the wall face itself; the
 * boundary cell's width: at the mirrored cell centre) and enters the diagonal only; a Neumann wall face is +0.0 and reads
 * neither.  The result is operators.stencil7_kappa(..., spacing = (hz, hy, hx))'s matrix bit for bit.
 * hz = hy = hx = NULL: the entry without widths.  Some but not all NULL, or widths together with a scale that is neither NULL
 * nor all ones: OMG_ERR_INVALID.  An interior width that is not finite and > 0 or a ghost width that is not finite and >= 0:
 * OMG_ERR_INVALID naming the axis and the index (-1 or the extent for a ghost entry), before any launch. */
int omg_kappa_assemble_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *sigma,
                              int sigma_kind, int sigma_on_device, const double *scale, const double *hz, const double *hy,
                              const double *hx, int32_t *indptr, int32_t *indices, double *data, int out_on_device);
int omg_hierarchy_create_from_kappa_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls,
                                           const double *sigma, int sigma_kind, int sigma_on_device, const double *scale,
                                           const double *hz, const double *hy, const double *hx, int n_restrictions,
                                           const omg_hierarchy_options *opt, omg_hierarchy **out);
int omg_hierarchy_update_kappa_spaced(omg_hierarchy *h, const int64_t *shape, const double *kappa, int kappa_on_device,
                                      const int *walls, const double *sigma, int sigma_kind, int sigma_on_device, const double *scale,
                                      const double *hz, const double *hy, const double *hx);
/* ---- the right-hand side that goes with that operator ---------------------------------------------------
 * b, n = nz ny nx doubles in C order: a source per cell and inhomogeneous boundary data for the operator the entries above
 * make of (shape, kappa, walls, scale | hz, hy, hx); sigma plays no part.  operators.rhs_kappa is the definition; the result
 * has its bits.  f: NULL (OMG_VALUE_NONE), one double in HOST memory (OMG_VALUE_SCALAR) or one per cell (OMG_VALUE_FIELD, in
 * host memory or — f_on_device != 0 — in HBM).  value_kinds: six OMG_VALUE_* in the order of the walls (NULL: none has a
 * value); value_scalars: six doubles, read where the kind is SCALAR; value_fields: six pointers, read where the kind is
 * FIELD — one double per face of that wall, (ny, nx) for the z walls, (nz, nx) for the y walls, (nz, ny) for the x walls, C
 * order, all of them in host memory or — values_on_device != 0 — all in HBM.  b lies in host memory or — b_on_device != 0 —
 * in HBM, and may then be f itself (in place).  Host fields are staged in HBM by the entry, as omg_kappa_assemble stages them.
 *   a Dirichlet wall's value g: the boundary value where the operator puts it (the mirrored ghost-cell centre; with widths,
 *     where the ghost width says — 0: on the wall face).  The cell gets c_wall g, c_wall the face coefficient the operator's
 *     diagonal took for this wall: the same expression with the ghost cell's kappa (and width), the same rounding.
 *   a Neumann wall's value: the OUTWARD flux q = kappa du/dn; with widths the cell gets q area[axis].  Without widths the
 *     library does not know the cell width h: the value is then q h, and the cell gets value * scale[axis].
 * Every operation is rounded once in double, nothing is contracted: the volume term is f ((hz[k] hy[j]) hx[i]) with widths,
 * f itself without, +0.0 for no f, and b = ((((((volume term + t-K) + t-J) + t-I) + t+I) + t+J) + t+K); an in-grid face and
 * a wall without a value contribute +0.0.  One launch: f read and b written once (16 bytes per cell); only the cells at a
 * Dirichlet wall with a value read kappa — their own and the ghost cell's — and the ghost width.  Ghost cells behind Neumann
 * walls, periodic walls and Dirichlet walls without a value are never read.
 * kappa is NOT validated here (omg_hierarchy_create_from_kappa / _update_kappa checked the same field), and may be NULL where
 * no Dirichlet wall has a value.  OMG_ERR_INVALID: a value on a periodic wall, NULL where a field is announced, an unknown
 * kind or wall, a periodic wall without its partner or on an extent below 3, widths or scale as the entries above refuse
 * them, n or the padded field beyond int32. */
#define OMG_VALUE_NONE   0
#define OMG_VALUE_SCALAR 1
#define OMG_VALUE_FIELD  2
int omg_kappa_rhs(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                  const double *f, int f_kind, int f_on_device, const int *value_kinds, const double *value_scalars,
                  const double *const *value_fields, int values_on_device, double *b, int b_on_device);
/* ... with the cell widths (hz = hy = hx = NULL: the entry above) */
int omg_kappa_rhs_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                         const double *hz, const double *hy, const double *hx, const double *f, int f_kind, int f_on_device,
                         const int *value_kinds, const double *value_scalars, const double *const *value_fields,
                         int values_on_device, double *b, int b_on_device);
/* ---- the face fluxes of a solution under that operator, and their cell balance ---------------------------
 * fz, fy, fx: (nz + 1) ny nx, nz (ny + 1) nx and nz ny (nx + 1) doubles in C order — F, the flux of -kappa grad u along the
 * +AXIS direction through every face, times the operator's own factor (scale[axis]; with widths the face area), so that the
 * differences of F are the operator's rows: for every u
 *     omg_face_divergence(F) (+ sigma u, with widths sigma V u) = A u - omg_kappa_rhs(f = NULL, the same values)
 * up to rounding.  operators.flux_kappa is the definition; the result has its bits.  shape, kappa, walls, scale | hz, hy, hx
 * and the value arguments are omg_kappa_rhs's; u: n doubles, in host memory or — u_on_device != 0 — in HBM.  Face m of an
 * axis of extent e lies between cell m - 1 (lo) and cell m (hi):
 *   an in-grid face, m = 1 .. e - 1: F = c (u_lo - u_hi), c the bits of -A[lo, hi] = -A[hi, lo].
 *   a periodic axis: faces 0 and e are one face and hold the same bits, c (u_{e-1} - u_0) with c of the cells e - 1 and 0.
 *   a Dirichlet wall: F[0] = c_wall (g - u_0), F[e] = c_wall (u_{e-1} - g); c_wall as in omg_kappa_rhs (the ghost cell's
 *     kappa and width), g the wall's value, +0.0 where it has none.
 *   a Neumann wall: +0.0 where it has no value.  With a value under omg_kappa_rhs's convention — the OUTWARD flux
 *     q = kappa du/dn; WITHOUT widths q times the cell width along the axis — t = value area[axis] (value scale[axis]) and
 *     F[0] = t, F[e] = -t: the outward flux of -kappa grad u is -q.
 * Every operation is rounded once in double, nothing is contracted: one subtraction and one multiplication per face, the
 * coefficient as the operator rounds it.  The ghost cells of kappa behind Neumann and periodic walls are never read; behind a
 * Dirichlet wall they are always read, with or without a value.  kappa is NOT validated, as in omg_kappa_rhs.
 * alpha = NULL: F is stored.  Else (one double in HOST memory) every face gets out = out + alpha F — one multiplication, one
 * addition; the two places of a periodic seam each from their own old value.  The outputs lie in host memory or —
 * out_on_device != 0 — in HBM; host arrays are staged as omg_kappa_rhs stages them.  One launch, each face computed once.
 * OMG_ERR_INVALID: what omg_kappa_rhs refuses; a NULL kappa, u or output; alpha not finite; an output that overlaps u, kappa
 * or another output (threads read their neighbours' u: the fluxes cannot be made in place); a face array beyond int32. */
int omg_kappa_flux(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                   const double *u, int u_on_device, const int *value_kinds, const double *value_scalars,
                   const double *const *value_fields, int values_on_device, const double *alpha, double *fz, double *fy, double *fx,
                   int out_on_device);
/* ... with the cell widths (hz = hy = hx = NULL: the entry above) */
int omg_kappa_flux_spaced(const int64_t *shape, const double *kappa, int kappa_on_device, const int *walls, const double *scale,
                          const double *hz, const double *hy, const double *hx, const double *u, int u_on_device,
                          const int *value_kinds, const double *value_scalars, const double *const *value_fields,
                          int values_on_device, const double *alpha, double *fz, double *fy, double *fx, int out_on_device);
/* out, n doubles: ((fz[k + 1] - fz[k]) + (fy[j + 1] - fy[j])) + (fx[i + 1] - fx[i]) per cell, in that order, each operation
 * rounded once (operators.divergence_faces' bits).  The face arrays all in host memory or — faces_on_device != 0 — all in HBM.
 * OMG_ERR_INVALID: a NULL argument, an extent below 1, a face array beyond int32, an output that overlaps a face array. */
int omg_face_divergence(const int64_t *shape, const double *fz, const double *fy, const double *fx, int faces_on_device,
                        double *out, int out_on_device);
/* ---- the 7-point operator of one coefficient per FACE ----------------------------------------------------
 * For callers that hold their coefficients on the faces (a MAC grid's 1 / rho, orthotropic media, metric factors): cz, cy, cx
 * are (nz + 1) ny nx, nz (ny + 1) nx and nz ny (nx + 1) doubles in C order — the face arrays omg_kappa_flux writes and
 * omg_face_divergence reads —, all three in host memory or — faces_on_device != 0 — all in HBM.  Along an axis of extent e,
 * face m lies between cell m - 1 and cell m.  The coefficients carry every factor: there is no scale and there are no widths.
 *   an in-grid face, m = 1 .. e - 1: A[lo, hi] = A[hi, lo] = -C[m].
 *   a Dirichlet wall: C[0] and C[e] enter the diagonal of the cell at the wall only.
 *   a Neumann wall: its face contributes +0.0 and its entry of C is never read (it may hold NaN).
 *   a periodic axis (both walls, extent >= 3): the seam's coefficient is C[0]; C[e] is never read.
 *   diagonal (((((c-K + c-J) + c-I) + c+I) + c+J) + c+K), then + sigma (no volume factor), every operation rounded once.
 * walls, sigma, the outputs and the pattern are omg_kappa_assemble's; the result is operators.stencil7_faces' matrix bit for bit.
 * A coefficient on a face that is read which is not finite and > 0, a sigma that is not finite and >= 0: OMG_ERR_INVALID
 * naming ONE offender — of the arrays in the order Cz, Cy, Cx, sigma the first that has one, and in it the smallest flat
 * index, as face (k, j, i) of that array's own shape (sigma: the cell) —; nothing faults, the next call works. */
int omg_faces_assemble(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                       const double *sigma, int sigma_kind, int sigma_on_device, int32_t *indptr, int32_t *indices, double *data,
                       int out_on_device);
/* omg_hierarchy_create_from_kappa's sequence with that assembly: level 0 is assembled in HBM, the rest is
 * omg_hierarchy_create_from_fine_opt's own — the object it builds from operators.stencil7_faces' matrix, bit for bit (one
 * download of level 0 for OMG_DTYPE_MIXED; periodic walls and levels that do not qualify: the ordinary route). */
int omg_hierarchy_create_from_faces(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device,
                                    const int *walls, const double *sigma, int sigma_kind, int sigma_on_device, int n_restrictions,
                                    const omg_hierarchy_options *opt, omg_hierarchy **out);
/* omg_hierarchy_update_kappa with that assembly: the values go into the same array the hierarchy holds in HBM and take
 * omg_hierarchy_update_fine's device path.  The same hierarchies (omg_hierarchy_can_update_fine, level 0 the 7-point
 * operator on `shape`, no periodic wall); any other, and a refused coefficient or sigma: OMG_ERR_INVALID, the hierarchy as before. */
int omg_hierarchy_update_faces(omg_hierarchy *h, const int64_t *shape, const double *cz, const double *cy, const double *cx,
                               int faces_on_device, const int *walls, const double *sigma, int sigma_kind, int sigma_on_device);
/* The right-hand side that goes with that operator (operators.rhs_faces' bits): b = ((((((f + t-K) + t-J) + t-I) + t+I) +
 * t+J) + t+K).  A Dirichlet wall with the value g gives the cell at it C_wall g (C[0] or C[e]); a Neumann wall's value is the
 * OUTWARD flux through the face already integrated over it, t = value with no factor; an in-grid face and a wall without a
 * value give +0.0.  f, the values and b as omg_kappa_rhs takes them.  Only the cells at a Dirichlet wall with a value read a
 * coefficient; the arrays may be NULL where there is none.  The coefficients are NOT validated here. */
int omg_faces_rhs(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                  const double *f, int f_kind, int f_on_device, const int *value_kinds, const double *value_scalars,
                  const double *const *value_fields, int values_on_device, double *b, int b_on_device);
/* The face fluxes of u under that operator (operators.flux_faces' bits), omg_kappa_flux's outputs, alpha and mapping:
 *   an in-grid face F[m] = C[m] (u_lo - u_hi); a periodic axis F[0] = F[e] = C[0] (u_{e-1} - u_0);
 *   a Dirichlet wall F[0] = C[0] (g - u_0), F[e] = C[e] (u_{e-1} - g), g = +0.0 without a value;
 *   a Neumann wall +0.0 without a value and nothing read, else F[0] = value, F[e] = -value.
 * One subtraction and one multiplication per face; with alpha out = out + alpha F, one multiplication and one addition.
 * omg_face_divergence(F) + sigma u = A u - omg_faces_rhs(f = NULL, the same values) up to rounding.
 * OMG_ERR_INVALID: what omg_faces_rhs refuses; a NULL array; alpha not finite; an output that overlaps u, a coefficient
 * array or another output. */
int omg_faces_flux(const int64_t *shape, const double *cz, const double *cy, const double *cx, int faces_on_device, const int *walls,
                   const double *u, int u_on_device, const int *value_kinds, const double *value_scalars,
                   const double *const *value_fields, int values_on_device, const double *alpha, double *fz, double *fy, double *fx,
                   int out_on_device);
int omg_hierarchy_dtype(const omg_hierarchy *h, int *dtype);
int omg_hierarchy_destroy(omg_hierarchy *h);
/* Run on a caller-owned hipStream_t instead of the hierarchy's own stream (NULL = own). */
int omg_hierarchy_set_stream(omg_hierarchy *h, void *hip_stream);
int omg_hierarchy_sync(omg_hierarchy *h);
/* Rows of level l; number of independent row sets one smoother sweep is split into. */
int omg_hierarchy_level_rows(const omg_hierarchy *h, int level, int64_t *n_rows);
int omg_hierarchy_level_sets(const omg_hierarchy *h, int level, int64_t *n_sets);
/* 1 when the smoother's last set launch of this level also produces that set's residual /
 * norm share (ROW_GS_RES / ROW_GS_NORM in csrc/common.h), so that the residual and norm
 * launches cover only the other sets.  Bit-identical results either way.                  */
int omg_hierarchy_level_fused(const omg_hierarchy *h, int level, int *fused);
/* Schedule choices of a level as a bit mask: 1 = fused last set (as above); 2 = prolongation
 * runs as a scatter over the restriction's row patterns (csrc/common.h ROW_SCATTER) instead of
 * a pass over the explicit transpose.  Bit-identical results either way.                   */
#define OMG_LEVEL_FUSED_LAST_SET   1
#define OMG_LEVEL_SCATTER_PROLONG  2
#define OMG_LEVEL_UNION_WALK       16  /* every smoother set of A runs rows_union_kernel (several rows per thread) */
#define OMG_LEVEL_MARCH            32  /* lexicographic Gauss-Seidel runs as one wavefront launch per sweep (march.hip) */
#define OMG_LEVEL_MARCH_SCAN       512 /* ... and that launch is the line-scan kernel (OMG_MARCH_SCAN=1 when the hierarchy was made: 3-D,
                                           at most 255 distinct rows, lines of at most 512 rows): rounding-level differences from
                                           the sequential loop, march.hip scan_gs_kernel */
#define OMG_LEVEL_PLANE            64  /* red-black sweeps of a grid star stencil: each half of a V(>=1, >=1) cycle over this
                                        * level (openmg/__init__.py:201-210 and :214-227) is ONE plane-pipelined launch (plane.hip) */
#define OMG_LEVEL_VAR7             256 /* 7-point grid stencil with per-row coefficients under the 2x2x2 aggregation, red-black:
                                        * each half of the cycle over this level is one launch (var7.hip) */
#define OMG_LEVEL_STENCIL27        128 /* 27-point grid stencil with per-row coefficients under the 2x2x2 aggregation, 8-colour
                                        * Gauss-Seidel (BASELINE configs[4]): the cycle over this level runs the octant-layout
                                        * kernels of stencil27.hip — four launches per sweep, the coefficients streamed once each */
#define OMG_LEVEL_TAIL_FUSED       1024 /* a V(1,1) cycle of the hierarchy's shape runs this level's up pass inside the fused
                                        * tail launch: the 16 x 16 x 16 sine solve + the up passes of the block levels above it
                                        * (OMG_TAIL_FUSE=0|1|2 when the hierarchy is made; plane.hip tail_up_kernel) */
#define OMG_LEVEL_LINE             2048 /* zebra line smoother (OMG_SMOOTH_LINE*; line.hip): two launches per sweep */
int omg_hierarchy_level_flags(const omg_hierarchy *h, int level, int *flags);
/* The axis a hierarchy made with OMG_SMOOTH_LINE* smooths along, by stride (0 = X, the unit-stride axis, 1 = Y, 2 = Z),
 * and the dimension of its grid (2 or 3); *axis = -1 and *dim = 0 for every other hierarchy (and one of a single level). */
int omg_hierarchy_line_axis(const omg_hierarchy *h, int *axis, int *dim);
/* The fused tail launch (OMG_LEVEL_TAIL_FUSED) as it actually ran: out[0] = launches of it put on the hierarchy's stream
 * since the hierarchy was made, by any entry; out[1] = how many of those came from replaying a captured graph.         */
int omg_hierarchy_tail_info(const omg_hierarchy *h, int64_t *out2);
/* Switch the plane-pipelined passes of a hierarchy off (enable = 0) or back on: the cycle then runs set
 * by set (same iterate, bit for bit; the norm's partial sums are associated differently).  A/B only.
 * OMG_PLANE=0 in the environment at creation never builds them.                                      */
int omg_hierarchy_use_plane(omg_hierarchy *h, int enable);
/* The shape of the cycles run on this hierarchy and their over-correction factor.  A cycle entered at level l with
 * shape k smooths, restricts the residual, visits level l + 1 — once for V (and wherever l + 1 is the coarsest level:
 * its direct solve is exact), twice otherwise, the second visit starting from the first one's result with the same
 * right-hand side: F = an F-cycle then a V-cycle, W = two W-cycles —, adds over_correction * R^T e and smooths.
 * Level l, 1 <= l < coarsest, is visited l + 1 times by an F-cycle and 2^l times by a W-cycle.  The factor is applied
 * as the prolongation's weight: every stored entry of R^T times the factor, rounded once to the level's precision; the
 * product with e is then rounded and added as before, and the restriction keeps R.  (OMG_CYCLE_V, 1.0), the default,
 * is the cycle of openmg/__init__.py:151-236.  A factor > 1 repairs the too-stiff Galerkin operators of plain
 * aggregation under F and W; under V the overshoot compounds down the levels and the iteration may diverge.
 * Every entry that runs cycles on the hierarchy obeys the setting (omg_vcycle*, omg_solve, omg_resident_cycle(s),
 * omg_resident_pcg, omg_hierarchy_cycle_dev, the OMG_DTYPE_MIXED entries); the multi-GPU runners are V only.  A call
 * that changes the setting drops the captured graphs; one that repeats it does nothing.  An unknown shape or a factor
 * that is not finite and positive: OMG_ERR_INVALID.                                                   */
#define OMG_CYCLE_V 0
#define OMG_CYCLE_F 1
#define OMG_CYCLE_W 2
int omg_hierarchy_set_cycle(omg_hierarchy *h, int shape, double over_correction);
int omg_hierarchy_get_cycle(const omg_hierarchy *h, int *shape, double *over_correction);
/* Tiling of a level's plane-pipelined passes: out[8] = cells per line, lines per plane, planes, a
 * workgroup's interior cells in x / lines / planes, workgroups, threads per workgroup (all 0 when the
 * level has none).                                                                                   */
int omg_hierarchy_plane_info(const omg_hierarchy *h, int level, int64_t *out8);
/* Rows and stored entries of one smoother set (for byte accounting of per-set launches). */
int omg_hierarchy_set_info(const omg_hierarchy *h, int level, int set, int64_t *rows, int64_t *nnz);
/* How an operator of level l sits in HBM (csrc/common.h "Block-dictionary coding": the device
 * format is a lossless recoding of the caller's CSR, chosen per row block).  op: 0 = A[l],
 * 1 = R[l], 2 = R[l]^T; set: one smoother set of A[l], or -1 for the whole operator.  out[]:
 *   0 rows  1 stored entries  2 row blocks
 *   3 row blocks / 4 rows / 5 entries held as row patterns (one byte per row)
 *   6 entries with a one-byte column code   7 entries with a one-byte value code
 *   8 bytes of the operator one launch over these rows reads from HBM in this format
 *   9 the same for plain int32 CSR: entries * (4 + sizeof value) + 4 * rows
 *  10 row blocks / 11 entries whose values sit block-transposed beside offset-only row patterns
 *     (variable coefficients: the one-thread-per-row kernel reads them coalesced)              */
#define OMG_FORMAT_FIELDS 12
int omg_hierarchy_format_info(const omg_hierarchy *h, int level, int op, int set, int64_t *out);
/* Host-only check of that recoding (needs no GPU): codes the operator exactly as an upload
 * would (one smoother set, dtype as in omg_hierarchy_create_ex), decodes it the way the kernels
 * do and compares every column and every value bit with the input; OMG_ERR_INVALID on any
 * difference.  out[] as above.                                                             */
int omg_format_selftest(const omg_csr *A, int dtype, int64_t *out);

/* replaces: openmg.mgCycle(A, b, level, R, parameters, initial) — openmg/__init__.py:151-236.
 * One V-cycle entered at `level` with pre/post = parameters['preIterations'|'postIterations'].
 * x holds `initial` on entry (zeros for initial=None, :191-192) and uOut on return.
 * *norm (nullable) = ||b - A[level] uOut||_2 (:227), 0 when level is the coarsest (:232). */
int omg_vcycle(omg_hierarchy *h, int level, const double *b, double *x,
               int pre, int post, double *norm);
/* The same cycle with the reference's in-place pre-smoother made explicit (Q2): gaussSeidel writes x[i] of the
 * caller's `initial` (openmg/solvers.py:68) and returns the same object (:75), so after mgCycle the array passed as
 * `initial` holds the PRE-SMOOTHED iterate (openmg/__init__.py:201) while uOut is a new array (:220 / :224).
 * x_in: initial iterate (NULL: zeros, :191-192; nothing is uploaded); x_out: uOut; x_pre (nullable): the iterate
 * after the pre-smoothing sweeps of `level` (equal to x_in when pre = 0).  One call, each vector over PCIe once. */
int omg_vcycle_ex(omg_hierarchy *h, int level, const double *b, const double *x_in, double *x_out, double *x_pre,
                  int pre, int post, double *norm);

/* replaces: the cycle loop of openmg.mgSolve — openmg/__init__.py:112-138.  At least one
 * cycle, then until cycle >= max_cycles (if max_cycles > 0) or norm < threshold (if
 * threshold > 0).  x: initial iterate in, solution out.  The both-off ValueError
 * (:118-119) is raised by the Python caller after the first cycle; here both-off is
 * OMG_ERR_INVALID.                                                                        */
int omg_solve(omg_hierarchy *h, const double *b, double *x, int pre, int post,
              int max_cycles, double threshold, int *cycles_done, double *norm);

/* replaces: openmg.mgCycle(A, b, level, R, parameters, initial) (openmg/__init__.py:151-236) for a caller whose b, initial
 * and uOut are DEVICE arrays (double, natural numbering; e.g. the result of the previous call): omg_vcycle_ex without the
 * PCIe copies — only the norm comes back to the host; the call returns when the outputs are complete.  x_in_dev NULL:
 * zeros (:191-192); x_pre_dev (NULL: not wanted; may be x_in_dev) receives the pre-smoothed iterate (Q2).               */
int omg_vcycle_dev(omg_hierarchy *h, int level, const double *b_dev, const double *x_in_dev, double *x_out_dev,
                   double *x_pre_dev, int pre, int post, double *norm);
/* omg_resident_load / omg_resident_fetch for device arrays (mgSolve for a caller on the GPU: openmg/__init__.py:112-138) */
int omg_resident_load_dev(omg_hierarchy *h, const double *b_dev, const double *x0_dev /* NULL = zeros */);
int omg_resident_fetch_dev(omg_hierarchy *h, double *x_dev);

/* Device-pointer cycle: b_dev, x_dev are level-0 DEVICE vectors in natural numbering, x starts
 * from zero, work is enqueued on hip_stream (NULL = the hierarchy's own) without host sync. */
int omg_hierarchy_cycle_dev(omg_hierarchy *h, const double *b_dev, double *x_dev, int pre, int post,
                            void *hip_stream);

/* Device-resident variants used by bench.py and by repeated mgCycle calls: level-0 b and x
 * live in HBM between calls.                                                             */
int omg_resident_load(omg_hierarchy *h, const double *b, const double *x0 /* NULL = zeros */);
int omg_resident_cycle(omg_hierarchy *h, int pre, int post, double *norm /* NULL = no readback */);
/* n_cycles cycles back to back with EVERY cycle's residual norm computed (openmg/__init__.py:227)
 * and returned in norms[n_cycles]; one host synchronisation at the end.  mgSolve's loop
 * (openmg/__init__.py:132-138) when it stops on a cycle count.  Where the ordering allows it
 * (two colour sets, or Jacobi) the norm of cycle k is finished inside the first launch of cycle
 * k + 1, which forms the same residuals anyway — same bits as n_cycles omg_resident_cycle calls;
 * OMG_NO_PRENORM=1 switches that off.                                                        */
int omg_resident_cycles(omg_hierarchy *h, int pre, int post, int n_cycles, double *norms /* nullable */);
int omg_resident_fetch(omg_hierarchy *h, double *x);
/* Fine-grid SpMV y = A[0] x (tools.flexibleMmult, openmg/tools.py:26) on the resident
 * operator, `reps` back-to-back launches inside one hipEvent bracket; *avg_ms per launch. */
int omg_resident_spmv_time(omg_hierarchy *h, int reps, double *avg_ms);
/* Flexible preconditioned conjugate gradients (FCG(1), Polak-Ribiere) on the resident level 0, one zero-start V-cycle
 * V(pre, post) as the preconditioner per iteration.  Starts from the resident iterate (omg_resident_load[_dev]); stops
 * at the first iteration whose recurrence norm ||r||_2 is below threshold (> 0), or after max_iter (>= 1).  Afterwards
 * the resident iterate is the solution and the resident right-hand side b again (omg_resident_fetch[_dev]; a later
 * omg_resident_cycle continues from it).  *iterations: iterations done; norms[max_iter] (nullable): the recurrence norm
 * of each; *true_norm: ||b - A x||_2 once at the end; *breakdown: 1 when (p, q) <= 0 or a scalar was not finite — the
 * last finite iterate stays resident and the call still returns OMG_OK.  Dots and scalars in double for either dtype;
 * the reductions are deterministic (same bits from run to run, with or without omg_resident_use_graph). */
int omg_resident_pcg(omg_hierarchy *h, int pre, int post, int max_iter, double threshold, int *iterations,
                     double *norms /* nullable */, double *true_norm, int *breakdown);
/* Norms of the resident state without running a cycle (either pointer may be NULL): *rhs_norm = ||b||_2 of the resident
 * right-hand side as it is held — after the null-space projection of omg_resident_load[_dev]; the fp64 outer b of an
 * OMG_DTYPE_MIXED hierarchy —, *residual_norm = ||b - A x||_2 of the resident iterate, A level 0's operator (the fp64
 * outer operator of a mixed hierarchy).  The residual is formed in the level's precision (double on a mixed hierarchy),
 * every sum in double: fixed partial slots and a one-workgroup fold, the same bits from run to run.  Works on every kind
 * of level 0 (a residual needs at least two levels: OMG_ERR_INVALID on a single-level hierarchy) and leaves b, x and the
 * levels' vectors untouched: a cycle, an omg_resident_pcg run or a replayed graph after it has the bits it would have
 * had without it.  A relative stop rule, or "the warm start is already good enough", is decided from these two. */
int omg_resident_norms(omg_hierarchy *h, double *rhs_norm, double *residual_norm);
/* Projection onto earlier solutions (Fischer 1998) for a sequence of right-hand sides on one operator: the hierarchy keeps
 * up to `capacity` vectors X_i with X_i^T A X_j = delta_ij — A level 0's operator as omg_resident_norms applies it —, in
 * the layout and precision of the resident iterate (double on OMG_DTYPE_F64 and OMG_DTYPE_MIXED hierarchies, float on
 * OMG_DTYPE_F32), every sum and scalar in double with the deterministic reductions of omg_resident_pcg.
 * omg_resident_projection allocates capacity + 1 vectors (1 <= capacity <= 64) and clears the set; 0 frees it.  Out of
 * memory: OMG_ERR_ALLOC, and the hierarchy stays usable without a set.  A single-level hierarchy: OMG_ERR_INVALID.  A new
 * hierarchy has no set; omg_hierarchy_update_fine and omg_hierarchy_update_kappa[_spaced] empty it (the vectors are
 * A-orthonormal for the old operator only) and keep the capacity.
 * omg_resident_project, after omg_resident_load[_dev]: the resident iterate becomes sum_i (X_i, b) X_i, b the resident
 * right-hand side (after its null-space projection), accumulated in double with i ascending and rounded once.  *used: the
 * vectors used; with none nothing is launched and the iterate stays what the load made it.  Enqueued only.
 * omg_resident_project_update, after the solve that followed omg_resident_project (a caller whose solve ran no cycle or
 * iteration skips it): a full set is emptied first and d = x, the whole solution; otherwise d = x - sum_i alpha_i X_i with
 * that projection's alphas.  With a null space d loses its mean.  Then w = A d, e0 = (d, w), beta_i = (X_i, w),
 * d -= sum_i beta_i X_i, w = A d once more, s2 = (d, w); d / sqrt(s2) joins the set exactly when s2 is finite, s2 > 0
 * and s2 >= 2^-26 e0 (decided on the device), otherwise the set stays as it was.  *size: the set's size afterwards;
 * *kept: whether d joined.  The resident right-hand side and iterate are not touched.
 * omg_resident_projection_fetch: vector `index` (< size) in the caller's numbering, to the host. */
int omg_resident_projection(omg_hierarchy *h, int capacity);
int omg_resident_project(omg_hierarchy *h, int *used /* nullable */);
int omg_resident_project_update(omg_hierarchy *h, int *size /* nullable */, int *kept /* nullable */);
int omg_resident_projection_fetch(omg_hierarchy *h, int index, double *v);
/* Average milliseconds of one launch, `reps` of each between hipEvents on the hierarchy's stream after a warm-up: the
 * inner products of the set's vectors with the resident right-hand side (what omg_resident_project launches for them:
 * the streaming kernel and its fold), the linear combination behind them (into a scratch vector), and the single inner
 * product of omg_resident_pcg's dot kernel on two vectors of the same length — the yardstick.  Needs a set that holds at
 * least one vector; any pointer may be NULL. */
int omg_resident_projection_time(omg_hierarchy *h, int reps, double *dots_ms, double *dot_ms, double *lincomb_ms);
/* Capture one resident cycle into a hipGraph and replay it on later omg_resident_cycle
 * calls with the same (pre, post).  enable = 0 drops the graph.                          */
int omg_resident_use_graph(omg_hierarchy *h, int enable);

/* Per-kernel timing of level-0 launches with hipEvents on the hierarchy's stream.
 * Classes: 0 smoother set-sweep, 1 residual, 2 restrict, 3 prolong-add, 4 residual+norm,
 * 5 plane-pipelined down pass (sweep + residual + restriction), 6 plane-pipelined up pass
 * (prolongation + sweep + norm).
 * omg_profile_enable(h, mask): bit c of mask switches class c on (-1 = all, 0 = off) and
 * clears the totals; each timed launch costs two hipEventRecords (~10 us of stream gap), so
 * bench.py times only class 1 inside its timed region.  omg_profile_read syncs and returns,
 * per class, launches and total milliseconds since the last omg_profile_enable.           */
#define OMG_PROFILE_CLASSES 7
int omg_profile_enable(omg_hierarchy *h, int mask);
int omg_profile_read(omg_hierarchy *h, int64_t *launches, double *total_ms);

/* ---- single operations on one level of a hierarchy (kernel-level parity tests) ------- */
/* replaces: solvers.smooth(A[l], b, x, iterations) — openmg/solvers.py:28-29; x in place. */
int omg_level_smooth(omg_hierarchy *h, int level, const double *b, double *x, int iterations);
/* replaces: tools.getresidual(b, A[l], x, N) — openmg/tools.py:12-15 (+ norm, __init__.py:227). */
int omg_level_residual(omg_hierarchy *h, int level, const double *b, const double *x,
                       double *r, double *norm /* nullable */);
/* replaces: tools.flexibleMmult(A[level], x) — openmg/tools.py:26 (csr_matvec) — on the operator as the hierarchy
 * holds it: a plane level (constant-coefficient grid stencil, red-black) applies it matrix-free, any other level walks
 * its device format; the same bits either way.                                                                        */
int omg_level_spmv(omg_hierarchy *h, int level, const double *x, double *y);
/* omg_level_spmv for DEVICE arrays (double, the caller's numbering): permuted in and out like omg_hierarchy_cycle_dev, on
 * the hierarchy's stream, through two vectors the hierarchy keeps for this entry alone — the resident right-hand side and
 * iterate stay as they are (a b - A u between omg_resident_load and omg_resident_fetch disturbs nothing).  y_dev may be
 * x_dev.  Returns after the stream has finished.  The same bits as omg_level_spmv.  An OMG_DTYPE_MIXED hierarchy:
 * OMG_ERR_UNSUPPORTED, like omg_hierarchy_cycle_dev. */
int omg_level_spmv_dev(omg_hierarchy *h, int level, const double *x_dev, double *y_dev);

/* replaces: flexibleMmult(R[l], residual) — openmg/__init__.py:210. */
int omg_level_restrict(omg_hierarchy *h, int level, const double *fine, double *coarse);
/* replaces: uApx + flexibleMmult(R[l].transpose(), coarseCorrection) — openmg/__init__.py:214,220,224. */
int omg_level_prolong_add(omg_hierarchy *h, int level, const double *coarse, double *fine_inout);
/* replaces: solvers.coarseSolve(A[-1], b) — openmg/solvers.py:16-26. */
int omg_coarse_solve(omg_hierarchy *h, const double *b, double *x);
/* How the coarsest operator is factored (the reference re-runs SuperLU on every cycle,
 * openmg/solvers.py:23; here once at setup): out[0] = interior blocks P (1 = explicit dense
 * inverse; > 1 = substructuring along the band into P blocks and P - 1 separators), out[1] =
 * unknowns, out[2] = half-bandwidth, out[3] = device bytes one solve reads.                  */
int omg_hierarchy_coarse_info(const omg_hierarchy *h, int64_t *out4);

/* ---- standalone operations ----------------------------------------------------------- */
/* replaces: tools.flexibleMmult(A, x) for sparse A, dense vector x — openmg/tools.py:26. */
int omg_spmv(const omg_csr *A, const double *x, double *y);
/* replaces: tools.getresidual — openmg/tools.py:12-15; *norm nullable. */
int omg_residual(const omg_csr *A, const double *b, const double *x, double *r, double *norm);
/* replaces: solvers.gaussSeidel(A, b, x, iterations, threshold) — openmg/solvers.py:34-75,
 * incl. smoothToThreshold (:31-32).  iterations < 0 = None, threshold < 0 = None; both
 * None = one sweep (:39-40).  The norm test runs before the first sweep and after every
 * sweep (:43-54).  x in place.  *sweeps_done nullable.                                    */
int omg_gauss_seidel(const omg_csr *A, const double *b, double *x, int smoother, double omega,
                     int iterations, double threshold, int *sweeps_done);
/* replaces: solvers.coarseSolve(A, b) for a one-off solve — openmg/solvers.py:16-26. */
int omg_direct_solve(const omg_csr *A, const double *b, double *x);

/* replaces: flexibleMmult(flexibleMmult(R, A), R.T) — openmg/operators.py:184-186.
 * Galerkin triple product on the device.  Two steps because the output size is unknown:
 * omg_rap() computes it and reports the shape, omg_csr_result_fetch() copies it into
 * caller-allocated arrays (columns sorted ascending inside each row) and frees it.       */
int omg_rap(const omg_csr *R, const omg_csr *A, omg_csr_result **out,
            int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
/* replaces: tools.flexibleMmult(X, Y) with both operands sparse — openmg/tools.py:26 (SciPy
 * csr_matmat).  C = X Y on the device; every C(i,j) is accumulated in SciPy's order.      */
int omg_spgemm(const omg_csr *X, const omg_csr *Y, omg_csr_result **out,
               int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
int omg_csr_result_fetch(omg_csr_result *res, int32_t *indptr, int32_t *indices, double *data);
int omg_csr_result_free(omg_csr_result *res);

/* replaces: operators.restriction(shape) — openmg/operators.py:15-89 — built on the device.
 * shape[0..dim-1], dim in 1..3; same index quirks as the reference (second-axis offset is
 * shape[0], third-axis offset shape[0]*shape[1]).  Output arrays are caller-allocated:
 * indptr[n/2^dim + 1], indices[n], data[n] with n = prod(shape) when all extents are even. */
int omg_restriction(int dim, const int64_t *shape, int32_t *indptr, int32_t *indices,
                    double *data, int64_t *n_rows, int64_t *nnz);

/* ---- Semicoarsening: a coarsening factor of 1 or 2 per axis and restriction (no reference counterpart) ----
 * On a grid-aligned anisotropic operator only the strongly coupled axes are coarsened; plain aggregation halves the
 * coupling of a coarsened axis relative to the others, so a few levels down the operator is isotropic and coarsening is
 * full again.  Every shape and factor tuple is in the grid's C order: the LAST axis has unit stride; dim is 2 or 3.
 *
 * omg_restriction_ex: the plain C-order aggregation of the grid `shape` by factors[0..dim-1], weight 1 / prod(factors),
 * ascending columns.  Caller-allocated indptr[n / prod(factors) + 1], indices[n], data[n], n = prod(shape).  A factor other
 * than 1 or 2, factors all 1, or a 2 on an extent that is odd or below 4: OMG_ERR_INVALID.  With all factors 2 on a shape
 * whose first and last extent are equal it is omg_restriction's matrix, bit for bit. */
int omg_restriction_ex(int dim, const int64_t *shape, const int *factors, int32_t *indptr, int32_t *indices, double *data);
/* Per-axis couplings of a grid operator held as CSR: sums3[a] = sum |a_ij| and counts4[a] = the number of the STORED
 * entries whose column offset is +- the stride of axis a of `shape`, counts4[3] = the stored entries at any other non-zero
 * offset (27-point, periodic wrap); a 2-D grid leaves sums3[2] = counts4[2] = 0.  A reduction on the device over fixed
 * slots in a fixed order: two calls give the same bits. */
int omg_axis_couplings(const omg_csr *A, int dim, const int64_t *shape, double *sums3, int64_t *counts4);
/* The rule that picks one level's factors from its couplings — a pure host function, no device: both setup routes call
 * this one statement of it.  An axis is eligible when its extent is even and >= 4; m is the eligible axis with the largest
 * mean sums3 / counts4; every eligible axis a with 2 S_a N_m >= S_m N_a (in double, no division: theta = 1/2, ties
 * coarsen) gets factor 2.  line_axis (an index into shape, or -1): the axis of a line smoother is left out of the maximum
 * whenever another axis is eligible, and is always coarsened when eligible.  factors3 all 1: no axis is eligible, the
 * hierarchy ends at this level.  counts4[3] != 0: OMG_ERR_UNSUPPORTED, `level` in the text. */
int omg_semicoarsen_rule(int dim, const int64_t *shape, const double *sums3, const int64_t *counts4, int line_axis, int level,
                         int *factors3);
/* omg_hierarchy_create_from_fine_opt with factors: n_restrictions * dim entries, restriction after restriction, or NULL =
 * 'auto' (couplings kernel, rule, restriction kernel, Galerkin product per level, all in HBM).  Under 'auto' the hierarchy
 * ends where no axis is eligible, and after the first restriction where the coarse level would have <= min_size rows
 * (min_size <= 0: no such rule) — it may have fewer than n_restrictions + 1 levels; named factors are all used.  The
 * operators are then fetched once and the levels made as omg_hierarchy_create_opt makes them from the same lists (same
 * object, same bits): a level whose restriction is not the full 2^dim aggregation runs the set-by-set row kernels.  The
 * line smoothers: OMG_ERR_UNSUPPORTED (omg_hierarchy_create_opt takes them).  omg_hierarchy_can_update_fine is false. */
int omg_hierarchy_create_from_fine_semi(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, const int *factors,
                                        int64_t min_size, const omg_hierarchy_options *opt, omg_hierarchy **out);
/* factors3[0..dim-1] of restriction `level` of a hierarchy made by omg_hierarchy_create_from_fine_semi (the rest 1); any
 * other hierarchy, or no such restriction: OMG_ERR_INVALID. */
int omg_hierarchy_coarsening(const omg_hierarchy *h, int level, int *factors3);

/* ---- Grids of any extent: an odd extent's last cell is merged (no reference counterpart) ----
 * The entries above halve an axis only where its extent is even.  With odd = OMG_ODD_MERGE an axis of ANY extent e >= 4
 * takes a factor 2: it gets e / 2 (rounded down) coarse cells, coarse cell i holds the fine cells 2i and 2i + 1, and the
 * last one also holds e - 1 when e is odd (an extent of 3 would collapse to 1 and stays).  Every stored entry of R keeps
 * the ONE weight 1 / prod(factors) — also in the rows with 3, 6, 9, 12, 18 or 27 members —, so that R^T 1 is a constant
 * vector and a Galerkin operator keeps the constant null space of its parent (OMG_NULLSPACE_CONSTANT works unchanged).
 * With odd = OMG_ODD_REFUSE every entry below is the entry above it is named after, bit for bit; any other value of odd:
 * OMG_ERR_INVALID. */
#define OMG_ODD_REFUSE 0   /* a factor 2 needs an even extent >= 4 (the entries above) */
#define OMG_ODD_MERGE  1   /* a factor 2 needs an extent >= 4; an odd extent's last aggregate takes three cells */
/* omg_restriction_ex with the flag.  Rows: prod(shape[d] / factors[d]) (rounded down per axis); caller-allocated
 * indptr[rows + 1], indices[n], data[n], n = prod(shape): every fine cell is in exactly one row, members in (d0, d1, d2)
 * order — ascending columns. */
int omg_restriction_ragged(int dim, const int64_t *shape, const int *factors, int odd, int32_t *indptr, int32_t *indices,
                           double *data);
/* omg_semicoarsen_rule with the flag: under OMG_ODD_MERGE an axis is eligible when its extent is >= 4, odd or even;
 * everything else in the rule is unchanged.  A pure host function; both setup routes call this one statement. */
int omg_semicoarsen_rule_ragged(int dim, const int64_t *shape, const double *sums3, const int64_t *counts4, int line_axis, int level,
                                int odd, int *factors3);
/* omg_hierarchy_create_from_fine_semi with the flag (factors NULL = 'auto').  A level whose outgoing restriction has a
 * three-cell aggregate runs the set-by-set row kernels, as a semicoarsened level does; the levels whose restriction is the
 * even 2^dim aggregation qualify for the fused passes as in every hierarchy made from lists.  omg_hierarchy_coarsening
 * reports the factors; omg_hierarchy_can_update_fine is false. */
int omg_hierarchy_create_from_fine_ragged(const omg_csr *A_in, int dim, const int64_t *shape, int n_restrictions, const int *factors,
                                          int64_t min_size, int odd, const omg_hierarchy_options *opt, omg_hierarchy **out);

/* Host-side helper of the mgCycle binding (no reference counterpart, no device involved): mgCycle(A, b, level, R,
 * parameters, initial) — openmg/__init__.py:151 — is handed the operator lists on EVERY call; the binding keeps the
 * device hierarchy between calls and recognises the lists by a checksum of every byte (an operator edited in place
 * must not meet a stale device copy).  64-bit digest of buf[0..bytes), chunks hashed on all host threads.           */
int omg_host_checksum(const void *buf, int64_t bytes, uint64_t *out);

/* ---- multi-GPU: one process per GPU, 1-D slabs, RCCL halo exchange ---------------------------
 * No reference counterpart (the reference is single-threaded): the same
 * mgCycle (openmg/__init__.py:151-236) run on a row-partitioned hierarchy.  Each rank owns a
 * contiguous row range of every level.  A level of one rank is described by:
 *   A      owned rows; columns 0..n_loc-1 are the owned unknowns (local numbering), columns
 *          n_loc..n_loc+n_halo-1 the remote unknowns its rows touch (the halo), grouped by
 *          owning peer in the order of `peers`;
 *   R      restriction to the next level, (coarse owned rows) x (fine owned rows) — slabs
 *          must be cut on aggregate boundaries (ignored on the coarsest level);
 *   keys   smoother set of every owned row, 0 <= key < n_sets, consistent across ranks
 *          (NULL: one set, e.g. Jacobi; ignored on the coarsest level);
 *   peers[n_peers], send_off[n_peers+1], send_idx[send_off[n_peers]] (owned rows, local
 *          numbering, sent to each peer), recv_off[n_peers+1] (slots of the halo region
 *          filled by each peer; recv_off[n_peers] == n_halo).
 * coarse_global is the WHOLE coarsest operator (replicated direct solve); coarse_counts[q] =
 * coarsest rows owned by rank q.                                                           */
typedef struct {
    omg_csr A;
    omg_csr R;
    int64_t n_halo;
    const int32_t *keys;
    int32_t n_sets;
    int32_t n_peers;
    const int32_t *peers;
    const int64_t *send_off;
    const int32_t *send_idx;
    const int64_t *recv_off;
    /* 1: plain sets.  2: sets come in (boundary, interior) pairs of one colour — rows that
     * other ranks need first, the rest second; the halo exchange of a pair then runs on a
     * second stream while the interior rows are still being relaxed.                        */
    int32_t set_group;
    /* Optional, one per (peer) entry: the smoother colour whose values the entry carries
     * (peers[] then repeats a rank once per colour).  After relaxing colour c only entries of
     * group c travel; the exchange after prolongation moves all of them.  NULL: every entry
     * is sent every time.                                                                  */
    const int32_t *entry_group;
} omg_dist_level;

typedef struct omg_dist omg_dist;
typedef struct omg_dist_group omg_dist_group;

int omg_dist_create(int rank, int n_ranks, int n_levels, const omg_dist_level *levels,
                    const omg_csr *coarse_global, const int64_t *coarse_counts,
                    int smoother, double omega, omg_dist **out);
/* Same with the levels stored / computed in `dtype` (OMG_DTYPE_F64 is omg_dist_create); halo
 * messages and the coarse all-gather then travel in that type.  Host vectors stay double.  */
int omg_dist_create_ex(int rank, int n_ranks, int n_levels, const omg_dist_level *levels,
                       const omg_csr *coarse_global, const int64_t *coarse_counts,
                       int smoother, double omega, int dtype, omg_dist **out);
int omg_dist_destroy(omg_dist *d);
/* Replicated tail: below the last distributed level every rank runs `tail` — an ordinary
 * omg_hierarchy whose finest operator is the WHOLE operator of that level — on the gathered
 * right-hand side and keeps its own slice of the correction; no exchange happens down there.
 * Pass coarse_global = NULL to omg_dist_create when a tail will be set.  `tail` is borrowed. */
int omg_dist_set_tail(omg_dist *d, omg_hierarchy *tail);
int omg_dist_set_stream(omg_dist *d, void *hip_stream);
int omg_dist_sync(omg_dist *d);
/* RCCL bootstrap: rank 0 makes a 128-byte id, the host broadcasts it (torch.distributed),
 * every rank connects.  librccl is dlopen'ed on first use.                                */
int omg_rccl_unique_id(void *out128);
int omg_dist_connect(omg_dist *d, const void *unique_id128);
/* Microseconds per grouped ncclSend + ncclRecv of `bytes` to the calling rank itself on a one-rank
 * communicator, each followed by a small kernel, `reps` back to back on one stream (hipEvents): the floor
 * of a halo exchange on this GPU (no link involved) — tools/exchange_probe.py, DESIGN.md section 7. */
int omg_rccl_self_exchange_time(int64_t bytes, int reps, double *avg_us);
/* Number of ranks of the RCCL communicator this rank is connected to (ncclCommCount); 0 before
 * omg_dist_connect.  bench.py prints it (config.rccl_ranks) as evidence that the N-GPU run
 * really is one N-rank communicator.                                                        */
int omg_dist_rccl_ranks(omg_dist *d, int *count);
/* owned part of b and of the initial iterate (NULL = zeros), natural local numbering */
int omg_dist_load(omg_dist *d, const double *b_local, const double *x0_local);
int omg_dist_fetch(omg_dist *d, double *x_local);
/* One V-cycle over all ranks (collective: every rank calls it).  *norm (nullable) = the
 * GLOBAL ||b - A x||_2 (openmg/__init__.py:227).                                          */
int omg_dist_cycle(omg_dist *d, int pre, int post, double *norm);
/* n_cycles cycles with every cycle's GLOBAL norm computed, norms[n_cycles] (nullable) returned at
 * the end — the multi-GPU form of omg_resident_cycles (same deferral of the first colour's share
 * of the norm into the next cycle's first launches, same bits as n_cycles omg_dist_cycle calls). */
int omg_dist_cycles(omg_dist *d, int pre, int post, int n_cycles, double *norms);
/* Per-GPU measurement helpers of a multi-GPU run: `reps` launches of y = A_0 x over this rank's
 * rows in one hipEvent bracket (average ms per launch), and omg_hierarchy_format_info for this
 * rank's operators.                                                                          */
int omg_dist_spmv_time(omg_dist *d, int reps, double *avg_ms);
int omg_dist_format_info(omg_dist *d, int level, int op, int set, int64_t *out);
/* Schedule of a smoothed level of this rank: OMG_LEVEL_SCATTER_PROLONG, 4 = (boundary, interior)
 * set pairs, 8 = the scatter prolongation is split the same way (boundary aggregates first). */
int omg_dist_level_flags(omg_dist *d, int level, int *flags);
/* Loopback group: ALL ranks of a decomposition inside one process on one GPU, halos moved by
 * device-to-device copies.  Same schedule as omg_dist_cycle; used to verify the distributed
 * algorithm where only one GPU is available.                                               */
int omg_dist_group_create(int n, omg_dist **ranks, omg_dist_group **out);
int omg_dist_group_destroy(omg_dist_group *g);
int omg_dist_group_cycle(omg_dist_group *g, int pre, int post, double *norm);
int omg_dist_group_cycles(omg_dist_group *g, int pre, int post, int n_cycles, double *norms);

/* ---- plane-pipelined slabs (csrc/dist.hip, round 3): the multi-GPU cycle of constant-coefficient grid stencils ----
 * A rank owns nz_global / n_ranks planes of every distributed level (halved per level) plus ghost planes; each half of
 * the cycle over a level is the single-GPU plane-pipelined launch on that slab (csrc/plane.hip), the exchanges are
 * ghost PLANES (three of x before a pass, two of the right-hand side / the coarse correction), the level below the
 * slabs is gathered and run replicated (`tail`, an ordinary hierarchy, borrowed).  coef7: seven coefficients per
 * distributed level (-K, -J, -I, diagonal, +I, +J, +K), weight: the aggregation's.  double, V(1,1).  The iterate is
 * bit-identical to the single-GPU cycle for every number of ranks.                                                  */
typedef struct omg_pdist omg_pdist;
typedef struct omg_pdist_group omg_pdist_group;
int omg_pdist_create(int rank, int n_ranks, int nx, int ny, int nz_global, int n_levels, const double *coef7, double weight,
                     omg_pdist **out);
int omg_pdist_destroy(omg_pdist *d);
int omg_pdist_set_tail(omg_pdist *d, omg_hierarchy *tail);
/* two communicators: the cycle's, and one for the exchanges that run on a second stream beside the coarser levels */
int omg_pdist_connect(omg_pdist *d, const void *unique_id128, const void *unique_id128_side);
int omg_pdist_rccl_ranks(omg_pdist *d, int *count);
int omg_pdist_load(omg_pdist *d, const double *b_local, const double *x0_local /* NULL = zeros */);   /* collective */
int omg_pdist_fetch(omg_pdist *d, double *x_local);
int omg_pdist_sync(omg_pdist *d);
/* out8: distributed levels; 1 when the finest level's passes run GATED between neighbours (one launch of inner chunks and
 * flag-gated edge chunks, the exchange beside it: csrc/dist.hip PlaneDist::gate); its tiling (cells per line, lines,
 * planes per chunk), workgroups, threads per workgroup; planes per inner chunk of a gated pass */
int omg_pdist_info(omg_pdist *d, int64_t *out8);
/* gated passes on / off (off at creation unless OMG_PDIST_GATE=1): the caller switches them on after a checked cycle */
int omg_pdist_set_gate(omg_pdist *d, int enable);
/* omg_pdist_trace(1): the stream writes a progress word (pinned host memory) between the phases of a cycle;
 * omg_pdist_progress reads it without synchronising: (cycle << 16) | (level << 8) | phase, phase 1 halo of x, 2 halo of
 * b, 3 down pass, 4 halo of x for the up pass, 5 gather + replicated tail, 6 halo of the correction, 7 up pass —
 * what a rank reports when a collective never completes (bench.py's preflight).                                   */
int omg_pdist_trace(omg_pdist *d, int enable);
int omg_pdist_progress(omg_pdist *d, unsigned *word);
int omg_pdist_cycles(omg_pdist *d, int n_cycles, double *norms /* nullable */);
/* V(pre, post) with pre, post in {0, 1} — the reference's default is V(1, 0), openmg/__init__.py:22-23 — as the passes
 * without their relaxation; over the RCCL exchanges (peer mode and split passes: V(1, 1) only)                      */
int omg_pdist_cycles_ex(omg_pdist *d, int pre, int post, int n_cycles, double *norms /* nullable */);

/* ---- peer mode: the slab exchanges as stores into the neighbours' memory over xGMI peer mappings ------------------
 * (no reference counterpart: openmg is single-process.)  The passes write their boundary planes straight into the
 * neighbours' ghost planes, raise a flag there when all their workgroups are done, and wait for their neighbours'
 * flags before reading a ghost plane: no exchange launches inside a cycle.  Setup: every rank exports
 * omg_pdist_p2p_handle_count() IPC handles of 64 bytes (omg_pdist_p2p_handles), the control plane hands them round,
 * every rank opens every other rank's (omg_pdist_p2p_open; ranks of one process: omg_pdist_p2p_local), then
 * omg_pdist_p2p_enable(mode) — 1: the passes wait themselves (one GPU per rank); 2: one-workgroup wait launches
 * (ranks sharing a GPU); 0: back to RCCL.  Every distributed level needs >= 4 planes per rank.  A wait that gives up
 * (OMG_P2P_SPIN polls, default 2^21) sets bit 0 of omg_pdist_p2p_status and lets the device run on.
 * omg_pdist_cycles_squares: the cycles without the norm's collective — this rank's sums of squared residuals. */
int omg_peer_access(int device, int peer_device, int *can);     /* hipDeviceCanAccessPeer (same device: 1): ask before mapping */
int omg_pdist_p2p_handle_count(omg_pdist *d, int *count);
int omg_pdist_p2p_handles(omg_pdist *d, void *handles64, int capacity);
int omg_pdist_p2p_open(omg_pdist *d, int peer_rank, const void *handles64, int count);
int omg_pdist_p2p_local(omg_pdist *d, omg_pdist *other);
int omg_pdist_p2p_enable(omg_pdist *d, int mode);
int omg_pdist_p2p_status(omg_pdist *d, unsigned *status);
/* Where the exported buffers sit in their allocations (tests, diagnostics).  omg_pdist_p2p_handles refuses, before the
 * first handle, an export whose computed base is not the base of the allocation that contains the buffer, as the
 * runtime reports it; this reports the same comparison.  out4: per buffer, in handle order, four values — the index of
 * its allocation among the exported ones (buffers that share a handle share the index), the byte offset of its first
 * element from the exported base, the allocation's size, and the distance of the exported base from the allocation's
 * base (0: right).  mapped: per rank of the decomposition, how many allocations of it this rank has opened. */
int omg_pdist_p2p_layout(omg_pdist *d, int64_t *out4, int capacity /* buffers */, int *mapped, int mapped_capacity);
int omg_pdist_cycles_squares(omg_pdist *d, int n_cycles, double *squares);                         /* collective */
/* all ranks in one process on one GPU, device copies in place of RCCL (verification) */
int omg_pdist_group_create(int n, omg_pdist **ranks, omg_pdist_group **out);
int omg_pdist_group_destroy(omg_pdist_group *g);
int omg_pdist_group_cycles(omg_pdist_group *g, int n_cycles, double *norms /* nullable */);
int omg_pdist_group_cycles_ex(omg_pdist_group *g, int pre, int post, int n_cycles, double *norms /* nullable */);

/* ---- 27-point slabs (csrc/dist27.hip, round 5): the multi-GPU cycle of 27-point grid stencils with per-row
 * coefficients (BASELINE configs[4]) on the kernels of csrc/stencil27.hip.  (No reference counterpart: openmg is
 * single-process; the cycle is openmg/__init__.py:151-236.)  A rank owns nz_global / n_ranks planes of each of the
 * n_levels distributed levels (halved per level, even on every one) plus one ghost AGGREGATE plane on either side; the
 * sweeps relax colours 0 .. 3 of the upper ghost plane redundantly, so ONE exchange of ghost planes serves a whole
 * 8-colour sweep: per V(p, q) cycle p + q exchanges on the finest level, 1 + p + q on the others, one all-gather above
 * the replicated `tail` (an ordinary hierarchy over the levels below the slabs, borrowed), one all-reduce per batch.
 * A_rows: this rank's rows of the finest operator (its planes, C order) with GLOBAL column indices — every row the full
 * 27-point stencil of its in-grid neighbours, ascending columns; the Galerkin products of the distributed levels are
 * made per rank on the device.  omg_sdist_coarse_*: this rank's rows (global columns) of the operator below the
 * slabs — the control plane gathers them and builds the tail.  dtype: OMG_DTYPE_F64 / OMG_DTYPE_F32 (vectors,
 * coefficients and messages).  The iterate is bit-identical to the single-GPU hierarchy's for every number of ranks
 * (tests/test_gpu_dist27.py). */
typedef struct omg_sdist omg_sdist;
typedef struct omg_sdist_group omg_sdist_group;
int omg_sdist_create(int rank, int n_ranks, int nx, int ny, int nz_global, int n_levels, const omg_csr *A_rows, double weight, int dtype,
                     omg_sdist **out);
int omg_sdist_destroy(omg_sdist *d);
int omg_sdist_coarse_size(omg_sdist *d, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
int omg_sdist_coarse_fetch(omg_sdist *d, int32_t *indptr, int32_t *indices, double *data);
int omg_sdist_set_tail(omg_sdist *d, omg_hierarchy *tail);
/* joins the communicator; collective: also fetches the neighbour's coefficient rows of the ghost planes */
int omg_sdist_connect(omg_sdist *d, const void *unique_id128);
int omg_sdist_rccl_ranks(omg_sdist *d, int *count);
/* out8: nx, ny, owned planes, aggregates per lane, workgroups, waves per workgroup of `level`; distributed levels;
 * halo exchanges the last omg_sdist_cycles call enqueued on this rank */
int omg_sdist_info(omg_sdist *d, int level, int64_t *out8);
int omg_sdist_load(omg_sdist *d, const double *b_local, const double *x0_local /* NULL = zeros */);
int omg_sdist_fetch(omg_sdist *d, double *x_local);
int omg_sdist_sync(omg_sdist *d);
/* n_cycles V(pre, post) cycles (openmg/__init__.py:22-23: the reference's default is V(1, 0)), every cycle's GLOBAL
 * residual norm (:227) computed and returned; collective */
int omg_sdist_cycles(omg_sdist *d, int pre, int post, int n_cycles, double *norms /* nullable */);
/* all ranks in one process on one GPU, device copies in place of RCCL (verification) */
/* Peer mode for the halo exchanges of the 27-point slabs (round 6): stores into the neighbours' ghost planes ordered by
 * flags, in place of the grouped ncclSend / ncclRecv launches — the calls of omg_pdist_p2p_* with 1 + 3 per level handles
 * (flag words, then x / tmp / b of every level); a rank opens its two NEIGHBOURS' only.  The gather below the slabs and the
 * norm's reduction stay on the communicator (omg_sdist_connect).  status bit 0: a bounded wait (OMG_P2P_SPIN polls) gave up. */
int omg_sdist_p2p_handle_count(omg_sdist *d, int *count);
int omg_sdist_p2p_handles(omg_sdist *d, void *handles64, int capacity);
int omg_sdist_p2p_open(omg_sdist *d, int peer_rank, const void *handles64, int count);
int omg_sdist_p2p_local(omg_sdist *d, omg_sdist *other);
int omg_sdist_p2p_enable(omg_sdist *d, int mode /* 0 | 1 */);
int omg_sdist_p2p_status(omg_sdist *d, unsigned *status);
/* as omg_pdist_p2p_layout; mapped2: the allocations opened of rank - 1 and of rank + 1 */
int omg_sdist_p2p_layout(omg_sdist *d, int64_t *out4, int capacity /* buffers */, int *mapped2);
int omg_sdist_group_create(int n, omg_sdist **ranks, omg_sdist_group **out);
int omg_sdist_group_destroy(omg_sdist_group *g);
int omg_sdist_group_cycles(omg_sdist_group *g, int pre, int post, int n_cycles, double *norms /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* OPENMG_HIP_H */
