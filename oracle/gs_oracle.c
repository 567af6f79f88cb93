/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this.
 *
 * Plain-C restatement of the reference's sequential kernels so that the CPU
 * checker finishes in seconds at sizes where the reference's Python loop takes
 * minutes.  Each function names the reference lines it follows
 * (reference = tsbertalan/openmg, mounted at /root/reference in the build container).
 *
 * Build: make -C oracle      ->  oracle/libmg_oracle.so
 */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

/* openmg/solvers.py:56-68 — one or more in-place lexicographic Gauss-Seidel sweeps.
 * Row sum runs over the STORED column order (solvers.py:63-65, np.dot of the row
 * slice with x gathered at the row's indices) and includes the diagonal term;
 * the update is x[i] += (b[i] - sum) / A[i,i] (solvers.py:68).  A[i,i] is the sum of
 * all stored entries of row i whose column is i (SciPy's A[i, i] adds duplicates).
 * Returns 0, or 1+i if row i has no stored diagonal (the reference would divide by 0). */
int oracle_gs_lex(int64_t n, const int32_t *indptr, const int32_t *indices,
                  const double *data, const double *b, double *x, int sweeps)
{
    for (int s = 0; s < sweeps; ++s) {
        for (int64_t i = 0; i < n; ++i) {
            double sum = 0.0, diag = 0.0;
            int have = 0;
            for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p) {
                sum += data[p] * x[indices[p]];
                if (indices[p] == i) { diag += data[p]; have = 1; }
            }
            if (!have) return (int)(1 + i);
            x[i] = x[i] + (b[i] - sum) / diag;
        }
    }
    return 0;
}

/* Same sweep, but rows are visited in the order given by `order` (a permutation of
 * 0..n-1).  With order = "all rows of colour 0, then colour 1, ..." this is
 * multi-colour Gauss-Seidel; it equals oracle_gs_lex applied to the symmetrically
 * permuted system, which is how the real reference pins it (tests/golden g4). */
int oracle_gs_ordered(int64_t n, const int32_t *indptr, const int32_t *indices,
                      const double *data, const double *b, double *x,
                      const int32_t *order, int sweeps)
{
    for (int s = 0; s < sweeps; ++s) {
        for (int64_t k = 0; k < n; ++k) {
            int64_t i = order[k];
            double sum = 0.0, diag = 0.0;
            int have = 0;
            for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p) {
                sum += data[p] * x[indices[p]];
                if (indices[p] == i) { diag += data[p]; have = 1; }
            }
            if (!have) return (int)(1 + i);
            x[i] = x[i] + (b[i] - sum) / diag;
        }
    }
    return 0;
}

/* openmg/tools.py:12-15 + :26 — r = b - A x, row sums in stored order
 * (scipy sparsetools csr_matvec accumulates in stored order too). */
void oracle_residual(int64_t n, const int32_t *indptr, const int32_t *indices,
                     const double *data, const double *b, const double *x, double *r)
{
    for (int64_t i = 0; i < n; ++i) {
        double sum = 0.0;
        for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p)
            sum += data[p] * x[indices[p]];
        r[i] = b[i] - sum;
    }
}

/* y = A x (tools.py:26 -> csr_matvec). */
void oracle_spmv(int64_t n, const int32_t *indptr, const int32_t *indices,
                 const double *data, const double *x, double *y)
{
    for (int64_t i = 0; i < n; ++i) {
        double sum = 0.0;
        for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p)
            sum += data[p] * x[indices[p]];
        y[i] = sum;
    }
}

/* Weighted Jacobi sweep, x_new = x + omega * D^-1 (b - A x).  NOT in the reference
 * (SURVEY D3): parity unpinned by the reference, checked only against this restatement. */
int oracle_jacobi(int64_t n, const int32_t *indptr, const int32_t *indices,
                  const double *data, const double *b, const double *x, double *xnew,
                  double omega)
{
    for (int64_t i = 0; i < n; ++i) {
        double sum = 0.0, diag = 0.0;
        int have = 0;
        for (int32_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            sum += data[p] * x[indices[p]];
            if (indices[p] == i) { diag += data[p]; have = 1; }
        }
        if (!have) return (int)(1 + i);
        xnew[i] = x[i] + omega * ((b[i] - sum) / diag);
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------
 * The row kernels' arithmetic, restated EXACTLY (openmg_amd/csrc/csr_kernels.hip; the rule is
 * written at ASSOC_LEN in common.h).  Unlike the loops above, which multiply and add separately,
 * these use fmaf / fma the way the kernels do, so that a device result can be compared with
 * np.array_equal.  One set of functions per element type: rows_*_f32, rows_*_f64.
 *
 * A row's sum over its STORED entries (duplicates and column order untouched):
 *   - at most ROWS_ASSOC_LEN entries: one fma chain in stored order from +0;
 *   - more: four chains, chain q takes entries q, q+4, ..., added as ((s0+s1)+s2)+s3;
 *   - more than ROWS_BLK_NNZ: the workgroup path (process_block's "one long row" branch): thread
 *     t of 256 chains entries t, t+256, ... in the element type; the partials are widened to
 *     double and added by wave_sum's shuffle tree inside each 64, the four waves are added in
 *     order 0..3 from +0.0, and the total is rounded once to the element type.
 * The diagonal is formed the same way from the entries whose column is the row: plain additions,
 * the entry at position e of the row going to the chain (or thread) its position selects.
 * ------------------------------------------------------------------------------------------- */
#define ROWS_ASSOC_LEN 16
#define ROWS_BLK_NNZ 2048
#define ROWS_THREADS 256

/* wave_sum + block_sum of csr_kernels.hip: lane i adds lane i + off for off = 32, 16, ..., 1
 * (lane 0 holds the wave's total), then the waves' totals are added in order from +0.0. */
static double rows_block_sum(const double *part)
{
    double tot = 0.0;
    for (int w = 0; w < ROWS_THREADS / 64; ++w) {
        double v[64];
        for (int i = 0; i < 64; ++i) v[i] = part[64 * w + i];
        for (int off = 32; off > 0; off >>= 1)
            for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
        tot += v[0];
    }
    return tot;
}

#define ROWS_DEFINE(T, SFX, FMA)                                                                    \
    /* sum and diagonal of row i under the rule above */                                            \
    static void rows_sum_one_##SFX(const int32_t *indptr, const int32_t *indices, const T *data,    \
                                   const T *x, int64_t i, T *sum, T *diag)                          \
    {                                                                                               \
        const int32_t beg = indptr[i], end = indptr[i + 1], len = end - beg;                        \
        if (len > ROWS_BLK_NNZ) {                                                                   \
            double part[ROWS_THREADS], dpart[ROWS_THREADS];                                         \
            for (int t = 0; t < ROWS_THREADS; ++t) {                                                \
                T p = (T)0, d = (T)0;                                                               \
                for (int32_t k = beg + t; k < end; k += ROWS_THREADS) {                             \
                    p = FMA(data[k], x[indices[k]], p);                                             \
                    if (indices[k] == i) d = d + data[k];                                           \
                }                                                                                   \
                part[t] = (double)p;                                                                \
                dpart[t] = (double)d;                                                               \
            }                                                                                       \
            *sum = (T)rows_block_sum(part);                                                         \
            *diag = (T)rows_block_sum(dpart);                                                       \
            return;                                                                                 \
        }                                                                                           \
        const int nch = len > ROWS_ASSOC_LEN ? 4 : 1;                                               \
        T s[4] = {(T)0, (T)0, (T)0, (T)0}, d[4] = {(T)0, (T)0, (T)0, (T)0};                         \
        for (int32_t e = 0; e < len; ++e) {                                                         \
            const int q = nch == 4 ? (e & 3) : 0;                                                   \
            s[q] = FMA(data[beg + e], x[indices[beg + e]], s[q]);                                   \
            if (indices[beg + e] == i) d[q] = d[q] + data[beg + e];                                 \
        }                                                                                           \
        *sum = nch == 4 ? ((s[0] + s[1]) + s[2]) + s[3] : s[0];                                     \
        *diag = nch == 4 ? ((d[0] + d[1]) + d[2]) + d[3] : d[0];                                    \
    }                                                                                               \
    /* every row's sum and diagonal (x has n_cols entries; diag[i] is +0 without a stored one) */   \
    void rows_sum_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices, const T *data,    \
                        const T *x, T *sum, T *diag)                                                \
    {                                                                                               \
        for (int64_t i = 0; i < n; ++i) rows_sum_one_##SFX(indptr, indices, data, x, i, sum + i, diag + i); \
    }                                                                                               \
    /* ROW_SPMV: y = A x */                                                                         \
    void rows_spmv_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices, const T *data,   \
                         const T *x, T *y)                                                          \
    {                                                                                               \
        T d;                                                                                        \
        for (int64_t i = 0; i < n; ++i) rows_sum_one_##SFX(indptr, indices, data, x, i, y + i, &d); \
    }                                                                                               \
    /* ROW_RESIDUAL: r = b - sum */                                                                 \
    void rows_residual_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices,              \
                             const T *data, const T *b, const T *x, T *r)                           \
    {                                                                                               \
        T s, d;                                                                                     \
        for (int64_t i = 0; i < n; ++i) {                                                           \
            rows_sum_one_##SFX(indptr, indices, data, x, i, &s, &d);                                \
            r[i] = b[i] - s;                                                                        \
        }                                                                                           \
    }                                                                                               \
    /* ROW_AXPY: y = y + sum, in place */                                                           \
    void rows_axpy_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices, const T *data,   \
                         const T *x, T *y)                                                          \
    {                                                                                               \
        T s, d;                                                                                     \
        for (int64_t i = 0; i < n; ++i) {                                                           \
            rows_sum_one_##SFX(indptr, indices, data, x, i, &s, &d);                                \
            y[i] = y[i] + s;                                                                        \
        }                                                                                           \
    }                                                                                               \
    /* ROW_GS over the rows in `order`, in place: x_i = x_i + (b_i - sum) / diag.  Returns 0, or    \
     * 1 + i if row i's diagonal is zero. */                                                        \
    int rows_gs_ordered_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices,             \
                              const T *data, const T *b, T *x, const int32_t *order, int sweeps)    \
    {                                                                                               \
        T s, d;                                                                                     \
        for (int it = 0; it < sweeps; ++it)                                                         \
            for (int64_t k = 0; k < n; ++k) {                                                       \
                const int64_t i = order[k];                                                         \
                rows_sum_one_##SFX(indptr, indices, data, x, i, &s, &d);                            \
                if (d == (T)0) return (int)(1 + i);                                                 \
                x[i] = x[i] + (b[i] - s) / d;                                                       \
            }                                                                                       \
        return 0;                                                                                   \
    }                                                                                               \
    /* ROW_JACOBI / ROW_JACOBI_PRENORM: xnew_i = fma(omega, (b_i - sum) / diag, x_i), omega         \
     * rounded to the element type first (make_kargs).  row_result spells the update                \
     * "x + omega * q"; the gfx950 assembly (hipcc -S, the instruction behind each division's       \
     * v_div_fixup) shows the product and the addition contracted to one v_fmac / v_fma in every    \
     * ROW_JACOBI and ROW_JACOBI_PRENORM instantiation of rows_kernel, rows_pattern_kernel and      \
     * rows_union_kernel, in float and in double: all instantiations agree.  rows_serial_kernel is  \
     * instantiated for ROW_GS only, whose epilogue x + (b - sum) / diag has no product to          \
     * contract (v_add behind the v_div_fixup): it has no Jacobi form. */                           \
    int rows_jacobi_##SFX(int64_t n, const int32_t *indptr, const int32_t *indices, const T *data,  \
                          const T *b, const T *x, T *xnew, double omega)                            \
    {                                                                                               \
        const T om = (T)omega;                                                                      \
        T s, d;                                                                                     \
        for (int64_t i = 0; i < n; ++i) {                                                           \
            rows_sum_one_##SFX(indptr, indices, data, x, i, &s, &d);                                \
            if (d == (T)0) return (int)(1 + i);                                                     \
            xnew[i] = FMA(om, (b[i] - s) / d, x[i]);                                                \
        }                                                                                           \
        return 0;                                                                                   \
    }

ROWS_DEFINE(float, f32, fmaf)
ROWS_DEFINE(double, f64, fma)
#undef ROWS_DEFINE
