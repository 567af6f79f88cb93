// Flexible preconditioned conjugate gradients on the finest level of a hierarchy (omg_resident_pcg; hierarchy.hip drives
// it, common.h declares the launchers).  Notay's FCG(1) in the Polak-Ribiere form, one zero-start V-cycle as the
// preconditioner per iteration:
//
//   r = b - A x ; z = M(r) ; p = z ; rho = (r, z)
//   loop:  q = A p ; alpha = rho / (p, q) ; x += alpha p ; r -= alpha q ; stop on ||r||
//          z = M(r) ; beta = -alpha (z, q) / rho ; rho = (r, z) ; p = z + beta p
//
// Every vector is in the level's own numbering (inner products do not depend on the order).  The scalars live on the
// device (PCG_* slots of one double array): every reduction leaves one partial per workgroup in a fixed slot, and a
// one-workgroup fold adds the slots in a fixed order and derives alpha / beta from them — the same bits from run to run,
// no host round trip per iteration, no float atomics.  A fold that meets convergence or a breakdown raises PCG_DONE;
// every kernel here returns at once when it is set, so the iterate stays that of the first converged iteration.
//
// Mixed precision (OMG_DTYPE_MIXED): the same kernels with a second element type Z for what the cycle reads and writes
// — z = M(r) arrives as float, and the update / residual kernels also leave fl32(r) in the cycle's right-hand side —
// while x, r, p, q, b and every scalar stay double.  With Z = V (the fp64 and fp32 hierarchies) they compute what they
// always computed.  The defect-correction kernels at the end (x += z, r = b - A x) serve the mixed plain cycle.
//
// The range of float is not the range of double, so the cycle never sees r itself: it gets fl32(2^-e r) and its z counts
// as 2^e z, with e the exponent of a norm the iteration already has — ||b|| (folded when b was loaded) for the first
// residual, the last residual norm after that (PCG_E_NEXT: what the kernels that write the cycle's right-hand side
// read; PCG_E_USED: the one the right-hand side the cycle last ran on was written with, what the kernels that read z
// use).  No pass over the vectors is added for it, and no host round trip.  Both factors are powers of two, so the bits are those of
// the unscaled iteration wherever no component of fl32(r) was subnormal, and a solve of 2^k b is 2^k times the solve of b.
#include <algorithm>
#include <type_traits>
#include <cmath>

#include "common.h"

namespace omg {
namespace {

constexpr int PCG_WG = 256;

// deterministic sum of the 256 values of a workgroup (fixed tree)
__device__ __forceinline__ double block_sum(double v, double *sh) {
    const int t = int(threadIdx.x);
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = PCG_WG / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// element chunks of 16 bytes (VW values) where every pointer is 16-byte aligned, single values otherwise
template <typename V, int VW>
struct Chunk {
    V v[VW];
};
template <typename V, int VW>
__device__ __forceinline__ Chunk<V, VW> ld(const V *p, int64_t c) {
    return reinterpret_cast<const Chunk<V, VW> *>(p)[c];
}
template <typename V, int VW>
__device__ __forceinline__ void st(V *p, int64_t c, const Chunk<V, VW> &v) {
    reinterpret_cast<Chunk<V, VW> *>(p)[c] = v;
}

__device__ __forceinline__ bool pcg_done(const double *sc) { return sc[PCG_DONE] != 0.0; }

// the mixed iteration's power-of-two factors (Z != V only; 1 otherwise, and the compiler drops the product)
template <bool LO>
__device__ __forceinline__ double scale_up(const double *sc) { return LO ? ldexp(1.0, int(sc[PCG_E_USED])) : 1.0; }
template <bool LO>
__device__ __forceinline__ double scale_down(const double *sc) { return LO ? ldexp(1.0, -int(sc[PCG_E_NEXT])) : 1.0; }
// the exponent a residual norm gives (0 for a norm that is zero or not finite); within +-1000 so that 2^-e is normal
__device__ __forceinline__ double scale_exponent(double norm) {
    if (!(norm > 0.0) || !std::isfinite(norm)) return 0.0;
    return double(min(1000, max(-1000, ilogb(norm))));
}

// (r, z) -> part[wg], (z, q) -> part[nwg + wg]
template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void dots_kernel(const V *__restrict__ r, const Z *__restrict__ z, const V *__restrict__ q,
                                                      int64_t n, double *__restrict__ part, const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const double up = scale_up<LO>(sc);
    auto zv = [&](Z v) -> double { return LO ? double(v) * up : double(v); };
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    double rz = 0.0, zq = 0.0;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<V, VW> a = ld<V, VW>(r, c), d = ld<V, VW>(q, c);
        const Chunk<Z, VW> b = ld<Z, VW>(z, c);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            rz = fma(double(a.v[e]), zv(b.v[e]), rz);
            zq = fma(zv(b.v[e]), double(d.v[e]), zq);
        }
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) {
            rz = fma(double(r[i]), zv(z[i]), rz);
            zq = fma(zv(z[i]), double(q[i]), zq);
        }
    rz = block_sum(rz, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = rz;
    __syncthreads();
    zq = block_sum(zq, sh);
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = zq;
}

// (a, b) -> part[wg]
template <typename V, int VW>
__global__ __launch_bounds__(PCG_WG) void dot_kernel(const V *__restrict__ a, const V *__restrict__ b, int64_t n,
                                                     double *__restrict__ part, const double *__restrict__ sc) {
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    double s = 0.0;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<V, VW> u = ld<V, VW>(a, c), w = ld<V, VW>(b, c);
#pragma unroll
        for (int e = 0; e < VW; ++e) s = fma(double(u.v[e]), double(w.v[e]), s);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) s = fma(double(a[i]), double(b[i]), s);
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// p2 = z + beta p
template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void pupdate_kernel(const Z *__restrict__ z, const V *__restrict__ p, V *__restrict__ p2,
                                                         int64_t n, const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    if (pcg_done(sc)) return;
    const double beta = sc[PCG_BETA];
    const double up = scale_up<LO>(sc);
    auto zv = [&](Z v) -> double { return LO ? double(v) * up : double(v); };
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<Z, VW> u = ld<Z, VW>(z, c);
        const Chunk<V, VW> w = ld<V, VW>(p, c);
        Chunk<V, VW> o;
#pragma unroll
        for (int e = 0; e < VW; ++e) o.v[e] = V(fma(beta, double(w.v[e]), zv(u.v[e])));
        st<V, VW>(p2, c, o);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) p2[i] = V(fma(beta, double(p[i]), zv(z[i])));
}

// x += alpha p ; r -= alpha q ; ||r||^2 -> part[wg]; Z != V: also rlo = fl32(2^-e r), the cycle's right-hand side
template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void update_kernel(V *__restrict__ x, const V *__restrict__ p, V *__restrict__ r,
                                                        const V *__restrict__ q, Z *__restrict__ rlo, int64_t n,
                                                        double *__restrict__ part, const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const double alpha = sc[PCG_ALPHA];
    const double down = scale_down<LO>(sc);
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    double rr = 0.0;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        Chunk<V, VW> xv = ld<V, VW>(x, c), rv = ld<V, VW>(r, c);
        const Chunk<V, VW> pv = ld<V, VW>(p, c), qv = ld<V, VW>(q, c);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            xv.v[e] = V(fma(alpha, double(pv.v[e]), double(xv.v[e])));
            rv.v[e] = V(fma(-alpha, double(qv.v[e]), double(rv.v[e])));
            rr = fma(double(rv.v[e]), double(rv.v[e]), rr);
        }
        st<V, VW>(x, c, xv);
        st<V, VW>(r, c, rv);
        if constexpr (LO) {
            Chunk<Z, VW> lo;
#pragma unroll
            for (int e = 0; e < VW; ++e) lo.v[e] = Z(double(rv.v[e]) * down);
            st<Z, VW>(rlo, c, lo);
        }
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) {
            x[i] = V(fma(alpha, double(p[i]), double(x[i])));
            r[i] = V(fma(-alpha, double(q[i]), double(r[i])));
            rr = fma(double(r[i]), double(r[i]), rr);
            if constexpr (LO) rlo[i] = Z(double(r[i]) * down);
        }
    rr = block_sum(rr, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = rr;
}

// r = b - q (r nullable) ; ||b - q||^2 -> part[wg].  Not gated by PCG_DONE (the set-up and the final true residual).
// Z != V: also rlo = fl32(2^-e (b - q)) (nullable; sc is read only then)
template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void residual_kernel(const V *__restrict__ b, const V *__restrict__ q, V *__restrict__ r,
                                                          Z *__restrict__ rlo, int64_t n, double *__restrict__ part,
                                                          const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    __shared__ double sh[PCG_WG];
    double down = 1.0;
    if constexpr (LO) { if (rlo) down = scale_down<LO>(sc); }
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    double rr = 0.0;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<V, VW> bv = ld<V, VW>(b, c), qv = ld<V, VW>(q, c);
        Chunk<V, VW> o;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            o.v[e] = bv.v[e] - qv.v[e];
            rr = fma(double(o.v[e]), double(o.v[e]), rr);
        }
        if (r) st<V, VW>(r, c, o);
        if constexpr (LO) {
            if (rlo) {
                Chunk<Z, VW> lo;
#pragma unroll
                for (int e = 0; e < VW; ++e) lo.v[e] = Z(double(o.v[e]) * down);
                st<Z, VW>(rlo, c, lo);
            }
        }
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) {
            const V o = b[i] - q[i];
            if (r) r[i] = o;
            if constexpr (LO) { if (rlo) rlo[i] = Z(double(o) * down); }
            rr = fma(double(o), double(o), rr);
        }
    rr = block_sum(rr, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = rr;
}

// p2 = z + beta p, q = A p2 and (p2, q) -> part[wg] on a plane level: the constant-coefficient 7-point operator in the
// plane passes' red-black layout (plane.hip: cell (i, j, k) of colour c = (i + j + k) & 1 sits at slot
// c nr + k ny hx + j hx + i / 2).  One output slot per thread; the neighbours' p2 (all of the other colour) is formed from
// their z and p again, so p2 goes to a buffer of its own.  Each row is the row kernels' fma chain in column order from +0
// (-K, -J, -I, diagonal, +I, +J, +K); a neighbour outside the grid contributes c * 0.
template <typename V, typename Z>
__global__ __launch_bounds__(PCG_WG) void plane_step_kernel(const Z *__restrict__ z, const V *__restrict__ p, V *__restrict__ p2,
                                                            V *__restrict__ q, PcgPlane g, double *__restrict__ part,
                                                            const double *__restrict__ sc) {
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const V beta = V(sc[PCG_BETA]);
    const V c0 = V(g.c[0]), c1 = V(g.c[1]), c2 = V(g.c[2]), c3 = V(g.c[3]), c4 = V(g.c[4]), c5 = V(g.c[5]), c6 = V(g.c[6]);
    const int64_t ps = int64_t(g.ny) * g.hx, n = 2 * g.nr, stride = int64_t(gridDim.x) * PCG_WG;
    constexpr bool LO = !std::is_same<V, Z>::value;
    const double up = scale_up<LO>(sc);
    auto pv = [&](int64_t s) -> V { return V(fma(double(beta), double(p[s]), LO ? double(z[s]) * up : double(z[s]))); };
    double pq = 0.0;
    for (int64_t s = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; s < n; s += stride) {
        const int colour = s >= g.nr ? 1 : 0;
        const int64_t u = s - (colour ? g.nr : 0);
        const int k = int(u / ps);
        const int64_t rem = u - int64_t(k) * ps;
        const int j = int(rem / g.hx), h = int(rem - int64_t(j) * g.hx);
        const int par = (j + k) & 1;
        const int i = 2 * h + (colour ? 1 - par : par);
        const int64_t ob = colour ? 0 : g.nr;                         // the other colour's first slot
        const int64_t line = ob + int64_t(k) * ps + int64_t(j) * g.hx;
        const V km = k > 0 ? pv(line - ps + (i >> 1)) : V(0);
        const V jm = j > 0 ? pv(line - g.hx + (i >> 1)) : V(0);
        const V im = i > 0 ? pv(line + ((i - 1) >> 1)) : V(0);
        const V d = pv(s);
        const V ip = i + 1 < g.nx ? pv(line + ((i + 1) >> 1)) : V(0);
        const V jp = j + 1 < g.ny ? pv(line + g.hx + (i >> 1)) : V(0);
        const V kp = k + 1 < g.nz ? pv(line + ps + (i >> 1)) : V(0);
        V a = fma(c0, km, V(0));
        a = fma(c1, jm, a);
        a = fma(c2, im, a);
        a = fma(c3, d, a);
        a = fma(c4, ip, a);
        a = fma(c5, jp, a);
        a = fma(c6, kp, a);
        p2[s] = d;
        q[s] = a;
        pq = fma(double(d), double(a), pq);
    }
    pq = block_sum(pq, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = pq;
}

// ---- defect correction of the mixed plain cycle: x' = x + z, r = b - A x', fl32(r) for the next cycle, ||r||^2 ----------

// x += 2^e z (any level); the fp64 SpMV and residual_kernel follow
template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void defect_add_kernel(V *__restrict__ x, const Z *__restrict__ z, int64_t n,
                                                            const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    const V up = V(scale_up<LO>(sc));
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        Chunk<V, VW> xv = ld<V, VW>(x, c);
        const Chunk<Z, VW> zv = ld<Z, VW>(z, c);
#pragma unroll
        for (int e = 0; e < VW; ++e) xv.v[e] = xv.v[e] + (LO ? V(zv.v[e]) * up : V(zv.v[e]));
        st<V, VW>(x, c, xv);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) x[i] = x[i] + (LO ? V(z[i]) * up : V(z[i]));
}

// On a plane level (the layout of plane_step_kernel): x2 = x + z, r = b - A x2 with the neighbours' x2 formed again from their
// x and 2^e z (so x2 is a buffer of its own), rlo = fl32(2^-e' r), ||r||^2 -> part[wg].  A x2 is plane_step_kernel's fma chain.
template <typename V, typename Z>
__global__ __launch_bounds__(PCG_WG) void defect_plane_kernel(const V *__restrict__ x, const Z *__restrict__ z, V *__restrict__ x2,
                                                              const V *__restrict__ b, Z *__restrict__ rlo, PcgPlane g,
                                                              double *__restrict__ part, const double *__restrict__ sc) {
    constexpr bool LO = !std::is_same<V, Z>::value;
    __shared__ double sh[PCG_WG];
    const V up = V(scale_up<LO>(sc));
    const double down = scale_down<LO>(sc);
    const V c0 = V(g.c[0]), c1 = V(g.c[1]), c2 = V(g.c[2]), c3 = V(g.c[3]), c4 = V(g.c[4]), c5 = V(g.c[5]), c6 = V(g.c[6]);
    const int64_t ps = int64_t(g.ny) * g.hx, n = 2 * g.nr, stride = int64_t(gridDim.x) * PCG_WG;
    auto xv = [&](int64_t s) -> V { return x[s] + (LO ? V(z[s]) * up : V(z[s])); };
    double rr = 0.0;
    for (int64_t s = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; s < n; s += stride) {
        const int colour = s >= g.nr ? 1 : 0;
        const int64_t u = s - (colour ? g.nr : 0);
        const int k = int(u / ps);
        const int64_t rem = u - int64_t(k) * ps;
        const int j = int(rem / g.hx), h = int(rem - int64_t(j) * g.hx);
        const int par = (j + k) & 1;
        const int i = 2 * h + (colour ? 1 - par : par);
        const int64_t ob = colour ? 0 : g.nr;
        const int64_t line = ob + int64_t(k) * ps + int64_t(j) * g.hx;
        const V km = k > 0 ? xv(line - ps + (i >> 1)) : V(0);
        const V jm = j > 0 ? xv(line - g.hx + (i >> 1)) : V(0);
        const V im = i > 0 ? xv(line + ((i - 1) >> 1)) : V(0);
        const V d = xv(s);
        const V ip = i + 1 < g.nx ? xv(line + ((i + 1) >> 1)) : V(0);
        const V jp = j + 1 < g.ny ? xv(line + g.hx + (i >> 1)) : V(0);
        const V kp = k + 1 < g.nz ? xv(line + ps + (i >> 1)) : V(0);
        V a = fma(c0, km, V(0));
        a = fma(c1, jm, a);
        a = fma(c2, im, a);
        a = fma(c3, d, a);
        a = fma(c4, ip, a);
        a = fma(c5, jp, a);
        a = fma(c6, kp, a);
        const V r = b[s] - a;
        x2[s] = d;
        rlo[s] = Z(LO ? double(r) * down : double(r));
        rr = fma(double(r), double(r), rr);
    }
    rr = block_sum(rr, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = rr;
}

// One workgroup: thread t adds slots t, t + 256, ... in order, then the fixed tree.
__device__ __forceinline__ double fold(const double *part, int nwg, double *sh) {
    double a = 0.0;
    for (int i = int(threadIdx.x); i < nwg; i += PCG_WG) a += part[i];
    return block_sum(a, sh);
}

__device__ __forceinline__ void pcg_break(double *sc) {
    sc[PCG_BREAK] = 1.0;
    sc[PCG_DONE] = 1.0;
}

// rho_new = (r, z); beta = -alpha (z, q) / rho_old (0 in the first iteration)
__global__ __launch_bounds__(PCG_WG) void fold_beta_kernel(const double *__restrict__ part, int nwg, double *__restrict__ sc, int first) {
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const double rz = fold(part, nwg, sh);
    __syncthreads();
    const double zq = fold(part + nwg, nwg, sh);
    if (threadIdx.x != 0) return;
    const double beta = first ? 0.0 : -sc[PCG_ALPHA] * zq / sc[PCG_RHO];
    if (!std::isfinite(rz) || !std::isfinite(beta)) { pcg_break(sc); return; }
    sc[PCG_BETA] = beta;
    sc[PCG_RHO] = rz;
}

// alpha = rho / (p, q); (p, q) <= 0 or anything not finite: breakdown
__global__ __launch_bounds__(PCG_WG) void fold_alpha_kernel(const double *__restrict__ part, int nwg, double *__restrict__ sc) {
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const double pq = fold(part, nwg, sh);
    if (threadIdx.x != 0) return;
    const double alpha = sc[PCG_RHO] / pq;
    if (!(pq > 0.0) || !std::isfinite(pq) || !std::isfinite(alpha)) { pcg_break(sc); return; }
    sc[PCG_ALPHA] = alpha;
}

// ||r|| of iteration k -> norms[k]; PCG_ITERS = k + 1; done when below the threshold (> 0)
__global__ __launch_bounds__(PCG_WG) void fold_norm_kernel(const double *__restrict__ part, int nwg, double *__restrict__ sc,
                                                           double *__restrict__ norms, int k, double threshold) {
    __shared__ double sh[PCG_WG];
    if (pcg_done(sc)) return;
    const double nr = sqrt(fold(part, nwg, sh));
    if (threadIdx.x != 0) return;
    norms[k] = nr;
    sc[PCG_ITERS] = double(k + 1);
    sc[PCG_E_USED] = sc[PCG_E_NEXT];       // (the update that just ran wrote the cycle's right-hand side with it)
    sc[PCG_E_NEXT] = scale_exponent(nr);
    if (!std::isfinite(nr)) pcg_break(sc);
    else if (threshold > 0.0 && nr < threshold) sc[PCG_DONE] = 1.0;
}

// sc (nullable): the mixed iteration's exponents move on as in fold_norm_kernel; first: both are this norm's
__global__ __launch_bounds__(PCG_WG) void fold_sqrt_kernel(const double *__restrict__ part, int nwg, double *__restrict__ out,
                                                           double *__restrict__ sc, int first) {
    __shared__ double sh[PCG_WG];
    const double s = fold(part, nwg, sh);
    if (threadIdx.x != 0) return;
    const double nr = sqrt(s);
    if (out) *out = nr;
    if (sc) {
        const double e = scale_exponent(nr);
        sc[PCG_E_USED] = first ? e : sc[PCG_E_NEXT];
        sc[PCG_E_NEXT] = e;
    }
}

// The start of a mixed iteration.  The first residual went to the cycle's right-hand side with the exponent of ||b||
// (known since the load), in the pass that formed it.  That is the right size for a start from zero and for any start
// within 2^60 of it either way; only for another one (a warm start far off, b = 0) do both exponents become that of
// ||r0|| itself, and PCG_RELOWER makes lower_kernel write fl32(2^-e (b - q)) once more.
constexpr double PCG_E_WINDOW = 60.0;
__global__ __launch_bounds__(PCG_WG) void fold_start_kernel(const double *__restrict__ part, int nwg, double *__restrict__ sc) {
    __shared__ double sh[PCG_WG];
    const double s = fold(part, nwg, sh);
    if (threadIdx.x != 0) return;
    const double e = scale_exponent(sqrt(s));
    if (fabs(e - sc[PCG_E_NEXT]) > PCG_E_WINDOW) {
        sc[PCG_E_USED] = e;
        sc[PCG_E_NEXT] = e;
        sc[PCG_RELOWER] = 1.0;
    }
}

template <typename V, typename Z, int VW>
__global__ __launch_bounds__(PCG_WG) void lower_kernel(const V *__restrict__ b, const V *__restrict__ q, Z *__restrict__ rlo,
                                                       int64_t n, const double *__restrict__ sc) {
    if (sc[PCG_RELOWER] == 0.0) return;
    const double down = scale_down<true>(sc);
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PCG_WG;
    for (int64_t c = int64_t(blockIdx.x) * PCG_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<V, VW> bv = ld<V, VW>(b, c), qv = ld<V, VW>(q, c);
        Chunk<Z, VW> lo;
#pragma unroll
        for (int e = 0; e < VW; ++e) lo.v[e] = Z(double(bv.v[e] - qv.v[e]) * down);
        st<Z, VW>(rlo, c, lo);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PCG_WG) rlo[i] = Z(double(b[i] - q[i]) * down);
}

template <typename V>
constexpr int vec_width() { return int(16 / sizeof(V)); }

bool aligned16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15u) == 0; }

}  // namespace

template <typename V>
int pcg_wgs(int64_t n) {
    const int64_t chunks = (n + vec_width<V>() - 1) / vec_width<V>();
    return int(std::max<int64_t>(1, std::min<int64_t>(PCG_MAX_WG, (chunks + PCG_WG - 1) / PCG_WG)));
}

// (each launcher picks the 16-byte form when every vector it touches is 16-byte aligned: the same sums either way
// only up to the order inside a thread, so the choice is made from the pointers alone and repeats from run to run)
#define PCG_LAUNCH(kern, ok, ...)                                                                                           \
    do {                                                                                                                \
        const int nwg_ = pcg_wgs<V>(n);                                                                                 \
        if (ok) hipLaunchKernelGGL((kern<V, Z, vec_width<V>()>), dim3(unsigned(nwg_)), dim3(PCG_WG), 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL((kern<V, Z, 1>), dim3(unsigned(nwg_)), dim3(PCG_WG), 0, s, __VA_ARGS__);                 \
        OMG_HIP(hipGetLastError());                                                                                     \
    } while (0)

template <typename V, typename Z>
void pcg_dots(const V *r, const Z *z, const V *q, int64_t n, double *part, const double *sc, hipStream_t s) {
    PCG_LAUNCH(dots_kernel, aligned16(r) && aligned16(z) && aligned16(q), r, z, q, n, part, sc);
}
template <typename V>
void pcg_dot(const V *a, const V *b, int64_t n, double *part, const double *sc, hipStream_t s) {
    const int nwg = pcg_wgs<V>(n);
    if (aligned16(a) && aligned16(b)) hipLaunchKernelGGL((dot_kernel<V, vec_width<V>()>), dim3(unsigned(nwg)), dim3(PCG_WG), 0, s, a, b, n, part, sc);
    else hipLaunchKernelGGL((dot_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PCG_WG), 0, s, a, b, n, part, sc);
    OMG_HIP(hipGetLastError());
}
template <typename V, typename Z>
void pcg_pupdate(const Z *z, const V *p, V *p2, int64_t n, const double *sc, hipStream_t s) {
    PCG_LAUNCH(pupdate_kernel, aligned16(z) && aligned16(p) && aligned16(p2), z, p, p2, n, sc);
}
template <typename V, typename Z>
void pcg_update(V *x, const V *p, V *r, const V *q, Z *rlo, int64_t n, double *part, const double *sc, hipStream_t s) {
    PCG_LAUNCH(update_kernel, aligned16(x) && aligned16(p) && aligned16(r) && aligned16(q) && aligned16(rlo), x, p, r, q, rlo, n, part, sc);
}
template <typename V, typename Z>
void pcg_residual(const V *b, const V *q, V *r, Z *rlo, int64_t n, double *part, const double *sc, hipStream_t s) {
    PCG_LAUNCH(residual_kernel, aligned16(b) && aligned16(q) && aligned16(r) && aligned16(rlo), b, q, r, rlo, n, part, sc);
}
template <typename V, typename Z>
void pcg_defect_add(V *x, const Z *z, int64_t n, const double *sc, hipStream_t s) {
    PCG_LAUNCH(defect_add_kernel, aligned16(x) && aligned16(z), x, z, n, sc);
}
template <typename V, typename Z>
void pcg_lower(const V *b, const V *q, Z *rlo, int64_t n, const double *sc, hipStream_t s) {
    PCG_LAUNCH(lower_kernel, aligned16(b) && aligned16(q) && aligned16(rlo), b, q, rlo, n, sc);
}
#undef PCG_LAUNCH

template <typename V, typename Z>
int pcg_plane_step(const PcgPlane &g, const Z *z, const V *p, V *p2, V *q, double *part, const double *sc, hipStream_t s) {
    const int64_t n = 2 * g.nr;
    const int nwg = int(std::max<int64_t>(1, std::min<int64_t>(PCG_MAX_WG, (n + PCG_WG - 1) / PCG_WG)));
    hipLaunchKernelGGL((plane_step_kernel<V, Z>), dim3(unsigned(nwg)), dim3(PCG_WG), 0, s, z, p, p2, q, g, part, sc);
    OMG_HIP(hipGetLastError());
    return nwg;
}

template <typename V, typename Z>
int pcg_defect_plane(const PcgPlane &g, const V *x, const Z *z, V *x2, const V *b, Z *rlo, double *part, const double *sc,
                     hipStream_t s) {
    const int64_t n = 2 * g.nr;
    const int nwg = int(std::max<int64_t>(1, std::min<int64_t>(PCG_MAX_WG, (n + PCG_WG - 1) / PCG_WG)));
    hipLaunchKernelGGL((defect_plane_kernel<V, Z>), dim3(unsigned(nwg)), dim3(PCG_WG), 0, s, x, z, x2, b, rlo, g, part, sc);
    OMG_HIP(hipGetLastError());
    return nwg;
}

void pcg_fold_beta(const double *part, int nwg, double *sc, bool first, hipStream_t s) {
    hipLaunchKernelGGL(fold_beta_kernel, dim3(1), dim3(PCG_WG), 0, s, part, nwg, sc, first ? 1 : 0);
    OMG_HIP(hipGetLastError());
}
void pcg_fold_alpha(const double *part, int nwg, double *sc, hipStream_t s) {
    hipLaunchKernelGGL(fold_alpha_kernel, dim3(1), dim3(PCG_WG), 0, s, part, nwg, sc);
    OMG_HIP(hipGetLastError());
}
void pcg_fold_norm(const double *part, int nwg, double *sc, double *norms, int k, double threshold, hipStream_t s) {
    hipLaunchKernelGGL(fold_norm_kernel, dim3(1), dim3(PCG_WG), 0, s, part, nwg, sc, norms, k, threshold);
    OMG_HIP(hipGetLastError());
}
void pcg_fold_start(const double *part, int nwg, double *sc, hipStream_t s) {
    hipLaunchKernelGGL(fold_start_kernel, dim3(1), dim3(PCG_WG), 0, s, part, nwg, sc);
    OMG_HIP(hipGetLastError());
}
void pcg_fold_sqrt(const double *part, int nwg, double *out, hipStream_t s, double *sc, bool first) {
    hipLaunchKernelGGL(fold_sqrt_kernel, dim3(1), dim3(PCG_WG), 0, s, part, nwg, out, sc, first ? 1 : 0);
    OMG_HIP(hipGetLastError());
}

#define PCG_INST(V, Z)                                                                                                  \
    template void pcg_dots<V, Z>(const V *, const Z *, const V *, int64_t, double *, const double *, hipStream_t);       \
    template void pcg_pupdate<V, Z>(const Z *, const V *, V *, int64_t, const double *, hipStream_t);                    \
    template void pcg_update<V, Z>(V *, const V *, V *, const V *, Z *, int64_t, double *, const double *, hipStream_t); \
    template void pcg_residual<V, Z>(const V *, const V *, V *, Z *, int64_t, double *, const double *, hipStream_t);    \
    template int pcg_plane_step<V, Z>(const PcgPlane &, const Z *, const V *, V *, V *, double *, const double *, hipStream_t);   \
    template void pcg_defect_add<V, Z>(V *, const Z *, int64_t, const double *, hipStream_t);                            \
    template int pcg_defect_plane<V, Z>(const PcgPlane &, const V *, const Z *, V *, const V *, Z *, double *, const double *, hipStream_t);
PCG_INST(double, double)
PCG_INST(float, float)
PCG_INST(double, float)
#undef PCG_INST
template void pcg_lower<double, float>(const double *, const double *, float *, int64_t, const double *, hipStream_t);
template int pcg_wgs<double>(int64_t);
template int pcg_wgs<float>(int64_t);
template void pcg_dot<double>(const double *, const double *, int64_t, double *, const double *, hipStream_t);
template void pcg_dot<float>(const float *, const float *, int64_t, double *, const double *, hipStream_t);

}  // namespace omg
