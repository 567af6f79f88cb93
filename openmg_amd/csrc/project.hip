// Projection onto earlier solutions (Fischer 1998; hierarchy.hip omg_resident_project[_update] drives it, common.h
// declares the launchers): the inner products of one vector with up to PROJECTION_MAX others, linear combinations of them
// with coefficients that live on the device, and the gated normalisation of a new direction.  The vectors X_0 ... X_{m-1}
// lie `stride` values apart in one allocation, in the layout and precision of the resident iterate; every sum and every
// scalar is a double.
//
// The inner products follow pcg.hip's reductions: every workgroup of a grid-stride launch (at most PROJECT_MAX_WG) leaves
// one partial per vector in that vector's own row of slots, then one workgroup per vector adds its row in a fixed order — no
// atomics, the same bits from run to run.  The vectors are taken in compile-time groups of DOT_GROUP so that a group's
// accumulators and its loads in flight are registers (no scratch: DESIGN.md §5u has the resource table); v is read once per
// group, every X_i once.  16-byte accesses where every vector is 16-byte aligned, single values for the tail (and for the
// whole vector otherwise); n values of each vector are touched, never a value behind them.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace omg {
namespace {

constexpr int PJ_WG = 256;
constexpr int DOT_GROUP = 8;

// deterministic sum of the 256 values of a workgroup (fixed tree)
__device__ __forceinline__ double block_sum(double v, double *sh) {
    const int t = int(threadIdx.x);
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = PJ_WG / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

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

// (X_i, v) for the M vectors at X -> part[i * PROJECT_MAX_WG + wg]
template <typename V, int VW, int M>
__device__ __forceinline__ void dot_group(const V *__restrict__ X, int64_t stride, const V *__restrict__ v, int64_t n,
                                          double *__restrict__ part, double *sh) {
    double acc[M];
#pragma unroll
    for (int i = 0; i < M; ++i) acc[i] = 0.0;
    const int64_t nc = n / VW, step = int64_t(gridDim.x) * PJ_WG;
    for (int64_t c = int64_t(blockIdx.x) * PJ_WG + threadIdx.x; c < nc; c += step) {
        const Chunk<V, VW> w = ld<V, VW>(v, c);
        Chunk<V, VW> x[M];
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = ld<V, VW>(X + int64_t(i) * stride, c);
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[i] = fma(double(x[i].v[e]), double(w.v[e]), acc[i]);
    }
    if (blockIdx.x == 0)
        for (int64_t j = nc * VW + threadIdx.x; j < n; j += PJ_WG) {
            const double w = double(v[j]);
#pragma unroll
            for (int i = 0; i < M; ++i) acc[i] = fma(double(X[int64_t(i) * stride + j]), w, acc[i]);
        }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const double s = block_sum(acc[i], sh);
        if (threadIdx.x == 0) part[int64_t(i) * PROJECT_MAX_WG + blockIdx.x] = s;
        __syncthreads();
    }
}

// (X_i, v), i < count: whole groups of DOT_GROUP, then the rest as a group of its own size
template <typename V, int VW>
__global__ __launch_bounds__(PJ_WG) void dots_kernel(const V *__restrict__ X, int64_t stride, int count, const V *__restrict__ v,
                                                     int64_t n, double *__restrict__ part) {
    __shared__ double sh[PJ_WG];
    int g = 0;
    for (; g + DOT_GROUP <= count; g += DOT_GROUP)
        dot_group<V, VW, DOT_GROUP>(X + int64_t(g) * stride, stride, v, n, part + int64_t(g) * PROJECT_MAX_WG, sh);
    const V *Xg = X + int64_t(g) * stride;
    double *pg = part + int64_t(g) * PROJECT_MAX_WG;
    switch (count - g) {
        case 1: dot_group<V, VW, 1>(Xg, stride, v, n, pg, sh); break;
        case 2: dot_group<V, VW, 2>(Xg, stride, v, n, pg, sh); break;
        case 3: dot_group<V, VW, 3>(Xg, stride, v, n, pg, sh); break;
        case 4: dot_group<V, VW, 4>(Xg, stride, v, n, pg, sh); break;
        case 5: dot_group<V, VW, 5>(Xg, stride, v, n, pg, sh); break;
        case 6: dot_group<V, VW, 6>(Xg, stride, v, n, pg, sh); break;
        case 7: dot_group<V, VW, 7>(Xg, stride, v, n, pg, sh); break;
        default: break;
    }
}

// Workgroup i: thread t adds slots t, t + 256, ... of vector i's row in order, then the fixed tree -> out[i]
__global__ __launch_bounds__(PJ_WG) void dots_fold_kernel(const double *__restrict__ part, int nwg, double *__restrict__ out) {
    __shared__ double sh[PJ_WG];
    const double *row = part + int64_t(blockIdx.x) * PROJECT_MAX_WG;
    double a = 0.0;
    for (int i = int(threadIdx.x); i < nwg; i += PJ_WG) a += row[i];
    a = block_sum(a, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// out = (base or 0) + sign * sum_i c_i X_i: accumulated in double with i ascending, rounded once.  out may be base (neither
// is any X_i).
template <typename V, int VW>
__global__ __launch_bounds__(PJ_WG) void lincomb_kernel(const V *base, const V *__restrict__ X, int64_t stride, int count,
                                                        const double *__restrict__ c, double sign, V *out, int64_t n) {
    const int64_t nc = n / VW, step = int64_t(gridDim.x) * PJ_WG;
    for (int64_t k = int64_t(blockIdx.x) * PJ_WG + threadIdx.x; k < nc; k += step) {
        double acc[VW];
        if (base) {
            const Chunk<V, VW> b = ld<V, VW>(base, k);
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = double(b.v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = 0.0;
        }
#pragma unroll 4
        for (int i = 0; i < count; ++i) {
            const Chunk<V, VW> x = ld<V, VW>(X + int64_t(i) * stride, k);
            const double ci = sign * c[i];
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = fma(ci, double(x.v[e]), acc[e]);
        }
        Chunk<V, VW> o;
#pragma unroll
        for (int e = 0; e < VW; ++e) o.v[e] = V(acc[e]);
        st<V, VW>(out, k, o);
    }
    if (blockIdx.x == 0)
        for (int64_t j = nc * VW + threadIdx.x; j < n; j += PJ_WG) {
            double acc = base ? double(base[j]) : 0.0;
            for (int i = 0; i < count; ++i) acc = fma(sign * c[i], double(X[int64_t(i) * stride + j]), acc);
            out[j] = V(acc);
        }
}

// The new direction d is kept exactly when s2 = (d, A d) is finite, > 0 and >= 2^-26 e0, e0 = (d, A d) before the
// orthogonalisation: then d <- d / sqrt(s2).  Every thread takes the decision from the same two scalars; status[0]: the set's
// size afterwards, status[1]: kept.
template <typename V, int VW>
__global__ __launch_bounds__(PJ_WG) void keep_scale_kernel(V *__restrict__ d, int64_t n, const double *__restrict__ s2p,
                                                           const double *__restrict__ e0p, int size, int32_t *__restrict__ status) {
    const double s2 = *s2p, e0 = *e0p;
    const bool keep = std::isfinite(s2) && s2 > 0.0 && s2 >= 0x1p-26 * e0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[0] = size + (keep ? 1 : 0);
        status[1] = keep ? 1 : 0;
    }
    if (!keep) return;
    const double r = 1.0 / sqrt(s2);
    const int64_t nc = n / VW, step = int64_t(gridDim.x) * PJ_WG;
    for (int64_t k = int64_t(blockIdx.x) * PJ_WG + threadIdx.x; k < nc; k += step) {
        Chunk<V, VW> x = ld<V, VW>(d, k);
#pragma unroll
        for (int e = 0; e < VW; ++e) x.v[e] = V(double(x.v[e]) * r);
        st<V, VW>(d, k, x);
    }
    if (blockIdx.x == 0)
        for (int64_t j = nc * VW + threadIdx.x; j < n; j += PJ_WG) d[j] = V(double(d[j]) * r);
}

template <typename V>
constexpr int vec_width() { return int(16 / sizeof(V)); }

// every vector a launch touches is 16-byte aligned: the pointers, and the distance between the X_i
template <typename V>
bool wide(int64_t stride, std::initializer_list<const void *> ptrs) {
    if ((size_t(stride) * sizeof(V)) & 15u) return false;
    for (const void *p : ptrs)
        if (p && (reinterpret_cast<uintptr_t>(p) & 15u)) return false;
    return true;
}

int workgroups(int64_t n, int vw) {
    const int64_t chunks = (n + vw - 1) / vw;
    return int(std::max<int64_t>(1, std::min<int64_t>(PROJECT_MAX_WG, (chunks + PJ_WG - 1) / PJ_WG)));
}

}  // namespace

// (each launcher picks the 16-byte form from the pointers and the stride alone: the order of the sums repeats from run to run)
template <typename V>
void project_dots(const V *X, int64_t stride, int count, const V *v, int64_t n, double *part, double *out, hipStream_t s) {
    if (count <= 0) return;
    const bool w = wide<V>(stride, {X, v});
    const int nwg = workgroups(n, w ? vec_width<V>() : 1);
    if (w) hipLaunchKernelGGL((dots_kernel<V, vec_width<V>()>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, X, stride, count, v, n, part);
    else hipLaunchKernelGGL((dots_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, X, stride, count, v, n, part);
    hipLaunchKernelGGL(dots_fold_kernel, dim3(unsigned(count)), dim3(PJ_WG), 0, s, part, nwg, out);
    OMG_HIP(hipGetLastError());
}

template <typename V>
void project_lincomb(const V *base, const V *X, int64_t stride, int count, const double *c, bool subtract, V *out, int64_t n,
                     hipStream_t s) {
    const bool w = wide<V>(stride, {base, X, out});
    const int nwg = workgroups(n, w ? vec_width<V>() : 1);
    const double sign = subtract ? -1.0 : 1.0;
    if (w) hipLaunchKernelGGL((lincomb_kernel<V, vec_width<V>()>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, base, X, stride, count, c, sign, out, n);
    else hipLaunchKernelGGL((lincomb_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, base, X, stride, count, c, sign, out, n);
    OMG_HIP(hipGetLastError());
}

template <typename V>
void project_keep_scale(V *d, int64_t n, const double *s2, const double *e0, int size, int32_t *status, hipStream_t s) {
    const bool w = wide<V>(0, {d});
    const int nwg = workgroups(n, w ? vec_width<V>() : 1);
    if (w) hipLaunchKernelGGL((keep_scale_kernel<V, vec_width<V>()>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, d, n, s2, e0, size, status);
    else hipLaunchKernelGGL((keep_scale_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PJ_WG), 0, s, d, n, s2, e0, size, status);
    OMG_HIP(hipGetLastError());
}

#define PROJECT_INST(V)                                                                                                   \
    template void project_dots<V>(const V *, int64_t, int, const V *, int64_t, double *, double *, hipStream_t);           \
    template void project_lincomb<V>(const V *, const V *, int64_t, int, const double *, bool, V *, int64_t, hipStream_t); \
    template void project_keep_scale<V>(V *, int64_t, const double *, const double *, int, int32_t *, hipStream_t);
PROJECT_INST(double)
PROJECT_INST(float)
#undef PROJECT_INST

}  // namespace omg
