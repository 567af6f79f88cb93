// Mean projection x <- x - mean(x) of a device vector (common.h launch_project_mean): what a singular operator with the
// constant null space needs of its right-hand side (a b with a mean has no solution: the cycles stall at |mean b| sqrt(n))
// and of the iterate it hands out (Gauss-Seidel lets the iterate's mean drift; the residual does not see it).
//
// The sum follows pcg.hip's reductions: every workgroup of a grid-stride launch adds its share in double and leaves it in
// its own slot, one workgroup adds the slots in a fixed order — no atomics, the same bits from run to run.  The subtraction
// is a second streaming launch that reads the folded sum; nothing comes back to the host in between.  16-byte accesses
// where the vector is 16-byte aligned, single values for the tail (and for the whole vector otherwise); n values are
// touched, never a value behind them.
#include <algorithm>

#include "common.h"

namespace omg {
namespace {

constexpr int PROJ_WG = 256;

// deterministic sum of the 256 values of a workgroup (fixed tree)
__device__ __forceinline__ double block_sum(double v, double *sh) {
    const int t = int(threadIdx.x);
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = PROJ_WG / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

template <typename V, int VW>
struct Chunk {
    V v[VW];
};

// sum of this workgroup's values -> part[wg]
template <typename V, int VW>
__global__ __launch_bounds__(PROJ_WG) void mean_sum_kernel(const V *__restrict__ x, int64_t n, double *__restrict__ part) {
    __shared__ double sh[PROJ_WG];
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PROJ_WG;
    double a = 0.0;
    for (int64_t c = int64_t(blockIdx.x) * PROJ_WG + threadIdx.x; c < nc; c += stride) {
        const Chunk<V, VW> u = reinterpret_cast<const Chunk<V, VW> *>(x)[c];
#pragma unroll
        for (int e = 0; e < VW; ++e) a += double(u.v[e]);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PROJ_WG) a += double(x[i]);
    a = block_sum(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// One workgroup: thread t adds slots t, t + 256, ... in order, then the fixed tree.
__global__ __launch_bounds__(PROJ_WG) void mean_fold_kernel(const double *__restrict__ part, int nwg, double *__restrict__ out) {
    __shared__ double sh[PROJ_WG];
    double a = 0.0;
    for (int i = int(threadIdx.x); i < nwg; i += PROJ_WG) a += part[i];
    a = block_sum(a, sh);
    if (threadIdx.x == 0) *out = a;
}

// x_i = V(double(x_i) - sum / n)
template <typename V, int VW>
__global__ __launch_bounds__(PROJ_WG) void mean_subtract_kernel(V *__restrict__ x, int64_t n, const double *__restrict__ sum) {
    const double mean = *sum / double(n);
    const int64_t nc = n / VW, stride = int64_t(gridDim.x) * PROJ_WG;
    for (int64_t c = int64_t(blockIdx.x) * PROJ_WG + threadIdx.x; c < nc; c += stride) {
        Chunk<V, VW> u = reinterpret_cast<const Chunk<V, VW> *>(x)[c];
#pragma unroll
        for (int e = 0; e < VW; ++e) u.v[e] = V(double(u.v[e]) - mean);
        reinterpret_cast<Chunk<V, VW> *>(x)[c] = u;
    }
    if (blockIdx.x == 0)
        for (int64_t i = nc * VW + threadIdx.x; i < n; i += PROJ_WG) x[i] = V(double(x[i]) - mean);
}

}  // namespace

template <typename V>
void launch_project_mean(V *x, int64_t n, double *scratch, hipStream_t s) {
    if (n <= 0) return;
    constexpr int VW = int(16 / sizeof(V));
    // (the 16-byte form is chosen from the pointer alone: the order of the sum, and with it its bits, repeats from run to run)
    const bool wide = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    const int64_t chunks = wide ? (n + VW - 1) / VW : n;
    const int nwg = int(std::max<int64_t>(1, std::min<int64_t>(PROJECT_MAX_WG, (chunks + PROJ_WG - 1) / PROJ_WG)));
    double *const sum = scratch + PROJECT_MAX_WG;
    if (wide) hipLaunchKernelGGL((mean_sum_kernel<V, VW>), dim3(unsigned(nwg)), dim3(PROJ_WG), 0, s, x, n, scratch);
    else hipLaunchKernelGGL((mean_sum_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PROJ_WG), 0, s, x, n, scratch);
    hipLaunchKernelGGL(mean_fold_kernel, dim3(1), dim3(PROJ_WG), 0, s, scratch, nwg, sum);
    if (wide) hipLaunchKernelGGL((mean_subtract_kernel<V, VW>), dim3(unsigned(nwg)), dim3(PROJ_WG), 0, s, x, n, sum);
    else hipLaunchKernelGGL((mean_subtract_kernel<V, 1>), dim3(unsigned(nwg)), dim3(PROJ_WG), 0, s, x, n, sum);
    OMG_HIP(hipGetLastError());
}

template void launch_project_mean<double>(double *, int64_t, double *, hipStream_t);
template void launch_project_mean<float>(float *, int64_t, double *, hipStream_t);

}  // namespace omg
