// The sine-transform solve of the 16 x 16 x 16 grid as a device function: the body of sine_cube16_kernel (coarse.hip) and
// the first stage of tail_up_kernel (plane.hip), which repeats the solve in every workgroup instead of waiting for a launch
// of its own.  One copy, so that the two cannot drift apart: same wave <-> plane assignment, same chains of matrix
// instructions, same order x y z | z x y, same division.
#pragma once
#include <hip/hip_runtime.h>

namespace omg {

typedef double v4d __attribute__((ext_vector_type(4)));

// Lanes of ONE wave exchange values through LDS: the stores of all lanes must be complete and visible before any lane's
// loads of the transposed addresses (nothing kept the compiler from reordering the may-alias accesses).
__device__ __forceinline__ void wave_lds_exchange() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int SINE16_N = 16, SINE16_PX = SINE16_N + 1;
constexpr int SINE16_BUF = SINE16_N * SINE16_N * SINE16_PX;       // doubles of LDS: (i, j, k) at (k N + j) PX + i

// The operands a thread of the 1024 feeds the matrix instructions with (A: lane 16 k + i holds S[i][k]; k-step ks:
// k = 4 ks + k4), requested together before anything waits for them
struct Sine16Operands {
    double sx[4], sy[4], sz[4], lam[4], rhs[4];
};
template <typename V>
__device__ __forceinline__ Sine16Operands sine_cube16_load(const V *__restrict__ b, const double *__restrict__ tables,
                                                           const double *__restrict__ lambda) {
    constexpr int N = SINE16_N;
    const int lane = int(threadIdx.x) & 63, w = int(threadIdx.x) >> 6;
    const int c = lane & 15, k4 = lane >> 4;
    Sine16Operands o;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        o.sx[ks] = tables[(0 * N + c) * N + 4 * ks + k4];
        o.sy[ks] = tables[(1 * N + c) * N + 4 * ks + k4];
        o.sz[ks] = tables[(2 * N + c) * N + 4 * ks + k4];
        o.rhs[ks] = double(b[(w * N + c) * N + 4 * ks + k4]);                 // line (k = w, j = c), element i = 4 ks + k4
        o.lam[ks] = lambda[((4 * ks + k4) * N + w) * N + c];                  // element (i = c, j = w, k = 4 ks + k4)
    }
    return o;
}

// Sixteen waves (1024 threads); wave w owns PLANE k = w for the transforms along x and y and the z-LINES (j = w, every i)
// for the transforms along z (coarse.hip has the whole account).  buf: SINE16_BUF doubles of LDS.  The result leaves from
// the last matrix instruction's registers: out(i, j, k, value) once for every cell, k = the wave.
template <typename OUT>
__device__ __forceinline__ void sine_cube16_solve(const Sine16Operands &o, double *buf, OUT out) {
    constexpr int N = SINE16_N, PX = SINE16_PX;
    const int lane = int(threadIdx.x) & 63, w = int(threadIdx.x) >> 6;
    const int c = lane & 15, k4 = lane >> 4;
    auto transform = [&](const double (&S)[4], const double (&in)[4]) -> v4d {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(S[ks], in[ks], acc, 0, 0, 0);
        return acc;
    };
    double in[4];
    // ---- forward along x and y, plane k = w -------------------------------------------------------------------
    v4d acc = transform(o.sx, o.rhs);                  // rows i' = 4 r + k4 of line j = c
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[(w * N + c) * PX + 4 * r + k4] = acc[r];
    wave_lds_exchange();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) in[ks] = buf[(w * N + 4 * ks + k4) * PX + c];       // line (k = w, i = c), element j
    acc = transform(o.sy, in);                         // rows j' = 4 r + k4 of line i = c
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[(w * N + 4 * r + k4) * PX + c] = acc[r];
    __syncthreads();
    // ---- along z: forward, the division, inverse — lines (j = w, i = c), in registers -----------------------------
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) in[ks] = buf[((4 * ks + k4) * N + w) * PX + c];
    acc = transform(o.sz, in);
#pragma unroll
    for (int r = 0; r < 4; ++r) in[r] = acc[r] / o.lam[r];
    acc = transform(o.sz, in);
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[((4 * r + k4) * N + w) * PX + c] = acc[r];
    __syncthreads();
    // ---- inverse along x and y, plane k = w; the result leaves from the matrix instruction's registers --------------
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) in[ks] = buf[(w * N + c) * PX + 4 * ks + k4];
    acc = transform(o.sx, in);
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[(w * N + c) * PX + 4 * r + k4] = acc[r];
    wave_lds_exchange();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) in[ks] = buf[(w * N + 4 * ks + k4) * PX + c];
    acc = transform(o.sy, in);
#pragma unroll
    for (int r = 0; r < 4; ++r) out(c, 4 * r + k4, w, acc[r]);
}

}  // namespace omg
