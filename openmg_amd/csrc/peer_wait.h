// Device code shared by the peer-store runners (plane.hip, dist.hip, dist27.hip); common.h stays host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace omg {

// Wait until a flag another GPU (or another process's kernel) stores into this GPU's memory holds at least seq
// (wrapping compare): system-scope loads, a bounded number of them — a wait that gives up sets bit 0 of *status
// and lets the caller run on (its results are then wrong and the host says so) instead of hanging the device.
__device__ __forceinline__ void peer_wait(const uint32_t *flag, uint32_t seq, uint32_t *status, uint32_t spin) {
    if (!flag) return;
    for (uint32_t n = 0;; ++n) {
        const uint32_t v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (int32_t(v - seq) >= 0) break;
        if (n >= spin) {
            if (status) __hip_atomic_fetch_or(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(16);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");      // what the flag's writer stored before it: not from this CU's L1 / this XCD's L2
}

}  // namespace omg
