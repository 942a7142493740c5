// The launch clock of the tag-1 (CXR-encoder) GEMMs (gemm_profile.hip): the kernel-side stamps of mode 2 and
// the pair of calls the dispatcher puts around a launch.  Not part of the C ABI (medp_gemm_profile_enable / _collect are).
#pragma once
#include "common.h"

// kernel-side halves of the launch clock: the first workgroup to arrive stamps the 100-MHz wall clock, the last to leave
// stamps it again (two agent-scope atomics per workgroup; works inside a replayed hipGraph, where HIP events cannot be read).
// prof: 4 x u64 {t_first_wg_in, t_last_wg_out, arrivals, departures}; flags 1: do not stamp the arrival, 2: not the departure
#define MEDP_PROF_ENTER(prof, flags)                                                                                       \
    do {                                                                                                                   \
        if ((prof) && !((flags) & 1) && threadIdx.x == 0) {                                                                                \
            const unsigned long long n__ = __hip_atomic_fetch_add((prof) + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
            if (n__ % gridDim.x == 0) __hip_atomic_store((prof), wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   \
        }                                                                                                                  \
    } while (0)
#define MEDP_PROF_LEAVE(prof, flags)                                                                                       \
    do {                                                                                                                   \
        if ((prof) && !((flags) & 2)) {                                                                                    \
            __syncthreads();                                                                                               \
            if (threadIdx.x == 0) {                                                                                        \
                const unsigned long long n__ = __hip_atomic_fetch_add((prof) + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
                if (n__ % gridDim.x == gridDim.x - 1)                                                                      \
                    __hip_atomic_store((prof) + 1, wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);            \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)

// Host side, around ONE tag-1 GEMM of `flops` on `stream`.  begin: mode 1 records the start event; mode 2 hands out the launch's
// clock slot in *slot if it takes the 256-tile kernels (`tile256`), else nullptr.  end: mode 1 records the stop event.
int medp_gemm_profile_begin(bool tile256, double flops, void* stream, unsigned long long** slot);
void medp_gemm_profile_end(double flops, void* stream);
