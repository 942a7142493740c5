// What the kernels that rank scores inside ONE workgroup share (resampled_metrics_kernel, youden_kernel): 8-byte keys staged in dynamic
// LDS and sorted descending, every thread the owner of a contiguous range of positions, positives before a range by an inclusive scan,
// the start of a tie group by binary search.  The key LAYOUT is the caller's (a compile-time mask names the bits that order the keys).
// Also the order-preserving fp32 <-> u32 map (Youden keys, trajectory_audit.hip's radix selection) and the fixed-tree fp64 workgroup sum.
#pragma once
#include "common.h"
#include "medp_hip.h"

// fp32 -> u32 in the order of the values (-0.0 below +0.0, NaNs at both ends: the caller decides what to do with either) and back
__host__ __device__ __forceinline__ unsigned f32_order_key(float v) {
    const unsigned b = __builtin_bit_cast(unsigned, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float f32_from_order_key(unsigned u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// Fixed-tree sums of NV values per thread over a workgroup of THREADS (a power of two): the same order on every run, every thread
// gets the totals.  NOT block_sum_wave_order_f64 (head_rules.h), which adds in another order.
template <int THREADS, int NV>
__device__ void block_sum_tree_f64(double (&v)[NV], double (*red)[THREADS], int tid) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NV; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = red[q][0];
}
template <int THREADS>
__device__ double block_sum_tree_f64(double v, double* red, int tid) {        // NV = 1 on a plain value and red[THREADS]
    double one[1] = {v};
    block_sum_tree_f64<THREADS, 1>(one, (double (*)[THREADS])red, tid);
    return one[0];
}

// Bitonic sort of keys[M] in LDS (M a power of two >= 2), descending by key & MASK: M / 2 compare-exchanges per step, a barrier after
// each.  Keys that agree under MASK end in either order.
template <int THREADS, unsigned long long MASK>
__device__ __forceinline__ void lds_sort_desc(unsigned long long* keys, int M, int tid) {
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < M / 2; t += THREADS) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool desc = (a & k) == 0;
                if (((ka & MASK) < (kb & MASK)) == desc) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            __syncthreads();
        }
}

// thread tid owns the C positions [c0, c1) of the L sorted keys (of M staged ones: an empty range past L)
struct OwnedRange { int C, c0, c1; };
template <int THREADS>
__device__ __forceinline__ OwnedRange owned_range(int M, int L, int tid) {
    const int C = M > THREADS ? M / THREADS : 1;
    const int c0 = min(tid * C, L);
    return {C, c0, min(c0 + C, L)};
}

// Inclusive scan over the workgroup of one int per thread (double-buffered Hillis-Steele; `scan` is the caller's scratch) -> the
// inclusive values of ALL threads: [tid] this thread's, [THREADS - 1] the total.  Valid until the caller's next use of `scan`.
template <int THREADS>
__device__ __forceinline__ const int* block_inclusive_scan(int v, int (*scan)[THREADS], int tid) {
    scan[0][tid] = v;
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < THREADS; s <<= 1) {
        scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= s ? scan[cur][tid - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    return scan[cur];
}

// first position in [lo, hi) of the descending keys with key & mask <= target (hi when there is none): the start of a tie group
__device__ __forceinline__ int first_at_most(const unsigned long long* keys, unsigned long long mask, unsigned long long target, int lo, int hi) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((keys[mid] & mask) > target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// host: the length to stage for replicates of up to max_len <= MEDP_LDS_SORT_MAX_LEN keys (a power of two >= 2); on the first call
// per device KERNEL's dynamic-LDS cap is raised to the bound's 128 KiB
template <auto KERNEL>
int lds_sort_staged_len(int max_len) {
    MEDP_ONCE_PER_DEVICE({ hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, MEDP_LDS_SORT_MAX_LEN * 8); });
    int M = 2;
    while (M < max_len) M <<= 1;
    return M;
}
