// Building blocks shared by the thread-per-key few-query attention kernels (attention_small.hip: <= 1024 keys in one
// workgroup; attention_fq_split.hip: any number of keys, split over workgroups).  Head dim 64, fp32, 256 threads.
#pragma once
#include "common.h"

namespace {

constexpr int FQ = 8;            // most queries
constexpr int FQ_T = 256;        // threads = keys per chunk

// The compiler would hoist all 8 x 16 broadcast LDS reads of a fully unrolled (d, q) loop nest to the top (512 VGPRs: the backward
// spilled 8 KB per lane); a compiler + scheduler barrier per d step keeps each step's 8 reads next to their 32 FMAs.
#define FQ_KEEP_IN_STEP()                    \
    do {                                     \
        asm volatile("" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)

// an LDS address the compiler cannot see through: loads from it can neither be hoisted above this point nor merged with
// earlier loads of the same bytes (kept in 512 VGPRs from the score phase to the dK phase otherwise)
__device__ __forceinline__ const float* FQ_OPAQUE(const float* p) {
    asm volatile("" : "+v"(p));
    return p;
}

__device__ __forceinline__ void fq_block_reduce(float (&v)[FQ], float* red, int lane, int wave, bool is_max) {
#pragma unroll
    for (int q = 0; q < FQ; ++q) v[q] = is_max ? wave_max(v[q]) : wave_sum(v[q]);
    __syncthreads();                                   // `red` may still be read from the previous reduction
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < FQ; ++q) red[wave * FQ + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        const float a = red[q], b = red[FQ + q], c = red[2 * FQ + q], d = red[3 * FQ + q];
        v[q] = is_max ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
    }
}

// out[q][0..63] = sum_j w[q][j] * rows[j][0..63]: thread = (16-B piece c of the row, key slice ks of 16); partial sums meet in LDS
__device__ __forceinline__ void fq_weighted_rows(const float* sW, int ldw, const float* rows, size_t ld, int Lk, int Lq, float* sR, int tid,
                                                 float* out, size_t ldo) {
    const int c = tid & 15, ks = tid >> 4;
    float4 acc[FQ];
#pragma unroll
    for (int q = 0; q < FQ; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = ks; j0 < Lk; j0 += 16 * 4) {
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = (j0 + 16 * u < Lk) ? *(const float4*)(rows + (size_t)(j0 + 16 * u) * ld + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = min(j0 + 16 * u, Lk - 1);            // (past the end the row is zero)
#pragma unroll
            for (int q = 0; q < FQ; ++q) {
                const float w = sW[q * ldw + j];
                acc[q].x += w * r[u].x; acc[q].y += w * r[u].y; acc[q].z += w * r[u].z; acc[q].w += w * r[u].w;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < FQ; ++q) *(float4*)(sR + ((ks * FQ + q) * 64 + c * 4)) = acc[q];
    __syncthreads();
    for (int t = tid; t < Lq * 64; t += FQ_T) {
        const int q = t >> 6, d = t & 63;
        float a = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) a += sR[(k2 * FQ + q) * 64 + d];
        out[(size_t)q * ldo + d] = a;
    }
}

}  // namespace
