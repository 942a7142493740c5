// What the grouped training layers (duett_train.hip) and the fused recompute MLP (duett_embed_train.hip) share: the BatchNorm formulas,
// the fixed-order tail of a workgroup's four partial sums and the ordered sum over row chunks.  ONE body per formula: the fused kernels
// are tested bit for bit against the grouped ones (tests/test_gpu_gmlp.py).  Operand order and grouping are part of the contract: every
// row-walking kernel must compile to the instructions it had before a change here (tools/diff_kernel_isa.py).  Not part of the C ABI.
#pragma once
#include "common.h"

namespace {

// the four row-lane (or wave) partials of a workgroup, always in this order
__device__ __forceinline__ float sum4_fixed(float a, float b, float c, float d) { return (a + b) + (c + d); }
// the chunks' shifted sums of (g, c), part [g][chunk][2][C], added in ascending chunk order
__device__ __forceinline__ void bn_sum_stat_chunks(const float* __restrict__ part, int g, int c, int C, int nchunk, float* s1, float* s2) {
    float a = 0.f, q = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) {
        const float* o = part + (((size_t)g * nchunk + k) * 2) * C;
        a += o[c];
        q += o[C + c];
    }
    *s1 = a, *s2 = q;
}
// shifted sums  s1 = sum (x - pivot),  s2 = sum (x - pivot)^2  over R rows -> mean and BIASED variance
__device__ __forceinline__ void bn_finish_stats(float s1, float s2, float pivot, int R, float* mu, float* var) {
    const float m1 = s1 / (float)R;
    *mu = pivot + m1;
    *var = fmaxf(s2 / (float)R - m1 * m1, 0.f);
}
// running = (1-m)*running + m*batch, the variance UNBIASED; num_batches_tracked is the caller's
__device__ __forceinline__ void bn_running_update(float* rmean, float* rvar, float mu, float var, int R, float momentum) {
    *rmean = (1.f - momentum) * *rmean + momentum * mu;
    *rvar = (1.f - momentum) * *rvar + momentum * var * ((float)R / (float)max(R - 1, 1));
}
// rs = rsqrt(var + eps)
__device__ __forceinline__ float bn_apply(float a, float mu, float rs, float w, float b) { return (a - mu) * rs * w + b; }
// train: dx = w*rs*(dy - s1/R - xhat*s2/R) with xhat = centred*rs, s1 = sum dy, s2 = sum dy*xhat ; eval (batch_stats == 0): dx = w*rs*dy.
// s1, centred, s2 and w are CALLABLES, each evaluated where the expression reads it: a kernel whose operands live in memory
// (gbn_bwd_dx_kernel) keeps its train-only loads behind the switch and the load of w after it, in this order.  Passed by value, the
// loads are hoisted and sunk again in another order: same values, another instruction schedule.
template <class S1, class XC, class S2, class W>
__device__ __forceinline__ float bn_dx(float dy, float rs, int R, int batch_stats, S1 s1, XC centred, S2 s2, W w) {
    float v = dy;
    if (batch_stats) v -= s1() / (float)R + centred() * rs * s2() / (float)R;
    return w() * rs * v;
}

// ---- ordered sum over row chunks, the second stage of the two-stage sums of both files: part [g][chunk][D], D = the segments' lengths
// back to back; segment s of the sum goes to its own tensor dst[s] [g][len[s]].  One thread per element, ascending chunk.
struct ChunkSumSegs { float* dst[4]; int len[4]; };           // unused segments: len 0
__global__ __launch_bounds__(256) void chunk_sum_kernel(const float* __restrict__ part, ChunkSumSegs segs, int nchunk, int D) {
    const int g = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D) return;
    float a = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) a += part[((size_t)g * nchunk + k) * D + i];
    int lo = 0;
#pragma unroll
    for (int s = 0; s < 4; lo += segs.len[s++])                // unrolled: the table is read with constant indices, from scalar registers
        if (i >= lo && i < lo + segs.len[s]) segs.dst[s][(size_t)g * segs.len[s] + (i - lo)] = a;
}
inline void chunk_sum(const float* part, int G, int nchunk, const ChunkSumSegs& segs, hipStream_t s) {
    const int D = segs.len[0] + segs.len[1] + segs.len[2] + segs.len[3];
    chunk_sum_kernel<<<dim3((D + 255) / 256, G), 256, 0, s>>>(part, segs, nchunk, D);
}
// eval mode: the "saved" statistics the apply and backward kernels read are the running ones
inline void bn_save_running(float* save_mean, float* save_var, const float* running_mean, const float* running_var, size_t n, hipStream_t s) {
    (void)hipMemcpyAsync(save_mean, running_mean, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(save_var, running_var, n * sizeof(float), hipMemcpyDeviceToDevice, s);
}

}  // namespace
