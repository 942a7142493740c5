// Rules the head-probe kernels share (head_probe.hip, pool_head_probe.hip): the label padding, the fixed-order block sum, torch's
// AdamW on one element, the masked BCE of one logit.  Each exists once, so every head takes the same update bit for bit.
#pragma once
#include <math.h>

#include "common.h"

constexpr int HEAD_LDS_BUDGET = 144 * 1024;                                  // of the CU's 160 KiB

// labels padded to a compile-time count (the accumulators stay in registers)
__host__ __device__ inline int head_lp(int L) { return L <= 2 ? 2 : L <= 8 ? 8 : 16; }

// every thread gets the sum; waves are added in wave order
template <int WAVES>
__device__ __forceinline__ double block_sum_wave_order_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[w];
    return s;
}

struct AdamScalars {
    float decay, omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};
// the scalars of step number t (1-based) from b1t = beta1^t, b2t = beta2^t
__host__ __device__ inline void adam_step_scalars(AdamScalars& a, double lr, double b1t, double b2t) {
    a.step_size = (float)(lr / (1.0 - b1t));
    a.bc2_sqrt = (float)sqrt(1.0 - b2t);
}
__host__ __device__ inline void adam_fixed_scalars(AdamScalars& a, double lr, double weight_decay, double beta1, double beta2, double eps) {
    a.decay = (float)(1.0 - lr * weight_decay);
    a.omb1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
}
// torch.optim.AdamW, single-tensor path: mul_(1 - lr wd); lerp_(g, 1 - b1); mul_(b2).addcmul_(g, g, 1 - b2);
// denom = sqrt(v) / sqrt(1 - b2^t) + eps; addcdiv_(m, denom, -lr / (1 - b1^t))
__device__ __forceinline__ void adamw(float* p, float* m, float* v, float g, const AdamScalars& a) {
    const float pn = *p * a.decay;
    const float mn = *m + a.omb1 * (g - *m);
    const float vn = *v * a.beta2 + (a.omb2 * g) * g;
    const float denom = sqrtf(vn) / a.bc2_sqrt + a.eps;
    *p = pn + (-a.step_size * mn) / denom;
    *m = mn;
    *v = vn;
}

// one label of the masked BCE: returns the loss term BCE(z, y) m and sets g = (sigmoid(z) - y) m / vc (0 when vc = 0: the
// reference's loss is logits.sum() * 0 then)
__device__ __forceinline__ double masked_bce_term(double z, double y, double m, double vc, float* g) {
    const double ex = exp(-fabs(z));
    const double sg = z >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
    *g = vc > 0.0 ? (float)((sg - y) * m / vc) : 0.f;
    return (fmax(z, 0.0) - y * z + log1p(ex)) * m;
}
