// Rules the head-probe kernels share (head_probe.hip, pool_head_probe.hip): the label padding and its compile-time dispatch, the
// fixed-order block sum, the step clock (step number, dropout seed, AdamW scalars), torch's AdamW on one element, the masked BCE of
// one logit, the epoch's loss sums, the store of one score, the launchers' checks of the steps, the permutation and the columns.
// Each exists once, so every head takes the same update bit for bit.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "medp_hip.h"

constexpr int HEAD_LDS_BUDGET = 144 * 1024;                                  // of the CU's 160 KiB
constexpr float kNaNf = __builtin_nanf("");

// labels padded to a compile-time count (the accumulators stay in registers)
__host__ __device__ inline int head_lp(int L) { return L <= 2 ? 2 : L <= 8 ? 8 : 16; }
// f(std::integral_constant<int, head_lp(L)>()): the one place that turns the padding into a template argument
template <class Fn>
__host__ __device__ __forceinline__ auto with_head_lp(int L, Fn&& f) {
    const int lp = head_lp(L);
    if (lp == 2) return f(std::integral_constant<int, 2>());
    if (lp == 8) return f(std::integral_constant<int, 8>());
    return f(std::integral_constant<int, 16>());
}

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
// The step clock of a head that has taken t0 steps.  advance() moves to the next step (t is 1-based): b1t = beta1^t and b2t = beta2^t
// by one fp64 multiply each, the AdamW scalars of step t into `a`, and it returns the step's dropout seed (medp_mix_epoch with the
// head's own step count).  `a` is the caller's, not a member: held inside this struct the seven floats reach adamw() in a form that
// changes which of its multiply-adds hipcc fuses in head_epoch, and with that the bits of W.
struct HeadSchedule {
    double lr, beta1, beta2, b1t, b2t;
    uint32_t seed;
    int t;
    __host__ __device__ HeadSchedule(AdamScalars& a, double lr_, double weight_decay, double beta1_, double beta2_, double eps, uint32_t seed_, int t0)
        : lr(lr_), beta1(beta1_), beta2(beta2_), b1t(pow(beta1_, (double)t0)), b2t(pow(beta2_, (double)t0)), seed(seed_), t(t0) {
        a.decay = (float)(1.0 - lr * weight_decay);
        a.omb1 = (float)(1.0 - beta1);
        a.beta2 = (float)beta2;
        a.omb2 = (float)(1.0 - beta2);
        a.eps = (float)eps;
    }
    __host__ __device__ uint32_t advance(AdamScalars& a) {
        ++t;
        b1t *= beta1;
        b2t *= beta2;
        a.step_size = (float)(lr / (1.0 - b1t));
        a.bc2_sqrt = (float)sqrt(1.0 - b2t);
        return seed + (uint32_t)t * 0x9E3779B9u;
    }
};
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
// one step into the epoch's (sum of loss * vc, sum of vc), lsum being the step's sum of loss terms: the reference adds
// loss.item() * vc with loss = lsum / vc, and nothing for a step that knows no label
__device__ __forceinline__ void add_step_loss(double& run_l, double& run_v, double lsum, double vc) {
    if (vc > 0.0) {
        run_l += lsum / vc * vc;
        run_v += vc;
    }
}

// the scores of row i of n, label l: the logit (NaN for a row outside the matrix) and the fp32 sigmoid, widened
__device__ __forceinline__ void head_store_score(float* __restrict__ logits, double* __restrict__ probs, int i, int l, int L, int n, bool ok, float z) {
    const float zf = ok ? z : kNaNf;
    logits[(size_t)i * L + l] = zf;
    probs[(size_t)l * n + i] = (double)(1.0f / (1.0f + expf(-zf)));
}

// ---- the launchers' checks (host)
inline int check_labels_and_columns(const char* what, int p, long long ldx, int N, int col0, int width, int L) {
    MEDP_CHECK_ARG(L >= 1 && L <= MEDP_HEAD_MAX_L, "%s: problem %d has L=%d, not in [1, %d]", what, p, L, MEDP_HEAD_MAX_L);
    MEDP_CHECK_ARG(N >= 1 && col0 >= 0 && (long long)col0 + width <= ldx, "%s: problem %d columns [%d, %lld) leave a row of %lld (N=%d)", what, p,
                   col0, (long long)col0 + width, ldx, N);
    return 0;
}
inline int check_steps(const char* what, int p, int N, int bs, int S, float dropout_p, double lr, double beta1, double beta2, double eps) {
    MEDP_CHECK_ARG(bs >= 1 && bs <= MEDP_HEAD_MAX_BS, "%s: problem %d has bs=%d, not in [1, %d]", what, p, bs, MEDP_HEAD_MAX_BS);
    MEDP_CHECK_ARG(S >= 1 && (long long)S * bs <= N, "%s: problem %d has S=%d steps of %d rows with N=%d", what, p, S, bs, N);
    MEDP_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: problem %d has dropout_p=%g, not in [0, 1)", what, p, (double)dropout_p);
    MEDP_CHECK_ARG(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                   "%s: problem %d has bad AdamW scalars", what, p);
    return 0;
}
// The host copy of a permutation, for the heads whose problem carries one.  The linear head's does not: its kernel checks on the
// device and writes NaN, which head_probe.train_heads turns into the error.
inline int check_perm(const char* what, int p, const int* perm_host, long long count, int N) {
    for (long long i = 0; i < count; ++i)
        MEDP_CHECK_ARG((unsigned)perm_host[i] < (unsigned)N, "%s: problem %d has permutation entry %lld = %d outside [0, %d)", what, p, i,
                       perm_host[i], N);
    return 0;
}
