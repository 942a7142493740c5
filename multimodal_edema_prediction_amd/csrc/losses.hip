// The training losses (gfx950): value + gradient in ONE single-workgroup launch each.  All of them are launch-bound ([B,7] logits,
// a few thousand read-out cells); what matters is fp32 math identical to the reference and a FIXED summation order (wave
// butterflies, then the four wave sums as (0+1)+(2+3)), so that a step reproduces bit for bit.
#include "common.h"
#include "medp_hip.h"

namespace {

// ---- the rules, each once ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_neg(float l) { return fmaxf(-l, 0.f) + log1pf(__expf(-fabsf(l))); }   // log(1+exp(-l))
__device__ __forceinline__ float sigmoid(float l) { return 1.f / (1.f + __expf(-l)); }
__device__ __forceinline__ float sigmoid_t(float z, float T) { return 1.f / (1.f + __expf(-z / T)); }   // at temperature T: -z / T negates first
// BCEWithLogits, with pos_weight: (1-y)*l + (1 + (pw-1)*y) * log(1+exp(-l)), and without
__device__ __forceinline__ float bce_logits(float l, float y, float pw) { return (1.f - y) * l + (1.f + (pw - 1.f) * y) * softplus_neg(l); }
__device__ __forceinline__ float bce_logits(float l, float y) { return (1.f - y) * l + softplus_neg(l); }
// d bce / dl.  Two algebraic forms on purpose (they round differently): (1-y) - (1+(pw-1)y)(1-sigmoid(l)) for the pos_weight
// kernels, sigmoid(l) - y for the unweighted ones.
__device__ __forceinline__ float bce_logits_grad(float l, float y, float pw) { return (1.f - y) - (1.f + (pw - 1.f) * y) * (1.f - sigmoid(l)); }
__device__ __forceinline__ float bce_logits_grad(float l, float y) { return sigmoid(l) - y; }
// KL(Bern(t) || Bern(p)) for p = clamp_prob(pr, eps), pr = sigmoid(logit), and its derivative with respect to that logit:
// d kl / d p = -t/p + (1-t)/(1-p), exactly zero where the clamp is active; d pr / d logit = pr (1 - pr)
__device__ __forceinline__ float clamp_prob(float pr, float eps) { return fminf(fmaxf(pr, eps), 1.f - eps); }
__device__ __forceinline__ float bern_kl(float t, float p) { return t * (logf(t) - logf(p)) + (1.f - t) * (logf(1.f - t) - logf(1.f - p)); }
__device__ __forceinline__ float bern_kl_dlogit(float t, float pr, float p, float eps) {
    const float inside = (pr > eps && pr < 1.f - eps) ? 1.f : 0.f;
    return inside * (-t / p + (1.f - t) / (1.f - p)) * pr * (1.f - pr);
}
// one element of the aux residual KL: the smoothed target, sigmoid(img + scaled) and its clamped form
constexpr float AUX_EPS = 1e-6f;
struct AuxCell { float ys, pr, p; };
__device__ __forceinline__ AuxCell aux_cell(float y, float img, float scaled, float smooth) {
    const float ys = y * (1.f - smooth) + (1.f - y) * smooth, pr = sigmoid(img + scaled);
    return {ys, pr, clamp_prob(pr, AUX_EPS)};
}

// ---- DualPathologyLoss (loss/losses_duett.py:131-194) forward + gradient in ONE single-block launch -------------------
// per branch r, label k:  per[r][k] = sum_b bce(l_bk, y_bk [,pos_weight_k]) * m_bk / (sum_b m_bk + eps)
// branch_total[r] = sum_k w_k per[r][k];  total = sum_r alpha_r branch_total[r]
// grad[r][b][k] = alpha_r * w_k * m_bk / (sum_b m_bk + eps) * dbce/dl
// out: [0] total, [1..3] branch totals, [4 .. 4+3K) per-label losses (img | ts | fus)
__global__ __launch_bounds__(256) void dual_loss_kernel(const float* __restrict__ img, const float* __restrict__ ts,
                                                        const float* __restrict__ fus, const float* __restrict__ y,
                                                        const float* __restrict__ mask, const float* __restrict__ lw,
                                                        const float* __restrict__ pw, float a_img, float a_ts, float a_fus, float eps,
                                                        float* __restrict__ out, float* __restrict__ g_img, float* __restrict__ g_ts,
                                                        float* __restrict__ g_fus, int B, int K) {
    __shared__ float s_per[3][32];
    __shared__ float s_den[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* L[3] = {img, ts, fus};
    // wave w handles labels w, w+4, ...
    for (int k = wave; k < K; k += 4) {
        float den = 0.f, acc[3] = {0.f, 0.f, 0.f};
        const float pwk = pw ? pw[k] : 1.f;
        for (int b = lane; b < B; b += 64) {
            const float m = mask[b * K + k], yy = y[b * K + k];
            den += m;
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[r] += bce_logits(L[r][b * K + k], yy, pwk) * m;
        }
        den = wave_sum(den);
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[r] = wave_sum(acc[r]);
        if (lane == 0) {
            s_den[k] = den + eps;
#pragma unroll
            for (int r = 0; r < 3; ++r) s_per[r][k] = acc[r] / (den + eps);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot[3] = {0.f, 0.f, 0.f};
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < K; ++k) {
                tot[r] += lw[k] * s_per[r][k];
                out[4 + r * K + k] = s_per[r][k];
            }
        out[0] = a_img * tot[0] + a_ts * tot[1] + a_fus * tot[2];
        out[1] = tot[0];
        out[2] = tot[1];
        out[3] = tot[2];
    }
    float* G[3] = {g_img, g_ts, g_fus};
    const float A[3] = {a_img, a_ts, a_fus};
    for (int i = threadIdx.x; i < B * K; i += 256) {
        const int k = i % K;
        const float m = mask[i], yy = y[i], pwk = pw ? pw[k] : 1.f;
        const float c = lw[k] * m / s_den[k];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (G[r]) G[r][i] = A[r] * c * bce_logits_grad(L[r][i], yy, pwk);
    }
}

// ---- StudentKDLoss (losses_duett.py:8-57): total = alpha*BCE(z_s,y) + (1-alpha)*T^2*mean KL(sig(z_t/T) || sig(z_s/T)) ----
// out: [0] total [1] bce [2] kd ; grad wrt z_s
__global__ __launch_bounds__(256) void kd_loss_kernel(const float* __restrict__ zs, const float* __restrict__ zt, const float* __restrict__ y,
                                                      float T, float alpha, float pos_weight, float eps, float* __restrict__ out,
                                                      float* __restrict__ g, int B) {
    __shared__ float red[2][4];
    float bce = 0.f, kl = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float l = zs[b], yy = y[b];
        bce += bce_logits(l, yy, pos_weight);
        const float pt_raw = sigmoid_t(zt[b], T), ps = sigmoid_t(l, T);
        const float psc = clamp_prob(ps, eps), pt = clamp_prob(pt_raw, eps);
        kl += bern_kl(pt, psc);
        if (g) {
            const float dbce = bce_logits_grad(l, yy, pos_weight);
            const float dkl = bern_kl_dlogit(pt, ps, psc, eps) / T;     // the student logit enters as l / T
            g[b] = (alpha * dbce + (1.f - alpha) * T * T * dkl) / (float)B;
        }
    }
    wave_sums_to_lds(bce, kl, red);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float b_ = sum4(red[0]) / (float)B;
        const float k_ = T * T * sum4(red[1]) / (float)B;
        out[0] = alpha * b_ + (1.f - alpha) * k_;
        out[1] = b_;
        out[2] = k_;
    }
}

// ---- engine extras (training_duett/engine.py:149-165, 217-223) and the linear-probe loss (cxr_linear_training.ipynb:426-437) ----
// aux residual KL: KL(Bern(y_smooth) || Bern(sigmoid(img.detach() + scaled))) masked mean; grad wrt `scaled` only.
__global__ __launch_bounds__(256) void aux_kl_kernel(const float* __restrict__ img, const float* __restrict__ scaled, const float* __restrict__ y,
                                                     const float* __restrict__ mask, float smooth, float* __restrict__ out,
                                                     float* __restrict__ g, int n) {
    __shared__ float red[2][4];
    float num = 0.f, den = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const AuxCell c = aux_cell(y[i], img[i], scaled[i], smooth);
        num += bern_kl(c.ys, c.p) * mask[i];
        den += mask[i];
    }
    wave_sums_to_lds(num, den, red);
    __syncthreads();
    const float D = fmaxf(sum4(red[1]), 1.f);
    if (threadIdx.x == 0) out[0] = sum4(red[0]) / D;
    if (g) {
        for (int i = threadIdx.x; i < n; i += 256) {           // the cell is computed again, not carried over the barrier
            const AuxCell c = aux_cell(y[i], img[i], scaled[i], smooth);
            g[i] = bern_kl_dlogit(c.ys, c.pr, c.p, AUX_EPS) * mask[i] / D;
        }
    }
}
// out = coef * mean(x^2), g = 2*coef*x/n        (LP regularisers beta_l2*mean(beta^2), corr_l2*mean(scaled^2))
__global__ __launch_bounds__(256) void sq_mean_kernel(const float* __restrict__ x, float coef, float* __restrict__ out, float* __restrict__ g, int n) {
    __shared__ float red[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        a += x[i] * x[i];
        if (g) g[i] = 2.f * coef * x[i] / (float)n;
    }
    wave_sums_to_lds(a, red);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = coef * sum4(red) / (float)n;
}
// one global masked mean: sum(bce*m)/max(sum(m),1)   (config 2 linear probe)
__global__ __launch_bounds__(256) void masked_bce_kernel(const float* __restrict__ l, const float* __restrict__ y, const float* __restrict__ mask,
                                                         float* __restrict__ out, float* __restrict__ g, int n) {
    __shared__ float red[2][4];
    float num = 0.f, den = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        num += bce_logits(l[i], y[i]) * mask[i];
        den += mask[i];
    }
    wave_sums_to_lds(num, den, red);
    __syncthreads();
    const float D = fmaxf(sum4(red[1]), 1.f);
    if (threadIdx.x == 0) out[0] = sum4(red[0]) / D;
    if (g)
        for (int i = threadIdx.x; i < n; i += 256) g[i] = bce_logits_grad(l[i], y[i]) * mask[i] / D;
}

// ---- losses of the DuETT-only step (BASELINE.json configs[0]; reference duett/duett.py:337-365): masked MSE of the value
// read-outs and (optionally weighted) mean BCE-with-logits
// out = mean(((a - b) * m)^2) ; g = 2 (a - b) m^2 / n
__global__ __launch_bounds__(256) void masked_mse_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ m,
                                                         float* __restrict__ out, float* __restrict__ g, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float mm = m ? m[i] : 1.f, d = (a[i] - b[i]) * mm;
        s += d * d;
        if (g) g[i] = 2.f * d * mm / (float)n;
    }
    wave_sums_to_lds(s, red);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = sum4(red) / (float)n;
}
// out = mean(w * bce(l, y)) ; g = w (sigmoid(l) - y) / n          (w may be NULL)
__global__ __launch_bounds__(256) void bce_mean_kernel(const float* __restrict__ l, const float* __restrict__ y, const float* __restrict__ w,
                                                       float* __restrict__ out, float* __restrict__ g, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float ww = w ? w[i] : 1.f;
        s += ww * bce_logits(l[i], y[i]);
        if (g) g[i] = ww * bce_logits_grad(l[i], y[i]) / (float)n;
    }
    wave_sums_to_lds(s, red);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = sum4(red) / (float)n;
}

}  // namespace

extern "C" int medp_dual_pathology_loss(const float* img, const float* ts, const float* fus, const float* y, const float* mask,
                                        const float* label_weights, const float* pos_weight, float alpha_img, float alpha_ts,
                                        float alpha_fus, float eps, float* out, float* g_img, float* g_ts, float* g_fus, int B, int K,
                                        void* stream) {
    MEDP_CHECK_ARG(img && ts && fus && y && mask && label_weights && out, "dual_pathology_loss: null argument");
    MEDP_CHECK_ARG(B > 0 && K > 0 && K <= 32, "dual_pathology_loss: need 0 < K <= 32 (got %d)", K);
    dual_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(img, ts, fus, y, mask, label_weights, pos_weight, alpha_img, alpha_ts, alpha_fus, eps,
                                                         out, g_img, g_ts, g_fus, B, K);
    MEDP_LAUNCH_CHECK("medp_dual_pathology_loss");
    return 0;
}
extern "C" int medp_student_kd_loss(const float* z_s, const float* z_t, const float* y, float T, float alpha, float pos_weight,
                                    float* out, float* g_zs, int B, void* stream) {
    MEDP_CHECK_ARG(z_s && z_t && y && out && B > 0 && T > 0.f, "student_kd_loss: bad argument");
    kd_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(z_s, z_t, y, T, alpha, pos_weight, 1e-7f, out, g_zs, B);
    MEDP_LAUNCH_CHECK("medp_student_kd_loss");
    return 0;
}
extern "C" int medp_aux_residual_kl(const float* img_logits, const float* scaled_correction, const float* y, const float* mask,
                                    float label_smoothing, float* out, float* g_scaled, int n, void* stream) {
    MEDP_CHECK_ARG(img_logits && scaled_correction && y && mask && out && n > 0, "aux_residual_kl: bad argument");
    aux_kl_kernel<<<1, 256, 0, (hipStream_t)stream>>>(img_logits, scaled_correction, y, mask, label_smoothing, out, g_scaled, n);
    MEDP_LAUNCH_CHECK("medp_aux_residual_kl");
    return 0;
}
extern "C" int medp_sq_mean(const float* x, float coef, float* out, float* g, int n, void* stream) {
    MEDP_CHECK_ARG(x && out && n > 0, "sq_mean: bad argument");
    sq_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(x, coef, out, g, n);
    MEDP_LAUNCH_CHECK("medp_sq_mean");
    return 0;
}
extern "C" int medp_masked_bce_global(const float* logits, const float* y, const float* mask, float* out, float* g, int n, void* stream) {
    MEDP_CHECK_ARG(logits && y && mask && out && n > 0, "masked_bce_global: bad argument");
    masked_bce_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, y, mask, out, g, n);
    MEDP_LAUNCH_CHECK("medp_masked_bce_global");
    return 0;
}
extern "C" int medp_masked_mse(const float* a, const float* b, const float* mask, float* out, float* g_a, int n, void* stream) {
    MEDP_CHECK_ARG(a && b && out && n > 0, "masked_mse: bad argument");
    masked_mse_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a, b, mask, out, g_a, n);
    MEDP_LAUNCH_CHECK("medp_masked_mse");
    return 0;
}
extern "C" int medp_bce_mean(const float* logits, const float* y, const float* weight, float* out, float* g, int n, void* stream) {
    MEDP_CHECK_ARG(logits && y && out && n > 0, "bce_mean: bad argument");
    bce_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, y, weight, out, g, n);
    MEDP_LAUNCH_CHECK("medp_bce_mean");
    return 0;
}
