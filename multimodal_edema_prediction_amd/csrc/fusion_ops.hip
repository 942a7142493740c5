// Pointwise / tiny-reduction kernels of the cross-modal fusion head (gfx950); the losses are in losses.hip.
// Everything here is launch-bound ([B,7] logits, [B*7,256] latents): the point is ONE launch per logical op, fp32
// math identical to the reference, and dropout masks that are regenerated (not stored) in backward.
#include "common.h"
#include "medp_hip.h"

namespace {

constexpr size_t GRID_CAP = 2048;          // workgroups per launch here (grid_for, common.h)

// y = dropout(gelu(x))                        (nn.GELU -> nn.Dropout, model :755, :573)
template <bool Y16>
__global__ __launch_bounds__(256) void gelu_dropout_fwd_kernel(const float* __restrict__ x, void* __restrict__ y, size_t n, float p,
                                                               float inv_keep, uint32_t seed0, uint32_t sid, const uint32_t* __restrict__ epoch) {
    const uint32_t seed = medp_mix_epoch(seed0, epoch);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = gelu_erf(x[i]);
        if (p > 0.f) v *= dropout_scale(seed, sid, (uint32_t)i, p, inv_keep);
        if constexpr (Y16) ((bf16_t*)y)[i] = f2bf(v);          // the next Linear's operand directly (same rounding as the cast kernel)
        else ((float*)y)[i] = v;
    }
}
// dx = dy * mask * gelu'(x); DX16: also the bf16 copy the previous Linear's two gradient GEMMs take as their operand
template <bool DX16>
__global__ __launch_bounds__(256) void gelu_dropout_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               float* __restrict__ dx, bf16_t* __restrict__ dx16, size_t n, float p, float inv_keep,
                                                               uint32_t seed0, uint32_t sid, const uint32_t* __restrict__ epoch) {
    const uint32_t seed = medp_mix_epoch(seed0, epoch);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float g = dy[i] * gelu_erf_grad(x[i]);
        if (p > 0.f) g *= dropout_scale(seed, sid, (uint32_t)i, p, inv_keep);
        dx[i] = g;
        if constexpr (DX16) dx16[i] = f2bf(g);
    }
}
// out = res + dropout(y)  (fwd, res may be null)   |   dy = dout * mask  (bwd: res == nullptr, y = dout)
__global__ __launch_bounds__(256) void dropout_add_kernel(const float* __restrict__ y, const float* __restrict__ res,
                                                          float* __restrict__ out, size_t n, float p, float inv_keep, uint32_t seed0,
                                                          uint32_t sid, const uint32_t* __restrict__ epoch) {
    const uint32_t seed = medp_mix_epoch(seed0, epoch);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = y[i];
        if (p > 0.f) v *= dropout_scale(seed, sid, (uint32_t)i, p, inv_keep);
        out[i] = res ? res[i] + v : v;
    }
}

// y[m] = <x[m,:], w> (+ b)        — the 64 -> 1 output layer of the pathology heads (model :574, :590); wave per row
__global__ __launch_bounds__(256) void rowdot_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y, int rows, int D) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float a = 0.f;
    for (int c = lane; c < D; c += 64) a += x[(size_t)row * ldx + c] * w[c];
    a = wave_sum(a);
    if (lane == 0) y[row] = a + (b ? b[0] : 0.f);
}
// dx[m,c] = dy[m]*w[c] ; dw[c] = sum_m dy[m]*x[m,c] ; db = sum_m dy[m]
// grid = ceil(D/64) blocks of 64 columns x 16 row-lanes (block 0 also writes db).  The heads have D = 64 and rows = B*K = 448,
// i.e. ONE block: 16 row-lanes (1024 threads) keep the per-thread chain at 28 dependent iterations instead of 112 (48 -> ~12 us,
// on the serial tail of the step behind the CXR encoder).
__global__ __launch_bounds__(1024) void rowdot_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, int ldx,
                                                          const float* __restrict__ w, float* __restrict__ dx, float* __restrict__ dw,
                                                          float* __restrict__ db, int rows, int D) {
    __shared__ float red[16][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    float a = 0.f;
    if (c < D) {
        const float wc = w[c];
#pragma unroll 4
        for (int m = rl; m < rows; m += 16) {
            const float g = dy[m];
            dx[(size_t)m * D + c] = g * wc;
            a += g * x[(size_t)m * ldx + c];
        }
    }
    red[rl][cl] = a;
    __syncthreads();
    if (rl == 0 && c < D) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cl];
        dw[c] = t;
    }
    if (db && blockIdx.x == 0) {
        __syncthreads();
        float bs = 0.f;
        for (int m = threadIdx.x; m < rows; m += 1024) bs += dy[m];
        bs = wave_sum(bs);
        if (cl == 0) red[0][rl] = bs;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += red[0][k];
            db[0] = t;
        }
    }
}

// residual-fusion logit assembly (model :634-639):
//   img = hi + image_label_bias ; ts = ht + temporal_label_bias ; corr = hc ; scaled = beta*corr ; fus = img.detach() + scaled
__global__ __launch_bounds__(256) void fusion_logits_fwd_kernel(const float* __restrict__ hi, const float* __restrict__ ht,
                                                                const float* __restrict__ hc, const float* __restrict__ ib,
                                                                const float* __restrict__ tb, const float* __restrict__ beta,
                                                                float* __restrict__ img, float* __restrict__ ts, float* __restrict__ scaled,
                                                                float* __restrict__ fus, int B, int K) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B * K; i += gridDim.x * 256) {
        const int k = i % K;
        const float a = hi[i] + ib[k], s = beta[k] * hc[i];
        img[i] = a;
        ts[i] = ht[i] + tb[k];
        scaled[i] = s;
        fus[i] = a + s;
    }
}
// grads: d_hi = d_img (fus is detached from img); d_ht = d_ts; d_hc = beta*(d_scaled + d_fus); per-label sums for the biases / beta
__global__ __launch_bounds__(64) void fusion_logits_bwd_kernel(const float* __restrict__ d_img, const float* __restrict__ d_ts,
                                                               const float* __restrict__ d_scaled, const float* __restrict__ d_fus,
                                                               const float* __restrict__ hc, const float* __restrict__ beta,
                                                               float* __restrict__ d_hi, float* __restrict__ d_ht, float* __restrict__ d_hc,
                                                               float* __restrict__ d_ib, float* __restrict__ d_tb, float* __restrict__ d_beta,
                                                               int B, int K) {
    const int k = threadIdx.x;
    if (k >= K) return;
    float sib = 0.f, stb = 0.f, sbe = 0.f;
    for (int b = 0; b < B; ++b) {
        const int i = b * K + k;
        const float gi = d_img ? d_img[i] : 0.f, gt = d_ts ? d_ts[i] : 0.f;
        const float gs = (d_scaled ? d_scaled[i] : 0.f) + (d_fus ? d_fus[i] : 0.f);
        d_hi[i] = gi;
        d_ht[i] = gt;
        d_hc[i] = beta[k] * gs;
        sib += gi;
        stb += gt;
        sbe += gs * hc[i];
    }
    d_ib[k] = sib;
    d_tb[k] = stb;
    d_beta[k] = sbe;
}

// mean over the first T tokens of [B, T+1, D] (StudentModel pool="mean", model :1231) and its backward
__global__ __launch_bounds__(256) void meanpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T, int T1, int D) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B * D; i += gridDim.x * 256) {
        const int b = i / D, d = i % D;
        float a = 0.f;
        for (int t = 0; t < T; ++t) a += x[((size_t)b * T1 + t) * D + d];
        y[i] = a / (float)T;
    }
}
__global__ __launch_bounds__(256) void meanpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int T, int T1, int D) {
    const size_t n = (size_t)B * T1 * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), t = (int)((i / D) % T1), b = (int)(i / ((size_t)D * T1));
        dx[i] = t < T ? dy[(size_t)b * D + d] / (float)T : 0.f;
    }
}

}  // namespace

extern "C" int medp_gelu_dropout_fwd(const float* x, float* y, long long n, float p, unsigned seed, unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(x && y && n > 0 && p >= 0.f && p < 1.f, "gelu_dropout_fwd: bad argument");
    gelu_dropout_fwd_kernel<false><<<grid_for((size_t)n, GRID_CAP), 256, 0, (hipStream_t)stream>>>(x, y, (size_t)n, p, 1.f / (1.f - p), seed, stream_id, medp_rng_epoch_ptr());
    MEDP_LAUNCH_CHECK("medp_gelu_dropout_fwd");
    return 0;
}
extern "C" int medp_gelu_dropout_fwd_bf16(const float* x, void* y_bf16, long long n, float p, unsigned seed, unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(x && y_bf16 && n > 0 && p >= 0.f && p < 1.f, "gelu_dropout_fwd_bf16: bad argument");
    gelu_dropout_fwd_kernel<true><<<grid_for((size_t)n, GRID_CAP), 256, 0, (hipStream_t)stream>>>(x, y_bf16, (size_t)n, p, 1.f / (1.f - p), seed, stream_id, medp_rng_epoch_ptr());
    MEDP_LAUNCH_CHECK("medp_gelu_dropout_fwd_bf16");
    return 0;
}
extern "C" int medp_gelu_dropout_bwd(const float* dy, const float* x, float* dx, long long n, float p, unsigned seed,
                                     unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(dy && x && dx && n > 0 && p >= 0.f && p < 1.f, "gelu_dropout_bwd: bad argument");
    gelu_dropout_bwd_kernel<false><<<grid_for((size_t)n, GRID_CAP), 256, 0, (hipStream_t)stream>>>(dy, x, dx, nullptr, (size_t)n, p, 1.f / (1.f - p), seed, stream_id, medp_rng_epoch_ptr());
    MEDP_LAUNCH_CHECK("medp_gelu_dropout_bwd");
    return 0;
}
extern "C" int medp_gelu_dropout_bwd_bf16(const float* dy, const float* x, float* dx, void* dx_bf16, long long n, float p, unsigned seed,
                                          unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(dy && x && dx && dx_bf16 && n > 0 && p >= 0.f && p < 1.f, "gelu_dropout_bwd_bf16: bad argument");
    gelu_dropout_bwd_kernel<true><<<grid_for((size_t)n, GRID_CAP), 256, 0, (hipStream_t)stream>>>(dy, x, dx, (bf16_t*)dx_bf16, (size_t)n, p, 1.f / (1.f - p), seed, stream_id,
                                                                                       medp_rng_epoch_ptr());
    MEDP_LAUNCH_CHECK("medp_gelu_dropout_bwd_bf16");
    return 0;
}
extern "C" int medp_dropout_add(const float* y, const float* residual, float* out, long long n, float p, unsigned seed,
                                unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(y && out && n > 0 && p >= 0.f && p < 1.f, "dropout_add: bad argument");
    dropout_add_kernel<<<grid_for((size_t)n, GRID_CAP), 256, 0, (hipStream_t)stream>>>(y, residual, out, (size_t)n, p, 1.f / (1.f - p), seed, stream_id, medp_rng_epoch_ptr());
    MEDP_LAUNCH_CHECK("medp_dropout_add");
    return 0;
}
extern "C" int medp_rowdot_fwd(const float* x, int ldx, const float* w, const float* b, float* y, int rows, int D, void* stream) {
    MEDP_CHECK_ARG(x && w && y && rows > 0 && D > 0, "rowdot_fwd: bad argument");
    rowdot_fwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, ldx, w, b, y, rows, D);
    MEDP_LAUNCH_CHECK("medp_rowdot_fwd");
    return 0;
}
extern "C" int medp_rowdot_bwd(const float* dy, const float* x, int ldx, const float* w, float* dx, float* dw, float* db, int rows,
                               int D, void* stream) {
    MEDP_CHECK_ARG(dy && x && w && dx && dw && rows > 0 && D > 0, "rowdot_bwd: bad argument");
    rowdot_bwd_kernel<<<(D + 63) / 64, 1024, 0, (hipStream_t)stream>>>(dy, x, ldx, w, dx, dw, db, rows, D);
    MEDP_LAUNCH_CHECK("medp_rowdot_bwd");
    return 0;
}
extern "C" int medp_fusion_logits_fwd(const float* hi, const float* ht, const float* hc, const float* img_bias, const float* ts_bias,
                                      const float* beta, float* img, float* ts, float* scaled, float* fus, int B, int K, void* stream) {
    MEDP_CHECK_ARG(hi && ht && hc && img_bias && ts_bias && beta && img && ts && scaled && fus && B > 0 && K > 0, "fusion_logits_fwd: bad argument");
    fusion_logits_fwd_kernel<<<grid_for((size_t)B * K, GRID_CAP), 256, 0, (hipStream_t)stream>>>(hi, ht, hc, img_bias, ts_bias, beta, img, ts, scaled, fus, B, K);
    MEDP_LAUNCH_CHECK("medp_fusion_logits_fwd");
    return 0;
}
extern "C" int medp_fusion_logits_bwd(const float* d_img, const float* d_ts, const float* d_scaled, const float* d_fus, const float* hc,
                                      const float* beta, float* d_hi, float* d_ht, float* d_hc, float* d_img_bias, float* d_ts_bias,
                                      float* d_beta, int B, int K, void* stream) {
    MEDP_CHECK_ARG(hc && beta && d_hi && d_ht && d_hc && d_img_bias && d_ts_bias && d_beta && B > 0 && K > 0 && K <= 64, "fusion_logits_bwd: bad argument");
    fusion_logits_bwd_kernel<<<1, 64, 0, (hipStream_t)stream>>>(d_img, d_ts, d_scaled, d_fus, hc, beta, d_hi, d_ht, d_hc, d_img_bias, d_ts_bias, d_beta, B, K);
    MEDP_LAUNCH_CHECK("medp_fusion_logits_bwd");
    return 0;
}
extern "C" int medp_meanpool_fwd(const float* x, float* y, int B, int T, int T1, int D, void* stream) {
    MEDP_CHECK_ARG(x && y && B > 0 && T > 0 && T1 >= T && D > 0, "meanpool_fwd: bad argument");
    meanpool_fwd_kernel<<<grid_for((size_t)B * D, GRID_CAP), 256, 0, (hipStream_t)stream>>>(x, y, B, T, T1, D);
    MEDP_LAUNCH_CHECK("medp_meanpool_fwd");
    return 0;
}
extern "C" int medp_meanpool_bwd(const float* dy, float* dx, int B, int T, int T1, int D, void* stream) {
    MEDP_CHECK_ARG(dy && dx && B > 0 && T > 0 && T1 >= T && D > 0, "meanpool_bwd: bad argument");
    meanpool_bwd_kernel<<<grid_for((size_t)B * T1 * D, GRID_CAP), 256, 0, (hipStream_t)stream>>>(dy, dx, B, T, T1, D);
    MEDP_LAUNCH_CHECK("medp_meanpool_bwd");
    return 0;
}

namespace {
__global__ void counter_advance_kernel(unsigned* c) { c[0] += 1u; }
}
extern "C" int medp_counter_advance(unsigned* dev_counter, void* stream) {
    MEDP_CHECK_ARG(dev_counter, "counter_advance: null pointer");
    counter_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(dev_counter);
    MEDP_LAUNCH_CHECK("medp_counter_advance");
    return 0;
}
