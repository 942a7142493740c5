// Gradient-flow diagnostics of the dual teacher (grad_flow_diagnostics.py): the reductions around ONE replicated backward pass.
// Layouts and contracts: include/medp_hip.h.  Latency-sized work (K <= 16, D = 256, B <= 64): 256-thread workgroups (four wave64),
// fp64 accumulators over fp32 inputs read in place, no floating-point atomics, every accumulator element has one owner and every
// sum runs in a fixed order (per-thread strided partials, the wave butterfly, four wave sums through LDS), so two runs are
// bit-identical.
#include "common.h"
#include "medp_hip.h"

namespace {

constexpr int kMaxK = MEDP_GRAD_FLOW_MAX_K;

// total over the 256 threads of the workgroup, returned to all of them; `red` [4] is reused by every call
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();                                        // the previous call's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the reference's `_cosine` from the three sums: a denominator <= 1e-12 gives 0
__device__ __forceinline__ double cosine_rule(double xy, double xx, double yy) {
    const double den = sqrt(xx) * sqrt(yy);
    return den <= 1e-12 ? 0.0 : xy / fmax(den, 1e-12);
}

// ---- seeds: column k of replica (branch, k) carries that label's loss cotangent, everything else is zero ----------------------
// g_* [B, K]: d(lw_k per_k^branch) / d logit, what medp_dual_pathology_loss writes with unit alphas; per [3K] its per-label losses
__global__ __launch_bounds__(256) void seeds_scatter_kernel(const float* __restrict__ g_img, const float* __restrict__ g_ts,
                                                            const float* __restrict__ g_fus, const float* __restrict__ per,
                                                            const float* __restrict__ lw, float* __restrict__ losses,
                                                            float* __restrict__ cot_img, float* __restrict__ cot_ts,
                                                            float* __restrict__ cot_fus, int B, int K) {
    const size_t n_img = (size_t)B * K * K, n_tf = 2 * n_img;
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    for (size_t i = i0; i < n_img; i += step) {             // [b, g, k]
        const int k = (int)(i % K), g = (int)((i / K) % K);
        const size_t b = i / ((size_t)K * K);
        cot_img[i] = g == k ? g_img[b * K + k] : 0.f;
    }
    for (size_t i = i0; i < n_tf; i += step) {              // [b, g, k], g < K: ts replicas, g >= K: fusion replicas
        const int k = (int)(i % K), g = (int)((i / K) % (2 * K));
        const size_t b = i / ((size_t)2 * K * K);
        cot_ts[i] = g == k ? g_ts[b * K + k] : 0.f;
        cot_fus[i] = g == k + K ? g_fus[b * K + k] : 0.f;
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 3 * K; i += 256) losses[i] = lw[i % K] * per[i];
}

// ---- accumulate, launch 1: workgroup b < B: the sample's sensitivity partials; the others add dq into the state ---------------
// part [B, 2 (img, ts), 1 + K (total, label 0 .. K-1), 2 (raw, scaled)]
__global__ __launch_bounds__(256) void accumulate_rows_kernel(const float* __restrict__ dq, const float* __restrict__ dI,
                                                              const float* __restrict__ dT, const float* __restrict__ I,
                                                              const float* __restrict__ T, double* __restrict__ state,
                                                              double* __restrict__ part, int B, int K, int D) {
    __shared__ double red[4];
    const int KD = K * D;
    if ((int)blockIdx.x >= B) {
        const size_t n = (size_t)3 * K * KD, step = (size_t)(gridDim.x - B) * 256;
        for (size_t i = (size_t)(blockIdx.x - B) * 256 + threadIdx.x; i < n; i += step) state[i] += (double)dq[i];
        return;
    }
    const size_t b = blockIdx.x;
    const float* grads[2] = {dI, dT};
    const float* toks[2] = {I, T};
    for (int m = 0; m < 2; ++m) {
        double* out = part + (b * 2 + m) * (size_t)(1 + K) * 2;
        const float* g = grads[m] ? grads[m] + b * (size_t)K * KD : nullptr;       // [K_label, K, D] of this sample
        const float* t = toks[m] + b * (size_t)KD;
        double tt = 0.0;
        for (int e = threadIdx.x; e < KD; e += 256) tt += (double)t[e] * (double)t[e];
        const double tok_norm = sqrt(block_sum(tt, red));
        for (int q = 0; q <= K; ++q) {                      // q = 0: the total gradient sum_k g[k]; q >= 1: label q - 1
            double ss = 0.0;
            if (g) {
                for (int e = threadIdx.x; e < KD; e += 256) {
                    double v = 0.0;
                    if (q == 0)
                        for (int k = 0; k < K; ++k) v += (double)g[(size_t)k * KD + e];
                    else
                        v = (double)g[(size_t)(q - 1) * KD + e];
                    ss += v * v;
                }
            }
            const double gn = sqrt(block_sum(ss, red));
            if (threadIdx.x == 0) {
                out[q * 2] = gn;
                out[q * 2 + 1] = gn * tok_norm;
            }
        }
    }
}

// ---- accumulate, launch 2 (one workgroup): sums over the samples, the batch cosine, losses and counts ------------------------
__global__ __launch_bounds__(256) void accumulate_batch_kernel(const float* __restrict__ dq, const float* __restrict__ mask,
                                                               const float* __restrict__ losses, const double* __restrict__ part,
                                                               double* __restrict__ state, int B, int K, int D) {
    __shared__ double red[4];
    const int KD = K * D;
    const size_t n_pl = (size_t)3 * K * KD;
    double* s_loss = state + n_pl;
    double* s_scal = s_loss + 3;                            // batch_cos_sum, negative count, batch_count, sample_count
    double* s_valid = s_scal + 4;
    double* s_sens = s_valid + K;                           // img_raw, ts_raw, img_scaled, ts_scaled
    double* s_sens_label = s_sens + 4;                      // [4, K] in the same key order
    const int cols = 2 * (1 + K) * 2;
    for (int c = 0; c < cols; ++c) {                        // c = (m, q, raw | scaled)
        double v = 0.0;
        for (int b = threadIdx.x; b < B; b += 256) v += part[(size_t)b * cols + c];
        v = block_sum(v, red);
        if (threadIdx.x == 0) {
            const int m = c / (2 * (1 + K)), q = (c / 2) % (1 + K), key = (c & 1) * 2 + m;
            if (q == 0)
                s_sens[key] += v;
            else
                s_sens_label[key * K + q - 1] += v;
        }
    }
    double aa = 0.0, bb = 0.0, ab = 0.0;
    for (int e = threadIdx.x; e < KD; e += 256) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < K; ++k) {
            a += (double)dq[(size_t)k * KD + e];
            b += (double)dq[(size_t)(K + k) * KD + e];
        }
        aa += a * a;
        bb += b * b;
        ab += a * b;
    }
    aa = block_sum(aa, red);
    bb = block_sum(bb, red);
    ab = block_sum(ab, red);
    if (threadIdx.x == 0) {
        const double c = cosine_rule(ab, aa, bb);
        s_scal[0] += c;
        s_scal[1] += c < 0.0 ? 1.0 : 0.0;
        s_scal[2] += 1.0;
        s_scal[3] += (double)B;
        for (int r = 0; r < 3; ++r) {
            double l = 0.0;
            for (int k = 0; k < K; ++k) l += (double)losses[r * K + k];
            s_loss[r] += l;
        }
    }
    if ((int)threadIdx.x < K) {
        double v = 0.0;
        for (int b = 0; b < B; ++b) v += (double)mask[(size_t)b * K + threadIdx.x];
        s_valid[threadIdx.x] += v;
    }
}

// ten sums of three vectors x_r[e] = inv_nb * sum_{k < nk} base[r * stride_r + k * n + e], e < n, and t = sum_r alpha_r x_r:
// out = xx yy zz xy xz yz tt xt yt zt.  All threads get all ten.
__device__ void gram3(const double* base, size_t stride_r, int nk, int n, double inv_nb, const double* alpha, double* out, double* red) {
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = threadIdx.x; e < n; e += 256) {
        double x[3];
        for (int r = 0; r < 3; ++r) {
            double v = 0.0;
            for (int k = 0; k < nk; ++k) v += base[r * stride_r + (size_t)k * n + e];
            x[r] = v * inv_nb;
        }
        const double t = alpha[0] * x[0] + alpha[1] * x[1] + alpha[2] * x[2];
        acc[0] += x[0] * x[0];
        acc[1] += x[1] * x[1];
        acc[2] += x[2] * x[2];
        acc[3] += x[0] * x[1];
        acc[4] += x[0] * x[2];
        acc[5] += x[1] * x[2];
        acc[6] += t * t;
        acc[7] += x[0] * t;
        acc[8] += x[1] * t;
        acc[9] += x[2] * t;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) out[i] = block_sum(acc[i], red);
}

// ---- report (one workgroup) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void report_kernel(const double* __restrict__ state, double a_img, double a_ts, double a_fus,
                                                     double* __restrict__ out, int K, int D) {
    __shared__ double red[4];
    const int KD = K * D;
    const size_t n_branch = (size_t)K * KD, n_pl = 3 * n_branch;
    const double* s_loss = state + n_pl;
    const double* s_scal = s_loss + 3;
    const double* s_valid = s_scal + 4;
    const double* s_sens = s_valid + K;
    const double* s_sens_label = s_sens + 4;
    const double alpha[3] = {a_img, a_ts, a_fus};
    const double nb = fmax(s_scal[2], 1.0), inv_nb = 1.0 / nb, ns = fmax(s_scal[3], 1.0);
    double g[10];
    gram3(state, n_branch, K, KD, inv_nb, alpha, g, red);   // the mean branch gradients: label sums of the per-label means
    if (threadIdx.x == 0) {
        for (int r = 0; r < 3; ++r) {
            out[4 * r] = s_loss[r] * inv_nb;
            out[4 * r + 1] = sqrt(g[r]);
            out[4 * r + 2] = sqrt(alpha[r] * alpha[r] * g[r]);
            out[4 * r + 3] = cosine_rule(alpha[r] * g[7 + r], alpha[r] * alpha[r] * g[r], g[6]);
        }
        out[12] = cosine_rule(g[3], g[0], g[1]);
        out[13] = cosine_rule(g[4], g[0], g[2]);
        out[14] = cosine_rule(g[5], g[1], g[2]);
        out[15] = s_scal[0] * inv_nb;
        out[16] = s_scal[1] * inv_nb;
        out[17] = out[2] / fmax(out[6], 1e-12);
        for (int i = 0; i < 4; ++i) out[18 + i] = s_sens[i] / ns;
        out[22] = out[18] / fmax(out[19], 1e-12);
        out[23] = out[20] / fmax(out[21], 1e-12);
        out[24] = s_scal[2];
        out[25] = s_scal[3];
    }
    for (int k = 0; k < K; ++k) {
        double* o = out + MEDP_GRAD_FLOW_REPORT_HEAD + (size_t)MEDP_GRAD_FLOW_REPORT_PER_LABEL * k;
        gram3(state + (size_t)k * KD, n_branch, 1, KD, inv_nb, alpha, g, red);
        double own[3];
        for (int r = 0; r < 3; ++r) {                       // row k of label k's gradient: the label's own query
            double v = 0.0;
            for (int d = threadIdx.x; d < D; d += 256) {
                const double x = state[r * n_branch + (size_t)k * KD + (size_t)k * D + d] * inv_nb;
                v += x * x;
            }
            own[r] = sqrt(block_sum(v, red));
        }
        if (threadIdx.x == 0) {
            const double nv = fmax(s_valid[k], 1.0);
            o[0] = s_valid[k];
            for (int r = 0; r < 3; ++r) {
                o[1 + r] = sqrt(g[r]);
                o[8 + r] = own[r] / fmax(o[1 + r], 1e-12);
            }
            o[4] = cosine_rule(g[3], g[0], g[1]);
            o[5] = cosine_rule(g[4], g[0], g[2]);
            o[6] = cosine_rule(g[5], g[1], g[2]);
            o[7] = sqrt(g[6]);
            for (int i = 0; i < 4; ++i) o[11 + i] = s_sens_label[i * K + k] / nv;
            o[15] = o[13] / fmax(o[14], 1e-12);
        }
    }
}

// ---- query geometry (one workgroup): thread (i, j) owns gram[s][i][j] for the three row sets ----------------------------------
__global__ __launch_bounds__(256) void query_geometry_kernel(const float* __restrict__ rows, double* __restrict__ out, int K, int D) {
    __shared__ double red[4];
    __shared__ double s_norm[3][kMaxK];
    for (int i = threadIdx.x; i < 3 * K; i += 256) {
        const float* r = rows + (size_t)i * D;
        double v = 0.0;
        for (int d = 0; d < D; ++d) v += (double)r[d] * (double)r[d];
        s_norm[i / K][i % K] = sqrt(v);
    }
    __syncthreads();
    double gap = 0.0;
    if ((int)threadIdx.x < K * K) {
        const int i = threadIdx.x / K, j = threadIdx.x % K;
        double gram[3];
        for (int s = 0; s < 3; ++s) {
            const float* a = rows + ((size_t)s * K + i) * D;
            const float* b = rows + ((size_t)s * K + j) * D;
            const double na = fmax(s_norm[s][i], 1e-12), nb = fmax(s_norm[s][j], 1e-12);
            double v = 0.0;
            for (int d = 0; d < D; ++d) v += ((double)a[d] / na) * ((double)b[d] / nb);
            gram[s] = v;
            out[(size_t)s * K * K + threadIdx.x] = v;
        }
        gap = (gram[1] - gram[2]) * (gram[1] - gram[2]);
    }
    gap = block_sum(gap, red);
    if ((int)threadIdx.x < K) out[(size_t)3 * K * K + threadIdx.x] = s_norm[0][threadIdx.x];
    if (threadIdx.x == 0) out[(size_t)3 * K * K + K] = sqrt(gap) / (double)K;
}

bool shape_ok(int K, int D) { return K > 0 && K <= kMaxK && D > 0 && D <= MEDP_GRAD_FLOW_MAX_D; }

}  // namespace

extern "C" size_t medp_grad_flow_state_doubles(int K, int D) {
    return shape_ok(K, D) ? (size_t)3 * K * K * D + 11 + (size_t)5 * K : 0;
}
extern "C" size_t medp_grad_flow_ws_doubles(int B, int K) {
    return (B > 0 && K > 0 && K <= kMaxK) ? (size_t)B * 4 * (1 + K) : 0;
}

extern "C" int medp_grad_flow_seeds(const float* img, const float* ts, const float* fus, const float* y, const float* mask,
                                    const float* label_weights, const float* pos_weight, float eps, float* ws, float* losses,
                                    float* cot_img, float* cot_ts, float* cot_fus, int B, int K, void* stream) {
    MEDP_CHECK_ARG(img && ts && fus && y && mask && label_weights && ws && losses && cot_img && cot_ts && cot_fus,
                   "grad_flow_seeds: null argument");
    MEDP_CHECK_ARG(B > 0 && B <= MEDP_GRAD_FLOW_MAX_B && K > 0 && K <= kMaxK, "grad_flow_seeds: need 0 < B <= %d, 0 < K <= %d (got %d, %d)",
                   MEDP_GRAD_FLOW_MAX_B, kMaxK, B, K);
    float* per = ws;                                        // [4 + 3K]: total, branch totals, per-label losses
    float* g = ws + 4 + 3 * K;                              // three [B, K] gradients
    const size_t bk = (size_t)B * K;
    // the BCE rule lives in losses.hip: with unit alphas its gradients ARE the per-label cotangents
    MEDP_TRY(medp_dual_pathology_loss(img, ts, fus, y, mask, label_weights, pos_weight, 1.f, 1.f, 1.f, eps, per, g, g + bk, g + 2 * bk, B, K,
                                      stream));
    seeds_scatter_kernel<<<grid_for(2 * bk * K, 64), 256, 0, (hipStream_t)stream>>>(g, g + bk, g + 2 * bk, per + 4, label_weights, losses,
                                                                                    cot_img, cot_ts, cot_fus, B, K);
    MEDP_LAUNCH_CHECK("medp_grad_flow_seeds");
    return 0;
}

extern "C" int medp_grad_flow_accumulate(const float* dq, const float* dI, const float* dT, const float* I, const float* T,
                                         const float* mask, const float* losses, double* state, double* ws, int B, int K, int D,
                                         void* stream) {
    MEDP_CHECK_ARG(dq && dT && I && T && mask && losses && state && ws, "grad_flow_accumulate: null argument");
    MEDP_CHECK_ARG(B > 0 && B <= MEDP_GRAD_FLOW_MAX_B && shape_ok(K, D), "grad_flow_accumulate: need 0 < B <= %d, 0 < K <= %d, 0 < D <= %d (got %d, %d, %d)",
                   MEDP_GRAD_FLOW_MAX_B, kMaxK, MEDP_GRAD_FLOW_MAX_D, B, K, D);
    const int dq_blocks = grid_for((size_t)3 * K * K * D, 16);
    accumulate_rows_kernel<<<B + dq_blocks, 256, 0, (hipStream_t)stream>>>(dq, dI, dT, I, T, state, ws, B, K, D);
    MEDP_LAUNCH_CHECK("medp_grad_flow_accumulate");
    accumulate_batch_kernel<<<1, 256, 0, (hipStream_t)stream>>>(dq, mask, losses, ws, state, B, K, D);
    MEDP_LAUNCH_CHECK("medp_grad_flow_accumulate");
    return 0;
}

extern "C" int medp_grad_flow_report(const double* state, double alpha_img, double alpha_ts, double alpha_fus, double* out, int K, int D,
                                     void* stream) {
    MEDP_CHECK_ARG(state && out, "grad_flow_report: null argument");
    MEDP_CHECK_ARG(shape_ok(K, D), "grad_flow_report: need 0 < K <= %d, 0 < D <= %d (got %d, %d)", kMaxK, MEDP_GRAD_FLOW_MAX_D, K, D);
    report_kernel<<<1, 256, 0, (hipStream_t)stream>>>(state, alpha_img, alpha_ts, alpha_fus, out, K, D);
    MEDP_LAUNCH_CHECK("medp_grad_flow_report");
    return 0;
}

extern "C" int medp_query_geometry(const float* rows, double* out, int K, int D, void* stream) {
    MEDP_CHECK_ARG(rows && out, "query_geometry: null argument");
    MEDP_CHECK_ARG(shape_ok(K, D), "query_geometry: need 0 < K <= %d, 0 < D <= %d (got %d, %d)", kMaxK, MEDP_GRAD_FLOW_MAX_D, K, D);
    query_geometry_kernel<<<1, 256, 0, (hipStream_t)stream>>>(rows, out, K, D);
    MEDP_LAUNCH_CHECK("medp_query_geometry");
    return 0;
}
