// Temporal-usage diagnostics (analysis/diagnose_temporal_usage.py; DESIGN.md "Temporal-usage diagnostics"): the two device pieces of
// the question "does a trained dual teacher use the time series, and their order?".
//
//   counterfactual_feats_kernel   `feats_to_input` (batch_assembly.hip) without augmentation for FIVE arrangements of one batch in one
//                                 launch: full, another patient's whole EHR package, another patient's measurements only, time
//                                 reversed, time permuted.  The reference transforms the RAW tuples and assembles afterwards, so the
//                                 flip / permutation act on the whole series BEFORE the truncation to the last max_len steps.  Pure data
//                                 movement: one output element per thread, grid-stride, coalesced on the output side.
//   temporal_usage_summary_kernel one workgroup per (condition, label): the fp32 sigmoid of the gathered logits, widened, in the
//                                 label-major layout the metrics kernel reads; mean |dp|, Pearson correlation against the full
//                                 condition (centred, two passes) and the normalised entropy of the full condition's attention.
//                                 Every reduction is a fixed tree (rank_lds.h's, the metrics kernel's too): two launches are
//                                 bit-identical, no floating-point atomics.
#include "rank_lds.h"

namespace {

constexpr int CF_CONDITIONS = MEDP_COUNTERFACTUAL_CONDITIONS;
enum { CF_FULL = 0, CF_PATIENT_SHUFFLE = 1, CF_TS_SHUFFLE = 2, CF_TIME_REVERSE = 3, CF_TIME_PERMUTE = 4 };

struct CfParams {
    const float* const* ts_ptrs;      // [B] device pointers to [T_i, 2V] (or null: ts_base + i * ts_stride)
    const float* ts_base;
    long long ts_stride;
    const float* const* time_ptrs;    // [B] device pointers to [T_i]      (or null: time_base + i * time_stride)
    const float* time_base;
    long long time_stride;
    const int* lengths;               // [B] original T_i (or null: all T_uniform)
    int T_uniform;
    const float* static_in;           // [B, Ds]
    const int* sample_perm;           // [B]
    const int* time_perm;             // [B, Tmax]
    float* xs_ts;                     // [5, B, Tpad, 2V+1]
    float* xs_times;                  // [5, B, Tpad]
    float* xs_static;                 // [5, B, Ds]
    int B, V, Ds, max_len, Tpad, Tmax;
};

__device__ __forceinline__ int cf_length(const CfParams& p, int b) { return p.lengths ? p.lengths[b] : p.T_uniform; }
// the sample whose EHR package (whole = series, times, static) or series (series only) stands at row b; -1: the permutation
// names no sample of this batch
__device__ __forceinline__ int cf_source(const CfParams& p, int cond, int b, bool series) {
    if (cond == CF_PATIENT_SHUFFLE || (cond == CF_TS_SHUFFLE && series)) {
        const int s = p.sample_perm[b];
        return (s < 0 || s >= p.B) ? -1 : s;
    }
    return b;
}

__global__ __launch_bounds__(256) void counterfactual_feats_kernel(const CfParams p) {
    const int F = 2 * p.V + 1;
    const long long n_ts = (long long)p.B * p.Tpad * F, n_tm = (long long)p.B * p.Tpad, n_st = (long long)p.B * p.Ds;
    const long long t_ts = CF_CONDITIONS * n_ts, t_tm = CF_CONDITIONS * n_tm, t_st = CF_CONDITIONS * n_st;
    const float nan = __builtin_nanf("");
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < t_ts + t_tm + t_st; i += (long long)gridDim.x * 256) {
        if (i < t_ts) {
            const int cond = (int)(i / n_ts);
            const long long e = i % n_ts;
            const int c = (int)(e % F);
            const long long bt = e / F;
            const int t = (int)(bt % p.Tpad), b = (int)(bt / p.Tpad);
            const int s = cf_source(p, cond, b, true);
            float v = 0.f;
            if (s < 0) {
                v = nan;
            } else {
                const int Ts = cf_length(p, s);
                const int n = min(Ts, p.max_len), off = Ts - n;          // the last max_len steps of the TRANSFORMED series
                if (t < n) {
                    int r = off + t;
                    if (cond == CF_TIME_REVERSE) r = Ts - 1 - r;
                    else if (cond == CF_TIME_PERMUTE) r = r < p.Tmax ? p.time_perm[(long long)b * p.Tmax + r] : -1;
                    if (r < 0 || r >= Ts) {
                        v = nan;
                    } else if (c < F - 1) {
                        const float* src = p.ts_ptrs ? p.ts_ptrs[s] : p.ts_base + (long long)s * p.ts_stride;
                        v = src[(long long)r * (2 * p.V) + c];
                    }
                }
            }
            p.xs_ts[i] = v;
        } else if (i < t_ts + t_tm) {
            const long long j = i - t_ts;
            const int cond = (int)(j / n_tm);
            const long long e = j % n_tm;
            const int t = (int)(e % p.Tpad), b = (int)(e / p.Tpad);
            const int s = cf_source(p, cond, b, false);
            float v = 0.f;
            if (s < 0) {
                v = nan;
            } else {
                const int Ts = cf_length(p, s);
                const int n = min(Ts, p.max_len), off = Ts - n;
                if (t < n) {
                    const float* src = p.time_ptrs ? p.time_ptrs[s] : p.time_base + (long long)s * p.time_stride;
                    v = src[off + t];                                    // the bin times are never reversed or permuted
                }
            }
            p.xs_times[j] = v;
        } else {
            const long long j = i - t_ts - t_tm;
            const int cond = (int)(j / n_st);
            const long long e = j % n_st;
            const int d = (int)(e % p.Ds), b = (int)(e / p.Ds);
            const int s = cf_source(p, cond, b, false);
            p.xs_static[j] = s < 0 ? nan : p.static_in[(long long)s * p.Ds + d];
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------------------
constexpr int TU_THREADS = 256;

// exp(x) in fp32 for |x| <= 50 by the algorithm of numpy's float32 `exp` loop (its SIMD kernel on x86 with FMA): round(x log2 e) by the
// 1.5 * 2^23 trick, Cody-Waite reduction by ln 2 in two fp32 pieces, a degree-5 / degree-2 rational in fused multiply-adds, an IEEE
// quotient, the exponent added back.  Every operation is one correctly rounded fp32 operation in numpy's order, so the bits are
// numpy's (up to 2.52 ulp from the exact exponential, as numpy states for it).  No contraction: the product x log2 e and the magic
// add must round separately.
__device__ __forceinline__ float tu_numpy_expf(float x) {
#pragma clang fp contract(off)
    float q = x * 1.442695040888963407359924681001892137f;
    q = (q + 12582912.0f) - 12582912.0f;
    float r = fmaf(q, -6.93145752e-1f, x);
    r = fmaf(q, -1.42860677e-6f, r);
    float num = fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
    num = fmaf(num, r, 5.114512081637298353406e-02f);
    num = fmaf(num, r, 2.473615434895520810817e-01f);
    num = fmaf(num, r, 7.257664613233124478488e-01f);
    num = fmaf(num, r, 9.999999999980870924916e-01f);
    float den = fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
    den = fmaf(den, r, 1.0f);
    return ldexpf(num / den, (int)q);
}

// the fp32 value 1 / (1 + exp(-clip(z, -50, 50))) of the reference's `_prob` on fp32 arrays, in ITS arithmetic: numpy's fp32 exp, an
// fp32 sum and an fp32 quotient.  An fp32 expf of the device library, or an fp64 evaluation rounded once, each landed up to 3 ulp from
// numpy's result (measured): the distance is numpy's own exp error, which only its own algorithm reproduces.
__device__ __forceinline__ float tu_prob(float z) {
#pragma clang fp contract(off)
    if (z != z) return z;
    const float zc = fminf(fmaxf(z, -50.0f), 50.0f);
    const float s = 1.0f + tu_numpy_expf(-zc);
    return 1.0f / s;
}

__global__ __launch_bounds__(TU_THREADS) void temporal_usage_summary_kernel(const float* __restrict__ fus, const float* __restrict__ ts,
                                                                             const float* __restrict__ attn, double* __restrict__ prob,
                                                                             double* __restrict__ sens, double* __restrict__ entropy,
                                                                             int C, int N, int K, int S) {
    __shared__ double red[4][TU_THREADS];
    const int tid = threadIdx.x, c = blockIdx.x / K, k = blockIdx.x % K;
    const size_t CKN = (size_t)C * K * N;
    double* pf = prob + ((size_t)c * K + k) * N;              // fus half
    double* pt = pf + CKN;                                    // ts half
    const float* zf = fus + (size_t)c * N * K + k;
    const float* zt = ts + (size_t)c * N * K + k;
    const float* zf0 = fus + k;                               // the full condition
    const float* zt0 = ts + k;
    // pass 1: probabilities out, sums of p_full, p_c, |dp fus|, |dp ts|
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = tid; n < N; n += TU_THREADS) {
        const double qf = (double)tu_prob(zf[(size_t)n * K]), qt = (double)tu_prob(zt[(size_t)n * K]);
        pf[n] = qf;
        pt[n] = qt;
        if (c > 0) {
            const double q0 = (double)tu_prob(zf0[(size_t)n * K]), t0 = (double)tu_prob(zt0[(size_t)n * K]);
            a[0] += q0;
            a[1] += qf;
            a[2] += fabs(q0 - qf);
            a[3] += fabs(t0 - qt);
        }
    }
    if (c > 0) {
        block_sum_tree_f64<TU_THREADS, 4>(a, red, tid);
        const double m0 = a[0] / (double)N, mc = a[1] / (double)N;
        // pass 2: centred second moments
        double m[3] = {0.0, 0.0, 0.0};
        for (int n = tid; n < N; n += TU_THREADS) {
            const double d0 = (double)tu_prob(zf0[(size_t)n * K]) - m0, dc = (double)tu_prob(zf[(size_t)n * K]) - mc;
            m[0] += d0 * d0;
            m[1] += dc * dc;
            m[2] += d0 * dc;
        }
        block_sum_tree_f64<TU_THREADS, 3>(m, red, tid);
        if (tid == 0) {
            double* o = sens + ((size_t)(c - 1) * K + k) * 3;
            o[0] = a[2] / (double)N;
            o[1] = (N < 2 || !(m[0] > 0.0) || !(m[1] > 0.0)) ? kNaN : m[2] / sqrt(m[0] * m[1]);
            o[2] = a[3] / (double)N;
        }
    } else if (attn) {
        // the full condition's workgroup of label k: mean over the rows of the normalised attention entropy
        const double inv_log_s = 1.0 / fmax(log((double)S), 1e-12);
        double h[1] = {0.0};
        for (int n = tid; n < N; n += TU_THREADS) {
            const float* row = attn + ((size_t)n * K + k) * S;
            double total = 0.0;
            for (int s = 0; s < S; ++s) total += (double)row[s];
            const double den = fmax(total, 1e-12);
            double e = 0.0;
            for (int s = 0; s < S; ++s) {
                const double w = (double)row[s] / den;               // a quotient, as in the reference: x / x is exactly 1 (S = 1 -> entropy 0)
                e -= w * log(fmax(w, 1e-12));
            }
            h[0] += e * inv_log_s;
        }
        block_sum_tree_f64<TU_THREADS, 1>(h, red, tid);
        if (tid == 0) entropy[k] = h[0] / (double)N;
    }
}

}  // namespace

extern "C" int medp_counterfactual_feats(const float* const* ts_ptrs, const float* ts_base, long long ts_stride,
                                         const float* const* time_ptrs, const float* time_base, long long time_stride, const int* lengths,
                                         int T_uniform, const float* static_in, const int* sample_perm, const int* time_perm, float* xs_ts,
                                         float* xs_times, float* xs_static, int B, int V, int Ds, int max_len, int Tpad, int Tmax,
                                         void* stream) {
    MEDP_CHECK_ARG((ts_ptrs || ts_base) && (time_ptrs || time_base) && static_in && sample_perm && time_perm && xs_ts && xs_times && xs_static,
                   "counterfactual_feats: null operand");
    MEDP_CHECK_ARG(B > 0 && V > 0 && Ds > 0 && max_len > 0 && Tpad > 0 && Tpad <= max_len && Tmax > 0,
                   "counterfactual_feats: bad shape B=%d V=%d Ds=%d max_len=%d Tpad=%d Tmax=%d", B, V, Ds, max_len, Tpad, Tmax);
    MEDP_CHECK_ARG(lengths || (T_uniform > 0 && T_uniform <= Tmax), "counterfactual_feats: neither per-sample lengths nor a uniform length within Tmax");
    CfParams p{ts_ptrs, ts_base, ts_stride, time_ptrs, time_base, time_stride, lengths, T_uniform, static_in, sample_perm, time_perm,
               xs_ts, xs_times, xs_static, B, V, Ds, max_len, Tpad, Tmax};
    const long long n = CF_CONDITIONS * ((long long)B * Tpad * (2 * V + 2) + (long long)B * Ds);
    counterfactual_feats_kernel<<<grid_for((size_t)n), 256, 0, (hipStream_t)stream>>>(p);
    MEDP_LAUNCH_CHECK("medp_counterfactual_feats");
    return 0;
}

extern "C" int medp_temporal_usage_summary(const float* fus, const float* ts, const float* attn, double* prob, double* sens,
                                           double* entropy, int C, int N, int K, int S, void* stream) {
    MEDP_CHECK_ARG(fus && ts && prob && (sens || C == 1), "temporal_usage_summary: null operand");
    MEDP_CHECK_ARG(!attn || entropy, "temporal_usage_summary: attention given without an entropy buffer");
    MEDP_CHECK_ARG(C >= 1 && N >= 1 && K >= 1 && (!attn || S >= 1), "temporal_usage_summary: bad shape C=%d N=%d K=%d S=%d", C, N, K, S);
    MEDP_CHECK_ARG(N <= MEDP_TEMPORAL_USAGE_MAX_N && (!attn || S <= MEDP_TEMPORAL_USAGE_MAX_S) && (long long)C * K <= 65535,
                   "temporal_usage_summary: N=%d, S=%d or C*K=%lld beyond the limits (%d, %d, 65535)", N, S, (long long)C * K,
                   MEDP_TEMPORAL_USAGE_MAX_N, MEDP_TEMPORAL_USAGE_MAX_S);
    temporal_usage_summary_kernel<<<C * K, TU_THREADS, 0, (hipStream_t)stream>>>(fus, ts, attn, prob, sens, entropy, C, N, K, S);
    MEDP_LAUNCH_CHECK("medp_temporal_usage_summary");
    return 0;
}
