// Few-query attention over ANY number of keys, split over workgroups (gfx950): the perceiver's cross blocks on large images
// (img_cross: <= 32 pathology queries over (image_size / 14)^2 patches — 1296 at 512^2, 2304 at 672^2), head dim 64, fp32.
// The one-workgroup kernels of attention_small.hip hold every key of a (batch, head) in one workgroup (<= 1024 keys); here the keys
// are cut into slices of FQ_T = 256 and each slice is a workgroup of its own, the thread-per-key scheme of attention_small.hip on it:
//   forward   attn_fqs_fwd_kernel      grid (B*H, slices, query groups of 8): scores of the slice's keys, the slice's max m and sum
//                                      l per query and the unnormalised sum_j e_j mask_j V_j -> workspace
//             attn_fqs_combine_kernel  merges the slices in ascending order -> o (fp32 / bf16) and lse = m + log l (natural log)
//             attn_fqs_avg_kernel      (optional) the head average of the post-dropout probabilities from lse, each element once
//   backward  attn_fqs_bwd_kernel      grid (B*H, slices): delta_q = <dO_q, O_q>, P = exp(s - lse) recomputed, the key's thread
//                                      writes its dK / dV rows whole (sum over all queries), the slice's partial dQ -> workspace
//             attn_fqs_dq_kernel       sums the slices' dQ in ascending order
// The bound is HBM traffic, not arithmetic (B 32, Lk 1296, 7 queries: 0.3 GFLOP against 85 MB of K / V in the forward, 170 MB of
// K, V, dK, dV in the backward), so fp32 VALU math with K and V read once per query group, no matrix cores.  No atomics (bitwise
// reproducible), no allocation or host synchronisation (the caller owns the workspace: graph-capturable).  Dropout: the mask
// stream of attention_small.hip, element ((b*H + h)*Lq + q)*Lk + j, so every kernel here and there draws the same mask.
#include <stdint.h>

#include "attention_fq.h"
#include "common.h"
#include "medp_hip.h"

namespace {

constexpr int FQS_MAXQ = 32;                    // queries (four groups of FQ)
constexpr int FQS_ML = 2;                       // (m, l) per (slice, query) in the forward workspace

struct FqsParams {
    const float *q, *k, *v;
    int ldq, ldkv;
    long long q_bs, kv_bs;                      // batch strides in elements
    int B, Lq, Lk, H, nsplit;
    float scale, drop_p, inv_keep;
    uint32_t seed, stream_id;
    const uint32_t* epoch;
};

// s[q] = <Q_q, K_j> for the FQ query rows in LDS (sQ[q * 64 + d]) and this thread's key row (16-B aligned, 64 floats), in the
// summation order of fq_probs (attention_small.hip)
__device__ __forceinline__ void fqs_scores(const float* sQ, const float* krow, float (&s)[FQ]) {
    const float4* kr = (const float4*)krow;
    float4 kv[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) kv[d] = kr[d];
#pragma unroll
    for (int q = 0; q < FQ; ++q) s[q] = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const float* sq = FQ_OPAQUE(sQ + d * 4);
#pragma unroll
        for (int q = 0; q < FQ; ++q) {
            const float4 x = *(const float4*)(sq + q * 64);
            s[q] += (x.x * kv[d].x + x.y * kv[d].y) + (x.z * kv[d].z + x.w * kv[d].w);
            asm volatile("" : "+v"(s[q]));          // the step's sums are formed here, not sunk past later steps into a use
        }
        FQ_KEEP_IN_STEP();
    }
}

__device__ __forceinline__ float fqs_mask(const FqsParams& p, uint32_t seed, int bh, int q, int j) {
    return p.drop_p > 0.f ? dropout_scale(seed, p.stream_id, ((uint32_t)bh * p.Lq + q) * p.Lk + j, p.drop_p, p.inv_keep) : 1.f;
}

// workspace layout (floats): forward  O[B*H][nsplit][Lq][64], then ml[B*H][nsplit][Lq][2];  backward  dQ[B*H][nsplit][Lq][64]
__host__ __device__ __forceinline__ size_t fqs_rows(int B, int H, int Lq, int nsplit) { return (size_t)B * H * nsplit * Lq; }

__global__ __launch_bounds__(FQ_T) void attn_fqs_fwd_kernel(const FqsParams p, float* __restrict__ ws) {
    __shared__ float sQ[FQ * 64];
    __shared__ float red[4 * FQ];
    __shared__ float sP[FQ * FQ_T];
    __shared__ float sR[16 * FQ * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, split = blockIdx.y, q0 = blockIdx.z * FQ;
    const int b = bh / p.H, h = bh % p.H;
    const int j0 = split * FQ_T, j = j0 + tid, nk = min(FQ_T, p.Lk - j0), nq = min(FQ, p.Lq - q0);
    const bool live = tid < nk;
    const float* kbase = p.k + (size_t)b * p.kv_bs + h * 64;
    const float* vbase = p.v + (size_t)b * p.kv_bs + h * 64;
    for (int t = tid; t < FQ * 64; t += FQ_T) {
        const int q = t >> 6, d = t & 63;
        sQ[t] = q < nq ? p.q[(size_t)b * p.q_bs + (size_t)(q0 + q) * p.ldq + h * 64 + d] : 0.f;
    }
    __syncthreads();
    float s[FQ], m[FQ], l[FQ];
    if (live) {
        fqs_scores(sQ, kbase + (size_t)j * p.ldkv, s);
    }
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        s[q] = live ? s[q] * p.scale : -INFINITY;
        m[q] = s[q];
    }
    fq_block_reduce(m, red, lane, wave, true);            // every slice holds >= 1 live key: m is finite
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        s[q] = live ? __expf(s[q] - m[q]) : 0.f;
        l[q] = s[q];
    }
    fq_block_reduce(l, red, lane, wave, false);
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
#pragma unroll
    for (int q = 0; q < FQ; ++q) sP[q * FQ_T + tid] = (live && q < nq) ? s[q] * fqs_mask(p, seed, bh, q0 + q, j) : 0.f;
    __syncthreads();
    const size_t row0 = ((size_t)bh * p.nsplit + split) * p.Lq + q0;          // this workgroup's first (slice, query) row
    fq_weighted_rows(sP, FQ_T, vbase + (size_t)j0 * p.ldkv, p.ldkv, nk, nq, sR, tid, ws + row0 * 64, 64);
    float* ml = ws + fqs_rows(p.B, p.H, p.Lq, p.nsplit) * 64 + row0 * FQS_ML;
#pragma unroll
    for (int q = 0; q < FQ; ++q) {
        if (tid == q && q < nq) {
            ml[q * FQS_ML] = m[q];
            ml[q * FQS_ML + 1] = l[q];
        }
    }
}

// thread = (batch-head-query row, d): o = sum_s O_s e^(m_s - M) / sum_s l_s e^(m_s - M), slices in ascending order
__global__ __launch_bounds__(64) void attn_fqs_combine_kernel(const FqsParams p, const float* __restrict__ ws, void* __restrict__ o,
                                                             int ldo, int o_bf16, float* __restrict__ lse) {
    const int row = blockIdx.x, d = threadIdx.x;                           // row = bh * Lq + q
    const int bh = row / p.Lq, q = row % p.Lq, b = bh / p.H, h = bh % p.H;
    const float* O = ws + ((size_t)bh * p.nsplit * p.Lq + q) * 64 + d;
    const float* ml = ws + fqs_rows(p.B, p.H, p.Lq, p.nsplit) * 64 + ((size_t)bh * p.nsplit * p.Lq + q) * FQS_ML;
    const size_t st = (size_t)p.Lq;                                        // rows from one slice to the next
    float M = -INFINITY;
    for (int s = 0; s < p.nsplit; ++s) M = fmaxf(M, ml[s * st * FQS_ML]);
    float L = 0.f, acc = 0.f;
    for (int s = 0; s < p.nsplit; ++s) {
        const float f = __expf(ml[s * st * FQS_ML] - M);
        L += ml[s * st * FQS_ML + 1] * f;
        acc += O[s * st * 64] * f;
    }
    const float r = acc / L;
    const size_t oi = ((size_t)b * p.Lq + q) * ldo + h * 64 + d;
    if (o_bf16) ((bf16_t*)o)[oi] = f2bf(r); else ((float*)o)[oi] = r;
    if (d == 0) lse[row] = M + __logf(L);
}

// attn_avg[b][q][j] = (1/H) sum_h P_bhqj mask_bhqj (nn.MultiheadAttention's need_weights / average_attn_weights): grid (B, slices,
// query groups), thread = key; heads summed in ascending order, every element written once
__global__ __launch_bounds__(FQ_T) void attn_fqs_avg_kernel(const FqsParams p, const float* __restrict__ lse, float* __restrict__ attn_avg) {
    __shared__ float sQ[FQ * 64];
    const int tid = threadIdx.x, b = blockIdx.x, q0 = blockIdx.z * FQ;
    const int j = blockIdx.y * FQ_T + tid, nq = min(FQ, p.Lq - q0);
    const bool live = j < p.Lk;
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
    const float inv_h = 1.0f / (float)p.H;
    float acc[FQ];
#pragma unroll
    for (int q = 0; q < FQ; ++q) acc[q] = 0.f;
    for (int h = 0; h < p.H; ++h) {
        __syncthreads();                                                   // sQ of the previous head is no longer read
        for (int t = tid; t < FQ * 64; t += FQ_T) {
            const int q = t >> 6, d = t & 63;
            sQ[t] = q < nq ? p.q[(size_t)b * p.q_bs + (size_t)(q0 + q) * p.ldq + h * 64 + d] : 0.f;
        }
        __syncthreads();
        if (live) {
            float s[FQ];
            fqs_scores(sQ, p.k + (size_t)b * p.kv_bs + (size_t)j * p.ldkv + h * 64, s);
            const int bh = b * p.H + h;
#pragma unroll
            for (int q = 0; q < FQ; ++q) {
                if (q < nq) {
                    const float w = __expf(s[q] * p.scale - lse[(size_t)bh * p.Lq + q0 + q]) * fqs_mask(p, seed, bh, q0 + q, j);
                    acc[q] += w * inv_h;
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int q = 0; q < FQ; ++q)
            if (q < nq) attn_avg[((size_t)b * p.Lq + q0 + q) * p.Lk + j] = acc[q];
    }
}

// Backward of one (batch-head, key slice), all Lq <= 32 queries in groups of FQ.  LDS (NQ = Lq rounded up to FQ):
// sQ, sDO [NQ][64], sPM (P * mask), sS (dS * scale) [NQ][FQ_T], sR [16][FQ][64], lse / delta [NQ]
__global__ __launch_bounds__(FQ_T) void attn_fqs_bwd_kernel(const FqsParams p, const float* __restrict__ dout, int lddo,
                                                            const float* __restrict__ o, int ldo, const float* __restrict__ lse,
                                                            float* __restrict__ dk, float* __restrict__ dv, int lddkv, long long dkv_bs,
                                                            float* __restrict__ ws) {
    extern __shared__ float sm[];
    const int NQ = (p.Lq + FQ - 1) / FQ * FQ;
    float* sQ = sm;
    float* sDO = sQ + NQ * 64;
    float* sPM = sDO + NQ * 64;
    float* sS = sPM + NQ * FQ_T;
    float* sR = sS + NQ * FQ_T;
    float* sLse = sR + 16 * FQ * 64;
    float* sDelta = sLse + NQ;
    const int tid = threadIdx.x;
    const int bh = blockIdx.x, split = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const int j0 = split * FQ_T, j = j0 + tid, nk = min(FQ_T, p.Lk - j0);
    const bool live = tid < nk;
    const float* kbase = p.k + (size_t)b * p.kv_bs + h * 64;
    const float* vbase = p.v + (size_t)b * p.kv_bs + h * 64;
    for (int t = tid; t < NQ * 64; t += FQ_T) {
        const int q = t >> 6, d = t & 63;
        sQ[t] = q < p.Lq ? p.q[(size_t)b * p.q_bs + (size_t)q * p.ldq + h * 64 + d] : 0.f;
        sDO[t] = q < p.Lq ? dout[((size_t)b * p.Lq + q) * lddo + h * 64 + d] : 0.f;
    }
    // delta_q = <dO_q, O_q> (= sum_j P_j dP_j with the dropout mask inside dP): 8 lanes per query, 8 columns each, fixed order
    {
        const int q = tid >> 3, part = tid & 7;
        float a = 0.f;
        if (q < p.Lq) {
            const float* orow = o + ((size_t)b * p.Lq + q) * ldo + h * 64 + part * 8;
            const float* drow = dout + ((size_t)b * p.Lq + q) * lddo + h * 64 + part * 8;
#pragma unroll
            for (int d = 0; d < 8; ++d) a += drow[d] * orow[d];
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) a += __shfl_xor(a, off, 64);
        if (part == 0 && q < NQ) {
            sDelta[q] = a;
            sLse[q] = q < p.Lq ? lse[(size_t)bh * p.Lq + q] : 0.f;
        }
    }
    __syncthreads();
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
    // per query group: P recomputed from lse, dP = <dO, V_j> mask, dS = P (dP - delta) scale -> this key's column of sPM / sS
    for (int g = 0; g < NQ; g += FQ) {
        float pm[FQ], ds[FQ];
#pragma unroll
        for (int q = 0; q < FQ; ++q) pm[q] = ds[q] = 0.f;
        if (live) {
            float s[FQ], dp[FQ];
            fqs_scores(sQ + g * 64, kbase + (size_t)j * p.ldkv, s);
            fqs_scores(sDO + g * 64, vbase + (size_t)j * p.ldkv, dp);
#pragma unroll
            for (int q = 0; q < FQ; ++q) {
                if (g + q < p.Lq) {
                    const float P = __expf(s[q] * p.scale - sLse[g + q]);
                    const float msk = fqs_mask(p, seed, bh, g + q, j);
                    pm[q] = P * msk;
                    ds[q] = P * (dp[q] * msk - sDelta[g + q]) * p.scale;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < FQ; ++q) {
            sPM[(g + q) * FQ_T + tid] = pm[q];
            sS[(g + q) * FQ_T + tid] = ds[q];
        }
    }
    // this key's dV row = sum_q (P mask)_q dO_q and dK row = sum_q dS_q Q_q over ALL queries (own LDS column: no barrier needed)
    if (live) {
        const float* wsrc[2] = {sPM, sS};
        const float* rsrc[2] = {sDO, sQ};
        float* dst[2] = {dv + (size_t)b * dkv_bs + (size_t)j * lddkv + h * 64, dk + (size_t)b * dkv_bs + (size_t)j * lddkv + h * 64};
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            float4 acc[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) acc[d] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q = 0; q < p.Lq; ++q) {
                const float w = wsrc[which][q * FQ_T + tid];
                const float* r = FQ_OPAQUE(rsrc[which] + q * 64);
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const float4 x = *(const float4*)(r + d * 4);
                    acc[d].x += w * x.x; acc[d].y += w * x.y; acc[d].z += w * x.z; acc[d].w += w * x.w;
                }
            }
            float4* out = (float4*)dst[which];
#pragma unroll
            for (int d = 0; d < 16; ++d) out[d] = acc[d];
        }
    }
    __syncthreads();
    // the slice's partial dQ = sum_j dS_j K_j, one query group at a time
    const size_t row0 = ((size_t)bh * p.nsplit + split) * p.Lq;
    for (int g = 0; g < p.Lq; g += FQ) {
        fq_weighted_rows(sS + g * FQ_T, FQ_T, kbase + (size_t)j0 * p.ldkv, p.ldkv, nk, min(FQ, p.Lq - g), sR, tid, ws + (row0 + g) * 64, 64);
        __syncthreads();                                                   // sR is written again by the next group
    }
}

// dq[b][q][h*64 + d] = sum_s dQ_s, slices in ascending order
__global__ __launch_bounds__(64) void attn_fqs_dq_kernel(const FqsParams p, const float* __restrict__ ws, float* __restrict__ dq, int lddq) {
    const int row = blockIdx.x, d = threadIdx.x;
    const int bh = row / p.Lq, q = row % p.Lq, b = bh / p.H, h = bh % p.H;
    const float* src = ws + ((size_t)bh * p.nsplit * p.Lq + q) * 64 + d;
    float a = 0.f;
    for (int s = 0; s < p.nsplit; ++s) a += src[(size_t)s * p.Lq * 64];
    dq[((size_t)b * p.Lq + q) * lddq + h * 64 + d] = a;
}

size_t bwd_lds_bytes(int Lq) {
    const int NQ = (Lq + FQ - 1) / FQ * FQ;
    return (size_t)(2 * NQ * 64 + 2 * NQ * FQ_T + 16 * FQ * 64 + 2 * NQ) * sizeof(float);
}

int check(const FqsParams& p, int dh, const char* who) {
    MEDP_CHECK_ARG(p.q && p.k && p.v, "%s: null operand", who);
    MEDP_CHECK_ARG(p.B > 0 && p.Lq > 0 && p.Lk > 0 && p.H > 0, "%s: bad shape", who);
    MEDP_CHECK_ARG(dh == 64, "%s: head dim %d != 64", who, dh);
    MEDP_CHECK_ARG(p.Lq <= FQS_MAXQ, "%s: Lq %d > %d", who, p.Lq, FQS_MAXQ);
    MEDP_CHECK_ARG((unsigned long long)p.B * p.H * p.Lq * p.Lk <= 0x100000000ull,
                   "%s: dropout element index ((b*H + h)*Lq + q)*Lk + j does not fit in 32 bits", who);
    MEDP_CHECK_ARG(p.drop_p >= 0.f && p.drop_p < 1.f, "%s: dropout p out of range", who);
    MEDP_CHECK_ARG((p.ldkv & 3) == 0 && (p.kv_bs & 3) == 0 && ((((uintptr_t)p.k | (uintptr_t)p.v) & 15) == 0),
                   "%s: K / V rows must be 16-byte aligned", who);
    return 0;
}

FqsParams make_params(const float* q, int ldq, long long q_bs, const float* k, const float* v, int ldkv, long long kv_bs, int B, int Lq,
                      int Lk, int H, float scale, float p, unsigned seed, unsigned stream_id) {
    return FqsParams{q, k, v, ldq, ldkv, q_bs, kv_bs, B, Lq, Lk, H, (Lk + FQ_T - 1) / FQ_T, scale, p, 1.0f / (1.0f - p), seed, stream_id,
                     medp_rng_epoch_ptr()};
}

}  // namespace

extern "C" size_t medp_attn_fq_split_ws_bytes(int B, int H, int Lq, int Lk, int bwd) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return 0;
    const size_t rows = fqs_rows(B, H, Lq, (Lk + FQ_T - 1) / FQ_T);
    return rows * (bwd ? 64 : 64 + FQS_ML) * sizeof(float);
}

extern "C" int medp_attn_fq_split_fwd(const float* q, int ldq, long long q_batch_stride, const float* k, const float* v, int ldkv,
                                      long long kv_batch_stride, void* o, int ldo, int o_bf16, float* lse, float* attn_avg, float* ws,
                                      size_t ws_bytes, int B, int Lq, int Lk, int H, int dh, float scale, float dropout_p, unsigned seed,
                                      unsigned stream_id, void* stream) {
    const FqsParams p = make_params(q, ldq, q_batch_stride, k, v, ldkv, kv_batch_stride, B, Lq, Lk, H, scale, dropout_p, seed, stream_id);
    MEDP_TRY(check(p, dh, "attn_fq_split_fwd"));
    MEDP_CHECK_ARG(o && lse && ws, "attn_fq_split_fwd: null output or workspace");
    MEDP_CHECK_ARG(ws_bytes >= medp_attn_fq_split_ws_bytes(B, H, Lq, Lk, 0), "attn_fq_split_fwd: workspace of %zu bytes < %zu", ws_bytes,
                   medp_attn_fq_split_ws_bytes(B, H, Lq, Lk, 0));
    hipStream_t st = (hipStream_t)stream;
    const int ngroups = (Lq + FQ - 1) / FQ;
    attn_fqs_fwd_kernel<<<dim3(B * H, p.nsplit, ngroups), FQ_T, 0, st>>>(p, ws);
    MEDP_LAUNCH_CHECK("medp_attn_fq_split_fwd(slices)");
    attn_fqs_combine_kernel<<<B * H * Lq, 64, 0, st>>>(p, ws, o, ldo, o_bf16, lse);
    MEDP_LAUNCH_CHECK("medp_attn_fq_split_fwd(combine)");
    if (attn_avg) {
        attn_fqs_avg_kernel<<<dim3(B, p.nsplit, ngroups), FQ_T, 0, st>>>(p, lse, attn_avg);
        MEDP_LAUNCH_CHECK("medp_attn_fq_split_fwd(head average)");
    }
    return 0;
}

extern "C" int medp_attn_fq_split_bwd(const float* dout, int lddo, const float* o, int ldo, const float* lse, const float* q, int ldq,
                                      long long q_batch_stride, const float* k, const float* v, int ldkv, long long kv_batch_stride,
                                      float* dq, int lddq, float* dk, float* dv, int lddkv, long long dkv_batch_stride, float* ws,
                                      size_t ws_bytes, int B, int Lq, int Lk, int H, int dh, float scale, float dropout_p, unsigned seed,
                                      unsigned stream_id, void* stream) {
    const FqsParams p = make_params(q, ldq, q_batch_stride, k, v, ldkv, kv_batch_stride, B, Lq, Lk, H, scale, dropout_p, seed, stream_id);
    MEDP_TRY(check(p, dh, "attn_fq_split_bwd"));
    MEDP_CHECK_ARG(dout && o && lse && dq && dk && dv && ws, "attn_fq_split_bwd: null operand, gradient or workspace");
    MEDP_CHECK_ARG((lddkv & 3) == 0 && (dkv_batch_stride & 3) == 0 && ((((uintptr_t)dk | (uintptr_t)dv) & 15) == 0),
                   "attn_fq_split_bwd: dK / dV rows must be 16-byte aligned");
    MEDP_CHECK_ARG(ws_bytes >= medp_attn_fq_split_ws_bytes(B, H, Lq, Lk, 1), "attn_fq_split_bwd: workspace of %zu bytes < %zu", ws_bytes,
                   medp_attn_fq_split_ws_bytes(B, H, Lq, Lk, 1));
    hipStream_t st = (hipStream_t)stream;
    MEDP_ONCE_PER_DEVICE({ hipFuncSetAttribute((const void*)attn_fqs_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    attn_fqs_bwd_kernel<<<dim3(B * H, p.nsplit), FQ_T, bwd_lds_bytes(Lq), st>>>(p, dout, lddo, o, ldo, lse, dk, dv, lddkv, dkv_batch_stride, ws);
    MEDP_LAUNCH_CHECK("medp_attn_fq_split_bwd(slices)");
    attn_fqs_dq_kernel<<<B * H * Lq, 64, 0, st>>>(p, ws, dq, lddq);
    MEDP_LAUNCH_CHECK("medp_attn_fq_split_bwd(dq)");
    return 0;
}
