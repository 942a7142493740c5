// MFMA attention for SMALL head dims (dh <= 16) on gfx950: DuETT's event / time axis encoders — 2 heads of dim 12 over
// 49 / 97 tokens (257 at the stress shapes), dense, no mask (x_transformers Encoder as built at reference duett/duett.py:95-105,
// invoked at models/main_architecture_duett.py:81,91; dropout on the probabilities in training).  Operands are rounded to bf16 for
// the matrix cores like every other GEMM operand of the path; softmax / dropout / all sums in fp32.
//
// One WAVE per (batch, head, 16-row tile), no LDS, no barrier, nothing adds into memory (bitwise reproducible):
//   forward  (wave = 16 queries):  S^T = K Q^T per 16-key tile (A := K rows, B := Q rows; dh padded to 16 with zeros)
//                                  -> keys on the accumulator rows, the query on the lane column: a query's scores sit on the 4 lanes
//                                  l, l+16, l+32, l+48; softmax = per-lane max / sum over its 4 x NT scores + a 2-step butterfly over
//                                  those 4 lanes; O^T = V^T P^T: the exponentiated accumulators, packed to bf16, ARE the B operand
//                                  (same register layout), A := V^T -> a lane holds 4 consecutive head-dim outputs of its query.
//                                  Two bodies of this one algorithm (why: DESIGN.md): inference (fp32 q|k|v rows of the fused QKV GEMM
//                                  in, bf16 out; every K / V fragment fetched before the first MFMA) and training (fp32 or bf16 in and
//                                  out, dropout, the row's log2-sum-exp kept for the backward; fragments fetched inside the loops)
//   backward dQ (wave = 16 queries): P^T from the saved log-sum-exp, dP^T = V dO^T, delta = sum_j P dP (also stored),
//                                  dS^T = P (dP - delta) scale, dQ^T = K^T dS^T
//   backward dK, dV (wave = 16 keys): the transposed orientation S = Q K^T per query tile, P and dS from the saved statistics,
//                                  dV += P^T dO, dK += dS^T Q accumulated over the query tiles IN REGISTERS
// MFMA v_mfma_f32_16x16x16_bf16: A lane (row = lane & 15, k = 4 (lane >> 4) ..+3), B lane (col = lane & 15, same k),
// accumulator lane (rows 4 (lane >> 4) + r, col = lane & 15) — an accumulator tile, packed to bf16, is at once a B operand
// indexed (k = its rows, col) and an A operand indexed (row = its col, k = its rows): no transposition through LDS anywhere.
// Dropout: the counter hash of common.h on ((b H + h) N + query) N + key, as attention_small.hip.
// The fp32 VALU kernels these replace (attention_small.hip, a wave per query row) ran a 97-step dependent-load chain on 12 of 64
// lanes for P V: 73 us per inference forward at B=64, N=97 for 58 MFLOP, 20 us per training forward and 143 us per backward.
#include <type_traits>

#include "common.h"
#include "medp_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short bf16x4_t;

struct Dh16Params {
    const float* qkv;     // rows [B*N][ld]: q | k | v column blocks of H*dh each
    bf16_t* o;            // [B*N][ldo]
    int B, N, H, dh, ld, ldo;
    float scale_log2e;
};

struct TrainParams {
    const void* qkv;      // rows [B*N][ld]: q | k | v column blocks of H*dh each; fp32, or bf16 in the 16-bit hand-over form (T = bf16_t)
    int ld;
    void* o;              // forward: [B*N][ldo], same element type as qkv
    int ldo;
    float* lse;           // [B*H*N] log2-domain log-sum-exp of the scaled scores
    const void* dout;     // backward: [B*N][lddo], same element type as qkv
    int lddo;
    float* delta;         // [B*H*N] sum_j P dP
    void* dqkv;           // [B*N][lddqkv], same column blocks, same element type
    int lddqkv;
    int B, N, H, dh;
    float scale_log2e, scale, drop_p, inv_keep;
    uint32_t seed, stream_id;
    const uint32_t* epoch;
};

__device__ __forceinline__ bf16x4_t pack4(float a, float b, float c, float d) {
    union { bf16x4_t v; uint32_t u[2]; } p;
    p.u[0] = pack_bf2(a, b);
    p.u[1] = pack_bf2(c, d);
    return p.v;
}
__device__ __forceinline__ bf16x4_t pack4(const f32x4& v) { return pack4(v[0], v[1], v[2], v[3]); }

// row `row` of a [N][ld] block, elements 4 g4 ..+3 (an operand indexed (row | col = lane & 15, k = head dim)).  fp32 storage is rounded to
// bf16 here; bf16 storage (the hand-over form: the producing GEMM rounded with the same f2bf) is loaded as it is — the same operand bits
__device__ __forceinline__ bf16x4_t row_frag(const float* base, int ld, int row, int N, int g4, bool dvalid) {
    if (row >= N || !dvalid) return (bf16x4_t){0, 0, 0, 0};
    const float4 x = *(const float4*)(base + (size_t)row * ld + 4 * g4);
    return pack4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ bf16x4_t row_frag(const bf16_t* base, int ld, int row, int N, int g4, bool dvalid) {
    if (row >= N || !dvalid) return (bf16x4_t){0, 0, 0, 0};
    return *(const bf16x4_t*)(base + (size_t)row * ld + 4 * g4);
}
// column `col` of rows r0 ..+3 (an operand indexed (row | col = head dim lane & 15, k = token))
__device__ __forceinline__ bf16x4_t col_frag(const float* base, int ld, int r0, int N, int col, int dh) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (col < dh) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r0 + i < N) v[i] = base[(size_t)(r0 + i) * ld + col];
    }
    return pack4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ bf16x4_t col_frag(const bf16_t* base, int ld, int r0, int N, int col, int dh) {
    bf16x4_t v = {0, 0, 0, 0};
    if (col < dh) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r0 + i < N) v[i] = (short)base[(size_t)(r0 + i) * ld + col];
    }
    return v;
}
__device__ __forceinline__ void store4(float* dst, float a, float b, float c, float d) { *(float4*)dst = make_float4(a, b, c, d); }
__device__ __forceinline__ void store4(bf16_t* dst, float a, float b, float c, float d) { *(bf16x4_t*)dst = pack4(a, b, c, d); }
__device__ __forceinline__ void store1(float* dst, float a) { *dst = a; }
__device__ __forceinline__ void store1(bf16_t* dst, float a) { *dst = f2bf(a); }

__device__ __forceinline__ float keep_scale(const TrainParams& p, uint32_t seed, int bh, int q, int key) {
    return dropout_scale(seed, p.stream_id, ((uint32_t)bh * p.N + q) * p.N + key, p.drop_p, p.inv_keep);
}

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0)

// Inference forward.  The fragment loads are written out here, not through row_frag / col_frag, and all of them come before the first MFMA:
// the kernel is one chain of dependent memory round trips, and through the helpers the compiler puts one more wait into it at NT = 4, 7, 10
// (5.06 -> 5.46 us at B = 64, N = 97); with the loads inside the loops as in the training form, NT = 7 takes 81 VGPRs, not 60 (4 waves, not 8).
template <int NT>
__global__ __launch_bounds__(256) void attn_dh16_fwd_kernel(const Dh16Params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x * 4 + wave;                    // 16-query tile of this wave
    if (qt * 16 >= p.N) return;
    const int b = blockIdx.y / p.H, h = blockIdx.y % p.H;
    const int c16 = lane & 15, g4 = lane >> 4;               // column / 4-row group of the MFMA layouts
    const int D = p.H * p.dh;
    const float* base = p.qkv + (size_t)b * p.N * p.ld + h * p.dh;
    const bool dvalid = 4 * g4 < p.dh;                       // this lane's 4 head-dim slots exist (dh is a multiple of 4)

    // Q fragment (B operand of S^T): query c16, head dims 4 g4 .. 4 g4 + 3
    const int q = qt * 16 + c16;
    bf16x4_t qf = {0, 0, 0, 0};
    if (q < p.N && dvalid) {
        const float4 x = *(const float4*)(base + (size_t)q * p.ld + 4 * g4);
        qf = pack4(x.x, x.y, x.z, x.w);
    }
    // K fragments (A operand): key kt*16 + c16, head dims 4 g4 ..; V^T fragments (A operand of O^T): head dim c16, keys kt*16 + 4 g4 ..
    bf16x4_t kf[NT], vf[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const int key = kt * 16 + c16;
        kf[kt] = (bf16x4_t){0, 0, 0, 0};
        if (key < p.N && dvalid) {
            const float4 x = *(const float4*)(base + D + (size_t)key * p.ld + 4 * g4);
            kf[kt] = pack4(x.x, x.y, x.z, x.w);
        }
        float v4[4] = {0.f, 0.f, 0.f, 0.f};
        if (c16 < p.dh) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = kt * 16 + 4 * g4 + i;
                if (kk < p.N) v4[i] = base[2 * D + (size_t)kk * p.ld + c16];
            }
        }
        vf[kt] = pack4(v4[0], v4[1], v4[2], v4[3]);
    }
    // ---- S^T tiles ------------------------------------------------------------------------------------------------------
    f32x4 st[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        st[kt] = MFMA16(kf[kt], qf, ((f32x4){0.f, 0.f, 0.f, 0.f}));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (kt * 16 + 4 * g4 + r >= p.N) st[kt][r] = -INFINITY;      // padded keys
            mx = fmaxf(mx, st[kt][r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * p.scale_log2e;
    float sum = 0.f;
    bf16x4_t pf[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = __builtin_amdgcn_exp2f(fmaf(st[kt][r], p.scale_log2e, -mc));      // exp2(-inf) = 0 for the padded keys
            sum += e[r];
        }
        pf[kt] = pack4(e[0], e[1], e[2], e[3]);
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    // ---- O^T = V^T P^T ---------------------------------------------------------------------------------------------------
    f32x4 ot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) ot = MFMA16(vf[kt], pf[kt], ot);
    if (q < p.N && dvalid) {
        const float inv = 1.0f / sum;
        uint2 o;
        o.x = pack_bf2(ot[0] * inv, ot[1] * inv);
        o.y = pack_bf2(ot[2] * inv, ot[3] * inv);
        *(uint2*)(p.o + ((size_t)b * p.N + q) * p.ldo + h * p.dh + 4 * g4) = o;
    }
}

template <int NT, typename T>
__global__ __launch_bounds__(256) void dh16_train_fwd_kernel(const TrainParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x * 4 + wave;
    if (qt * 16 >= p.N) return;
    const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const int c16 = lane & 15, g4 = lane >> 4, D = p.H * p.dh;
    const T* base = (const T*)p.qkv + (size_t)b * p.N * p.ld + h * p.dh;
    const bool dvalid = 4 * g4 < p.dh;
    const int q = qt * 16 + c16;
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
    const bf16x4_t qf = row_frag(base, p.ld, q, p.N, g4, dvalid);
    f32x4 st[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        st[kt] = MFMA16(row_frag(base + D, p.ld, kt * 16 + c16, p.N, g4, dvalid), qf, ((f32x4){0.f, 0.f, 0.f, 0.f}));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (kt * 16 + 4 * g4 + r >= p.N) st[kt][r] = -INFINITY;
            mx = fmaxf(mx, st[kt][r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * p.scale_log2e;
    float sum = 0.f;
    f32x4 ot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = __builtin_amdgcn_exp2f(fmaf(st[kt][r], p.scale_log2e, -mc));
            sum += e[r];                                                           // the softmax normalises BEFORE the dropout
            const int key = kt * 16 + 4 * g4 + r;
            if (p.drop_p > 0.f && q < p.N && key < p.N) e[r] *= keep_scale(p, seed, bh, q, key);
        }
        ot = MFMA16(col_frag(base + 2 * D, p.ld, kt * 16 + 4 * g4, p.N, c16, p.dh), pack4(e[0], e[1], e[2], e[3]), ot);
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (q < p.N) {
        if (g4 == 0) p.lse[(size_t)bh * p.N + q] = mc + __log2f(sum);
        if (dvalid) {
            const float inv = 1.0f / sum;
            store4((T*)p.o + ((size_t)b * p.N + q) * p.ldo + h * p.dh + 4 * g4, ot[0] * inv, ot[1] * inv, ot[2] * inv, ot[3] * inv);
        }
    }
}

template <int NT, typename T>
__global__ __launch_bounds__(256) void dh16_train_bwd_dq_kernel(const TrainParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x * 4 + wave;
    if (qt * 16 >= p.N) return;
    const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const int c16 = lane & 15, g4 = lane >> 4, D = p.H * p.dh;
    const T* base = (const T*)p.qkv + (size_t)b * p.N * p.ld + h * p.dh;
    const T* dob = (const T*)p.dout + (size_t)b * p.N * p.lddo + h * p.dh;
    const bool dvalid = 4 * g4 < p.dh;
    const int q = qt * 16 + c16;
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
    const bf16x4_t qf = row_frag(base, p.ld, q, p.N, g4, dvalid), dof = row_frag(dob, p.lddo, q, p.N, g4, dvalid);
    const float lse = q < p.N ? p.lse[(size_t)bh * p.N + q] : 0.f;
    f32x4 pt[NT], dpt[NT];
    float delta = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        const f32x4 s = MFMA16(row_frag(base + D, p.ld, kt * 16 + c16, p.N, g4, dvalid), qf, ((f32x4){0.f, 0.f, 0.f, 0.f}));
        dpt[kt] = MFMA16(row_frag(base + 2 * D, p.ld, kt * 16 + c16, p.N, g4, dvalid), dof, ((f32x4){0.f, 0.f, 0.f, 0.f}));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = kt * 16 + 4 * g4 + r;
            const bool live = q < p.N && key < p.N;
            pt[kt][r] = live ? __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2e, -lse)) : 0.f;
            if (p.drop_p > 0.f && live) dpt[kt][r] *= keep_scale(p, seed, bh, q, key);
            delta += pt[kt][r] * dpt[kt][r];
        }
    }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
    f32x4 dq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = pt[kt][r] * (dpt[kt][r] - delta) * p.scale;
        dq = MFMA16(col_frag(base + D, p.ld, kt * 16 + 4 * g4, p.N, c16, p.dh), pack4(ds), dq);       // dQ^T += K^T dS^T
    }
    if (q < p.N) {
        if (g4 == 0) p.delta[(size_t)bh * p.N + q] = delta;
        if (dvalid) store4((T*)p.dqkv + ((size_t)b * p.N + q) * p.lddqkv + h * p.dh + 4 * g4, dq[0], dq[1], dq[2], dq[3]);
    }
}

template <int NT, typename T>
__global__ __launch_bounds__(256) void dh16_train_bwd_dkv_kernel(const TrainParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kt = blockIdx.x * 4 + wave;
    if (kt * 16 >= p.N) return;
    const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const int c16 = lane & 15, g4 = lane >> 4, D = p.H * p.dh;
    const T* base = (const T*)p.qkv + (size_t)b * p.N * p.ld + h * p.dh;
    const T* dob = (const T*)p.dout + (size_t)b * p.N * p.lddo + h * p.dh;
    const bool dvalid = 4 * g4 < p.dh;
    const int key = kt * 16 + c16;
    const uint32_t seed = p.drop_p > 0.f ? medp_mix_epoch(p.seed, p.epoch) : 0u;
    const bf16x4_t kb = row_frag(base + D, p.ld, key, p.N, g4, dvalid), vb = row_frag(base + 2 * D, p.ld, key, p.N, g4, dvalid);
    f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
        if (qt * 16 >= p.N) break;
        const int qrow = qt * 16 + c16;                                             // operand row of this lane
        const f32x4 s = MFMA16(row_frag(base, p.ld, qrow, p.N, g4, dvalid), kb, ((f32x4){0.f, 0.f, 0.f, 0.f}));       // S = Q K^T
        const f32x4 dp = MFMA16(row_frag(dob, p.lddo, qrow, p.N, g4, dvalid), vb, ((f32x4){0.f, 0.f, 0.f, 0.f}));      // dP = dO V^T
        f32x4 pm, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qt * 16 + 4 * g4 + r;                                     // accumulator row of this lane
            const bool live = q < p.N && key < p.N;
            const float pr = live ? __builtin_amdgcn_exp2f(fmaf(s[r], p.scale_log2e, -p.lse[(size_t)bh * p.N + q])) : 0.f;
            const float msk = (p.drop_p > 0.f && live) ? keep_scale(p, seed, bh, q, key) : 1.f;
            pm[r] = pr * msk;
            ds[r] = live ? pr * (dp[r] * msk - p.delta[(size_t)bh * p.N + q]) * p.scale : 0.f;
        }
        dv = MFMA16(pack4(pm), col_frag(dob, p.lddo, qt * 16 + 4 * g4, p.N, c16, p.dh), dv);          // dV += P^T dO
        dk = MFMA16(pack4(ds), col_frag(base, p.ld, qt * 16 + 4 * g4, p.N, c16, p.dh), dk);           // dK += dS^T Q
    }
    // the lane holds keys kt 16 + 4 g4 + r of head dim c16
    if (c16 < p.dh) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = kt * 16 + 4 * g4 + r;
            if (kk < p.N) {
                T* row = (T*)p.dqkv + ((size_t)b * p.N + kk) * p.lddqkv + h * p.dh + c16;
                store1(row + D, dk[r]);
                store1(row + 2 * D, dv[r]);
            }
        }
    }
}

// the shapes these kernels take.  `a` is read as 16-byte rows; `b2` needs `align2` bytes (the inference forward stores 8-byte pieces of
// bf16 o, everything else 16-byte ones).  The training kernels also index the dropout stream with 32 bits.
bool supported(int B, int N, int H, int dh, int ld, int ld2, const void* a, const void* b2, uintptr_t align2, bool train) {
    return dh <= 16 && dh % 4 == 0 && N <= 272 && ld % 4 == 0 && ld2 % 4 == 0 && (H * dh) % 4 == 0 && !((uintptr_t)a & 15) &&
           !((uintptr_t)b2 & (align2 - 1)) && (long long)B * H <= 65535 && (!train || (long long)B * H * N * N < (1ll << 32));
}

// f(std::integral_constant<int, NT>) for the smallest built NT >= nt 16-row tiles
template <typename F>
void with_nt(int nt, F f) {
    if (nt <= 2) f(std::integral_constant<int, 2>{});
    else if (nt <= 4) f(std::integral_constant<int, 4>{});
    else if (nt <= 7) f(std::integral_constant<int, 7>{});
    else if (nt <= 10) f(std::integral_constant<int, 10>{});
    else f(std::integral_constant<int, 17>{});
}

// one launch, a wave per 16-row tile; kernel_of(NT) names the instantiation
template <typename P, typename F>
void launch(const P& p, void* stream, F kernel_of) {
    const int nt = (p.N + 15) / 16;
    const dim3 grid((nt + 3) / 4, p.B * p.H);
    with_nt(nt, [&](auto NT) { kernel_of(NT)<<<grid, 256, 0, (hipStream_t)stream>>>(p); });
}

}  // namespace

// returns -2 when the shape is outside what this kernel is built for (the caller then takes medp_attn_small_fwd)
extern "C" int medp_attn_dh16_fwd(const float* qkv, int ld, void* o_bf16, int ldo, int B, int N, int H, int dh, float scale, void* stream) {
    MEDP_CHECK_ARG(qkv && o_bf16 && B > 0 && N > 0 && H > 0 && dh > 0, "attn_dh16_fwd: bad argument");
    if (!supported(B, N, H, dh, ld, ldo, qkv, o_bf16, 8, false)) return -2;
    MEDP_CHECK_ARG(ld >= 3 * H * dh && ldo >= H * dh && scale > 0.f, "attn_dh16_fwd: bad leading dimension / scale");
    Dh16Params p{qkv, (bf16_t*)o_bf16, B, N, H, dh, ld, ldo, scale * 1.4426950408889634f};
    launch(p, stream, [](auto NT) { return attn_dh16_fwd_kernel<decltype(NT)::value>; });
    MEDP_LAUNCH_CHECK("medp_attn_dh16_fwd");
    return 0;
}

extern "C" int medp_attn_dh16_train_supported(int B, int N, int H, int dh, int ld, int ldo) {
    return B > 0 && N > 0 && H > 0 && dh > 0 && ld >= 3 * H * dh && ldo >= H * dh && supported(B, N, H, dh, ld, ldo, nullptr, nullptr, 16, true) ? 1 : 0;
}

// returns -2 (nothing launched) for shapes these kernels are not built for: the caller then uses medp_attn_small_fwd / _bwd
extern "C" int medp_attn_dh16_train_fwd(const void* qkv, int ld, void* o, int ldo, float* lse, int io_bf16, int B, int N, int H, int dh,
                                        float scale, float dropout_p, unsigned seed, unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(qkv && o && lse && B > 0 && N > 0 && H > 0 && dh > 0, "attn_dh16_train_fwd: bad argument");
    MEDP_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f && scale > 0.f, "attn_dh16_train_fwd: dropout p / scale out of range");
    if (!supported(B, N, H, dh, ld, ldo, qkv, o, 16, true)) return -2;
    MEDP_CHECK_ARG(ld >= 3 * H * dh && ldo >= H * dh, "attn_dh16_train_fwd: bad leading dimension");
    TrainParams p{qkv, ld, o, ldo, lse, nullptr, 0, nullptr, nullptr, 0, B, N, H, dh, scale * 1.4426950408889634f, scale, dropout_p,
                  1.0f / (1.0f - dropout_p), seed, stream_id, medp_rng_epoch_ptr()};
    launch(p, stream, [&](auto NT) {
        return io_bf16 ? dh16_train_fwd_kernel<decltype(NT)::value, bf16_t> : dh16_train_fwd_kernel<decltype(NT)::value, float>;
    });
    MEDP_LAUNCH_CHECK("medp_attn_dh16_train_fwd");
    return 0;
}

// dqkv [B*N][lddqkv] receives dQ | dK | dV in the column blocks of qkv; delta_ws: B*H*N floats of scratch
extern "C" int medp_attn_dh16_train_bwd(const void* dout, int lddo, const void* qkv, int ld, const float* lse, float* delta_ws, void* dqkv,
                                        int lddqkv, int io_bf16, int B, int N, int H, int dh, float scale, float dropout_p, unsigned seed,
                                        unsigned stream_id, void* stream) {
    MEDP_CHECK_ARG(dout && qkv && lse && delta_ws && dqkv && B > 0 && N > 0 && H > 0 && dh > 0, "attn_dh16_train_bwd: bad argument");
    MEDP_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f && scale > 0.f, "attn_dh16_train_bwd: dropout p / scale out of range");
    if (!supported(B, N, H, dh, ld, lddo, qkv, dout, 16, true) || lddqkv % 4 != 0 || ((uintptr_t)dqkv & 15)) return -2;
    MEDP_CHECK_ARG(ld >= 3 * H * dh && lddqkv >= 3 * H * dh && lddo >= H * dh, "attn_dh16_train_bwd: bad leading dimension");
    TrainParams p{qkv, ld, nullptr, 0, (float*)lse, dout, lddo, delta_ws, dqkv, lddqkv, B, N, H, dh, scale * 1.4426950408889634f, scale,
                  dropout_p, 1.0f / (1.0f - dropout_p), seed, stream_id, medp_rng_epoch_ptr()};
    launch(p, stream, [&](auto NT) { return io_bf16 ? dh16_train_bwd_dq_kernel<decltype(NT)::value, bf16_t> : dh16_train_bwd_dq_kernel<decltype(NT)::value, float>; });
    MEDP_LAUNCH_CHECK("medp_attn_dh16_train_bwd(dq)");
    launch(p, stream, [&](auto NT) { return io_bf16 ? dh16_train_bwd_dkv_kernel<decltype(NT)::value, bf16_t> : dh16_train_bwd_dkv_kernel<decltype(NT)::value, float>; });
    MEDP_LAUNCH_CHECK("medp_attn_dh16_train_bwd(dk, dv)");
    return 0;
}
