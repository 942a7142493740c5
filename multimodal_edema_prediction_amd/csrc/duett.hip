// DuETT (dual-axis event x time transformer) encode path for gfx950, inference form (BatchNorm folded to an affine):
//   DuettFeatureExtractor.encode, reference models/main_architecture_duett.py:31-94 (== duett/duett.py:245-280).
//
// The embedding stage (duett_embed.hip) builds psi [B, T+1, V+1, E] directly in the event view, and the time embedding.
// The layer loop alternates the two token views of psi
//     event view [B, V+1, (T+1)E]  <->  time view [B, T+1, (V+1)E]
// through "axis swap + add" kernels that move whole E-float (96 B) cells with 16-B accesses and fuse the positional
// add and the preceding encoder's final ScaleNorm scaling (per-row 1/||x||), so psi makes one HBM round trip per swap.
// Each encoder (x_transformers Encoder(depth=1), restated in oracle/xt_encoder.py) is
//     x += to_out(attn(ScaleNorm(x)));  x += ff2(gelu(ff1(ScaleNorm(x))));  [x = ScaleNorm(x)]
// with ScaleNorm emitting bf16 straight into the MFMA GEMMs and both residual adds fused in GEMM epilogues.
#include "common.h"
#include "duett_front.h"
#include "medp_hip.h"
#include "norm_rows.h"

namespace {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- axis swaps (K7): cells of E floats move between [B, A1, A2, E] and [B, A2, A1, E] ------------------------------------
// out[b][a2][a1][:] = in[b][a1][a2][:] * rowscale(b, a1) + add        add: either per-(a2,a1,e) table (event embedding,
// batch-invariant, add_bs = 0) or per-(b,a2,a1,e) tensor (time embedding, add_bs = A2*A1*E).  rowscale = rnorm * gain
// applies the producing encoder's final ScaleNorm (row = one (b, a1) token of A2*E features); rnorm == nullptr -> 1.
__global__ __launch_bounds__(256) void axis_swap_add_kernel(const float* __restrict__ in, const float* __restrict__ rnorm,
                                                            const float* __restrict__ g, float gain_sqrt_dim,
                                                            const float* __restrict__ add, long long add_bs,
                                                            float* __restrict__ out, int B, int A1, int A2, int E4) {
    // 32-bit index arithmetic (the launcher checks B*A1*A2*E4 < 2^31): the 64-bit divisions of the first version cost more than
    // the memory traffic (33 us for 87 MB)
    const unsigned total = (unsigned)B * A1 * A2 * E4;
    const float gain = rnorm ? gain_sqrt_dim * g[0] : 1.f;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        // iterate in OUTPUT order (coalesced writes): i = ((b*A2 + a2)*A1 + a1)*E4 + e4
        const int e4 = (int)(i % (unsigned)E4);
        unsigned r = i / (unsigned)E4;
        const int a1 = (int)(r % (unsigned)A1);
        r /= (unsigned)A1;
        const int a2 = (int)(r % (unsigned)A2);
        const int b = (int)(r / (unsigned)A2);
        const float4 v = *(const float4*)(in + ((((size_t)b * A1 + a1) * A2 + a2) * E4 + e4) * 4);
        const float sc = rnorm ? rnorm[(size_t)b * A1 + a1] * gain : 1.f;
        const float4 ad = *(const float4*)(add + (size_t)b * add_bs + (((size_t)a2 * A1 + a1) * E4 + e4) * 4);
        *(float4*)(out + (size_t)i * 4) = make_float4(v.x * sc + ad.x, v.y * sc + ad.y, v.z * sc + ad.z, v.w * sc + ad.w);
    }
}

// ---- axis swap + positional add + the NEXT encoder's first ScaleNorm in one pass (wave per output row, row in registers) --------
// x[b][a2][a1][:] = in[b][a1][a2][:] * rowscale(b, a1) + add ;  h = ScaleNorm(x) as bf16.  One read of psi, one fp32 + one bf16
// write, instead of swap (read + write) then ScaleNorm (read + write).  The row holder and the ScaleNorm tail are those of
// scalenorm_fwd_reg_kernel (norm_rows.h): bit-identical.
template <int NV>
__global__ __launch_bounds__(256) void swap_add_norm_kernel(const float* __restrict__ in, const float* __restrict__ rnorm,
                                                            const float* __restrict__ g_prev, float gain_sqrt_dim,
                                                            const float* __restrict__ add, long long add_bs,
                                                            const float* __restrict__ g_norm, float norm_eps, float* __restrict__ x_out,
                                                            bf16_t* __restrict__ h_out, int B, int A1, int A2, int E4) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * A2) return;
    const int b = row / A2, a2 = row - b * A2;
    const int D = A1 * E4 * 4;
    const float gain = rnorm ? gain_sqrt_dim * g_prev[0] : 1.f;
    const float* addr = add + (size_t)b * add_bs + (size_t)a2 * D;
    float* xrow = x_out + (size_t)row * D;
    const RowRegs<NV> x(lane, D, [&](int i) {
        const int a1 = i / E4, e4 = i - a1 * E4;
        const float4 s = *(const float4*)(in + ((((size_t)b * A1 + a1) * A2 + a2) * E4 + e4) * 4);
        const float sc = rnorm ? rnorm[(size_t)b * A1 + a1] * gain : 1.f;
        const float4 ad = *(const float4*)(addr + 4 * i);
        const float4 v = make_float4(s.x * sc + ad.x, s.y * sc + ad.y, s.z * sc + ad.z, s.w * sc + ad.w);
        *(float4*)(xrow + 4 * i) = v;
        return v;
    });
    scalenorm_fwd_row<true>(x, g_norm, norm_eps, h_out, D, nullptr, row);
}

int launch_swap_add_norm(const float* in, const float* rnorm, const float* g_prev, float gain_sqrt_dim, const float* add, long long add_bs,
                         const float* g_norm, float norm_eps, float* x_out, void* h_out, int B, int A1, int A2, int E4, hipStream_t s) {
    const int nv = (A1 * E4 + 63) / 64, grid = (B * A2 + 3) / 4;
    if (!dispatch_nv<5, 10, 16, 25>(nv, [&](auto NV) {
            swap_add_norm_kernel<decltype(NV)::value><<<grid, 256, 0, s>>>(in, rnorm, g_prev, gain_sqrt_dim, add, add_bs, g_norm, norm_eps, x_out,
                                                                          (bf16_t*)h_out, B, A1, A2, E4);
        }))
        return 1;          // wider rows: the caller takes the two-launch path
    MEDP_LAUNCH_CHECK("duett swap+add+norm");
    return 0;
}

// `src` [B, A1, A2, E] to the other view: x = swap(src * pending row scale) + add.  rn (may be null) / g_prev: the pending final
// ScaleNorm of the encoder that produced src; add / add_bs as in the kernels above; g_norm: the gain of the first ScaleNorm of the
// encoder that takes x.  *h_ready: that ScaleNorm is in `h` already (one pass); false for rows the fused kernel is not built for,
// where x alone is written and the encoder norms it itself.
int swap_view(const float* src, const float* rn, const float* g_prev, const float* add, long long add_bs, const float* g_norm, float norm_eps,
              float* x, void* h, int B, int A1, int A2, int E4, hipStream_t s, bool* h_ready) {
    const float gain_sqrt_dim = sqrtf((float)(A2 * E4 * 4));
    const int rc = launch_swap_add_norm(src, rn, g_prev, gain_sqrt_dim, add, add_bs, g_norm, norm_eps, x, h, B, A1, A2, E4, s);
    *h_ready = rc == 0;
    if (rc != 1) return rc;
    axis_swap_add_kernel<<<grid_for((size_t)B * A1 * A2 * E4), 256, 0, s>>>(src, rn, g_prev, gain_sqrt_dim, add, add_bs, x, B, A1, A2, E4);
    MEDP_LAUNCH_CHECK("duett swap");
    return 0;
}

struct DuettWs {
    size_t xe, xt, temb, h, qkv, o, f, rn, split, split_bytes, total;
};
DuettWs plan(const MedpDuettWeights* w, int B, int T) {
    const size_t V1 = w->n_vars + 1, T1 = T + 1, E = w->d_embedding;
    const size_t cells = (size_t)B * T1 * V1 * E;
    const size_t rows = (size_t)B * max(T1, V1);
    DuettWs s{};
    size_t off = 0;
    s.xe = off;   off += al(cells * 4);
    s.xt = off;   off += al(cells * 4);
    s.temb = off; off += al(cells * 4);
    s.h = off;    off += al(cells * 2);
    s.qkv = off;  off += al(rows * 3 * E * 4);
    s.o = off;    off += al(rows * E * 2);
    s.f = off;    off += al(rows * (size_t)w->d_ff * 2);
    s.rn = off;   off += al(rows * 4);
    // split-K partial sums of the skinny GEMMs (medp_gemm_bf16_nt_ws): the largest need over both axes' four shapes
    size_t sp = 0;
    for (int axis = 0; axis < 2; ++axis) {
        const int M = (int)(B * (axis ? T1 : V1)), D = (int)(E * (axis ? V1 : T1));
        sp = max(sp, medp_gemm_nt_workspace_bytes(M, 3 * (int)E, D));
        sp = max(sp, medp_gemm_nt_workspace_bytes(M, D, (int)E));
        sp = max(sp, medp_gemm_nt_workspace_bytes(M, w->d_ff, D));
        sp = max(sp, medp_gemm_nt_workspace_bytes(M, D, w->d_ff));
    }
    s.split = off; s.split_bytes = sp; off += al(sp);
    s.total = off;
    return s;
}

// one x_transformers encoder block on x [M = B*N tokens, D] (in place); leaves the FINAL ScaleNorm to the caller
int encoder_forward(const MedpEncoderWeights& e, const MedpDuettWeights* w, float* x, int B, int N, int D, char* base,
                    const DuettWs& ws, void* stream, bool h_ready) {
    const int M = B * N, E = w->d_embedding, H = w->n_heads, dh = E / H;
    void* h = base + ws.h;
    float* qkv = (float*)(base + ws.qkv);
    void* o = base + ws.o;
    void* f = base + ws.f;
    float* sp = (float*)(base + ws.split);
    if (!h_ready)      // else: the producer of x (embed / swap kernel) has written ScaleNorm(x) to ws.h already
        MEDP_TRY(medp_scalenorm_fwd(x, D, e.g_attn, h, D, 1, nullptr, M, D, w->norm_eps, stream));
    MEDP_TRY(medp_gemm_bf16_nt_ws(h, e.qkv_w, qkv, M, 3 * E, D, D, D, 3 * E, nullptr, nullptr, nullptr, 0, 0, 0, sp, ws.split_bytes, stream));
    // both axes' attention on the matrix cores (attention_dh16.hip); shapes it is not built for take the fp32 VALU kernel
    static const bool mfma_attn = medp_env_int("MEDP_DUETT_MFMA_ATTN", 1) != 0;
    int arc = mfma_attn ? medp_attn_dh16_fwd(qkv, 3 * E, o, E, B, N, H, dh, 1.0f / sqrtf((float)dh), stream) : -2;
    if (arc == -2)
        arc = medp_attn_small_fwd(qkv, 3 * E, (long long)N * 3 * E, qkv + E, qkv + 2 * E, 3 * E, (long long)N * 3 * E, o, E, 1, nullptr, B, N,
                                  N, H, dh, 1.0f / sqrtf((float)dh), 0.f, 0u, 0u, stream);
    MEDP_TRY(arc);
    MEDP_TRY(medp_gemm_bf16_nt_ws(o, e.out_w, x, M, D, E, E, E, D, nullptr, nullptr, x, D, 0, 0, sp, ws.split_bytes, stream));
    MEDP_TRY(medp_scalenorm_fwd(x, D, e.g_ff, h, D, 1, nullptr, M, D, w->norm_eps, stream));
    MEDP_TRY(medp_gemm_bf16_nt_ws(h, e.ff1_w, f, M, w->d_ff, D, D, D, w->d_ff, e.ff1_b, nullptr, nullptr, 0, 1, 1, sp, ws.split_bytes, stream));
    MEDP_TRY(medp_gemm_bf16_nt_ws(f, e.ff2_w, x, M, D, w->d_ff, w->d_ff, w->d_ff, D, e.ff2_b, nullptr, x, D, 0, 0, sp, ws.split_bytes, stream));
    return 0;
}

}  // namespace

extern "C" size_t medp_duett_workspace_bytes(const MedpDuettWeights* w, int B, int T) {
    if (!w || B <= 0 || T <= 0) return 0;
    return plan(w, B, T).total;
}

extern "C" int medp_duett_encode(const MedpDuettWeights* w, const float* xs_static, const float* xs_ts, const float* xs_times,
                                 int B, int T, float* tokens_f32, void* tokens_bf16, float* psi0_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    MEDP_CHECK_ARG(w && xs_static && xs_ts && xs_times && workspace, "duett_encode: null argument");
    MEDP_CHECK_ARG(tokens_f32, "duett_encode: tokens_f32 output is required");
    MEDP_CHECK_ARG(B > 0 && T > 0, "duett_encode: bad shape B=%d T=%d", B, T);
    MEDP_CHECK_ARG(w->d_embedding == 24 && w->d_hidden_embed == 64, "duett_encode: built for d_embedding 24 / hidden 64 (duett.py:50)");
    MEDP_CHECK_ARG(w->d_embedding % w->n_heads == 0 && (3 * w->d_embedding) % 4 == 0, "duett_encode: bad head split");
    const DuettWs ws = plan(w, B, T);
    MEDP_CHECK_ARG(workspace_bytes >= ws.total, "duett_encode: workspace %zu < required %zu", workspace_bytes, ws.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    const int V1 = w->n_vars + 1, T1 = T + 1, E = w->d_embedding, E4 = E / 4;
    const int et = E * T1, tt = E * V1;
    float* xe = (float*)(base + ws.xe);      // event view [B, V1, T1, E]; rows (b,v) of et features
    float* xt = (float*)(base + ws.xt);      // time view [B, T1, V1, E]; rows (b,t) of tt features
    float* temb = (float*)(base + ws.temb);
    float* rn = (float*)(base + ws.rn);      // pending final-ScaleNorm row scales of the view swapped next
    void* h = base + ws.h;
    const float* pending = w->final_norm ? rn : nullptr;

    MEDP_CHECK_ARG((size_t)B * T1 * V1 * E4 < (1ull << 31), "duett_encode: B*(T+1)*(V+1)*E/4 must stay below 2^31");
    // Layer 0, event view, in ONE launch: psi build + axis swap + event embedding + the event encoder's first ScaleNorm.
    MEDP_TRY(medp_duett_psi_embed_launch(w, xs_static, xs_ts, xe, h, psi0_out, B, T, s));
    MEDP_TRY(medp_duett_time_embed_launch(w, xs_times, temb, B, T, s));

    for (int l = 0; l < w->n_layers; ++l) {
        // time view -> event view (+ event embedding), applying the previous time encoder's final norm      (model :80)
        bool h_ready = true;                     // layer 0: the embed kernel wrote xe and ScaleNorm(xe) already
        if (l > 0)
            MEDP_TRY(swap_view(xt, pending, w->time_enc[l - 1].g_final, (const float*)w->event_embedding, 0, w->event_enc[l].g_attn, w->norm_eps,
                               xe, h, B, T1, V1, E4, s, &h_ready));
        MEDP_TRY(encoder_forward(w->event_enc[l], w, xe, B, V1, et, base, ws, stream, h_ready));              // (model :81)
        // final ScaleNorm of the event encoder: statistics now, scaling fused into the swap below
        if (w->final_norm) MEDP_TRY(medp_scalenorm_fwd(xe, et, w->event_enc[l].g_final, h, et, 1, rn, B * V1, et, w->norm_eps, stream));
        // event view -> time view (+ time embedding) (+ the time encoder's first ScaleNorm)                   (model :81,:90)
        MEDP_TRY(swap_view(xe, pending, w->event_enc[l].g_final, temb, (long long)T1 * V1 * E, w->time_enc[l].g_attn, w->norm_eps, xt, h, B, V1,
                           T1, E4, s, &h_ready));
        MEDP_TRY(encoder_forward(w->time_enc[l], w, xt, B, T1, tt, base, ws, stream, h_ready));               // (model :91)
        if (l + 1 < w->n_layers) {
            // the next layer's first swap reads xt and writes xe
            if (w->final_norm) MEDP_TRY(medp_scalenorm_fwd(xt, tt, w->time_enc[l].g_final, h, tt, 1, rn, B * T1, tt, w->norm_eps, stream));
        } else if (w->final_norm) {
            MEDP_TRY(medp_scalenorm_fwd(xt, tt, w->time_enc[l].g_final, tokens_f32, tt, 0, nullptr, B * T1, tt, w->norm_eps, stream));
        } else {
            hipError_t e = hipMemcpyAsync(tokens_f32, xt, (size_t)B * T1 * tt * 4, hipMemcpyDeviceToDevice, s);
            MEDP_CHECK_ARG(e == hipSuccess, "duett_encode: output copy failed");
        }
    }
    if (tokens_bf16) MEDP_TRY(medp_cast_f32_bf16(tokens_f32, tt, tokens_bf16, tt, B * T1, tt, stream));
    return 0;
}

// x_out[b][a2][a1][:] = in[b][a1][a2][:] * (rnorm ? rnorm[b][a1] * sqrt(A2*E) * g_prev : 1) + add ;  h_out = ScaleNorm(x_out) (bf16).
// add: [A2, A1, E] table (add_batch_stride 0) or [B, A2, A1, E].
extern "C" int medp_duett_swap_add_norm(const float* in, const float* rnorm, const float* g_prev, const float* add, long long add_batch_stride,
                                        const float* g_norm, float norm_eps, float* x_out, void* h_out, int B, int A1, int A2, int E,
                                        void* stream) {
    MEDP_CHECK_ARG(in && add && g_norm && x_out && h_out && B > 0 && A1 > 0 && A2 > 0 && E > 0 && E % 4 == 0, "duett_swap_add_norm: bad argument");
    MEDP_CHECK_ARG(!rnorm || g_prev, "duett_swap_add_norm: rnorm needs g_prev");
    MEDP_CHECK_ARG((size_t)B * A1 * A2 * (E / 4) < (1ull << 31), "duett_swap_add_norm: too large");
    const int rc = launch_swap_add_norm(in, rnorm, g_prev, sqrtf((float)A2 * E), add, add_batch_stride, g_norm, norm_eps, x_out, h_out, B, A1, A2,
                                        E / 4, (hipStream_t)stream);
    MEDP_CHECK_ARG(rc != 1, "duett_swap_add_norm: rows of more than 6400 floats are not built");
    return rc;
}
