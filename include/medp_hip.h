/* libmedp_hip — C ABI of the MI355X (gfx950) hot path of lastdancewithyou/multimodal_edema_prediction.
 *
 * The reference is 100 % Python and has NO plugin / FFI interface of its own: every
 * kernel it runs is dispatched by PyTorch/ATen or by the third-party x_transformers package.  The drop-in
 * boundary is therefore the Python nn.Module protocol between training_duett/{engine,trainer,evaluator}.py
 * and models/main_architecture_duett.py + loss/losses_duett.py; this library sits BEHIND the build's
 * mirror of those classes.  Each entry point cites the reference arithmetic it replaces
 * (paths relative to /root/reference; "model" = models/main_architecture_duett.py).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = invalid argument, >0 = hipError_t; the message is
 *     available from medp_last_error() (thread-local).  No exception crosses the ABI.
 *   - plain pointers + sizes; all pointers are DEVICE pointers unless named host_*; `stream` is a
 *     hipStream_t passed as void*.  Functions only ENQUEUE: no allocation, no synchronisation, no hidden
 *     state — callers own every buffer, including workspaces (query *_workspace_bytes first).
 *   - "bf16" buffers hold raw bfloat16 bits (uint16); matrices are row-major with an explicit leading
 *     dimension in ELEMENTS.
 */
#ifndef MEDP_HIP_H
#define MEDP_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------------ */
const char* medp_last_error(void);
int medp_version(void);            /* 100*major + minor */
const char* medp_arch(void);       /* "gfx950" */

/* ---- GEMM: C[M,N] = epi(A[M,K] · W[N,K]^T), bf16 MFMA, fp32 accumulate ---------------------------
 * Replaces every nn.Linear / Conv2d-as-GEMM on the path: Dinov2 query/key/value/dense/fc1/fc2 and patch
 * projection (transformers modeling_dinov2.py:139,199-201,246,286,291), x_transformers to_q/k/v/out + ff
 * (duett/duett.py:95-105), img_proj / ts_proj / perceiver in_proj, out_proj, ff (model :566,:749-757,:1027).
 * epi: (+bias[n]) -> (act==1: GELU erf) -> (*scale[n], Dinov2 LayerScale :278) -> (+residual[m,n] fp32).
 * (GELU: erf to 1.5e-7 for an fp32 result; the large-tile kernels use a degree-17 odd polynomial, |GELU error| <= 6.3e-5,
 * where the result is rounded to bf16 anyway.)
 * Requirements: K, lda, ldw multiples of 8; N, ldc, ldr multiples of 4; 16-B aligned bases.  M, N, K ragged OK. */
int medp_gemm_bf16_nt(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                      const float* bias, const float* scale, const float* residual, int ldr, int act, int out_bf16,
                      void* stream);

/* The same GEMM with a caller-owned workspace: small grids (DuETT's skinny GEMMs, duett/duett.py:95-105 at M = B(V+1) / B(T+1) rows:
 * 25-100 tiles for 256 CUs) are split along K into slices that fill the chip; the slices' fp32 partial sums go to the workspace
 * and a second pass sums them in a fixed order and applies the epilogue (deterministic, no atomics).
 * medp_gemm_nt_workspace_bytes returns 0 where the one-pass kernel is used anyway. */
size_t medp_gemm_nt_workspace_bytes(int M, int N, int K);
int medp_gemm_bf16_nt_ws(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc, const float* bias,
                         const float* scale, const float* residual, int ldr, int act, int out_bf16, float* workspace,
                         size_t workspace_bytes, void* stream);

/* FP32 KERNEL MODE (SURVEY.md 7 "always keep an fp32 kernel mode for tight checks"; 8(d) fp32 tolerances): the same two GEMMs with
 * fp32 operands and fp32 FMA accumulation on the vector ALUs (no matrix cores): a parity instrument, selected explicitly by the
 * host layer (functional.set_precision("fp32")), never by tensor dtype.  No alignment requirements. */
int medp_gemm_f32_nt(const float* A, const float* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, const float* bias,
                     const float* scale, const float* residual, int ldr, int act, void* stream);
int medp_gemm_f32_tn(const float* dY, const float* X, float* C, int M, int N, int K, int lddy, int ldx, void* stream);

/* Weight gradient C[N,K] = sum_m dY[m,n] X[m,k] (fp32 out, bf16 row-major operands, transposing LDS reads, split over m with
 * a deterministic slab reduction): the dW of every trainable Linear (autograd of model :566,:749-757,:1027, duett.py:95-105). */
size_t medp_gemm_tn_workspace_bytes(int M, int N, int K);
int medp_gemm_bf16_tn(const void* dY, const void* X, float* C, int M, int N, int K, int lddy, int ldx, float* workspace, void* stream);

/* How many CUs the persistent 256 x 256 GEMM (multi-round grids: the CXR encoder's qkv / fc1) may hold for a whole launch:
 * launches issued or CAPTURED from now on start at most `cap` workgroups (a multiple of 8 in 8..256 is used; 0 = the default,
 * 256 or MEDP_V7_WGS) and, below the cap, the fewest that still finish in the same number of rounds.  A step whose OTHER branch
 * is the long one (graph_step.GraphedStudentStep: the student's DuETT forward/backward beside the frozen teacher) leaves it
 * more of the chip this way.  Returns the previous cap. */
int medp_gemm_persistent_cap(int cap);

/* Live timing of the step's dominant kernel (the CXR-encoder block GEMMs launched by medp_vit_forward), bench.py's roofline
 * leg.  mode 1: HIP events bracket every such launch on its own stream (eager launches).  mode 2: every such launch issued
 * or CAPTURED while the mode is on carries an in-kernel launch clock (first workgroup in / last workgroup out stamp the
 * 100-MHz wall clock into a private device slot), so the begin / end of the LAST execution of each launch can be read after
 * replaying a hipGraph - the in-step figure.  mode 0 stops arming and keeps what was gathered.  collect() (device
 * synchronised by the caller in mode 2) returns the summed kernel time, the launch count and the algorithmic FLOPs
 * (2*M*N*K per launch). */
int medp_gemm_profile_enable(int mode);
int medp_gemm_profile_collect(double* host_total_ms, long long* host_n_launches, double* host_total_flops);

/* ---- attention ---------------------------------------------------------------------------------- */
/* Dense softmax(QK^T*scale)V, head dim 64, bf16 in/out: Dinov2 eager_attention_forward (modeling_dinov2.py:153-178).
 * q/k/v: [B*S, ...] rows with strides ld*, head h at column h*64.  o: [B*S, H*64]. */
int medp_attn_fwd_dh64(const void* q, const void* k, const void* v, void* o, int B, int S, int H, int ldq, int ldk,
                       int ldv, int ldo, float scale, void* stream);
/* Dense self-attention for small head dims (dh <= 16, dh % 4 == 0, N <= 272) on the matrix cores: DuETT's event / time axis
 * encoders (x_transformers Encoder, duett/duett.py:95-105: 2 heads of dim 12 over V+1 / T+1 tokens, no mask), inference form.
 * qkv: fp32 rows [B*N, ld] holding q | k | v column blocks of H*dh each (the fused QKV GEMM's output); o: bf16 [B*N, ldo].
 * Returns -2 (nothing launched) for shapes it is not built for: the caller then uses medp_attn_small_fwd. */
int medp_attn_dh16_fwd(const float* qkv, int ld, void* o_bf16, int ldo, int B, int N, int H, int dh, float scale, void* stream);
/* The same attention in TRAINING form (the student-KD step: dropout on the probabilities, gradients to q, k, v; autograd of
 * duett/duett.py:95-105): forward writes o [B*N][ldo] and the rows' log2-sum-exp lse [B*H*N]; backward writes dQ | dK | dV into
 * the column blocks of dqkv [B*N][lddqkv] (delta_ws: B*H*N floats of scratch).  Three MFMA kernels, a wave per 16-row tile, no LDS,
 * nothing added into memory (bitwise reproducible); same dropout stream as medp_attn_small_*.  Both return -2 (nothing launched)
 * for unsupported shapes. */
/* io_bf16 = 0: qkv, dout fp32 in, o, dqkv fp32 out (rounded to bf16 MFMA operands inside).  io_bf16 = 1: all four are bf16 — the
 * 16-bit hand-over between the projection GEMMs and the attention of a training step; the same operand bits, so the same results. */
int medp_attn_dh16_train_supported(int B, int N, int H, int dh, int ld, int ldo);   /* 1: the shapes these kernels take (16-byte aligned buffers assumed) */
int medp_attn_dh16_train_fwd(const void* qkv, int ld, void* o, int ldo, float* lse, int io_bf16, int B, int N, int H, int dh, float scale,
                             float dropout_p, unsigned seed, unsigned stream_id, void* stream);
int medp_attn_dh16_train_bwd(const void* dout, int lddo, const void* qkv, int ld, const float* lse, float* delta_ws, void* dqkv,
                             int lddqkv, int io_bf16, int B, int N, int H, int dh, float scale, float dropout_p, unsigned seed,
                             unsigned stream_id, void* stream);
/* Training form (--unfreeze_cxr, run.py:184-187): the same forward that also writes lse[B,H,S], the log2-domain logsumexp of the
 * scaled scores, and the flash backward that consumes it.  prep: dsum[b,h,s] = <dout, o> and the bf16 copy of dout.
 * bwd: dq/dk/dv fp32 with row stride ldd (e.g. the three column blocks of one [B*S, 3*H*64] buffer); q/k/v/dout_bf16 bf16. */
int medp_attn_fwd_dh64_lse(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int H, int ldq,
                           int ldk, int ldv, int ldo, float scale, void* stream);
int medp_attn_bwd_dh64_prep(const float* dout, int lddout, const void* o_bf16, int ldo, void* dout_bf16, int lddob,
                            float* dsum, int B, int S, int H, void* stream);
int medp_attn_bwd_dh64(const void* q, const void* k, const void* v, int ldqkv, const void* dout_bf16, int lddo,
                       const float* lse, const float* dsum, float* dq, float* dk, float* dv, int ldd, int B, int S, int H,
                       float scale, void* stream);
/* Small fp32 attention (head dim <= 64, Lk <= 1536), fwd/bwd with optional dropout on the probabilities and
 * optional head-averaged weights ([B,Lq,Lk]; every element is written once, heads added in a fixed order: bitwise
 * reproducible, need not be zeroed): x_transformers Attention inside the DuETT encoders
 * (model :81,:91) and nn.MultiheadAttention inside _PerceiverBlock (model :759-762, need_weights/average).
 * Few queries over more than 1024 keys: medp_attn_fq_split_* below. */
int medp_attn_small_fwd(const float* q, int ldq, long long q_batch_stride, const float* k, const float* v, int ldkv,
                        long long kv_batch_stride, void* o, int ldo, int o_bf16, float* attn_avg, int B, int Lq, int Lk,
                        int H, int dh, float scale, float dropout_p, unsigned seed, unsigned stream_id, void* stream);
int medp_attn_small_bwd(const float* dout, int lddo, const float* q, int ldq, long long q_batch_stride, const float* k,
                        const float* v, int ldkv, long long kv_batch_stride, float* dq, int lddq, float* dk, int lddkv,
                        float* dv, int reserved, long long dkv_batch_stride, int B, int Lq, int Lk, int H, int dh, float scale,
                        float dropout_p, unsigned seed, unsigned stream_id, void* stream);
/* The same with a key-padding mask (nn.MultiheadAttention(key_padding_mask=...); analysis/train_trajectory_probe.py:156-163):
 * key_mask [B, Lk] bytes (rows mask_batch_stride apart), non-zero = key ignored: score -inf, probability exactly 0.  The dropout
 * stream is indexed over the full Lk as above (same seed: same mask on the surviving keys).  attn_avg, if not null, need not be
 * zeroed: every element is written once, heads added in a fixed order (bitwise reproducible), masked keys exactly 0.  The backward
 * writes exact zeros to the dk / dv rows of masked keys.  A batch element whose keys are all masked gives zero probabilities, output
 * and gradients.  Always the wave-per-query kernels (the few-query and split-key kernels take no mask). */
int medp_attn_small_masked_fwd(const float* q, int ldq, long long q_batch_stride, const float* k, const float* v, int ldkv,
                               long long kv_batch_stride, void* o, int ldo, int o_bf16, float* attn_avg, int B, int Lq, int Lk,
                               int H, int dh, float scale, float dropout_p, unsigned seed, unsigned stream_id, void* stream,
                               const unsigned char* key_mask, long long mask_batch_stride);
int medp_attn_small_masked_bwd(const float* dout, int lddo, const float* q, int ldq, long long q_batch_stride, const float* k,
                               const float* v, int ldkv, long long kv_batch_stride, float* dq, int lddq, float* dk, int lddkv,
                               float* dv, int reserved, long long dkv_batch_stride, int B, int Lq, int Lk, int H, int dh, float scale,
                               float dropout_p, unsigned seed, unsigned stream_id, void* stream, const unsigned char* key_mask,
                               long long mask_batch_stride);

/* Few-query attention over ANY number of keys (head dim 64, 1 <= Lq <= 32, Lk >= 1, fp32): the perceiver's img_cross block on images
 * above 32 x 32 patches (nn.MultiheadAttention, model :759-762).  The keys are split into slices of 256, one workgroup each; the
 * slices' partial softmax statistics and sums go to a caller-owned workspace (size from medp_attn_fq_split_ws_bytes, bwd = 0 / 1)
 * and are merged in a fixed order (no atomics: bitwise reproducible; no allocation: graph-capturable).  Operands as in
 * medp_attn_small_*: q rows may be shared by the batch (q_batch_stride 0), k / v the two column halves of one [B, Lk(+skip), 2D]
 * projection, dk / dv a strided view of the same shape; k, v, dk, dv rows 16-byte aligned.  The forward writes o [B, Lq, ldo]
 * (fp32, or bf16 with o_bf16), lse [B, H, Lq] (natural-log logsumexp of the scaled scores) and, if attn_avg is not null, the head
 * average of the post-dropout probabilities [B, Lq, Lk] (every element written).  The backward takes o (fp32) and lse from the
 * forward and writes dq [B, Lq, lddq], dk, dv.  Same dropout stream as medp_attn_small_*. */
size_t medp_attn_fq_split_ws_bytes(int B, int H, int Lq, int Lk, int bwd);
int medp_attn_fq_split_fwd(const float* q, int ldq, long long q_batch_stride, const float* k, const float* v, int ldkv,
                           long long kv_batch_stride, void* o, int ldo, int o_bf16, float* lse, float* attn_avg, float* ws,
                           size_t ws_bytes, int B, int Lq, int Lk, int H, int dh, float scale, float dropout_p, unsigned seed,
                           unsigned stream_id, void* stream);
int medp_attn_fq_split_bwd(const float* dout, int lddo, const float* o, int ldo, const float* lse, const float* q, int ldq,
                           long long q_batch_stride, const float* k, const float* v, int ldkv, long long kv_batch_stride, float* dq,
                           int lddq, float* dk, float* dv, int lddkv, long long dkv_batch_stride, float* ws, size_t ws_bytes, int B,
                           int Lq, int Lk, int H, int dh, float scale, float dropout_p, unsigned seed, unsigned stream_id,
                           void* stream);

/* ---- normalisation -------------------------------------------------------------------------------- */
/* nn.LayerNorm (modeling_dinov2.py:348,353 eps 1e-6; model :750-753 eps 1e-5).  y is bf16 (feeds a GEMM) or fp32. */
int medp_layernorm_fwd(const float* x, int ldx, const float* w, const float* b, void* y, int ldy, int y_bf16, float* mean,
                       float* rstd, int rows, int D, float eps, void* stream);
size_t medp_colsum_workspace_bytes(int rows, int D);
int medp_layernorm_bwd(const float* dy, int lddy, const float* x, int ldx, const float* w, const float* mean,
                       const float* rstd, float* dx, int lddx, int accumulate_dx, float* dw, float* db, float* workspace,
                       int rows, int D, void* stream);
/* out[c] = sum_r x[r][c] (bias gradients; deterministic two-stage reduction) */
int medp_colsum_f32(const float* x, int ldx, float* out, float* workspace, int rows, int D, void* stream);
/* x_transformers ScaleNorm: y = x / max(||x||, eps) * sqrt(D) * g  (duett/duett.py:95-105 use_scalenorm=True) */
int medp_scalenorm_fwd(const float* x, int ldx, const float* g, void* y, int ldy, int y_bf16, float* rnorm, int rows, int D,
                       float eps, void* stream);
int medp_scalenorm_bwd(const float* dy, int lddy, const float* x, int ldx, const float* g, const float* rnorm, float* dx,
                       int lddx, int accumulate_dx, float* dg, float* workspace_rows, int rows, int D, void* stream);
/* dx = add + d ScaleNorm(x) / dx applied to dy: the residual join of a pre-norm block (x feeds the norm AND the residual) in the backward,
 * out of place — `add` (the gradient that arrived through the residual) is only read.  dg as above. */
int medp_scalenorm_bwd_add(const float* dy, int lddy, const float* x, int ldx, const float* g, const float* rnorm, const float* add,
                           int ldadd, float* dx, int lddx, float* dg, float* workspace_rows, int rows, int D, void* stream);

/* ---- layout / pointwise ------------------------------------------------------------------------------ */
/* y[r][c] = (bf16) x[r][c]: cols, ldx, ldy multiples of 4; ldy >= cols unless rows == 1 (ldx may be smaller than cols: a broadcast row) */
int medp_cast_f32_bf16(const float* x, int ldx, void* y, int ldy, int rows, int cols, void* stream);
int medp_transpose_to_bf16(const void* x, int x_is_bf16, int ldx, void* y, int ldy, int rows, int cols, void* stream);
/* The bf16 GEMM operands of MANY fp32 weight matrices in one launch (the per-step casts of a training step's trainable weights: each
 * nn.Linear of the reference needs W as bf16 [N,K] for y = x W^T and W^T as bf16 [K, Npad8] for dX = dY W).  Job: src fp32 [rows, ld_src];
 * dst_plain bf16 [rows, ld_plain] and / or dst_t bf16 [cols, ld_t] (either may be NULL; pad columns of dst_t are the caller's zeros).
 * Block b handles the 64x64 tile dev_block_tile[b] (row-major over ceil(rows/64) x ceil(cols/64)) of job dev_block_job[b].
 * Same rounding as medp_cast_f32_bf16 / medp_transpose_to_bf16. */
typedef struct {
    const void* src;
    void* dst_plain;
    void* dst_t;
    int rows, cols, ld_src, ld_plain, ld_t, reserved_;
} MedpOperandJob;
int medp_weight_operands_multi(const MedpOperandJob* dev_jobs, const int* dev_block_job, const int* dev_block_tile, int n_blocks,
                               void* stream);
int medp_gelu_bwd(const float* dy, const float* pre, float* dx, long long n, void* stream);
/* bf16 forms (trainable CXR encoder, fused blocks): out = gelu(pre); dx = dy * gelu'(pre); all three bf16, n % 8 == 0 */
int medp_gelu_bf16_fwd(const void* pre, void* out, long long n, void* stream);
int medp_gelu_bf16_bwd(const void* dy, const void* pre, void* dx, long long n, void* stream);
/* Dinov2PatchEmbeddings conv14/s14 as im2col (modeling_dinov2.py:139,148) */
int medp_im2col_patch(const float* pix, void* A, int B, int C, int H, int W, int patch, int kpad, void* stream);
/* cls token + position embeddings (modeling_dinov2.py:108-112) */
int medp_vit_assemble(const float* patch, const float* cls, const float* pos, float* x, int B, int P, int D, void* stream);
/* interpolate_pos_encoding, bicubic align_corners=False (modeling_dinov2.py:57-95) */
int medp_pos_embed_bicubic(const float* pos, float* out, int src_side, int gh, int gw, int D, void* stream);
/* its transpose (the trainable encoder): dout [1 + gh*gw, D] -> dpos [1 + src_side^2, D]; a gather, deterministic */
int medp_pos_embed_bicubic_bwd(const float* dout, float* dpos, int src_side, int gh, int gw, int D, void* stream);

/* ---- whole-module forward of the frozen CXR encoder: CXREncoder.forward (model :152-158) ---------- */
typedef struct {
    const float *ln1_w, *ln1_b;
    const void* qkv_w;            /* bf16 [3*hidden, hidden]: query | key | value rows */
    const float* qkv_b;           /* [3*hidden] */
    const void* proj_w;           /* bf16 [hidden, hidden]  attention.output.dense */
    const float *proj_b, *ls1;    /* layer_scale1.lambda1 */
    const float *ln2_w, *ln2_b;
    const void* fc1_w;            /* bf16 [mlp, hidden] */
    const float* fc1_b;
    const void* fc2_w;            /* bf16 [hidden, mlp] */
    const float *fc2_b, *ls2;
} MedpVitLayer;

typedef struct {
    int hidden, n_layers, n_heads, mlp_hidden, patch, pos_side, patch_kpad;
    float ln_eps;
    const void* patch_w;          /* bf16 [hidden, patch_kpad] (conv weight flattened c,i,j; zero padded) */
    const float *patch_b, *cls, *pos;   /* pos: fp32 [pos_side^2 + 1, hidden] */
    const float *final_ln_w, *final_ln_b;
    const MedpVitLayer* layers;   /* HOST array of n_layers entries */
} MedpVitWeights;

size_t medp_vit_workspace_bytes(const MedpVitWeights* host_w, int B, int H, int W);
/* pixels fp32 [B,3,H,W] -> tokens_f32 [B, P+1, hidden] (may be NULL) and/or tokens_bf16 (may be NULL) after the final LN */
int medp_vit_forward(const MedpVitWeights* host_w, const float* pixels, int B, int H, int W, float* tokens_f32,
                     void* tokens_bf16, void* workspace, size_t workspace_bytes, void* stream);
/* The same forward in pieces: the embedding stage runs when first_layer == 0, encoder layers [first_layer, last_layer), the final
 * LayerNorm (and the outputs) when last_layer == n_layers.  Between calls the fp32 token stream lives in `workspace`, which
 * the caller must leave untouched.  (graph_step.py splits the frozen encoder of the NEXT batch across the two captured graphs
 * of a multi-GPU step, so that the gradient all-reduce and the optimiser run beside encoder layers instead of after them.) */
int medp_vit_forward_part(const MedpVitWeights* w, const float* pixels, int B, int H, int W, float* tokens_f32, void* tokens_bf16,
                          void* workspace, size_t workspace_bytes, int first_layer, int last_layer, void* stream);

/* ---- whole-module forward of the DuETT backbone in inference form: DuettFeatureExtractor.encode (model :31-94) -----
 * BatchNorm layers are folded by the caller into (scale, shift) = (w/sqrt(var+eps), b - mean*scale): eval-mode
 * BatchNormLastDim (duett/duett.py:11-22).  Encoder = x_transformers.Encoder(depth=1) (duett/duett.py:95-105),
 * restated in oracle/xt_encoder.py (parity unpinned at that boundary). */
typedef struct {
    const float* g_attn;          /* ScaleNorm gain before attention [1] */
    const void* qkv_w;            /* bf16 [3*E, D]: to_q | to_k | to_v rows (no bias) */
    const void* out_w;            /* bf16 [D, E]   to_out (no bias) */
    const float* g_ff;            /* ScaleNorm gain before the feed-forward [1] */
    const void* ff1_w;            /* bf16 [d_ff, D] */
    const float* ff1_b;
    const void* ff2_w;            /* bf16 [D, d_ff] */
    const float* ff2_b;
    const float* g_final;         /* final ScaleNorm gain [1] (used when final_norm != 0) */
} MedpEncoderWeights;

typedef struct {
    int n_vars, n_static, d_embedding, n_heads, n_layers, d_ff, d_hidden_embed, d_hidden_tab, d_hidden_time, n_obs_rows,
        final_norm;
    float norm_eps;
    /* per-variable embedding MLPs stacked over V: Linear(2,64) -> ReLU -> BN -> Linear(64,E)  (duett.py:84-86), in the layout the
     * embed kernel stages in LDS: emb_b4 fp32 [V,E] = the second Linear's bias; emb_l0 fp32 [V,64,8] = (w0[j][0], w0[j][1], b0[j],
     * bn_scale[j], bn_shift[j], 0, 0, 0); emb_w4t fp32 [V,64,E] = w4 transposed */
    const void *emb_b4, *emb_l0, *emb_w4t;
    const void* n_obs_table;      /* fp32 [n_obs_rows] (n_obs_embedding.weight[:,0]) */
    const void *tab_w0, *tab_b0, *tab_bn_scale, *tab_bn_shift, *tab_w4, *tab_b4;   /* tab_encoder (duett.py:124-125) */
    const void* special;          /* fp32 [8, E] special_embeddings */
    const void *time_w0, *time_b0, *time_bn_scale, *time_bn_shift, *time_w3t, *time_b3;   /* full_time_embedding = cve (duett.py:151-157); time_w3t = weight of the last Linear TRANSPOSED, fp32 [h, tt] */
    const void* rep_embedding;    /* fp32 [tt_dim]  full_rep_embedding.weight[:,0] */
    const void* event_embedding;  /* fp32 [V+1, et_dim] full_event_embedding.weight */
    const MedpEncoderWeights* event_enc;   /* HOST arrays of n_layers entries */
    const MedpEncoderWeights* time_enc;
} MedpDuettWeights;

/* The embedding stage of medp_duett_encode on its own (model :41-69; kernel-level parity and the per-kernel HBM table of bench.py).
 * stages bit 0: static encoder + FUSED psi build: psi (model :45-66) is produced directly in the EVENT view with the event
 *   embedding added (model :80) and the event encoder's first ScaleNorm applied: xe_out fp32 [B, V+1, (T+1)E], h_out bf16 (same
 *   shape), psi0_out (optional) psi in the time view [B, T+1, V+1, E] before the add; tab_workspace: unused (may be NULL).
 * stages bit 1: time embedding cve(xs_times) with the REP row appended (model :67-69): temb_out fp32 [B, T+1, (V+1)E]. */
int medp_duett_embed_fwd(const MedpDuettWeights* host_w, const float* xs_static, const float* xs_ts, const float* xs_times, int B, int T,
                         float* xe_out, void* h_out_bf16, float* temb_out, float* psi0_out, float* tab_workspace, int stages, void* stream);
/* Axis swap + positional add + the next encoder's first ScaleNorm in one pass (model :80 / :90 + x_transformers pre-norm):
 * x_out[b][a2][a1][:] = in[b][a1][a2][:] * rowscale(b,a1) + add, h_out = ScaleNorm(x_out) as bf16.  rowscale applies the previous
 * encoder's pending final ScaleNorm (rnorm [B*A1] from medp_scalenorm_fwd, gain g_prev) or is 1 when rnorm is NULL.
 * add: [A2, A1, E] (add_batch_stride 0) or [B, A2, A1, E] (stride A2*A1*E). */
int medp_duett_swap_add_norm(const float* in, const float* rnorm, const float* g_prev, const float* add, long long add_batch_stride,
                             const float* g_norm, float norm_eps, float* x_out, void* h_out_bf16, int B, int A1, int A2, int E,
                             void* stream);

/* ---- device-side batch assembly -------------------------------------------------------------------------
 * medp_feats_to_input replaces the host loop of Model.feats_to_input (duett/duett.py:159-187): sample b is a ragged series
 * [T_b, 2V] (values | observation counts) with bin times [T_b], given EITHER by device pointer tables (ts_ptrs / time_ptrs,
 * [B] device arrays of device pointers) OR as rows of one stacked buffer (ts_base + b*ts_stride, time_base + b*time_stride,
 * strides in elements); lengths [B] int32 device array of T_b (NULL: every sample has T_uniform steps).
 * Output: xs_ts [B, Tpad, 2V+1] (last max_len steps, zero mask column appended, zero padded; Tpad = the longest kept length,
 * computed by the caller from the shapes), xs_times [B, Tpad], xs_static [B, Ds].
 * Training augmentation (duett.py:169-175,184-185): values += aug_noise * N(0,1) * count; timesteps dropped with probability
 * aug_mask (row := 0, mask column := 1); static += aug_noise * N(0,1); draws from the counter-based hash (seed, stream_id,
 * element, RNG epoch) - with both rates 0 the result is bit-exact. */
int medp_feats_to_input(const float* const* ts_ptrs, const float* ts_base, long long ts_stride, const float* const* time_ptrs,
                        const float* time_base, long long time_stride, const int* lengths, int T_uniform, const float* static_in,
                        float* xs_ts, float* xs_times, float* xs_static, int B, int V, int Ds, int max_len, int Tpad, float aug_noise,
                        float aug_mask, unsigned seed, unsigned stream_id, void* stream);
/* Masking half of Model.pretrain_prep_batch (duett.py:189-237) for pretrain_masked_steps == 1: mask_t [B] int32 = masked
 * timestep, event_idx [B] int32 = masked variable (NULL: predict_events off), keep [B,V] uint8 = the variable-dropout draw
 * (NULL: pretrain_dropout 0) - the HOST draws them (numpy Generator, reference order).  Writes the clipped input
 * [B,T,2V+1], y_ts / y_masks [B,V], y_events / y_events_mask [B,T]. */
int medp_ssl_mask_batch(const float* xs_ts, const int* mask_t, const int* event_idx, const unsigned char* keep, float* clipped,
                        float* y_ts, float* y_masks, float* y_events, float* y_events_mask, int B, int T, int V, void* stream);

size_t medp_duett_workspace_bytes(const MedpDuettWeights* host_w, int B, int T);
/* xs_static [B,Ds], xs_ts [B,T,2V+1], xs_times [B,T] fp32 (outputs of feats_to_input) -> tokens [B, T+1, E*(V+1)];
 * psi0_out (optional, [B,T+1,V+1,E]) receives psi after the embedding stage for parity checks. */
int medp_duett_encode(const MedpDuettWeights* host_w, const float* xs_static, const float* xs_ts, const float* xs_times, int B,
                      int T, float* tokens_f32, void* tokens_bf16, float* psi0_out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- fusion head pointwise ops (fp32), dropout masks regenerated from (seed, stream_id, element index) --------- */
int medp_gelu_dropout_fwd(const float* x, float* y, long long n, float p, unsigned seed, unsigned stream_id, void* stream);
int medp_gelu_dropout_bwd(const float* dy, const float* x, float* dx, long long n, float p, unsigned seed, unsigned stream_id,
                          void* stream);
/* 16-bit hand-over forms for a fused feed-forward node (ScaleNorm -> Linear -> GELU -> Dropout -> Linear of x_transformers' FeedForward):
 * the forward writes the next Linear's bf16 operand directly; the backward writes dx in fp32 (bias gradient) AND its bf16 copy (operand of
 * the previous Linear's gradient GEMMs).  Same rounding as medp_cast_f32_bf16 on the fp32 result. */
int medp_gelu_dropout_fwd_bf16(const float* x, void* y_bf16, long long n, float p, unsigned seed, unsigned stream_id, void* stream);
int medp_gelu_dropout_bwd_bf16(const float* dy, const float* x, float* dx, void* dx_bf16, long long n, float p, unsigned seed,
                               unsigned stream_id, void* stream);
/* out = residual + dropout(y) (residual may be NULL; backward = same call on the incoming gradient with residual NULL) */
int medp_dropout_add(const float* y, const float* residual, float* out, long long n, float p, unsigned seed, unsigned stream_id,
                     void* stream);
/* Linear(D,1) output layer of the pathology heads (model :574,:590) */
int medp_rowdot_fwd(const float* x, int ldx, const float* w, const float* b, float* y, int rows, int D, void* stream);
int medp_rowdot_bwd(const float* dy, const float* x, int ldx, const float* w, float* dx, float* dw, float* db, int rows, int D,
                    void* stream);
/* per-label biases + residual fusion  fusion = img.detach() + beta*correction  (model :634-639) */
int medp_fusion_logits_fwd(const float* hi, const float* ht, const float* hc, const float* img_bias, const float* ts_bias,
                           const float* beta, float* img, float* ts, float* scaled, float* fus, int B, int K, void* stream);
int medp_fusion_logits_bwd(const float* d_img, const float* d_ts, const float* d_scaled, const float* d_fus, const float* hc,
                           const float* beta, float* d_hi, float* d_ht, float* d_hc, float* d_img_bias, float* d_ts_bias,
                           float* d_beta, int B, int K, void* stream);
/* StudentModel pool="mean" over the T hourly tokens of [B, T1, D] (model :1231) */
int medp_meanpool_fwd(const float* x, float* y, int B, int T, int T1, int D, void* stream);
int medp_meanpool_bwd(const float* dy, float* dx, int B, int T, int T1, int D, void* stream);

/* ---- losses: value + gradient in one launch ------------------------------------------------------------------------
 * DualPathologyLoss (loss/losses_duett.py:131-194).  out: [0] total, [1] img_total, [2] ts_total, [3] fus_total,
 * [4..4+3K) img_per | ts_per | fus_per.  g_*: d total / d logits (any may be NULL).  pos_weight may be NULL. */
int medp_dual_pathology_loss(const float* img, const float* ts, const float* fus, const float* y, const float* mask,
                             const float* label_weights, const float* pos_weight, float alpha_img, float alpha_ts,
                             float alpha_fus, float eps, float* out, float* g_img, float* g_ts, float* g_fus, int B, int K,
                             void* stream);
/* StudentKDLoss + VanillaKLKD (loss/losses_duett.py:8-57).  out: [0] total [1] bce [2] kd.  pos_weight = 1 for none. */
int medp_student_kd_loss(const float* z_s, const float* z_t, const float* y, float T, float alpha, float pos_weight, float* out,
                         float* g_zs, int B, void* stream);

/* engine extras: aux residual KL with label smoothing (training_duett/engine.py:149-165); LP regularisers
 * coef*mean(x^2) (engine.py:217-223); the linear probe's global masked BCE (cxr_linear_training.ipynb:426-437).
 * Each writes the scalar to out[0] and, when g != NULL, the gradient w.r.t. its differentiable input. */
int medp_aux_residual_kl(const float* img_logits, const float* scaled_correction, const float* y, const float* mask,
                         float label_smoothing, float* out, float* g_scaled, int n, void* stream);
int medp_sq_mean(const float* x, float coef, float* out, float* g, int n, void* stream);
int medp_masked_bce_global(const float* logits, const float* y, const float* mask, float* out, float* g, int n, void* stream);

/* DuETT-only step losses (duett/duett.py:337-365): mean(((a-b)*mask)^2) and mean(weight * BCEWithLogits); mask/weight may be NULL */
int medp_masked_mse(const float* a, const float* b, const float* mask, float* out, float* g_a, int n, void* stream);
int medp_bce_mean(const float* logits, const float* y, const float* weight, float* out, float* g, int n, void* stream);

/* ---- optimiser: torch.optim.AdamW semantics over a device table of tensors (trainer.py:77-116,383) -------------- */
typedef struct {
    void* param;            /* fp32, updated in place */
    const void* grad;       /* fp32 */
    void* exp_avg;          /* fp32 */
    void* exp_avg_sq;       /* fp32 */
    long long numel;
    float lr, weight_decay;
} MedpAdamTensor;
int medp_adamw_chunk_elems(void);   /* elements one workgroup updates; block b handles chunk dev_block_chunk[b] of tensor dev_block_tensor[b] */
/* step: host step count (>= 1), used when dev_step == NULL; dev_step: device counter holding the step (graph replay) */
int medp_adamw_multi(const MedpAdamTensor* dev_descs, const int* dev_block_tensor, const int* dev_block_chunk, int n_blocks,
                     float beta1, float beta2, float eps, int step, const unsigned* dev_step, float grad_scale, void* stream);
/* Global-norm gradient clipping on the device (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False; the gradients themselves
 * are not rewritten).  medp_grad_sumsq_multi: over the same table and block map, workgroup b writes its chunk's sum of squares to
 * dev_partials[b] (n_blocks floats, caller-owned); a single workgroup then adds them in index order (no atomics: bitwise
 * reproducible) and writes dev_out[0] = norm, dev_out[1] = min(1, max_norm / (norm + 1e-6)).  medp_adamw_multi_dscale is
 * medp_adamw_multi with the gradient scale read from device memory (dev_out + 1), so the clip can sit inside a captured step. */
int medp_grad_sumsq_multi(const MedpAdamTensor* dev_descs, const int* dev_block_tensor, const int* dev_block_chunk, int n_blocks,
                          float* dev_partials, float max_norm, float* dev_out, void* stream);
int medp_adamw_multi_dscale(const MedpAdamTensor* dev_descs, const int* dev_block_tensor, const int* dev_block_chunk, int n_blocks,
                            float beta1, float beta2, float eps, int step, const unsigned* dev_step, const float* dev_grad_scale,
                            void* stream);

/* ---- HIP-graph support: state that must change between replays lives in device memory --------------------------------
 * medp_rng_set_epoch_ptr: device uint32 mixed into every dropout seed (NULL = off); medp_counter_advance: *c += 1 */
int medp_rng_set_epoch_ptr(const unsigned* dev_ptr);
int medp_counter_advance(unsigned* dev_counter, void* stream);

/* ---- DuETT embedding stage in TRAINING form (student KD path; BatchNorm batch statistics, gradients everywhere) ------
 * grouped tiny layers, group = variable: x [G,R,K], W [G,N,K], b [G,N]   (duett/duett.py:24-39,84-86,124-125,151-157) */
int medp_glinear_fwd(const float* x, const float* W, const float* b, float* y, int G, int R, int K, int N, void* stream);
size_t medp_glinear_bwd_workspace_bytes(int G, int R, int K, int N);
int medp_glinear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, float* workspace, int G, int R,
                     int K, int N, void* stream);
/* The per-variable embedding MLP Linear(KIN, C) -> ReLU -> BatchNormLastDim(C) -> Linear(C, E) (duett/duett.py:24-39 `simple_mlp` with
 * hidden_batch_norm, model file :45-55) of ALL variables as fused kernels that never store the hidden activations (csrc/duett_embed_train.hip):
 * x [G][R][KIN], W0 [G][C][KIN], b0 / bn_w / bn_b / running_* / save_* [G][C], W1 [G][E][C], b1 [G][E], out [G][R][E].  batch_stats = 1:
 * train() (batch statistics normalise, running statistics updated in place), 0: eval().  Built for (KIN, C, E) = (2, 64, 24) — the
 * reference's defaults; medp_gmlp_supported says so, the entry points return -2 otherwise (use medp_glinear_* / medp_gbn_* / medp_act_*).
 * bwd: dx may be NULL; every other gradient is written (dbn_w / dbn_b: BatchNorm weight / bias).  Bitwise reproducible. */
int medp_gmlp_supported(int KIN, int C, int E);
size_t medp_gmlp_workspace_bytes(int G, int R, int KIN, int C, int E);
int medp_gmlp_fwd(const float* x, const float* W0, const float* b0, const float* bn_w, const float* bn_b, float* running_mean,
                  float* running_var, const float* W1, const float* b1, float* out, float* save_mean, float* save_var, int G, int R,
                  int KIN, int C, int E, float eps, float momentum, int batch_stats, float* workspace, void* stream);
int medp_gmlp_bwd(const float* dout, const float* x, const float* W0, const float* b0, const float* bn_w, const float* bn_b,
                  const float* save_mean, const float* save_var, const float* W1, float* dx, float* dW0, float* db0, float* dbn_w,
                  float* dbn_b, float* dW1, float* db1, int G, int R, int KIN, int C, int E, float eps, int batch_stats,
                  float* workspace, void* stream);
/* BatchNormLastDim over the R rows of every group (duett/duett.py:11-22): batch_stats=1 train (biased var normalises,
 * unbiased updates running), 0 eval.  save_mean/save_var [G,C] feed the backward. */
size_t medp_gbn_workspace_bytes(int G, int R, int C);   /* per-chunk partial sums of the two-stage (deterministic) row reductions */
int medp_gbn_fwd(const float* x, const float* w, const float* b, float* running_mean, float* running_var, float* y, float* save_mean,
                 float* save_var, int G, int R, int C, float eps, float momentum, int batch_stats, float* workspace, void* stream);
int medp_gbn_bwd(const float* dy, const float* x, const float* w, const float* save_mean, const float* save_var, float* dx, float* dw,
                 float* db, int G, int R, int C, float eps, int batch_stats, float* workspace, void* stream);
int medp_act_fwd(const float* x, float* y, long long n, int mode /*0 relu, 1 tanh*/, void* stream);
int medp_act_bwd(const float* dy, const float* y, float* dx, long long n, int mode, void* stream);
/* (value, n_obs_embedding[clip(int(count),0,15)]) pairs per variable, zero-padded to KP columns (model :41-52) */
int medp_embed_inputs_fwd(const float* xs_ts, const float* n_obs_table, int table_rows, float* xin, int B, int T, int V, int KP,
                          void* stream);
int medp_embed_inputs_bwd_blocks(int B, int T, int V);
int medp_embed_inputs_bwd(const float* xs_ts, const float* d_xin, float* partial, int table_rows, int B, int T, int V, int KP,
                          void* stream);
/* psi assembly with special-token overrides (model :53-66) and its backward */
int medp_psi_assemble_fwd(const float* xs_ts, const float* var_out, const float* tab_out, const float* special, float* psi, int B, int T,
                          int V, int E, void* stream);
/* backward: d_var_out [V][B*T][E] (zero where a cell was overridden) and, per batch element and SLICE of its cells (S =
 * medp_psi_assemble_bwd_slices), the partial sums d_tab_partial [B][S][E] (static column) and d_special_partial [B][S][2][E]
 * (masked / REP cells): the caller adds the slices (a fixed order: deterministic) */
int medp_psi_assemble_bwd_slices(int B, int T, int V);
int medp_psi_assemble_bwd(const float* xs_ts, const float* dpsi, float* d_var_out, float* d_tab_partial, float* d_special_partial, int B,
                          int T, int V, int E, void* stream);
int medp_axis_swap(const float* in, float* out, int B, int A1, int A2, int E, void* stream);
/* the axis swap with the new leading axis' positional embedding added on the way: mode 1: add [A2][A1][E] shared by the batch (model :80-81);
 * mode 3: add [B*(A2-1)][A1][E] per sample for a2 < A2-1 and add_last [A1][E] for the last row (model :90 without the concatenation) */
int medp_axis_swap_add(const float* in, const float* add, const float* add_last, float* out, int B, int A1, int A2, int E, int mode,
                       void* stream);
int medp_add_bcast(const float* a, const float* b, float* out, long long per_batch, int B, int broadcast_b, void* stream);

/* ---- LocalTrajectoryEncoder (models/main_architecture_duett.py:1242-1391) -------------------------------
 * The Linear / LayerNorm / GELU stages of the module are the kernels above; these are the rest.
 * medp_traj_features: x [B,T,2V] fp32 (values | counts) -> out [B*V, T, 8] fp32 = {value (0 where unobserved), observed,
 *   log1p(count)/ln 16, steps since the previous observation / T, (T - t) / T, 0, 0, 0}  (:1316-1330, :1342-1358; the five
 *   features padded to 8 so that Linear(5, d) runs as a K = 8 GEMM).
 * medp_gru_fwd: one-layer batch-first nn.GRU, h0 = 0 (:1297-1303, :1366), hidden size d = 128 only (anything else: rc < 0).
 *   gi [S,T,3d] fp32 = x_t W_ih^T + b_ih (gate order r | z | n), whh_bf16 [3d,d], bhh [3d] -> hseq [S,T,d]; gates [S,T,3d]
 *   (r | z | n) and hn [S,T,d] (= W_hn h + b_hn) are saved for the backward (both null: inference).
 * medp_gru_bwd: dh [S,T,d] (gradient w.r.t. every h_t) -> dgi [S,T,3d], dghn [S,T,d] (gradient w.r.t. W_hn h + b_hn) and
 *   dgh_bf16 [S,T,3d] (r | z | n parts of the gradient w.r.t. h W_hh^T + b_hh; dW_hh = dgh^T h_prev is a medp_gemm_bf16_tn).
 *   whh_t_bf16 [d,3d] = W_hh transposed.
 * medp_gru_fwd_f32: the forward with fp32 weights, fp32 products and libm exp / tanh (the fp32 kernel mode: a parity instrument);
 *   whh_t [d, ld_whh_t >= 3d] fp32 = W_hh transposed; same outputs, so medp_gru_bwd serves it too.
 * Stacked GRU (n_layers > 1; layer k >= 1 reads every hidden state of layer k - 1, with dropout between the layers in training):
 * medp_gru_fwd_h16: medp_gru_fwd that also writes hseq_bf16 [S,T,d] = bf16(h_t * mask), the next layer's input, from the registers
 *   that hold h_t; mask = the inter-layer dropout keep-mask times 1 / (1 - p), drawn by (seed, stream_id, RNG epoch) on the flat
 *   element index of [S,T,d]; dropout_p = 0: a plain rounding.
 * medp_gru_bwd_dgi16: medp_gru_bwd that also writes dgi_bf16 [S,T,3d], the bf16 copy of dgi an upper layer's dW_ih = dgi^T x and
 *   dx = dgi W_ih GEMMs read. */
int medp_traj_features(const float* x, float* out, int B, int T, int V, void* stream);
int medp_gru_fwd(const float* gi, const void* whh_bf16, const float* bhh, float* hseq, float* gates, float* hn, int S, int T, int d,
                 void* stream);
int medp_gru_fwd_f32(const float* gi, const float* whh_t, int ld_whh_t, const float* bhh, float* hseq, float* gates, float* hn, int S,
                     int T, int d, void* stream);
int medp_gru_bwd(const float* dh, const float* gates, const float* hn, const float* hseq, const void* whh_t_bf16, float* dgi,
                 float* dghn, void* dgh_bf16, int S, int T, int d, void* stream);
int medp_gru_fwd_h16(const float* gi, const void* whh_bf16, const float* bhh, float* hseq, float* gates, float* hn, void* hseq_bf16,
                     float dropout_p, unsigned seed, unsigned stream_id, int S, int T, int d, void* stream);
int medp_gru_bwd_dgi16(const float* dh, const float* gates, const float* hn, const float* hseq, const void* whh_t_bf16, float* dgi,
                       float* dghn, void* dgh_bf16, void* dgi_bf16, int S, int T, int d, void* stream);

/* ---- Raw-trajectory conditional probe (analysis/raw_trajectory_conditional_probe.py, default path) -------------------------
 * All arithmetic is fp64, as in the reference.
 * medp_raw_traj_summary: x [B,T,2V] fp32 (values | counts, the layout medp_traj_features reads) -> out [B,V,14] fp64 =
 *   {last, mean, std, min, max | delta, slope24, slope_recent, recent_shift | observed_fraction, log_total_count,
 *   time_since_last, recent_observed_fraction, log_recent_count}: _summarize_one_variable (:329-405) with one row per hour
 *   (slot_idx = t), its NaN rules and its centred two-pass std / slopes.  1 <= recent_hours <= T, otherwise rc < 0.
 * medp_offset_logistic_valgrad: objective and gradient of _fit_offset_weights (:578-584) for G candidate columns at once:
 *   X [n, ldx >= F] row-major, y [n] (0 / 1 as fp64), offset [n], W [F,G], l2 [G] ->
 *   obj [G] = mean(logaddexp(0, s) - y s) + 0.5 l2 w.w,  grad [F,G] = X^T (expit(s) - y) / n + l2 w,  s = offset + X w.
 *   X is read from HBM once (a workgroup keeps its row block in LDS between the two halves; a row longer than the LDS budget,
 *   F > 18432, is re-read through L2 instead).  Partial sums go through ws (medp_offset_logistic_ws_bytes) and are added in
 *   a fixed order: bit-stable, no floating-point atomics.  1 <= G <= MEDP_OFFSET_LOGISTIC_MAX_G, F >= 1, n >= 1, otherwise rc < 0.
 * medp_resampled_binary_metrics: out [R,3] = {BCE, AUROC, AUPRC} of R resampled replicates, one workgroup each.
 *   y [N] u8; p [Rp,N] with Rp = 1 (one vector shared by all replicates) or Rp = R; replicate r gathers positions
 *   idx[offsets[r] .. offsets[r+1]) (int32 in [0, N); offsets int64 [R+1]); idx = null: every replicate is the identity over
 *   all N (offsets unused).  Probabilities are clipped to [1e-7, 1 - 1e-7] after the gather (_safe_metrics :109-119), sorted in
 *   LDS; AUROC and AUPRC take one threshold per DISTINCT score (sklearn's roc_auc_score / average_precision_score on ties).
 *   One class only: AUROC = AUPRC = NaN, BCE finite.  An empty replicate, or one with an index outside [0, N): NaN, NaN, NaN.
 *   max_len = the longest replicate (the caller drew the indices); above MEDP_RESAMPLED_METRICS_MAX_LEN: rc < 0, no launch. */
#define MEDP_OFFSET_LOGISTIC_MAX_G 8
#define MEDP_LDS_SORT_MAX_LEN 16384 /* the one bound of the kernels that sort in LDS (csrc/rank_lds.h): the two names below */
#define MEDP_RESAMPLED_METRICS_MAX_LEN MEDP_LDS_SORT_MAX_LEN /* 8-byte keys: 128 KiB of the CU's 160 KiB LDS, a power of two for the bitonic sort */
int medp_raw_traj_summary(const float* x, double* out, int B, int T, int V, int recent_hours, void* stream);
size_t medp_offset_logistic_ws_bytes(int n, int F, int G);
int medp_offset_logistic_valgrad(const double* X, long long ldx, const double* y, const double* offset, const double* W,
                                 const double* l2, double* obj, double* grad, void* ws, size_t ws_bytes, int n, int F, int G,
                                 void* stream);
int medp_resampled_binary_metrics(const unsigned char* y, const double* p, const int* idx, const long long* offsets, double* out,
                                  int N, int Rp, int R, int max_len, void* stream);

/* ---- Temporal-usage diagnostics (analysis/diagnose_temporal_usage.py; csrc/temporal_diag.hip) -----------------------------
 * medp_counterfactual_feats: medp_feats_to_input without augmentation for the five arrangements of ONE batch the diagnostic
 *   compares, in one launch.  The series / times / lengths / static arguments are those of medp_feats_to_input (pointer tables
 *   or rows of one stacked buffer; lengths or T_uniform).  sample_perm [B] int32 pairs every sample with another one;
 *   time_perm [B, Tmax] int32: row b is a permutation of [0, T_b), Tmax >= every T_b, entries past T_b are unread.
 *   Outputs, condition-major in the order {full, patient_shuffle, ts_shuffle, time_reverse, time_permute}:
 *   xs_ts [5, B, Tpad, 2V+1], xs_times [5, B, Tpad], xs_static [5, B, Ds].  The reference transforms the RAW tuples and then
 *   assembles, so with n = min(T, max_len), off = T - n of the series that supplies the rows, output step t < n holds
 *     full            sample b,        row off + t                 times b,        static b
 *     patient_shuffle sample perm[b],  row off + t                 times perm[b],  static perm[b]
 *     ts_shuffle      sample perm[b],  row off + t                 times b,        static b
 *     time_reverse    sample b,        row T_b - 1 - (off + t)     times b (not reversed), static b
 *     time_permute    sample b,        row time_perm[b][off + t]   times b,        static b
 *   i.e. reversal and permutation act BEFORE the truncation to the last max_len steps.  The mask column is 0, steps t >= n are 0.
 *   ts_shuffle is defined only where lengths[perm[b]] == lengths[b] (the reference's padding goes negative otherwise): the
 *   caller checks that; the kernel stays in bounds either way.  A sample_perm entry outside [0, B) or a time_perm entry
 *   outside [0, T_b) is never dereferenced: the output rows that depend on it become NaN (the convention of
 *   medp_resampled_binary_metrics).  Null pointers or non-positive sizes: rc < 0, no launch.
 * medp_temporal_usage_summary: fus, ts [C, N, K] fp32 logits (condition 0 = full), attn [N, K, S] fp32 or null ->
 *   prob [2, C, K, N] fp64 (fus then ts): the FP32 value 1 / (1 + exp(-clip(z, -50, 50))) widened, in the reference's own
 *     arithmetic (numpy's float32 exp algorithm, fp32 sum and quotient: numpy's bits where it takes its x86 SIMD loop), the
 *     convention of medp_head_scores and the label-major layout medp_resampled_binary_metrics reads;
 *   sens [C-1, K, 3] fp64 = {mean |p_full - p_c| of fus, Pearson correlation of p_full and p_c of fus, mean |p_full - p_c| of ts}
 *     over all N rows, centred two-pass moments; the correlation is NaN when either side has zero variance or N < 2;
 *   entropy [K] fp64 = mean over N of -sum_s a log(max(a, 1e-12)) / max(log S, 1e-12), a = attn / max(sum_s attn, 1e-12);
 *     unwritten when attn is null.
 *   One workgroup per (condition, label), partial sums through LDS in a fixed tree: no floating-point atomics, two launches
 *   are bit-identical.  One workgroup walks a label's N rows (and, for the entropy, one thread a row's S weights), hence
 *   N <= MEDP_TEMPORAL_USAGE_MAX_N, S <= MEDP_TEMPORAL_USAGE_MAX_S and C K <= 65535: beyond them rc < 0, no launch. */
#define MEDP_COUNTERFACTUAL_CONDITIONS 5
#define MEDP_TEMPORAL_USAGE_MAX_N (1 << 22)
#define MEDP_TEMPORAL_USAGE_MAX_S 4096
int medp_counterfactual_feats(const float* const* ts_ptrs, const float* ts_base, long long ts_stride, const float* const* time_ptrs,
                              const float* time_base, long long time_stride, const int* lengths, int T_uniform, const float* static_in,
                              const int* sample_perm, const int* time_perm, float* xs_ts, float* xs_times, float* xs_static, int B,
                              int V, int Ds, int max_len, int Tpad, int Tmax, void* stream);
int medp_temporal_usage_summary(const float* fus, const float* ts, const float* attn, double* prob, double* sens, double* entropy,
                                int C, int N, int K, int S, void* stream);

/* ---- Modality complementarity (analysis/complementarity.py; csrc/complementarity.hip) --------------------------------------
 * medp_youden_thresholds: scores [H, N, K] fp32 (H heads stacked: img, ts, fus), y, mask [N, K] fp32 ->
 *   thr, youden_j [H, K] fp64: `_youden_threshold` (:103-108), thr[argmax(tpr - fpr)] of sklearn's roc_curve(y, score) over the
 *     rows with mask != 0, and the J reached there;  counts [K, 2] int32 = {known rows, known positives (y != 0)}.
 *   One workgroup per (head, label): the known rows are compacted into LDS, sorted descending, one ROC point per DISTINCT score
 *   (-0.0 and +0.0 are one score; a zero threshold carries the sign of the first known row that holds a zero, which is what
 *   sklearn's stable sort reports).  Three properties of roc_curve + argmax are reproduced:
 *     start point    (0, 0) at threshold +inf comes first and argmax keeps the FIRST maximum: no point with J > 0 -> thr = +inf, J = 0;
 *     arithmetic     J = (double)tp / P - (double)fp / Nneg, two rounded fp64 quotients and one difference, compared as such;
 *     dropped points drop_intermediate: an interior point g (0 < g < G-1) whose second differences of tp AND fp are zero is skipped.
 *   The argmax is a fixed-tree reduction on (J, point index), larger J first, then the lower index: two launches are bit-identical.
 *   Fewer than two known rows or one class only: thr = J = NaN.  A non-finite score among the known rows: thr = J = NaN.
 *   The sort stages 8-byte keys in LDS (the arithmetic of medp_resampled_binary_metrics): a label with more than
 *   MEDP_YOUDEN_MAX_LEN known rows gives rc < 0 and the threshold kernel is not launched (for N above the bound the known rows are
 *   counted on the device first and read back: one synchronisation, and `counts` is already written).  Null pointers or
 *   non-positive sizes: rc < 0, no launch.
 * medp_complementarity_cells: scores [3, N, K] fp32, y, mask [N, K] fp32, thr [3, K] fp64 -> cells [K, 16] int32: over the rows
 *   with mask != 0 the count of every combination  (y != 0) | ip << 1 | tp << 2 | fp << 3,  ip / tp / fp = (double)score > thr of the
 *   image / TS / fusion head (numpy's float32 > float64; a NaN or +inf threshold predicts False: `_binarize` :126-135).  Integer
 *   counts only (LDS histograms, integer atomics into the zeroed output): deterministic.  Everything `_analyze_pathology` and
 *   `_plot_venn` report is a function of these 16 integers.  Null pointers or non-positive sizes: rc < 0, no launch. */
#define MEDP_YOUDEN_MAX_LEN MEDP_LDS_SORT_MAX_LEN /* 8-byte keys: 128 KiB of the CU's 160 KiB LDS, a power of two for the bitonic sort */
int medp_youden_thresholds(const float* scores, const float* y, const float* mask, double* thr, double* youden_j, int* counts, int H,
                           int N, int K, void* stream);
int medp_complementarity_cells(const float* scores, const float* y, const float* mask, const double* thr, int* cells, int N, int K,
                               void* stream);

/* ---- Trajectory-availability audit (analysis/trajectory_availability.py; csrc/trajectory_audit.hip) -----------------------
 * medp_trajectory_cells: x [n, T, 2V] fp32 (values | counts, the layout medp_raw_traj_summary reads); a cell is observed iff its
 *   count > 0.  For sample n0 + i and variable v, into variable-major planes [V, ld] (ld >= n0 + n):
 *     obs_hours int32        the number of observed hours;
 *     total fp32             the sum of ALL counts over t, in t order;
 *     recency fp32           n_timesteps - last observed t (n_timesteps need not equal T), NaN if never observed;
 *     within_std fp32        population std (ddof 0) of the observed values, fp64 two-pass, rounded ONCE to fp32; NaN below two hours;
 *     endpoint_change fp32   value[last] - value[first], one fp32 subtraction; NaN below two observed hours;
 *   per_sample [ld, 4] int32 = {#v with >= 1, >= 2, >= 3 observed hours, sum_v obs_hours}: rows [n0, n0 + n) are cleared, then summed;
 *   var_counts [V, 4] int64  = {#samples >= 1, >= 2, >= 3, sum obs_hours}: ADDED to a buffer the caller zeroed before the first chunk.
 *   The value of an unobserved cell enters no figure (NaN / inf there do not leak).  The n0 / ld pair lets a caller stream a
 *   dataset through in chunks and end with full columns: every (sample, variable) is computed by one thread from its own cells, so
 *   chunked calls give bit-identical planes to one call.  Only integer atomics (one per row, figure and workgroup): two launches
 *   are bit-identical.  Null pointers, non-positive sizes, n0 < 0 or ld < n0 + n: rc < 0, no launch.
 * medp_column_medians: n_cols columns of length N at stride ld (elements), fp32 or int32 (is_int32), optionally |.| first
 *   (take_abs) -> median [n_cols] fp64, n_valid [n_cols] int32: what numpy reports.  NaNs are dropped (np.nanmedian); with m valid
 *   entries and a, b the values at sorted ranks (m-1)/2 and m/2: fp32 columns give (float)(a + b) * 0.5f widened to fp64 (m odd: a
 *   itself, numpy averages one element), int32 columns (a + b) / 2.0 in fp64; m = 0 gives NaN.  One workgroup per column selects
 *   rank (m-1)/2 by radix: four 8-bit passes over order-preserving uint32 keys, an LDS histogram per wave, integer atomics; b is
 *   a unless rank m/2 lies past the copies of a, then one more pass finds the smallest key above a.  Nothing is sorted or staged
 *   in LDS, the column is re-read each pass: exact and deterministic for any N <= MEDP_COLUMN_MEDIAN_MAX_N.  -0.0 sorts below
 *   +0.0.  Null pointers, non-positive sizes, ld < N or N above the bound: rc < 0, no launch. */
#define MEDP_COLUMN_MEDIAN_MAX_N (1 << 30) /* every counter is 32-bit unsigned, element offsets are 64-bit */
int medp_trajectory_cells(const float* x, int n, int T, int V, int n_timesteps, int n0, long long ld, int* obs_hours, float* total,
                          float* recency, float* within_std, float* endpoint_change, int* per_sample, long long* var_counts,
                          void* stream);
int medp_column_medians(const void* planes, long long ld, int n_cols, int N, int is_int32, int take_abs, double* median, int* n_valid,
                        void* stream);

/* ---- Conditional-information probe (analysis/conditional_information_probe.py; csrc/cond_probe.hip) -----------------------
 * The device half of a batched damped-Newton fit of Pipeline(StandardScaler, LogisticRegression(C)) with a free, unpenalised
 * intercept.  All arithmetic is fp64; no floating-point atomics; every reduction runs in a fixed order (two launches are
 * bit-identical).  One launch serves P problems, described by a table of MedpProbeProblem: problem p reads the F columns
 * X[r, col_off .. col_off + F) of one fp32 matrix X [N, ldx] for the rows r = rows[row_off .. row_off + n_rows) (int32 indices,
 * ragged: the label's mask) and the labels y[r, y_col] of y fp32 [N, ldy].  The table is passed twice: table_host is checked
 * before anything is launched, table_dev (the same bytes in device memory) is what the kernels read.  rows_total = the length of
 * `rows`; the stretches of the problems follow one another in table order without overlap (per-row values live at a row's
 * position in the list).  A row index outside [0, N) is never dereferenced; it turns the outputs of its problem into NaN.
 * Layouts: theta, g [P, Fmax+1] (standardised space; entries [F, Fmax) are padding, the intercept is LAST, at index Fmax);
 * mean, scale [P, Fmax] (padding: 0 and 1); H [P, Fmax+1, Fmax+1].
 * medp_probe_moments: per problem and column the mean (fp64 sum of the widened values / n), the population variance (two-pass,
 *   centred) and scale = sqrt(var), except that a constant column (var <= n eps var + (n mean eps)^2, StandardScaler's test) keeps 1.
 * medp_logistic_newton_terms: with a_i = ((x_i - mean) / scale, 1), s_i = a_i.theta, p_i = expit(s_i), d_i = p_i (1 - p_i):
 *   f [P] = mean_i BCE(s_i, y_i) + 0.5 l2 sum_{j<F} theta_j^2,  g = mean_i (p_i - y_i) a_i + l2 (theta_0 .. theta_{F-1}, 0) and, when
 *   H is not null, H = mean_i d_i a_i a_i^T + l2 diag(1, .., 1, 0), written exactly symmetric; padded entries of g and H are 0,
 *   with 1 on H's padded diagonal (a padded solve is well posed).  l2 [P] (the caller passes 1 / (C n)).  H = null: the
 *   value-and-gradient mode of a line search.  ws: medp_probe_terms_ws_bytes(P, Fmax, longest problem, rows_total) bytes.
 * medp_probe_scores: out[row_off + i] = sum_{j0 <= j < j1} theta_j (x_ij - mean_j) / scale_j (+ theta[Fmax] when add_intercept)
 *   for the rows of ANY row list (another split, with the training moments); a column range gives one part of a score.
 * All three: rc < 0, nothing launched, for a null pointer, P < 1, F < 1 or F > Fmax, fewer than 2 rows in a problem, columns
 *   outside a row of X, rows outside the list, a label column outside y (terms), a column range outside [0, F] (scores). */
typedef struct {
    long long col_off; /* first column: element offset into a row of X */
    long long row_off; /* its rows: rows[row_off .. row_off + n_rows) */
    int n_rows, F, y_col;
    int j0, j1;        /* medp_probe_scores only: the columns summed */
    int reserved_;
} MedpProbeProblem;
int medp_probe_moments(const float* X, long long ldx, int N, const MedpProbeProblem* table_host, const MedpProbeProblem* table_dev,
                       const int* rows, long long rows_total, double* mean, double* scale, int P, int Fmax, void* stream);
size_t medp_probe_terms_ws_bytes(int P, int Fmax, int max_rows, long long rows_total);
int medp_logistic_newton_terms(const float* X, long long ldx, int N, const float* y, int ldy, const MedpProbeProblem* table_host,
                               const MedpProbeProblem* table_dev, const int* rows, long long rows_total, const double* theta,
                               const double* mean, const double* scale, const double* l2, double* f, double* g, double* H, void* ws,
                               size_t ws_bytes, int P, int Fmax, void* stream);
int medp_probe_scores(const float* X, long long ldx, int N, const MedpProbeProblem* table_host, const MedpProbeProblem* table_dev,
                      const int* rows, long long rows_total, const double* theta, const double* mean, const double* scale, double* out,
                      int P, int Fmax, int add_intercept, void* stream);

/* ---- Linear-head probes (analysis/unimodal_linear_probe.py, analysis/logit_fusion_probe.py; csrc/head_probe.hip) ------------
 * Minibatch AdamW on a tiny head over frozen features: every sequential step of ONE epoch in one launch.  fp32 in storage, as the
 * reference; sums (logits, gradients, the loss, the valid count) are accumulated in fp64 and rounded once.  No floating-point
 * atomics, every reduction in a fixed order: two launches on the same inputs are bit-identical.  functional.precision() is not
 * consulted.
 * medp_head_train_epoch: P independent problems, one workgroup each (a step depends on the one before it; there is no barrier
 *   between workgroups).  Problem p trains z = (x o dropout) W^T + b on the rows perm[s bs .. (s+1) bs) of X for s = 0 .. S-1:
 *     label_width = 0: every label reads the F columns X[r, col0 .. col0 + F); W [L, F]                    (Dropout -> Linear)
 *     label_width = w > 0: label l reads the columns col0 + [l w, (l+1) w), F = L w; W [L, w]              (LogitFusionHead per_label, w = 2)
 *   loss = sum(BCE(z, Y) M) / vc with vc = sum of M over ALL labels of the minibatch; vc = 0: zero gradients, AdamW still steps.
 *   AdamW as torch.optim.AdamW on W and b, weight decay on both; t[0] (device) is the number of steps taken so far and is advanced
 *   by S.  Dropout: element r_in_batch * F + j of step number k = t + 1 (1-based) is kept iff the counter hash of
 *   (seed + k * 0x9E3779B9, stream_id, index) says so (medp_mix_epoch with the problem's own step count; the registered RNG epoch is
 *   not read).  loss_out [2] = {sum over steps of loss * vc, sum of vc}.
 *   A permutation entry outside [0, N) is never dereferenced: W, b and loss_out of its problem become NaN.
 *   W and both moments live in LDS for the epoch when medp_head_train_onchip(F, L, label_width, bs) = 1, in (L2-resident) global
 *   memory otherwise.  The table is passed twice: table_host is checked before anything is launched, table_dev (the same bytes in
 *   device memory) is what the kernel reads.  rc < 0, nothing launched: a null pointer, P < 1, F outside [1, MEDP_HEAD_MAX_F],
 *   L outside [1, MEDP_HEAD_MAX_L], bs outside [1, MEDP_HEAD_MAX_BS], S < 1 or S bs > N, label_width < 0 or L label_width != F,
 *   ldx < col0 + F, ldy < L, dropout_p outside [0, 1).
 * medp_head_scores: logits [n, L] fp32 of the rows `rows` [n] (int32 in [0, N); null: rows 0 .. n-1) under (W, b), label_width
 *   honoured, and probs [L, n] fp64 = the fp32 value 1 / (1 + exp(-logit)) widened: the layout medp_resampled_binary_metrics reads.
 *   A row outside [0, N) is not dereferenced: NaN. */
#define MEDP_HEAD_MAX_F 32768
#define MEDP_HEAD_MAX_L 16
#define MEDP_HEAD_MAX_BS 1024
typedef struct {
    const float* X;         /* [N, ldx] features, read in place */
    const float* Y;         /* [N, ldy] labels */
    const float* M;         /* [N, ldy] 1 = known */
    float* W;               /* [L, F] (label_width 0) or [L, label_width] */
    float* b;               /* [L] */
    float* mW;              /* Adam first / second moments, the shapes of W and b */
    float* vW;
    float* mb;
    float* vb;
    int* t;                 /* [1] steps taken so far */
    const int* perm;        /* [S * bs] this epoch's row order */
    double* loss_out;       /* [2] */
    long long ldx;
    int N, ldy, col0, F, L, label_width, bs, S;
    double lr, weight_decay, beta1, beta2, eps;
    float dropout_p;
    unsigned seed, stream_id;
    int reserved_;
} MedpHeadProblem;
int medp_head_train_onchip(int F, int L, int label_width, int bs);
int medp_head_train_epoch(const MedpHeadProblem* table_host, const MedpHeadProblem* table_dev, int P, void* stream);
int medp_head_scores(const float* X, long long ldx, int N, int col0, int F, int L, int label_width, const float* W, const float* b,
                     const int* rows, int n, float* logits, double* probs, void* stream);

/* ---- Probe heads with a hidden stage (csrc/pool_head_probe.hip) ---------------------------------------------------------------
 * The two heads of the linear-head probes that are not a plain linear map.  fp32 in storage, fp64 accumulators, no floating-point
 * atomics, no wait between workgroups, every reduction in a fixed order: two calls from the same state are bit-identical.
 *
 * Attention-pooled head (LinearHead(use_attn_pool=True)): over X [N, T, d] contiguous,
 *     s_t = x_t . q / sqrt(d),  w = softmax_t(s),  pooled = sum_t w_t x_t,  z = (pooled o dropout) W^T + b,
 *   the masked BCE of medp_head_train_epoch (vc = the known labels of the whole minibatch; vc = 0: zero gradients, AdamW still
 *   steps), torch's AdamW with weight decay on q [d], W [L, d] and b [L].
 * medp_pool_head_train_epoch: the S = pb->S steps of one epoch, TWO launches per step, all enqueued on `stream` by this one call
 *   (no host work between steps that waits for the device, no copy, no synchronisation).  Step s (step number k = step0 + s + 1):
 *     row kernel     grid bs, workgroup r takes row perm[s bs + r]: scores, softmax, pooled, the dropout factor of element r d + j
 *                    from the counter hash of (seed + k * 0x9E3779B9, stream_id, r d + j), logits, vc (every workgroup sums the
 *                    bs L mask values itself, in the same order), g = (sigmoid(z) - y) M / vc, the row's loss part and its backward
 *                    down to dq_row; writes pooled o dropout [d], g [L padded], the loss part and dq_row [d] into `ws`;
 *     column kernel  thread per column j: dW[:, j] and dq[j] summed over the rows IN ORDER in fp64, AdamW on W[:, j] and q[j];
 *                    block 0 also steps b and adds the step's (loss vc, vc) to loss_out [2] (set, not added, at s = 0).
 *   The row's T d tokens stay in LDS for the whole row kernel when medp_pool_head_rows_onchip(T, d) = 1 (16 T + 4 T d bytes within
 *   144 KiB), and are re-read from global memory / L2 otherwise.  The step number is the host scalar step0: the caller adds S
 *   after every call; there is no device counter.  `ws`: medp_pool_head_ws_bytes(d, L, bs) bytes, 16-byte aligned, contents
 *   undefined between calls.  perm_host [S bs] is checked before anything is launched (every entry in [0, N)); pb->perm is the
 *   same array in device memory and is what the kernels read.  rc < 0, nothing launched: a null pointer, T outside [1, 1024],
 *   d outside [1, MEDP_HEAD_MAX_F], L outside [1, MEDP_HEAD_MAX_L], bs outside [1, MEDP_HEAD_MAX_BS], S < 1 or S bs > N, ldy < L,
 *   dropout_p outside [0, 1), step0 < 0, bad AdamW scalars, a permutation entry outside [0, N); a null pb->perm is reported
 *   last, so every other check can be driven without a device.
 * medp_pool_head_scores: the row kernel's forward without dropout for the rows `rows` [n] (int32; null: rows 0 .. n-1):
 *   logits [n, L] fp32 and probs [L, n] fp64 = the fp32 value 1 / (1 + exp(-logit)) widened, as medp_head_scores writes them.
 *   A row outside [0, N) is not dereferenced: NaN.
 *
 * MLP fusion head (LogitFusionHead("mlp")): z = W2 (dropout o gelu(W1 x + b1)) + b2 over the K columns X[r, col0 .. col0 + K), GELU
 *   exact (erf), W1 [H, K], W2 [L, H].
 * medp_mlp_head_train_epoch: P problems, one 512-thread workgroup each, ALL steps of the epoch in one launch, as
 *   medp_head_train_epoch: the four parameter tensors and their Adam moments live in LDS for the epoch, as do the minibatch's
 *   pre-activations and masked hidden activations.  The dropout factor of hidden element r H + k of step number k' = t + 1 comes
 *   from (seed + k' * 0x9E3779B9, stream_id, r H + k); t[0] (device) is advanced by S.  Every gradient sum takes the rows in
 *   order, in fp64.  medp_mlp_head_supported(K, L, H, bs) = 1 when 8 bs H + 4 bs Lpad + 12 (H K + H + L H + L) bytes fit 144 KiB
 *   (Lpad = 2, 8 or 16).  perm_host of every problem is checked before the launch, as above; rc < 0, nothing launched: a null
 *   pointer, P outside [1, 65535], K outside [1, MEDP_MLP_HEAD_MAX_K], H outside [1, MEDP_MLP_HEAD_MAX_H], L, bs, S, ldx, ldy,
 *   dropout_p, AdamW scalars as above, an unsupported shape, a permutation entry outside [0, N); a null table_dev last.
 * medp_mlp_head_scores: logits [n, L] fp32 and probs [L, n] fp64 of the rows `rows` (null: rows 0 .. n-1), no dropout. */
#define MEDP_POOL_HEAD_MAX_T 1024
#define MEDP_MLP_HEAD_MAX_K 64
#define MEDP_MLP_HEAD_MAX_H 1024
typedef struct {
    const float* X;         /* [N, T, d] contiguous */
    const float* Y;         /* [N, ldy] labels */
    const float* M;         /* [N, ldy] 1 = known */
    float* q;               /* [d] attn_query */
    float* W;               /* [L, d] */
    float* b;               /* [L] */
    float* mq;              /* Adam first / second moments, the shapes of q, W and b */
    float* vq;
    float* mW;
    float* vW;
    float* mb;
    float* vb;
    const int* perm;        /* [S * bs] this epoch's row order, device memory */
    void* ws;               /* medp_pool_head_ws_bytes(d, L, bs) bytes */
    double* loss_out;       /* [2] */
    int N, T, d, L, ldy, bs, S;
    int step0;              /* steps taken before this call */
    double lr, weight_decay, beta1, beta2, eps;
    float dropout_p;
    unsigned seed, stream_id;
    int reserved_;
} MedpPoolHeadProblem;
typedef struct {
    const float* X;         /* [N, ldx] the inputs, read in place */
    const float* Y;         /* [N, ldy] */
    const float* M;         /* [N, ldy] */
    float* W1;              /* [H, K] */
    float* b1;              /* [H] */
    float* W2;              /* [L, H] */
    float* b2;              /* [L] */
    float* mom;             /* Adam moments: first then second, each H K + H + L H + L floats in the order W1, b1, W2, b2 */
    int* t;                 /* [1] steps taken so far */
    const int* perm;        /* [S * bs] device memory */
    const int* perm_host;   /* the same entries in host memory: checked, never read by the kernel */
    double* loss_out;       /* [2] */
    long long ldx;
    int N, ldy, col0, K, H, L, bs, S, reserved0_;
    double lr, weight_decay, beta1, beta2, eps;
    float dropout_p;
    unsigned seed, stream_id;
    int reserved_;
} MedpMlpHeadProblem;
int medp_pool_head_rows_onchip(int T, int d);
size_t medp_pool_head_ws_bytes(int d, int L, int bs);
int medp_pool_head_train_epoch(const MedpPoolHeadProblem* pb, const int* perm_host, void* stream);
int medp_pool_head_scores(const float* X, int N, int T, int d, int L, const float* q, const float* W, const float* b, const int* rows,
                          int n, float* logits, double* probs, void* stream);
int medp_mlp_head_supported(int K, int L, int H, int bs);
int medp_mlp_head_train_epoch(const MedpMlpHeadProblem* table_host, const MedpMlpHeadProblem* table_dev, int P, void* stream);
int medp_mlp_head_scores(const float* X, long long ldx, int N, int col0, int K, int H, int L, const float* W1, const float* b1,
                         const float* W2, const float* b2, const int* rows, int n, float* logits, double* probs, void* stream);

/* ---- Gradient-flow diagnostics of the dual teacher (csrc/grad_flow.hip) --------------------------------------------------------
 * The reductions around ONE backward pass over a replicated query bank (grad_flow_diagnostics.py): replica g = (branch, label) of
 * the K pathology queries is seeded with that label's loss cotangent only, so its slice of the replicated leaf's gradient is
 * d(lw_k per_k^branch) / d queries.  fp32 inputs read in place, fp64 accumulators, no floating-point atomics, every accumulator
 * element has one owner, sums over samples go through per-sample partials and a fixed-order workgroup sum: two runs from the same
 * state are bit-identical.  Branch order everywhere: img, ts, fus.  K <= MEDP_GRAD_FLOW_MAX_K, D <= MEDP_GRAD_FLOW_MAX_D,
 * B <= MEDP_GRAD_FLOW_MAX_B; a null pointer (other than the nullable ones named below) or a size outside its range: rc < 0,
 * nothing launched.
 *
 * medp_grad_flow_seeds: logits img / ts / fus [B, K], y, mask [B, K], label_weights [K], pos_weight [K] or null, eps ->
 *     losses  [3, K] fp32      lw_k per_k^branch (per = the masked BCE mean of medp_dual_pathology_loss, whose kernel computes it:
 *                              this call launches it with unit alphas into `ws` and scatters its gradients)
 *     cot_img [B, K, K]        replica g of the image pass: column g = lw_g d per_g^img / d logit[b, g], zero elsewhere
 *     cot_ts  [B, 2K, K]       replica g < K of the time-series pass: column g likewise for the ts branch; replicas g >= K zero
 *     cot_fus [B, 2K, K]       replica K + g: column g for the fusion branch; replicas g < K zero
 *   ws: 4 + 3K + 3BK floats, contents undefined afterwards.
 *
 * medp_grad_flow_accumulate: one call per batch adds to `state` (medp_grad_flow_state_doubles(K, D) doubles, zeroed by the caller):
 *     [0, 3 K K D)             per_label_grad_sums [3, K_label, K, D] += dq
 *     + 3                      loss_sums [3]                          += sum_k losses[r, k]
 *     + 4                      batch_cos_sum += c, negative_count += (c < 0), batch_count += 1, sample_count += B, where
 *                              c = cos(sum_k dq[img, k], sum_k dq[ts, k])  (the branch gradients, by linearity)
 *     + K                      valid_label_count [K]                  += sum_b mask[b, k]
 *     + 4                      fusion sensitivity img_raw, ts_raw, img_scaled, ts_scaled: raw = sum_b ||g_b||, scaled =
 *                              sum_b ||g_b|| ||token_b||, norms over the sample's flattened [K, D], g_b = sum_k dX[b, k]
 *     + 4 K                    the same four per label, [4, K], g_b = dX[b, k]
 *   dq [3, K_label, K, D]; dT [B, K_label, K, D] the fusion replicas' gradients w.r.t. the ts tokens; dI likewise for the image
 *   tokens or null (= zeros: fusion_logits does not depend on them); I, T [B, K, D] the tokens; mask [B, K]; losses [3, K].
 *   ws: medp_grad_flow_ws_doubles(B, K) doubles.  Cosines follow the reference's rule: a denominator <= 1e-12 gives 0.  Two launches.
 *
 * medp_grad_flow_report: state, the three alphas -> out [MEDP_GRAD_FLOW_REPORT_HEAD + MEDP_GRAD_FLOW_REPORT_PER_LABEL K] fp64:
 *     4 r + (0 .. 3)           branch r: loss, ||g||, ||alpha g||, cos(alpha g, sum_r alpha_r g_r)
 *     12 .. 16                 cos img-ts, img-fus, ts-fus of the mean gradients, batch cosine mean, negative batch fraction
 *     17                       ||alpha_img g_img|| / max(||alpha_ts g_ts||, 1e-12)
 *     18 .. 23                 sensitivities / max(samples, 1) in the state's order, raw img / ts, scaled img / ts (max(., 1e-12))
 *     24, 25                   batches, samples
 *     HEAD + 16 k + (0 .. 15)  label k: valid samples; ||g|| per branch; cos img-ts, img-fus, ts-fus; ||sum_r alpha_r g_r||; the
 *                              own-row fractions ||g_r[k, k, :]|| / max(||g_r[k]||, 1e-12) per branch; the four sensitivities
 *                              / max(valid, 1); scaled img / ts
 *   Gradients are means over batches (/ max(batch_count, 1)).  The mean BRANCH gradients are the label sums of the per-label means;
 *   the reference accumulates separately computed branch totals, equal up to rounding.
 *
 * medp_query_geometry: rows [3, K, D] fp32 (the raw prototypes, the image-effective and the ts-effective queries) -> out fp64
 *   [3 K K + K + 1]: the three Gram matrices of the rows divided by max(||row||, 1e-12), the K prototype norms (rows[0]) and
 *   ||G_img - G_ts||_F / K. */
#define MEDP_GRAD_FLOW_MAX_K 16
#define MEDP_GRAD_FLOW_MAX_D 4096
#define MEDP_GRAD_FLOW_MAX_B 4096
#define MEDP_GRAD_FLOW_REPORT_HEAD 26
#define MEDP_GRAD_FLOW_REPORT_PER_LABEL 16
size_t medp_grad_flow_state_doubles(int K, int D);
size_t medp_grad_flow_ws_doubles(int B, int K);
int medp_grad_flow_seeds(const float* img, const float* ts, const float* fus, const float* y, const float* mask,
                         const float* label_weights, const float* pos_weight, float eps, float* ws, float* losses, float* cot_img,
                         float* cot_ts, float* cot_fus, int B, int K, void* stream);
int medp_grad_flow_accumulate(const float* dq, const float* dI, const float* dT, const float* I, const float* T, const float* mask,
                              const float* losses, double* state, double* ws, int B, int K, int D, void* stream);
int medp_grad_flow_report(const double* state, double alpha_img, double alpha_ts, double alpha_fus, double* out, int K, int D,
                          void* stream);
int medp_query_geometry(const float* rows, double* out, int K, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEDP_HIP_H */
