// Probe heads with a hidden stage (reference analysis/unimodal_linear_probe.py `LinearHead(use_attn_pool=True)`,
// analysis/logit_fusion_probe.py `LogitFusionHead("mlp")`; DESIGN.md "Linear-head probes"): minibatch AdamW as in head_probe.hip.
//
// Attention-pooled head.  A minibatch row is T d fp32 tokens (113 KB at T 24, d 1176), a minibatch 14 MB: one workgroup per HEAD
// (head_probe.hip) would stream that through one CU per step.  Here a step is two launches and the stream order is the only
// dependency between workgroups:
//   pool_row_kernel   grid bs, one workgroup per minibatch row.  The row's tokens are read once into LDS (ONCHIP) or re-read from
//                     global memory / L2.  wave per time step: scores; softmax over T; thread per column: pooled, its dropout
//                     factor, the partial logits (block-reduced in wave order); vc of the whole minibatch, summed by every
//                     workgroup in the same order; g, the loss part; then backward: dpooled (thread per column), dw_t (wave per
//                     time step), ds_t, dq_row (thread per column).  Writes pooled o dropout, g, the loss part, dq_row to ws.
//   pool_col_kernel   thread per column j: dW[:, j], dq[j] over the rows in order, AdamW; block 0: b and the loss sums.
//   pool_scores_kernel  the row kernel's forward without dropout, one workgroup per scored row.
// MLP fusion head.  Everything is tiny (H = 32, K = 2 L <= 32): the pattern of head_train_epoch_kernel, one workgroup per problem,
// all steps of the epoch in one launch, parameters, moments and the minibatch's activations in LDS.
//   A  thread per (row, hidden unit): pre-activation, exact GELU, dropout     C1  thread per (row, hidden unit): d pre-activation
//   B  thread per (row, label): logits; vc, g, the loss                       C2  thread per parameter: its gradient over the rows
//                                                                                 in order, AdamW
// fp32 in storage; fp64 accumulators; no floating-point atomics; every reduction in a fixed order.  The rules shared with
// head_probe.hip are head_rules.h: the pool head's host loop and mlp_epoch step the same HeadSchedule as head_epoch, and the two
// launchers check their steps, permutations and columns with the same functions.
#include "common.h"
#include "head_rules.h"
#include "medp_hip.h"

namespace {

constexpr int PH_THREADS = 512, PH_WAVES = PH_THREADS / 64;
constexpr int PC_THREADS = 256;                                              // column kernel
constexpr int MS_THREADS = 256;                                              // mlp scores: thread per row

// ---- attention-pooled head ------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long pool_small_bytes(int T) { return 16LL * T; }            // w [T], dw [T] in fp64
__host__ __device__ inline bool pool_onchip(int T, int d) { return pool_small_bytes(T) + 4LL * T * d <= HEAD_LDS_BUDGET; }

struct PoolWs {
    double* lossp;   // [bs] the rows' loss parts
    double* vc;      // [1]
    float* g;        // [bs, LP]
    float* pooled;   // [bs, d] pooled o dropout
    float* dq;       // [bs, d] dq_row (dpooled on the way)
};
__host__ __device__ inline PoolWs pool_ws(void* ws, int d, int L, int bs) {
    PoolWs w;
    w.lossp = (double*)ws;
    w.vc = w.lossp + bs;
    w.g = (float*)(w.vc + 1);
    w.pooled = w.g + (size_t)bs * head_lp(L);
    w.dq = w.pooled + (size_t)bs * d;
    return w;
}
__host__ __device__ inline size_t pool_ws_bytes(int d, int L, int bs) {
    return 8 * ((size_t)bs + 1) + 4 * ((size_t)bs * head_lp(L) + 2 * (size_t)bs * d);
}

struct PoolShared {
    double red[PH_WAVES];
    double zred[PH_WAVES][MEDP_HEAD_MAX_L];
    double lsh[MEDP_HEAD_MAX_L];
    float zs[MEDP_HEAD_MAX_L];
    float gsh[MEDP_HEAD_MAX_L];
};

// Forward of one row: the softmax weights into wv [T], the logits into sh.zs; returns the pointer the tokens are read through.
template <int LP, bool ONCHIP>
__device__ __forceinline__ const float* pool_forward(const float* __restrict__ xg, float* xs, double* wv, PoolShared& sh, const float* q,
                                                     const float* W, const float* b, int T, int d, int L, bool drop, uint32_t seed,
                                                     uint32_t sid, uint32_t idx0, float p, float inv_keep, float* pooled_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ONCHIP) {
        if (((T * d) & 3) == 0 && ((size_t)xg & 15) == 0) {                // xs is 16-byte aligned: 16 T bytes into the LDS image
            for (int e = tid; e < (T * d) >> 2; e += PH_THREADS) ((f32x4*)xs)[e] = ((const f32x4*)xg)[e];
        } else {
            for (int e = tid; e < T * d; e += PH_THREADS) xs[e] = xg[e];
        }
        __syncthreads();
    }
    const float* x = ONCHIP ? xs : xg;
    const double sqrt_d = sqrt((double)d);
    for (int t = wave; t < T; t += PH_WAVES) {
        const float* xt = x + t * d;
        double acc = 0.0;
#pragma unroll 2
        for (int j = lane; j < d; j += 64) acc = fma((double)xt[j], (double)q[j], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) wv[t] = acc / sqrt_d;
    }
    __syncthreads();
    double mx = wv[0];
    for (int t = 1; t < T; ++t) mx = fmax(mx, wv[t]);
    __syncthreads();
    for (int t = tid; t < T; t += PH_THREADS) wv[t] = exp(wv[t] - mx);
    __syncthreads();
    double den = 0.0;
    for (int t = 0; t < T; ++t) den += wv[t];
    __syncthreads();
    for (int t = tid; t < T; t += PH_THREADS) wv[t] = wv[t] / den;
    __syncthreads();
    double acc[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) acc[l] = 0.0;
    for (int j = tid; j < d; j += PH_THREADS) {
        double pj = 0.0;
        for (int t = 0; t < T; ++t) pj = fma(wv[t], (double)x[t * d + j], pj);
        float pm = (float)pj;
        if (drop) pm *= dropout_scale(seed, sid, idx0 + (uint32_t)j, p, inv_keep);
        if (pooled_out) pooled_out[j] = pm;
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) acc[l] = fma((double)pm, (double)W[(size_t)l * d + j], acc[l]);
    }
#pragma unroll
    for (int l = 0; l < LP; ++l) {
        acc[l] = wave_sum_f64(acc[l]);
        if (lane == 0) sh.zred[wave][l] = acc[l];
    }
    __syncthreads();
    if (tid < L) {
        double z = 0.0;
#pragma unroll
        for (int w = 0; w < PH_WAVES; ++w) z += sh.zred[w][tid];
        sh.zs[tid] = (float)(z + (double)b[tid]);
    }
    __syncthreads();
    return x;
}

// grid bs; `perm` points at this step's bs entries, `seed` has the step number mixed in
template <int LP, bool ONCHIP>
__global__ __launch_bounds__(PH_THREADS) void pool_row_kernel(MedpPoolHeadProblem pb, const int* __restrict__ perm, uint32_t seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
    __shared__ PoolShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = pb.T, d = pb.d, L = pb.L, bs = pb.bs, r = blockIdx.x;
    double* wv = (double*)pool_smem;
    double* dwv = wv + T;
    float* xs = (float*)(dwv + T);
    const PoolWs ws = pool_ws(pb.ws, d, L, bs);
    const int row = perm[r];
    const float p = pb.dropout_p, inv_keep = 1.f / (1.f - p);
    const bool drop = p > 0.f;
    const uint32_t idx0 = (uint32_t)r * (uint32_t)d;
    const float* x = pool_forward<LP, ONCHIP>(pb.X + (size_t)row * T * d, xs, wv, sh, pb.q, pb.W, pb.b, T, d, L, drop, seed, pb.stream_id,
                                              idx0, p, inv_keep, ws.pooled + (size_t)r * d);
    // ---- vc over the whole minibatch (every workgroup, the same order), g and the row's loss part
    double part = 0.0;
    for (int e = tid; e < bs * L; e += PH_THREADS) part += (double)pb.M[(size_t)perm[e / L] * pb.ldy + e % L];
    const double vc = block_sum_wave_order_f64<PH_WAVES>(part, sh.red);
    if (tid < LP) {
        float g = 0.f;
        double lt = 0.0;
        if (tid < L) {
            const size_t o = (size_t)row * pb.ldy + tid;
            lt = masked_bce_term((double)sh.zs[tid], (double)pb.Y[o], (double)pb.M[o], vc, &g);
        }
        sh.gsh[tid] = g;
        sh.lsh[tid] = lt;
        ws.g[(size_t)r * LP + tid] = g;                                      // the label padding is written as zero
    }
    __syncthreads();
    if (tid == 0) {
        double ls = 0.0;
        for (int l = 0; l < L; ++l) ls += sh.lsh[l];
        ws.lossp[r] = ls;
        if (r == 0) ws.vc[0] = vc;
    }
    // ---- backward: dpooled_j = mask_j sum_l g_l W[l, j]
    float* dp = ws.dq + (size_t)r * d;
    for (int j = tid; j < d; j += PH_THREADS) {
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) a = fma((double)sh.gsh[l], (double)pb.W[(size_t)l * d + j], a);
        float v = (float)a;
        if (drop) v *= dropout_scale(seed, pb.stream_id, idx0 + (uint32_t)j, p, inv_keep);
        dp[j] = v;
    }
    __syncthreads();
    // dw_t = dpooled . x_t
    for (int t = wave; t < T; t += PH_WAVES) {
        const float* xt = x + t * d;
        double acc = 0.0;
#pragma unroll 2
        for (int j = lane; j < d; j += 64) acc = fma((double)dp[j], (double)xt[j], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) dwv[t] = acc;
    }
    __syncthreads();
    // ds_t = w_t (dw_t - sum_u w_u dw_u) / sqrt(d)
    double c = 0.0;
    for (int u = 0; u < T; ++u) c = fma(wv[u], dwv[u], c);
    __syncthreads();
    const double sqrt_d = sqrt((double)d);
    for (int t = tid; t < T; t += PH_THREADS) dwv[t] = wv[t] * (dwv[t] - c) / sqrt_d;
    __syncthreads();
    // dq_row_j = sum_t ds_t x[t, j]
    for (int j = tid; j < d; j += PH_THREADS) {
        double a = 0.0;
        for (int t = 0; t < T; ++t) a = fma(dwv[t], (double)x[t * d + j], a);
        dp[j] = (float)a;
    }
}

// grid ceil(d / PC_THREADS)
template <int LP>
__global__ __launch_bounds__(PC_THREADS) void pool_col_kernel(MedpPoolHeadProblem pb, AdamScalars a, int first) {
    const int tid = threadIdx.x, j = blockIdx.x * PC_THREADS + tid;
    const int d = pb.d, L = pb.L, bs = pb.bs;
    const PoolWs ws = pool_ws(pb.ws, d, L, bs);
    if (j < d) {
        double acc[LP], dq = 0.0;
#pragma unroll
        for (int l = 0; l < LP; ++l) acc[l] = 0.0;
#pragma unroll 4
        for (int r = 0; r < bs; ++r) {
            const double pm = (double)ws.pooled[(size_t)r * d + j];
#pragma unroll
            for (int l = 0; l < LP; ++l) acc[l] = fma((double)ws.g[(size_t)r * LP + l], pm, acc[l]);
            dq += (double)ws.dq[(size_t)r * d + j];
        }
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) adamw(pb.W + (size_t)l * d + j, pb.mW + (size_t)l * d + j, pb.vW + (size_t)l * d + j, (float)acc[l], a);
        adamw(pb.q + j, pb.mq + j, pb.vq + j, (float)dq, a);
    }
    if (blockIdx.x == 0) {
        if (tid < L) {
            double acc = 0.0;
            for (int r = 0; r < bs; ++r) acc += (double)ws.g[(size_t)r * LP + tid];
            adamw(pb.b + tid, pb.mb + tid, pb.vb + tid, (float)acc, a);
        }
        if (tid == 64) {
            double ls = 0.0;
            for (int r = 0; r < bs; ++r) ls += ws.lossp[r];
            const double vc = ws.vc[0];
            double run_l = first ? 0.0 : pb.loss_out[0], run_v = first ? 0.0 : pb.loss_out[1];
            add_step_loss(run_l, run_v, ls, vc);
            pb.loss_out[0] = run_l;
            pb.loss_out[1] = run_v;
        }
    }
}

// grid n
template <int LP, bool ONCHIP>
__global__ __launch_bounds__(PH_THREADS) void pool_scores_kernel(const float* __restrict__ X, int N, int T, int d, int L, const float* q,
                                                                  const float* W, const float* b, const int* __restrict__ rows, int n,
                                                                  float* __restrict__ logits, double* __restrict__ probs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
    __shared__ PoolShared sh;
    const int tid = threadIdx.x, i = blockIdx.x;
    const int row = rows ? rows[i] : i;
    const bool ok = (unsigned)row < (unsigned)N;                             // uniform over the workgroup
    if (ok) {
        double* wv = (double*)pool_smem;
        float* xs = (float*)(wv + 2 * T);
        pool_forward<LP, ONCHIP>(X + (size_t)row * T * d, xs, wv, sh, q, W, b, T, d, L, false, 0u, 0u, 0u, 0.f, 1.f, nullptr);
    }
    if (tid < L) head_store_score(logits, probs, i, tid, L, n, ok, sh.zs[tid]);
}

size_t pool_lds_bytes(int T, int d) { return (size_t)(pool_small_bytes(T) + (pool_onchip(T, d) ? 4LL * T * d : 0)); }

template <int LP, bool ONCHIP>
int launch_pool_row(const MedpPoolHeadProblem& pb, const int* perm, uint32_t seed, hipStream_t st) {
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)pool_row_kernel<LP, ONCHIP>, hipFuncAttributeMaxDynamicSharedMemorySize, HEAD_LDS_BUDGET);
    });
    pool_row_kernel<LP, ONCHIP><<<pb.bs, PH_THREADS, pool_lds_bytes(pb.T, pb.d), st>>>(pb, perm, seed);
    MEDP_LAUNCH_CHECK("medp_pool_head_train_epoch (row kernel)");
    return 0;
}
template <int LP>
int launch_pool_step(const MedpPoolHeadProblem& pb, const int* perm, uint32_t seed, const AdamScalars& a, int first, hipStream_t st) {
    if (pool_onchip(pb.T, pb.d)) MEDP_TRY((launch_pool_row<LP, true>(pb, perm, seed, st)));
    else MEDP_TRY((launch_pool_row<LP, false>(pb, perm, seed, st)));
    pool_col_kernel<LP><<<(pb.d + PC_THREADS - 1) / PC_THREADS, PC_THREADS, 0, st>>>(pb, a, first);
    MEDP_LAUNCH_CHECK("medp_pool_head_train_epoch (column kernel)");
    return 0;
}

template <int LP, bool ONCHIP>
int launch_pool_scores(const float* X, int N, int T, int d, int L, const float* q, const float* W, const float* b, const int* rows, int n,
                       float* logits, double* probs, hipStream_t st) {
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)pool_scores_kernel<LP, ONCHIP>, hipFuncAttributeMaxDynamicSharedMemorySize, HEAD_LDS_BUDGET);
    });
    pool_scores_kernel<LP, ONCHIP><<<n, PH_THREADS, pool_lds_bytes(T, d), st>>>(X, N, T, d, L, q, W, b, rows, n, logits, probs);
    MEDP_LAUNCH_CHECK("medp_pool_head_scores");
    return 0;
}

int check_pool_shape(const char* what, int N, int T, int d, int L) {
    MEDP_CHECK_ARG(T >= 1 && T <= MEDP_POOL_HEAD_MAX_T, "%s: T=%d is not in [1, %d]", what, T, MEDP_POOL_HEAD_MAX_T);
    MEDP_CHECK_ARG(d >= 1 && d <= MEDP_HEAD_MAX_F, "%s: d=%d is not in [1, %d]", what, d, MEDP_HEAD_MAX_F);
    MEDP_CHECK_ARG(L >= 1 && L <= MEDP_HEAD_MAX_L, "%s: L=%d is not in [1, %d]", what, L, MEDP_HEAD_MAX_L);
    MEDP_CHECK_ARG(N >= 1, "%s: N=%d < 1", what, N);
    return 0;
}

// ---- MLP fusion head ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long mlp_np(int K, int L, int H) { return (long long)H * K + H + (long long)L * H + L; }
__host__ __device__ inline long long mlp_lds_bytes(int K, int L, int H, int bs) {
    return 8LL * bs * H + 4LL * bs * head_lp(L) + 12 * mlp_np(K, L, H);
}

__device__ __forceinline__ float gelu_exact(float a) {
    return (float)(0.5 * (double)a * (1.0 + erf((double)a * 0.70710678118654752440)));
}
__device__ __forceinline__ float gelu_exact_grad(float a) {
    const double x = (double)a;
    return (float)(0.5 * (1.0 + erf(x * 0.70710678118654752440)) + x * 0.39894228040143267794 * exp(-0.5 * x * x));
}

template <int LP>
__device__ __forceinline__ void mlp_epoch(const MedpMlpHeadProblem& pb, float* smem, double* red) {
    const int tid = threadIdx.x;
    const int K = pb.K, H = pb.H, L = pb.L, bs = pb.bs;
    const int np = (int)mlp_np(K, L, H), oB1 = H * K, oW2 = oB1 + H, oB2 = oW2 + L * H;
    float* par = smem;
    float* mo1 = par + np;
    float* mo2 = mo1 + np;
    float* pre = mo2 + np;
    float* hm = pre + bs * H;
    float* gs = hm + bs * H;
    const float *W1 = par, *b1 = par + oB1, *W2 = par + oW2, *b2 = par + oB2;
    for (int e = tid; e < np; e += PH_THREADS) {
        par[e] = e < oB1 ? pb.W1[e] : e < oW2 ? pb.b1[e - oB1] : e < oB2 ? pb.W2[e - oW2] : pb.b2[e - oB2];
        mo1[e] = pb.mom[e];
        mo2[e] = pb.mom[np + e];
    }
    for (int e = tid; e < bs * LP; e += PH_THREADS) gs[e] = 0.f;          // the label padding stays zero
    __syncthreads();
    const float* Xc = pb.X + pb.col0;
    const float p = pb.dropout_p, inv_keep = 1.f / (1.f - p);
    const bool drop = p > 0.f;
    const int t0 = pb.t[0];
    AdamScalars a;
    HeadSchedule sched(a, pb.lr, pb.weight_decay, pb.beta1, pb.beta2, pb.eps, pb.seed, t0);
    double run_l = 0.0, run_v = 0.0;
    for (int s = 0; s < pb.S; ++s) {
        const uint32_t seed = sched.advance(a);
        const int* pr = pb.perm + (size_t)s * bs;
        // ---- A: pre-activations and the masked hidden activations
        for (int e = tid; e < bs * H; e += PH_THREADS) {
            const int r = e / H, k = e % H;
            const float* xr = Xc + (size_t)pr[r] * pb.ldx;
            double acc = (double)b1[k];
            for (int i = 0; i < K; ++i) acc = fma((double)xr[i], (double)W1[k * K + i], acc);
            const float af = (float)acc;
            pre[e] = af;
            float h = gelu_exact(af);
            if (drop) h *= dropout_scale(seed, pb.stream_id, (uint32_t)e, p, inv_keep);
            hm[e] = h;
        }
        __syncthreads();
        // ---- B: logits into gs
        for (int e = tid; e < bs * L; e += PH_THREADS) {
            const int r = e / L, l = e % L;
            double acc = (double)b2[l];
            for (int k = 0; k < H; ++k) acc = fma((double)hm[r * H + k], (double)W2[l * H + k], acc);
            gs[r * LP + l] = (float)acc;
        }
        double part = 0.0;
        for (int e = tid; e < bs * L; e += PH_THREADS) part += (double)pb.M[(size_t)pr[e / L] * pb.ldy + e % L];
        const double vc = block_sum_wave_order_f64<PH_WAVES>(part, red);    // its barriers also publish the logits
        part = 0.0;
        for (int e = tid; e < bs * L; e += PH_THREADS) {
            const int r = e / L, l = e % L;
            const size_t o = (size_t)pr[r] * pb.ldy + l;
            part += masked_bce_term((double)gs[r * LP + l], (double)pb.Y[o], (double)pb.M[o], vc, gs + r * LP + l);
        }
        add_step_loss(run_l, run_v, block_sum_wave_order_f64<PH_WAVES>(part, red), vc);       // the sum's barriers publish g
        // ---- C1: d pre-activation = mask (g W2) gelu'(pre), in place of the pre-activation
        for (int e = tid; e < bs * H; e += PH_THREADS) {
            const int r = e / H, k = e % H;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < LP; ++l)
                if (l < L) acc = fma((double)gs[r * LP + l], (double)W2[l * H + k], acc);
            float dh = (float)acc;
            if (drop) dh *= dropout_scale(seed, pb.stream_id, (uint32_t)e, p, inv_keep);
            pre[e] = dh * gelu_exact_grad(pre[e]);
        }
        __syncthreads();
        // ---- C2: every parameter's gradient over the rows in order, AdamW
        for (int e = tid; e < np; e += PH_THREADS) {
            double acc = 0.0;
            if (e < oB1) {
                const int k = e / K, i = e % K;
                for (int r = 0; r < bs; ++r) acc = fma((double)pre[r * H + k], (double)Xc[(size_t)pr[r] * pb.ldx + i], acc);
            } else if (e < oW2) {
                const int k = e - oB1;
                for (int r = 0; r < bs; ++r) acc += (double)pre[r * H + k];
            } else if (e < oB2) {
                const int l = (e - oW2) / H, k = (e - oW2) % H;
                for (int r = 0; r < bs; ++r) acc = fma((double)gs[r * LP + l], (double)hm[r * H + k], acc);
            } else {
                const int l = e - oB2;
                for (int r = 0; r < bs; ++r) acc += (double)gs[r * LP + l];
            }
            adamw(par + e, mo1 + e, mo2 + e, (float)acc, a);
        }
        __syncthreads();                                                     // this step's parameters before the next step's forward
    }
    for (int e = tid; e < np; e += PH_THREADS) {
        float* dst = e < oB1 ? pb.W1 + e : e < oW2 ? pb.b1 + (e - oB1) : e < oB2 ? pb.W2 + (e - oW2) : pb.b2 + (e - oB2);
        *dst = par[e];
        pb.mom[e] = mo1[e];
        pb.mom[np + e] = mo2[e];
    }
    if (tid == 0) {
        pb.t[0] = t0 + pb.S;
        pb.loss_out[0] = run_l;
        pb.loss_out[1] = run_v;
    }
}

__global__ __launch_bounds__(PH_THREADS) void mlp_head_train_epoch_kernel(const MedpMlpHeadProblem* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    __shared__ double red[PH_WAVES];
    const MedpMlpHeadProblem pb = tab[blockIdx.x];
    with_head_lp(pb.L, [&](auto lp) { mlp_epoch<lp>(pb, (float*)mlp_smem, red); });
}

// thread per scored row
template <int LP>
__device__ __forceinline__ void mlp_scores_row(const float* __restrict__ X, long long ldx, int N, int col0, int K, int H, int L,
                                               const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                               const float* __restrict__ b2, const int* __restrict__ rows, int n, float* __restrict__ logits,
                                               double* __restrict__ probs) {
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int row = rows ? rows[i] : i;
    const bool ok = (unsigned)row < (unsigned)N;
    double acc[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) acc[l] = 0.0;
    if (ok) {
        const float* xr = X + (size_t)row * ldx + col0;
        for (int k = 0; k < H; ++k) {
            double a = (double)b1[k];
            for (int c = 0; c < K; ++c) a = fma((double)xr[c], (double)W1[k * K + c], a);
            const double h = (double)gelu_exact((float)a);
#pragma unroll
            for (int l = 0; l < LP; ++l)
                if (l < L) acc[l] = fma(h, (double)W2[l * H + k], acc[l]);
        }
    }
#pragma unroll
    for (int l = 0; l < LP; ++l)
        if (l < L) head_store_score(logits, probs, i, l, L, n, ok, (float)(acc[l] + (double)b2[l]));
}

__global__ __launch_bounds__(MS_THREADS) void mlp_head_scores_kernel(const float* __restrict__ X, long long ldx, int N, int col0, int K, int H,
                                                                      int L, const float* __restrict__ W1, const float* __restrict__ b1,
                                                                      const float* __restrict__ W2, const float* __restrict__ b2,
                                                                      const int* __restrict__ rows, int n, float* __restrict__ logits,
                                                                      double* __restrict__ probs) {
    with_head_lp(L, [&](auto lp) { mlp_scores_row<lp>(X, ldx, N, col0, K, H, L, W1, b1, W2, b2, rows, n, logits, probs); });
}

int check_mlp_shape(const char* what, int p, long long ldx, int N, int col0, int K, int H, int L) {
    MEDP_CHECK_ARG(K >= 1 && K <= MEDP_MLP_HEAD_MAX_K, "%s: problem %d has K=%d, not in [1, %d]", what, p, K, MEDP_MLP_HEAD_MAX_K);
    MEDP_CHECK_ARG(H >= 1 && H <= MEDP_MLP_HEAD_MAX_H, "%s: problem %d has H=%d, not in [1, %d]", what, p, H, MEDP_MLP_HEAD_MAX_H);
    return check_labels_and_columns(what, p, ldx, N, col0, K, L);
}

}  // namespace

extern "C" int medp_pool_head_rows_onchip(int T, int d) {
    if (T < 1 || T > MEDP_POOL_HEAD_MAX_T || d < 1 || d > MEDP_HEAD_MAX_F) return 0;
    return pool_onchip(T, d) ? 1 : 0;
}

extern "C" size_t medp_pool_head_ws_bytes(int d, int L, int bs) {
    if (d < 1 || L < 1 || L > MEDP_HEAD_MAX_L || bs < 1) return 0;
    return pool_ws_bytes(d, L, bs);
}

extern "C" int medp_pool_head_train_epoch(const MedpPoolHeadProblem* pbp, const int* perm_host, void* stream) {
    const char* what = "pool_head_train_epoch";
    MEDP_CHECK_ARG(pbp, "%s: null problem", what);
    const MedpPoolHeadProblem& pb = *pbp;
    MEDP_CHECK_ARG(pb.X && pb.Y && pb.M && pb.q && pb.W && pb.b && pb.mq && pb.vq && pb.mW && pb.vW && pb.mb && pb.vb && pb.ws && pb.loss_out
                       && perm_host,
                   "%s: null pointer", what);
    MEDP_TRY(check_pool_shape(what, pb.N, pb.T, pb.d, pb.L));
    MEDP_CHECK_ARG(pb.ldy >= pb.L, "%s: ldy=%d < L=%d", what, pb.ldy, pb.L);
    MEDP_TRY(check_steps(what, 0, pb.N, pb.bs, pb.S, pb.dropout_p, pb.lr, pb.beta1, pb.beta2, pb.eps));
    MEDP_CHECK_ARG(pb.step0 >= 0, "%s: step0=%d < 0", what, pb.step0);
    MEDP_CHECK_ARG(((size_t)pb.ws & 15) == 0, "%s: the workspace is not 16-byte aligned", what);
    MEDP_TRY(check_perm(what, 0, perm_host, (long long)pb.S * pb.bs, pb.N));
    MEDP_CHECK_ARG(pb.perm, "%s: null device permutation", what);           // after the checks: they can be driven without a device
    AdamScalars a;
    HeadSchedule sched(a, pb.lr, pb.weight_decay, pb.beta1, pb.beta2, pb.eps, pb.seed, pb.step0);
    for (int s = 0; s < pb.S; ++s) {
        const uint32_t seed = sched.advance(a);
        const int* perm = pb.perm + (size_t)s * pb.bs;
        MEDP_TRY(with_head_lp(pb.L, [&](auto lp) { return launch_pool_step<lp>(pb, perm, seed, a, s == 0, (hipStream_t)stream); }));
    }
    return 0;
}

extern "C" int medp_pool_head_scores(const float* X, int N, int T, int d, int L, const float* q, const float* W, const float* b,
                                     const int* rows, int n, float* logits, double* probs, void* stream) {
    MEDP_TRY(check_pool_shape("pool_head_scores", N, T, d, L));
    MEDP_CHECK_ARG(n >= 1, "pool_head_scores: n=%d < 1", n);
    MEDP_CHECK_ARG(X && q && W && b && logits && probs, "pool_head_scores: null argument");
    hipStream_t st = (hipStream_t)stream;
    return with_head_lp(L, [&](auto lp) {
        return pool_onchip(T, d) ? launch_pool_scores<lp, true>(X, N, T, d, L, q, W, b, rows, n, logits, probs, st)
                                 : launch_pool_scores<lp, false>(X, N, T, d, L, q, W, b, rows, n, logits, probs, st);
    });
}

extern "C" int medp_mlp_head_supported(int K, int L, int H, int bs) {
    if (K < 1 || K > MEDP_MLP_HEAD_MAX_K || L < 1 || L > MEDP_HEAD_MAX_L || H < 1 || H > MEDP_MLP_HEAD_MAX_H || bs < 1 || bs > MEDP_HEAD_MAX_BS)
        return 0;
    return mlp_lds_bytes(K, L, H, bs) <= HEAD_LDS_BUDGET ? 1 : 0;
}

extern "C" int medp_mlp_head_train_epoch(const MedpMlpHeadProblem* table_host, const MedpMlpHeadProblem* table_dev, int P, void* stream) {
    const char* what = "mlp_head_train_epoch";
    MEDP_CHECK_ARG(table_host, "%s: null host table", what);
    MEDP_CHECK_ARG(P >= 1 && P <= 65535, "%s: P=%d is not in [1, 65535]", what, P);
    long long lds = 0;
    for (int p = 0; p < P; ++p) {
        const MedpMlpHeadProblem& q = table_host[p];
        MEDP_CHECK_ARG(q.X && q.Y && q.M && q.W1 && q.b1 && q.W2 && q.b2 && q.mom && q.t && q.perm && q.perm_host && q.loss_out,
                       "%s: problem %d has a null pointer", what, p);
        MEDP_TRY(check_mlp_shape(what, p, q.ldx, q.N, q.col0, q.K, q.H, q.L));
        MEDP_CHECK_ARG(q.ldy >= q.L, "%s: problem %d has ldy=%d < L=%d", what, p, q.ldy, q.L);
        MEDP_TRY(check_steps(what, p, q.N, q.bs, q.S, q.dropout_p, q.lr, q.beta1, q.beta2, q.eps));
        const long long need = mlp_lds_bytes(q.K, q.L, q.H, q.bs);
        MEDP_CHECK_ARG(need <= HEAD_LDS_BUDGET, "%s: problem %d (K=%d, H=%d, L=%d, bs=%d) needs %lld bytes of LDS, more than %d", what, p, q.K,
                       q.H, q.L, q.bs, need, HEAD_LDS_BUDGET);
        MEDP_TRY(check_perm(what, p, q.perm_host, (long long)q.S * q.bs, q.N));
        lds = need > lds ? need : lds;
    }
    MEDP_CHECK_ARG(table_dev, "%s: null device table", what);               // after the checks: the host copy alone can be validated
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)mlp_head_train_epoch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HEAD_LDS_BUDGET);
    });
    mlp_head_train_epoch_kernel<<<P, PH_THREADS, (size_t)lds, (hipStream_t)stream>>>(table_dev);
    MEDP_LAUNCH_CHECK("medp_mlp_head_train_epoch");
    return 0;
}

extern "C" int medp_mlp_head_scores(const float* X, long long ldx, int N, int col0, int K, int H, int L, const float* W1, const float* b1,
                                    const float* W2, const float* b2, const int* rows, int n, float* logits, double* probs, void* stream) {
    MEDP_TRY(check_mlp_shape("mlp_head_scores", 0, ldx, N, col0, K, H, L));
    MEDP_CHECK_ARG(n >= 1, "mlp_head_scores: n=%d < 1", n);
    MEDP_CHECK_ARG(X && W1 && b1 && W2 && b2 && logits && probs, "mlp_head_scores: null argument");
    mlp_head_scores_kernel<<<(n + MS_THREADS - 1) / MS_THREADS, MS_THREADS, 0, (hipStream_t)stream>>>(X, ldx, N, col0, K, H, L, W1, b1, W2, b2,
                                                                                                     rows, n, logits, probs);
    MEDP_LAUNCH_CHECK("medp_mlp_head_scores");
    return 0;
}
