// Linear-head probes (reference analysis/unimodal_linear_probe.py `train_linear_head`, analysis/logit_fusion_probe.py
// `train_fusion_head`; DESIGN.md "Linear-head probes"): minibatch AdamW on a tiny head over frozen features.
//
//   head_train_epoch_kernel  ALL sequential steps of one epoch of one problem per workgroup (grid = P problems).  A step:
//       A  logits     wave per minibatch row, lanes stride the columns, one fp64 accumulator per label, a fixed butterfly;
//       -  vc, g      vc = sum of M over the whole minibatch (a fixed-order block sum), g = (sigmoid(z) - y) M / vc into LDS,
//                     the loss sum beside it;
//       B  update     thread per column: dW[:, j] = sum over the rows IN ORDER of g[r, :] x[r, j] in fp64, then torch's AdamW on
//                     W[:, j] and its moments; thread l < L does the same for b[l].
//     The dropout factor of element (r, j) is regenerated from the counter hash in A and in B.  W and the two moments live in LDS
//     for the whole epoch when they fit (head_onchip), in global memory (a few hundred KB: L2-resident) otherwise; b and its
//     moments (<= 16 values) stay in global memory.  No workgroup waits for another.
//   head_scores_kernel       logits and fp32 sigmoid probabilities of a row list, the summation order of phase A.
// fp32 in storage; fp64 accumulators; no floating-point atomics; every reduction in a fixed order.  What a head has in common with
// those of pool_head_probe.hip (step clock, AdamW, masked BCE, loss sums, score store, label-padding dispatch, the launchers' checks
// of steps and columns) is head_rules.h; here are the linear head's own loops.
#include "common.h"
#include "head_rules.h"
#include "medp_hip.h"

namespace {

constexpr int HT_THREADS = 512, HT_WAVES = HT_THREADS / 64;
constexpr int HS_THREADS = 256, HS_WAVES = HS_THREADS / 64, HS_ROWS = 32;   // scores: rows per workgroup

__host__ __device__ inline long long head_nw(int F, int L, int w) { return w == 0 ? (long long)L * F : (long long)F; }
__host__ __device__ inline long long head_g_bytes(int L, int bs) { return (long long)bs * head_lp(L) * 4; }
__host__ __device__ inline bool head_onchip(int F, int L, int w, int bs) {
    return head_g_bytes(L, bs) + 12 * head_nw(F, L, w) <= HEAD_LDS_BUDGET;
}

// dot products of one row with every label's weights: lanes stride the columns, the result (all lanes) per label in acc[]
template <int LP>
__device__ __forceinline__ void row_dots(const float* __restrict__ xr, const float* Wp, int F, int L, int lane, bool drop, uint32_t seed,
                                         uint32_t sid, uint32_t idx0, float p, float inv_keep, double (&acc)[LP]) {
#pragma unroll
    for (int l = 0; l < LP; ++l) acc[l] = 0.0;
#pragma unroll 2
    for (int j = lane; j < F; j += 64) {
        float xv = xr[j];
        if (drop) xv *= dropout_scale(seed, sid, idx0 + (uint32_t)j, p, inv_keep);
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) acc[l] = fma((double)xv, (double)Wp[(size_t)l * F + j], acc[l]);
    }
#pragma unroll
    for (int l = 0; l < LP; ++l) acc[l] = wave_sum_f64(acc[l]);
}

template <int LP, bool ONCHIP>
__device__ __forceinline__ void head_epoch(const MedpHeadProblem& pb, float* gs, float* st, double* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = pb.F, L = pb.L, w = pb.label_width, bs = pb.bs;
    const int nW = (int)head_nw(F, L, w);
    float* Wp = ONCHIP ? st : pb.W;
    float* mW = ONCHIP ? st + nW : pb.mW;
    float* vW = ONCHIP ? st + 2 * nW : pb.vW;
    if (ONCHIP)
        for (int e = tid; e < nW; e += HT_THREADS) {
            Wp[e] = pb.W[e];
            mW[e] = pb.mW[e];
            vW[e] = pb.vW[e];
        }
    for (int e = tid; e < bs * LP; e += HT_THREADS) gs[e] = 0.f;          // the label padding stays zero
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
        // ---- A: logits into gs
        if (w == 0) {
            for (int r = wave; r < bs; r += HT_WAVES) {
                double acc[LP];
                row_dots<LP>(Xc + (size_t)pr[r] * pb.ldx, Wp, F, L, lane, drop, seed, pb.stream_id, (uint32_t)r * (uint32_t)F, p, inv_keep, acc);
                double z = 0.0;
#pragma unroll
                for (int l = 0; l < LP; ++l)
                    if (lane == l) z = acc[l];
                if (lane < L) gs[r * LP + lane] = (float)(z + (double)pb.b[lane]);
            }
        } else {
            for (int e = tid; e < bs * L; e += HT_THREADS) {
                const int r = e / L, l = e % L;
                const float* xr = Xc + (size_t)pr[r] * pb.ldx;
                double acc = 0.0;
                for (int k = 0; k < w; ++k) {
                    const int j = l * w + k;
                    float xv = xr[j];
                    if (drop) xv *= dropout_scale(seed, pb.stream_id, (uint32_t)r * (uint32_t)F + (uint32_t)j, p, inv_keep);
                    acc = fma((double)xv, (double)Wp[j], acc);
                }
                gs[r * LP + l] = (float)(acc + (double)pb.b[l]);
            }
        }
        // ---- vc over the whole minibatch, then g = (sigmoid(z) - y) M / vc and the loss sum
        double part = 0.0;
        for (int e = tid; e < bs * L; e += HT_THREADS) part += (double)pb.M[(size_t)pr[e / L] * pb.ldy + e % L];
        const double vc = block_sum_wave_order_f64<HT_WAVES>(part, red);     // its barriers also publish the logits
        part = 0.0;
        for (int e = tid; e < bs * L; e += HT_THREADS) {
            const int r = e / L, l = e % L;
            const size_t o = (size_t)pr[r] * pb.ldy + l;
            part += masked_bce_term((double)gs[r * LP + l], (double)pb.Y[o], (double)pb.M[o], vc, gs + r * LP + l);
        }
        add_step_loss(run_l, run_v, block_sum_wave_order_f64<HT_WAVES>(part, red), vc);      // the sum's barriers publish g
        // ---- B: gradient of every column in row order, AdamW
        for (int j = tid; j < F; j += HT_THREADS) {
            if (w == 0) {
                double acc[LP];
#pragma unroll
                for (int l = 0; l < LP; ++l) acc[l] = 0.0;
#pragma unroll 4
                for (int r = 0; r < bs; ++r) {
                    float xv = Xc[(size_t)pr[r] * pb.ldx + j];
                    if (drop) xv *= dropout_scale(seed, pb.stream_id, (uint32_t)r * (uint32_t)F + (uint32_t)j, p, inv_keep);
#pragma unroll
                    for (int l = 0; l < LP; ++l) acc[l] = fma((double)gs[r * LP + l], (double)xv, acc[l]);
                }
#pragma unroll
                for (int l = 0; l < LP; ++l)
                    if (l < L) adamw(Wp + (size_t)l * F + j, mW + (size_t)l * F + j, vW + (size_t)l * F + j, (float)acc[l], a);
            } else {
                const int l = j / w;
                double acc = 0.0;
#pragma unroll 4
                for (int r = 0; r < bs; ++r) {
                    float xv = Xc[(size_t)pr[r] * pb.ldx + j];
                    if (drop) xv *= dropout_scale(seed, pb.stream_id, (uint32_t)r * (uint32_t)F + (uint32_t)j, p, inv_keep);
                    acc = fma((double)gs[r * LP + l], (double)xv, acc);
                }
                adamw(Wp + j, mW + j, vW + j, (float)acc, a);
            }
        }
        if (tid < L) {
            double acc = 0.0;
            for (int r = 0; r < bs; ++r) acc += (double)gs[r * LP + tid];
            adamw(pb.b + tid, pb.mb + tid, pb.vb + tid, (float)acc, a);
        }
        __syncthreads();                                                     // W, b of this step before the next step's logits
    }
    if (ONCHIP)
        for (int e = tid; e < nW; e += HT_THREADS) {
            pb.W[e] = Wp[e];
            pb.mW[e] = mW[e];
            pb.vW[e] = vW[e];
        }
    if (tid == 0) {
        pb.t[0] = t0 + pb.S;
        pb.loss_out[0] = run_l;
        pb.loss_out[1] = run_v;
    }
}

__global__ __launch_bounds__(HT_THREADS) void head_train_epoch_kernel(const MedpHeadProblem* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
    __shared__ double red[HT_WAVES];
    const MedpHeadProblem pb = tab[blockIdx.x];
    const int tid = threadIdx.x;
    // a permutation entry outside [0, N) is never dereferenced: the problem's outputs become NaN
    int bad = 0;
    for (int i = tid; i < pb.S * pb.bs; i += HT_THREADS) bad |= (unsigned)pb.perm[i] >= (unsigned)pb.N;
    if (__syncthreads_or(bad)) {
        const int nW = (int)head_nw(pb.F, pb.L, pb.label_width);
        for (int e = tid; e < nW; e += HT_THREADS) pb.W[e] = kNaNf;
        if (tid < pb.L) pb.b[tid] = kNaNf;
        if (tid == 0) pb.loss_out[0] = pb.loss_out[1] = (double)kNaNf;
        return;
    }
    float* gs = (float*)head_smem;
    const bool on = head_onchip(pb.F, pb.L, pb.label_width, pb.bs);          // uniform over the workgroup
    with_head_lp(pb.L, [&](auto lp) {
        float* st = gs + pb.bs * lp;
        if (on) head_epoch<lp, true>(pb, gs, st, red);
        else head_epoch<lp, false>(pb, gs, st, red);
    });
}

// grid (ceil(n / HS_ROWS)); wave per row
template <int LP>
__device__ __forceinline__ void head_scores_rows(const float* __restrict__ X, long long ldx, int N, int col0, int F, int L, int w,
                                                 const float* __restrict__ W, const float* __restrict__ b, const int* __restrict__ rows,
                                                 int n, float* __restrict__ logits, double* __restrict__ probs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * HS_ROWS;
    for (int i = i0 + wave; i < min(i0 + HS_ROWS, n); i += HS_WAVES) {
        const int row = rows ? rows[i] : i;
        const bool ok = (unsigned)row < (unsigned)N;
        double z = 0.0;
        if (ok) {
            const float* xr = X + (size_t)row * ldx + col0;
            if (w == 0) {
                double acc[LP];
                row_dots<LP>(xr, W, F, L, lane, false, 0u, 0u, 0u, 0.f, 1.f, acc);
#pragma unroll
                for (int l = 0; l < LP; ++l)
                    if (lane == l) z = acc[l];
            } else if (lane < L) {
                for (int k = 0; k < w; ++k) z = fma((double)xr[lane * w + k], (double)W[lane * w + k], z);
            }
        }
        if (lane < L) head_store_score(logits, probs, i, lane, L, n, ok, (float)(z + (double)b[lane]));
    }
}

__global__ __launch_bounds__(HS_THREADS) void head_scores_kernel(const float* __restrict__ X, long long ldx, int N, int col0, int F, int L,
                                                                  int w, const float* __restrict__ W, const float* __restrict__ b,
                                                                  const int* __restrict__ rows, int n, float* __restrict__ logits,
                                                                  double* __restrict__ probs) {
    with_head_lp(L, [&](auto lp) { head_scores_rows<lp>(X, ldx, N, col0, F, L, w, W, b, rows, n, logits, probs); });
}

int check_head_shape(const char* what, int p, long long ldx, int N, int ldy, int col0, int F, int L, int w) {
    MEDP_CHECK_ARG(F >= 1 && F <= MEDP_HEAD_MAX_F, "%s: problem %d has F=%d, not in [1, %d]", what, p, F, MEDP_HEAD_MAX_F);
    MEDP_TRY(check_labels_and_columns(what, p, ldx, N, col0, F, L));
    MEDP_CHECK_ARG(w >= 0 && (w == 0 || (long long)L * w == F), "%s: problem %d has label_width=%d with L=%d, F=%d (F = L label_width is needed)",
                   what, p, w, L, F);
    MEDP_CHECK_ARG(ldy < 0 || ldy >= L, "%s: problem %d has ldy=%d < L=%d", what, p, ldy, L);
    return 0;
}

}  // namespace

extern "C" int medp_head_train_onchip(int F, int L, int label_width, int bs) {
    if (F < 1 || L < 1 || L > MEDP_HEAD_MAX_L || label_width < 0 || bs < 1) return 0;
    return head_onchip(F, L, label_width, bs) ? 1 : 0;
}

extern "C" int medp_head_train_epoch(const MedpHeadProblem* table_host, const MedpHeadProblem* table_dev, int P, void* stream) {
    MEDP_CHECK_ARG(table_host, "head_train_epoch: null host table");
    MEDP_CHECK_ARG(P >= 1 && P <= 65535, "head_train_epoch: P=%d is not in [1, 65535]", P);
    long long lds = 0;
    for (int p = 0; p < P; ++p) {
        const MedpHeadProblem& q = table_host[p];
        MEDP_CHECK_ARG(q.X && q.Y && q.M && q.W && q.b && q.mW && q.vW && q.mb && q.vb && q.t && q.perm && q.loss_out,
                       "head_train_epoch: problem %d has a null pointer", p);
        MEDP_TRY(check_head_shape("head_train_epoch", p, q.ldx, q.N, q.ldy, q.col0, q.F, q.L, q.label_width));
        MEDP_TRY(check_steps("head_train_epoch", p, q.N, q.bs, q.S, q.dropout_p, q.lr, q.beta1, q.beta2, q.eps));
        long long need = head_g_bytes(q.L, q.bs);
        if (head_onchip(q.F, q.L, q.label_width, q.bs)) need += 12 * head_nw(q.F, q.L, q.label_width);
        lds = need > lds ? need : lds;
    }
    MEDP_CHECK_ARG(table_dev, "head_train_epoch: null device table");      // after the checks: the host copy alone can be validated
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)head_train_epoch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HEAD_LDS_BUDGET);
    });
    head_train_epoch_kernel<<<P, HT_THREADS, (size_t)lds, (hipStream_t)stream>>>(table_dev);
    MEDP_LAUNCH_CHECK("medp_head_train_epoch");
    return 0;
}

extern "C" int medp_head_scores(const float* X, long long ldx, int N, int col0, int F, int L, int label_width, const float* W,
                                const float* b, const int* rows, int n, float* logits, double* probs, void* stream) {
    MEDP_CHECK_ARG(X && W && b && logits && probs, "head_scores: null argument");
    MEDP_TRY(check_head_shape("head_scores", 0, ldx, N, -1, col0, F, L, label_width));
    MEDP_CHECK_ARG(n >= 1, "head_scores: n=%d < 1", n);
    head_scores_kernel<<<(n + HS_ROWS - 1) / HS_ROWS, HS_THREADS, 0, (hipStream_t)stream>>>(X, ldx, N, col0, F, L, label_width, W, b, rows, n,
                                                                                          logits, probs);
    MEDP_LAUNCH_CHECK("medp_head_scores");
    return 0;
}
