// Raw-trajectory conditional probe (reference analysis/raw_trajectory_conditional_probe.py; DESIGN.md "Raw-trajectory probe"):
// the two data-parallel fp64 parts of the reference's default path that are this probe's own (the metrics of its replicates come
// from binary_metrics.hip).  Everything here is fp64, as in the reference; there is no bf16 mode and functional.precision() is not
// consulted.
//
//   raw_summary_kernel          one thread per (window, variable): the 14 statistics of _summarize_one_variable (:329-405) from the
//                               [B,T,2V] values | counts tensor, with the reference's centred two-pass std and slopes.
//   valgrad_tile_kernel<G> +    objective and gradient of _fit_offset_weights (:578-584) for G candidate weight columns at once.
//   valgrad_finish_kernel       A workgroup streams its row block of X from HBM ONCE: the rows go to LDS while the same
//                               registers feed X.W; after the residuals expit(s) - y are known the X^T.R half reads the rows
//                               back from LDS.  The per-workgroup partial gradients / losses are summed by the finish kernel in
//                               a fixed order (two-stage, no floating-point atomics: bit-stable).
#include "common.h"
#include "medp_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// (a) per-(window, variable) summaries
// ---------------------------------------------------------------------------------------------------------------------
struct WSum {            // count-weighted sums of one set of valid points
    double w = 0.0, wv = 0.0, wt = 0.0;
    int n = 0;
};

__global__ void raw_summary_kernel(const float* __restrict__ x, double* __restrict__ out, int B, int T, int V, int recent_hours) {
#pragma clang fp contract(off)          // the reference's arithmetic, operation by operation (no fused multiply-add)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * V) return;
    const int b = i / V, v = i % V;
    const float* base = x + (size_t)b * T * 2 * V;
    const int recent_start = T - recent_hours;          // 1 <= recent_hours <= T (checked by the launcher)

    // pass 1: order statistics, counts and the weighted sums the means need
    WSum all, rec, ear;
    double first = kNaN, last = kNaN, mn = kNaN, mx = kNaN;
    int n_obs = 0, n_obs_rec = 0, last_obs = -1;
    double cnt_all = 0.0, cnt_rec = 0.0;
    for (int t = 0; t < T; ++t) {
        const float* row = base + (size_t)t * 2 * V;
        const double val = (double)row[v], cnt = (double)row[V + v];
        const bool observed = isfinite(cnt) && cnt > 0.0;
        if (!observed) continue;
        ++n_obs;
        cnt_all += cnt;
        last_obs = t;
        if (t >= recent_start) {
            ++n_obs_rec;
            cnt_rec += cnt;
        }
        if (!isfinite(val)) continue;
        if (all.n == 0) {
            first = val;
            mn = val;
            mx = val;
        } else {
            mn = val < mn ? val : mn;
            mx = val > mx ? val : mx;
        }
        last = val;
        WSum& part = t >= recent_start ? rec : ear;
        all.w += cnt;   all.wv += cnt * val;   all.wt += cnt * (double)t;   ++all.n;
        part.w += cnt;  part.wv += cnt * val;  part.wt += cnt * (double)t;  ++part.n;
    }
    const double mean = all.n ? all.wv / all.w : kNaN;
    const double tmean = all.n ? all.wt / all.w : kNaN;
    const double rmean = rec.n ? rec.wv / rec.w : kNaN;
    const double rtmean = rec.n ? rec.wt / rec.w : kNaN;

    // pass 2: centred second moments
    double var = 0.0, den = 0.0, num = 0.0, rden = 0.0, rnum = 0.0;
    if (all.n) {
        for (int t = 0; t < T; ++t) {
            const float* row = base + (size_t)t * 2 * V;
            const double val = (double)row[v], cnt = (double)row[V + v];
            if (!(isfinite(cnt) && cnt > 0.0 && isfinite(val))) continue;
            const double dv = val - mean, dt = (double)t - tmean;
            var += cnt * (dv * dv);
            den += cnt * (dt * dt);
            num += cnt * dt * dv;
            if (t >= recent_start) {
                const double rdt = (double)t - rtmean;
                rden += cnt * (rdt * rdt);
                rnum += cnt * rdt * (val - rmean);
            }
        }
    }
    double* o = out + (size_t)i * 14;
    o[0] = last;
    o[1] = mean;
    o[2] = all.n ? sqrt(fmax(var / all.w, 0.0)) : kNaN;
    o[3] = mn;
    o[4] = mx;
    o[5] = all.n >= 2 ? last - first : kNaN;
    o[6] = (all.n >= 2 && den > 0.0) ? num / den : kNaN;
    o[7] = (rec.n >= 2 && rden > 0.0) ? rnum / rden : kNaN;
    o[8] = (rec.n && ear.n) ? rmean - ear.wv / ear.w : kNaN;
    o[9] = (double)n_obs / (double)T;
    o[10] = log1p(fmax(cnt_all, 0.0));
    o[11] = n_obs ? fmax((double)((T - 1) - last_obs), 0.0) : (double)T;
    o[12] = (double)n_obs_rec / (double)(T - recent_start > 1 ? T - recent_start : 1);
    o[13] = log1p(fmax(cnt_rec, 0.0));
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) offset-logistic objective + gradient for G candidates
// ---------------------------------------------------------------------------------------------------------------------
constexpr int VG_THREADS = 512;                   // 8 waves: two per SIMD
constexpr int VG_WAVES = VG_THREADS / 64;
constexpr int VG_MAX_ROWS = 32;                   // rows of X per workgroup
constexpr int VG_LDS_X = 144 * 1024;              // LDS bytes for the row block (of the CU's 160 KiB; the rest holds R and the wave partials)

// rows per workgroup: as many as fit the LDS budget, at most VG_MAX_ROWS; 0: not even one row fits, the X^T.R half re-reads
// the row from global memory (it was just read by the same CU: an L2 hit, not a second HBM pass)
inline int vg_rows(int F) {
    const long long fit = (long long)VG_LDS_X / ((long long)F * 8);
    return (int)(fit > VG_MAX_ROWS ? VG_MAX_ROWS : fit);
}

template <int G>
__global__ __launch_bounds__(VG_THREADS) void valgrad_tile_kernel(const double* __restrict__ X, long long ldx, const double* __restrict__ y,
                                                                  const double* __restrict__ offset, const double* __restrict__ W,
                                                                  double* __restrict__ gpart, double* __restrict__ lpart, int n, int F,
                                                                  int rows, int staged) {
    extern __shared__ __attribute__((aligned(16))) double xs[];          // [rows][F] when staged
    __shared__ double rs[VG_MAX_ROWS][8];                                 // residuals expit(s) - y
    __shared__ double lw[VG_WAVES][8];                                    // per-wave loss sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * rows;
    const int rb = min(rows, n - r0);
    double loss = 0.0;                                                   // lane g < G of each wave: that wave's rows, in row order
    for (int r = wave; r < rb; r += VG_WAVES) {
        const double* xr = X + (size_t)(r0 + r) * ldx;
        double acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.0;
        for (int f = lane; f < F; f += 64) {
            const double xv = xr[f];
            if (staged) xs[(size_t)r * F + f] = xv;
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = fma(xv, W[(size_t)f * G + g], acc[g]);
        }
        double mine = 0.0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double s = wave_sum_f64(acc[g]);
            if (lane == g) mine = s;
        }
        if (lane < G) {
            const double s = offset[r0 + r] + mine, yy = y[r0 + r];
            const double e = exp(-fabs(s));                              // stable logaddexp(0, s) and expit(s)
            loss += fmax(s, 0.0) + log1p(e) - yy * s;
            rs[r][lane] = (s >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - yy;
        }
    }
    if (lane < G) lw[wave][lane] = loss;
    __syncthreads();
    if (tid < G) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < VG_WAVES; ++w) s += lw[w][tid];
        lpart[(size_t)blockIdx.x * G + tid] = s;
    }
    // X^T.R over this block's rows: thread per feature, rows in order
    for (int f = tid; f < F; f += VG_THREADS) {
        double acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.0;
        for (int r = 0; r < rb; ++r) {
            const double xv = staged ? xs[(size_t)r * F + f] : X[(size_t)(r0 + r) * ldx + f];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = fma(xv, rs[r][g], acc[g]);
        }
        double* gp = gpart + ((size_t)blockIdx.x * F + f) * G;
#pragma unroll
        for (int g = 0; g < G; ++g) gp[g] = acc[g];
    }
}

// stage two: sums in a fixed order.  Workgroups [0, gblocks) own FIN_ELEMS gradient elements each: FIN_SLICES threads per element add
// every FIN_SLICES-th partial (block order within a slice), then one thread adds the slices in order; the last workgroup owns the G
// objectives.  Spreading an element's partials over FIN_SLICES threads keeps the whole chip busy: F*G alone is a few thousand elements.
constexpr int FIN_ELEMS = 16, FIN_SLICES = 16;          // 16 consecutive doubles: one 128-B segment per slice and load

__global__ __launch_bounds__(256) void valgrad_finish_kernel(const double* __restrict__ gpart, const double* __restrict__ lpart,
                                                             const double* __restrict__ W, const double* __restrict__ l2,
                                                             double* __restrict__ obj, double* __restrict__ grad, int n, int F, int G,
                                                             int nblocks, int gblocks) {
    __shared__ double red[FIN_SLICES][FIN_ELEMS];
    const int tid = threadIdx.x;
    const double inv_n = 1.0 / (double)n;
    if ((int)blockIdx.x < gblocks) {
        const int el = tid % FIN_ELEMS, slice = tid / FIN_ELEMS;
        const size_t e = (size_t)blockIdx.x * FIN_ELEMS + el, FG = (size_t)F * G;
        double s = 0.0;
        if (e < FG)
            for (int b = slice; b < nblocks; b += FIN_SLICES) s += gpart[(size_t)b * FG + e];
        red[slice][el] = s;
        __syncthreads();
        if (tid < FIN_ELEMS && e < FG) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < FIN_SLICES; ++k) t += red[k][tid];
            grad[e] = t * inv_n + l2[e % G] * W[e];
        }
        return;
    }
    const int lane = tid & 63, wave = tid >> 6;                          // 4 waves, candidates wave, wave + 4
    for (int g = wave; g < G; g += 4) {
        double ls = 0.0, ww = 0.0;
        for (int b = lane; b < nblocks; b += 64) ls += lpart[(size_t)b * G + g];
        for (int f = lane; f < F; f += 64) {
            const double w = W[(size_t)f * G + g];
            ww = fma(w, w, ww);
        }
        ls = wave_sum_f64(ls);
        ww = wave_sum_f64(ww);
        if (lane == 0) obj[g] = ls * inv_n + 0.5 * l2[g] * ww;
    }
}

template <int G>
int launch_valgrad_tile(const double* X, long long ldx, const double* y, const double* offset, const double* W, double* gpart,
                        double* lpart, int n, int F, hipStream_t st) {
    MEDP_ONCE_PER_DEVICE({ hipFuncSetAttribute((const void*)valgrad_tile_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, VG_LDS_X); });
    const int fit = vg_rows(F), rows = fit > 0 ? fit : 1, staged = fit > 0;
    const int nblocks = (n + rows - 1) / rows;
    const size_t lds = staged ? (size_t)rows * F * 8 : 0;
    valgrad_tile_kernel<G><<<nblocks, VG_THREADS, lds, st>>>(X, ldx, y, offset, W, gpart, lpart, n, F, rows, staged);
    MEDP_LAUNCH_CHECK("medp_offset_logistic_valgrad");
    return 0;
}

}  // namespace

extern "C" int medp_raw_traj_summary(const float* x, double* out, int B, int T, int V, int recent_hours, void* stream) {
    MEDP_CHECK_ARG(x && out, "raw_traj_summary: null argument");
    MEDP_CHECK_ARG(B > 0 && T > 0 && V > 0, "raw_traj_summary: bad shape B=%d T=%d V=%d", B, T, V);
    MEDP_CHECK_ARG((long long)B * V <= 0x7fffffffLL, "raw_traj_summary: B*V = %lld overflows int", (long long)B * V);
    MEDP_CHECK_ARG(recent_hours >= 1 && recent_hours <= T, "raw_traj_summary: recent_hours %d is not in [1, %d]", recent_hours, T);
    const int n = B * V;
    raw_summary_kernel<<<(n + 127) / 128, 128, 0, (hipStream_t)stream>>>(x, out, B, T, V, recent_hours);
    MEDP_LAUNCH_CHECK("medp_raw_traj_summary");
    return 0;
}

extern "C" size_t medp_offset_logistic_ws_bytes(int n, int F, int G) {
    if (n < 1 || F < 1 || G < 1 || G > MEDP_OFFSET_LOGISTIC_MAX_G) return 0;
    const int fit = vg_rows(F), rows = fit > 0 ? fit : 1;
    const size_t nblocks = ((size_t)n + rows - 1) / rows;
    return nblocks * ((size_t)F * G + G) * sizeof(double);
}

extern "C" int medp_offset_logistic_valgrad(const double* X, long long ldx, const double* y, const double* offset, const double* W,
                                            const double* l2, double* obj, double* grad, void* ws, size_t ws_bytes, int n, int F, int G,
                                            void* stream) {
    MEDP_CHECK_ARG(X && y && offset && W && l2 && obj && grad && ws, "offset_logistic_valgrad: null argument");
    MEDP_CHECK_ARG(n >= 1 && F >= 1, "offset_logistic_valgrad: bad shape n=%d F=%d", n, F);
    MEDP_CHECK_ARG(G >= 1 && G <= MEDP_OFFSET_LOGISTIC_MAX_G, "offset_logistic_valgrad: G=%d is not in [1, %d]", G, MEDP_OFFSET_LOGISTIC_MAX_G);
    MEDP_CHECK_ARG(ldx >= F, "offset_logistic_valgrad: leading dimension %lld < F=%d", ldx, F);
    MEDP_CHECK_ARG((long long)F * G <= 0x7fffffffLL, "offset_logistic_valgrad: F*G overflows int");
    MEDP_CHECK_ARG(ws_bytes >= medp_offset_logistic_ws_bytes(n, F, G), "offset_logistic_valgrad: workspace %zu < %zu bytes", ws_bytes,
                   medp_offset_logistic_ws_bytes(n, F, G));
    const int fit = vg_rows(F), rows = fit > 0 ? fit : 1;
    const int nblocks = (n + rows - 1) / rows;
    double* gpart = (double*)ws;
    double* lpart = gpart + (size_t)nblocks * F * G;
    hipStream_t st = (hipStream_t)stream;
    switch (G) {
        case 1: MEDP_TRY(launch_valgrad_tile<1>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 2: MEDP_TRY(launch_valgrad_tile<2>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 3: MEDP_TRY(launch_valgrad_tile<3>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 4: MEDP_TRY(launch_valgrad_tile<4>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 5: MEDP_TRY(launch_valgrad_tile<5>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 6: MEDP_TRY(launch_valgrad_tile<6>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        case 7: MEDP_TRY(launch_valgrad_tile<7>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
        default: MEDP_TRY(launch_valgrad_tile<8>(X, ldx, y, offset, W, gpart, lpart, n, F, st)); break;
    }
    const int gblocks = (int)(((size_t)F * G + FIN_ELEMS - 1) / FIN_ELEMS);
    valgrad_finish_kernel<<<gblocks + 1, 256, 0, st>>>(gpart, lpart, W, l2, obj, grad, n, F, G, nblocks, gblocks);
    MEDP_LAUNCH_CHECK("medp_offset_logistic_valgrad (finish)");
    return 0;
}
