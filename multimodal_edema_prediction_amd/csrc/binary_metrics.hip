// BCE / AUROC / AUPRC of resampled replicates (the reference's `_safe_metrics` over bootstrap, permutation or per-label index
// lists; DESIGN.md "Raw-trajectory probe", "Conditional-information probe", "Linear-head probes"): the one metrics kernel of all the
// analysis probes (probe_stats.py).  fp64 throughout.
//
//   resampled_metrics_kernel    one resampled replicate per workgroup: gather, clip, sort in LDS, then tie-aware (one threshold
//                               per distinct score) ROC area and average precision.  The sort, the owned ranges with their scan,
//                               the tie search and the fixed-tree sum are rank_lds.h's; the key layout is this kernel's.
#include "rank_lds.h"

namespace {

constexpr int RM_THREADS = 1024;
constexpr unsigned long long RM_LABEL = 1ull << 63, RM_SCORE = ~RM_LABEL;     // the clipped score is positive: its sign bit carries the label

struct RmScratch {
    double red[RM_THREADS];
    int scan[2][RM_THREADS];
    int total_pos;
    int bad;
};

__global__ __launch_bounds__(RM_THREADS) void resampled_metrics_kernel(const unsigned char* __restrict__ y, const double* __restrict__ p,
                                                                        const int* __restrict__ idx, const long long* __restrict__ offsets,
                                                                        double* __restrict__ out, int N, int Rp, int M) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [M], M a power of two >= the replicate's length
    __shared__ RmScratch sc;
    const int tid = threadIdx.x, r = blockIdx.x;
    const long long o0 = idx ? offsets[r] : 0;
    const long long len = idx ? offsets[r + 1] - o0 : N;
    double* o = out + (size_t)r * 3;
    if (len <= 0 || len > M) {              // empty replicate: NaN by definition; over the staged size: refuse (never index past LDS)
        if (tid < 3) o[tid] = kNaN;
        return;
    }
    const int L = (int)len;
    if (tid == 0) sc.bad = 0;
    __syncthreads();
    const double* pr = p + (Rp == 1 ? 0 : (size_t)r * N);
    double bce = 0.0;
    for (int j = tid; j < M; j += RM_THREADS) {
        unsigned long long key = 0ull;       // padding: below every clipped score
        if (j < L) {
            const int src = idx ? idx[o0 + j] : j;
            if (src < 0 || src >= N) {
                sc.bad = 1;
            } else {
                const double q = fmin(fmax(pr[src], 1e-7), 1.0 - 1e-7);
                const bool pos = y[src] != 0;
                bce -= pos ? log(q) : log(1.0 - q);
                key = (unsigned long long)__double_as_longlong(q) | (pos ? RM_LABEL : 0ull);
            }
        }
        keys[j] = key;
    }
    bce = block_sum_tree_f64<RM_THREADS>(bce, sc.red, tid) / (double)L;
    if (sc.bad) {                            // an index outside [0, N): no metric is defined
        if (tid < 3) o[tid] = kNaN;
        return;
    }
    lds_sort_desc<RM_THREADS, RM_SCORE>(keys, M, tid);            // descending by score: the label bit takes no part
    // thread t owns positions [c0, c1); positives before c0 by an inclusive scan of the per-thread counts
    const auto [C, c0, c1] = owned_range<RM_THREADS>(M, L, tid);
    int cnt = 0;
    for (int j = c0; j < c1; ++j) cnt += (int)(keys[j] >> 63);
    const int* incl = block_inclusive_scan<RM_THREADS>(cnt, sc.scan, tid);
    const int tp0 = incl[tid] - cnt;                                     // positives in [0, c0)
    const int P = incl[RM_THREADS - 1], Nn = L - P;
    // positives before the tie group that is open at c0 (its first element may lie in an earlier thread's range)
    int tp_prev = tp0, fp_prev = c0 - tp0;
    if (c0 < c1 && c0 > 0 && ((keys[c0 - 1] ^ keys[c0]) & RM_SCORE) == 0) {
        const int lo = first_at_most(keys, RM_SCORE, keys[c0] & RM_SCORE, 0, c0);
        const int owner = lo / C;
        int tp = owner > 0 ? incl[owner - 1] : 0;
        for (int j = owner * C; j < lo; ++j) tp += (int)(keys[j] >> 63);
        tp_prev = tp;
        fp_prev = lo - tp;
    }
    // one threshold per distinct score: the group that ENDS at j contributes a trapezoid to the ROC area and a step to AP
    long long area2 = 0;                                                 // twice the ROC area in (FP, TP) counts: exact
    double ap = 0.0;
    int tp = tp0;
    for (int j = c0; j < c1; ++j) {
        tp += (int)(keys[j] >> 63);
        if (j == L - 1 || ((keys[j] ^ keys[j + 1]) & RM_SCORE) != 0) {
            const int fp = j + 1 - tp;
            area2 += (long long)(fp - fp_prev) * (long long)(tp + tp_prev);
            ap += ((double)(tp - tp_prev) / (double)P) * ((double)tp / (double)(j + 1));
            tp_prev = tp;
            fp_prev = fp;
        }
    }
    const double area = block_sum_tree_f64<RM_THREADS>((double)area2, sc.red, tid);      // integers below 2^53: exact in any order
    ap = block_sum_tree_f64<RM_THREADS>(ap, sc.red, tid);
    if (tid == 0) {
        const bool both = P > 0 && Nn > 0;
        o[0] = bce;
        o[1] = both ? area / (2.0 * (double)P * (double)Nn) : kNaN;
        o[2] = both ? ap : kNaN;
    }
}

}  // namespace

extern "C" int medp_resampled_binary_metrics(const unsigned char* y, const double* p, const int* idx, const long long* offsets,
                                             double* out, int N, int Rp, int R, int max_len, void* stream) {
    MEDP_CHECK_ARG(y && p && out, "resampled_binary_metrics: null argument");
    MEDP_CHECK_ARG(N >= 1 && R >= 1, "resampled_binary_metrics: bad shape N=%d R=%d", N, R);
    MEDP_CHECK_ARG(Rp == 1 || Rp == R, "resampled_binary_metrics: Rp=%d is neither 1 nor R=%d", Rp, R);
    MEDP_CHECK_ARG(idx == nullptr || offsets != nullptr, "resampled_binary_metrics: a gather needs its offsets");
    if (idx == nullptr) max_len = N;
    MEDP_CHECK_ARG(max_len >= 0, "resampled_binary_metrics: max_len %d < 0", max_len);
    MEDP_CHECK_ARG(max_len <= MEDP_RESAMPLED_METRICS_MAX_LEN, "resampled_binary_metrics: replicate length %d exceeds the in-LDS sort limit %d",
                   max_len, MEDP_RESAMPLED_METRICS_MAX_LEN);
    const int M = lds_sort_staged_len<resampled_metrics_kernel>(max_len);
    resampled_metrics_kernel<<<R, RM_THREADS, (size_t)M * 8, (hipStream_t)stream>>>(y, p, idx, offsets, out, N, Rp, M);
    MEDP_LAUNCH_CHECK("medp_resampled_binary_metrics");
    return 0;
}
