// Modality complementarity (the reference's analysis/complementarity.py; DESIGN.md "Modality complementarity"): the operating point of
// every (head, label) and the 3-way contingency counts of a split, on the logits `conditional_information_probe.gather` leaves on the device.
//
//   youden_kernel      one workgroup per (head, label): compact the known rows into LDS, sort descending, one ROC point per
//                      distinct score, and the FIRST maximum of the fp64 expression tp / P - fp / N over the points sklearn's
//                      roc_curve keeps (the (0, 0) start point at +inf, drop_intermediate's second-difference rule).  The sort,
//                      the owned ranges with their scan, the tie search and the score's image are rank_lds.h's (shared with
//                      resampled_metrics_kernel); the key layout and the argmax tree are this kernel's.
//   known_counts_kernel  known rows and known positives per label, for the length check of an N above the in-LDS sort limit.
//   cells_kernel       per label the 16 counts of (y, img > thr, ts > thr, fus > thr) over the known rows; integers only.
#include <climits>
#include <vector>

#include "rank_lds.h"

namespace {

constexpr int YD_THREADS = 1024;
constexpr unsigned long long YD_SCORE = 0xffffffff00000000ull;        // high word: the score's image; low word: label, later the positive count

struct YdScratch {
    double best_j[YD_THREADS];
    int best_i[YD_THREADS];
    int scan[2][YD_THREADS];
    int len, pos, bad, zero_row;
};

// fp32 -> u32 with the order of the finite scores; -0.0 and +0.0 share one image (one tie group)
__device__ __forceinline__ unsigned score_image(float s) { return f32_order_key(s == 0.0f ? 0.0f : s); }

__global__ __launch_bounds__(YD_THREADS) void youden_kernel(const float* __restrict__ scores, const float* __restrict__ y,
                                                             const float* __restrict__ mask, double* __restrict__ thr,
                                                             double* __restrict__ youden_j, int* __restrict__ counts, int N, int K, int M) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [M], M a power of two >= the known rows of any label
    __shared__ YdScratch sc;
    const int tid = threadIdx.x, h = blockIdx.x / K, k = blockIdx.x % K;
    if (tid == 0) {
        sc.len = sc.pos = sc.bad = 0;
        sc.zero_row = INT_MAX;
    }
    for (int j = tid; j < M; j += YD_THREADS) keys[j] = 0ull;                   // padding: below the image of every finite score
    __syncthreads();
    // compact the known rows; their order is free (the sort compares whole keys, equal keys are interchangeable)
    const float* s = scores + (size_t)h * N * K;
    for (int r = tid; r < N; r += YD_THREADS) {
        const size_t o = (size_t)r * K + k;
        if (mask[o] != 0.0f) {
            const float v = s[o];
            const bool pos = y[o] != 0.0f;
            const int at = atomicAdd(&sc.len, 1);
            if (pos) atomicAdd(&sc.pos, 1);
            if (!isfinite(v)) sc.bad = 1;
            if (v == 0.0f) atomicMin(&sc.zero_row, r);      // the zero sklearn's stable sort reports for the tie group of +-0.0
            if (at < M) keys[at] = ((unsigned long long)score_image(v) << 32) | (pos ? 1ull : 0ull);
        }
    }
    __syncthreads();
    const int L = sc.len, P = sc.pos, Nn = L - P;
    const size_t out = (size_t)h * K + k;
    if (h == 0 && tid == 0) {
        counts[2 * k] = L;
        counts[2 * k + 1] = P;
    }
    if (L < 2 || P == 0 || Nn == 0 || sc.bad || L > M) {     // no curve (`_derive_thresholds`, `_youden_threshold`), a non-finite score, or over the staged size
        if (tid == 0) thr[out] = youden_j[out] = kNaN;
        return;
    }
    lds_sort_desc<YD_THREADS, ~0ull>(keys, M, tid);  // descending by (score, label): whole keys
    // thread t owns positions [c0, c1); the low word becomes the inclusive count of positives at its position
    const auto [C, c0, c1] = owned_range<YD_THREADS>(M, L, tid);
    int cnt = 0;
    for (int j = c0; j < c1; ++j) cnt += (int)(keys[j] & 1ull);
    int run = block_inclusive_scan<YD_THREADS>(cnt, sc.scan, tid)[tid] - cnt;
    for (int j = c0; j < c1; ++j) {
        run += (int)(keys[j] & 1ull);
        keys[j] = (keys[j] & YD_SCORE) | (unsigned long long)run;
    }
    __syncthreads();
    // one ROC point per distinct score, at the END of its tie group; (0, 0) at +inf is point -1 with J = 0 and wins every tie
    double bj = 0.0;
    int bi = -1;
    const unsigned first = (unsigned)(keys[0] >> 32);
    for (int j = c0; j < c1; ++j) {
        const unsigned hj = (unsigned)(keys[j] >> 32);
        const bool last = j == L - 1;
        if (!last && (unsigned)(keys[j + 1] >> 32) == hj) continue;
        const int tp = (int)(unsigned)keys[j], fp = j + 1 - tp;
        if (!last && hj != first) {                          // drop_intermediate: an interior point on a straight stretch of both counts
            const unsigned below_next = (unsigned)(keys[j + 1] >> 32) - 1u;
            const int pe = first_at_most(keys, YD_SCORE, (unsigned long long)hj << 32, 0, j) - 1;                 // end of the previous group
            const int ne = first_at_most(keys, YD_SCORE, (unsigned long long)below_next << 32, j + 1, L) - 1;     // end of the next group
            const int tp_p = (int)(unsigned)keys[pe], fp_p = pe + 1 - tp_p;
            const int tp_n = (int)(unsigned)keys[ne], fp_n = ne + 1 - tp_n;
            if (tp_p - 2 * tp + tp_n == 0 && fp_p - 2 * fp + fp_n == 0) continue;
        }
        const double J = (double)tp / (double)P - (double)fp / (double)Nn;
        if (J > bj) {                                        // ascending j: the first maximum of this range stays
            bj = J;
            bi = j;
        }
    }
    // fixed-tree argmax: the larger J, on equal J the lower index
    sc.best_j[tid] = bj;
    sc.best_i[tid] = bi;
    __syncthreads();
    for (int st = YD_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const double ja = sc.best_j[tid], jb = sc.best_j[tid + st];
            const int ia = sc.best_i[tid], ib = sc.best_i[tid + st];
            if (jb > ja || (jb == ja && ib < ia)) {
                sc.best_j[tid] = jb;
                sc.best_i[tid] = ib;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int best = sc.best_i[0];
        double t = best < 0 ? kInf : (double)f32_from_order_key((unsigned)(keys[best] >> 32));
        if (t == 0.0) t = (double)s[(size_t)sc.zero_row * K + k];      // its sign: that of the first known row holding a zero
        thr[out] = t;
        youden_j[out] = best < 0 ? 0.0 : sc.best_j[0];
    }
}

__global__ __launch_bounds__(YD_THREADS) void known_counts_kernel(const float* __restrict__ y, const float* __restrict__ mask,
                                                                   int* __restrict__ counts, int N, int K) {
    __shared__ int tot[2];
    const int tid = threadIdx.x, k = blockIdx.x;
    if (tid < 2) tot[tid] = 0;
    __syncthreads();
    int len = 0, pos = 0;
    for (int r = tid; r < N; r += YD_THREADS) {
        const size_t o = (size_t)r * K + k;
        if (mask[o] != 0.0f) {
            ++len;
            pos += y[o] != 0.0f;
        }
    }
    atomicAdd(&tot[0], len);
    atomicAdd(&tot[1], pos);
    __syncthreads();
    if (tid < 2) counts[2 * k + tid] = tot[tid];
}

constexpr int CELL_THREADS = 256, CELL_ROWS = 4096;            // rows of one label per workgroup

__global__ __launch_bounds__(CELL_THREADS) void cells_kernel(const float* __restrict__ scores, const float* __restrict__ y,
                                                              const float* __restrict__ mask, const double* __restrict__ thr,
                                                              int* __restrict__ cells, int N, int K) {
    __shared__ int hist[16];
    const int tid = threadIdx.x, k = blockIdx.x % K;
    const long long r0 = (long long)(blockIdx.x / K) * CELL_ROWS;
    const int r1 = (int)min(r0 + (long long)CELL_ROWS, (long long)N);
    if (tid < 16) hist[tid] = 0;
    __syncthreads();
    const double t_img = thr[k], t_ts = thr[K + k], t_fus = thr[2 * K + k];
    const size_t head = (size_t)N * K;
    for (int r = (int)r0 + tid; r < r1; r += CELL_THREADS) {
        const size_t o = (size_t)r * K + k;
        if (mask[o] != 0.0f) {
            const int c = (y[o] != 0.0f ? 1 : 0) | ((double)scores[o] > t_img ? 2 : 0) | ((double)scores[head + o] > t_ts ? 4 : 0) |
                          ((double)scores[2 * head + o] > t_fus ? 8 : 0);
            atomicAdd(&hist[c], 1);
        }
    }
    __syncthreads();
    if (tid < 16 && hist[tid] != 0) atomicAdd(&cells[(size_t)k * 16 + tid], hist[tid]);
}

}  // namespace

extern "C" int medp_youden_thresholds(const float* scores, const float* y, const float* mask, double* thr, double* youden_j, int* counts,
                                      int H, int N, int K, void* stream) {
    MEDP_CHECK_ARG(scores && y && mask && thr && youden_j && counts, "youden_thresholds: null argument");
    MEDP_CHECK_ARG(H >= 1 && N >= 1 && K >= 1, "youden_thresholds: bad shape H=%d N=%d K=%d", H, N, K);
    MEDP_CHECK_ARG((long long)H * K <= INT_MAX, "youden_thresholds: H K = %lld workgroups", (long long)H * K);
    hipStream_t st = (hipStream_t)stream;
    int max_len = N;
    if (N > MEDP_YOUDEN_MAX_LEN) {          // only the known rows are sorted: count them before refusing
        known_counts_kernel<<<K, YD_THREADS, 0, st>>>(y, mask, counts, N, K);
        MEDP_LAUNCH_CHECK("medp_youden_thresholds (counts)");
        std::vector<int> host((size_t)K * 2);
        hipError_t e = hipMemcpyAsync(host.data(), counts, host.size() * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            medp_set_error("youden_thresholds: reading the counts back failed: %s", hipGetErrorString(e));
            return (int)e;
        }
        max_len = 0;
        for (int k = 0; k < K; ++k) max_len = host[2 * k] > max_len ? host[2 * k] : max_len;
    }
    MEDP_CHECK_ARG(max_len <= MEDP_YOUDEN_MAX_LEN, "youden_thresholds: %d known rows of one label exceed the in-LDS sort limit %d", max_len,
                   MEDP_YOUDEN_MAX_LEN);
    const int M = lds_sort_staged_len<youden_kernel>(max_len);
    youden_kernel<<<H * K, YD_THREADS, (size_t)M * 8, st>>>(scores, y, mask, thr, youden_j, counts, N, K, M);
    MEDP_LAUNCH_CHECK("medp_youden_thresholds");
    return 0;
}

extern "C" int medp_complementarity_cells(const float* scores, const float* y, const float* mask, const double* thr, int* cells, int N,
                                          int K, void* stream) {
    MEDP_CHECK_ARG(scores && y && mask && thr && cells, "complementarity_cells: null argument");
    MEDP_CHECK_ARG(N >= 1 && K >= 1, "complementarity_cells: bad shape N=%d K=%d", N, K);
    const long long blocks = (long long)((N + CELL_ROWS - 1) / CELL_ROWS) * K;
    MEDP_CHECK_ARG(blocks <= INT_MAX, "complementarity_cells: %lld workgroups", blocks);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(cells, 0, (size_t)K * 16 * sizeof(int), st);
    if (e != hipSuccess) {
        medp_set_error("complementarity_cells: clearing the counts failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    cells_kernel<<<(unsigned)blocks, CELL_THREADS, 0, st>>>(scores, y, mask, thr, cells, N, K);
    MEDP_LAUNCH_CHECK("medp_complementarity_cells");
    return 0;
}
