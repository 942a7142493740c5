// Trajectory-availability audit (the reference's analysis/trajectory_availability.py; DESIGN.md "Trajectory availability"): do the
// pre-CXR windows hold per-variable trajectories at all?  A data audit, no model.
//
//   traj_cells_kernel      one workgroup per tile of 32 samples x 32 variables, one thread per (sample, variable): x is read once, lanes
//                          along v; observed hours, count total, recency, fp64 two-pass std and endpoint change of that cell column.  The
//                          tile goes through LDS, so every plane store is a 128-byte run along n, and the per-sample / per-variable counts
//                          are shuffle sums of the tile followed by ONE integer atomic per (row, figure) and workgroup.
//   column_median_kernel   one workgroup per column: exact selection by radix (four 8-bit passes over order-preserving keys, histograms in
//                          LDS with integer atomics), then the smallest key above the lower median where the upper one is not its equal.
//                          No sort, nothing of the column is staged: any length up to MEDP_COLUMN_MEDIAN_MAX_N.  The fp32 key and its
//                          inverse are rank_lds.h's (the Youden kernel's score image); NaN rejection, |.| and the int32 keys are here.
#include <climits>

#include "rank_lds.h"

namespace {

constexpr float kNaNf = __builtin_nanf("");

// ---------------------------------------------------------------------------------------------------------------------------------
// cells
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int TC_TILE = 32, TC_THREADS = TC_TILE * TC_TILE, TC_PAD = TC_TILE + 1, TC_UNROLL = 8;

struct TcTile {
    int hours[TC_TILE][TC_PAD];          // [variable][sample]
    float total[TC_TILE][TC_PAD], recency[TC_TILE][TC_PAD], within_std[TC_TILE][TC_PAD], endpoint[TC_TILE][TC_PAD];
};

// sum over the 32 lanes that share threadIdx.x / 32 (a half wave): a fixed butterfly, every lane ends with the total
__device__ __forceinline__ int half_wave_sum(int v) {
#pragma unroll
    for (int o = TC_TILE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TC_THREADS) void traj_cells_kernel(const float* __restrict__ x, int n, int T, int V, int n_timesteps, int n0,
                                                                 long long ld, int* __restrict__ obs_hours, float* __restrict__ total,
                                                                 float* __restrict__ recency, float* __restrict__ within_std,
                                                                 float* __restrict__ endpoint_change, int* __restrict__ per_sample,
                                                                 unsigned long long* __restrict__ var_counts) {
    __shared__ TcTile tile;
    const int row = threadIdx.x / TC_TILE, col = threadIdx.x % TC_TILE;
    const long long s0 = (long long)blockIdx.x * TC_TILE;
    const int v0 = blockIdx.y * TC_TILE;
    {   // thread = (sample s0 + row, variable v0 + col): lanes run along v
        const long long s = s0 + row;
        const int v = v0 + col;
        int k = 0, first_t = 0, last_t = 0;
        float tot = 0.0f, first_v = 0.0f, last_v = 0.0f;
        double sum = 0.0;
        const bool live = s < n && v < V;
        const float* xs = x + (size_t)(live ? s : 0) * T * 2 * V + (live ? v : 0);
        if (live) {
            // TC_UNROLL hours per trip: their 2 TC_UNROLL loads are issued before the first is used (a thread alone has nothing
            // else in flight, and the launch is bound by memory latency otherwise); the hours are then taken in t order
            for (int t0 = 0; t0 < T; t0 += TC_UNROLL) {
                float c[TC_UNROLL], val[TC_UNROLL];
#pragma unroll
                for (int u = 0; u < TC_UNROLL; ++u) {
                    const bool in = t0 + u < T;
                    const float* cell = xs + (size_t)(in ? t0 + u : t0) * 2 * V;
                    c[u] = cell[V];
                    val[u] = cell[0];
                }
#pragma unroll
                for (int u = 0; u < TC_UNROLL; ++u) {
                    const int t = t0 + u;
                    if (t >= T) break;
                    tot += c[u];
                    if (c[u] > 0.0f) {                   // the value of an unobserved cell enters nothing
                        if (k == 0) {
                            first_v = val[u];
                            first_t = t;
                        }
                        last_v = val[u];
                        last_t = t;
                        sum += (double)val[u];
                        ++k;
                    }
                }
            }
        }
        float sd = kNaNf, ep = kNaNf;
        if (k >= 2) {                                    // second pass, over [first_t, last_t] only: served by the cache
            const double mean = sum / (double)k;
            double ss = 0.0;
            for (int t0 = first_t; t0 <= last_t; t0 += TC_UNROLL) {
                float c[TC_UNROLL], val[TC_UNROLL];
#pragma unroll
                for (int u = 0; u < TC_UNROLL; ++u) {
                    const bool in = t0 + u <= last_t;
                    const float* cell = xs + (size_t)(in ? t0 + u : t0) * 2 * V;
                    c[u] = cell[V];
                    val[u] = cell[0];
                }
#pragma unroll
                for (int u = 0; u < TC_UNROLL; ++u)
                    if (t0 + u <= last_t && c[u] > 0.0f) {
                        const double d = (double)val[u] - mean;
                        ss += d * d;
                    }
            }
            sd = (float)sqrt(ss / (double)k);            // fp64 throughout, ONE rounding to fp32
            ep = last_v - first_v;
        }
        tile.hours[col][row] = k;
        tile.total[col][row] = tot;
        tile.recency[col][row] = k >= 1 ? (float)(n_timesteps - last_t) : kNaNf;
        tile.within_std[col][row] = sd;
        tile.endpoint[col][row] = ep;
        // per sample: over the 32 variables of this tile (dead lanes hold k = 0)
        const int c1 = half_wave_sum(k >= 1), c2 = half_wave_sum(k >= 2), c3 = half_wave_sum(k >= 3), ch = half_wave_sum(k);
        if (col == 0 && s < n) {
            int* ps = per_sample + ((size_t)n0 + (size_t)s) * 4;
            if (c1) atomicAdd(ps + 0, c1);
            if (c2) atomicAdd(ps + 1, c2);
            if (c3) atomicAdd(ps + 2, c3);
            if (ch) atomicAdd(ps + 3, ch);
        }
    }
    __syncthreads();
    {   // thread = (variable v0 + row, sample s0 + col): lanes run along n
        const int v = v0 + row;
        const long long s = s0 + col;
        const bool live = s < n && v < V;
        const int k = live ? tile.hours[row][col] : 0;
        if (live) {
            const size_t o = (size_t)v * (size_t)ld + (size_t)n0 + (size_t)s;
            obs_hours[o] = k;
            total[o] = tile.total[row][col];
            recency[o] = tile.recency[row][col];
            within_std[o] = tile.within_std[row][col];
            endpoint_change[o] = tile.endpoint[row][col];
        }
        const int c1 = half_wave_sum(k >= 1), c2 = half_wave_sum(k >= 2), c3 = half_wave_sum(k >= 3), ch = half_wave_sum(k);
        if (col == 0 && v < V) {
            unsigned long long* vc = var_counts + (size_t)v * 4;
            if (c1) atomicAdd(vc + 0, (unsigned long long)c1);
            if (c2) atomicAdd(vc + 1, (unsigned long long)c2);
            if (c3) atomicAdd(vc + 2, (unsigned long long)c3);
            if (ch) atomicAdd(vc + 3, (unsigned long long)ch);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// medians
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int CM_THREADS = 1024, CM_WAVES = CM_THREADS / MEDP_WAVE, CM_BINS = 256;

struct CmScratch {
    unsigned hist[CM_WAVES][CM_BINS];    // one histogram per wave: lanes of different waves never meet on an address
    unsigned merged[CM_BINS];
    unsigned prefix, rank, below, equal, next_key;
};

// element i of a column -> its key, unsigned and in the order of the values; false: a NaN, which the median drops
template <bool IS_INT, bool TAKE_ABS>
__device__ __forceinline__ bool column_key(const void* column, size_t i, unsigned& key) {
    if (IS_INT) {
        unsigned b = (unsigned)((const int*)column)[i];
        if (TAKE_ABS && (b & 0x80000000u)) b = 0u - b;
        key = b ^ 0x80000000u;
        return true;
    }
    float v = ((const float*)column)[i];
    if (v != v) return false;
    if (TAKE_ABS) v = fabsf(v);
    key = f32_order_key(v);
    return true;
}

template <bool IS_INT>
__device__ __forceinline__ double key_value_sum(unsigned ka, unsigned kb) {
    if (IS_INT) return ((double)(int)(ka ^ 0x80000000u) + (double)(int)(kb ^ 0x80000000u)) / 2.0;
    const float a = f32_from_order_key(ka);
    if (ka == kb) return (double)a;                      // numpy averages ONE element when the count is odd: no a + a overflow
    const float b = f32_from_order_key(kb);
    return (double)((a + b) * 0.5f);
}

template <bool IS_INT, bool TAKE_ABS>
__global__ __launch_bounds__(CM_THREADS) void column_median_kernel(const void* __restrict__ planes, long long ld, int N,
                                                                    double* __restrict__ median, int* __restrict__ n_valid) {
    __shared__ CmScratch sc;
    const int tid = threadIdx.x, wave = tid / MEDP_WAVE;
    const void* column = (const char*)planes + (size_t)blockIdx.x * (size_t)ld * 4;
    if (tid == 0) {
        sc.prefix = 0u;
        sc.rank = 0u;
        sc.below = 0u;
    }
    unsigned m = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned fixed = pass == 0 ? 0u : 0xffffffffu << (shift + 8);     // the key bits earlier passes settled
        for (int j = tid; j < CM_WAVES * CM_BINS; j += CM_THREADS) (&sc.hist[0][0])[j] = 0u;
        __syncthreads();
        const unsigned prefix = sc.prefix;
        // a run of equal digits in a thread's own elements costs one atomic (columns of few distinct values are the common case)
        unsigned run_bin = 0, run = 0;
        for (size_t i = tid; i < (size_t)N; i += CM_THREADS) {
            unsigned key;
            if (!column_key<IS_INT, TAKE_ABS>(column, i, key) || (key & fixed) != prefix) continue;
            const unsigned bin = (key >> shift) & 0xffu;
            if (bin != run_bin && run) {
                atomicAdd(&sc.hist[wave][run_bin], run);
                run = 0;
            }
            run_bin = bin;
            ++run;
        }
        if (run) atomicAdd(&sc.hist[wave][run_bin], run);
        __syncthreads();
        if (tid < CM_BINS) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < CM_WAVES; ++w) s += sc.hist[w][tid];
            sc.merged[tid] = s;
        }
        __syncthreads();
        if (pass == 0) {                                 // the first histogram holds every valid entry
            for (int b = 0; b < CM_BINS; ++b) m += sc.merged[b];
            if (m == 0) {
                if (tid == 0) {
                    median[blockIdx.x] = kNaN;
                    n_valid[blockIdx.x] = 0;
                }
                return;
            }
        }
        if (tid == 0) {
            unsigned r = pass == 0 ? (m - 1) / 2 : sc.rank, cum = 0;
            int b = 0;
            for (; b < CM_BINS - 1 && cum + sc.merged[b] <= r; ++b) cum += sc.merged[b];
            sc.prefix = prefix | ((unsigned)b << shift);
            sc.rank = r - cum;                           // the rank among the keys that share the new prefix
            sc.below += cum;                             // keys strictly below every key with the new prefix
            sc.equal = sc.merged[b];
            sc.next_key = 0xffffffffu;
        }
        __syncthreads();
    }
    const unsigned ka = sc.prefix;                       // the key at sorted rank (m - 1) / 2
    const unsigned at_most = sc.below + sc.equal;        // keys <= ka
    unsigned kb = ka;
    if (m / 2 >= at_most) {                              // rank m / 2 lies past the copies of ka: the smallest key above it
        unsigned best = 0xffffffffu;
        for (size_t i = tid; i < (size_t)N; i += CM_THREADS) {
            unsigned key;
            if (column_key<IS_INT, TAKE_ABS>(column, i, key) && key > ka) best = min(best, key);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
        if ((tid & (MEDP_WAVE - 1)) == 0) atomicMin(&sc.next_key, best);
        __syncthreads();
        kb = sc.next_key;
    }
    if (tid == 0) {
        median[blockIdx.x] = key_value_sum<IS_INT>(ka, kb);
        n_valid[blockIdx.x] = (int)m;
    }
}

}  // namespace

extern "C" int medp_trajectory_cells(const float* x, int n, int T, int V, int n_timesteps, int n0, long long ld, int* obs_hours,
                                     float* total, float* recency, float* within_std, float* endpoint_change, int* per_sample,
                                     long long* var_counts, void* stream) {
    MEDP_CHECK_ARG(x && obs_hours && total && recency && within_std && endpoint_change && per_sample && var_counts,
                   "trajectory_cells: null argument");
    MEDP_CHECK_ARG(n >= 1 && T >= 1 && V >= 1 && n0 >= 0, "trajectory_cells: bad shape n=%d T=%d V=%d n0=%d", n, T, V, n0);
    MEDP_CHECK_ARG(ld >= (long long)n0 + n, "trajectory_cells: ld=%lld is shorter than n0 + n = %lld", ld, (long long)n0 + n);
    MEDP_CHECK_ARG((long long)V * 2 <= INT_MAX, "trajectory_cells: V=%d", V);
    const unsigned tiles_n = (unsigned)((n + TC_TILE - 1) / TC_TILE), tiles_v = (unsigned)((V + TC_TILE - 1) / TC_TILE);
    MEDP_CHECK_ARG(tiles_v <= 65535u, "trajectory_cells: V=%d needs %u variable tiles", V, tiles_v);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(per_sample + (size_t)n0 * 4, 0, (size_t)n * 4 * sizeof(int), st);      // this chunk's rows only
    if (e != hipSuccess) {
        medp_set_error("trajectory_cells: clearing the per-sample counts failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    traj_cells_kernel<<<dim3(tiles_n, tiles_v), TC_THREADS, 0, st>>>(x, n, T, V, n_timesteps, n0, ld, obs_hours, total, recency, within_std,
                                                                     endpoint_change, per_sample, (unsigned long long*)var_counts);
    MEDP_LAUNCH_CHECK("medp_trajectory_cells");
    return 0;
}

extern "C" int medp_column_medians(const void* planes, long long ld, int n_cols, int N, int is_int32, int take_abs, double* median,
                                   int* n_valid, void* stream) {
    MEDP_CHECK_ARG(planes && median && n_valid, "column_medians: null argument");
    MEDP_CHECK_ARG(n_cols >= 1 && N >= 1 && ld >= N, "column_medians: bad shape n_cols=%d N=%d ld=%lld", n_cols, N, ld);
    MEDP_CHECK_ARG(N <= MEDP_COLUMN_MEDIAN_MAX_N, "column_medians: N=%d exceeds MEDP_COLUMN_MEDIAN_MAX_N=%d", N, MEDP_COLUMN_MEDIAN_MAX_N);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_cols);
    if (is_int32) {
        if (take_abs) column_median_kernel<true, true><<<grid, CM_THREADS, 0, st>>>(planes, ld, N, median, n_valid);
        else column_median_kernel<true, false><<<grid, CM_THREADS, 0, st>>>(planes, ld, N, median, n_valid);
    } else {
        if (take_abs) column_median_kernel<false, true><<<grid, CM_THREADS, 0, st>>>(planes, ld, N, median, n_valid);
        else column_median_kernel<false, false><<<grid, CM_THREADS, 0, st>>>(planes, ld, N, median, n_valid);
    }
    MEDP_LAUNCH_CHECK("medp_column_medians");
    return 0;
}
