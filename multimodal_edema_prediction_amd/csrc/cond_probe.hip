// Conditional-information probe (reference analysis/conditional_information_probe.py; DESIGN.md "Conditional-information probe"):
// the device half of a batched damped-Newton fit of Pipeline(StandardScaler, LogisticRegression(C)) with a free, unpenalised
// intercept, for P problems (label x probe) per launch.  Everything here is fp64; functional.precision() is not consulted.  The
// features are read in place from the teacher's fp32 outputs through the problem table (medp_hip.h, MedpProbeProblem) and are
// standardised on the fly: no standardised copy is ever made.
//
//   probe_moments_kernel     mean / population variance (two-pass centred) / scale of every column of every problem.
//   probe_valgrad_kernel +   objective and gradient, plus the per-row curvature d_i = p_i (1 - p_i) into the workspace.  A
//   probe_finish_kernel      workgroup owns PT_ROWS rows of one problem; a row is dotted by a group of `lpr` lanes (4 / 16 / 64 by
//                            the launch's Fmax, so that the three-column logit probes do not idle 61 lanes of 64).  The X^T.r half
//                            re-reads the block's rows (the same CU read them a moment ago: L1 / L2 hits).  Per-block partials are
//                            added by the finish kernel in block order: no floating-point atomics, two launches are bit-identical.
//   probe_hessian_kernel     weighted Gram matrix mean_i d_i a_i a_i^T: a workgroup owns one 32 x 32 tile of the UPPER triangle of
//                            one problem and walks all of its rows in order (no partials), then stores the tile and its mirror
//                            image from the same registers: H is exactly symmetric.
//   probe_scores_kernel      decision-function parts sum_{j0 <= j < j1} theta_j a_ij (+ intercept) over any row list.
// A row index outside [0, N) is never dereferenced: it poisons its problem's outputs with NaN.
#include "common.h"
#include "medp_hip.h"

namespace {

constexpr int PT_THREADS = 256, PT_WAVES = PT_THREADS / 64;
constexpr int PT_ROWS = 64;                       // rows of one problem per workgroup (valgrad, scores)
constexpr int MO_SLICES = 16, MO_THREADS = 64 * MO_SLICES;
constexpr int HT = 32;                            // Hessian tile edge; 256 threads own 2 x 2 entries each
constexpr int HC = 32;                            // rows staged per step of the Hessian walk

// sum over the aligned group of `lpr` (a power of two <= 64) lanes this lane belongs to: a fixed butterfly, the same on every run
__device__ __forceinline__ double group_sum_f64(double v, int lpr) {
    for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// moments: grid (ceil(Fmax / 64), P); lane = column (coalesced), the 16 waves deal the rows round-robin and are added in order
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void probe_moments_kernel(const float* __restrict__ X, long long ldx, int N,
                                                                    const MedpProbeProblem* __restrict__ tab, const int* __restrict__ rows,
                                                                    double* __restrict__ mean, double* __restrict__ scale, int Fmax) {
    __shared__ double red[MO_SLICES][64];
    __shared__ double mu[64];
    const MedpProbeProblem pb = tab[blockIdx.y];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const bool live = col < pb.F;
    const int n = pb.n_rows;
    const int* rl = rows + pb.row_off;
    const float* xc = X + pb.col_off + col;
    double s = 0.0;
    if (live)
        for (int i = slice; i < n; i += MO_SLICES) {
            const int r = rl[i];
            s += (unsigned)r < (unsigned)N ? (double)xc[(size_t)r * ldx] : kNaN;
        }
    red[slice][lane] = s;
    __syncthreads();
    if (slice == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < MO_SLICES; ++k) t += red[k][lane];
        mu[lane] = t / (double)n;
    }
    __syncthreads();
    const double m = mu[lane];
    double q = 0.0;
    if (live)
        for (int i = slice; i < n; i += MO_SLICES) {
            const int r = rl[i];
            const double dv = ((unsigned)r < (unsigned)N ? (double)xc[(size_t)r * ldx] : kNaN) - m;
            q = fma(dv, dv, q);
        }
    __syncthreads();
    red[slice][lane] = q;
    __syncthreads();
    if (slice == 0 && col < Fmax) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < MO_SLICES; ++k) t += red[k][lane];
        const double var = t / (double)n, eps = 2.220446049250313e-16, nm = (double)n * m * eps;
        // a constant column keeps scale 1 (StandardScaler's test, Preprocessor.fit); a padded column reads as mean 0, scale 1
        const bool constant = var <= (double)n * eps * var + nm * nm;
        const size_t o = (size_t)blockIdx.y * Fmax + col;
        mean[o] = live ? m : 0.0;
        scale[o] = live ? (constant ? 1.0 : sqrt(var)) : 1.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// objective + gradient (+ d_i): grid (nblk, P)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void probe_valgrad_kernel(const float* __restrict__ X, long long ldx, int N,
                                                                    const float* __restrict__ y, int ldy,
                                                                    const MedpProbeProblem* __restrict__ tab, const int* __restrict__ rows,
                                                                    const double* __restrict__ theta, const double* __restrict__ mean,
                                                                    const double* __restrict__ scale, double* __restrict__ gpart,
                                                                    double* __restrict__ lpart, double* __restrict__ dws, int Fmax, int nblk,
                                                                    int lpr) {
    __shared__ double rs[PT_ROWS];                // residuals p_i - y_i
    __shared__ int ri[PT_ROWS];                   // checked row indices (-1: outside [0, N))
    __shared__ double lw[PT_WAVES];
    const MedpProbeProblem pb = tab[blockIdx.y];
    const int r0 = blockIdx.x * PT_ROWS;
    if (r0 >= pb.n_rows) return;                  // the grid is sized by the longest problem
    const int rb = min(PT_ROWS, pb.n_rows - r0), F = pb.F, S = Fmax + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gpw = 64 / lpr, sub = lane / lpr, gl = lane % lpr;
    const double* th = theta + (size_t)blockIdx.y * S;
    const double* mu = mean + (size_t)blockIdx.y * Fmax;
    const double* sc = scale + (size_t)blockIdx.y * Fmax;
    const float* xb = X + pb.col_off;
    double loss = 0.0;                            // a group's leader lane: its rows in row order
    for (int r = wave * gpw + sub; r < PT_ROWS; r += PT_WAVES * gpw) {      // the same trip count for every lane of a wave
        const bool in = r < rb;
        const int row = in ? rows[pb.row_off + r0 + r] : 0;
        const bool ok = in && (unsigned)row < (unsigned)N;
        double acc = 0.0;
        if (ok) {
            const float* xr = xb + (size_t)row * ldx;
            for (int f = gl; f < F; f += lpr) acc = fma(((double)xr[f] - mu[f]) / sc[f], th[f], acc);
        }
        acc = group_sum_f64(acc, lpr);
        if (in && gl == 0) {
            const double s = ok ? acc + th[Fmax] : kNaN, yy = ok ? (double)y[(size_t)row * ldy + pb.y_col] : kNaN;
            const double e = exp(-fabs(s));                                  // overflow-safe logaddexp(0, s) and expit(s)
            loss += fmax(s, 0.0) + log1p(e) - yy * s;
            rs[r] = (s >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - yy;
            ri[r] = ok ? row : -1;
            if (dws) dws[pb.row_off + r0 + r] = e / ((1.0 + e) * (1.0 + e));  // p (1 - p) without the cancellation near p = 1
        }
    }
    loss = group_sum_f64(loss, 64);
    if (lane == 0) lw[wave] = loss;
    __syncthreads();
    double* gp = gpart + ((size_t)blockIdx.y * nblk + blockIdx.x) * S;
    if (tid == PT_THREADS - 1) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < PT_WAVES; ++w) s += lw[w];
        lpart[(size_t)blockIdx.y * nblk + blockIdx.x] = s;
        double g = 0.0;
        for (int r = 0; r < rb; ++r) g += rs[r];
        gp[Fmax] = g;                             // the intercept's column of ones
    }
    // X^T.r over this block's rows: thread per column, rows in order
    for (int f = tid; f < F; f += PT_THREADS) {
        const double m = mu[f], sd = sc[f];
        double acc = 0.0;
        for (int r = 0; r < rb; ++r) {
            const int row = ri[r];
            const double a = row >= 0 ? ((double)xb[(size_t)row * ldx + f] - m) / sd : kNaN;
            acc = fma(a, rs[r], acc);
        }
        gp[f] = acc;
    }
}

// grid (P): block-order sums of the partials; with H, also the padded rows / columns of H (zero, 1 on the diagonal)
__global__ __launch_bounds__(PT_THREADS) void probe_finish_kernel(const MedpProbeProblem* __restrict__ tab, const double* __restrict__ theta,
                                                                   const double* __restrict__ l2, const double* __restrict__ gpart,
                                                                   const double* __restrict__ lpart, double* __restrict__ f,
                                                                   double* __restrict__ g, double* __restrict__ H, int Fmax, int nblk) {
    const int p = blockIdx.x, tid = threadIdx.x, S = Fmax + 1;
    const MedpProbeProblem pb = tab[p];
    const int F = pb.F, nb = (pb.n_rows + PT_ROWS - 1) / PT_ROWS;
    const double inv_n = 1.0 / (double)pb.n_rows, lam = l2[p];
    const double* th = theta + (size_t)p * S;
    for (int j = tid; j < S; j += PT_THREADS) {
        double v = 0.0;
        if (j < F || j == Fmax) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += gpart[((size_t)p * nblk + b) * S + j];
            v = s * inv_n + (j < F ? lam * th[j] : 0.0);                     // the intercept is not penalised
        }
        g[(size_t)p * S + j] = v;
    }
    if (tid < 64) {
        double ls = 0.0, ww = 0.0;
        for (int b = tid; b < nb; b += 64) ls += lpart[(size_t)p * nblk + b];
        for (int j = tid; j < F; j += 64) ww = fma(th[j], th[j], ww);
        ls = group_sum_f64(ls, 64);
        ww = group_sum_f64(ww, 64);
        if (tid == 0) f[p] = ls * inv_n + 0.5 * lam * ww;
    }
    if (H) {
        double* Hp = H + (size_t)p * S * S;
        const int pad = Fmax - F;
        for (int e = tid; e < pad * S; e += PT_THREADS) {
            const int j = F + e / S, k = e % S;
            Hp[(size_t)j * S + k] = j == k ? 1.0 : 0.0;
            Hp[(size_t)k * S + j] = j == k ? 1.0 : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Hessian: grid (nt (nt + 1) / 2, P), nt = ceil((Fmax + 1) / HT).  Logical column j < F is feature j, j == F the intercept's ones.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void probe_hessian_kernel(const float* __restrict__ X, long long ldx, int N,
                                                                    const MedpProbeProblem* __restrict__ tab, const int* __restrict__ rows,
                                                                    const double* __restrict__ mean, const double* __restrict__ scale,
                                                                    const double* __restrict__ l2, const double* __restrict__ dws,
                                                                    double* __restrict__ H, int Fmax, int nt) {
    __shared__ __attribute__((aligned(16))) double As[HC][HT];              // d_i a_i over the tile's row range of columns
    __shared__ __attribute__((aligned(16))) double Bs[HC][HT];              // a_i over the tile's column range
    const int p = blockIdx.y, tid = threadIdx.x, S = Fmax + 1;
    const MedpProbeProblem pb = tab[p];
    const int F = pb.F, L = F + 1, n = pb.n_rows;
    int ti = 0, rem = blockIdx.x;
    while (ti < nt && rem >= nt - ti) {           // at most nt steps: the launch's tile count
        rem -= nt - ti;
        ++ti;
    }
    const int tj = ti + rem;
    if (ti * HT >= L || tj * HT >= L) return;     // a narrower problem of a mixed-width launch
    const double* mu = mean + (size_t)p * Fmax;
    const double* sc = scale + (size_t)p * Fmax;
    const float* xb = X + pb.col_off;
    const int tx = tid & 15, ty = tid >> 4;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int c0 = 0; c0 < n; c0 += HC) {
        for (int e = tid; e < HC * HT; e += PT_THREADS) {
            const int r = e / HT, c = e % HT, i = c0 + r;
            double a = 0.0, b = 0.0;
            if (i < n) {
                const int row = rows[pb.row_off + i];
                const bool ok = (unsigned)row < (unsigned)N;
                const double d = dws[pb.row_off + i];
                const int ja = ti * HT + c, jb = tj * HT + c;
                if (ja < F) a = ok ? d * (((double)xb[(size_t)row * ldx + ja] - mu[ja]) / sc[ja]) : kNaN;
                else if (ja == F) a = ok ? d : kNaN;
                if (jb < F) b = ok ? ((double)xb[(size_t)row * ldx + jb] - mu[jb]) / sc[jb] : kNaN;
                else if (jb == F) b = ok ? 1.0 : kNaN;
            }
            As[r][c] = a;
            Bs[r][c] = b;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < HC; ++r) {
            const double a0 = As[r][ty * 2], a1 = As[r][ty * 2 + 1], b0 = Bs[r][tx * 2], b1 = Bs[r][tx * 2 + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    const double inv_n = 1.0 / (double)n, lam = l2[p];
    double* Hp = H + (size_t)p * S * S;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int ja = ti * HT + ty * 2 + ii, jb = tj * HT + tx * 2 + jj;
            if (ja >= L || jb >= L || ja > jb) continue;                     // the upper triangle only; its mirror is stored from here
            const double v = acc[ii][jj] * inv_n + (ja == jb && ja < F ? lam : 0.0);
            const int oa = ja < F ? ja : Fmax, ob = jb < F ? jb : Fmax;      // the intercept sits last, after the padding
            Hp[(size_t)oa * S + ob] = v;
            if (ja != jb) Hp[(size_t)ob * S + oa] = v;
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// scores: grid (nblk, P)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void probe_scores_kernel(const float* __restrict__ X, long long ldx, int N,
                                                                   const MedpProbeProblem* __restrict__ tab, const int* __restrict__ rows,
                                                                   const double* __restrict__ theta, const double* __restrict__ mean,
                                                                   const double* __restrict__ scale, double* __restrict__ out, int Fmax,
                                                                   int add_intercept, int lpr) {
    const MedpProbeProblem pb = tab[blockIdx.y];
    const int r0 = blockIdx.x * PT_ROWS;
    if (r0 >= pb.n_rows) return;
    const int rb = min(PT_ROWS, pb.n_rows - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gpw = 64 / lpr, sub = lane / lpr, gl = lane % lpr;
    const double* th = theta + (size_t)blockIdx.y * (Fmax + 1);
    const double* mu = mean + (size_t)blockIdx.y * Fmax;
    const double* sc = scale + (size_t)blockIdx.y * Fmax;
    for (int r = wave * gpw + sub; r < PT_ROWS; r += PT_WAVES * gpw) {
        const bool in = r < rb;
        const int row = in ? rows[pb.row_off + r0 + r] : 0;
        const bool ok = in && (unsigned)row < (unsigned)N;
        double acc = 0.0;
        if (ok) {
            const float* xr = X + pb.col_off + (size_t)row * ldx;
            for (int f = pb.j0 + gl; f < pb.j1; f += lpr) acc = fma(((double)xr[f] - mu[f]) / sc[f], th[f], acc);
        }
        acc = group_sum_f64(acc, lpr);
        if (in && gl == 0) out[pb.row_off + r0 + r] = ok ? acc + (add_intercept ? th[Fmax] : 0.0) : kNaN;
    }
}

// the argument checks every entry point shares; the table is read on the host here and on the device by the kernels
int check_table(const char* what, const void* X, long long ldx, int N, const MedpProbeProblem* th, const MedpProbeProblem* td,
                const int* rows, long long rows_total, int P, int Fmax, int ldy, bool ranges, int* max_rows) {
    MEDP_CHECK_ARG(X && th && td && rows, "%s: null argument", what);
    MEDP_CHECK_ARG(P >= 1 && P <= 65535, "%s: P=%d is not in [1, 65535]", what, P);
    MEDP_CHECK_ARG(Fmax >= 1 && N >= 1 && ldx >= 1, "%s: bad shape Fmax=%d N=%d ldx=%lld", what, Fmax, N, ldx);
    int longest = 0;
    long long prev_end = 0;
    for (int p = 0; p < P; ++p) {
        const MedpProbeProblem& q = th[p];
        MEDP_CHECK_ARG(q.F >= 1 && q.F <= Fmax, "%s: problem %d has F=%d, not in [1, Fmax=%d]", what, p, q.F, Fmax);
        MEDP_CHECK_ARG(q.n_rows >= 2, "%s: problem %d has %d rows (at least 2 are needed)", what, p, q.n_rows);
        MEDP_CHECK_ARG(q.col_off >= 0 && q.col_off + q.F <= ldx, "%s: problem %d columns [%lld, %lld) leave a row of %lld", what, p,
                       q.col_off, q.col_off + q.F, ldx);
        MEDP_CHECK_ARG(q.row_off >= 0 && q.row_off + q.n_rows <= rows_total, "%s: problem %d rows [%lld, %lld) leave the list of %lld",
                       what, p, q.row_off, q.row_off + q.n_rows, rows_total);
        // per-row values (d_i, the scores) live at a row's position in the list: the stretches follow one another without overlap
        MEDP_CHECK_ARG(q.row_off >= prev_end, "%s: problem %d rows start at %lld, before problem %d ends (%lld)", what, p, q.row_off, p - 1,
                       prev_end);
        prev_end = q.row_off + q.n_rows;
        if (ldy > 0) MEDP_CHECK_ARG(q.y_col >= 0 && q.y_col < ldy, "%s: problem %d label column %d is not in [0, %d)", what, p, q.y_col, ldy);
        if (ranges) MEDP_CHECK_ARG(q.j0 >= 0 && q.j0 <= q.j1 && q.j1 <= q.F, "%s: problem %d column range [%d, %d) is not within [0, F=%d]",
                                   what, p, q.j0, q.j1, q.F);
        longest = q.n_rows > longest ? q.n_rows : longest;
    }
    *max_rows = longest;
    return 0;
}

inline int host_lanes_per_row(int Fmax) { return Fmax <= 4 ? 4 : Fmax <= 16 ? 16 : 64; }

}  // namespace

extern "C" int medp_probe_moments(const float* X, long long ldx, int N, const MedpProbeProblem* table_host,
                                  const MedpProbeProblem* table_dev, const int* rows, long long rows_total, double* mean, double* scale,
                                  int P, int Fmax, void* stream) {
    int max_rows = 0;
    MEDP_TRY(check_table("probe_moments", X, ldx, N, table_host, table_dev, rows, rows_total, P, Fmax, 0, false, &max_rows));
    MEDP_CHECK_ARG(mean && scale, "probe_moments: null argument");
    probe_moments_kernel<<<dim3((Fmax + 63) / 64, P), MO_THREADS, 0, (hipStream_t)stream>>>(X, ldx, N, table_dev, rows, mean, scale, Fmax);
    MEDP_LAUNCH_CHECK("medp_probe_moments");
    return 0;
}

extern "C" size_t medp_probe_terms_ws_bytes(int P, int Fmax, int max_rows, long long rows_total) {
    if (P < 1 || Fmax < 1 || max_rows < 2 || rows_total < max_rows) return 0;
    const size_t nblk = ((size_t)max_rows + PT_ROWS - 1) / PT_ROWS;
    return ((size_t)P * nblk * (Fmax + 2) + (size_t)rows_total) * sizeof(double);
}

extern "C" int medp_logistic_newton_terms(const float* X, long long ldx, int N, const float* y, int ldy,
                                          const MedpProbeProblem* table_host, const MedpProbeProblem* table_dev, const int* rows,
                                          long long rows_total, const double* theta, const double* mean, const double* scale,
                                          const double* l2, double* f, double* g, double* H, void* ws, size_t ws_bytes, int P, int Fmax,
                                          void* stream) {
    int max_rows = 0;
    MEDP_CHECK_ARG(ldy >= 1, "logistic_newton_terms: ldy=%d < 1", ldy);
    MEDP_TRY(check_table("logistic_newton_terms", X, ldx, N, table_host, table_dev, rows, rows_total, P, Fmax, ldy, false, &max_rows));
    MEDP_CHECK_ARG(y && theta && mean && scale && l2 && f && g && ws, "logistic_newton_terms: null argument");
    const size_t need = medp_probe_terms_ws_bytes(P, Fmax, max_rows, rows_total);
    MEDP_CHECK_ARG(ws_bytes >= need, "logistic_newton_terms: workspace %zu < %zu bytes", ws_bytes, need);
    const int nblk = (max_rows + PT_ROWS - 1) / PT_ROWS, S = Fmax + 1;
    double* gpart = (double*)ws;
    double* lpart = gpart + (size_t)P * nblk * S;
    double* dws = lpart + (size_t)P * nblk;
    hipStream_t st = (hipStream_t)stream;
    probe_valgrad_kernel<<<dim3(nblk, P), PT_THREADS, 0, st>>>(X, ldx, N, y, ldy, table_dev, rows, theta, mean, scale, gpart, lpart,
                                                               H ? dws : nullptr, Fmax, nblk, host_lanes_per_row(Fmax));
    MEDP_LAUNCH_CHECK("medp_logistic_newton_terms");
    probe_finish_kernel<<<P, PT_THREADS, 0, st>>>(table_dev, theta, l2, gpart, lpart, f, g, H, Fmax, nblk);
    MEDP_LAUNCH_CHECK("medp_logistic_newton_terms (finish)");
    if (H) {
        const int nt = (S + HT - 1) / HT;
        MEDP_CHECK_ARG((long long)nt * (nt + 1) / 2 <= 0x7fffffffLL, "logistic_newton_terms: too many Hessian tiles");
        probe_hessian_kernel<<<dim3(nt * (nt + 1) / 2, P), PT_THREADS, 0, st>>>(X, ldx, N, table_dev, rows, mean, scale, l2, dws, H, Fmax, nt);
        MEDP_LAUNCH_CHECK("medp_logistic_newton_terms (Hessian)");
    }
    return 0;
}

extern "C" int medp_probe_scores(const float* X, long long ldx, int N, const MedpProbeProblem* table_host,
                                 const MedpProbeProblem* table_dev, const int* rows, long long rows_total, const double* theta,
                                 const double* mean, const double* scale, double* out, int P, int Fmax, int add_intercept, void* stream) {
    int max_rows = 0;
    MEDP_TRY(check_table("probe_scores", X, ldx, N, table_host, table_dev, rows, rows_total, P, Fmax, 0, true, &max_rows));
    MEDP_CHECK_ARG(theta && mean && scale && out, "probe_scores: null argument");
    const int nblk = (max_rows + PT_ROWS - 1) / PT_ROWS;
    probe_scores_kernel<<<dim3(nblk, P), PT_THREADS, 0, (hipStream_t)stream>>>(X, ldx, N, table_dev, rows, theta, mean, scale, out, Fmax,
                                                                               add_intercept, host_lanes_per_row(Fmax));
    MEDP_LAUNCH_CHECK("medp_probe_scores");
    return 0;
}
