// DuETT embedding stage for gfx950, inference form (BatchNorm folded to an affine): psi and the time embedding
//   (reference models/main_architecture_duett.py:41-69), as medp_duett_encode (duett.hip) launches them and on their own.
//
// psi [B, T+1, V+1, E] is built by ONE launch, directly in the event view [B, V+1, (T+1)E] with the event embedding added and the
// event encoder's first ScaleNorm applied (the reference runs V sequential 5-op MLPs, ~250 eager launches); the time embedding
// [B, T+1, (V+1)E] by a second.  Both have an exact-fp32 matrix-core form and the VALU form it replaced, bit for bit alike.
#include "common.h"
#include "duett_cells.h"
#include "duett_front.h"
#include "medp_hip.h"
#include "norm_rows.h"

namespace {

// ---- time embedding (K6): cve(batch_norm) = Linear(1,h) -> tanh -> BN affine -> Linear(h, tt) ; REP row appended ------
// 16 rows (b, t) per workgroup and one output column per thread: a column of the second Linear is read once per 16 rows and the
// hidden activations come from LDS by broadcast.  (One row per workgroup re-read the whole 34 x 1176 weight for every row:
// 127 us for a 29-MB result.)  Per output the products are still summed in ascending j: results unchanged.
constexpr int TE_ROWS = 16;
__global__ __launch_bounds__(256) void time_embed_kernel(const float* __restrict__ times, const float* __restrict__ w0,
                                                         const float* __restrict__ b0, const float* __restrict__ s,
                                                         const float* __restrict__ sh, const float* __restrict__ w3,
                                                         const float* __restrict__ b3, const float* __restrict__ rep,
                                                         float* __restrict__ out, int B, int T, int Hd, int tt) {
    extern __shared__ float hid[];              // [Hd][TE_ROWS]; the kernel's only LDS, so it starts 16-B aligned (the float4 reads below)
    const int rows = B * (T + 1);
    const int r0 = blockIdx.x * TE_ROWS;
    for (int idx = threadIdx.x; idx < TE_ROWS * Hd; idx += 256) {
        const int rr = idx / Hd, j = idx - rr * Hd, row = r0 + rr;
        float h = 0.f;
        if (row < rows) {
            const int b = row / (T + 1), t = row - b * (T + 1);
            if (t < T) h = fmaf(tanhf(fmaf(w0[j], times[(size_t)b * T + t], b0[j])), s[j], sh[j]);      // (explicit fmaf: the same in time_embed_mfma_kernel)
        }
        hid[j * TE_ROWS + rr] = h;             // [Hd][TE_ROWS]: the 16 rows of one hidden unit are one 64-B broadcast read
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= tt) return;
    float acc[TE_ROWS];
    const float bias = b3[c];
#pragma unroll
    for (int rr = 0; rr < TE_ROWS; ++rr) acc[rr] = bias;
    // w3t is the TRANSPOSED weight [Hd][tt]: consecutive threads read consecutive addresses
    // (eight weight loads in flight: one per iteration made the loop a chain of L2 round trips)
    int j = 0;
    for (; j + 8 <= Hd; j += 8) {
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = w3[(size_t)(j + u) * tt + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4* hj = (const float4*)(hid + (j + u) * TE_ROWS);
#pragma unroll
            for (int q = 0; q < TE_ROWS / 4; ++q) {
                const float4 h4 = hj[q];
                acc[4 * q] = fmaf(w[u], h4.x, acc[4 * q]); acc[4 * q + 1] = fmaf(w[u], h4.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(w[u], h4.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(w[u], h4.w, acc[4 * q + 3]);
            }
        }
    }
    for (; j < Hd; ++j) {
        const float w = w3[(size_t)j * tt + c];
#pragma unroll
        for (int rr = 0; rr < TE_ROWS; ++rr) acc[rr] = fmaf(w, hid[j * TE_ROWS + rr], acc[rr]);
    }
    const float repc = rep[c];
#pragma unroll
    for (int rr = 0; rr < TE_ROWS; ++rr) {
        const int row = r0 + rr;
        if (row < rows) out[(size_t)row * tt + c] = (row % (T + 1) == T) ? repc : acc[rr];     // REP row appended
    }
}

// ---- time embedding on the matrix cores, in exact fp32 --------------------------------------------------------------------------------
// out[row][c] = b3[c] + sum_j w3t[j][c] * hid[row][j] is a [B(T+1) x Hd] x [Hd x tt] product (6208 x 34 x 1176 at cfg3): 0.5 GFLOP behind a
// 29-MB store.  v_mfma_f32_16x16x4_f32 takes fp32 operands and its result is bit for bit the k-ordered fmaf chain the VALU kernel above
// computes (C-in = the bias, products added in ascending j; the rows of k past Hd are zeros: fma(0, 0, acc) = acc), so the fp32 kernel
// mode needs no second form.  A wave owns 16 rows: each lane computes 9 of their 16 x 36 hidden activations (the A fragments, kept in
// registers for the whole launch) and walks its share of the 16-column tiles; the B fragments come straight from the L2-resident weight.
constexpr int TEM_KS = 9;                                    // k-steps of 4: hidden widths up to 36
constexpr int TEM_CW = 208;                                  // columns per workgroup (13 tiles of 16); 208 floats = 6.5 x 32 banks: the two
                                                             // 16-lane k-groups of a 32-lane half read disjoint bank sets (conflict-free ds_read_b32)
__global__ __launch_bounds__(256) void time_embed_mfma_kernel(const float* __restrict__ times, const float* __restrict__ w0,
                                                              const float* __restrict__ b0, const float* __restrict__ s,
                                                              const float* __restrict__ sh, const float* __restrict__ w3t,
                                                              const float* __restrict__ b3, const float* __restrict__ rep,
                                                              float* __restrict__ out, int B, int T, int Hd, int tt) {
    // the workgroup's slice of the second Linear, [4 TEM_KS][TEM_CW] + bias + REP rows, staged once (coalesced) and read back as B
    // fragments by all four waves for every column tile: the first form loaded them from L2 tile by tile — 13 dependent ~1-us round
    // trips per wave, 18.7 us for a launch whose matrix work is 3.5 us
    __shared__ __attribute__((aligned(16))) float sw[(4 * TEM_KS + 2) * TEM_CW];
    const int lane = threadIdx.x & 63, rr = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = B * (T + 1);
    const int c0 = blockIdx.y * TEM_CW, ncol = min(TEM_CW, tt - c0);
    {   // 38 rows of 52 float4 (the tail rows: zeros, bias, REP); every thread's 8 loads are independent and issued together — one load
        // per loop iteration made the staging a chain of 31 L2 round trips (23 us for the launch)
        constexpr int C4 = TEM_CW / 4, N4 = (4 * TEM_KS + 2) * C4;
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i4 = threadIdx.x + 256 * u, j = i4 / C4, cc = (i4 - j * C4) * 4;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i4 < N4 && cc < ncol) {                    // (tt and the chunk width are multiples of 4: a float4 is all in or all out)
                const float* src = j < Hd ? w3t + (size_t)j * tt : (j == 4 * TEM_KS ? b3 : (j == 4 * TEM_KS + 1 ? rep : nullptr));
                if (src) v[u] = *(const float4*)(src + c0 + cc);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i4 = threadIdx.x + 256 * u;
            if (i4 < N4) *(float4*)(sw + 4 * i4) = v[u];
        }
    }
    const int r0 = (blockIdx.x * 4 + wave) * 16;
    float a[TEM_KS];
    {
        const int row = r0 + rr;
        const int b = row / (T + 1), t = row - b * (T + 1);
        const bool live = row < rows && t < T;
        const float tv = live ? times[(size_t)b * T + t] : 0.f;
#pragma unroll
        for (int ks = 0; ks < TEM_KS; ++ks) {
            const int j = 4 * ks + kk;
            a[ks] = (live && j < Hd) ? fmaf(tanhf(fmaf(w0[j], tv, b0[j])), s[j], sh[j]) : 0.f;
        }
    }
    __syncthreads();
    if (r0 >= rows) return;
    bool is_rep[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) is_rep[r] = (r0 + kk * 4 + r) % (T + 1) == T;
    const int ntile = (ncol + 15) >> 4;
    for (int ct = 0; ct < ntile; ++ct) {
        const int cc = ct * 16 + rr;
        const float bias = sw[4 * TEM_KS * TEM_CW + cc], repc = sw[(4 * TEM_KS + 1) * TEM_CW + cc];
        f32x4 acc = (f32x4){bias, bias, bias, bias};
#pragma unroll
        for (int ks = 0; ks < TEM_KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], sw[(4 * ks + kk) * TEM_CW + cc], acc, 0, 0, 0);
        if (cc < ncol) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + kk * 4 + r;
                if (row < rows) out[(size_t)row * tt + c0 + cc] = is_rep[r] ? repc : acc[r];          // REP row appended
            }
        }
    }
}

// MEDP_EMBED_MFMA=0 (or medp_dbg_embed_mfma(0), tests): the VALU forms of the two embedding kernels, for A/B runs and bit comparisons
int g_embed_mfma = -1;
int embed_mfma_on() {
    if (g_embed_mfma < 0) g_embed_mfma = medp_env_int("MEDP_EMBED_MFMA", 1) != 0;
    return g_embed_mfma;
}

// ---- psi build + (time view -> event view) + event embedding + the event encoder's first ScaleNorm --------------------------
// One workgroup per event-view row (b, v): its T+1 cells are CONTIGUOUS in the event view ((T+1)*E floats), so the row is
// assembled in LDS and leaves in whole-row coalesced 16-B stores (a psi kernel in the time view writes 96-B cells 4.7 KB apart).
// psi0 is never written unless asked for; the launch reads 2.4 MB and writes |psi| fp32 + bf16.
// The row's norm is scalenorm_rn over the LDS tile: the re-read form of norm_rows.h, which agrees with the register form of the
// separate ScaleNorm launch up to the rounding of a row's sum; the bf16 `h` has equalled it in every tested case.
struct TabWeights {
    const float *xs, *w0, *b0, *s, *sh, *w4, *b4;
    int Ds, Hd;
};
template <int E, int HD>
__global__ __launch_bounds__(128) void psi_embed_event_kernel(const float* __restrict__ xs_ts, const float* __restrict__ l0,
                                                              const float* __restrict__ w4t, const float* __restrict__ b4,
                                                              const float* __restrict__ nobs_table, int nobs_rows, const TabWeights tw,
                                                              const float* __restrict__ special,
                                                              const float* __restrict__ event_emb, const float* __restrict__ g_norm,
                                                              float norm_eps, float* __restrict__ xe, bf16_t* __restrict__ h,
                                                              float* __restrict__ psi0_out, int B, int T, int V, int use_mfma) {
    // A workgroup = one variable v of one batch element b (one cell per lane and pass); the variable's MLP (7.5 KB) is staged in
    // LDS once per workgroup and read back by broadcast 16-B reads.  What bounds the VALU form: every lane needs the same 29 floats
    // per hidden unit, and a wave-wide LDS read returns 1 KB through the CU's 128-B/clk LDS return path whether or not the lanes
    // share an address: 64 hidden units x 8 reads x 8 clocks per wave = 38 us of LDS time per CU at cfg3 (measured 44 us).  Tried
    // and measured: weights by scalar loads into SGPRs (48 us, 79 % of the wave cycles parked in s_waitcnt: SMEM returns out of
    // order, so only lgkmcnt(0) is available and the loads of a hidden unit cannot be overlapped with the previous one's FMAs);
    // 2 / 4 rows per workgroup, i.e. cells per lane, to amortise the reads (53 / 77 us: the launch then has 3 / 1.5 waves per SIMD
    // and the long waves no longer hide each other's latency).
    extern __shared__ __attribute__((aligned(16))) float tile[];          // [(T+1)*E] the row
    __shared__ __attribute__((aligned(16))) float sl0[HD * 8], sw4[HD * E], sb4[E];
    __shared__ float s_rn, s_tab[E], s_hid[256], s_part[2][E], s_nobs[64];
    const int v = blockIdx.y, b = blockIdx.x;
    const int T1 = T + 1, D = T1 * E, D4 = D >> 2;
    if (threadIdx.x < 64) s_nobs[threadIdx.x] = nobs_table[min((int)threadIdx.x, nobs_rows - 1)];
    if (v < V) {
        for (int i = threadIdx.x; i < HD * 8 / 4; i += 128) ((float4*)sl0)[i] = ((const float4*)(l0 + (size_t)v * HD * 8))[i];
        for (int i = threadIdx.x; i < HD * E / 4; i += 128) ((float4*)sw4)[i] = ((const float4*)(w4t + (size_t)v * HD * E))[i];
        if (threadIdx.x < E) sb4[threadIdx.x] = b4[(size_t)v * E + threadIdx.x];
    } else {
        // the static column's row: the sample's tab_encoder output (Linear(Ds,Hd) -> ReLU -> BN affine -> Linear(Hd,E), model :57,
        // duett.py:124-125) computed here, one hidden unit per thread — no separate launch in front of the psi build
        for (int j = threadIdx.x; j < tw.Hd; j += 128) {
            float a = tw.b0[j];
            for (int i = 0; i < tw.Ds; ++i) a += tw.w0[j * tw.Ds + i] * tw.xs[(size_t)b * tw.Ds + i];
            s_hid[j] = fmaxf(a, 0.f) * tw.s[j] + tw.sh[j];
        }
        __syncthreads();
        // second Linear: lane j multiplies hidden unit j (coalesced weight reads), wave tree + the two waves' halves per output
        // (a thread per output walked its 128 weights 512 B apart: 12 us per sample, the long pole of the whole launch)
        for (int e = 0; e < E; ++e) {
            float pa = 0.f;
            for (int j = threadIdx.x; j < tw.Hd; j += 128) pa += tw.w4[e * tw.Hd + j] * s_hid[j];
            pa = wave_sum(pa);
            if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][e] = pa;
        }
        __syncthreads();
        if (threadIdx.x < E) s_tab[threadIdx.x] = tw.b4[threadIdx.x] + s_part[0][threadIdx.x] + s_part[1][threadIdx.x];
        __syncthreads();
    }
    __syncthreads();
    // (whole waves enter: the matrix-core path below needs all 64 lanes; t >= T1 is "no cell" and is never stored)
    for (int t = threadIdx.x; t < ((T1 + 63) & ~63); t += 128) {
        float out[E];
        // every input this lane needs, loaded up front and unconditionally (independent loads in flight): behind the
        // data-dependent branches below they formed a chain of three L2 round trips per cell
        const PsiCellIn in(xs_ts, b, t, v, T, V);
        const int kind = psi_cell_classify(in, t, v, T, V);          // the cell rule: duett_cells.h
        const float val = in.val;
        const bool any_mlp = kind == PSI_VAR;
        // whole-vector overrides: static column (model :57), REP row (:58-60), masked timestep / event (:61-66; "no cell" too: never stored)
        const float* src = kind == PSI_STATIC ? s_tab : kind == PSI_REP ? special + E : special;
        float nob = 0.f;
        if (any_mlp) {
            src = nullptr;
            nob = s_nobs[min(max((int)in.count, 0), nobs_rows - 1)];            // .to(int).clip(0, 15) (model :41)
        }
        // ---- the variable's MLP on the matrix cores, in exact fp32: out[cell][e] = b4[e] + sum_j w4[e][j] h_j(cell) is a
        // [cells x 64] x [64 x 24] product per variable.  v_mfma_f32_16x16x4_f32 is bit for bit the ascending-j fmaf chain of the VALU
        // form below (C-in = b4), so results are unchanged and the fp32 kernel mode needs no second form.  A wave takes the cells of ITS
        // lanes in groups of 16 (t = 16 g .. 16 g + 15); a lane computes 16 of the group's 16 x 64 hidden activations (2 FMA + max + FMA
        // each: the A fragments), the second Linear's weights are the B fragments (read once per wave: 32 registers), and the VALU form's
        // 8 broadcast LDS reads per hidden unit and cell — what bound it (44 us) — are gone.
        bool mfma_done = false;
        if (use_mfma && v < V) {
            mfma_done = true;
            const int lane = threadIdx.x & 63, rr = lane & 15, kk = lane >> 4;
            const int tbase = t & ~63;                                    // first cell of this wave in this pass
            const unsigned long long need = __ballot(any_mlp);
            float bw0[16], bw1[16];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                bw0[ks] = sw4[(4 * ks + kk) * E + rr];
                bw1[ks] = rr < E - 16 ? sw4[(4 * ks + kk) * E + 16 + rr] : 0.f;
            }
            const float c0 = sb4[rr], c1 = rr < E - 16 ? sb4[16 + rr] : 0.f;
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {
                if (tbase + 16 * g >= T) break;                            // no time step in this group (wave-uniform)
                if (((need >> (16 * g)) & 0xffffull) == 0) continue;       // every cell of the group is an override row
                const float vg = __shfl(val, 16 * g + rr, 64), ng = __shfl(nob, 16 * g + rr, 64);
                f32x4 a0 = (f32x4){c0, c0, c0, c0}, a1 = (f32x4){c1, c1, c1, c1};
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    const int j = 4 * ks + kk;
                    const float4 la = *(const float4*)(sl0 + j * 8);
                    const float hj = fmaf(fmaxf(fmaf(la.x, vg, fmaf(la.y, ng, la.z)), 0.f), la.w, sl0[j * 8 + 4]);   // (as the VALU form below)
                    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(hj, bw0[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(hj, bw1[ks], a1, 0, 0, 0);
                }
                // C layout: column e = rr (+16), rows = cells 4 kk + r of the group
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tc = tbase + 16 * g + 4 * kk + r;
                    if (tc < T1) {
                        tile[tc * E + rr] = a0[r];
                        if (rr < E - 16) tile[tc * E + 16 + rr] = a1[r];
                    }
                }
            }
            // the wave's own LDS operations execute in order: the override rows below (same wave, same cells) land after these
            asm volatile("" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
        if (!mfma_done && v < V && __any(any_mlp)) {
#pragma unroll
            for (int e = 0; e < E; ++e) out[e] = sb4[e];
#pragma unroll 2
            for (int j = 0; j < HD; ++j) {
                const float4 la = *(const float4*)(sl0 + j * 8);        // w0[j][0], w0[j][1], b0[j], bn scale
                const float lsh = sl0[j * 8 + 4];                        // bn shift
                const float hj = fmaf(fmaxf(fmaf(la.x, val, fmaf(la.y, nob, la.z)), 0.f), la.w, lsh);   // explicit fmaf: both forms round alike
                const float4* wj = (const float4*)(sw4 + j * E);
#pragma unroll
                for (int e4 = 0; e4 < E / 4; ++e4) {
                    const float4 w = wj[e4];
                    out[4 * e4] = fmaf(w.x, hj, out[4 * e4]); out[4 * e4 + 1] = fmaf(w.y, hj, out[4 * e4 + 1]);
                    out[4 * e4 + 2] = fmaf(w.z, hj, out[4 * e4 + 2]); out[4 * e4 + 3] = fmaf(w.w, hj, out[4 * e4 + 3]);
                }
            }
        }
        if (t >= T1) continue;
        if (src) {
#pragma unroll
            for (int e = 0; e < E; ++e) out[e] = src[e];
        } else if (mfma_done) {                                      // the cell's row is in the tile already (written by this wave): take it back
#pragma unroll                                                        // for the psi0 copy, and rewrite it unchanged below
            for (int e = 0; e < E; ++e) out[e] = tile[t * E + e];
        }
        if (psi0_out) {                                              // parity checks only: psi0 in the time view, before the add
            float* d0 = psi0_out + (((size_t)b * T1 + t) * (V + 1) + v) * E;
#pragma unroll
            for (int e = 0; e < E; e += 4) *(float4*)(d0 + e) = make_float4(out[e], out[e + 1], out[e + 2], out[e + 3]);
        }
#pragma unroll
        for (int e = 0; e < E; e += 4) *(float4*)(tile + t * E + e) = make_float4(out[e], out[e + 1], out[e + 2], out[e + 3]);
    }
    __syncthreads();
    // + event embedding (row v of [V+1, (T+1)E]) ; fp32 row out, coalesced
    const size_t rbase = ((size_t)b * (V + 1) + v) * D;
    for (int i = threadIdx.x; i < D4; i += 128) {
        float4 x = *(float4*)(tile + 4 * i);
        const float4 a = *(const float4*)(event_emb + (size_t)v * D + 4 * i);
        x = make_float4(x.x + a.x, x.y + a.y, x.z + a.z, x.w + a.w);
        *(float4*)(tile + 4 * i) = x;
        *(float4*)(xe + rbase + 4 * i) = x;
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // the row's norm: wave 0
        const float rn = scalenorm_rn(RowReread(threadIdx.x, D, tile), norm_eps);
        if (threadIdx.x == 0) s_rn = rn;
    }
    __syncthreads();
    const float sc = s_rn * sqrtf((float)D) * g_norm[0];
    for (int i = threadIdx.x; i < D4; i += 128) {
        const float4 x = *(const float4*)(tile + 4 * i);
        store_row4<true>(h + rbase, i, x.x * sc, x.y * sc, x.z * sc, x.w * sc);
    }
}

}  // namespace

int medp_duett_time_embed_launch(const MedpDuettWeights* w, const float* xs_times, float* temb, int B, int T, hipStream_t s) {
    const int T1 = T + 1, tt = w->d_embedding * (w->n_vars + 1);
    const int mfma_on = embed_mfma_on();
    if (mfma_on && w->d_hidden_time <= 4 * TEM_KS) {
        time_embed_mfma_kernel<<<dim3((B * T1 + 63) / 64, (tt + TEM_CW - 1) / TEM_CW), 256, 0, s>>>(
            xs_times, (const float*)w->time_w0, (const float*)w->time_b0, (const float*)w->time_bn_scale, (const float*)w->time_bn_shift,
            (const float*)w->time_w3t, (const float*)w->time_b3, (const float*)w->rep_embedding, temb, B, T, w->d_hidden_time, tt);
    } else {
        time_embed_kernel<<<dim3((B * T1 + TE_ROWS - 1) / TE_ROWS, (tt + 255) / 256), 256, TE_ROWS * w->d_hidden_time * sizeof(float), s>>>(
            xs_times, (const float*)w->time_w0, (const float*)w->time_b0, (const float*)w->time_bn_scale, (const float*)w->time_bn_shift,
            (const float*)w->time_w3t, (const float*)w->time_b3, (const float*)w->rep_embedding, temb, B, T, w->d_hidden_time, tt);
    }
    MEDP_LAUNCH_CHECK("duett time_embed");
    return 0;
}

int medp_duett_psi_embed_launch(const MedpDuettWeights* w, const float* xs_static, const float* xs_ts, float* xe, void* h, float* psi0_out,
                                int B, int T, hipStream_t s) {
    MEDP_CHECK_ARG(w->emb_l0 && w->emb_w4t, "duett: emb_l0 / emb_w4t (transposed weight layout) missing");
    MEDP_CHECK_ARG(w->d_hidden_tab <= 256 && w->n_obs_rows >= 1 && w->n_obs_rows <= 64, "duett: tab encoder hidden size above 256 / n_obs table above 64 rows");
    const int V = w->n_vars, T1 = T + 1, E = w->d_embedding;
    const size_t lds = (size_t)T1 * E * sizeof(float);
    MEDP_CHECK_ARG(lds <= 120 * 1024, "duett: a (T+1)*E row does not fit the embed kernel's LDS tile");
    MEDP_ONCE_PER_DEVICE({
        (void)hipFuncSetAttribute((const void*)psi_embed_event_kernel<24, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    });
    const TabWeights tw{xs_static, (const float*)w->tab_w0, (const float*)w->tab_b0, (const float*)w->tab_bn_scale, (const float*)w->tab_bn_shift,
                        (const float*)w->tab_w4, (const float*)w->tab_b4, w->n_static, w->d_hidden_tab};
    psi_embed_event_kernel<24, 64><<<dim3(B, V + 1), 128, lds, s>>>(
        xs_ts, (const float*)w->emb_l0, (const float*)w->emb_w4t, (const float*)w->emb_b4, (const float*)w->n_obs_table, w->n_obs_rows, tw,
        (const float*)w->special, (const float*)w->event_embedding, (const float*)w->event_enc[0].g_attn, w->norm_eps, xe, (bf16_t*)h, psi0_out,
        B, T, V, embed_mfma_on());
    MEDP_LAUNCH_CHECK("duett psi_embed_event");
    return 0;
}

// ---- the embedding stage on its own (kernel-level parity checks and bench.py's per-kernel HBM table) ------------------------------
// stages: bit 0 = static encoder + fused psi build (writes xe_out fp32 [B,V+1,(T+1)E], h_out bf16 same shape, psi0_out optional);
//         bit 1 = time embedding (writes temb_out fp32 [B,T+1,(V+1)E]).
extern "C" int medp_duett_embed_fwd(const MedpDuettWeights* w, const float* xs_static, const float* xs_ts, const float* xs_times, int B, int T,
                                    float* xe_out, void* h_out, float* temb_out, float* psi0_out, float* tab_workspace, int stages,
                                    void* stream) {
    MEDP_CHECK_ARG(w && xs_static && xs_ts && xs_times && B > 0 && T > 0, "duett_embed_fwd: bad argument");
    MEDP_CHECK_ARG(w->d_embedding == 24 && w->d_hidden_embed == 64, "duett_embed_fwd: built for d_embedding 24 / hidden 64 (duett.py:50)");
    hipStream_t s = (hipStream_t)stream;
    if (stages & 1) {
        MEDP_CHECK_ARG(xe_out && h_out, "duett_embed_fwd: stage 1 needs xe_out and h_out");
        (void)tab_workspace;          // kept in the signature; the static encoder runs inside the fused kernel
        MEDP_TRY(medp_duett_psi_embed_launch(w, xs_static, xs_ts, xe_out, h_out, psi0_out, B, T, s));
    }
    if (stages & 2) {
        MEDP_CHECK_ARG(temb_out, "duett_embed_fwd: stage 2 needs temb_out");
        MEDP_TRY(medp_duett_time_embed_launch(w, xs_times, temb_out, B, T, s));
    }
    return 0;
}

// Debug hook (NOT part of the C ABI in include/medp_hip.h; tests/test_gpu_duett_fused.py): 1 / 0 = the fp32-MFMA / VALU forms of the
// time-embedding and psi-embedding kernels, -1 = back to the environment's choice.  Returns the previous setting.
extern "C" int medp_dbg_embed_mfma(int on) {
    const int prev = g_embed_mfma;
    g_embed_mfma = on < 0 ? -1 : (on != 0);
    return prev;
}
