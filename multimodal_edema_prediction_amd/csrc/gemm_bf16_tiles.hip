// bf16 MFMA GEMM for gfx950:  C[M,N] = epilogue( A[M,K] · W[N,K]^T )
//
// Both operands are K-contiguous (torch `nn.Linear` layout), which is the natural operand layout
// of v_mfma_f32_16x16x32_bf16: a lane's fragment is 8 consecutive k of one row (16 B).
//
// Structure (one 256-thread workgroup = 4 waves in 2x2, tile BM x BN x 64):
//   * global -> LDS by LDS-DMA (`global_load_lds_dwordx4`, 16 B per lane, no VGPR round trip),
//     double-buffered: the loads of K-tile t+1 are in flight while tile t is multiplied.
//   * LDS rows are 128 B (64 bf16); the 16-B chunk index is XOR-swizzled with (row & 7) so that the
//     ds_read_b128 fragment reads of 16 different rows are bank-conflict free.  LDS-DMA writes LDS
//     linearly (wave base + lane*16), so the swizzle is applied to the per-lane SOURCE address and
//     again on the read (both-sides-or-neither).
//   * MFMA operand roles are swapped (A-operand := W rows, B-operand := activation rows) so each
//     lane ends up with 4 consecutive output columns of one output row -> 16-B vector epilogue.
//   * Ragged M / N / K: out-of-range 16-B chunks are sourced from a zero buffer (the LDS-DMA source
//     address is per lane), so no padding convention is imposed on callers (K % 8 == 0 only).
//   * Fused epilogue: + bias[n] -> GELU(erf) -> * scale[n] (LayerScale) -> + residual[m,n] -> fp32 or bf16.
//   * blockIdx -> tile map is XCD-aware (bijective): the 8 XCDs each get a contiguous run of tiles that
//     walks N fastest, so one XCD's L2 sees one A row-panel and the whole W.
//
// This file: the 128-row-tile kernel described above, v3 (256 x 128 tiles, below), the split-K finish pass and their launchers; which
// shape takes which of them is gemm_plan's business (gemm_bf16.hip).
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_variants.h"

namespace {

__device__ __attribute__((aligned(16))) uint32_t g_zero16[4] = {0, 0, 0, 0};

struct GemmParams {
    const bf16_t* A;
    const bf16_t* W;
    void* C;
    int M, N, K, lda, ldw, ldc;
    const float* bias;
    const float* scale;
    const float* residual;
    int ldr;
    int act;
    int out_bf16;
    float* partial;     // split-K (small grids): blockIdx.y = K slice, raw fp32 partial sums go to partial[slice][M][N]
    int nsplit;
};
// the kernels of this file take the operands in their own layout: made from the front end's MedpGemmArgs here and nowhere else
GemmParams gemm_params(const MedpGemmArgs& a, float* partial, int nsplit) {
    return GemmParams{(const bf16_t*)a.A, (const bf16_t*)a.W, a.C, a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.bias, a.scale, a.residual,
                      a.ldr, a.act, a.out_bf16, partial, nsplit};
}

// TAG only gives the CXR-encoder launches their own kernel symbol, so a kernel trace separates the ViT GEMMs (the step's
// dominant kernel, 4 shapes x 12 layers) from the DuETT / fusion-head launches of the same code.
template <int BM, int BN, int TAG>
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int TM = BM / 32, TN = BN / 32;   // 16x16 tiles per wave along m / n (wave tile = BM/2 x BN/2)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;

    // ---- XCD-aware, bijective block -> tile map -----------------------------------------------
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int nwg = tiles_m * tiles_n;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int m0 = (wg / tiles_n) * BM, n0 = (wg % tiles_n) * BN;

    // split-K: slice blockIdx.y owns K-tiles [kt_begin, kt_begin + nkt)
    const int nkt_all = (p.K + 63) >> 6;
    const int per_split = (nkt_all + p.nsplit - 1) / p.nsplit;
    const int kt_begin = blockIdx.y * per_split;
    const int nkt = max(0, min(nkt_all, kt_begin + per_split) - kt_begin);
    const bf16_t* zero = (const bf16_t*)g_zero16;

    auto stage = [&](int buf, int kt) {
        char* sa = smem + buf * STAGE;
        char* sb = sa + A_BYTES;
        const int k0 = (kt_begin + kt) << 6;
#pragma unroll
        for (int i = 0; i < BM * 8 / 256; ++i) {
            const int qd = i * 256 + tid;
            const int row = qd >> 3, c = (qd & 7) ^ (row & 7);
            const int gr = m0 + row, gk = k0 + c * 8;
            const bf16_t* src = (gr < p.M && gk < p.K) ? p.A + (size_t)gr * p.lda + gk : zero;
            glds16(src, sa + (i * 256 + wave * 64) * 16);
        }
#pragma unroll
        for (int i = 0; i < BN * 8 / 256; ++i) {
            const int qd = i * 256 + tid;
            const int row = qd >> 3, c = (qd & 7) ^ (row & 7);
            const int gr = n0 + row, gk = k0 + c * 8;
            const bf16_t* src = (gr < p.N && gk < p.K) ? p.W + (size_t)gr * p.ldw + gk : zero;
            glds16(src, sb + (i * 256 + wave * 64) * 16);
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (nkt > 0) stage(0, 0);
    MEDP_WAIT_LDS_DMA();
    __syncthreads();   // tile 0 landed (explicit wait) before any wave reads it

    const int a_row0 = wr * (BM / 2) + fr, b_row0 = wc * (BN / 2) + fr;
    const int sw = fr & 7;   // (row & 7): every row base is a multiple of 16

    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) stage(cur ^ 1, kt + 1);
        const char* sa = smem + cur * STAGE;
        const char* sb = sa + A_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int coff = ((s * 4 + kq) ^ sw) << 4;
            bf16x8 xa[TM], wb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) xa[i] = *(const bf16x8*)(sa + (a_row0 + i * 16) * 128 + coff);
#pragma unroll
            for (int j = 0; j < TN; ++j) wb[j] = *(const bf16x8*)(sb + (b_row0 + j * 16) * 128 + coff);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xa[i], acc[i][j], 0, 0, 0);
        }
        MEDP_WAIT_LDS_DMA();   // tile kt+1 (issued at the top of this iteration) has landed
        __syncthreads();
    }

    // ---- epilogue: lane holds C[m][n..n+3],  m = tile row (lane&15),  n = 4*(lane>>4) ----------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wr * (BM / 2) + i * 16 + fr;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wc * (BN / 2) + j * 16 + kq * 4;
            if (n >= p.N) continue;
            f32x4 v = acc[i][j];
            if (p.partial) {          // split-K: raw partial sums; bias / activation / residual happen in splitk_finish_kernel
                *(f32x4*)(p.partial + ((size_t)blockIdx.y * p.M + m) * p.N + n) = v;
                continue;
            }
            gemm_store4(p.C, p.ldc, p.out_bf16, m, n, gemm_epi_tested(v, p.bias, p.scale, p.residual, p.ldr, p.act, m, n));
        }
    }
}


// ------------------------------------------------------------------------------------------------------------------
// v3: the LDS-traffic fix.  v1 gives each wave a 64x64 output tile: 32 flop per LDS byte read, and the LDS (fragment
// reads + LDS-DMA fills) is as busy as the matrix pipe.  v3 gives each wave 128 x 64 (8 x 4 MFMA tiles, 128 accumulator
// VGPRs): 43 flop per LDS byte, 12 ds_read_b128 per 32 MFMAs.
//   block 256 x 128, 4 waves (2 x 2), BK = 32 (64-B LDS rows), THREE 24-KiB slots (72 KiB -> 2 blocks per CU),
//   LDS-DMA two K-tiles ahead, one raw s_barrier per K-tile and a COUNTED s_waitcnt vmcnt (never 0 in the loop), so the loads of
//   tiles t+1 / t+2 stay in flight across the barrier while tile t is multiplied.
//   64-B rows: chunk' = chunk ^ (((row >> 2) & 1) << 1) makes every ds_read_b128 lane group hit 16 distinct 16-B slots.
template <int TAG>
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_v3_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 256, BN = 128;
    constexpr int A_BYTES = BM * 64, B_BYTES = BN * 64, STAGE = A_BYTES + B_BYTES;   // 24 KiB

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;

    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int nwg = tiles_m * tiles_n;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    // L2-aware linearisation: an XCD's contiguous run of ~nwg/8 ids walks one BAND of 8 row-tiles in SUPER-COLUMNS of 8
    // column-tiles, so the 64 tiles it runs concurrently (2 per CU x 32 CUs) share 8 A panels and 8 W panels (~4.7 MB at
    // K = 768) instead of 3 A panels and ALL of W (PMC: 2.4x the algorithmic fetch with the row-major order).
    constexpr int MB = 8, SN = 8;
    const int band = wg / (MB * tiles_n), rb = wg % (MB * tiles_n);
    const int mb = min(MB, tiles_m - band * MB);
    const int sc = rb / (mb * SN), r2 = rb % (mb * SN);
    const int sn = min(SN, tiles_n - sc * SN);
    const int m0 = (band * MB + r2 / sn) * BM, n0 = (sc * SN + r2 % sn) * BN;
    const int nkt = (p.K + 31) >> 5;
    const bf16_t* zero = (const bf16_t*)g_zero16;

    // one 1-KiB LDS-DMA piece per call: pieces 0..3 = A rows, 4..5 = W rows of K-tile kt
    auto stage_piece = [&](int slot, int kt, int piece) {
        char* sa = smem + slot * STAGE;
        const int k0 = kt << 5;
        if (piece < 4) {
            const int qd = piece * 256 + tid;
            const int row = qd >> 2, c = (qd & 3) ^ (((row >> 2) & 1) << 1);
            const int gr = m0 + row, gk = k0 + c * 8;
            const bf16_t* src = (gr < p.M && gk < p.K) ? p.A + (size_t)gr * p.lda + gk : zero;
            glds16(src, sa + (piece * 256 + wave * 64) * 16);
        } else {
            const int qd = (piece - 4) * 256 + tid;
            const int row = qd >> 2, c = (qd & 3) ^ (((row >> 2) & 1) << 1);
            const int gr = n0 + row, gk = k0 + c * 8;
            const bf16_t* src = (gr < p.N && gk < p.K) ? p.W + (size_t)gr * p.ldw + gk : zero;
            glds16(src, sa + A_BYTES + ((piece - 4) * 256 + wave * 64) * 16);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int pc = 0; pc < 6; ++pc) stage_piece(0, 0, pc);
    // tiles past the end of K are sourced from the zero chunk (bounds check in stage_piece), so the prefetch is issued
    // unconditionally: no branch in the loop body, one basic block, and the wait is always vmcnt(6)
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) stage_piece(1, 1, pc);

    const int coff = (kq ^ (((fr >> 2) & 1) << 1)) << 4;
    const int a_off = (wm * 128 + fr) * 64 + coff, b_off = (wn * 64 + fr) * 64 + coff;
    int slot = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const char* sa = smem + slot * STAGE + a_off;
        const char* sb = smem + slot * STAGE + A_BYTES + b_off;
        const int nslot = slot == 0 ? 2 : slot - 1;
        bf16x8 xa[8], wb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wb[j] = *(const bf16x8*)(sb + j * 16 * 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) xa[i] = *(const bf16x8*)(sa + i * 16 * 64);
        // MFMA rows in fragment-arrival order; the next-next tile's six LDS-DMA pieces are issued between the MFMA groups
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xa[i], acc[i][j], 0, 0, 0);
            if (i < 6) stage_piece(nslot, kt + 2, i);
        }
        // shape the schedule: 6 fragment reads up front, then one more read behind every group of 4 MFMAs, so each MFMA group
        // waits (counted lgkmcnt) only for the fragments it consumes instead of for all 12 reads
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        slot = slot == 2 ? 0 : slot + 1;
    }

    // ---- epilogue through LDS: every global access is a whole 256-B (fp32) / 128-B (bf16) row segment ----------------
    // Each wave owns a private [64][68] fp32 patch (17 KiB); two passes cover its 128 rows.  Accumulator layout (lane =
    // output row, 4 consecutive columns) would store 32-B pieces of 16 different rows per instruction; after the LDS
    // transpose a wave instruction covers 4 full rows, and bias / LayerScale / residual loads are coalesced too.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the trailing (zero-sourced) prefetches must land before LDS is reused
    __syncthreads();                                   // last slot fully consumed by every wave, no LDS-DMA in flight
    float* wl = (float*)(smem + wave * (64 * 68 * 4));
    const int er = lane >> 4, ec = (lane & 15) * 4;
    const int n = n0 + wn * 64 + ec;
    f32x4 bias4 = (f32x4){0.f, 0.f, 0.f, 0.f}, scale4 = (f32x4){1.f, 1.f, 1.f, 1.f};
    if (n < p.N) {
        if (p.bias) bias4 = *(const f32x4*)(p.bias + n);
        if (p.scale) scale4 = *(const f32x4*)(p.scale + n);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
            for (int j = 0; j < 4; ++j) *(f32x4*)(wl + (i4 * 16 + fr) * 68 + j * 16 + kq * 4) = acc[half * 4 + i4][j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            const int rr = it * 4 + er;
            const int m = m0 + wm * 128 + half * 64 + rr;
            f32x4 v = *(const f32x4*)(wl + rr * 68 + ec);
            if (m < p.M && n < p.N) {
                v = gemm_epi_preloaded<false>(v, bias4, scale4, p.act, p.out_bf16);
                if (p.residual) v += *(const f32x4*)(p.residual + (size_t)m * p.ldr + n);
                gemm_store4(p.C, p.ldc, p.out_bf16, m, n, v);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// split-K second pass: C = epi(sum_s partial[s]) — the slices are summed in ascending order (deterministic), then the same
// epilogue as the one-pass kernel
__global__ __launch_bounds__(256) void splitk_finish_kernel(const GemmParams p) {
    const int n4 = p.N >> 2;
    const size_t total = (size_t)p.M * n4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / n4), n = (int)(i % n4) * 4;
        f32x4 v = *(const f32x4*)(p.partial + (size_t)m * p.N + n);
        for (int s = 1; s < p.nsplit; ++s) v += *(const f32x4*)(p.partial + ((size_t)s * p.M + m) * p.N + n);
        // gemm_epi_tested written out: through the function the compiler inverts one branch of this loop
        if (p.bias) v += *(const f32x4*)(p.bias + n);
        if (p.act == 1) v = gelu_erf4(v);
        if (p.scale) v *= *(const f32x4*)(p.scale + n);
        if (p.residual) v += *(const f32x4*)(p.residual + (size_t)m * p.ldr + n);
        gemm_store4(p.C, p.ldc, p.out_bf16, m, n, v);
    }
}

template <int TAG>
int launch_v3(const GemmParams& p, hipStream_t stream) {
    const int tiles = ((p.M + 255) / 256) * ((p.N + 127) / 128);
    constexpr int LDS = 3 * (256 + 128) * 64;
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)gemm_bf16_nt_v3_kernel<TAG>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    });
    gemm_bf16_nt_v3_kernel<TAG><<<tiles, 256, LDS, stream>>>(p);
    MEDP_LAUNCH_CHECK("medp_gemm_bf16_nt(v3)");
    return 0;
}

template <int BM, int BN, int TAG>
int launch(const GemmParams& p, hipStream_t stream) {
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    constexpr int LDS = 2 * (BM + BN) * 128;
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)gemm_bf16_nt_kernel<BM, BN, TAG>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    });
    gemm_bf16_nt_kernel<BM, BN, TAG><<<dim3(tiles, p.nsplit), 256, LDS, stream>>>(p);
    MEDP_LAUNCH_CHECK("medp_gemm_bf16_nt");
    if (p.partial) {
        const size_t items = (size_t)p.M * (p.N >> 2);
        splitk_finish_kernel<<<(int)min((size_t)2048, (items + 255) / 256), 256, 0, stream>>>(p);
        MEDP_LAUNCH_CHECK("medp_gemm_bf16_nt(split-K finish)");
    }
    return 0;
}

}  // namespace

int medp_gemm_tile128_launch(const MedpGemmArgs& a, int bn, int tag, float* partial, int nsplit, void* stream) {
    const GemmParams p = gemm_params(a, partial, nsplit);
    hipStream_t s = (hipStream_t)stream;
    if (bn == 64) return launch<128, 64, 0>(p, s);
    return tag == 1 ? launch<128, 128, 1>(p, s) : launch<128, 128, 0>(p, s);
}

int medp_gemm_v3_launch(const MedpGemmArgs& a, int tag, void* stream) {
    const GemmParams p = gemm_params(a, nullptr, 1);
    return tag == 1 ? launch_v3<1>(p, (hipStream_t)stream) : launch_v3<0>(p, (hipStream_t)stream);
}
