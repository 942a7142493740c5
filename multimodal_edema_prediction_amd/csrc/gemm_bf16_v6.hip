// v6: the 256 x 256 x 64 ping-pong K-loop of gemm_tile256.h (tile map, phase plan and counted waits are described there), ONE tile
// per workgroup, for every epilogue: bias / GELU / LayerScale / fp32 residual, fp32 or bf16 result.
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_tile256.h"
#include "gemm_variants.h"

namespace {

constexpr int LDS_MAIN = 2 * KBUF, LDS_EPI = 8 * 64 * 68 * 4;
constexpr int LDS_BYTES = LDS_EPI > LDS_MAIN ? LDS_EPI : LDS_MAIN;
static_assert(LDS_BYTES >= LDS_MAIN && LDS_BYTES <= 160 * 1024, "v6 LDS plan");

// GR = tile rows per ping-pong group: 128 (256 x 256 tiles) or 112 (224 x 256 tiles for the N = 768 launches, see launch_v6).
// With GR = 112 the LDS layout, the DMA piece plan and therefore every vmcnt count stay those of GR = 128: a group's A half
// still holds 128 rows, rows 112-127 are staged from the zero chunk, and the wave's last 16-row block (i = 3 of a = 1)
// does no MFMA.  Every output element sees the same MFMAs in the same K order under either GR.
// BUF: the A / W stream goes through buffer descriptors (K % 64 == 0, see launch_v6_gr); without it every lane builds its
// own address and selects the zero chunk for what lies past M, N or K.  Same pieces in the same order either way.
template <int TAG, int GR, bool BUF>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_v6_kernel(const MedpGemmArgs p) {
    static_assert(GR == 128 || GR == 112, "v6 group rows");
    constexpr int BM = 2 * GR;
    constexpr int NI1 = (GR - 64) / 16;                // 16-row blocks of the wave's second 64-row quadrant (a = 1)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;          // wm = ping-pong group
    const bf16_t* A = (const bf16_t*)p.A;
    const bf16_t* W = (const bf16_t*)p.W;
    const bf16_t* zero = (const bf16_t*)g_zero16_t256;
    MEDP_PROF_ENTER(p.prof, p.prof_flags);

    const Tile256Map map(p.M, p.N, BM);
    const int bid = blockIdx.x;                 // workgroup b owns tile b
    int m0, n0;
    map.origin(bid, 8, 4, BM, m0, n0);          // bands of 8 row-tiles x super-columns of 4 column-tiles = one round of an XCD's 32 CUs
    const int nkt = (p.K + 63) >> 6;

    // ---- LDS-DMA staging: half-tile = 128 rows x 8 chunks; lane's two pieces are rows (tid>>3) and (tid>>3)+64 ------
    const int srow = tid >> 3, schunk = (tid & 7) ^ (srow & 7);       // source chunk for LDS position (tid & 7)
    const bf16_t* a_src[2][2];                                        // [half][piece] row base (k = 0) or nullptr
    const bf16_t* w_src[2][2];
    // BUF: one descriptor in SGPRs per piece position (base = its first row, num_records = its rows below M / N in bytes: at most
    // 64, 48 for rows 64-111 of a 112-row group, whose rows 112-127 nobody reads) and one byte offset per operand and lane, as
    // in gemm_bf16_v7.hip; the K advance is the scalar offset.  (readfirstlane: see there.)
    const unsigned voff_a = ((unsigned)srow * (unsigned)p.lda + (unsigned)(schunk * 8)) * 2u;
    const unsigned voff_w = ((unsigned)srow * (unsigned)p.ldw + (unsigned)(schunk * 8)) * 2u;
    medp_rsrc_t ra[2][2], rw[2][2];
    const medp_rsrc_t none_rsrc = lds_dma_rsrc(A, 0);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (BUF) {
                const int ra0 = m0 + h * GR + j * 64, rw0 = n0 + h * 128 + j * 64;
                const int na = min(j == 0 ? 64 : GR - 64, max(0, p.M - ra0)), nw = min(64, max(0, p.N - rw0));
                ra[h][j] = lds_dma_rsrc(A + (size_t)ra0 * (size_t)p.lda, (unsigned)__builtin_amdgcn_readfirstlane(na * p.lda * 2));
                rw[h][j] = lds_dma_rsrc(W + (size_t)rw0 * (size_t)p.ldw, (unsigned)__builtin_amdgcn_readfirstlane(nw * p.ldw * 2));
            } else {
                const int ra = m0 + h * GR + j * 64 + srow, rw = n0 + h * 128 + j * 64 + srow;
                a_src[h][j] = ((GR == 128 || j * 64 + srow < GR) && ra < p.M) ? A + (size_t)ra * p.lda + schunk * 8 : nullptr;
                w_src[h][j] = rw < p.N ? W + (size_t)rw * p.ldw + schunk * 8 : nullptr;
            }
        }
    // piece j (rows 64 j .. 64 j + 63) of half-tile `which` (0: A rows 0-127, 1: A rows 128-255, 2: W rows 0-127, 3: W rows
    // 128-255) of K-tile kt -> buffer kt & 1; past K (the tail of the stream) the source is the zero chunk (BUF: a descriptor
    // without records: nothing is read), counts stay uniform
    auto stage_piece = [&](int kt, int which, int j) {
        char* dst = piece_dst(smem, kt & 1, which, wave, j);
        const int k0 = kt * 64;
        if constexpr (BUF) {
            const bool past = kt >= nkt;
            const medp_rsrc_t live = which < 2 ? ra[which & 1][j] : rw[which & 1][j];
            blds16(past ? none_rsrc : live, which < 2 ? voff_a : voff_w, past ? 0u : (unsigned)k0 * 2u, dst);
        } else {
            const bool kin = k0 + schunk * 8 < p.K;
            const bf16_t* base = which < 2 ? a_src[which & 1][j] : w_src[which & 1][j];
            glds16((base != nullptr && kin) ? base + k0 : zero, dst);
        }
    };
    auto stage_a = [&](int kt, int j) { stage_piece(kt, 0, j); stage_piece(kt, 1, j); };
    auto stage_w = [&](int kt, int h) { stage_piece(kt, 2 + h, 0); stage_piece(kt, 2 + h, 1); };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue: K-tiles 0 and 1, in the order of the steady-state stream (gemm_tile256.h)
    stage_a(0, 0); stage_w(0, 0); stage_w(0, 1); stage_a(0, 1);
    stage_a(1, 0); stage_w(1, 0); stage_w(1, 1);           // (A rows 64-127 of K-tile 1 follow in P1 of K-tile 0)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");       // A rows 0-63 and W of K-tile 0

    // fragment read addresses: row = base + 16*i + fr, chunk (kh*4 + kq) ^ (row & 7); row & 7 == fr & 7 (bases are multiples of 16)
    const int sw = fr & 7;
    const int fa_off = wm * HALF + fr * 128;                          // + a*64 rows*128 + i*16*128 ; chunk term added per kh
    const int fw_off = 2 * HALF + (wn >> 1) * HALF + ((wn & 1) * 64 + fr) * 128;
    const int ch0 = ((0 + kq) ^ sw) << 4, ch1 = ((4 + kq) ^ sw) << 4;

    bf16x8 fa[4][2], fw0a[2][2], fw0b[2][2], fw1[2][2];      // two W0 sets: K-tile t+1's is read while K-tile t's still multiplies
    auto read_a = [&](const char* buf, int a) {
#pragma unroll
        for (int i = 0; i < (a == 0 ? 4 : NI1); ++i) {
            const char* rp = buf + fa_off + (a * 64 + i * 16) * 128;
            fa[i][0] = *(const bf16x8*)(rp + ch0);
            fa[i][1] = *(const bf16x8*)(rp + ch1);
        }
    };
    auto read_w = [&](const char* buf, int b, bf16x8 (*fw)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* rp = buf + fw_off + (b * 32 + j * 16) * 128;
            fw[j][0] = *(const bf16x8*)(rp + ch0);
            fw[j][1] = *(const bf16x8*)(rp + ch1);
        }
    };
    // ragged last row-tile (M = 64 * 257 leaves 64 valid rows of 256): a 64-row quadrant entirely past M keeps its zero
    // accumulators and skips its MFMAs (wave-uniform), so that tile costs its loads and barriers only
    const bool rows_live[2] = {m0 + wm * GR < p.M, m0 + wm * GR + 64 < p.M};
    auto mma = [&](int a, int b, const bf16x8 (*fw)[2]) {
        if (!rows_live[a]) return;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int i = 0; i < (a == 0 ? 4 : NI1); ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[a * 4 + i][b * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j][kh], fa[i][kh], acc[a * 4 + i][b * 2 + j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };

    MEDP_BAR();                    // K-tile 0 (A rows 0-63, W) visible to everyone
    read_w(smem, 0, fw0a);
    if (wm == 1) MEDP_BAR();       // group 1 runs one barrier behind (group 0 pays its extra barrier after the loop)

    auto none = [](int) {};
    auto ktile = [&](int kt, const bf16x8 (*fw0)[2], bf16x8 (*fw0n)[2]) {
        tile256_ktile<false>(smem, kt, fw0, fw0n, fw1, read_a, read_w, mma, stage_a, stage_w, none, none);
    };
    for (int kt = 0; kt < nkt; kt += 2) {
        ktile(kt, fw0a, fw0b);
        if (kt + 1 < nkt) ktile(kt + 1, fw0b, fw0a);
    }
    if (wm == 0) MEDP_BAR();

    // ---- epilogue through LDS (whole-row coalesced global accesses), as v3 ------------------------------------------
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float* wl = (float*)(smem + wave * (64 * 68 * 4));
    const int er = lane >> 4, ec = (lane & 15) * 4;
    const int n = n0 + wn * 64 + ec;
    f32x4 bias4 = (f32x4){0.f, 0.f, 0.f, 0.f}, scale4 = (f32x4){1.f, 1.f, 1.f, 1.f};
    if (n < p.N) {
        if (p.bias) bias4 = *(const f32x4*)(p.bias + n);
        if (p.scale) scale4 = *(const f32x4*)(p.scale + n);
    }
    // The fp32 residual tile (proj / fc2: 256 KiB per workgroup) is fetched into registers BEFORE the accumulators go through
    // LDS — 16 independent 16-B loads per lane and half, all in flight at once (the fragment registers are free now).  Loading
    // it inside the store loop made the epilogue a chain of exposed HBM round trips: 40 us of the 61-us proj GEMM.
    f32x4 res[2][16];
    auto load_res = [&](int half) {
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int m = m0 + wm * GR + half * 64 + it * 4 + er;
            res[half][it] = (half * 64 + it * 4 < GR && m < p.M && n < p.N) ? *(const f32x4*)(p.residual + (size_t)m * p.ldr + n) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    const bool has_res = p.residual != nullptr;
    if (has_res) load_res(0);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
            for (int j = 0; j < 4; ++j) *(f32x4*)(wl + (i4 * 16 + fr) * 68 + j * 16 + kq * 4) = acc[half * 4 + i4][j];
        MEDP_WAVE_LDS_SYNC();
        if (half == 0 && has_res) load_res(1);      // second half's residual flies while the first half is stored
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            if (half * 64 + it * 4 >= GR) continue;   // (compile time) rows of the next tile
            const int rr = it * 4 + er;
            const int m = m0 + wm * GR + half * 64 + rr;
            f32x4 v = *(const f32x4*)(wl + rr * 68 + ec);
            if (m < p.M && n < p.N) {
                v += bias4;
                v = gemm_act_scale<true>(v, scale4, p.act, p.out_bf16);
                if (has_res) v += res[half][it];
                gemm_store4<true>(p.C, p.ldc, p.out_bf16, m, n, v);      // non-temporal
            }
        }
        MEDP_WAVE_LDS_SYNC();
    }
    MEDP_PROF_LEAVE(p.prof, p.prof_flags);
}

template <int TAG, int GR, bool BUF>
int launch_v6_buf(const MedpGemmArgs& a, hipStream_t stream) {
    constexpr int BM = 2 * GR;
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    MEDP_ONCE_PER_DEVICE({
        hipFuncSetAttribute((const void*)gemm_bf16_nt_v6_kernel<TAG, GR, BUF>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    });
    gemm_bf16_nt_v6_kernel<TAG, GR, BUF><<<tiles, 512, LDS_BYTES, stream>>>(a);
    MEDP_LAUNCH_CHECK("medp_gemm_bf16_nt(v6)");
    return 0;
}

// The buffer-descriptor stream needs whole K-tiles (no chunk past K inside a K-tile: only the per-lane path can zero those) and
// 64 rows of a piece within a descriptor's 32-bit num_records; everything else keeps the per-lane addresses.
template <int TAG, int GR>
int launch_v6_gr(const MedpGemmArgs& a, hipStream_t stream) {
    const bool buf = a.K % 64 == 0 && a.lda < (1 << 24) && a.ldw < (1 << 24);
    return buf ? launch_v6_buf<TAG, GR, true>(a, stream) : launch_v6_buf<TAG, GR, false>(a, stream);
}

// 224 x 256 tiles (GR = 112) for N = 768 where 256 x 256 tiles leave part of the chip idle: proj / fc2 at M = 64 x 257 are
// 65 x 3 = 195 tiles of 256 rows on 256 CUs, 74 x 3 = 222 of 224 rows.  Taken for the launches with a residual (proj / fc2)
// only.  MEDP_V6_N768=0: always 256 x 256 (A/B runs); 2: also the N = 768 launches without a residual.
bool v6_use_224(const MedpGemmArgs& a) {
    static const int mode = medp_env_int("MEDP_V6_N768", 1);
    const int tiles256 = ((a.M + 255) / 256) * ((a.N + 255) / 256);
    const int tiles224 = ((a.M + 223) / 224) * ((a.N + 255) / 256);
    return mode != 0 && a.N == 768 && (a.residual != nullptr || mode == 2) && tiles256 < 256 && tiles224 <= 256;
}

}  // namespace

int medp_gemm_v6_launch(const MedpGemmArgs& a, int tag, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (v6_use_224(a)) return tag == 1 ? launch_v6_gr<1, 112>(a, s) : launch_v6_gr<0, 112>(a, s);
    return tag == 1 ? launch_v6_gr<1, 128>(a, s) : launch_v6_gr<0, 128>(a, s);
}
