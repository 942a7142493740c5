// v7: the 256 x 256 x 64 ping-pong K-loop of gemm_tile256.h (the one gemm_bf16_v6.hip runs once per workgroup) made PERSISTENT for grids of
// more than one round of workgroups with a bf16 result and no residual (qkv: 585 tiles, fc1: 780 tiles on 256 CUs).
//
// 256 workgroups (MEDP_V7_WGS) stay resident and walk the tile list:
//   * the LDS-DMA stream never stops: from K-tile nkt-2 on it carries K-tiles 0 and 1 of the NEXT tile (all but the last A
//     piece, which P1 of the next K-tile 0 issues as in the steady state) — the next K-loop starts two K-tiles deep;
//   * the epilogue needs no K buffer: bias / GELU / bf16 pack happen on the accumulator layout, the transposition to whole
//     128-B rows goes through a 16-row bf16 patch per wave behind the K buffers, the bias slice arrives by LDS-DMA.  A FULL tile
//     runs a straight line per activation with the patch chain software-pipelined (row block i+1 is packed while row block i's
//     two patch reads are in flight; no bounds test), a clipped tile the serial chain with a test per store: 2.4 -> 1.6 us per
//     tile for qkv, 5.8 -> 4.7 us for fc1 (profiles/r07_gemm_v7_epilogue.txt);
//   * nothing waits for the output stores until P2 of the next K-tile 1 (vmcnt is in order: the wait that ends the epilogue is
//     counted so that it stops just before the 16 stores of a full tile — both epilogue forms issue exactly 16 per wave, in the
//     same row order — and there is no register-returning load anywhere in the steady state whose wait the compiler would have
//     to place).
// What it bought (tools/trace_gemm_v7.py): the tile walk itself ~2 % on qkv / fc1 and 24 % fewer L2 misses;
// dispatch, first-tile latency and the store drain turned out NOT to be what a round of workgroups pays for — the K-loop is
// bound by L2 -> LDS delivery (L2 channels 79 % busy).
// Tiles: workgroup b takes tile b first (static, so a workgroup that becomes resident late still has work that nobody else
// does) and then draws tickets from the queue of ITS XCD (b % 8): ticket i is tile 256 + 8 i + b % 8, i.e. exactly the tile
// the hardware dispatcher would have sent to that XCD in v6, so the band x super-column L2 locality of the v6 map holds.
// A workgroup that draws a ticket past the end leaves; the last one to leave zeroes the tickets for the next launch.
// The ticket block is private to one launch (host side: a ring for eager launches, never-reused slots under stream capture).
#include <string.h>

#include <atomic>
#include <type_traits>

#include "common.h"
#include "gemm_tile256.h"
#include "gemm_variants.h"

namespace {

constexpr int SLOT_WORDS = 16;                    // 8 per-XCD ticket counters, 1 exit counter, padding (64 B)
constexpr int RING_SLOTS = 1024, CAPTURE_SLOTS = 15360;
__device__ unsigned g_v7_slots[(RING_SLOTS + CAPTURE_SLOTS) * SLOT_WORDS];   // zero at module load, self-resetting

constexpr int BM = 256;
constexpr int PROW = 144;                                              // bytes per patch row: 64 bf16 + 16 B pad (b128 reads stay aligned)
constexpr int PATCH = 16 * PROW;                                       // one wave's 16 x 64 bf16 patch
constexpr int MAILBOX = 2 * KBUF + 8 * PATCH;                          // the next tile index, written by wave 0
constexpr int BIASBUF = MAILBOX + 256;                                 // 2 x 256 floats: bias slice of this / the next tile
constexpr int TRACEBUF = BIASBUF + 2048;                               // debug timeline (medp_dbg_gemm_v7_trace): 8 tiles x 5 x u64
constexpr int LDS_BYTES = TRACEBUF + 512;
static_assert(LDS_BYTES <= 160 * 1024, "K buffers + patches + mailbox exceed the LDS");
constexpr int NWG = 256;                                               // resident workgroups = CUs of an MI355X

// -DMEDP_V7_PHASE_TRACE (tools/build_trace_lib.sh, a separate library): every wave sums, per K-tile phase, the clock ticks
// of {load section, wait at its barrier, MFMA issue, wait at its barrier}; dumped behind the tile timeline.
#ifdef MEDP_V7_PHASE_TRACE
#define PT(k)                                                          \
    do {                                                               \
        const unsigned now_ = (unsigned)__builtin_readcyclecounter();  \
        pt_acc[k] += now_ - pt_last;                                   \
        pt_last = now_;                                                \
    } while (0)
#else
#define PT(k) do { } while (0)
#endif

template <int TAG>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_v7_kernel(const MedpGemmArgs p, unsigned* slot, unsigned long long* trace, const int MB, const int SN) {
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
    const int ntiles = map.tiles_m * map.tiles_n;
    const int nkt = p.K >> 6;                          // host guarantees K % 128 == 0 and K >= 256: nkt even, >= 4
    const int xcd = blockIdx.x & 7;

    int m0, n0;
    map.origin(blockIdx.x, MB, SN, BM, m0, n0);

    // ---- LDS-DMA staging: half-tile = 128 rows x 8 chunks; lane's two pieces are rows (tid>>3) and (tid>>3)+64 ------
    const int srow = tid >> 3, schunk = (tid & 7) ^ (srow & 7);       // source chunk for LDS position (tid & 7)
    // Source state: TWO buffer descriptors in SGPRs, one per operand, for the tile the A / W stream currently reads from (base = the
    // tile's first row, num_records = the bytes of its rows below M / N, at most 256 rows), rebuilt with scalar operations where the
    // stream switches to the next tile near the end of a K-loop (nobody, i.e. no next tile: no records), and ONE loop-invariant byte
    // offset per operand and lane (row tid >> 3 of a 64-row piece).  Which piece and which K-tile is the instruction's scalar
    // offset: q * 64 * ld * 2 + k0 * 2, wave-uniform, scalar ALU only.  A load section therefore holds no address arithmetic on
    // the vector ALU (it used to build a 64-bit address and select the zero chunk per piece, ~15 VALU per section, issued beside the
    // partner wave's prioritised MFMAs), and rows past M / N are dropped by the range check, in which the scalar offset takes part:
    // gemm_tile256.h says why that is exact and why whatever LDS then holds is harmless.  (One descriptor per 64-row piece position,
    // as gemm_bf16_v6.hip keeps them, is 32 SGPRs across the K-loop: the compiler then spilled 57 SGPRs to VGPR lanes around it.)
    const unsigned voff_a = ((unsigned)srow * (unsigned)p.lda + (unsigned)(schunk * 8)) * 2u;
    const unsigned voff_w = ((unsigned)srow * (unsigned)p.ldw + (unsigned)(schunk * 8)) * 2u;
    const unsigned piece_a = (unsigned)p.lda * 128u, piece_w = (unsigned)p.ldw * 128u;       // 64 rows in bytes
    medp_rsrc_t ra, rw;
    // (readfirstlane: the clamp of a wave-uniform value is still selected as one vector instruction (v_med3), and a descriptor word
    //  in a VGPR wraps every load that uses it in a loop over its distinct values)
    auto set_m = [&](int mm) {         // mm < 0: nobody
        const int rows = mm < 0 ? 0 : min(BM, max(0, p.M - mm));
        ra = lds_dma_rsrc(A + (size_t)(mm < 0 ? 0 : mm) * (size_t)p.lda, (unsigned)__builtin_amdgcn_readfirstlane(rows * p.lda) * 2u);
    };
    auto set_n = [&](int nn) {
        const int rows = nn < 0 ? 0 : min(BN, max(0, p.N - nn));
        rw = lds_dma_rsrc(W + (size_t)(nn < 0 ? 0 : nn) * (size_t)p.ldw, (unsigned)__builtin_amdgcn_readfirstlane(rows * p.ldw) * 2u);
    };
    set_m(m0);
    set_n(n0);
#ifdef MEDP_V7_ABLATE_LOADS
    bool ablate_on = false;          // the prologue still loads (the first tile's waits count what it issued)
#endif
    // piece j (rows 64 j .. 64 j + 63) of half-tile `which` (0: A rows 0-127, 1: A rows 128-255, 2: W rows 0-127, 3: W rows
    // 128-255) of the K-tile at element offset k0 of the CURRENT source tile -> K buffer `b`
    auto stage_piece = [&](int k0, int b, int which, int j) {
#ifdef MEDP_V7_ABLATE_LOADS      // timing-only build (tools/ablate_gemm_v7.py): the K-loop without its staging stream (wrong results)
        if (ablate_on) return;
#endif
        char* dst = piece_dst(smem, b, which, wave, j);
        const int q = (which & 1) * 2 + j;
        if (which < 2) blds16(ra, voff_a, (unsigned)q * piece_a + (unsigned)k0 * 2u, dst);      // (K % 128 == 0: no chunk lies past K)
        else blds16(rw, voff_w, (unsigned)q * piece_w + (unsigned)k0 * 2u, dst);
    };
    auto stage_a = [&](int k0, int b, int j) { stage_piece(k0, b, 0, j); stage_piece(k0, b, 1, j); };
    auto stage_w = [&](int k0, int b, int h) { stage_piece(k0, b, 2 + h, 0); stage_piece(k0, b, 2 + h, 1); };
    typedef __attribute__((address_space(3))) volatile int lds_int;
    lds_int* mailbox = (lds_int*)(__attribute__((address_space(3))) char*)(smem + MAILBOX);
    // debug timeline: wave 0 stamps the 100-MHz wall clock into LDS at four points of every tile; dumped at exit
    typedef __attribute__((address_space(3))) volatile unsigned long long lds_u64;
    lds_u64* tbuf = (lds_u64*)(__attribute__((address_space(3))) char*)(smem + TRACEBUF);
    int tcount = 0;
    auto stamp = [&](int k, long long tile) {
        if (trace && wave == 0 && tcount < 8) {
            if (k == 0) tbuf[tcount * 5] = (unsigned long long)tile;
            tbuf[tcount * 5 + 1 + k] = wall_clock64();
        }
    };

    f32x4 acc[8][4];

    // fragment read addresses: row = base + 16*i + fr, chunk (kh*4 + kq) ^ (row & 7); row & 7 == fr & 7 (bases are multiples of 16)
    const int sw = fr & 7;
    const int fa_off = wm * HALF + fr * 128;
    const int fw_off = 2 * HALF + (wn >> 1) * HALF + ((wn & 1) * 64 + fr) * 128;
    const int ch0 = ((0 + kq) ^ sw) << 4, ch1 = ((4 + kq) ^ sw) << 4;

    bf16x8 fa[4][2], fw0a[2][2], fw0b[2][2], fw1[2][2];      // two W0 sets: K-tile t+1's is read while K-tile t's still multiplies
    auto read_a = [&](const char* buf, int a) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
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
    bool rows_live[2];
    auto mma = [&](int a, int b, const bf16x8 (*fw)[2]) {
        if (!rows_live[a]) return;
#ifdef MEDP_V7_ABLATE_MFMA       // timing-only build: fragment reads kept alive, no matrix instructions (wrong results)
#pragma unroll
        for (int i = 0; i < 4; ++i) { asm volatile("" ::"v"(fa[i][0]), "v"(fa[i][1])); }
#pragma unroll
        for (int j = 0; j < 2; ++j) { asm volatile("" ::"v"(fw[j][0]), "v"(fw[j][1])); }
        return;
#endif
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[a * 4 + i][b * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j][kh], fa[i][kh], acc[a * 4 + i][b * 2 + j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };

    // ticket for the tile after the one in hand; the result is parked in LDS (wave 0) and read at K-tile nkt-2 of the next
    // K-loop.  Inline asm: the compiler would wait for the returned value where it is drawn.
    unsigned ticket = 0;
    auto draw_ticket = [&]() {
        if (tid == 0) {
            const unsigned one = 1;
            asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=&v"(ticket) : "v"(slot + xcd), "v"(one) : "memory");
        }
    };
    auto post_ticket = [&]() {
        if (wave == 0) {
            const int tn = (int)gridDim.x + 8 * (int)ticket + xcd;      // (the grid is a multiple of 8)
            mailbox[lane] = tn < ntiles ? tn : -1;     // lane 0 holds the ticket
        }
    };

    // The bias slice of a tile (256 floats) travels by LDS-DMA as well (one 16-B piece per lane of wave 0, double-buffered,
    // issued between the K-loops for the NEXT tile).  A register-returning load would either be pending at a K-loop back edge
    // (the compiler then retires the whole DMA stream at the top of every K-tile) or be waited for where it is used — and
    // vmcnt is in order: that wait would cover every output store issued before it.
    auto stage_bias = [&](int nn, bool live, int which) {
        if (wave == 0) {
            const int nj = nn + lane * 4;
            const float* src = (live && p.bias && nj < p.N) ? p.bias + nj : (const float*)zero;
            glds16(src, smem + BIASBUF + which * 1024);
        }
    };
    int bias_cur = 0;
    // prologue of the FIRST tile: K-tile 0 and K-tile 1 complete — the state every later tile starts from
    stage_bias(n0, true, 0);
    draw_ticket();
    stage_a(0, 0, 0); stage_w(0, 0, 0); stage_w(0, 0, 1); stage_a(0, 0, 1);        // the order of the steady-state stream
    stage_a(64, 1, 0); stage_w(64, 1, 0); stage_w(64, 1, 1);                        // (A rows 64-127 of K-tile 1: P1 of K-tile 0)
    __builtin_amdgcn_s_waitcnt(0x0f70);                    // vmcnt(0)
    asm volatile("" : "+v"(ticket)::"memory");
    post_ticket();
    bool first = true;
#ifdef MEDP_V7_ABLATE_LOADS
    ablate_on = true;
#endif

#ifdef MEDP_V7_PHASE_TRACE
    unsigned pt_acc[17], pt_last = 0;
#pragma unroll
    for (int i = 0; i < 17; ++i) pt_acc[i] = 0;
#endif
    for (;;) {
        // ---- tile top: K-tiles 0 and 1 of this tile have landed in every wave; the barrier makes them (and the mailbox) visible
        MEDP_BAR();
        stamp(0, ((long long)m0 << 32) | (unsigned)n0);
        rows_live[0] = m0 + wm * 128 < p.M;
        rows_live[1] = m0 + wm * 128 + 64 < p.M;
        // (Zeroed here, with the matrix pipe idle, and not where the epilogue has finished with a row block.  Written there, the
        //  compiler sees one zero value and still copies it into the 128 registers at this point; with 128 separately opaque
        //  zeros every accumulator stays live through the epilogue, whose temporaries otherwise reuse the row blocks already
        //  packed, and 170-220 VGPRs spill.)
        float z;                       // an opaque zero: a known-zero accumulator makes the compiler peel K-tile 0 (code x6, +30 VGPRs)
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){z, z, z, z};
        if (first) read_w(smem, 0, fw0a);     // later tiles: read in P4 of the previous tile's last K-tile
        first = false;
        if (wm == 1) MEDP_BAR();       // group 1 runs one barrier behind (group 0 pays its extra barrier after the loop)

#ifdef MEDP_V7_PHASE_TRACE
        pt_last = (unsigned)__builtin_readcyclecounter();
#endif
        int t_next = -1, m0n = 0, n0n = 0;
        // The K-tile body is the shared one (gemm_tile256.h).  The stream runs two K-tiles ahead and from K-tile nkt-2 on belongs
        // to the NEXT tile (its K-tiles 0 and 1; nobody: descriptors without records): when the loop ends all of them but the last A piece are
        // issued, and the W0 fragments of the next K-tile 0 are in registers.  Tiles start with those landed, so the waits of
        // K-tile 0 are skipped: the first wait that covers the previous tile's output stores is P2 of K-tile 1.
        auto before_p2 = [&](int kt) {
            if (kt == nkt - 2) {       // from here on the stream reads the next tile (P1 still staged this tile's last A piece)
                t_next = __builtin_amdgcn_readfirstlane(mailbox[0]);
                if (t_next >= 0) map.origin(t_next, MB, SN, BM, m0n, n0n);
                set_m(t_next >= 0 ? m0n : -1);
                set_n(t_next >= 0 ? n0n : -1);
            }
        };
        auto clock = [&](int k) { PT(k); };
        auto ktile = [&](int kt, const bf16x8 (*fw0)[2], bf16x8 (*fw0n)[2]) {
            // where K-tiles kt + 1 and kt + 2 of the stream live: element offset in the source tile and K buffer (computed here, at the
            // top of the K-tile, and not inside the stream lambdas: that keeps the compiler's code the one the waits were measured with)
            const int k2 = kt + 2 < nkt ? (kt + 2) * 64 : (kt + 2 - nkt) * 64;
            const int k1 = kt + 1 < nkt ? (kt + 1) * 64 : 0;
            const int b2 = kt & 1;
            auto stream_a = [&](int t, int j) { if (t == kt + 1) stage_a(k1, b2 ^ 1, j); else stage_a(k2, b2, j); };
            auto stream_w = [&](int, int h) { stage_w(k2, b2, h); };
            tile256_ktile<true>(smem, kt, fw0, fw0n, fw1, read_a, read_w, mma, stream_a, stream_w, before_p2, clock);
        };
#pragma clang loop unroll(disable)
        for (int kt = 0; kt < nkt; kt += 2) {
            ktile(kt, fw0a, fw0b);
            ktile(kt + 1, fw0b, fw0a);
        }
        if (wm == 0) MEDP_BAR();

        // ---- between K-loops: K-tiles 0 and 1 of the next tile are in flight; its bias slice and the ticket after it join them
        stamp(1, 0);
        draw_ticket();
        stage_bias(n0n, t_next >= 0, bias_cur ^ 1);

        // ---- epilogue: bias / GELU / bf16 pack on the accumulator layout (a lane holds 4 consecutive columns of one row), then a
        // 16-row x 64-column bf16 patch per wave through LDS so that every global store instruction writes whole 128-B rows
        f32x4 bj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bj[j] = *(const f32x4*)(smem + BIASBUF + bias_cur * 1024 + (wn * 64 + j * 16 + kq * 4) * 4);
        char* wl = smem + 2 * KBUF + wave * PATCH;
        const bool full_tile = m0 + BM <= p.M && n0 + BN <= p.N;
        const int prow = lane >> 3, pchunk = lane & 7;
        const int ncol = n0 + wn * 64 + pchunk * 8;
        typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
        // FULL tiles: one straight line per activation, no bounds test, and the patch chain software-pipelined.
        // The serial form below pays, per row block, LDS write -> read latency + store issue with nothing to fill it (the memory
        // clobbers hold block i+1's arithmetic behind block i's read).  Here block i+1 is computed and packed WHILE block i's two
        // ds_read_b128 are in flight; they are the only LDS operations outstanding at that point (the bias slice was waited for by
        // its first use, in block 0), so the wait the compiler places in front of the stores is exactly "those two reads".  Block
        // i+1's patch writes follow block i's reads in program order, which is all the LDS needs (MEDP_WAVE_LDS_SYNC); the
        // sched_barriers keep the compiler from moving the arithmetic back out of the shadow of the reads.  16 stores per wave, rows
        // in the same order as below: the vmcnt(16) that ends the epilogue counts them.
        auto pack_block = [&](int i, auto act, u32x2 (&pk)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v = acc[i][j] + bj[j];
                if constexpr (decltype(act)::value) v = gelu_bf16_4(v);
                pk[j] = (u32x2){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
            }
        };
        auto epilogue_full = [&](auto act) {
            char* cp = (char*)((bf16_t*)p.C + (size_t)(m0 + wm * 128 + prow) * p.ldc + ncol);
            const size_t rows8 = (size_t)p.ldc * 16;                       // 8 rows of C in bytes
            u32x2 pk[4];
            u32x4 o[2];
            auto through_patch = [&]() {
#pragma unroll
                for (int j = 0; j < 4; ++j) *(u32x2*)(wl + fr * PROW + j * 32 + kq * 8) = pk[j];
                MEDP_WAVE_LDS_SYNC();
#pragma unroll
                for (int h = 0; h < 2; ++h) o[h] = *(const u32x4*)(wl + (h * 8 + prow) * PROW + pchunk * 16);
                MEDP_WAVE_LDS_SYNC();
            };
            pack_block(0, act, pk);
            through_patch();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __builtin_amdgcn_sched_barrier(0);
                if (i + 1 < 8) pack_block(i + 1, act, pk);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    __builtin_nontemporal_store(o[h], (u32x4*)cp);
                    cp += rows8;
                }
                if (i + 1 < 8) through_patch();
            }
        };
        if (full_tile) {
            if (p.act == 1) epilogue_full(std::true_type{});
            else epilogue_full(std::false_type{});
        } else {
            // clipped tiles: one row block after the other, every store tested.  (Written in place: as a lambda beside epilogue_full
            // the same text allocates 252 / 256 VGPRs instead of 237 / 241.)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 v = acc[i][j] + bj[j];
                    if (p.act == 1) v = gelu_bf16_4(v);
                    *(u32x2*)(wl + fr * PROW + j * 32 + kq * 8) = (u32x2){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
                }
                MEDP_WAVE_LDS_SYNC();
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = h * 8 + prow;
                    const int m = m0 + wm * 128 + i * 16 + row;
                    const u32x4 o = *(const u32x4*)(wl + row * PROW + pchunk * 16);
                    if (m < p.M && ncol < p.N) __builtin_nontemporal_store(o, (u32x4*)((bf16_t*)p.C + (size_t)m * p.ldc + ncol));
                }
                MEDP_WAVE_LDS_SYNC();
            }
        }
        // K-tiles 0 and 1 of the next tile (and the ticket) have landed once everything older than the 16 output stores of a
        // full tile has; a clipped tile issues an unknown number of stores and waits for all of them
        stamp(2, 0);
        if (full_tile) __builtin_amdgcn_s_waitcnt(0x4f70);     // vmcnt(16)
        else __builtin_amdgcn_s_waitcnt(0x0f70);               // vmcnt(0)
        asm volatile("" : "+v"(ticket)::"memory");
        stamp(3, 0);
        ++tcount;
        post_ticket();
        bias_cur ^= 1;
        if (t_next < 0) break;
        m0 = m0n;
        n0 = n0n;
    }
    if (trace && wave == 0) {
        __builtin_amdgcn_s_waitcnt(0xc07f);
        if (lane < 40) trace[(size_t)blockIdx.x * 40 + lane] = lane < tcount * 5 ? tbuf[lane] : 0ull;
    }
#ifdef MEDP_V7_PHASE_TRACE
    if (trace && lane < 16) {
        unsigned v = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) v = lane == i ? pt_acc[i] : v;
        trace[256 * 40 + ((size_t)blockIdx.x * 8 + wave) * 16 + lane] = v;
    }
#endif
    // the last workgroup to leave re-arms the ticket block (the next launch on this slot starts after this kernel ends)
    if (tid == 0) {
        const unsigned left = __hip_atomic_fetch_add(slot + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left == gridDim.x - 1) {
#pragma unroll
            for (int i = 0; i < 9; ++i) __hip_atomic_store(slot + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    MEDP_PROF_LEAVE(p.prof, p.prof_flags);
}

std::atomic<unsigned> g_ring_next{0}, g_capture_next{0};
std::atomic<int> g_api_cap{0};           // medp_gemm_persistent_cap: 0 = default
unsigned long long* g_trace = nullptr;   // debug hook, see medp_dbg_gemm_v7_trace

// A ticket block nobody else is using while the launch it is handed to runs: launches being CAPTURED (replayed for the life of
// their graph) never share one, eager launches take the next of a ring.  nullptr: none left (the caller launches without tickets).
unsigned* ticket_block(hipStream_t stream) {
    static unsigned* slots_of[MEDP_MAX_DEVICES] = {};      // the ticket blocks are a __device__ symbol: one copy per device
    int dev = 0;
    (void)hipGetDevice(&dev);
    MEDP_ONCE_PER_DEVICE({
        unsigned* sp = nullptr;
        if (hipGetSymbolAddress((void**)&sp, HIP_SYMBOL(g_v7_slots)) == hipSuccess) slots_of[dev % MEDP_MAX_DEVICES] = sp;
    });
    unsigned* slots = slots_of[dev % MEDP_MAX_DEVICES];
    if (!slots) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(stream, &cs);
    unsigned s;
    if (cs == hipStreamCaptureStatusActive) {
        s = g_capture_next.fetch_add(1);
        if (s >= (unsigned)CAPTURE_SLOTS) return nullptr;
        s += RING_SLOTS;
    } else {
        s = g_ring_next.fetch_add(1) % RING_SLOTS;
    }
    return slots + (size_t)s * SLOT_WORDS;
}

template <int TAG>
int launch_v7(const MedpGemmArgs& a, hipStream_t stream) {
    MEDP_ONCE_PER_DEVICE({
        (void)hipFuncSetAttribute((const void*)gemm_bf16_nt_v7_kernel<TAG>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    });
    unsigned* slot = ticket_block(stream);
    if (!slot) return -1;                                  // out of private blocks: the caller falls back to v6
    // Resident workgroups: the FEWEST (a multiple of 8) that still finish in the same number of rounds as 256 would — qkv (585
    // tiles) and fc1 (780) need 3 and 4 rounds on 256 CUs and equally on 200; the 56 CUs left alone serve the other branches of
    // the step for the whole launch (teacher step 5.39 -> 5.19 ms, and the GEMMs themselves run 4 % faster: fewer L2 clients).
    // MEDP_V7_WGS (a multiple of 8, <= 256) caps the count: the rounds are then counted against the cap.
    static const int env_cap = [] { const int v = medp_env_int("MEDP_V7_WGS", NWG); return (v >= 8 && v <= NWG) ? (v & ~7) : NWG; }();
    const int api_cap = g_api_cap.load();
    const int cap = api_cap > 0 ? api_cap : env_cap;
    const int ntiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    const int rounds = (ntiles + cap - 1) / cap;
    static const int fewest = medp_env_int("MEDP_V7_FEWEST_WGS", 1);      // 0: always `cap` workgroups (A/B)
    const int nwg = fewest ? min(cap, ((ntiles + rounds - 1) / rounds + 7) & ~7) : cap;
    // Tile walk inside an XCD: blocks of MB row-tiles x SN column-tiles (8 x 4 = one round of an XCD's 32 CUs; MEDP_V7_BLOCK=MBxSN
    // overrides).  Measured (FETCH_SIZE per launch, mean of qkv / fc1; in-box step time): 256 workgroups 8x4: 51.1 k KiB, 5.26 ms;
    // 200 workgroups 8x4: 69.2 k, 5.03-5.11 ms (the rounds of 25 per XCD straddle the blocks, the K-loops drift out of step and
    // re-fetch panels); 200 with 5x5: 71.1 k, same time; 192 workgroups 8x3 + the ragged rows as their own launch (every round
    // exactly one block): 48.0 k but 5.25 ms.  HBM traffic is not what binds these GEMMs (142.5 MB algorithmic = 18 us at 8 TB/s
    // against 65-100 us): the fastest arrangement is kept, the extra re-fetch is reported (profiles/traffic.json).
    static const int env_mb = medp_env_int("MEDP_V7_BLOCK", 0);
    static const int env_sn = [] { const char* e = getenv("MEDP_V7_BLOCK"); const char* x = e ? strchr(e, 'x') : nullptr; return x ? atoi(x + 1) : 0; }();
    int mb = 8, sn = 4;
    if (env_mb > 0 && env_sn > 0) { mb = env_mb; sn = env_sn; }
    gemm_bf16_nt_v7_kernel<TAG><<<nwg, 512, LDS_BYTES, stream>>>(a, slot, g_trace, mb, sn);
    MEDP_LAUNCH_CHECK("medp_gemm_bf16_nt(v7)");
    return 0;
}

}  // namespace

bool medp_gemm_v7_supports(const MedpGemmArgs& a) {
    return a.out_bf16 && a.residual == nullptr && a.scale == nullptr && a.N % 8 == 0 && a.ldc % 8 == 0 &&
           a.K % 128 == 0 && a.K >= 256 && (long long)a.M * a.lda < (1ll << 31) && (long long)a.N * a.ldw < (1ll << 31) &&
           a.lda < (1 << 23) && a.ldw < (1 << 23);       // (the 256 rows of a tile within a descriptor's 32-bit offsets and num_records)
}

bool medp_gemm_v7_eligible(const MedpGemmArgs& a) {
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    return tiles > NWG && medp_gemm_v7_supports(a);
}

// returns -1 when no private ticket block is left (caller launches v6 instead)
int medp_gemm_v7_launch(const MedpGemmArgs& a, int tag, void* stream) {
    return tag == 1 ? launch_v7<1>(a, (hipStream_t)stream) : launch_v7<0>(a, (hipStream_t)stream);
}

extern "C" int medp_gemm_persistent_cap(int cap) {
    const int v = cap <= 0 ? 0 : (cap < 8 ? 8 : (cap > NWG ? NWG : (cap & ~7)));
    return g_api_cap.exchange(v);
}

// Debug hook (NOT part of the C ABI in include/medp_hip.h; tools/trace_gemm_v7.py): while `buf` (device memory, 256 x 40 x u64)
// is set, every v7 launch dumps per workgroup and tile {origin, t(tile top), t(K-loop done), t(epilogue issued), t(next tile
// landed)} in 10-ns ticks.  Pass nullptr to switch it off.
extern "C" int medp_dbg_gemm_v7_trace(void* buf) {
    g_trace = (unsigned long long*)buf;
    return 0;
}
