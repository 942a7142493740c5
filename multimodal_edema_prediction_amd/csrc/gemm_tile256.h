// The shared core of the 256 x 256 x 64 block GEMMs (gemm_bf16_v6.hip: one tile per workgroup; gemm_bf16_v7.hip: persistent):
// LDS geometry, LDS-DMA helper, tile map and the four-phase K-tile body with its hand-counted waits.  Internal,
// not part of the C ABI.  Both kernels must compile to the instructions they had before a change here: tools/diff_kernel_isa.py.
//
// 256 x 256 x 64 tiles, EIGHT waves (2 x 4, 128 x 64 per wave), two waves per SIMD in PING-PONG.
//
// v3/v5 measurements: a wave that owns its SIMD alone pays for every LDS-DMA issue (~100+ cycles inside a K-step that also
// carries the fragment reads) and for every barrier with an idle matrix pipe.  Here each SIMD holds one wave of group 0
// (rows 0..127 of the tile) and one of group 1 (rows 128..255).  A K-tile (64 deep) is four PHASES of 16 MFMAs (one
// 64 x 32 quadrant of the wave's 128 x 64 output, both k-halves); every phase is
//     [load section: ds_read fragments, 2 LDS-DMA pieces, lgkmcnt(0)]  s_barrier  [16 MFMA at raised priority]  s_barrier
// and group 1 runs ONE barrier behind group 0, so between any two consecutive barriers one group multiplies while the
// other issues its loads: the matrix pipe always has a wave whose operands are already in registers.
//
// LDS: two K-tile buffers of 64 KiB = four 16-KiB half-tiles each (A rows 0-127 | A rows 128-255 | W rows 0-127 |
// W rows 128-255), 128-B rows, 16-B chunk c stored at c ^ (row & 7) (conflict-free ds_read_b128 lane groups).
// Fragment schedule of K-tile t (per wave): P1 reads A0 (8) + W0 (4), P2 W1 (4), P3 A1 (8), P4 nothing;
// MFMA quadrants: P1 (A0,W0)  P2 (A0,W1)  P3 (A1,W1)  P4 (A1,W0).
// Phase plan of K-tile t (per wave; in-kernel phase clocks, tools/trace_gemm_v7.py --phases, decided it: a load section with
// 12 ds_read_b128 took 670 ticks against ~330 for the 16 MFMAs it has to hide behind, one with 8 or 4 reads 300-360):
//     P1: read A rows 0-63 (8),   DMA A rows 64-127 (t+1)   MFMA (A0, W0)
//     P2: read W1 (4),            DMA A rows 0-63 (t+2)     MFMA (A0, W1)    wait vmcnt(10): A rows 64-127 of K-tile t
//     P3: read A rows 64-127 (8), DMA W half 0 (t+2)        MFMA (A1, W1)    wait vmcnt(6):  W of K-tile t+1
//     P4: read W0 of K-TILE t+1 (4) into the other W0 register set,
//                                 DMA W half 1 (t+2)        MFMA (A1, W0)
// i.e. no load section carries more than 8 fragment reads or more than 2 DMA pieces (4 pieces + 4 reads in one section cost
// 560-700 ticks).  Every LDS region is refilled (same buffer) one or two phases after its last read.  The counts of the
// waits are "everything but the pieces issued after the one needed" (2 pieces per phase, in the order above).
// RAW: a wait sits in a load section, before a barrier every wave passes, and the data is first read one phase later (group 1
// runs one barrier behind: a wait placed after the MFMAs would not yet have been executed by it).  WAR: every ds_read is
// retired (lgkmcnt(0)) before the barrier that ends its load section; the refill is issued one phase later.
// The PROLOGUE of a kernel issues K-tiles 0 and 1 in the order of this steady-state stream — A rows 0-63, W half 0, W half 1,
// A rows 64-127 of K-tile 0, then A rows 0-63, W half 0, W half 1 of K-tile 1 (its A rows 64-127 follow in P1 of K-tile 0) —
// so the counts hold from the first K-tile on.
//
// ADDRESSING of the A / W stream: buffer-addressed LDS-DMA (blds16 in common.h, `buffer_load_dwordx4 ... offen lds`).  The descriptors
// live in SGPRs and are built with scalar operations once per tile; a lane's vector offset (srow * ld + schunk * 8) * 2 is
// loop-invariant, one VGPR per operand; what moves is the instruction's scalar offset.  A steady-state load section is then ds_reads,
// two m0 writes and two loads: no vector instruction computes an address (the per-lane 64-bit address and the select of a zero chunk
// were ~15 VALU per section, issued at priority 0 beside the partner wave's 16 prioritised MFMAs: profiles/r05_gemm_buffer_dma.txt).
// The buffer form counts in vmcnt exactly like the flat one, dropped lanes included: the hand-counted waits above are unchanged.
//   * gemm_bf16_v6.hip: one descriptor per 64-row piece position of the tile (A rows 0-63 .. 192-255, W likewise): base = the
//     position's first row, num_records = the bytes of its rows below M / N (at most 64 rows); the scalar offset carries the K
//     advance only.
//   * gemm_bf16_v7.hip: ONE descriptor per operand: base = the tile's first row, num_records = the bytes of its rows below M / N (at
//     most 256 rows; none where the stream has no next tile); the scalar offset is q * 64 * ld * 2 + k0 * 2 for piece position q.
//     (Eight descriptors are 32 SGPRs held across the K-loop; around it the compiler spilled 57 SGPRs to VGPR lanes.)
// What the range check is relied on for (tools/probe_buffer_lds.hip measured both on gfx950):
//   * the scalar offset TAKES PART in the check (each dword of a lane is dropped iff vector + scalar offset of that dword is
//     >= num_records).  v6 holds either way: all row and tile movement is in the descriptors' bases, the scalar offset never leaves a
//     row (k0 + 64 <= K <= ld), so the last live row's chunk still ends at or below num_records = rows * ld * 2 while the first dead
//     row starts at it.  v7 DEPENDS on it: a lane of piece q addresses byte ((q * 64 + srow) * ld + k0 + schunk * 8) * 2 of the tile,
//     row r = q * 64 + srow, and since k0 + schunk * 8 + 8 <= K <= ld all 16 bytes lie in [r * ld * 2, (r + 1) * ld * 2): below
//     num_records = rows * ld * 2 iff r < rows, whole chunks either way.  The sum stays below 2^32 (256 * ld * 2 with ld < 2^23,
//     medp_gemm_v7_supports), so it cannot wrap back into range.  Without the scalar offset in the check, rows past M / N of a tile
//     would be READ (up to 255 rows past the operand's end) — the results would still be right, by the next point, the reads not;
//   * a lane past num_records reads nothing and writes ZEROS to LDS, as the zero chunk did — but nothing depends on it: a row of
//     A at or past M only ever feeds output rows >= M, a row of W at or past N only output columns >= N, and neither is stored
//     (every epilogue tests m < M and n < N per element, or runs on a tile that lies wholly below M and N).  Rows 112-127 of a
//     group's A half under 224-row tiles lie past their descriptor (48 rows) and are skipped at compile time by read_a / mma.
//     Whatever such LDS rows hold — zeros or a previous K-tile — cannot reach a stored element.
// The one-tile kernel keeps the per-lane form for K % 64 != 0 (chunks past K INSIDE a K-tile need a select per lane); the bias
// side stream stays on glds16.
#pragma once
#include "common.h"

namespace {

__device__ __attribute__((aligned(16))) uint32_t g_zero16_t256[4] = {0, 0, 0, 0};   // source of every out-of-range 16-B chunk

constexpr int BN = 256, HALF = 128 * 128, KBUF = 4 * HALF;   // 16 KiB half-tile, 64 KiB K-tile buffer

// patch write -> read (and read -> next write) inside ONE wave: the LDS executes a wave's operations in order, only the
// compiler must not reorder them.  (A workgroup-scope fence here also emits vmcnt(0): the epilogue would wait for the global
// stores it issued before.)
#define MEDP_WAVE_LDS_SYNC()                        \
    do {                                            \
        asm volatile("" ::: "memory");              \
        __builtin_amdgcn_wave_barrier();            \
        asm volatile("" ::: "memory");              \
    } while (0)

#define MEDP_BAR()                                  \
    do {                                            \
        __builtin_amdgcn_sched_barrier(0);          \
        __builtin_amdgcn_s_barrier();               \
        __builtin_amdgcn_sched_barrier(0);          \
    } while (0)

// Tile index -> origin.  Workgroups are dispatched in index order, block b to XCD b % 8, one per CU (32 CUs per XCD).  The
// FULL row-tiles come first: XCD x gets a contiguous run of them, walked in bands of MB row-tiles x super-columns of SN
// column-tiles (see v3 in gemm_bf16_tiles.hip), so its L2 sees few panels; the cheap tiles of a ragged last row (M = 64 * 257: 64 live
// rows, three quarters of their MFMAs skipped) take the highest indices, i.e. they are dispatched LAST.  fc1 (768 full + 12
// ragged tiles) is then 96 full tiles = exactly 3 rounds per XCD plus a short ragged tail, instead of a fourth round that
// holds one full tile per XCD.
struct Tile256Map {
    int tiles_n, tiles_m, tm_full, nfull, full8;
    __device__ __forceinline__ Tile256Map(int M, int N, int BM) {
        tiles_n = (N + BN - 1) / BN;
        tiles_m = (M + BM - 1) / BM;
        const int rag = (M % BM) ? 1 : 0;
        tm_full = tiles_m - rag;
        nfull = tm_full * tiles_n;
        full8 = nfull & ~7;                            // full tiles dealt in runs of nfull/8 per XCD; the rest by index
    }
    __device__ __forceinline__ void origin(int bid, int MB, int SN, int BM, int& m0, int& n0) const {
        if (bid < nfull) {
            const int wg = bid < full8 ? (bid & 7) * (full8 >> 3) + (bid >> 3) : bid;   // the < 8 leftover full tiles keep their index
            const int band = wg / (MB * tiles_n), rb = wg % (MB * tiles_n);
            const int mb = min(MB, tm_full - band * MB);
            const int sc = rb / (mb * SN), r2 = rb % (mb * SN);
            const int sn = min(SN, tiles_n - sc * SN);
            m0 = (band * MB + r2 / sn) * BM;
            n0 = (sc * SN + r2 % sn) * BN;
        } else {                                       // the ragged row, one tile per column
            m0 = tm_full * BM;
            n0 = (bid - nfull) * BN;
        }
    }
};

// LDS address of LDS-DMA piece j (rows 64 j .. 64 j + 63) of half-tile `which` (0: A rows 0-127, 1: A rows 128-255, 2: W rows
// 0-127, 3: W rows 128-255) in K buffer b, for this wave: a half-tile = 128 rows x 8 chunks, a lane's two pieces are rows
// (tid >> 3) and (tid >> 3) + 64, and LDS position (tid & 7) of a row holds source chunk (tid & 7) ^ (row & 7)
__device__ __forceinline__ char* piece_dst(char* smem, int b, int which, int wave, int j) {
    return smem + b * KBUF + which * HALF + wave * 1024 + j * 8192;
}

// One K-tile: the phase plan at the top of this file, written once for both kernels.  fw0 holds the W0 fragments of K-tile kt,
// fw0n receives those of kt + 1, fw1 is the W1 set.  The kernel passes its own pieces:
//   read_a(buf, a) / read_w(buf, b, fw) / mma(a, b, fw): fragment reads and one MFMA quadrant (16 MFMAs at raised priority);
//   stage_a(t, j): issue A rows 64 j .. 64 j + 63 (both groups) of K-tile t of the stream;  stage_w(t, h): W half h of K-tile t
//                  (TWO LDS-DMA pieces each: the counted waits depend on it);
//   FIRST_LANDED:  K-tiles 0 and 1 have landed before the loop (v7: the previous tile's loop streamed them), so K-tile 0 skips
//                  its counted waits;
//   before_p2(kt): runs at the top of P2 (v7 switches the stream's source to the next tile there);
//   clock(k):      phase-clock hook, k = 0..15 = {load section, wait at its barrier, MFMA issue, wait at its barrier} x P1..P4.
template <bool FIRST_LANDED, class ReadA, class ReadW, class Mma, class StageA, class StageW, class BeforeP2, class Clock>
__device__ __forceinline__ void tile256_ktile(const char* smem, int kt, const bf16x8 (*fw0)[2], bf16x8 (*fw0n)[2], bf16x8 (*fw1)[2],
                                              ReadA&& read_a, ReadW&& read_w, Mma&& mma, StageA&& stage_a, StageW&& stage_w,
                                              BeforeP2&& before_p2, Clock&& clock) {
    const char* buf = smem + (kt & 1) * KBUF;
    // ---- P1
    read_a(buf, 0);
    stage_a(kt + 1, 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0), vmcnt/expcnt untouched
    clock(0);
    MEDP_BAR();
    clock(1);
    mma(0, 0, fw0);
    clock(2);
    MEDP_BAR();
    clock(3);
    // ---- P2
    before_p2(kt);
    read_w(buf, 1, fw1);
    stage_a(kt + 2, 0);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (!FIRST_LANDED || kt >= 1) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");   // A rows 64-127 of K-tile kt (issued in P1(kt-1)) have landed
    clock(4);
    MEDP_BAR();
    clock(5);
    mma(0, 1, fw1);
    clock(6);
    MEDP_BAR();
    clock(7);
    // ---- P3
    read_a(buf, 1);
    stage_w(kt + 2, 0);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (!FIRST_LANDED || kt >= 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // W (and A rows 0-63) of K-tile kt+1 (issued in P2..P4(kt-1)) have landed
    clock(8);
    MEDP_BAR();
    clock(9);
    mma(1, 1, fw1);
    clock(10);
    MEDP_BAR();
    clock(11);
    // ---- P4
    read_w(smem + ((kt + 1) & 1) * KBUF, 0, fw0n);
    stage_w(kt + 2, 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    clock(12);
    MEDP_BAR();
    clock(13);
    mma(1, 0, fw0);
    clock(14);
    MEDP_BAR();
    clock(15);
}

}  // namespace
