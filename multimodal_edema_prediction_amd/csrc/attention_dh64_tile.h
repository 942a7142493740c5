// The LDS image of the head-dim-64 attention kernels (attention_dh64.hip forward, attention_dh64_bwd.hip backward) and everything that
// must agree on it.  Internal, not part of the C ABI.  The kernels must compile to the instructions they had before a change here
// (tools/diff_kernel_isa.py); that gate, not taste, decided which helper is a function and which a macro, and in which association an
// offset is summed: the same rule written as an inlined function gave another schedule in some callers.
//
// An image holds up to KC rows (keys or queries) of one (batch, head), row-major [row][64] bf16: a row is IMG_ROW = 128 bytes = eight
// 16-B chunks, and chunk c of row r is stored at chunk position IMG_CHUNK(c, r) = c ^ (r & 7) (conflict-free ds_read_b128 lane groups
// and transposing reads).  It is FILLED by LDS-DMA, a wave's 64 lanes handing over 8 whole rows that land in lane order, so the swizzle
// is applied to the SOURCE chunk a lane fetches (img_stage_piece); rows past the end of the sequence come from the zero chunk.
// It is READ row-wise (img_frag) and transposed (img_tr, img_tr_rows).
#pragma once
#include "common.h"

namespace {

__device__ __attribute__((aligned(16))) uint32_t g_zero16_attn[4] = {0, 0, 0, 0};   // source of every out-of-range 16-B chunk

constexpr int KC = 320;        // most rows per LDS image (5 blocks of 64)
constexpr int IMG_ROW = 128;   // bytes per image row
#define IMG_CHUNK(chunk, row) ((chunk) ^ ((row) & 7))

// two f32x4 -> eight bf16 (the B operand of the second product, straight from the accumulators of the first)
__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
    union { bf16x8 v; uint32_t u[4]; } pk;
    pk.u[0] = pack_bf2(a[0], a[1]);
    pk.u[1] = pack_bf2(a[2], a[3]);
    pk.u[2] = pack_bf2(b[0], b[1]);
    pk.u[3] = pack_bf2(b[2], b[3]);
    return pk.v;
}

// row -> the two halves (d = 8 kq .. + 7 and 32 + 8 kq .. + 7) of an MFMA 16x16x32 A operand
__device__ __forceinline__ void img_frag(const char* img, int row, int kq, bf16x8& f0, bf16x8& f1) {
    const char* base = img + row * IMG_ROW;
    f0 = *(const bf16x8*)(base + (IMG_CHUNK(0 + kq, row) << 4));
    f1 = *(const bf16x8*)(base + (IMG_CHUNK(4 + kq, row) << 4));
}

// Transposed read (ds_read_b64_tr_b16): lane 4 qq + pp of a 16-lane group reads row qq, columns 4 pp .. 4 pp + 3 of a 16 x 16 tile; for
// the d-tile dt (features 16 dt .. + 15) that is chunk 2 dt + (pp >> 1), half pp & 1, of image row `row`.  IMG_TR_TERMS is that byte offset
// as a sum WITHOUT outer parentheses: the forward adds the terms to the image pointer one by one (IMG_TR_ROWS / img_tr_rows: the two
// 16-row tiles row0, row1 = row0 + 16 of a k = 32 operand), the backward sums them first and reads both its images at o0, o1 (img_tr).
#define IMG_TR_TERMS(row, dt, tr_p) (row) * IMG_ROW + (IMG_CHUNK((dt) * 2 + ((tr_p) >> 1), row) << 4) + ((tr_p) & 1) * 8
#define IMG_TR_ROWS(img, row0, row1, dt, tr_p) \
    __builtin_shufflevector(lds_tr16((img) + IMG_TR_TERMS(row0, dt, tr_p)), lds_tr16((img) + IMG_TR_TERMS(row1, dt, tr_p)), 0, 1, 2, 3, 4, 5, 6, 7)
__device__ __forceinline__ bf16x8 img_tr_rows(const char* img, int row0, int row1, int dt, int tr_p) { return IMG_TR_ROWS(img, row0, row1, dt, tr_p); }
__device__ __forceinline__ bf16x8 img_tr(const char* img, int o0, int o1) { return __builtin_shufflevector(lds_tr16(img + o0), lds_tr16(img + o1), 0, 1, 2, 3, 4, 5, 6, 7); }

// Staging pass i of an NT-thread workgroup: this thread's 16-B piece of BOTH images.  Piece i * NT + tid is chunk (piece & 7) of image row
// piece >> 3 (img_piece_row); rows at or past nrows come from `zero`.  grow0 = the global row of image row 0, h = the head.
template <int NT> __device__ __forceinline__ int img_piece_row(int i, int tid) { return (i * NT + tid) >> 3; }
template <int NT>
__device__ __forceinline__ void img_stage_piece(const bf16_t* gX, int ldX, const bf16_t* gY, int ldY, const bf16_t* zero, char* sX, char* sY,
                                                size_t grow0, int nrows, int h, int i, int tid, int wave) {
    const int qd = i * NT + tid;
    const int row = qd >> 3, c = IMG_CHUNK(qd & 7, row);
    const bool ok = row < nrows;
    const size_t grow = grow0 + row;
    glds16(ok ? gX + grow * ldX + h * 64 + c * 8 : zero, sX + (i * NT + wave * 64) * 16);
    glds16(ok ? gY + grow * ldY + h * 64 + c * 8 : zero, sY + (i * NT + wave * 64) * 16);
}

}  // namespace

// A launch plan (host): attn_dh64_plan in attention_dh64.hip, attn_dh64_bwd_plan in attention_dh64_bwd.hip.
enum { ATTN_DH64_W4 = 4, ATTN_DH64_W8 = 8, ATTN_DH64_S257 = 257, ATTN_DH64_BWD = 2 };     // `kernel`, as medp_dbg_attn_dh64_plan reports it
struct AttnDh64Plan {
    int kernel, gx, gy, gz, threads;
    int lds, crows;      // dynamic LDS bytes; LDS rows per image
};
AttnDh64Plan attn_dh64_bwd_plan(int B, int S, int H);
