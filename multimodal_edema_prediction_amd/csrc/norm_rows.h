// The two ways a 64-lane wave holds one row in the wave-per-row norm kernels of norm.hip and duett.hip, and what those kernels share.
//
// THE CANONICAL ORDER lives in the holders' each(): lane l owns the float4 i = l, l + 64, ... of the row, ascending; a float4 adds
// (x, y) + (z, w) to the lane's partial sum; wave_sum folds the 64 partials.
// THE ROUNDING of a float4's products is the holder's dot4 and is written out, never left to -ffp-contract: the register form rounds
// every product, the re-read form fuses the second product of (x, y) and the first of (z, w).  So a formula's two forms share the
// order and every operation but that one, and agree to the last bits of a row's sum, not in them; each form reproduces itself on any
// compiler.  (Left to the compiler, the choice differed from instantiation to instantiation.)
#pragma once
#include <type_traits>

#include "common.h"

// The row in registers: NV float4 per lane (D <= 256 * NV); the float4 past the row's end read as zero and are skipped.
template <int NV>
struct RowRegs {
    float4 v[NV];
    int lane, D;
    // v[k] = f(i) for the lane's float4 of the row
    template <class F>
    __device__ __forceinline__ RowRegs(int lane, int D, F f) : lane(lane), D(D) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            v[k] = i < (D >> 2) ? f(i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ RowRegs(int lane, int D, const float* p) : RowRegs(lane, D, [p](int i) { return *(const float4*)(p + 4 * i); }) {}
    // f(i, float4 i of the row) for the lane's float4, in order; with a second row of the same form: f(i, this one's, o's)
    template <class F>
    __device__ __forceinline__ void each(F f) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            if (i < (D >> 2)) f(i, v[k]);
        }
    }
    template <class F>
    __device__ __forceinline__ void each(const RowRegs& o, F f) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            if (i < (D >> 2)) f(i, v[k], o.v[k]);
        }
    }
    // (a.x b.x + a.y b.y) + (a.z b.z + a.w b.w), four rounded products (on pairs: two v_pk_mul_f32)
    static __device__ __forceinline__ float dot4(float4 a, float4 b) {
#pragma clang fp contract(off)
        const f32x2 p = (f32x2){a.x, a.y} * (f32x2){b.x, b.y}, q = (f32x2){a.z, a.w} * (f32x2){b.z, b.w};
        return (p[0] + p[1]) + (q[0] + q[1]);
    }
};

// The row re-read on every traversal from p: global memory (the later sweeps hit L1 / L2) or an LDS tile.
struct RowReread {
    const float* p;
    int lane, D;
    __device__ __forceinline__ RowReread(int lane, int D, const float* p) : p(p), lane(lane), D(D) {}
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        for (int i = lane; i < (D >> 2); i += 64) f(i, *(const float4*)(p + 4 * i));
    }
    template <class F>
    __device__ __forceinline__ void each(const RowReread& o, F f) const {
        for (int i = lane; i < (D >> 2); i += 64) f(i, *(const float4*)(p + 4 * i), *(const float4*)(o.p + 4 * i));
    }
    // the same sum with two of the four products fused (one v_pk_mul_f32 + one v_pk_fma_f32)
    static __device__ __forceinline__ float dot4(float4 a, float4 b) {
#pragma clang fp contract(off)
        return fmaf(a.y, b.y, a.x * b.x) + fmaf(a.z, b.z, a.w * b.w);
    }
};

// four floats to elements 4 i .. 4 i + 3 of the output row at yrow: one float4, or two dwords of packed bf16
template <bool OUT_BF16>
__device__ __forceinline__ void store_row4(void* yrow, int i, float o0, float o1, float o2, float o3) {
    if (OUT_BF16) {
        uint2 o;
        o.x = pack_bf2(o0, o1);
        o.y = pack_bf2(o2, o3);
        *(uint2*)((bf16_t*)yrow + 4 * i) = o;
    } else {
        *(float4*)((float*)yrow + 4 * i) = make_float4(o0, o1, o2, o3);
    }
}
template <bool OUT_BF16>
__device__ __forceinline__ void* row_ptr(void* y, size_t off) { return OUT_BF16 ? (void*)((bf16_t*)y + off) : (void*)((float*)y + off); }

// ScaleNorm forward: y = x / max(||x||_2, eps) * sqrt(D) * g        (x_transformers ScaleNorm; g is a 1-element parameter)
template <class Row>
__device__ __forceinline__ float scalenorm_rn(const Row& r, float eps) {       // 1 / max(||row||_2, eps), on every lane
    float ss = 0.f;
    r.each([&](int, float4 v) { ss += Row::dot4(v, v); });
    return 1.0f / fmaxf(sqrtf(wave_sum(ss)), eps);
}
template <bool OUT_BF16, class Row>
__device__ __forceinline__ void scalenorm_fwd_row(const Row& r, const float* g, float eps, void* y, int ldy, float* rnorm_out, int row) {
    void* yrow = row_ptr<OUT_BF16>(y, (size_t)row * ldy);
    const float rn = scalenorm_rn(r, eps);
    if (r.lane == 0 && rnorm_out) rnorm_out[row] = rn;
    const float sc = rn * sqrtf((float)r.D) * g[0];
    r.each([&](int i, float4 v) { store_row4<OUT_BF16>(yrow, i, v.x * sc, v.y * sc, v.z * sc, v.w * sc); });
}

// Host side: f(std::integral_constant<int, NV>) for the first register width NV of the list with nv <= NV; false, f not called, if none
template <int... NVs, class F>
inline bool dispatch_nv(int nv, F f) {
    return ((nv <= NVs && (f(std::integral_constant<int, NVs>{}), true)) || ...);
}
