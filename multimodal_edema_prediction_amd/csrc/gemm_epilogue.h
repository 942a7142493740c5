// The fused GEMM epilogue  + bias[n] -> GELU -> * scale[n] (LayerScale) -> + residual[m,n] -> fp32 or bf16  of a lane that holds
// C[m][n .. n+3]: the store tail and the arithmetic in front of it.  The two forms are NOT the same arithmetic (v + 0 flips a -0,
// the two GELUs round differently): each kernel keeps the one it has always had.
#pragma once
#include "common.h"

// fp32, or bf16 packed into two dwords.  NT: non-temporal (v6: written once, all 256 workgroups flush together; -2 % step time)
template <bool NT = false>
__device__ __forceinline__ void gemm_store4(void* C, int ldc, int out_bf16, int m, int n, f32x4 v) {
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    if (out_bf16) {
        const u32x2 o = (u32x2){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        u32x2* dst = (u32x2*)((bf16_t*)C + (size_t)m * ldc + n);
        if constexpr (NT) __builtin_nontemporal_store(o, dst);
        else *dst = o;
    } else {
        f32x4* dst = (f32x4*)((float*)C + (size_t)m * ldc + n);
        if constexpr (NT) __builtin_nontemporal_store(v, dst);
        else *dst = v;
    }
}

// pointer-tested form (128-tile and split-K finish kernels): an absent bias / scale / residual is skipped; GELU is gelu_erf4
__device__ __forceinline__ f32x4 gemm_epi_tested(f32x4 v, const float* bias, const float* scale, const float* residual, int ldr,
                                                 int act, int m, int n) {
    if (bias) v += *(const f32x4*)(bias + n);
    if (act == 1) v = gelu_erf4(v);
    if (scale) v *= *(const f32x4*)(scale + n);
    if (residual) v += *(const f32x4*)(residual + (size_t)m * ldr + n);
    return v;
}

// preloaded form (v3, v6, ragged rows): bias4 / scale4 were loaded once per lane (0 / 1 where absent) and are always applied; the
// residual is the caller's.  BF16_GELU: gelu_bf16_4 for a bf16 result (v6, ragged rows); v3 uses gelu_erf4 throughout.
template <bool BF16_GELU>
__device__ __forceinline__ f32x4 gemm_act_scale(f32x4 v, f32x4 scale4, int act, int out_bf16) {
    if (act == 1) v = (BF16_GELU && out_bf16) ? gelu_bf16_4(v) : gelu_erf4(v);
    return v * scale4;
}
template <bool BF16_GELU>
__device__ __forceinline__ f32x4 gemm_epi_preloaded(f32x4 v, f32x4 bias4, f32x4 scale4, int act, int out_bf16) {
    return gemm_act_scale<BF16_GELU>(v + bias4, scale4, act, out_bf16);
}
