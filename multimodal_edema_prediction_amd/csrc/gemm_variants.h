// Internal interface of the bf16 GEMM: the front end (gemm_bf16.hip: checks, plan, dispatcher), its kernel files (gemm_bf16_tiles.hip,
// gemm_bf16_v6.hip, gemm_bf16_v7.hip, gemm_ragged_rows.hip) and the internal callers (vit.hip); not part of the C ABI.
#pragma once
#include "gemm_profile.h"
// The operands of one GEMM, from the C entry points to the launchers.  The 256-tile kernels take the struct by value as their first
// kernel argument: a new field moves the offsets of the arguments behind it.
struct MedpGemmArgs {
    const void* A;
    const void* W;
    void* C;
    int M, N, K, lda, ldw, ldc;
    const float* bias;
    const float* scale;
    const float* residual;
    int ldr, act, out_bf16;
    unsigned long long* prof;   // optional in-kernel launch clock (gemm_profile.h)
    int prof_flags;      // 1: do not stamp the arrival, 2: do not stamp the departure (a GEMM issued as two launches shares one clock)
};
// The front end (gemm_bf16.hip): argument checks, gemm_plan, launch.  tag 1 = the CXR-encoder block GEMMs: their own kernel symbols
// and the launch clock.  `workspace` (may be null) allows split-K (medp_gemm_nt_workspace_bytes).
int medp_gemm_run(const MedpGemmArgs& a, int tag, float* workspace, size_t workspace_bytes, void* stream);

// ---- launchers, one per kernel family (which shape takes which: gemm_plan) ----
// gemm_bf16_tiles.hip: 128 x bn tiles (bn 64 or 128; partial / nsplit > 1: split-K with its finish pass) and v3 (256 x 128 tiles)
int medp_gemm_tile128_launch(const MedpGemmArgs& a, int bn, int tag, float* partial, int nsplit, void* stream);
int medp_gemm_v3_launch(const MedpGemmArgs& a, int tag, void* stream);
int medp_gemm_v6_launch(const MedpGemmArgs& a, int tag, void* stream);
// rows [m_begin, a.M) (at most 128 of them) as a skinny launch of their own (gemm_ragged_rows.hip): same bits as the tile kernels
int medp_gemm_ragged_rows_launch(const MedpGemmArgs& a, int m_begin, void* stream);
// v7 = v6 made persistent for grids of more than 256 tiles (gemm_bf16_v7.hip); launch returns -1 when it has no private
// ticket block left, and the caller launches v6 instead
bool medp_gemm_v7_eligible(const MedpGemmArgs& a);
// what the kernel itself asks of a launch (medp_gemm_v7_eligible: this and a grid of more than one round of 256 workgroups)
bool medp_gemm_v7_supports(const MedpGemmArgs& a);
int medp_gemm_v7_launch(const MedpGemmArgs& a, int tag, void* stream);
