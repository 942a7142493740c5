// Internal interface of the DuETT inference path: the embedding stage (duett_embed.hip) as the layer loop (duett.hip) launches it;
// not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "medp_hip.h"

// psi (model :45-66) built directly in the EVENT view with the event embedding added and the event encoder's first ScaleNorm applied:
// xe fp32 [B, V+1, (T+1)E], h bf16 (same shape), psi0_out (optional) psi in the time view [B, T+1, V+1, E] before the add
int medp_duett_psi_embed_launch(const MedpDuettWeights* w, const float* xs_static, const float* xs_ts, float* xe, void* h, float* psi0_out,
                                int B, int T, hipStream_t s);
// cve(xs_times) with the REP row appended (model :67-69): temb fp32 [B, T+1, (V+1)E]
int medp_duett_time_embed_launch(const MedpDuettWeights* w, const float* xs_times, float* temb, int B, int T, hipStream_t s);
