// The psi cell rule (model :53-66): which of its four sources fills cell (b, t, v) of psi [B, T+1, V+1, E].  One statement of the
// conditions for the training-form assembly (duett_train.hip: forward and backward) and the inference embed kernel (duett_embed.hip).
//   psi[b][t][v][:] = var_out[v][b*T+t][:] | tab_out[b][:] (v == V) | special[0] (masked timestep / masked event) | special[1] (t == T, event not masked at t = 0)
#pragma once
#include "common.h"

enum { PSI_VAR = 0, PSI_STATIC = 1, PSI_MASKED = 2, PSI_REP = 3 };

// `in` hands out the cell's inputs from xs [B, T, 2V+1]: msk() the mask column and cnt() variable v's count at timestep t, cnt0() that
// count at timestep 0.  Either it reads them where a condition asks (PsiCellLazy) or it holds them already (PsiCellIn).
template <class In>
__device__ __forceinline__ int psi_cell_classify(const In& in, int t, int v, int T, int V) {
    // REP row; the reference extends the event mask to it with TIMESTEP 0's row (duett.py:250), so a variable whose event is masked
    // there carries the MASKED embedding in the REP row too (every SSL batch: the masked event's count is -1 at all timesteps)
    if (t == T) return (v < V && in.cnt0() == -1.0f) ? PSI_MASKED : PSI_REP;
    if (in.msk() == 1.0f) return PSI_MASKED;                // masked timestep
    if (v == V) return PSI_STATIC;                          // static column
    if (in.cnt() == -1.0f) return PSI_MASKED;               // masked event
    return PSI_VAR;                                         // variable MLP output
}

// the loads behind the conditions: a cell reads only what decides it
struct PsiCellLazy {
    const float* xs;
    int b, t, v, T, V;
    __device__ const float* row() const { return xs + ((size_t)b * T + t) * (2 * V + 1); }
    __device__ float msk() const { return row()[2 * V]; }
    __device__ float cnt() const { return row()[V + v]; }
    __device__ float cnt0() const { return xs[(size_t)b * T * (2 * V + 1) + V + v]; }
};
__device__ __forceinline__ int psi_cell_kind(const float* __restrict__ xs, int b, int t, int v, int T, int V) {
    return psi_cell_classify(PsiCellLazy{xs, b, t, v, T, V}, t, v, T, V);
}

// the loads up front, for a kernel that wants all of a cell's loads in flight before the first condition: the count is the one the
// rule will ask for (timestep 0's in the REP row), val is variable v's value (what the MLP of a PSI_VAR cell reads).
// t > T is "no cell": nothing is read and the kind is PSI_MASKED.
struct PsiCellIn {
    float mask = 1.f, count = 0.f, val = 0.f;
    __device__ PsiCellIn(const float* __restrict__ xs, int b, int t, int v, int T, int V) {
        if (t > T) return;
        const float* row = xs + ((size_t)b * T + (t == T ? 0 : t)) * (2 * V + 1);
        if (t < T) mask = row[2 * V];
        if (v < V) {
            count = row[V + v];
            if (t < T) val = row[v];
        }
    }
    __device__ float msk() const { return mask; }
    __device__ float cnt() const { return count; }
    __device__ float cnt0() const { return count; }
};
