"""Plain torch restatements that the kernel-level tests of losses.hip and duett_train.hip compare against, for the
cases the oracle does not state in a callable form: losses whose clamp bounds must be the kernels' fp32 constants, and the pieces of
`duett_ref.build_psi` that the training glue computes one kernel at a time.  Every function works in the dtype of its inputs (the
GPU tests hand it float64) and is differentiable, so gradients come from autograd.  tests/test_kernel_refs_cpu.py shows that each
one equals the oracle function it restates."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

# the clamp bounds as the kernels hold them: fp32 constants, `1.f - eps` evaluated in fp32
KD_LO = float(np.float32(1e-7))
KD_HI = float(np.float32(1.0) - np.float32(1e-7))
AUX_LO = float(np.float32(1e-6))
AUX_HI = float(np.float32(1.0) - np.float32(1e-6))


def kd_loss(z_s, z_t, y, T, alpha, pos_weight=None, lo=KD_LO, hi=KD_HI):
    """losses_ref.student_kd_loss with the probability clamp [lo, hi] spelt out."""
    p_t = torch.sigmoid(z_t.detach() / T).clamp(lo, hi)
    p_s = torch.sigmoid(z_s / T).clamp(lo, hi)
    kl = p_t * (p_t.log() - p_s.log()) + (1 - p_t) * ((1 - p_t).log() - (1 - p_s).log())
    kd = (T ** 2) * kl.mean()
    pw = None if pos_weight is None else torch.tensor([pos_weight], dtype=z_s.dtype)
    bce = F.binary_cross_entropy_with_logits(z_s, y.to(z_s.dtype), pos_weight=pw)
    return {"total": alpha * bce + (1 - alpha) * kd, "bce": bce.detach(), "kd": kd.detach()}


def aux_residual_kl(img_logits, scaled_correction, y_multi, mask, smoothing, lo=AUX_LO, hi=AUX_HI):
    """losses_ref.aux_residual_kl with the probability clamp [lo, hi] spelt out."""
    y = y_multi.to(scaled_correction.dtype)
    ys = y * (1 - smoothing) + (1 - y) * smoothing
    p = torch.sigmoid(img_logits.detach() + scaled_correction).clamp(min=lo, max=hi)
    kl = ys * (torch.log(ys) - torch.log(p)) + (1 - ys) * (torch.log(1 - ys) - torch.log(1 - p))
    m = mask.to(scaled_correction.dtype)
    return (kl * m).sum() / m.sum().clamp(min=1.0)


def masked_mse(a, b, mask=None):
    """The value terms of duett_ref.ssl_loss: F.mse_loss(a * m, b * m); no mask = all ones."""
    return F.mse_loss(a, b) if mask is None else F.mse_loss(a * mask, b * mask)


def bce_mean(logits, y, weight=None):
    """The presence terms of duett_ref.ssl_loss (weight: torch's own per-element weight)."""
    return F.binary_cross_entropy_with_logits(logits, y, weight=weight)


def ssl_like_inputs(B, T, V, g):
    """xs [B, T, 2V+1] with every kind of cell: counts -1 (masked event; one variable masked at EVERY step, as the SSL batch has it, and
    some at single steps, timestep 0 among them), counts above the table, non-integers, masked timesteps, both in one cell."""
    xs = torch.zeros(B, T, 2 * V + 1)
    xs[:, :, :V] = torch.randn(B, T, V, generator=g)
    cnt = torch.randint(0, 20, (B, T, V), generator=g).float()
    cnt[torch.rand(B, T, V, generator=g) < 0.15] = 2.7
    cnt[torch.rand(B, T, V, generator=g) < 0.1] = 15.9
    cnt[torch.rand(B, T, V, generator=g) < 0.1] = -0.5
    cnt[torch.rand(B, T, V, generator=g) < 0.1] = 1e6
    cnt[torch.rand(B, T, V, generator=g) < 0.15] = -1.0
    cnt[0, :, V - 1] = -1.0                                       # the SSL batch's masked event: every timestep of one variable
    cnt[B - 1, 0, 0] = -1.0                                       # masked at timestep 0 only
    xs[:, :, V:2 * V] = cnt
    xs[:, :, 2 * V] = (torch.rand(B, T, generator=g) < 0.3).float()
    xs[0, T - 1, 2 * V] = 1.0                                     # masked timestep across the masked event and the static column
    if T > 1:
        xs[B - 1, 0, 2 * V] = 0.0
    return xs


def embed_inputs(xs, table):
    """xs [B, T, 2V+1], table [rows, 1] -> [V, B*T, 2]: (value, table[clip(int(count))]) as duett_ref.build_psi pairs them."""
    B, T, Fd = xs.shape
    V = (Fd - 1) // 2
    idx = xs[:, :, V:2 * V].to(torch.int64).clip(0, table.shape[0] - 1)
    n_obs = table[idx].squeeze(-1)
    return torch.stack((xs[:, :, :V], n_obs.to(xs.dtype)), dim=-1).permute(2, 0, 1, 3).reshape(V, B * T, 2)


def embed_indices(xs, rows):
    B, T, Fd = xs.shape
    V = (Fd - 1) // 2
    return xs[:, :, V:2 * V].to(torch.int64).clip(0, rows - 1).permute(2, 0, 1).reshape(V, B * T)


def psi_assemble(xs, var_out, tab_out, special):
    """The assembly half of duett_ref.build_psi: var_out [V, B*T, E], tab_out [B, E], special [>= 2, E] -> psi [B, T+1, V+1, E]."""
    B, T, Fd = xs.shape
    V = (Fd - 1) // 2
    E = special.shape[1]
    psi = torch.zeros((B, T + 1, V + 1, E), dtype=var_out.dtype)
    psi[:, :-1, :V, :] = var_out.view(V, B, T, E).permute(1, 2, 0, 3)
    psi[:, :-1, -1, :] = tab_out.unsqueeze(1)
    psi[:, -1, :, :] = special[1]
    mask_inds = torch.cat((xs[:, :, -1] == 1, torch.zeros((B, 1), dtype=torch.bool)), dim=1)
    psi[mask_inds] = special[0]
    ev = xs[:, :, V:2 * V] == -1
    ev = torch.cat((ev, torch.zeros((B, T, 1), dtype=torch.bool)), dim=2)
    ev = torch.cat((ev, ev[:, :1, :]), dim=1)
    psi[ev] = special[0]
    return psi


def glinear_dw_workspace_bytes_before(G, R, K, N):
    """medp_glinear_bwd_workspace_bytes before the chunk plan looked at K and N (R / 96 chunks, at most 64)."""
    return G * max(1, min(64, R // 96)) * (N * K + N) * 4
