"""Time-series-only pathology probe over the trajectory encoder: mirror of `TrajectoryPathologyProbe`, `masked_bce` and the
`train_epoch` / `evaluate` bodies of the reference's analysis/train_trajectory_probe.py (:98-262) — the only live consumer of
`LocalTrajectoryEncoder`.  Encoder -> (variable, recency-window) tokens, REP dropped -> ONE cross-attention
block of the pathology queries over those tokens under the encoder's key-padding mask (a window without an observation still
yields a token; the queries must not see it) -> feed-forward -> per-query head + label bias.

Same constructor, parameter names and shapes as the reference class, so a state_dict moves either way.  What runs where: the
encoder = trajectory.py; LayerNorms, the packed in-projection, the Linears (bf16 MFMA GEMMs), GELU + dropout and the Linear(64, 1)
row dot = the kernels the fusion head uses; the attention = the key-masked wave-per-query kernels (csrc/attention_small.hip).
`nn.MultiheadAttention` is only the parameter container.  The global-norm clip of the reference step lives in the optimiser
(`FusedAdamW(max_grad_norm=...)`).  Parity: tests/test_gpu_trajectory_probe.py against the reference's own class."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import autograd_ops as A
from . import evaluator
from .main_architecture_duett import _BroadcastRowsFn
from .trajectory import LocalTrajectoryEncoder

_SID_ATTN, _SID_FF, _SID_FF2, _SID_HEAD = 70, 71, 72, 73


class TrajectoryPathologyProbe(nn.Module):
    def __init__(self, n_vars: int, n_pathologies: int, n_timesteps: int, d_model: int, gru_layers: int, n_heads: int, dropout: float,
                 recency_windows: tuple):
        super().__init__()
        self.encoder = LocalTrajectoryEncoder(n_vars=n_vars, n_timesteps=n_timesteps, d_model=d_model, n_layers=gru_layers,
                                              dropout=dropout, recency_windows=recency_windows)
        self.pathology_queries = nn.Parameter(torch.randn(n_pathologies, d_model) * 0.02)
        self.norm_q = nn.LayerNorm(d_model)
        self.norm_kv = nn.LayerNorm(d_model)
        self.cross_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)      # parameters only
        self.norm_ff = nn.LayerNorm(d_model)
        self.ff = nn.Sequential(nn.Linear(d_model, 4 * d_model), nn.GELU(), nn.Dropout(dropout), nn.Linear(4 * d_model, d_model),
                                nn.Dropout(dropout))
        self.head = nn.Sequential(nn.LayerNorm(d_model), nn.Linear(d_model, 64), nn.GELU(), nn.Dropout(dropout), nn.Linear(64, 1))
        self.label_bias = nn.Parameter(torch.zeros(n_pathologies))

    def forward(self, x_ts_list, return_attn: bool = False):
        tokens, pad = self.encoder(x_ts_list, return_padding_mask=True)
        tokens, pad = tokens[:, :-1], pad[:, :-1]                # the REP token and its mask column are not used (:150-153)
        B, d = tokens.shape[0], tokens.shape[-1]
        mha, H = self.cross_attn, self.cross_attn.num_heads
        p = float(mha.dropout) if self.training else 0.0
        seed = A.next_seed() if p > 0 else 0
        q0 = _BroadcastRowsFn.apply(self.pathology_queries, B)
        # the queries are the same rows for every sample: norm_q and the Q projection run once; norm_kv(tokens) once for K and V
        qn = A.layer_norm(self.pathology_queries, self.norm_q.weight, self.norm_q.bias, self.norm_q.eps, lowp=True)
        kn = A.layer_norm(tokens, self.norm_kv.weight, self.norm_kv.bias, self.norm_kv.eps, lowp=True)
        Q, KV = A.in_proj(qn, kn, mha.in_proj_weight, mha.in_proj_bias, d)
        o, attn = A.attn_small(Q, KV, H, (d // H) ** -0.5, p, seed, _SID_ATTN, 0, return_attn, key_mask=pad)
        q = A.linear(o, mha.out_proj.weight, mha.out_proj.bias, residual=q0)
        h = A.layer_norm(q, self.norm_ff.weight, self.norm_ff.bias, self.norm_ff.eps, lowp=True)
        h = A.gelu_dropout(A.linear(h, self.ff[0].weight, self.ff[0].bias), p, seed, _SID_FF, lowp=True)
        if p > 0:
            q = A.dropout_add(A.linear(h, self.ff[3].weight, self.ff[3].bias), q, p, seed, _SID_FF2)
        else:
            q = A.linear(h, self.ff[3].weight, self.ff[3].bias, residual=q)
        h = A.layer_norm(q, self.head[0].weight, self.head[0].bias, self.head[0].eps)
        h = A.gelu_dropout(A.linear(h, self.head[1].weight, self.head[1].bias), p, seed, _SID_HEAD)
        logits = A.rowdot(h, self.head[4].weight, self.head[4].bias) + self.label_bias.unsqueeze(0)
        return (logits, attn) if return_attn else logits


def masked_bce(logits, y, mask):
    """:170-174: sum(bce * mask) / clamp_min(sum(mask), 1).  The kernel clamps the denominator on the device, so a batch with
    no labelled entry gives 0 (and a zero gradient) without a host-side test."""
    return A.masked_bce_global(logits, y, mask)


def train_probe_batch(model, batch: dict, optimizer) -> dict:
    """One step of the reference's `train_epoch` body (:205-215) on a batch already on the device ("x_ts", "y", "mask").  The
    clip of :214 is the optimiser's: pass `FusedAdamW(..., max_grad_norm=args.grad_clip)`."""
    optimizer.zero_grad(set_to_none=True)
    loss = masked_bce(model(batch["x_ts"]), batch["y"], batch["mask"])
    loss.backward()
    optimizer.step()
    return {"loss": loss.detach()}


def move_batch(batch: dict, device) -> dict:
    """Cohort collate layout ("x_ts" tuple, "y_multi", "y_multi_mask") or the reference's ("y", "mask") -> device tensors."""
    y, mask = ("y_multi", "y_multi_mask") if "y_multi" in batch else ("y", "mask")
    x = batch["x_ts"]
    x = x if torch.is_tensor(x) else torch.stack(tuple(x))
    return {"x_ts": x.to(device, non_blocking=True), "y": batch[y].to(device, non_blocking=True).float(),
            "mask": batch[mask].to(device, non_blocking=True).float()}


@torch.no_grad()
def evaluate(model, loader, device, labels) -> dict:
    """:221-262 with the evaluator's AUROC / AUPRC in place of sklearn's: mean batch BCE, per-label and macro metrics over the
    labelled entries (a label with one class only is NaN and left out of the macro means)."""
    model.eval()
    zs, ys, ms, losses = [], [], [], []
    for raw in loader:
        b = move_batch(raw, device)
        z = model(b["x_ts"])
        losses.append(float(masked_bce(z, b["y"], b["mask"])))
        zs.append(z.float().cpu())
        ys.append(b["y"].cpu())
        ms.append(b["mask"].cpu())
    z, y, m = torch.cat(zs).numpy(), torch.cat(ys).numpy(), torch.cat(ms).numpy().astype(bool)
    prob = 1.0 / (1.0 + np.exp(-np.clip(z, -30.0, 30.0)))
    rows = []
    for k, label in enumerate(labels):
        yk, pk = y[m[:, k], k], prob[m[:, k], k]
        two = yk.size > 0 and np.unique(yk).size == 2
        rows.append({"label": label, "n": int(m[:, k].sum()), "pos": int(yk.sum()),
                     "auroc": float(evaluator.auroc(yk, pk)) if two else float("nan"),
                     "auprc": float(evaluator.average_precision(yk, pk)) if two else float("nan")})

    def macro(key):
        v = [r[key] for r in rows if np.isfinite(r[key])]
        return float(np.mean(v)) if v else float("nan")
    return {"loss": float(np.mean(losses)), "macro_auroc": macro("auroc"), "macro_auprc": macro("auprc"), "per_label": rows}
