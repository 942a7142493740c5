"""`LocalTrajectoryEncoder` (reference models/main_architecture_duett.py:1242-1391) on the HIP kernels:
per-variable local features -> Linear(5, d) + GELU + LayerNorm + variable / hour embeddings -> a shared GRU over the B*V
sequences -> one token per (variable, recency window) + REP, with the key-padding mask of windows that saw no observation.

Same constructor, parameter names (`input_proj.0/2`, `variable_embedding`, `hour_embedding`, `temporal.weight_ih_l0` ...,
`window_embedding`, `output_norm`, `rep_token`) and outputs as the reference class, so a state_dict moves either way.
What runs where: features (sequential scan), GRU recurrence forward / backward = csrc/trajectory.hip; the two Linears = bf16
MFMA GEMMs (autograd_ops.linear, weight gradients by the transposed GEMM); GELU, LayerNorms = the kernels the fusion head
uses; embeddings, window means, concatenations and the mask = torch index / elementwise plumbing.  `nn.GRU` is only the
parameter container.  Hidden size 128 (the module's default `d_model`) is what the GRU kernels are built for.
`n_layers > 1` (torch's stacked GRU: layer k reads every hidden state of layer k - 1, dropout between the layers in training) is
ONE autograd node, `GruStackFn`: a layer hands its hidden states on as the bf16 tensor its recurrence kernel writes from registers,
dropout mask applied, which is also the operand of the upper layer's dW_ih; `n_layers = 1` is the one-layer node `GruFn` unchanged.
Parity: tests/test_gpu_trajectory.py against oracle/trajectory_ref.py, itself pinned by the reference's own class."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import autograd_ops as A
from . import functional as Fn
from .abi import check, lib, ptr, stream

F32, BF16 = torch.float32, torch.bfloat16


def traj_features(x: torch.Tensor, n_vars: int) -> torch.Tensor:
    """x [B,T,2V] fp32 -> [B*V, T, 8] fp32 (five features, zero padded)."""
    B, T, C = x.shape
    xc = x.detach().to(F32).contiguous()
    out = torch.empty((B * n_vars, T, 8), dtype=F32, device=x.device)
    check(lib().medp_traj_features(ptr(xc), ptr(out), B, T, n_vars, stream()), "traj_features")
    return out


def _gru_weight_t_bf16(w_hh: torch.Tensor) -> torch.Tensor:
    """W_hh^T as the backward kernel reads it: bf16 whatever the precision mode (it is bf16 MFMA only; the fp32 mode's cached
    operand is fp32 and would be read as garbage)."""
    if Fn.precision() != "fp32":
        return A.weight_t_bf16(w_hh)
    return Fn.transpose_to_bf16(w_hh.detach().contiguous())


def _gru_bwd_layer(dh, gates, hn, hseq, w_hh, want_dgi16):
    """One layer's BPTT -> dgi [S,T,3d] fp32 (with its bf16 copy if asked), dW_hh, db_hh."""
    S, T, d = hseq.shape
    dgi = torch.empty((S, T, 3 * d), dtype=F32, device=dh.device)
    dghn = torch.empty((S, T, d), dtype=F32, device=dh.device)
    dgh16 = torch.empty((S, T, 3 * d), dtype=BF16, device=dh.device)
    dgi16 = torch.empty((S, T, 3 * d), dtype=BF16, device=dh.device) if want_dgi16 else None
    wt = _gru_weight_t_bf16(w_hh)
    if want_dgi16:
        check(lib().medp_gru_bwd_dgi16(ptr(dh), ptr(gates), ptr(hn), ptr(hseq), ptr(wt), ptr(dgi), ptr(dghn), ptr(dgh16), ptr(dgi16),
                                       S, T, d, stream()), "gru_bwd_dgi16")
    else:
        check(lib().medp_gru_bwd(ptr(dh), ptr(gates), ptr(hn), ptr(hseq), ptr(wt), ptr(dgi), ptr(dghn), ptr(dgh16), S, T, d, stream()), "gru_bwd")
    hprev = torch.zeros_like(hseq)                   # dW_hh = sum over (sequence, step) of dgh^T h_{t-1}; h_{-1} = 0
    hprev[:, 1:] = hseq[:, :-1]
    dw = Fn.gemm_tn(dgh16.view(S * T, 3 * d), Fn.to_bf16(hprev.view(S * T, d)))
    db = torch.cat([Fn.colsum(dgi.view(S * T, 3 * d))[:2 * d], Fn.colsum(dghn.view(S * T, d))])
    return dgi, dgi16, dw, db


class GruFn(torch.autograd.Function):
    """gi [S,T,3d] fp32 (x_t W_ih^T + b_ih), W_hh [3d,d], b_hh [3d] -> every hidden state [S,T,d]; h0 = 0."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh):
        S, T, d3 = gi.shape
        d = d3 // 3
        gi = gi.contiguous()
        need = gi.requires_grad or w_hh.requires_grad or b_hh.requires_grad
        hseq = torch.empty((S, T, d), dtype=F32, device=gi.device)
        gates = torch.empty((S, T, d3), dtype=F32, device=gi.device) if need else None
        hn = torch.empty((S, T, d), dtype=F32, device=gi.device) if need else None
        if Fn.precision() == "fp32":                 # fp32 weights and products; the backward below stays the bf16 kernel
            wt = A.weight_t_bf16(w_hh)               # (fp32 mode: the fp32 [d, 3d] transpose)
            check(lib().medp_gru_fwd_f32(ptr(gi), ptr(wt), wt.stride(0), ptr(b_hh.detach().contiguous()), ptr(hseq), ptr(gates), ptr(hn),
                                         S, T, d, stream()), "gru_fwd_f32")
        else:
            check(lib().medp_gru_fwd(ptr(gi), ptr(A.weight_bf16(w_hh)), ptr(b_hh.detach().contiguous()), ptr(hseq), ptr(gates), ptr(hn),
                                     S, T, d, stream()), "gru_fwd")
        ctx.save_for_backward(gates, hn, hseq, w_hh)
        return hseq

    @staticmethod
    def backward(ctx, dh):
        gates, hn, hseq, w_hh = ctx.saved_tensors
        dgi, _, dw, db = _gru_bwd_layer(dh.contiguous(), gates, hn, hseq, w_hh, False)
        return dgi, dw, db


# RNG stream id of the dropout between GRU layers k and k + 1: 80 + k (the encoder's input dropout is 0, the probe has 70-73, the
# perceiver and the heads 0-50, DuETT's augmentation 200-202)
_SID_GRU_LAYER = 80


class GruStackFn(torch.autograd.Function):
    """torch's stacked GRU (num_layers = L > 1, batch_first, h0 = 0) as one node.  gi [S,T,3d] fp32 = layer 0's x_t W_ih^T + b_ih;
    `params` = W_hh, b_hh of layer 0, then W_ih, W_hh, b_ih, b_hh of every upper layer -> the hidden states of the LAST layer.
    `p` > 0: dropout on the output of every layer but the last, stream id 80 + k on the flat index of [S,T,d], drawn inside the
    recurrence kernel as it writes the bf16 hand-over `x16` (the next layer's input and its dW_ih operand).  Saved per layer: gates,
    hn, hseq (what one layer saves) + that one bf16 [S,T,d].  An upper layer's input product is A.linear's GEMM on the bf16 hand-over;
    fp32 mode: fp32 GEMM + medp_gru_fwd_f32 per layer on fp32 hand-overs.
    Backward, top down: medp_gru_bwd(_dgi16); dW_ih = dgi^T x16 (transposed GEMM), db_ih = column sums, dx = dgi W_ih times the same
    mask = the layer below's dh."""

    @staticmethod
    def forward(ctx, gi, p, seed, *params):
        S, T, d3 = gi.shape
        d = d3 // 3
        L = 1 + (len(params) - 2) // 4
        layers = [(None, params[0], None, params[1])] + [tuple(params[2 + 4 * (k - 1):2 + 4 * k]) for k in range(1, L)]
        fp32 = Fn.precision() == "fp32"
        need = gi.requires_grad or any(q.requires_grad for q in params)
        dev = gi.device
        gi = gi.contiguous()
        saved, x = [], None
        for k, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
            last = k == L - 1
            hseq = torch.empty((S, T, d), dtype=F32, device=dev)
            gates = torch.empty((S, T, d3), dtype=F32, device=dev) if need else None
            hn = torch.empty((S, T, d), dtype=F32, device=dev) if need else None
            bh, sid = b_hh.detach().contiguous(), _SID_GRU_LAYER + k
            xin = x
            if fp32:
                if k:
                    gi = Fn.gemm(x.view(S * T, d), A.weight_bf16(w_ih), bias=b_ih.detach().contiguous()).view(S, T, d3)
                wt = A.weight_t_bf16(w_hh)
                check(lib().medp_gru_fwd_f32(ptr(gi), ptr(wt), wt.stride(0), ptr(bh), ptr(hseq), ptr(gates), ptr(hn), S, T, d, stream()),
                      "gru_fwd_f32")
                x = hseq
                if not last and p > 0:
                    x = torch.empty_like(hseq)
                    check(lib().medp_dropout_add(ptr(hseq), None, ptr(x), hseq.numel(), p, seed, sid, stream()), "dropout")
            else:
                x = None if last else torch.empty((S, T, d), dtype=BF16, device=dev)
                if k:
                    gi = Fn.gemm(xin.view(S * T, d), A.weight_bf16(w_ih), bias=b_ih.detach().contiguous()).view(S, T, d3)
                if last:
                    check(lib().medp_gru_fwd(ptr(gi), ptr(A.weight_bf16(w_hh)), ptr(bh), ptr(hseq), ptr(gates), ptr(hn), S, T, d, stream()),
                          "gru_fwd")
                else:
                    check(lib().medp_gru_fwd_h16(ptr(gi), ptr(A.weight_bf16(w_hh)), ptr(bh), ptr(hseq), ptr(gates), ptr(hn), ptr(x),
                                                 p, seed, sid, S, T, d, stream()), "gru_fwd_h16")
            saved += [gates, hn, hseq, xin]
            gi = None
        ctx.save_for_backward(*saved, *params)
        ctx.cfg = (L, p, seed)
        return hseq

    @staticmethod
    def backward(ctx, dh):
        L, p, seed = ctx.cfg
        saved, params = ctx.saved_tensors[:4 * L], ctx.saved_tensors[4 * L:]
        fp32 = Fn.precision() == "fp32"
        grads = [None] * len(params)
        dh = dh.contiguous()
        for k in range(L - 1, -1, -1):
            gates, hn, hseq, xin = saved[4 * k:4 * k + 4]
            S, T, d = hseq.shape
            w_hh = params[0] if k == 0 else params[2 + 4 * (k - 1) + 1]
            dgi, dgi16, dw_hh, db_hh = _gru_bwd_layer(dh, gates, hn, hseq, w_hh, bool(k) and not fp32)
            if k == 0:
                grads[0], grads[1] = dw_hh, db_hh
                break
            base = 2 + 4 * (k - 1)
            w_ih = params[base]
            g2 = (dgi if fp32 else dgi16).view(S * T, 3 * d)
            grads[base], grads[base + 1] = Fn.gemm_tn(g2, xin.view(S * T, d)), dw_hh
            grads[base + 2], grads[base + 3] = Fn.colsum(dgi.view(S * T, 3 * d)), db_hh
            dx = Fn.gemm(g2, A.weight_t_bf16(w_ih), out_dtype=F32, k=3 * d)
            if p > 0:                                # the mask the layer below applied to its hand-over (same seed, stream id, index)
                dxm = torch.empty_like(dx)
                check(lib().medp_dropout_add(ptr(dx), None, ptr(dxm), dx.numel(), p, seed, _SID_GRU_LAYER + k - 1, stream()), "dropout(bwd)")
                dx = dxm
            dh = dx.view(S, T, d)
        return (dgi, None, None, *grads)


class LocalTrajectoryEncoder(nn.Module):
    """Drop-in for the reference class (same arguments, defaults and errors, :1261-1309)."""

    def __init__(self, n_vars: int, n_timesteps: int = 24, d_model: int = 128, n_layers: int = 1, dropout: float = 0.1,
                 recency_windows: tuple = (6, 12, 24)):
        super().__init__()
        if n_vars <= 0 or n_timesteps <= 0 or d_model <= 0:
            raise ValueError("n_vars, n_timesteps, and d_model must be positive")
        windows = tuple(sorted(set(int(w) for w in recency_windows)))
        if not windows or windows[-1] != n_timesteps:
            raise ValueError(f"recency_windows must end at n_timesteps={n_timesteps}, got {windows}")
        if windows[0] <= 0 or windows[-1] > n_timesteps:
            raise ValueError(f"invalid recency_windows={windows}")
        self.n_layers = int(n_layers)
        self.n_vars, self.n_timesteps, self.d_model, self.recency_windows = n_vars, n_timesteps, d_model, windows
        self.p_drop = float(dropout)
        self.input_proj = nn.Sequential(nn.Linear(5, d_model), nn.GELU(), nn.LayerNorm(d_model))
        self.variable_embedding = nn.Embedding(n_vars, d_model)
        self.hour_embedding = nn.Embedding(n_timesteps, d_model)
        self.temporal = nn.GRU(input_size=d_model, hidden_size=d_model, num_layers=n_layers, batch_first=True,
                               dropout=dropout if n_layers > 1 else 0.0)                                 # parameters only
        self.window_embedding = nn.Embedding(len(windows), d_model)
        self.output_norm = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.rep_token = nn.Parameter(torch.randn(1, 1, d_model) * 0.02)

    @property
    def d_representation(self) -> int:
        return self.d_model

    def forward(self, x_ts_list, return_padding_mask: bool = False):
        x = torch.stack(tuple(x_ts_list), dim=0)
        if x.ndim != 3:
            raise ValueError(f"x_ts must stack to [B,T,2V], got {tuple(x.shape)}")
        B, T, C = x.shape
        V, d = self.n_vars, self.d_model
        if T != self.n_timesteps or C != 2 * V:
            raise ValueError(f"expected [B,{self.n_timesteps},{2 * V}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("LocalTrajectoryEncoder runs on the GPU only (there is no CPU fallback)")
        local = traj_features(x, V)                                               # [B*V, T, 8]
        w0 = torch.nn.functional.pad(self.input_proj[0].weight, (0, 3))           # Linear(5, d) as a K = 8 GEMM
        h = A.linear(local.view(B * V * T, 8), w0, self.input_proj[0].bias)
        h = A.gelu_dropout(h, 0.0, 0, 0)
        h = A.layer_norm(h, self.input_proj[2].weight, self.input_proj[2].bias, self.input_proj[2].eps).view(B, V, T, d)
        h = h + self.variable_embedding.weight.view(1, V, 1, d) + self.hour_embedding.weight[:T].view(1, 1, T, d)
        if self.training and self.p_drop > 0:
            h = A.DropoutFn.apply(h.contiguous().view(-1, d), self.p_drop, A.next_seed(), 0).view(B, V, T, d)
        gi = A.linear(h.reshape(B * V * T, d), self.temporal.weight_ih_l0, self.temporal.bias_ih_l0).view(B * V, T, 3 * d)
        if self.n_layers == 1:
            hs = GruFn.apply(gi, self.temporal.weight_hh_l0, self.temporal.bias_hh_l0)                # [B*V, T, d]
        else:
            g, p = self.temporal, self.p_drop if self.training else 0.0
            upper = [getattr(g, f"{n}_l{k}") for k in range(1, self.n_layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            hs = GruStackFn.apply(gi, p, A.next_seed() if p > 0 else 0, g.weight_hh_l0, g.bias_hh_l0, *upper)
        # non-overlapping windows measured backwards from the CXR anchor (:1370-1381)
        obs = (x[:, :, V:] > 0).permute(0, 2, 1)                                  # [B,V,T]
        pooled, valid, prev = [], [], 0
        for wi, boundary in enumerate(self.recency_windows):
            s, e = T - boundary, T - prev
            pooled.append(hs[:, s:e, :].mean(dim=1) + self.window_embedding.weight[wi])
            valid.append(obs[:, :, s:e].any(dim=-1))
            prev = boundary
        W = len(self.recency_windows)
        tokens = torch.stack(pooled, dim=1)                                       # [B*V, W, d]
        tokens = A.layer_norm(tokens.reshape(B * V * W, d), self.output_norm.weight, self.output_norm.bias, self.output_norm.eps)
        tokens = torch.cat([tokens.view(B, V * W, d), self.rep_token.expand(B, -1, -1)], dim=1)
        if not return_padding_mask:
            return tokens
        pad = ~torch.cat([torch.stack(valid, dim=2).reshape(B, -1), torch.ones((B, 1), dtype=torch.bool, device=x.device)], dim=1)
        return tokens, pad
