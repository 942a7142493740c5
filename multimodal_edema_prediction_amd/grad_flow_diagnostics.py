"""Gradient-flow diagnostics of a trained dual teacher: the device-side counterpart of the reference's
`analysis/grad_flow_diagnostics.py`.  Which of the three heads (image, time series, fusion) drives the shared pathology queries: do
the image and the time-series head pull them in opposing directions, and how sensitive is the fusion loss to each modality's tokens?

    python -m multimodal_edema_prediction_amd.grad_flow_diagnostics --ckpt runs/t0/best.pt --outdir runs/t0/grad_diag --split train

The contract is THE SCRIPT'S ARITHMETIC ON THE MODEL AS THE REFERENCE'S MODEL FILE DEFINES IT and as this package mirrors it, with the
reference's public names, signatures and report dictionary (keys, nesting, types).  Two deviations, both forced by the reference's
HEAD: its `_find_pathology_query_banks` looks for `image_queries` + `temporal_queries` or one `pathology_queries` and so does not
find the live model's `shared_queries` (it raises); and the script imports `analysis/visualize_pathology.py`, which is not ported.
Here `shared_queries` of a `PatchDualPathologyPerceiver` is accepted as the one shared bank (`query_layout: "shared"`,
`query_parameter: "perceiver.shared_queries"`, own bank 0 for all three branches); every other perceiver, the `dual` mode's
`DualPathologyPerceiver` included (it has no image tokens), raises the reference's RuntimeError text.  The CLI loads a
`train_synthetic` checkpoint.  `accelerator` other than None raises NotImplementedError (no multi-GPU reduction).

Layered entry points
  run_dual_gradient_diagnostics   the reference's signature.  Both encoders run ONCE per batch under no_grad (frozen CXR tokens,
                                  DuETT tokens, `img_proj`), then the perceiver-level core takes over.
  perceiver_gradient_diagnostics  the core, public so that it can be tested on a tiny perceiver: `batches` yields
                                  (ts_selected, img_patches_proj, img_skip, y_multi, y_multi_mask).
  format_gradient_diagnostics, gradient_diagnostics_to_log_dict     host-only restatements.

One backward instead of 4K + 4.  The reference calls `torch.autograd.grad` 3 (branch totals) + 3K (per-label losses) + 1 + K (token
sensitivities) times per batch, each walking the whole perceiver.  Branch totals are sum_k lw_k per_k, so their gradients are sums
of the per-label ones; and in eval mode the cross block (cross attention, LayerNorm, linears, FF) treats query rows independently.
So the query bank is replicated G times into a detached leaf `q_rep [G K, D]`, the cross block runs with G K queries per sample, its
result [B, G K, D] is viewed as [B G, K, D] for the self block and the heads, and replica g = (branch, label) is seeded with that
label's loss cotangent only: `q_rep.grad.view(G, K, D)[g]` IS d(lw_k per_k^branch) / d queries, and the token gradients of the fusion
replicas are the per-label token gradients.  The image half takes K replicas, the time-series half 2K (ts and fusion; fusion needs no
image branch because `img_logits` is detached in `fusion_logits`).  Above 1536 keys the split-key attention takes at most 32 queries:
the replicas are then processed in chunks of floor(32 / K).

Model state: eval mode for the pass, every submodule's train / eval flag restored on exit (also on error).  The leaf is the detached replica: no
`.grad` of a model parameter is written.  While the core runs, the perceiver's parameters have `requires_grad` off (restored on exit),
so that no autograd node computes a weight gradient nobody asked for.

Where the work runs: `medp_grad_flow_seeds` (losses + cotangents; the BCE rule is `medp_dual_pathology_loss`'s),
`medp_grad_flow_accumulate` (one call per batch into an fp64 device state), `medp_grad_flow_report` and `medp_query_geometry` at the
end.  Everything accumulated stays on the device; the run synchronises ONCE, with one device-to-host copy of the report vector and
the three K x K Gram matrices.  `_looped_reference` evaluates the same report by the reference's literal procedure on the public
`teacher(..., return_attn=True)`; it is the baseline of the equivalence test and of tools/time_grad_flow.py, never the default path.
Without a GPU everything that reaches a kernel raises (no CPU fallback)."""
from __future__ import annotations

import argparse
import json
import os
from typing import Any, Dict, Iterable, Mapping, Optional, Sequence

import torch

from .abi import check, lib, ptr, require_gpu, stream

F32, F64 = torch.float32, torch.float64
BRANCHES = ("img", "ts", "fus")
SENSITIVITY_KEYS = ("img_raw", "ts_raw", "img_scaled", "ts_scaled")
REPORT_HEAD, REPORT_PER_LABEL = 26, 16           # MEDP_GRAD_FLOW_REPORT_HEAD / _PER_LABEL
SPLIT_KEY_MIN_KEYS, SPLIT_KEY_MAX_QUERIES = 1536, 32


# ------------------------------------------------------------------------------------------------------------------------------
# the query bank
# ------------------------------------------------------------------------------------------------------------------------------
def _unwrap_model(model: torch.nn.Module) -> torch.nn.Module:
    while hasattr(model, "module"):
        model = model.module
    return model


def _find_pathology_query_banks(model: torch.nn.Module):
    """-> ((name,), (parameter,)): the `shared_queries` of a patch-dual perceiver.  Anything else: the reference's RuntimeError."""
    named = dict(model.named_parameters())
    perceiver = getattr(model, "perceiver", None)
    if perceiver is not None and all(hasattr(perceiver, a) for a in ("img_cross", "ts_cross", "shared_queries")):
        found = [(n, p) for n, p in named.items() if n.endswith("shared_queries")]
        if len(found) == 1:
            return (found[0][0],), (found[0][1],)
    count = lambda suffix: sum(1 for n in named if n.endswith(suffix))  # noqa: E731
    raise RuntimeError("Expected image_queries + temporal_queries, or one legacy "
                       f"pathology_queries; found image={count('image_queries')}, temporal={count('temporal_queries')}, "
                       f"shared={count('pathology_queries')}")


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
def state_size(K: int, D: int) -> int:
    n = int(lib().medp_grad_flow_state_doubles(K, D))
    if n == 0:
        raise ValueError(f"grad_flow: K = {K}, D = {D} outside the kernels' range")
    return n


def grad_flow_seeds(img, ts, fus, y, mask, label_weights, pos_weight, eps: float):
    """Logits [B, K] x 3 -> (losses [3, K] = lw_k per_k, cot_img [B, K, K], cot_ts [B, 2K, K], cot_fus [B, 2K, K]); include/medp_hip.h."""
    img, ts, fus, y, mask = (t.detach().contiguous().to(F32) for t in (img, ts, fus, y, mask))
    B, K = img.shape
    dev = img.device
    ws = torch.empty(4 + 3 * K + 3 * B * K, dtype=F32, device=dev)
    losses = torch.empty((3, K), dtype=F32, device=dev)
    cot_img = torch.empty((B, K, K), dtype=F32, device=dev)
    cot_ts, cot_fus = (torch.empty((B, 2 * K, K), dtype=F32, device=dev) for _ in range(2))
    check(lib().medp_grad_flow_seeds(ptr(img), ptr(ts), ptr(fus), ptr(y), ptr(mask), ptr(label_weights), ptr(pos_weight), float(eps), ptr(ws),
                                     ptr(losses), ptr(cot_img), ptr(cot_ts), ptr(cot_fus), B, K, stream()), "grad_flow_seeds")
    return losses, cot_img, cot_ts, cot_fus


def grad_flow_accumulate(state, dq, dI, dT, I, T, mask, losses) -> None:
    """One batch into `state` (fp64 [state_size(K, D)], zeroed by the caller); dI may be None (= zeros)."""
    B, K, D = T.shape
    ws = torch.empty(int(lib().medp_grad_flow_ws_doubles(B, K)), dtype=F64, device=state.device)
    check(lib().medp_grad_flow_accumulate(ptr(dq), ptr(dI), ptr(dT), ptr(I), ptr(T), ptr(mask), ptr(losses), ptr(state), ptr(ws), B, K, D,
                                          stream()), "grad_flow_accumulate")


def grad_flow_report(state, alphas, out, K: int, D: int) -> None:
    check(lib().medp_grad_flow_report(ptr(state), float(alphas[0]), float(alphas[1]), float(alphas[2]), ptr(out), K, D, stream()),
          "grad_flow_report")


def query_geometry(rows, out) -> None:
    """rows [3, K, D] fp32 -> out fp64 [3 K K + K + 1]."""
    check(lib().medp_query_geometry(ptr(rows), ptr(out), rows.shape[1], rows.shape[2], stream()), "query_geometry")


def _effective_queries(block, prototypes):
    """`norm_q` followed by the Q slice of the packed `in_proj`, through the package's own ops."""
    from . import autograd_ops as A
    d = prototypes.shape[-1]
    attn = block.attn
    if attn.in_proj_weight is None:
        raise RuntimeError("The diagnostic currently expects MultiheadAttention with a packed in_proj_weight.")
    normalized = A.layer_norm(prototypes, block.norm_q.weight, block.norm_q.bias, block.norm_q.eps)
    bias = None if attn.in_proj_bias is None else attn.in_proj_bias[:d]
    return A.linear(normalized, attn.in_proj_weight[:d], bias)


def report_from_vector(vec, n_labels: int, label_names: Sequence[str], alphas: Sequence[float], query_name: str) -> Dict[str, Any]:
    """The host half: the kernels' fp64 vector (report, then Gram matrices, prototype norms, gap) -> the reference's dictionary."""
    K = n_labels
    v = [float(x) for x in vec]
    branch = {name: {"loss": v[4 * r], "alpha": float(alphas[r]), "raw_grad_norm": v[4 * r + 1], "weighted_grad_norm": v[4 * r + 2],
                     "cos_to_total_update": v[4 * r + 3]} for r, name in enumerate(BRANCHES)}
    sensitivity = {key: v[18 + i] for i, key in enumerate(SENSITIVITY_KEYS)}
    sensitivity["raw_img_over_ts"], sensitivity["scaled_img_over_ts"] = v[22], v[23]
    per_label = []
    for k, name in enumerate(label_names):
        o = v[REPORT_HEAD + REPORT_PER_LABEL * k:REPORT_HEAD + REPORT_PER_LABEL * (k + 1)]
        label_sensitivity = {key: o[11 + i] for i, key in enumerate(SENSITIVITY_KEYS)}
        label_sensitivity["scaled_img_over_ts"] = o[15]
        per_label.append({"label": str(name), "valid_samples": int(round(o[0])), "img_grad_norm": o[1], "ts_grad_norm": o[2],
                          "fus_grad_norm": o[3], "img_ts_cos": o[4], "img_fus_cos": o[5], "ts_fus_cos": o[6],
                          "weighted_total_grad_norm": o[7], "img_own_query_fraction": o[8], "ts_own_query_fraction": o[9],
                          "fus_own_query_fraction": o[10], "fusion_token_sensitivity": label_sensitivity})
    g0 = REPORT_HEAD + REPORT_PER_LABEL * K
    gram = lambda s: [[v[g0 + (s * K + i) * K + j] for j in range(K)] for i in range(K)]  # noqa: E731
    return {"query_parameter": query_name, "query_layout": "shared", "batches": int(round(v[24])), "samples": int(round(v[25])),
            "branch": branch,
            "pairwise_gradient_cosine": {"img_ts": v[12], "img_fus": v[13], "ts_fus": v[14], "img_ts_batch_mean": v[15],
                                         "img_ts_negative_batch_fraction": v[16]},
            "weighted_img_over_ts": v[17], "fusion_token_sensitivity": sensitivity, "per_label": per_label,
            "query_geometry": {"prototype_norms": v[g0 + 3 * K * K:g0 + 3 * K * K + K], "raw_cosine": gram(0),
                               "image_effective_cosine": gram(1), "ts_effective_cosine": gram(2),
                               "image_ts_gram_gap": v[g0 + 3 * K * K + K]}}


# ------------------------------------------------------------------------------------------------------------------------------
# the replicated pass
# ------------------------------------------------------------------------------------------------------------------------------
def _replica_leaf(queries, G: int):
    return queries.detach().repeat(G, 1).requires_grad_(True)


def _image_forward(pc, img_kv, skip: int, G: int):
    """G replicas of the image half -> (q_rep, I [B G, K, D], hi [B G, K], img_logits [B G, K])."""
    from . import autograd_ops as A
    from .main_architecture_duett import _SID, _BroadcastRowsFn
    B = img_kv.shape[0]
    K, D = pc.shared_queries.shape
    q_rep = _replica_leaf(pc.shared_queries, G)
    q0 = _BroadcastRowsFn.apply(q_rep, B)
    I = pc.img_cross(q0, img_kv, True, _kv_skip=skip, _shared_q=q_rep, _seed=0)[0].reshape(B * G, K, D)     # return_attn: see _ts_forward
    I = pc.img_self(I, I, _seed=0)
    hi = pc._head(I, pc.image_head, 0, _SID["image_head"])
    zero = torch.zeros_like(hi)
    img_logits = A.FusionLogitsFn.apply(hi, zero, zero, pc.image_label_bias, pc.temporal_label_bias, pc.beta)[0]
    return q_rep, I, hi, img_logits


def _ts_forward(pc, ts_kv, hi0, G: int):
    """G replicas of the time-series half -> (q_rep, T [B G, K, D], ts_logits, fusion_logits [B G, K]).  hi0 [B, K]: the image
    head's output, a constant of the fusion logits."""
    from . import autograd_ops as A
    from .main_architecture_duett import _SID, _BroadcastRowsFn
    B = ts_kv.shape[0]
    K, D = pc.shared_queries.shape
    q_rep = _replica_leaf(pc.shared_queries, G)
    q0 = _BroadcastRowsFn.apply(q_rep, B)
    # return_attn=True as in the forward the reference differentiates: the cross attention then takes the wave-per-query kernels for
    # every replica count, so a chunked pass and the looped form round like the unchunked pass (the average itself is dropped)
    T = pc.ts_cross(q0, ts_kv, True, _shared_q=q_rep, _seed=0)[0].reshape(B * G, K, D)
    T = pc.ts_self(T, T, _seed=0)
    ht = pc._head(T, pc.temporal_head, 0, _SID["temporal_head"])
    ch = pc.correction_head
    c = A.layer_norm(T, ch[0].weight, ch[0].bias, ch[0].eps)
    c = A.linear(c, ch[1].weight, ch[1].bias)
    c = A.gelu_dropout(c, 0.0, 0, _SID["correction_head"])
    hc = A.rowdot(c, ch[4].weight, None)
    hi_rep = hi0.unsqueeze(1).expand(B, G, K).reshape(B * G, K)
    _, ts_logits, _, fusion_logits = A.FusionLogitsFn.apply(hi_rep, ht, hc, pc.image_label_bias, pc.temporal_label_bias, pc.beta)
    return q_rep, T, ts_logits, fusion_logits


def _eval_mode(module):
    """Put `module` in eval mode -> what `_restore_modes` needs to put every submodule back as it was (a teacher in training keeps its
    frozen encoders in eval mode: `train(was_training)` on the root would not restore that)."""
    modes = [(m, m.training) for m in module.modules()]
    module.eval()
    return modes


def _restore_modes(modes) -> None:
    for m, training in modes:
        m.training = training


def _chunks(n: int, size: int):
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _replicas_per_pass(n_keys: int, K: int, forced: Optional[int]) -> Optional[int]:
    if forced is not None:
        return max(1, int(forced))
    return max(1, SPLIT_KEY_MAX_QUERIES // K) if n_keys > SPLIT_KEY_MIN_KEYS else None


def _batch_gradients(pc, ts_selected, img_kv, skip: int, y, mask, loss_fn, chunk: Optional[int], mark):
    """One batch -> (dq [3, K, K, D], dT [B, K, K, D], I, T [B, K, D], losses [3, K]): one forward and one backward per half (per
    chunk of replicas when the key count or `chunk` asks for it)."""
    from . import autograd_ops as A
    K, D = pc.shared_queries.shape
    B = img_kv.shape[0]
    dev = img_kv.device
    with torch.no_grad():
        ts_kv = A.linear(ts_selected, pc.ts_proj.weight, pc.ts_proj.bias)
    per_img = _replicas_per_pass(img_kv.shape[1] - skip, K, chunk) or K
    per_ts = _replicas_per_pass(ts_kv.shape[1], K, chunk) or 2 * K
    img_chunks, ts_chunks = _chunks(K, per_img), _chunks(2 * K, per_ts)
    dq = torch.empty((3, K, K, D), dtype=F32, device=dev)
    dT = torch.empty((B, K, K, D), dtype=F32, device=dev)
    with torch.enable_grad():
        first_img = _image_forward(pc, img_kv, skip, img_chunks[0][1] - img_chunks[0][0])
        G = img_chunks[0][1]
        hi0 = first_img[2].detach().view(B, G, K)[:, 0].contiguous()
        I_tok = first_img[1].detach().view(B, G, K, D)[:, 0].contiguous()
        img_logits = first_img[3].detach().view(B, G, K)[:, 0]
        first_ts = _ts_forward(pc, ts_kv, hi0, ts_chunks[0][1] - ts_chunks[0][0])
        G = ts_chunks[0][1]
        T_tok = first_ts[1].detach().view(B, G, K, D)[:, 0].contiguous()
        ts_logits, fus_logits = (t.detach().view(B, G, K)[:, 0] for t in first_ts[2:])
        mark("forward")
        losses, cot_img, cot_ts, cot_fus = grad_flow_seeds(img_logits, ts_logits, fus_logits, y, mask, loss_fn.label_weights,
                                                           getattr(loss_fn, "pos_weight", None), float(getattr(loss_fn, "eps", 1e-6)))
        mark("seeds")
        for i, (a, b) in enumerate(img_chunks):
            q_rep, _, _, logits = first_img if i == 0 else _image_forward(pc, img_kv, skip, b - a)
            (gq,) = torch.autograd.grad(logits, q_rep, cot_img[:, a:b].reshape(B * (b - a), K))
            dq[0, a:b] = gq.view(b - a, K, D)
        first_img = None
        for i, (a, b) in enumerate(ts_chunks):
            q_rep, T, lt, lf = first_ts if i == 0 else _ts_forward(pc, ts_kv, hi0, b - a)
            G = b - a
            gq, gT = torch.autograd.grad([lt, lf], [q_rep, T], [cot_ts[:, a:b].reshape(B * G, K), cot_fus[:, a:b].reshape(B * G, K)])
            gq, gT = gq.view(G, K, D), gT.view(B, G, K, D)
            if a < K:                                           # time-series replicas a .. min(b, K)
                dq[1, a:min(b, K)] = gq[:min(b, K) - a]
            if b > K:                                           # fusion replicas max(a, K) .. b
                lo = max(a, K)
                dq[2, lo - K:b - K] = gq[lo - a:]
                dT[:, lo - K:b - K] = gT[:, lo - a:]
        mark("backward")
    return dq, dT, I_tok, T_tok, losses


def perceiver_gradient_diagnostics(perceiver, batches, loss_fn, *, label_names: Optional[Sequence[str]] = None,
                                   _chunk: Optional[int] = None, _query_name: str = "perceiver.shared_queries", _collect=None,
                                   _mark=None) -> Dict[str, Any]:
    """The perceiver-level core.  `batches` yields (ts_selected [B, T, d_ts], img_patches_proj [B, skip + P, D], img_skip, y_multi,
    y_multi_mask [B, K]) on the device.  `_chunk` (private): replicas per pass; `_collect` (private): a list that receives every
    batch's (dq, dT); `_mark` (private): called with a stage name at every stage boundary (tools/time_grad_flow.py)."""
    require_gpu()
    pc = perceiver
    mark = _mark or (lambda name: None)
    K, D = pc.shared_queries.shape
    if label_names is None:
        label_names = [f"label_{k}" for k in range(K)]
    if len(label_names) != K:
        raise ValueError(f"label_names has {len(label_names)} entries but queries have {K} rows")
    dev = pc.shared_queries.device
    alphas = tuple(float(getattr(loss_fn, "alpha_" + name, 1.0)) for name in BRANCHES)
    state = torch.zeros(state_size(K, D), dtype=F64, device=dev)
    thawed = [p for p in pc.parameters() if p.requires_grad]
    n_batches = 0
    modes = _eval_mode(pc)
    try:
        for p in thawed:
            p.requires_grad_(False)
        for ts_selected, img_kv, skip, y, mask in batches:
            mask32 = mask.detach().contiguous().to(F32)
            dq, dT, I_tok, T_tok, losses = _batch_gradients(pc, ts_selected, img_kv, int(skip), y, mask32, loss_fn, _chunk, mark)
            grad_flow_accumulate(state, dq, None, dT, I_tok, T_tok, mask32, losses)
            mark("accumulate")
            if _collect is not None:
                _collect.append((dq, dT))
            n_batches += 1
        if n_batches == 0:
            raise RuntimeError("The diagnostic loader yielded no batches")
        n_report = REPORT_HEAD + REPORT_PER_LABEL * K
        out = torch.empty(n_report + 3 * K * K + K + 1, dtype=F64, device=dev)
        grad_flow_report(state, alphas, out, K, D)
        with torch.no_grad():
            prototypes = pc.shared_queries.detach()
            rows = torch.stack([prototypes.float(), _effective_queries(pc.img_cross, prototypes).float(),
                                _effective_queries(pc.ts_cross, prototypes).float()]).contiguous()
        query_geometry(rows, out[n_report:])
    finally:
        for p in thawed:
            p.requires_grad_(True)
        _restore_modes(modes)
    return report_from_vector(out.cpu().tolist(), K, label_names, alphas, _query_name)        # the run's one synchronisation


def _move_batch(batch: Mapping[str, Any], device) -> Dict[str, Any]:
    """The fields the teacher and the loss read, on `device`."""
    moved = {key: tuple(t.to(device) for t in batch[key]) for key in ("x_ts", "x_static", "bin_ends")}
    moved.update({key: batch[key].to(device) for key in ("pixel_values", "y_multi", "y_multi_mask")})
    return moved


def _encoded_batches(model, loader, device, max_batches: int, mark):
    """Per batch: both encoders once, under no_grad -> what the core takes."""
    from . import autograd_ops as A
    pc = model.perceiver
    for index, batch in enumerate(loader):
        if index >= max_batches:
            break
        b = _move_batch(batch, device)
        with torch.no_grad():
            B = b["pixel_values"].shape[0]
            ts_tokens = model.duett.encode(model.duett.feats_to_input((b["x_ts"], b["x_static"], b["bin_ends"]), B))
            tokens16 = model.cxr.forward_bf16(b["pixel_values"])
            img_proj_full = A.linear(tokens16, model.img_proj.weight, model.img_proj.bias)
        mark("encoders")
        yield pc._select_ts(ts_tokens, "hourly_only"), img_proj_full, 1, b["y_multi"], b["y_multi_mask"]


def run_dual_gradient_diagnostics(teacher: torch.nn.Module, loader: Iterable[Mapping[str, Any]], loss_fn, device, *, max_batches: int = 8,
                                  label_names: Optional[Sequence[str]] = None, accelerator=None, _chunk: Optional[int] = None,
                                  _collect=None, _mark=None) -> Dict[str, Any]:
    """Objective gradients w.r.t. the shared pathology queries and the fusion loss's token sensitivity, aggregated over the first
    `max_batches` batches of `loader` (prefer a deterministic, non-shuffled subset of the training set).  `teacher`: a TeacherModel
    in `dual_patch` mode; `loss_fn`: the DualPathologyLoss instance (label weights, positive weights, alphas and masking reused)."""
    if max_batches <= 0:
        raise ValueError("max_batches must be positive")
    if accelerator is not None:
        raise NotImplementedError("run_dual_gradient_diagnostics: accelerator is not supported (no multi-GPU reduction); pass None")
    model = _unwrap_model(teacher)
    names, parameters = _find_pathology_query_banks(model)
    for name, parameter in zip(names, parameters):
        if not parameter.requires_grad:
            raise RuntimeError(f"{name} does not require gradients")
    modes = _eval_mode(model)
    try:
        mark = _mark or (lambda name: None)
        return perceiver_gradient_diagnostics(model.perceiver, _encoded_batches(model, loader, torch.device(device), max_batches, mark),
                                              loss_fn, label_names=label_names, _chunk=_chunk, _query_name="+".join(names),
                                              _collect=_collect, _mark=_mark)
    finally:
        _restore_modes(modes)


# ------------------------------------------------------------------------------------------------------------------------------
# the looped form: the reference's literal procedure, 4K + 4 walks of the graph per batch (baseline only)
# ------------------------------------------------------------------------------------------------------------------------------
def _looped_reference(teacher, loader, loss_fn, device, *, max_batches: int = 8, label_names: Optional[Sequence[str]] = None,
                      _collect=None) -> Dict[str, Any]:
    """The same report through `teacher(..., return_attn=True)` and 4K + 4 calls of `torch.autograd.grad(..., retain_graph=True,
    allow_unused=True)` per batch: 3 branch totals, 3K per-label losses, 1 + K token gradients.  The per-label tensors then go
    through the same accumulate / report kernels (which form the totals by linearity); the separately computed totals are handed
    to `_collect` (private: a list that receives (dq, dT, branch_totals [3, K, D], total_token_grads) per batch)."""
    import torch.nn.functional as F
    require_gpu()
    model = _unwrap_model(teacher)
    names, (queries,) = _find_pathology_query_banks(model)
    if not queries.requires_grad:
        raise RuntimeError(f"{names[0]} does not require gradients")
    K, D = queries.shape
    label_names = list(label_names) if label_names is not None else [f"label_{k}" for k in range(K)]
    alphas = tuple(float(getattr(loss_fn, "alpha_" + name, 1.0)) for name in BRANCHES)
    dev = torch.device(device)
    state = torch.zeros(state_size(K, D), dtype=F64, device=dev)
    pos_weight, eps = getattr(loss_fn, "pos_weight", None), float(getattr(loss_fn, "eps", 1e-6))

    def grad(loss, targets):
        values = torch.autograd.grad(loss, tuple(targets), retain_graph=True, create_graph=False, allow_unused=True)
        return [None if v is None else v.detach().float() for v in values]

    def per_label_bce(logits, y, mask):
        cells = []
        for k in range(K):
            e = F.binary_cross_entropy_with_logits(logits[:, k], y[:, k], reduction="none", pos_weight=None if pos_weight is None else pos_weight[k:k + 1])
            valid = mask[:, k].to(e.dtype)
            cells.append((e * valid).sum() / (valid.sum() + eps))
        return torch.stack(cells)

    modes = _eval_mode(model)
    n_batches = 0
    try:
        for index, batch in enumerate(loader):
            if index >= max_batches:
                break
            b = _move_batch(batch, dev)
            y, mask = b["y_multi"].float(), b["y_multi_mask"].float()
            with torch.enable_grad():
                out = model(b["x_ts"], b["x_static"], b["bin_ends"], b["pixel_values"], return_attn=True)
                lw = loss_fn.label_weights.to(device=dev, dtype=out["fusion_logits"].dtype)
                per = {name: per_label_bce(out[key], y, mask) for name, key in zip(BRANCHES, ("img_logits", "ts_logits", "fusion_logits"))}
                totals = torch.stack([grad((lw * per[name]).sum(), (queries,))[0] for name in BRANCHES])
                dq = torch.stack([torch.stack([grad(lw[k] * per[name][k], (queries,))[0] for k in range(K)]) for name in BRANCHES]).contiguous()
                I_tok, T_tok = out["img_tokens"], out["ts_tokens"]
                total_token = grad((lw * per["fus"]).sum(), (I_tok, T_tok))
                label_token = [grad(lw[k] * per["fus"][k], (I_tok, T_tok)) for k in range(K)]
            if any(g[0] is not None for g in label_token):
                dI = torch.stack([g[0] if g[0] is not None else torch.zeros_like(I_tok) for g in label_token], 1).contiguous()
            else:
                dI = None
            dT = torch.stack([g[1] for g in label_token], 1).contiguous()
            losses = torch.stack([lw * per[name].detach() for name in BRANCHES]).float().contiguous()
            grad_flow_accumulate(state, dq, dI, dT, I_tok.detach().contiguous(), T_tok.detach().contiguous(), mask.contiguous(), losses)
            if _collect is not None:
                _collect.append((dq, dT, totals, total_token))
            n_batches += 1
            del out, per
        if n_batches == 0:
            raise RuntimeError("The diagnostic loader yielded no batches")
        n_report = REPORT_HEAD + REPORT_PER_LABEL * K
        vec = torch.empty(n_report + 3 * K * K + K + 1, dtype=F64, device=dev)
        grad_flow_report(state, alphas, vec, K, D)
        with torch.no_grad():
            pc, prototypes = model.perceiver, queries.detach()
            rows = torch.stack([prototypes.float(), _effective_queries(pc.img_cross, prototypes).float(),
                                _effective_queries(pc.ts_cross, prototypes).float()]).contiguous()
        query_geometry(rows, vec[n_report:])
    finally:
        _restore_modes(modes)
    return report_from_vector(vec.cpu().tolist(), K, label_names, alphas, "+".join(names))


# ------------------------------------------------------------------------------------------------------------------------------
# host-only restatements
# ------------------------------------------------------------------------------------------------------------------------------
def format_gradient_diagnostics(report: Mapping[str, Any]) -> str:
    """The reference's console summary, character for character."""
    lines = [f"[grad-diag] parameter={report['query_parameter']} layout={report.get('query_layout', 'shared')} "
             f"batches={report['batches']} samples={report['samples']}",
             "",
             "branch      loss    alpha    ||g raw||   ||alpha*g||   cos(g,total)",
             "-" * 67]
    for name in BRANCHES:
        b = report["branch"][name]
        lines.append(f"{name:<7} {b['loss']:>9.5f} {b['alpha']:>7.3f} {b['raw_grad_norm']:>12.6g} {b['weighted_grad_norm']:>13.6g} "
                     f"{b['cos_to_total_update']:>14.5f}")
    cosine, sensitivity = report["pairwise_gradient_cosine"], report["fusion_token_sensitivity"]
    if report.get("query_layout") == "independent":
        lines += ["", "img–ts query-gradient cosine is expected to be 0: the modality queries occupy disjoint parameter banks."]
    lines += ["",
              f"gradient cosine: img-ts={cosine['img_ts']:+.5f}  img-fus={cosine['img_fus']:+.5f}  ts-fus={cosine['ts_fus']:+.5f}",
              f"batch img-ts cosine: mean={cosine['img_ts_batch_mean']:+.5f}  "
              f"negative_fraction={cosine['img_ts_negative_batch_fraction']:.3f}",
              f"weighted gradient dominance: img/ts={report['weighted_img_over_ts']:.4f}",
              f"fusion token sensitivity: raw img/ts={sensitivity['raw_img_over_ts']:.4f}  "
              f"scale-normalized img/ts={sensitivity['scaled_img_over_ts']:.4f}",
              "",
              "label                         ||g_img||   ||g_ts||  cos(i,t)  fusSens(i/t)  ownQ(img/ts/fus)",
              "-" * 100]
    for item in report["per_label"]:
        lines.append(f"{item['label']:<28} {item['img_grad_norm']:>10.5g} {item['ts_grad_norm']:>10.5g} {item['img_ts_cos']:>+9.4f} "
                     f"{item['fusion_token_sensitivity']['scaled_img_over_ts']:>13.4f} "
                     f"{item['img_own_query_fraction']:.2f}/{item['ts_own_query_fraction']:.2f}/{item['fus_own_query_fraction']:.2f}")
    geometry = report["query_geometry"]
    lines += ["",
              "query geometry: prototype norms=" + ", ".join(f"{value:.4f}" for value in geometry["prototype_norms"]),
              f"effective image-vs-TS Gram gap={geometry['image_ts_gram_gap']:.6f}"]
    return "\n".join(lines)


def gradient_diagnostics_to_log_dict(report: Mapping[str, Any], prefix: str = "grad_diag") -> Dict[str, float]:
    """The values worth a WandB / TensorBoard curve, flattened under `prefix` (the reference's keys, in its order)."""
    values: Dict[str, float] = {}
    for name, item in report["branch"].items():
        for key, source in (("loss", "loss"), ("raw_grad_norm", "raw_grad_norm"), ("weighted_grad_norm", "weighted_grad_norm"),
                            ("cos_to_total", "cos_to_total_update")):
            values[f"{prefix}/{name}/{key}"] = float(item[source])
    for key, value in report["pairwise_gradient_cosine"].items():
        values[f"{prefix}/cosine/{key}"] = float(value)
    values[f"{prefix}/dominance/weighted_img_over_ts"] = float(report["weighted_img_over_ts"])
    for key in ("raw_img_over_ts", "scaled_img_over_ts"):
        values[f"{prefix}/fusion_sensitivity/{key}"] = float(report["fusion_token_sensitivity"][key])
    values[f"{prefix}/query_geometry/image_ts_gram_gap"] = float(report["query_geometry"]["image_ts_gram_gap"])
    for item in report["per_label"]:
        base = f"{prefix}/label/{item['label'].replace('/', '_')}"
        for key in ("img_grad_norm", "ts_grad_norm", "fus_grad_norm", "img_ts_cos"):
            values[f"{base}/{key}"] = float(item[key])
        values[f"{base}/fusion_scaled_img_over_ts"] = float(item["fusion_token_sensitivity"]["scaled_img_over_ts"])
    return values


# ------------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser("Gradient flow diagnostics for dual_patch teacher")
    p.add_argument("--ckpt", type=str, required=True, help="teacher best.pt written by train_synthetic")
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--split", type=str, default="train", choices=["train", "val", "test"])
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=2)
    p.add_argument("--max_batches", type=int, default=16, help="deterministic subset size in batches")
    return p.parse_args(argv)


def build_model_and_loader(args, state: dict, device):
    """-> (teacher, loader, labels, loss_fn, n_needed, n_split): the teacher restored UNFROZEN from its own checkpoint, the first
    max_batches * batch_size samples of the split, unshuffled; label weights and alphas from the checkpoint's args (label_weights
    absent: uniform; alphas under the reference's `aux_*_alpha` names or train_synthetic's `alpha_*`)."""
    from . import checkpoint, train_synthetic
    from .cohort import collate
    from .losses_duett import DualPathologyLoss
    ck = state["args"]
    mode = ck.get("perceiver_type")
    if mode != "dual_patch":
        raise RuntimeError(f"perceiver_type={mode} is not supported: dual_patch only")
    t_args = argparse.Namespace(**ck)
    teacher = checkpoint.load_model_state(train_synthetic.build_teacher(t_args, device), state, freeze=False)
    labels = tuple(s.strip() for s in ck["pathology_labels"].split(","))
    raw = ck.get("label_weights")
    if raw:
        label_weights = torch.tensor([float(w) for w in raw.split(",")], dtype=F32)
        if label_weights.numel() != len(labels):
            raise ValueError(f"label_weights len ({label_weights.numel()}) != pathology_labels len ({len(labels)})")
    else:
        label_weights = torch.ones(len(labels), dtype=F32)
    alpha = lambda name, default: float(ck.get(f"aux_{name}_alpha", ck.get(f"alpha_{name}", default)))  # noqa: E731
    loss_fn = DualPathologyLoss(label_weights, None, alpha("img", 0.5), alpha("ts", 0.5), alpha("fus", 1.0)).to(device)
    dataset = dict(zip(("train", "val", "test"), train_synthetic._datasets(t_args)))[args.split]
    n_needed = min(args.max_batches * args.batch_size, len(dataset))
    subset = torch.utils.data.Subset(dataset, list(range(n_needed)))
    loader = torch.utils.data.DataLoader(subset, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers, pin_memory=True,
                                         collate_fn=lambda items: collate(items, "teacher"), drop_last=False)
    return teacher, loader, labels, loss_fn, n_needed, len(dataset)


def main(argv=None) -> dict:
    """The reference's `main()` on a `train_synthetic` teacher checkpoint: prints the report and writes grad_flow_report.txt / .json."""
    from . import checkpoint
    args = parse_args(argv)
    os.makedirs(args.outdir, exist_ok=True)
    require_gpu()
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"[grad-diag] device={device}")
    state = checkpoint.load_ckpt(args.ckpt)
    teacher, loader, labels, loss_fn, n_needed, n_split = build_model_and_loader(args, state, device)
    print(f"[grad-diag] ckpt: {args.ckpt}")
    print(f"[grad-diag] mode=dual_patch  K={len(labels)}  labels={labels}")
    print(f"[grad-diag] loss alphas: img={loss_fn.alpha_img} ts={loss_fn.alpha_ts} fus={loss_fn.alpha_fus}")
    print(f"[grad-diag] split={args.split}: first {n_needed}/{n_split} samples → up to {args.max_batches} batches of {args.batch_size}")
    report = run_dual_gradient_diagnostics(teacher, loader, loss_fn, device, max_batches=args.max_batches, label_names=list(labels))
    text = format_gradient_diagnostics(report)
    print("\n" + text)
    txt_path, json_path = os.path.join(args.outdir, "grad_flow_report.txt"), os.path.join(args.outdir, "grad_flow_report.json")
    with open(txt_path, "w") as f:
        f.write(text + "\n")
    with open(json_path, "w") as f:
        json.dump(report, f, indent=2)
    print(f"\n[grad-diag] saved: {txt_path}")
    print(f"[grad-diag] saved: {json_path}")
    return {"report": report, "txt": txt_path, "json": json_path}


if __name__ == "__main__":
    main()
