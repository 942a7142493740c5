#!/usr/bin/env python3
"""Golden fixtures for the gradient-flow diagnostics (analysis/grad_flow_diagnostics.py): runs the REFERENCE'S OWN functions
(`run_dual_gradient_diagnostics`, `format_gradient_diagnostics`, `gradient_diagnostics_to_log_dict`, `_branch_losses`, `_grads`;
stubs as in make_golden.py) and stores numbers and recorded text only.

At the reference's HEAD the module does not work as it stands: `_find_pathology_query_banks` looks for `image_queries` +
`temporal_queries` or one `pathology_queries` and raises on the live model's `shared_queries`, and the script imports
`analysis/visualize_pathology.py`, which needs packages that are absent here.  This maker replaces EXACTLY ONE function,
`_find_pathology_query_banks`, with one that returns the `shared_queries` bank, and stubs the `visualize_pathology` import (its two
names are used by the CLI only).  All arithmetic stays the reference's.

tests/golden/grad_flow_small.npz
  The reference's `PatchDualPathologyPerceiver(K=3, d_ts=24, d_latent=32, n_heads=4, dropout=0, head_dropout=0)` inside a minimal
  wrapper module that exposes `.perceiver` and takes pre-made `ts_tokens` / `img_patches_proj` through the `x_ts` / `pixel_values`
  arguments.  Seeded weights with a non-zero `correction_head[-1].weight`, queries scaled so that every branch gradient is non-zero
  (asserted).  Three batches, B = 6, 6, 4, T = 6 (+1 rep token), P = 10 patches.  `DualPathologyLoss` with non-uniform label weights,
  a `pos_weight`, alphas 0.5 / 0.5 / 1.0.  About 80 % of the labels known; label 1 is fully masked in the whole of batch 1 (the
  zero-gradient / zero-denominator path).  Every batch's image-ts cosine has magnitude > 1e-3 (asserted), so the negative fraction
  cannot flip on rounding; the seed is searched for one at which both signs occur, and the maker says whether it found one.
  Stored: the weights, inputs, y, mask, the reference's report (JSON text), the text of `format_gradient_diagnostics`, the
  `gradient_diagnostics_to_log_dict` items and, for every batch, dq [3, K, K, D], dT [B, K, K, D], the tokens and the losses
  obtained with the reference's own `_grads` calls.
tests/golden/grad_flow_cfg1.npz
  The reference's report only, on the cfg1 teacher of make_golden.py (same seeds and `synth_state_dict`, K = 7, 224 x 224), batches
  `make_batch(ccfg, 100, 8)` and `make_batch(ccfg, 101, 8)`, `DualPathologyLoss(ones, None, 0.5, 0.5, 1.0)`.  No weights stored.
Build container only.

Usage:  python tests/golden/make_golden_grad_flow.py [output directory]"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs, shapes_of, synth_state_dict  # noqa: E402
from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch  # noqa: E402

K, D_TS, D, HEADS, T, P = 3, 24, 32, 4, 6, 10
BATCH_SIZES = (6, 6, 4)
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
LABEL_WEIGHTS, POS_WEIGHT = (1.0, 0.5, 2.0), (1.5, 1.0, 0.75)
ALPHAS = (0.5, 0.5, 1.0)
MASKED_BATCH, MASKED_LABEL = 1, 1


def import_reference():
    install_stubs()
    sys.path.insert(0, REF)
    stub = types.ModuleType("analysis.visualize_pathology")           # the CLI's loader helpers: not ported, not used here
    stub._loader = stub.load_teacher = None
    sys.modules["analysis.visualize_pathology"] = stub
    import analysis.grad_flow_diagnostics as ref

    def shared_bank(model):
        found = [(n, p) for n, p in model.named_parameters() if n.endswith("shared_queries")]
        assert len(found) == 1
        return (found[0][0],), (found[0][1],)

    ref._find_pathology_query_banks = shared_bank                      # the ONE replaced function
    return ref


class Wrapper(nn.Module):
    """What the reference's diagnostic needs of a teacher: `.perceiver` and the five-argument forward."""

    def __init__(self, perceiver):
        super().__init__()
        self.perceiver = perceiver

    def forward(self, x_ts, x_static, bin_ends, pixel_values, return_attn=False):
        return self.perceiver(torch.stack(tuple(x_ts)), pixel_values, return_attn=return_attn)


def small_problem(seed: int):
    from models.main_architecture_duett import PatchDualPathologyPerceiver
    torch.manual_seed(seed)
    pc = PatchDualPathologyPerceiver(n_pathologies=K, d_ts=D_TS, d_latent=D, n_heads=HEADS, dropout=0.0, head_dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        pc.correction_head[-1].weight.copy_(0.3 * torch.randn(pc.correction_head[-1].weight.shape, generator=g))
        pc.shared_queries.mul_(25.0)                                   # 0.02 -> 0.5: the queries matter to the attention
        pc.beta.copy_(1.0 + 0.1 * torch.randn(K, generator=g))
        pc.image_label_bias.copy_(0.1 * torch.randn(K, generator=g))
        pc.temporal_label_bias.copy_(0.1 * torch.randn(K, generator=g))
    batches = []
    for i, B in enumerate(BATCH_SIZES):
        mask = (torch.rand(B, K, generator=g) < 0.8).float()
        mask[0] = 1.0                                                  # no label without a known sample by accident
        if i == MASKED_BATCH:
            mask[:, MASKED_LABEL] = 0.0
        batches.append({"x_ts": torch.randn(B, T + 1, D_TS, generator=g), "x_static": (), "bin_ends": (),
                        "pixel_values": torch.randn(B, P, D, generator=g), "y_multi": (torch.rand(B, K, generator=g) < 0.4).float(),
                        "y_multi_mask": mask})
    return Wrapper(pc), batches


def per_batch_tensors(ref, model, batches, loss_fn):
    """dq, dT, tokens and losses of every batch through the reference's own `_branch_losses` / `_grads`."""
    out = {}
    queries = (model.perceiver.shared_queries,)
    model.eval()
    for i, b in enumerate(batches):
        with torch.enable_grad():
            o = model(tuple(b["x_ts"]), (), (), b["pixel_values"], return_attn=True)
            losses = ref._branch_losses(o, b["y_multi"], b["y_multi_mask"], loss_fn)
            lw = losses["label_weights"]
            dq = torch.stack([torch.stack([ref._grads(lw[k] * losses[per][k], queries)[0] for k in range(K)])
                              for per in ("img_per", "ts_per", "fus_per")])
            totals = torch.stack([ref._grads(losses[name], queries)[0] for name in ("img", "ts", "fus")])
            token = [ref._grads(lw[k] * losses["fus_per"][k], (o["img_tokens"], o["ts_tokens"])) for k in range(K)]
        assert all(float(g[0].abs().max()) == 0.0 for g in token), "fusion_logits must not depend on the image tokens"
        out.update({f"b{i}_dq": dq, f"b{i}_dq_totals": totals, f"b{i}_dT": torch.stack([g[1] for g in token], 1),
                    f"b{i}_I": o["img_tokens"].detach(), f"b{i}_T": o["ts_tokens"].detach(),
                    f"b{i}_losses": torch.stack([lw * losses[per].detach() for per in ("img_per", "ts_per", "fus_per")]),
                    f"b{i}_cos": ref._cosine(totals[0], totals[1])})
    return out


def make_small(ref, out_dir):
    from loss.losses_duett import DualPathologyLoss
    loss_fn = DualPathologyLoss(torch.tensor(LABEL_WEIGHTS), torch.tensor(POS_WEIGHT), *ALPHAS)
    chosen = None
    for seed in range(64):
        model, batches = small_problem(seed)
        tensors = per_batch_tensors(ref, model, batches, loss_fn)
        cos = [float(tensors[f"b{i}_cos"]) for i in range(len(batches))]
        if all(abs(c) > 1e-3 for c in cos) and chosen is None:
            chosen = (seed, model, batches, tensors, cos)
        if all(abs(c) > 1e-3 for c in cos) and min(cos) < 0 < max(cos):
            chosen = (seed, model, batches, tensors, cos)
            break
    assert chosen is not None, "no seed with every batch cosine away from zero"
    seed, model, batches, tensors, cos = chosen
    both = min(cos) < 0 < max(cos)
    print(f"small: seed {seed}, batch cosines {cos}: " + ("both signs occur" if both else "NO seed in 0..63 gave both signs"))
    assert all(abs(c) > 1e-3 for c in cos)
    report = ref.run_dual_gradient_diagnostics(model, batches, loss_fn, torch.device("cpu"), max_batches=len(batches), label_names=LABELS)
    for name in ("img", "ts", "fus"):
        assert report["branch"][name]["raw_grad_norm"] > 1e-6, (name, report["branch"][name])
    assert all(p.grad is None for p in model.parameters())
    text = ref.format_gradient_diagnostics(report)
    log = ref.gradient_diagnostics_to_log_dict(report)
    print(text)
    out = {"cfg": np.array([K, D_TS, D, HEADS, T, P, seed]), "batch_sizes": np.array(BATCH_SIZES), "labels": np.array(LABELS),
           "label_weights": np.array(LABEL_WEIGHTS, dtype=np.float32), "pos_weight": np.array(POS_WEIGHT, dtype=np.float32),
           "alphas": np.array(ALPHAS), "both_signs": np.array(both), "report_json": np.array(json.dumps(report)),
           "format_text": np.array(text), "log_keys": np.array(list(log)), "log_values": np.array(list(log.values()), dtype=np.float64)}
    for name, value in model.perceiver.state_dict().items():
        out["w:" + name] = value.detach().numpy()
    for i, b in enumerate(batches):
        out.update({f"b{i}_ts_tokens": b["x_ts"].numpy(), f"b{i}_img_patches_proj": b["pixel_values"].numpy(),
                    f"b{i}_y": b["y_multi"].numpy(), f"b{i}_mask": b["y_multi_mask"].numpy()})
    out.update({k: v.detach().numpy() for k, v in tensors.items()})
    path = os.path.join(out_dir, "grad_flow_small.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote grad_flow_small.npz: {os.path.getsize(path) / 1e3:.0f} kB")


def cfg1_teacher():
    """The teacher of make_golden.py's fixtures (5)-(7): same construction, same seeds."""
    from models.main_architecture_duett import CXREncoder, DuettFeatureExtractor, PatchDualPathologyPerceiver, TeacherModel
    from transformers import Dinov2Config, Dinov2Model
    T1, V, DS, K1 = 32, 16, 8, 7
    vit = Dinov2Model(Dinov2Config(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_ratio=4, patch_size=14, image_size=518,
                                   layerscale_value=1.0, qkv_bias=True, use_swiglu_ffn=False))
    vit.load_state_dict(synth_state_dict(shapes_of(vit.state_dict()), 3), strict=True)
    vit.eval()
    cxr = CXREncoder.__new__(CXREncoder)
    nn.Module.__init__(cxr)
    cxr.backbone, cxr.d_out, cxr.return_patches, cxr._frozen = vit, 768, True, True
    for p in cxr.backbone.parameters():
        p.requires_grad = False
    backbone = DuettFeatureExtractor(d_static_num=DS, d_time_series_num=V, d_target=1, pretrain=False, masked_transform_timesteps=T1,
                                     max_len=T1, aug_noise=0.0, aug_mask=0.0, transformer_dropout=0.0)
    for p in backbone.parameters():
        p.requires_grad = False
    backbone.eval()
    perceiver = PatchDualPathologyPerceiver(n_pathologies=K1, d_ts=backbone.d_representation, d_latent=256, n_heads=4, dropout=0.0,
                                            head_dropout=0.0)
    teacher = TeacherModel(backbone, cxr, perceiver, head_hidden=128, head_dropout=0.0, cxr_return_patches=True, d_img=768,
                           use_aux_cxr=False, patch_dual_pathology_mode=True)
    sd = synth_state_dict(shapes_of(teacher.state_dict()), seed=4)
    for k, v in vit.state_dict().items():
        sd["cxr.backbone." + k] = v.clone()
    teacher.load_state_dict(sd, strict=True)
    return teacher, CohortCfg(n_timesteps=T1, n_vars=V, d_static=DS, image_size=224, seed=1234), K1


def make_cfg1(ref, out_dir):
    from loss.losses_duett import DualPathologyLoss
    teacher, ccfg, K1 = cfg1_teacher()
    batches = [make_batch(ccfg, 100, 8, mode="teacher"), make_batch(ccfg, 101, 8, mode="teacher")]
    loss_fn = DualPathologyLoss(torch.ones(K1), None, 0.5, 0.5, 1.0)
    report = ref.run_dual_gradient_diagnostics(teacher, batches, loss_fn, torch.device("cpu"), max_batches=2)
    print(ref.format_gradient_diagnostics(report))
    path = os.path.join(out_dir, "grad_flow_cfg1.npz")
    np.savez_compressed(path, report_json=np.array(json.dumps(report)), batch_starts=np.array([100, 101]), batch_size=np.array(8))
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote grad_flow_cfg1.npz: {os.path.getsize(path) / 1e3:.0f} kB")


def main(out_dir=HERE):
    torch.set_num_threads(8)
    ref = import_reference()
    make_small(ref, out_dir)
    make_cfg1(ref, out_dir)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
