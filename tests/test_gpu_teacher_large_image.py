"""The teacher on chest X-rays above 546 x 546 (more than 1536 image patches): the perceiver's img_cross block attends the
pathology queries over every patch through the split-key kernels (attention_fq_split.hip).  HIP path against the CPU oracle on
the same seeded weights and inputs, with the tolerances of the stress-shape parity test; the captured step against the eager one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multimodal_edema_prediction_amd import engine  # noqa: E402
from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch  # noqa: E402
from multimodal_edema_prediction_amd.losses_duett import DualPathologyLoss  # noqa: E402
from multimodal_edema_prediction_amd.main_architecture_duett import (CXREncoder, PatchDualPathologyPerceiver,  # noqa: E402
                                                                       TeacherModel, load_duett_backbone)
from oracle import duett_ref, losses_ref, step_ref, vit_ref  # noqa: E402

T, V, DS, K, B = 32, 16, 8, 7, 2
DEV = "cuda"


def build_teacher(seed=0):
    torch.manual_seed(seed)
    backbone = load_duett_backbone("synthetic", d_static_num=DS, d_time_series_num=V, n_timesteps=T, freeze=True)
    cxr = CXREncoder("synthetic", freeze=True)
    per = PatchDualPathologyPerceiver(K, backbone.d_representation, dropout=0.0, head_dropout=0.0)
    torch.nn.init.normal_(per.correction_head[-1].weight, std=0.05)
    return TeacherModel(backbone, cxr, per, cxr_return_patches=True, d_img=768, use_aux_cxr=False, patch_dual_pathology_mode=True).to(DEV)


def test_teacher_forward_and_loss_at_672():
    """672^2: 48 x 48 = 2304 patches, beyond the 1536 keys of the wave-per-query kernels."""
    teacher = build_teacher()
    sd = {k: v.detach().float().cpu().clone() for k, v in teacher.state_dict().items()}
    batch = make_batch(CohortCfg(n_timesteps=T, n_vars=V, d_static=DS, image_size=672, n_labels=K), 0, B, mode="teacher")
    loss_fn = DualPathologyLoss(torch.ones(K)).to(DEV)
    engine._set_train_with_frozen_eval(teacher)
    b = engine._move_lists(batch, DEV)
    out = teacher(b["x_ts"], b["x_static"], b["bin_ends"], b["pixel_values"], return_attn=True)
    assert out["img_attn"].shape == (B, K, 2304)
    L = loss_fn(out["img_logits"], out["ts_logits"], out["fusion_logits"], b["y_multi"], b["y_multi_mask"])
    L["total"].backward()
    dcfg = duett_ref.DuettCfg(d_static_num=DS, d_time_series_num=V, n_timesteps=T)
    ref = step_ref.teacher_forward(sd, dcfg, vit_ref.VitCfg(), batch, return_attn=True)
    for k in ("img_logits", "ts_logits", "fusion_logits", "scaled_correction"):
        err = float((out[k].detach().cpu() - ref[k]).abs().max())
        assert err < 3e-2, (k, err)
    assert float((out["img_attn"].cpu() - ref["img_attn"]).abs().max()) < 5e-3
    Lr = losses_ref.dual_pathology_loss(ref["img_logits"], ref["ts_logits"], ref["fusion_logits"], batch["y_multi"], batch["y_multi_mask"],
                                        torch.ones(K))
    assert abs(float(L["total"]) - float(Lr["total"])) <= 1e-2 * abs(float(Lr["total"]))
    assert all(torch.isfinite(p.grad).all() for p in teacher.parameters() if p.grad is not None)


def test_graphed_step_equals_eager_step_at_560():
    """560^2 (1600 patches): the captured teacher step does the eager engine step's arithmetic (dropout off)."""
    from multimodal_edema_prediction_amd.graph_step import GraphedTeacherStep
    from multimodal_edema_prediction_amd.optim import FusedAdamW, make_param_groups
    batch = make_batch(CohortCfg(n_timesteps=T, n_vars=V, d_static=DS, image_size=560, n_labels=K), 0, B, mode="teacher")
    loss_fn = DualPathologyLoss(torch.ones(K), None, 0.5, 0.5, 1.0).to(DEV)
    te = build_teacher()
    oe = FusedAdamW(make_param_groups(te, 8e-5), weight_decay=5e-2)
    eager_losses = [engine.train_teacher_dual_pathology_batch(batch, te, loss_fn, oe, torch.device(DEV))["loss"] for _ in range(3)]
    tg = build_teacher()
    og = FusedAdamW(make_param_groups(tg, 8e-5), weight_decay=5e-2)
    gs = GraphedTeacherStep(tg, loss_fn, og, batch, torch.device(DEV), warmup=3)
    graph_losses = [float(gs.step(batch)["loss"].item()) for _ in range(3)]
    np.testing.assert_allclose(graph_losses, eager_losses, rtol=1e-5, atol=1e-6)
    for (k, a), (_, b) in zip(te.named_parameters(), tg.named_parameters()):
        if a.requires_grad:
            assert float((a - b).abs().max()) <= 1e-6, k
    assert og._step == oe._step == 3
