"""The training head with dropout on (the configuration the benchmark trains: perceiver dropout 0.2, head dropout 0.2) against the fp64
oracle, mask for mask: PatchDualPathologyPerceiver draws one seed per forward and uses it at its 15 dropout sites; the oracle
(oracle/fusion_ref.py, `drop=` hook) applies the host replica's mask of each site (tests/dropout_twin.py).  Image tokens with a CLS row
(skipped) over 256 keys (the one-workgroup few-query kernels) and 1369 / 2304 keys (the split-key kernels)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_twin as T  # noqa: E402
from dropout_twin import pinned_epoch  # noqa: E402

DEV = "cuda"
B, K, D, H, HID, D_TS, T_HOURS = 4, 7, 256, 4, 128, 128, 48
SEED = 1234567


def _drop_hook(sids):
    """drop(t, p, site) for the oracle: t * (mask * scale) of the site's stream id and layout, epoch NULL."""
    def drop(t, p, site):
        name, _, part = site.partition(".")
        if part == "attn":
            Bq, Hq, Lq, Lk = t.shape
            ms = T.mask_scale(SEED, sids[name], T.attn_index(Bq, Hq, Lq, Lk), p)
        else:
            sid = sids[name] + {"": 0, "ff_gelu": 1, "ff_out": 2}[part]
            ms = T.mask_scale(SEED, sid, T.flat_index(tuple(t.shape)), p)
        return t * torch.from_numpy(ms).to(t.dtype)
    return drop


def _cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)), float(a.norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Lk", [256, 1369, 2304])
def test_perceiver_training_forward_backward_with_dropout_against_oracle(Lk, mode, monkeypatch):
    from multimodal_edema_prediction_amd import autograd_ops as A
    from multimodal_edema_prediction_amd import functional as Fn
    from multimodal_edema_prediction_amd.losses_duett import DualPathologyLoss
    from multimodal_edema_prediction_amd.main_architecture_duett import _SID, PatchDualPathologyPerceiver
    from oracle import fusion_ref, losses_ref

    kv_probe = torch.empty(B, Lk + 1, 2 * D, device=DEV)                 # the layout of img_cross's fused K | V projection
    assert A._fq_split_route(kv_probe, 1, K, Lk, D // H) == (Lk > 1024), "the kernel family this size is meant to cover changed"

    torch.manual_seed(0)
    model = PatchDualPathologyPerceiver(K, D_TS, d_latent=D, n_heads=H, dropout=0.2, head_dropout=0.2, head_hidden=HID)
    torch.nn.init.normal_(model.correction_head[-1].weight, std=0.05)       # a live correction branch (its dropout site included)
    model = model.to(DEV).train()
    sd = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}

    g = torch.Generator().manual_seed(Lk)
    ts = torch.randn(B, T_HOURS + 1, D_TS, generator=g)
    img = torch.randn(B, Lk + 1, D, generator=g)
    y = (torch.rand(B, K, generator=g) > 0.5).float()
    ymask = (torch.rand(B, K, generator=g) > 0.2).float()
    r_img, r_ts = torch.randn(B, K, D, generator=g) * 0.05, torch.randn(B, K, D, generator=g) * 0.05

    monkeypatch.setattr(A, "next_seed", lambda: SEED)
    tsd, imgd = ts.to(DEV).requires_grad_(True), img.to(DEV).requires_grad_(True)
    with pinned_epoch(None), Fn.precision_mode(mode):
        out = model(tsd, imgd, _img_skip=1)
        L = DualPathologyLoss(torch.ones(K)).to(DEV)(out["img_logits"], out["ts_logits"], out["fusion_logits"], y.to(DEV), ymask.to(DEV))
        total = L["total"] + (out["img_tokens"] * r_img.to(DEV)).sum() + (out["ts_tokens"] * r_ts.to(DEV)).sum()
        model.zero_grad()
        total.backward()
        torch.cuda.synchronize()

    tsr, imgr = ts.double().requires_grad_(True), img.double().requires_grad_(True)
    ref = fusion_ref.perceiver_forward(sd, tsr, imgr[:, 1:], H, dropout=0.2, head_dropout=0.2, training=True, drop=_drop_hook(_SID))
    Lr = losses_ref.dual_pathology_loss(ref["img_logits"], ref["ts_logits"], ref["fusion_logits"], y.double(), ymask.double(),
                                        torch.ones(K, dtype=torch.float64))
    total_r = Lr["total"] + (ref["img_tokens"] * r_img.double()).sum() + (ref["ts_tokens"] * r_ts.double()).sum()
    total_r.backward()

    logit_tol = 1e-4 if mode == "fp32" else 3e-2
    for k in ("img_logits", "ts_logits", "fusion_logits", "scaled_correction"):
        err = float((out[k].detach().double().cpu() - ref[k].detach()).abs().max())
        assert err <= logit_tol, (mode, k, err)
    loss_tol = 1e-5 if mode == "fp32" else 1e-2
    for got, want in ((L["total"], Lr["total"]), (total, total_r)):
        assert abs(float(got) - float(want)) <= loss_tol * abs(float(want)), (mode, float(got), float(want))

    named = dict(model.named_parameters())
    grads = [(k, named[k].grad, sd[k].grad) for k in named] + [("ts_tokens", tsd.grad, tsr.grad), ("img_tokens", imgd.grad, imgr.grad)]
    assert len(named) >= 60
    for k, got, want in grads:
        assert got is not None and want is not None, k
        if mode == "fp32":
            err = float((got.double().cpu() - want).abs().max())
            scale = float(want.abs().max())
            assert err <= 2e-4 * scale + 1e-7, f"{k}: max |dg| {err:.3e}, max |g| {scale:.3e}"
        else:
            c, ratio = _cos(got, want)
            assert c > 0.99 and abs(ratio - 1) < 0.1, (k, c, ratio)
