"""The ViT front end as the model runs it — patch GEMM, class token, position embeddings (resized or stored), final LayerNorm —
with NOTHING between it and the check: an encoder of zero blocks (hidden 128, a 5 x 5 stored grid, K = 588 padded to 592), frozen
(`medp_vit_forward`) and trainable (`cxr_train.forward_training`), against tests/vit_front_refs.front_end in float64 with float64
autograd.  Class token, positions (unit scale, not 0.02), bias and the final LayerNorm are random; pixels and the patch weight are
bf16-representable, so the GEMM's operands are exact and what is left is fp32 accumulation.

The wrapper accepts zero blocks, so no block with zeroed LayerScale stands in.

Worst observed error / bound on an MI355X (each test prints its own):
  tokens, frozen     0.0088 (98x98: 2.3e-6 absolute); trainable 0.0097; the two paths' tokens are NOT bit-equal in any of the cases
  gradients          positions 0.0037, class token 0.0006, patch bias 0.0015, patch weight 0.419 (1.68e-3 relative),
                     final LayerNorm weight 0.050, bias 0.008
  PatchEmbedFn       forward 0.0022, dW 0.422 (1.69e-3 relative), db 0.0010
  PosBicubicFn       forward 0.030, backward 0.019"""
import functools
import math

import pytest
import torch

import vit_front_refs as R
from oracle.vit_ref import VitCfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, SIDE, PATCH, B = 128, 5, 14, 2
LAYERS = 0
# native grid (no resize) | 3 x 4: resized, non-square | 5 x 4 with remainder pixels ignored | 7 x 7: up-sampling
IMAGES = [(70, 70), (42, 56), (75, 61), (98, 98)]
REF_CFG = VitCfg(hidden=D, layers=0, heads=2, patch=PATCH, image_size=PATCH * SIDE)
GEMM_RTOL, GEMM_ATOL = 1e-4, 2e-4                                   # test_gpu_kernels.test_gemm_plain
GRAD_TOL = {"embeddings.position_embeddings": 1e-4, "embeddings.cls_token": 1e-4, "embeddings.patch_embeddings.projection.bias": 1e-4,
            # the weight-gradient GEMM rounds dY to bf16, at most 2^-9 relative per element: twice that worst case
            "embeddings.patch_embeddings.projection.weight": 4e-3}
LN_RTOL, LN_ATOL = 1e-4, 1e-4                                       # test_gpu_kernels.test_layernorm_fwd_bwd: dw, db


def bf_round(x):
    return x.bfloat16().float()


@functools.lru_cache(maxsize=None)
def _params():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"embeddings.cls_token": r(1, 1, D), "embeddings.position_embeddings": r(1, 1 + SIDE * SIDE, D),
            "embeddings.patch_embeddings.projection.weight": bf_round(r(D, 3, PATCH, PATCH) / math.sqrt(3 * PATCH * PATCH)),
            "embeddings.patch_embeddings.projection.bias": r(D), "layernorm.weight": 1 + 0.3 * r(D), "layernorm.bias": 0.3 * r(D)}


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """pixels, read-out, and the float64 reference (tokens, stream before the LayerNorm, gradients): computed once per image"""
    g = torch.Generator().manual_seed(H * 1000 + W)
    px = bf_round(torch.randn(B, 3, H, W, generator=g))
    S = 1 + (H // PATCH) * (W // PATCH)
    wsel = torch.randn(S, D, generator=g)                           # a fixed linear read-out as the loss
    leaves = {k: v.double().requires_grad_(True) for k, v in _params().items()}
    tok, stream = R.front_end(leaves, REF_CFG, px.double(), return_stream=True)
    grads = dict(zip(leaves, torch.autograd.grad((tok * wsel.double()).sum(), list(leaves.values()))))
    return {"px": px, "wsel": wsel, "tok": tok.detach(), "stream": stream.detach(), "grads": grads}


@functools.lru_cache(maxsize=None)
def _encoder(freeze):
    from multimodal_edema_prediction_amd.cxr import Dinov2Cfg
    from multimodal_edema_prediction_amd.main_architecture_duett import CXREncoder
    enc = CXREncoder(freeze=freeze, config=Dinov2Cfg(hidden_size=D, num_hidden_layers=LAYERS, num_attention_heads=2, image_size=PATCH * SIDE))
    named = dict(enc.backbone.named_parameters())
    with torch.no_grad():
        for k, v in _params().items():
            named[k].copy_(v)
    return enc.to(DEV) if freeze else enc.to(DEV).train()


def _tokens_close(tok, case, what):
    """|tok - ref| <= f * (atol + rtol |x|) element by element: test_gemm_plain's bound on the stream x before the LayerNorm, times
    the factor f = max|w| * rstd(row) by which the final LayerNorm y = w (x - mean) rstd + b hands an error of x on."""
    x = case["stream"]
    rstd = (x.var(-1, unbiased=False, keepdim=True) + REF_CFG.ln_eps).rsqrt()
    f = float(_params()["layernorm.weight"].abs().max()) * rstd
    tol = f * (GEMM_ATOL + GEMM_RTOL * x.abs())
    got = tok.detach().double().cpu()
    ratio = (got - case["tok"]).abs() / tol
    print(f"{what}: max err {float((got - case['tok']).abs().max()):.3e}, worst {float(ratio.max()):.4f} of the bound (factor {float(f.min()):.3f} .. {float(f.max()):.3f})")
    assert got.shape == case["tok"].shape and bool(torch.isfinite(got).all()) and bool((ratio <= 1).all()), what


@pytest.mark.parametrize("H,W", IMAGES)
def test_frozen_front_end(H, W):
    case = _case(H, W)
    tok, _ = _encoder(True).backbone(case["px"].to(DEV))
    assert tok.dtype == torch.float32 and not tok.requires_grad
    _tokens_close(tok, case, f"frozen {H}x{W}")


@pytest.mark.parametrize("H,W", IMAGES)
def test_trainable_front_end_and_its_gradients(H, W):
    case = _case(H, W)
    enc = _encoder(False)
    tok, _ = enc.backbone(case["px"].to(DEV))
    assert tok.dtype == torch.float32 and tok.requires_grad
    _tokens_close(tok, case, f"trainable {H}x{W}")
    frozen, _ = _encoder(True).backbone(case["px"].to(DEV))
    print(f"  trainable tokens bit-equal to the frozen path's: {torch.equal(tok.detach(), frozen)}")
    enc.zero_grad()
    (tok * case["wsel"].to(DEV)).sum().backward()
    named = dict(enc.backbone.named_parameters())
    for k, tol in GRAD_TOL.items():
        got, want = named[k].grad.double().cpu(), case["grads"][k]
        rel = float((got - want).norm() / want.norm())
        print(f"  d {k}: |ref| {float(want.norm()):.3e}, relative error {rel:.3e}: {rel / tol:.4f} of the bound")
        assert float(want.norm()) > 1e-4, (k, "a dead path")
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and rel <= tol, (k, rel)
    for k in ("layernorm.weight", "layernorm.bias"):
        got, want = named[k].grad.double().cpu(), case["grads"][k]
        ratio = (got - want).abs() / (LN_ATOL + LN_RTOL * want.abs())
        print(f"  d {k}: |ref| {float(want.norm()):.3e}, worst {float(ratio.max()):.4f} of the bound")
        assert float(want.norm()) > 1e-4, (k, "a dead path")
        assert bool(torch.isfinite(got).all()) and bool((ratio <= 1).all()), k


# ------------------------------------------------------------------------------------------------ the two autograd nodes on their own
@pytest.mark.parametrize("H,W", IMAGES)
def test_patch_embed_fn(H, W):
    from multimodal_edema_prediction_amd.cxr_train import PatchEmbedFn
    case, p = _case(H, W), _params()
    w, b = p["embeddings.patch_embeddings.projection.weight"], p["embeddings.patch_embeddings.projection.bias"]
    P = (H // PATCH) * (W // PATCH)
    dy = torch.randn(B, P, D, generator=torch.Generator().manual_seed(H + W))
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    want = (R.im2col(case["px"].double(), PATCH, 3 * PATCH * PATCH) @ wr.reshape(D, -1).T + br).view(B, P, D)
    dw_ref, db_ref = torch.autograd.grad((want * dy.double()).sum(), (wr, br))
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = PatchEmbedFn.apply(case["px"].to(DEV), wd, bd, PATCH)
    y.backward(dy.to(DEV))
    ratio = (y.detach().double().cpu() - want.detach()).abs() / (GEMM_ATOL + GEMM_RTOL * want.detach().abs())
    print(f"patch embed {H}x{W}: worst {float(ratio.max()):.4f} of the bound")
    assert y.shape == want.shape and bool(torch.isfinite(y).all()) and bool((ratio <= 1).all())
    for name, got, ref, tol in (("dW", wd.grad, dw_ref, 4e-3), ("db", bd.grad, db_ref, 1e-4)):
        rel = float((got.double().cpu() - ref).norm() / ref.norm())
        print(f"  {name}: |ref| {float(ref.norm()):.3e}, relative error {rel:.3e}: {rel / tol:.4f} of the bound")
        assert float(ref.norm()) > 1e-4 and got.shape == ref.shape and bool(torch.isfinite(got).all()) and rel <= tol, (name, rel)


@pytest.mark.parametrize("H,W", IMAGES)
def test_pos_bicubic_fn(H, W):
    from multimodal_edema_prediction_amd.cxr_train import PosBicubicFn
    gh, gw = H // PATCH, W // PATCH
    pos = _params()["embeddings.position_embeddings"]
    dout = torch.randn(1, 1 + gh * gw, D, generator=torch.Generator().manual_seed(gh * 10 + gw))
    pr = pos.double().requires_grad_(True)
    want = R.pos_bicubic(pr, SIDE, gh, gw)
    (dref,) = torch.autograd.grad((want * dout[0].double()).sum(), pr)
    pd = pos.to(DEV).requires_grad_(True)
    out = PosBicubicFn.apply(pd, SIDE, gh, gw)
    out.backward(dout.to(DEV))
    assert out.shape == (1, 1 + gh * gw, D) and pd.grad.shape == pos.shape
    for name, got, ref in (("forward", out[0], want.detach()), ("backward", pd.grad, dref)):
        got = got.detach().double().cpu()
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"pos bicubic {SIDE} -> {gh}x{gw} {name}: max err {err:.3e} of max|ref| {scale:.3e}: {err / (R.BICUBIC_TOL * scale):.4f} of the bound")
        assert scale > 1e-4 and bool(torch.isfinite(got).all()) and err <= R.BICUBIC_TOL * scale, name
    if (gh, gw) == (SIDE, SIDE):
        assert torch.equal(out.detach().cpu(), pos)                 # onto the stored grid: a copy
