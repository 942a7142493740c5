"""CPU checks behind the kernel-level GPU tests of csrc/elementwise.hip: the restatements of tests/vit_front_refs.py equal the oracle
functions they restate (oracle/vit_ref.py, torch's own conv2d / gelu), so the float64 references of test_gpu_vit_front_kernels.py and
test_gpu_vit_front_end.py are themselves checked without a device."""
import math

import pytest
import torch
import torch.nn.functional as F

import vit_front_refs as R
from oracle import vit_ref


@pytest.mark.parametrize("B,C,H,W,patch", [(2, 3, 28, 42, 14), (1, 3, 37, 30, 14), (3, 1, 16, 24, 8), (2, 2, 13, 22, 4)])
def test_im2col_times_weight_is_the_strided_convolution(B, C, H, W, patch):
    g = torch.Generator().manual_seed(H * 100 + W)
    pix = torch.randn(B, C, H, W, generator=g).double()
    w, b = torch.randn(5, C, patch, patch, generator=g).double(), torch.randn(5, generator=g).double()
    K = C * patch * patch
    kpad = (K + 7) // 8 * 8 + 8
    cols = R.im2col(pix, patch, kpad)
    gh, gw = H // patch, W // patch
    assert cols.shape == (B * gh * gw, kpad) and bool((cols[:, K:] == 0).all())
    got = (cols[:, :K] @ w.reshape(5, K).T + b).view(B, gh, gw, 5).permute(0, 3, 1, 2)
    torch.testing.assert_close(got, F.conv2d(pix, w, b, stride=patch), rtol=1e-12, atol=1e-12)
    # [b, py, px] rows, [c, i, j] columns: one entry by hand
    bb, py, px, c, i, j = B - 1, gh - 1, gw - 1, C - 1, patch - 1, 1
    assert cols[(bb * gh + py) * gw + px, (c * patch + i) * patch + j] == pix[bb, c, py * patch + i, px * patch + j]
    assert R.im2col(pix.float(), patch, kpad).dtype == torch.float32


@pytest.mark.parametrize("s,gh,gw", R.BICUBIC_CASES + [(5, 5, 5), (37, 37, 37)])
def test_pos_bicubic_equals_the_oracle_resize(s, gh, gw):
    g = torch.Generator().manual_seed(s * 10000 + gh * 100 + gw)
    pos = torch.randn(1, 1 + s * s, 8, generator=g)
    cfg = vit_ref.VitCfg(hidden=8, patch=14, image_size=14 * s)
    want = vit_ref.interpolate_pos_embed(pos, cfg, 14 * gh, 14 * gw)[0].double()           # fp32 interpolate
    got = R.pos_bicubic(pos.double(), s, gh, gw)
    assert got.shape == want.shape == (1 + gh * gw, 8)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"fp32 interpolate against float64: {err / scale:.2e} of max|ref| (bound {R.BICUBIC_TOL:.0e})")
    assert err <= R.BICUBIC_TOL * scale
    assert torch.equal(got[0], pos[0, 0].double())
    if (gh, gw) == (s, s):
        assert torch.equal(got, pos[0].double())
    # differentiable, and the gradient is the transpose: <resize(p), d> = <p, resize^T(d)> for a second, unrelated pair
    p = torch.randn(1 + s * s, 8, generator=g).double().requires_grad_(True)
    d = torch.randn(1 + gh * gw, 8, generator=g).double()
    (dp,) = torch.autograd.grad((R.pos_bicubic(p, s, gh, gw) * d).sum(), p)
    lhs, rhs = float((R.pos_bicubic(p.detach(), s, gh, gw) * d).sum()), float((p.detach() * dp).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(R.pos_bicubic(p.detach(), s, gh, gw).norm() * d.norm())


def test_gelu_and_its_gradient():
    x = torch.linspace(-9.0, 9.0, 2001).double()
    # x Phi(x) with Phi by erfc, which keeps its relative accuracy on the negative tail; F.gelu forms 1 + erf there and is off by
    # up to 2^-53 |x| absolute, nine orders of magnitude below the absolute term of the GPU tests' bound
    want = 0.5 * x * torch.erfc(-x / math.sqrt(2.0))
    torch.testing.assert_close(R.gelu(x), want, rtol=1e-14, atol=1e-15)
    dwant = 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    torch.testing.assert_close(R.gelu_grad(x), dwant, rtol=1e-12, atol=1e-15)
    assert R.gelu_grad(x).shape == x.shape and not x.requires_grad


def _front_sd(D, s, patch, g):
    r = lambda *sh: torch.randn(*sh, generator=g).double()
    return {"embeddings.cls_token": r(1, 1, D), "embeddings.position_embeddings": r(1, 1 + s * s, D),
            "embeddings.patch_embeddings.projection.weight": r(D, 3, patch, patch) / math.sqrt(3 * patch * patch),
            "embeddings.patch_embeddings.projection.bias": r(D), "layernorm.weight": 1 + 0.3 * r(D), "layernorm.bias": 0.3 * r(D)}


@pytest.mark.parametrize("H,W", [(70, 70), (42, 56), (75, 61), (98, 98), (70, 75)])
def test_front_end_equals_the_oracle_vit_without_blocks(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    D, s, patch = 16, 5, 14
    sd = _front_sd(D, s, patch, g)
    cfg = vit_ref.VitCfg(hidden=D, layers=0, heads=1, patch=patch, image_size=patch * s)
    px = torch.randn(2, 3, H, W, generator=g).double()
    cls, patches = vit_ref.vit_forward(sd, cfg, px)
    want = torch.cat((cls.unsqueeze(1), patches), dim=1)
    got, stream = R.front_end(sd, cfg, px, return_stream=True)
    gh, gw = H // patch, W // patch
    assert got.shape == want.shape == (2, 1 + gh * gw, D) and stream.shape == got.shape
    if (gh, gw) == (s, s) and H == W:
        tol = 1e-12                                                  # the oracle adds the stored positions as they are: float64 both
    else:
        # the oracle resizes in fp32 (`.float()`): the positions differ by at most BICUBIC_TOL * max|pos|, and the LayerNorm hands
        # that on times |w| * rstd
        rstd = (stream.var(-1, unbiased=False) + cfg.ln_eps).rsqrt().max()
        tol = float(R.BICUBIC_TOL * sd["embeddings.position_embeddings"].abs().max() * sd["layernorm.weight"].abs().max() * rstd)
    err = float((got - want).abs().max())
    print(f"front_end against vit_forward(layers=0): max err {err:.2e} (tol {tol:.2e})")
    assert err <= tol
    torch.testing.assert_close(F.layer_norm(stream, (D,), sd["layernorm.weight"], sd["layernorm.bias"], cfg.ln_eps), got, rtol=0, atol=0)
