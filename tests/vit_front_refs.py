"""Plain torch restatements of the ViT front end and of GELU that the kernel-level tests of csrc/elementwise.hip compare against
(tests/test_gpu_vit_front_kernels.py, tests/test_gpu_vit_front_end.py).  Every function works in the dtype of its inputs (the GPU
tests hand it float64) and is differentiable, so the backward references come from autograd.  tests/test_vit_front_refs_cpu.py shows
that each one equals the oracle function it restates (oracle/vit_ref.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# (s, gh, gw) of the position-grid resize: down-sampling, up-sampling, non-square, small non-square, one output row, native in one
# axis only, every tap clamped, exact 2x
BICUBIC_CASES = [(37, 16, 16), (37, 48, 48), (37, 40, 23), (5, 3, 9), (4, 1, 7), (37, 37, 36), (3, 12, 2), (37, 74, 74)]
# the resize is within this of float64, relative to max|reference|: fp32 source coordinate, weights and accumulation give 5.3e-6 at
# worst (37 -> 48, where the fp32 scale 37/48 is inexact), torch's own fp32 interpolate the same; a wrong coefficient or clamp 1e-1
BICUBIC_TOL = 3e-5


def im2col(pix, patch, kpad):
    """pix [B, C, H, W] -> [B * gh * gw, kpad]: row [b, py, px], column [c, i, j] = pix[b, c, py*patch + i, px*patch + j], columns
    C*patch^2 .. kpad-1 zero.  Stride = patch, so the H % patch bottom rows and W % patch right columns take no part."""
    B, C, H, W = pix.shape
    gh, gw = H // patch, W // patch
    K = C * patch * patch
    cols = pix[:, :, :gh * patch, :gw * patch].unfold(2, patch, patch).unfold(3, patch, patch)          # [B, C, gh, gw, i, j]
    out = pix.new_zeros((B * gh * gw, kpad))
    out[:, :K] = cols.permute(0, 2, 3, 1, 4, 5).reshape(B * gh * gw, K)
    return out


def pos_bicubic(pos, s, gh, gw):
    """pos [1 + s*s, D] (or [1, 1 + s*s, D]) -> [1 + gh*gw, D]: the class row copied, the s x s patch grid resized by
    F.interpolate(mode="bicubic", align_corners=False) in pos's dtype.  (s, s) -> (s, s) goes through the resize too: its taps are
    exactly (0, 1, 0, 0)."""
    D = pos.shape[-1]
    p = pos.reshape(1 + s * s, D)
    grid = p[1:].reshape(1, s, s, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat((p[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)), dim=0)


def gelu(x):
    """0.5 x (1 + erf(x / sqrt 2)) in x's dtype."""
    return F.gelu(x)


def gelu_grad(x):
    """d gelu / dx, element by element, from autograd of F.gelu."""
    xr = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(xr).sum(), xr)
    return g


def front_end(sd, cfg, pixels, return_stream=False):
    """Dinov2's embeddings followed at once by the final LayerNorm (an encoder of zero blocks): the patch convolution as
    im2col x weight^T + bias, the class token in front, the position embeddings (resized unless the patch grid is the stored one),
    LayerNorm.  `sd` is keyed like Dinov2Model.state_dict(); `cfg` has .patch, .image_size, .hidden, .ln_eps (oracle.vit_ref.VitCfg).
    -> tokens [B, 1 + gh*gw, D]; with `return_stream` also the token stream before the LayerNorm."""
    B, C, H, W = pixels.shape
    p, D = cfg.patch, cfg.hidden
    gh, gw, s = H // p, W // p, cfg.image_size // p
    w = sd["embeddings.patch_embeddings.projection.weight"]
    x = im2col(pixels, p, C * p * p) @ w.reshape(D, -1).T + sd["embeddings.patch_embeddings.projection.bias"]
    x = torch.cat((sd["embeddings.cls_token"].reshape(1, 1, D).expand(B, 1, D), x.view(B, gh * gw, D)), dim=1)
    pos = sd["embeddings.position_embeddings"].reshape(1 + s * s, D)
    if (gh, gw) != (s, s):
        pos = pos_bicubic(pos, s, gh, gw)
    x = x + pos
    y = F.layer_norm(x, (D,), sd["layernorm.weight"], sd["layernorm.bias"], cfg.ln_eps)
    return (y, x) if return_stream else y
