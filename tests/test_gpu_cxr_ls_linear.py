"""cxr_train.ls_linear_backward — the gradients of out = (x W^T + b) * lam + res that both halves of a trainable Dinov2 block use —
tensor by tensor against fp64 computed from the SAME rounded operands (the device's own bf16 copies of dY and lam * W, read back), so
operand rounding is not part of the error and a wrong sign or factor in one output cannot hide in a whole-encoder cosine.

Bound per element: every output is a sum of n fp32-accumulated terms followed by at most two fp32 multiplies, so
|err| <= (n + 4) * 2^-24 * sum|terms|, with n = M for dW and db, M + K for dlam, N for dX, and sum|terms| the same expression evaluated
on absolute values in fp64; a bf16 dX adds one bf16 rounding, 2^-8 * |dX_ref|.  The shapes are the smallest that meet gemm_tn's
alignment rule (N % 8 == 0, K % 8 == 0, row stride % 8 == 0), with M = 24, 72 and 130: below 64 rows, and past one and two multiples of 64 without being one."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
SHAPES = [(24, 16, 40), (72, 8, 8), (130, 24, 200)]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Device inputs and the fp64 reference with its per-element sums of absolute terms (built once per shape, never written to)."""
    from multimodal_edema_prediction_amd import functional as Fn
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(M * 10000 + N * 100 + K)
    dy = torch.randn(M, N, generator=g).to(dev)
    x16 = torch.randn(M, K, generator=g).to(dev).to(BF16)
    W = (0.2 * torch.randn(N, K, generator=g)).to(dev)
    b = (0.1 * torch.randn(N, generator=g)).to(dev)
    lam = (0.5 + torch.rand(N, generator=g)).to(dev)
    dyb = Fn.to_bf16(dy)
    lw16 = Fn.transpose_to_bf16((lam[:, None] * W).contiguous())[:, :N].t()        # bf16(lam * W) as the dX GEMM reads it, [N, K]
    h = lambda t: t.detach().to("cpu").to(F64)
    dy_h, dyb_h, x_h, W_h, b_h, lam_h, lw_h = h(dy), h(dyb), h(x16), h(W), h(b), h(lam), h(lw16)
    G, Ga = dyb_h.t() @ x_h, dyb_h.abs().t() @ x_h.abs()
    s, sa = dy_h.sum(0), dy_h.abs().sum(0)
    ref = {"dW": lam_h[:, None] * G, "db": lam_h * s, "dlam": (W_h * G).sum(1) + b_h * s, "dX": dyb_h @ lw_h}
    mag = {"dW": lam_h.abs()[:, None] * Ga, "db": lam_h.abs() * sa, "dlam": (W_h.abs() * Ga).sum(1) + b_h.abs() * sa,
           "dX": dyb_h.abs() @ lw_h.abs()}
    n = {"dW": M, "db": M, "dlam": M + K, "dX": N}
    return (dy, dyb, x16, W, b, lam), ref, mag, n


@pytest.mark.parametrize("dx_dtype", [F32, BF16, None], ids=["dx_fp32", "dx_bf16", "no_dx"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_ls_linear_backward_matches_fp64_on_the_same_operands(M, N, K, dx_dtype):
    from multimodal_edema_prediction_amd.cxr_train import ls_linear_backward
    args, ref, mag, n = _case(M, N, K)
    dx, dW, db, dlam = ls_linear_backward(*args, dx_dtype=dx_dtype)
    torch.cuda.synchronize()
    got = {"dW": dW, "db": db, "dlam": dlam}
    if dx_dtype is None:
        assert dx is None
    else:
        assert dx.dtype == dx_dtype
        got["dX"] = dx
    for name, t in got.items():
        assert t.shape == ref[name].shape, (name, tuple(t.shape))
        err = (t.detach().to("cpu").to(F64) - ref[name]).abs()
        bound = (n[name] + 4) * U * mag[name]
        if t.dtype == BF16:
            bound = bound + 2.0 ** -8 * ref[name].abs()
        worst = float((err / mag[name].clamp_min(1e-300)).max())
        print(f"{name} M={M} N={N} K={K} dx={dx_dtype}: max err / sum|terms| = {worst:.3e}, bound {(n[name] + 4) * U:.3e}"
              + (" + 2^-8 |ref| / sum|terms|" if t.dtype == BF16 else ""))
        assert bool(torch.isfinite(err).all()) and bool((err <= bound).all()), (name, worst, float((err - bound).max()))
