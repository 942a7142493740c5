"""DuETT's attention in training form on the matrix cores (csrc/attention_dh16.hip: 2 heads of dim 12 over 49 / 97 tokens,
dropout on the probabilities): forward and all three gradients against fp64 on the bf16-rounded operands, the dropout mask
against the fp32 VALU kernels of attention_small.hip (same counter hash), the autograd function the student path uses, and the
inference export of the same file, which is the same arithmetic."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(qkv, do, H):
    B, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    x = qkv.bfloat16().double().requires_grad_(True)             # the kernels round q, k, v to bf16
    q, k, v = [x[..., i * D:(i + 1) * D].reshape(B, N, H, dh).transpose(1, 2) for i in range(3)]
    w = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
    o = (w @ v).transpose(1, 2).reshape(B, N, D)
    o.backward(do.double())
    return o.detach(), x.grad


def _call(qkv, do, H, p=0.0, seed=0, sid=0, io16=False):
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    B, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    if io16:
        qkv, do = qkv.to(torch.bfloat16), do.to(torch.bfloat16)
    o = torch.empty(B, N, D, device=DEV, dtype=qkv.dtype)
    lse, delta = torch.empty(B * H * N, device=DEV), torch.empty(B * H * N, device=DEV)
    dqkv = torch.full_like(qkv, float("nan"))
    check(lib().medp_attn_dh16_train_fwd(ptr(qkv), D3, ptr(o), D, ptr(lse), int(io16), B, N, H, dh, dh ** -0.5, p, seed, sid, stream()), "fwd")
    check(lib().medp_attn_dh16_train_bwd(ptr(do), D, ptr(qkv), D3, ptr(lse), ptr(delta), ptr(dqkv), D3, int(io16), B, N, H, dh, dh ** -0.5, p,
                                         seed, sid, stream()), "bwd")
    return o, dqkv


@pytest.mark.parametrize("B,N,H,dh,p", [(5, 97, 2, 12, 0.0), (7, 49, 2, 12, 0.3), (2, 130, 1, 16, 0.1), (1, 5, 3, 4, 0.0)])
def test_bf16_hand_over_form_has_the_bits_of_the_fp32_form(B, N, H, dh, p):
    """io_bf16 = 1 reads bf16 q | k | v / dO and writes bf16 o / dQ | dK | dV: the fp32 form rounds the same fp32 values to the same MFMA
    operands, so on inputs that are exactly representable in bf16 both compute the same numbers and differ only by the final rounding."""
    torch.manual_seed(3)
    qkv = (torch.randn(B, N, 3 * H * dh) * 0.8).to(DEV).to(torch.bfloat16).float()
    do = torch.randn(B, N, H * dh).to(DEV).to(torch.bfloat16).float()
    o32, g32 = _call(qkv, do, H, p, seed=5, sid=3)
    o16, g16 = _call(qkv, do, H, p, seed=5, sid=3, io16=True)
    assert o16.dtype == torch.bfloat16 and g16.dtype == torch.bfloat16 and not torch.isnan(g16.float()).any()
    assert torch.equal(o16, o32.to(torch.bfloat16)) and torch.equal(g16, g32.to(torch.bfloat16))


@pytest.mark.parametrize("B,N,H,dh", [(5, 97, 2, 12), (7, 49, 2, 12), (3, 17, 2, 12), (2, 130, 1, 16), (2, 257, 2, 8), (1, 5, 3, 4)])
def test_forward_and_gradients_against_fp64(B, N, H, dh):
    torch.manual_seed(0)
    qkv = (torch.randn(B, N, 3 * H * dh) * 0.8).to(DEV)
    do = torch.randn(B, N, H * dh).to(DEV)
    o, dqkv = _call(qkv, do, H)
    o_ref, g_ref = _ref(qkv.cpu(), do.cpu(), H)
    assert float((o.cpu().double() - o_ref).abs().max()) <= 1e-2 * float(o_ref.abs().max())          # bf16 probabilities / V
    assert not torch.isnan(dqkv).any()                                                                 # every element written
    err = float((dqkv.cpu().double() - g_ref).abs().max())
    assert err <= 2e-2 * float(g_ref.abs().max()), err
    a, b = dqkv.cpu().double().flatten(), g_ref.flatten()
    assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.9995
    o2, dqkv2 = _call(qkv, do, H)
    assert torch.equal(o, o2) and torch.equal(dqkv, dqkv2)                                             # nothing is accumulated in memory


def test_dropout_mask_is_the_one_of_the_fp32_kernels_and_backward_regenerates_it():
    from multimodal_edema_prediction_amd import functional as Fn
    torch.manual_seed(1)
    B, N, H, dh, p = 4, 97, 2, 12, 0.3
    D = H * dh
    qkv = (torch.randn(B, N, 3 * D) * 0.8).to(DEV)
    do = torch.randn(B, N, D).to(DEV)
    o, dqkv = _call(qkv, do, H, p, seed=99, sid=7)
    o_valu = Fn.attn_small_fwd(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], B, N, N, H, dh, dh ** -0.5, q_batch_stride=N * 3 * D,
                               kv_batch_stride=N * 3 * D, dropout_p=p, seed=99, stream_id=7)
    assert float((o - o_valu).abs().max()) <= 2e-2 * float(o_valu.abs().max())                        # same mask: only bf16 rounding apart
    o0, _ = _call(qkv, do, H)
    assert float((o - o0).abs().max()) > 0.1 * float(o0.abs().max())                                   # the mask does something
    # <dO, o(V)> is linear in V with gradient dV: <dV, V> = <dO, o> (V rounded to bf16 as the kernel sees it)
    v = qkv[..., 2 * D:].bfloat16().double()
    lhs = float((dqkv[..., 2 * D:].double() * v).sum())
    rhs = float((do.double() * o.double()).sum())
    assert abs(lhs - rhs) <= 2e-2 * max(1.0, abs(rhs))


def test_autograd_function_takes_the_mfma_path_and_matches_the_fp32_mode():
    from multimodal_edema_prediction_amd import functional as Fn
    from multimodal_edema_prediction_amd.duett_train import SelfAttnQKVFn
    torch.manual_seed(2)
    B, N, H, dh = 6, 49, 2, 12
    qkv = (torch.randn(B, N, 3 * H * dh) * 0.8).to(DEV)
    do = torch.randn(B, N, H * dh).to(DEV)

    def run(mode):
        x = qkv.clone().requires_grad_(True)
        with Fn.precision_mode(mode):
            o = SelfAttnQKVFn.apply(x, H, 0.0, 0, 0)
            o.backward(do)
        return o.detach(), x.grad

    o16, g16 = run("bf16")
    o32, g32 = run("fp32")
    assert float((o16 - o32).abs().max()) <= 1e-2 * float(o32.abs().max())
    assert float((g16 - g32).abs().max()) <= 3e-2 * float(g32.abs().max())
    assert not torch.equal(o16, o32)                                                                   # (two different kernels did run)


def _inference(qkv, H, o=None):
    from multimodal_edema_prediction_amd.abi import lib, ptr, stream
    B, N, D3 = qkv.shape
    D = D3 // 3
    o = torch.full((B, N, D), float("nan"), device=DEV, dtype=torch.bfloat16) if o is None else o
    return lib().medp_attn_dh16_fwd(ptr(qkv), D3, ptr(o), D, B, N, H, D // H, (D // H) ** -0.5, stream()), o


# one shape per NT bucket edge (2 / 4 / 7 / 10 / 17 key tiles of 16) and the ragged ones
@pytest.mark.parametrize("B,N,H,dh", [(1, 16, 1, 4), (3, 17, 2, 12), (2, 33, 2, 12), (2, 97, 2, 12), (1, 113, 1, 16), (1, 161, 3, 8), (1, 272, 1, 12)])
def test_inference_export_has_the_bits_of_the_training_forward(B, N, H, dh):
    """medp_attn_dh16_fwd (fp32 in, bf16 out) and medp_attn_dh16_train_fwd at p = 0 (fp32 in and out) are one arithmetic: the same MFMA chain,
    the same exp2(fma) and the same ascending sum, so the bf16 output is the fp32 output rounded."""
    torch.manual_seed(4)
    qkv = (torch.randn(B, N, 3 * H * dh) * 0.8).to(DEV)
    rc, o16 = _inference(qkv, H)
    assert rc == 0
    o32, _ = _call(qkv, torch.zeros(B, N, H * dh, device=DEV), H)
    assert not torch.isnan(o16.float()).any()                                                          # every element written
    assert torch.equal(o16, o32.to(torch.bfloat16))


def test_shapes_outside_the_kernels_return_minus_two():
    """Both forwards answer -2 (nothing launched: the caller takes attention_small.hip) to a head dim, a token count or a row stride they are not
    built for.  An o that is only 8-byte aligned is enough for the inference form's 8-byte stores of bf16, not for the training form."""
    from multimodal_edema_prediction_amd.abi import lib, ptr, stream

    def both(B, N, H, dh, ld):
        D = H * dh
        qkv = torch.zeros(B * N, ld, device=DEV)
        o16, o32, lse = torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16), torch.zeros(B * N, D, device=DEV), torch.zeros(B * H * N, device=DEV)
        return (lib().medp_attn_dh16_fwd(ptr(qkv), ld, ptr(o16), D, B, N, H, dh, dh ** -0.5, stream()),
                lib().medp_attn_dh16_train_fwd(ptr(qkv), ld, ptr(o32), D, ptr(lse), 0, B, N, H, dh, dh ** -0.5, 0.0, 0, 0, stream()))

    assert both(1, 16, 1, 20, 60) == (-2, -2)                     # head dim 20
    assert both(1, 273, 1, 4, 12) == (-2, -2)                     # N = 273
    assert both(1, 16, 2, 12, 3 * 24 + 2) == (-2, -2)             # row stride 3 D + 2
    assert both(1, 16, 2, 12, 3 * 24) == (0, 0)                   # (the same shape with the plain stride is taken)
    torch.manual_seed(5)
    B, N, H, dh = 1, 16, 2, 12
    D = H * dh
    qkv = (torch.randn(B, N, 3 * D) * 0.8).to(DEV)
    rc, o_ref = _inference(qkv, H)
    buf16 = torch.full((B * N * D + 4,), float("nan"), device=DEV, dtype=torch.bfloat16)
    rc8, o8 = _inference(qkv, H, o=buf16[4:].view(B, N, D))       # 8 bytes past a 16-byte boundary
    assert (rc, rc8) == (0, 0) and torch.equal(o8, o_ref) and torch.isnan(buf16[:4].float()).all()
    buf32, lse = torch.zeros(B * N * D + 2, device=DEV), torch.zeros(B * H * N, device=DEV)
    assert lib().medp_attn_dh16_train_fwd(ptr(qkv), 3 * D, ptr(buf32[2:]), D, ptr(lse), 0, B, N, H, dh, dh ** -0.5, 0.0, 0, 0, stream()) == -2
