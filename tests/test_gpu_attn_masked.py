"""Key-masked small attention (medp_attn_small_masked_fwd / _bwd; nn.MultiheadAttention(key_padding_mask=...)) against an fp64
restatement written out below: o, the head-averaged weights, dq, dk, dv; exact zeros at masked keys (outputs pre-filled with NaN),
a fully masked batch element, bit-identity with the unmasked kernels under an all-zero mask, and dropout 0.25 against the host
replica of the kernels' mask (tests/dropout_twin.py) — the stream is indexed over the FULL Lk, so the surviving keys keep the draws
the unmasked call gives them.  Tolerance: the project's kernel tolerance 1e-4 (fp32 kernels, bf16-representable inputs, O(1) values).
Shapes: the probe's head layout at 18 keys (3 x 4 x 32, 7 queries) and 2 x 2 x 12 with 5 queries over 70 keys (two keys per lane,
Lk % 64 != 0); q shared by the batch and per batch; K | V the two column halves of one projection, as AttnSmallFn passes them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_twin as T  # noqa: E402
from dropout_twin import pinned_epoch  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
SHAPES = [(3, 4, 32, 7, 18), (2, 2, 12, 5, 70)]
SEED, SID = 1234567, 70


def make_mask(kind, B, Lk, gen):
    m = torch.rand(B, Lk, generator=gen) < 0.3
    if kind == "mixed":
        m[0] = True                      # a batch element with every key masked
        m[1] = False                     # and one with none
    return m


def make_inputs(B, H, dh, Lq, Lk, shared, seed=0):
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    bf = lambda t: t.bfloat16().float()  # noqa: E731
    q = bf(torch.randn((Lq, D) if shared else (B, Lq, D), generator=g))
    kv = bf(torch.randn(B, Lk, 2 * D, generator=g))
    do = bf(torch.randn(B, Lq, D, generator=g))
    return q, kv, do, g


def reference(q, kv, do, mask, H, scale, drop=None):
    """fp64: softmax over the unmasked keys (a fully masked row: all-zero probabilities), optional dropout factor [B,H,Lq,Lk]."""
    B, Lk, D2 = kv.shape
    D, dh = D2 // 2, D2 // 2 // H
    shared = q.dim() == 2
    q64 = q.double().requires_grad_(True)
    kv64 = kv.double().requires_grad_(True)
    qb = (q64.unsqueeze(0).expand(B, -1, -1) if shared else q64).view(B, -1, H, dh).transpose(1, 2)
    k = kv64[..., :D].view(B, Lk, H, dh).transpose(1, 2)
    v = kv64[..., D:].view(B, Lk, H, dh).transpose(1, 2)
    s = (qb @ k.transpose(-1, -2)) * scale
    dead = mask.all(-1)[:, None, None, None]
    s = s.masked_fill(mask[:, None, None, :] & ~dead, float("-inf"))
    p = torch.softmax(s, -1) * (~dead)
    if drop is not None:
        p = p * drop
    o = (p @ v).transpose(1, 2).reshape(B, -1, D)
    (o * do.double()).sum().backward()
    dq = q64.grad if not shared else None
    return o.detach(), p.detach().mean(1), q64.grad, kv64.grad, dq


def run_masked(q, kv, do, mask, H, scale, p=0.0, want_avg=True):
    from multimodal_edema_prediction_amd import functional as Fn
    B, Lk, D2 = kv.shape
    D, dh, Lq = D2 // 2, D2 // 2 // H, q.shape[-2]
    shared = q.dim() == 2
    qg, kvg, dog = q.cuda(), kv.cuda(), do.cuda()
    mg = None if mask is None else mask.to(torch.uint8).cuda()
    kw = dict(q_batch_stride=0 if shared else None, kv_batch_stride=kvg.stride(0), dropout_p=p, seed=SEED, stream_id=SID)
    if mask is None:
        avg = torch.zeros(B, Lq, Lk, device="cuda") if want_avg else None
    else:
        avg = torch.full((B, Lq, Lk), float("nan"), device="cuda") if want_avg else None
    o = Fn.attn_small_fwd(qg, kvg[..., :D], kvg[..., D:], B, Lq, Lk, H, dh, scale, attn_avg=avg, key_mask=mg, **kw)
    dkv = torch.full((B, Lk, 2 * D), float("nan"), device="cuda")
    dq, _, _ = Fn.attn_small_bwd(dog, qg, kvg[..., :D], kvg[..., D:], B, Lq, Lk, H, dh, scale, dkv_out=dkv, key_mask=mg, **kw)
    torch.cuda.synchronize()
    return o.cpu(), None if avg is None else avg.cpu(), dq.cpu(), dkv.cpu()


def check_against_reference(shape, shared, kind, p):
    B, H, dh, Lq, Lk = shape
    q, kv, do, g = make_inputs(B, H, dh, Lq, Lk, shared)
    mask = make_mask(kind, B, Lk, g)
    scale = dh ** -0.5
    drop = None
    if p > 0:
        drop = torch.from_numpy(T.mask_scale(SEED, SID, T.attn_index(B, H, Lq, Lk), p).astype(np.float64))
    with pinned_epoch(None):
        o, avg, dq, dkv = run_masked(q, kv, do, mask, H, scale, p)
    ro, ravg, rdq, rdkv, _ = reference(q, kv, do, mask, H, scale, drop)
    for t in (o, avg, dq, dkv):
        assert bool(torch.isfinite(t).all()), "NaN / inf (an output element left unwritten, or 0 * inf in a fully masked row)"
    dq_sum = dq.double().sum(0) if shared else dq.double()
    errs = {"o": (o.double() - ro).abs().max().item(), "attn_avg": (avg.double() - ravg).abs().max().item(),
            "dq": (dq_sum - rdq).abs().max().item(), "dkv": (dkv.double() - rdkv).abs().max().item()}
    print(shape, "shared" if shared else "per-batch", kind, p, errs)
    assert max(errs.values()) <= TOL, errs
    gone = mask[:, None, :].expand(B, Lq, Lk)
    assert bool((avg[gone] == 0).all()), "attn_avg must be exactly 0 at masked keys"
    assert bool((dkv[mask] == 0).all()), "dk / dv rows of masked keys must be exact zeros"
    if kind == "mixed":                  # the fully masked element: zero output, zero weights, zero gradients
        assert bool((o[0] == 0).all()) and bool((avg[0] == 0).all()) and bool((dq[0] == 0).all()) and bool((dkv[0] == 0).all())
    return avg, mask


@pytest.mark.parametrize("kind", ["random", "mixed"])
@pytest.mark.parametrize("shared", [True, False], ids=["q-shared", "q-per-batch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_average_and_gradients_match_fp64(shape, shared, kind):
    check_against_reference(shape, shared, kind, 0.0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_all_zero_mask_is_bit_identical_to_the_unmasked_kernels(shape):
    """Head dims 32 and 12: the unmasked call takes the wave-per-query kernels too (the few-query kernels are head dim 64 only)."""
    B, H, dh, Lq, Lk = shape
    q, kv, do, _ = make_inputs(B, H, dh, Lq, Lk, shared=False, seed=1)
    for p in (0.0, 0.25):
        with pinned_epoch(None):
            a = run_masked(q, kv, do, torch.zeros(B, Lk, dtype=torch.bool), H, dh ** -0.5, p)
            b = run_masked(q, kv, do, None, H, dh ** -0.5, p)
        for name, x, y in zip(("o", "attn_avg", "dq", "dkv"), a, b):
            if name == "attn_avg" and H > 2:
                # the unmasked forward adds the heads with float atomics in whatever order their workgroups run (three or more
                # terms: not associative); the masked form adds them in head order.  Same terms, so a few ulp of O(1/Lk) values.
                assert (x - y).abs().max().item() <= 1e-6, name
            else:
                assert torch.equal(x, y), (name, p)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_keeps_the_unmasked_calls_stream_and_is_reproducible(shape):
    B, H, dh, Lq, Lk = shape
    p = 0.25
    # against fp64 with the host replica of the kernels' mask, drawn at ((b H + h) Lq + q) Lk + j over the full Lk
    avg, mask = check_against_reference(shape, False, "mixed", p)
    # next to the unmasked call with the same seed: attn_avg is 0 at a surviving key exactly where every head dropped it, and the
    # two calls must agree on those positions (and with the replica)
    q, kv, do, _ = make_inputs(B, H, dh, Lq, Lk, shared=False)
    with pinned_epoch(None):
        o1, a1, dq1, dkv1 = run_masked(q, kv, do, mask, H, dh ** -0.5, p)
        o2, a2, dq2, dkv2 = run_masked(q, kv, do, mask, H, dh ** -0.5, p)
        _, au, _, _ = run_masked(q, kv, do, None, H, dh ** -0.5, p)
    live = (~mask)[:, None, :].expand(B, Lq, Lk)
    assert torch.equal((a1 == 0)[live], (au == 0)[live]), "dropped positions on surviving keys differ from the unmasked call's"
    keep_all = torch.from_numpy(T.keep_mask(SEED, SID, T.attn_index(B, H, Lq, Lk), p)).any(1)
    assert torch.equal((a1 != 0)[live], keep_all[live])
    for x, y in ((o1, o2), (a1, a2), (dq1, dq2), (dkv1, dkv2)):
        assert torch.equal(x, y), "two runs differ"


def test_autograd_function_takes_the_mask_and_defaults_to_none():
    """AttnSmallFn through `attn_small(..., key_mask=pad)`: same numbers as the direct calls, gradients to q and the K | V projection."""
    from multimodal_edema_prediction_amd import autograd_ops as A
    B, H, dh, Lq, Lk = SHAPES[0]
    q, kv, do, g = make_inputs(B, H, dh, Lq, Lk, shared=True)
    mask = make_mask("mixed", B, Lk, g)
    qg, kvg = q.cuda().requires_grad_(True), kv.cuda().requires_grad_(True)
    o, avg = A.attn_small(qg, kvg, H, dh ** -0.5, want_avg=True, key_mask=mask.cuda())
    (o * do.cuda()).sum().backward()
    ro, ravg, rdq, rdkv, _ = reference(q, kv, do, mask, H, dh ** -0.5)
    assert (o.detach().cpu().double() - ro).abs().max().item() <= TOL
    assert (avg.cpu().double() - ravg).abs().max().item() <= TOL
    assert (qg.grad.cpu().double() - rdq).abs().max().item() <= TOL
    assert (kvg.grad.cpu().double() - rdkv).abs().max().item() <= TOL
    o2, none = A.attn_small(qg, kvg, H, dh ** -0.5)                    # every current caller: no mask, no average
    assert none is None and o2.shape == o.shape
