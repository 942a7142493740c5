"""Split-key few-query attention (attention_fq_split.hip): head dim 64, <= 32 queries over any number of keys — the perceiver's
img_cross block on images above 32 x 32 patches.  Forward, logsumexp, head-averaged weights and backward against fp64 torch at the
tolerances of the one-workgroup few-query kernels (1e-4 rel, 1e-5 abs); the dropout mask against the wave-per-query kernels;
bitwise determinism, also next to a busy second stream; and AttnSmallFn's routing of > 1024 keys to these kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from multimodal_edema_prediction_amd import autograd_ops as A  # noqa: E402
from multimodal_edema_prediction_amd import functional as Fn  # noqa: E402

DEV = "cuda"
H, DH = 4, 64
D = H * DH
SCALE = DH ** -0.5


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def assert_close(got, want, rtol, atol, what=""):
    got = got.detach().float().cpu().double()
    want = want.detach().double()
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e}"


def ref_attn(q, k, v):
    """fp64 multi-head attention: q [B, Lq, D], k / v [B, Lk, D] -> (o, lse [B, H, Lq], head-averaged weights [B, Lq, Lk])."""
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    sp = lambda t, L: t.reshape(B, L, H, DH).transpose(1, 2)
    s = sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) * SCALE
    w = torch.softmax(s, dim=-1)
    return (w @ sp(v, Lk)).transpose(1, 2).reshape(B, Lq, D), torch.logsumexp(s, dim=-1), w.mean(dim=1)


SHAPES = [(2, 7, 1025), (2, 7, 1296), (1, 7, 1537), (1, 7, 2304), (1, 8, 4097), (2, 14, 2304), (1, 32, 1600), (1, 1, 3000)]


@pytest.mark.parametrize("B,Lq,Lk", SHAPES)
def test_fq_split_against_fp64(B, Lq, Lk):
    q, k, v, do = rnd(B, Lq, D, seed=1), rnd(B, Lk, D, seed=2), rnd(B, Lk, D, seed=3), rnd(B, Lq, D, seed=4)
    qr, kr, vr = [t.double().requires_grad_(True) for t in (q, k, v)]
    o_ref, lse_ref, avg_ref = ref_attn(qr, kr, vr)
    o_ref.backward(do.double())
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o, lse, avg = Fn.attn_fq_split_fwd(qd, kd, vd, B, Lq, Lk, H, SCALE, want_avg=True)
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    assert_close(lse, lse_ref, 1e-4, 1e-5, "lse")
    assert avg.shape == (B, Lq, Lk)
    assert_close(avg, avg_ref, 1e-4, 1e-5, "head-averaged weights")
    dq, dk, dv = Fn.attn_fq_split_bwd(do.to(DEV), o, lse, qd, kd, vd, B, Lq, Lk, H, SCALE)
    assert_close(dq, qr.grad, 1e-4, 1e-5, "dq")
    assert_close(dk, kr.grad, 1e-4, 1e-5, "dk")
    assert_close(dv, vr.grad, 1e-4, 1e-5, "dv")


@pytest.mark.parametrize("Lq,Lk", [(7, 1296), (11, 2304)])
def test_fq_split_shared_query_and_cls_skip(Lq, Lk):
    """The perceiver's operands: one query block shared by the batch (batch stride 0), K | V the column halves of a fused
    [B, Lk+1, 2D] projection whose CLS row is skipped, dK | dV into rows 1.. of a [B, Lk+1, 2D] gradient (row 0 untouched)."""
    B = 3
    q, kv, do = rnd(Lq, D, seed=5), rnd(B, Lk + 1, 2 * D, seed=6), rnd(B, Lq, D, seed=7)
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    o_ref, _, avg_ref = ref_attn(qr.expand(B, -1, -1), kvr[:, 1:, :D], kvr[:, 1:, D:])
    o_ref.backward(do.double())
    qd, kvd = q.to(DEV), kv.to(DEV)
    kbs = (Lk + 1) * 2 * D
    o, lse, avg = Fn.attn_fq_split_fwd(qd, kvd[:, 1:, :D], kvd[:, 1:, D:], B, Lq, Lk, H, SCALE, q_batch_stride=0, kv_batch_stride=kbs,
                                       want_avg=True)
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    assert_close(avg, avg_ref, 1e-4, 1e-5, "avg")
    dkv = torch.full((B, Lk + 1, 2 * D), 7.0, device=DEV)
    dq, _, _ = Fn.attn_fq_split_bwd(do.to(DEV), o, lse, qd, kvd[:, 1:, :D], kvd[:, 1:, D:], B, Lq, Lk, H, SCALE, q_batch_stride=0,
                                    kv_batch_stride=kbs, dkv_out=dkv[:, 1:, :])
    assert_close(dq.sum(0), qr.grad, 1e-4, 1e-5, "dq (summed over the batch)")
    assert_close(dkv[:, 1:], kvr.grad[:, 1:], 1e-4, 1e-5, "dkv")
    assert bool((dkv[:, 0] == 7.0).all()), "the skipped CLS row of dkv was written"


def test_fq_split_dropout_matches_wave_per_query_kernels():
    """With dropout on, the split forward draws the mask of attn_small_fwd (same (seed, stream_id) element index), its averaged
    weights included."""
    B, Lq, Lk = 2, 7, 1296
    q, k, v = rnd(B, Lq, D, seed=8).to(DEV), rnd(B, Lk, D, seed=9).to(DEV), rnd(B, Lk, D, seed=10).to(DEV)
    args = dict(dropout_p=0.25, seed=77, stream_id=3)
    o, _, avg = Fn.attn_fq_split_fwd(q, k, v, B, Lq, Lk, H, SCALE, want_avg=True, **args)
    avg_old = torch.zeros(B, Lq, Lk, device=DEV)
    o_old = Fn.attn_small_fwd(q, k, v, B, Lq, Lk, H, DH, SCALE, attn_avg=avg_old, **args)
    assert_close(o, o_old.cpu(), 1e-4, 1e-5, "split fwd vs wave-per-query fwd under the same dropout mask")
    assert_close(avg, avg_old.cpu(), 1e-4, 1e-5, "averaged weights under the same dropout mask")
    o_nod, _, _ = Fn.attn_fq_split_fwd(q, k, v, B, Lq, Lk, H, SCALE)
    assert float((o - o_nod).abs().max()) > 1e-3                                           # the mask is really applied


def test_fq_split_dropout_backward_regenerates_the_mask():
    """<dV, V> = <dO, o>: both are sum_j (P mask)_qj <dO_q, V_j>, true only if the backward draws the forward's mask."""
    B, Lq, Lk, p = 1, 7, 2304, 0.5
    q, k, v, do = (rnd(B, Lq, D, seed=11).to(DEV), rnd(B, Lk, D, seed=12).to(DEV), rnd(B, Lk, D, seed=13).to(DEV),
                   rnd(B, Lq, D, seed=14).to(DEV))
    args = dict(dropout_p=p, seed=123, stream_id=5)
    o, lse, avg = Fn.attn_fq_split_fwd(q, k, v, B, Lq, Lk, H, SCALE, want_avg=True, **args)
    _, _, dv = Fn.attn_fq_split_bwd(do, o, lse, q, k, v, B, Lq, Lk, H, SCALE, **args)
    lhs, rhs = float((dv.double() * v.double()).sum()), float((do.double() * o.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(rhs)), (lhs, rhs)
    zero = float((avg == 0).double().mean())                                                # dropped in all H heads: p^H
    assert abs(zero - p ** H) < 0.01, zero


def _launch(q, k, v, do, B, Lq, Lk):
    args = dict(dropout_p=0.1, seed=9, stream_id=2)
    o, lse, _ = Fn.attn_fq_split_fwd(q, k, v, B, Lq, Lk, H, SCALE, **args)
    dq, dk, dv = Fn.attn_fq_split_bwd(do, o, lse, q, k, v, B, Lq, Lk, H, SCALE, **args)
    return [o, lse, dq, dk, dv]


def test_fq_split_bitwise_deterministic():
    B, Lq, Lk = 4, 7, 2304
    ins = [rnd(B, Lq, D, seed=15), rnd(B, Lk, D, seed=16), rnd(B, Lk, D, seed=17), rnd(B, Lq, D, seed=18)]
    q, k, v, do = [t.to(DEV) for t in ins]
    a = _launch(q, k, v, do, B, Lq, Lk)
    b = _launch(q, k, v, do, B, Lq, Lk)
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), name


def test_fq_split_bit_stable_next_to_a_busy_stream():
    """Captured with a stream of short kernels on a second stream (test_gpu_bit_stability.py's screen): every replay must
    reproduce the eager launch bit for bit."""
    B, Lq, Lk = 8, 7, 1296
    ins = [rnd(B, Lq, D, seed=19), rnd(B, Lk, D, seed=20), rnd(B, Lk, D, seed=21), rnd(B, Lq, D, seed=22)]
    q, k, v, do = [t.to(DEV) for t in ins]
    x = torch.randn(448, 256, device=DEV)
    w = torch.randn(256, 256, device=DEV).bfloat16()
    lw, lb = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    side = torch.cuda.Stream()

    def body():
        cur = torch.cuda.current_stream()
        side.wait_stream(cur)
        y = x
        with torch.cuda.stream(side):
            for _ in range(200):
                y = Fn.gemm(Fn.layernorm(y, lw, lb, 1e-5), w, out_dtype=torch.float32)
        outs = _launch(q, k, v, do, B, Lq, Lk)
        cur.wait_stream(side)
        return outs, y

    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        body()
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs, keep = body()
    good = [t.clone() for t in _launch(q, k, v, do, B, Lq, Lk)]
    torch.cuda.synchronize()
    odd = 0
    for _ in range(20):
        g.replay()
        torch.cuda.synchronize()
        odd += sum(int(not torch.equal(a, b)) for a, b in zip(outs, good))
    assert odd == 0, f"{odd} of {20 * len(outs)} outputs deviated bit-wise next to a busy second stream"


@pytest.mark.parametrize("shared", [True, False])
def test_attn_small_fn_routes_many_keys_to_the_split_kernels(shared):
    """AttnSmallFn (every perceiver attention) at 2304 keys, above the 1536 the wave-per-query kernels take: o, the averaged
    weights, dQ (summed over the batch for a shared query block) and dKV (CLS row zero) against fp64 autograd."""
    B, Lq, Lk = 2, 7, 2304
    q = rnd(Lq, D, seed=23) if shared else rnd(B, Lq, D, seed=23)
    kv, do = rnd(B, Lk + 1, 2 * D, seed=24), rnd(B, Lq, D, seed=25)
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    o_ref, _, avg_ref = ref_attn(qr.expand(B, -1, -1) if shared else qr, kvr[:, 1:, :D], kvr[:, 1:, D:])
    o_ref.backward(do.double())
    qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    o, avg = A.attn_small(qd, kvd, H, SCALE, 0.0, 0, 0, 1, True)
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    assert_close(avg, avg_ref, 1e-4, 1e-5, "avg")
    o.backward(do.to(DEV))
    assert_close(qd.grad, qr.grad, 1e-4, 1e-5, "dq")
    assert_close(kvd.grad, kvr.grad, 1e-4, 1e-5, "dkv")
    assert bool((kvd.grad[:, 0] == 0).all())


def test_attn_small_fn_keeps_the_old_kernels_up_to_1024_keys():
    """<= 1024 keys (the 256-patch teacher) keep the one-workgroup kernels and their bits."""
    B, Lq, Lk = 2, 7, 1024
    q, kv = rnd(Lq, D, seed=26).to(DEV), rnd(B, Lk, 2 * D, seed=27).to(DEV)
    o, _ = A.attn_small(q, kv, H, SCALE)
    o_old = Fn.attn_small_fwd(q, kv[:, :, :D], kv[:, :, D:], B, Lq, Lk, H, DH, SCALE, q_batch_stride=0, kv_batch_stride=kv.stride(0))
    assert torch.equal(o, o_old)
