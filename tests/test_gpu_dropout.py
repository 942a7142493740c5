"""Every dropout kernel against the host replica of its mask (tests/dropout_twin.py) and fp64: the masks bit for bit, GELU + dropout and
dropout + add forward and backward, their autograd nodes, attention with dropout on the probabilities (thread-per-key and wave-per-query
kernels, the perceiver's shared-query form, the split-key kernels, DuETT's MFMA kernels), and the RNG epoch of a replayed graph.
Each test pins the library's epoch counter (a tensor of its own, or NULL) and hands the registration back afterwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_twin as T  # noqa: E402
from dropout_twin import pinned_epoch  # noqa: E402
from multimodal_edema_prediction_amd import autograd_ops as A  # noqa: E402
from multimodal_edema_prediction_amd import functional as Fn  # noqa: E402
from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream  # noqa: E402

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ms_flat(shape, p, seed, sid, epoch):
    """fp32 mask * scale of an element-wise kernel over a contiguous tensor of `shape` (CPU tensor)."""
    return torch.from_numpy(T.mask_scale(seed, sid, T.flat_index(shape), p, epoch))


def ms_attn(B, H, Lq, Lk, p, seed, sid, epoch):
    return torch.from_numpy(T.mask_scale(seed, sid, T.attn_index(B, H, Lq, Lk), p, epoch))


def assert_close(got, want, rtol, atol, what=""):
    got = got.detach().float().cpu().double()
    want = want.detach().double()
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e}"


def gelu64(x):
    return torch.nn.functional.gelu(x.double())


def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


# ------------------------------------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("n", [13, 4099, 2048 * 256 * 2 + 13])                 # the last: past the 2048-block grid-stride cap
@pytest.mark.parametrize("epoch", [None, 0, 1, 7])
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_dropout_mask_bit_exact(p, epoch, n):
    seed, sid = 2 ** 31 - 2 if n == 13 else 1000003 + n, 17 + int(10 * p)
    with pinned_epoch(epoch):
        y = torch.ones(n, device=DEV)
        out = torch.empty_like(y)
        check(lib().medp_dropout_add(ptr(y), None, ptr(out), n, p, seed, sid, stream()), "dropout_add")
        want = ms_flat((n,), p, seed, sid, epoch)
        assert torch.equal(out.cpu(), want), f"{int((out.cpu() != want).sum())} of {n} elements differ from the replica"


@pytest.mark.parametrize("shape,p,epoch", [((448, 1024), 0.2, None), ((448, 128), 0.1, 3), ((3, 4099), 0.5, 0), ((1, 13), 0.2, 7)])
def test_gelu_dropout_kernels_against_fp64(shape, p, epoch):
    seed, sid = 4242, 21
    x, dy = rnd(*shape, seed=1, scale=2.0), rnd(*shape, seed=2)
    n = x.numel()
    with pinned_epoch(epoch):
        ms = ms_flat(shape, p, seed, sid, epoch).double()
        xd, dyd = x.to(DEV), dy.to(DEV)
        y, y16 = torch.empty_like(xd), torch.empty(shape, dtype=torch.bfloat16, device=DEV)
        check(lib().medp_gelu_dropout_fwd(ptr(xd), ptr(y), n, p, seed, sid, stream()), "gelu_dropout_fwd")
        check(lib().medp_gelu_dropout_fwd_bf16(ptr(xd), ptr(y16), n, p, seed, sid, stream()), "gelu_dropout_fwd_bf16")
        dx, dx2 = torch.empty_like(xd), torch.empty_like(xd)
        dx16 = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
        check(lib().medp_gelu_dropout_bwd(ptr(dyd), ptr(xd), ptr(dx), n, p, seed, sid, stream()), "gelu_dropout_bwd")
        check(lib().medp_gelu_dropout_bwd_bf16(ptr(dyd), ptr(xd), ptr(dx2), ptr(dx16), n, p, seed, sid, stream()), "gelu_dropout_bwd_bf16")
    assert_close(y, gelu64(x) * ms, 1e-6, 1e-6, "gelu_dropout_fwd")
    assert_close(dx, dy.double() * gelu_grad64(x) * ms, 1e-5, 1e-6, "gelu_dropout_bwd")
    assert torch.equal(y16, y.to(torch.bfloat16)), "bf16 forward is not the bf16 rounding of the fp32 forward"
    assert torch.equal(dx2, dx), "gelu_dropout_bwd_bf16's fp32 gradient differs from gelu_dropout_bwd's"
    assert torch.equal(dx16, dx.to(torch.bfloat16)), "dx16 is not the bf16 rounding of dx"


@pytest.mark.parametrize("epoch", [None, 5])
def test_dropout_add_forward_and_backward_form(epoch):
    shape, p, seed, sid = (448, 256), 0.2, 99, 12
    y, res, dout = rnd(*shape, seed=3), rnd(*shape, seed=4), rnd(*shape, seed=5)
    with pinned_epoch(epoch):
        ms = ms_flat(shape, p, seed, sid, epoch)
        out, g = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
        yd, rd, dd = y.to(DEV), res.to(DEV), dout.to(DEV)
        check(lib().medp_dropout_add(ptr(yd), ptr(rd), ptr(out), y.numel(), p, seed, sid, stream()), "dropout_add")
        check(lib().medp_dropout_add(ptr(dd), None, ptr(g), y.numel(), p, seed, sid, stream()), "dropout_add(bwd)")
    assert_close(out, res.double() + y.double() * ms.double(), 1e-6, 1e-6, "residual + dropout(y)")
    assert torch.equal(g.cpu(), dout * ms), "backward form: dout * mask * scale, one fp32 product"


@pytest.mark.parametrize("epoch", [None, 2])
def test_autograd_nodes_against_fp64(epoch):
    """GeluDropoutFn, DropoutAddFn, DropoutFn: forward and gradients against fp64 autograd with the replica's mask held fixed."""
    shape, p, seed = (7 * 32, 1024), 0.2, 31337
    x, r, dy = rnd(*shape, seed=6, scale=2.0), rnd(*shape, seed=7), rnd(*shape, seed=8)
    with pinned_epoch(epoch):
        m1, m2, m3 = (ms_flat(shape, p, seed, s, epoch).double() for s in (11, 12, 60))
        xd, rdd = x.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
        h = A.GeluDropoutFn.apply(xd, p, seed, 11)
        y = A.DropoutAddFn.apply(h, rdd, p, seed, 12)
        z = A.DropoutFn.apply(y, p, seed, 60)
        z.backward(dy.to(DEV))
    xr, rr = x.double().requires_grad_(True), r.double().requires_grad_(True)
    hr = gelu64(xr) * m1
    yr = rr + hr * m2
    zr = yr * m3
    zr.backward(dy.double())
    assert_close(h, hr, 1e-6, 1e-6, "GeluDropoutFn forward")
    assert_close(y, yr, 1e-6, 1e-6, "DropoutAddFn forward")
    assert_close(z, zr, 1e-6, 1e-6, "DropoutFn forward")
    assert_close(rdd.grad, rr.grad, 1e-6, 1e-7, "d residual")
    assert_close(xd.grad, xr.grad, 1e-5, 1e-6, "d x")


# ------------------------------------------------------------------------------------------------ attention
def ref_attn_drop(q, k, v, ms, H, scale):
    """fp64: P = softmax(q k^T scale), Pd = P * M * s, o = Pd v, head average of Pd.  q [B, Lq, D], k / v [B, Lk, D], ms [B, H, Lq, Lk]."""
    B, Lq, Lk, D = q.shape[0], q.shape[1], k.shape[1], q.shape[2]
    dh = D // H
    sp = lambda t, L: t.reshape(B, L, H, dh).transpose(1, 2)
    P = torch.softmax(sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) * scale, dim=-1)
    Pd = P * ms.double()
    return (Pd @ sp(v, Lk)).transpose(1, 2).reshape(B, Lq, D), Pd.mean(dim=1)


def _attn_case(B, Lq, Lk, H, dh, p, seed, sid, epoch, want_avg):
    D = H * dh
    scale = dh ** -0.5
    q, k, v, do = rnd(B, Lq, D, seed=11), rnd(B, Lk, D, seed=12), rnd(B, Lk, D, seed=13), rnd(B, Lq, D, seed=14)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, avg_ref = ref_attn_drop(qr, kr, vr, ms_attn(B, H, Lq, Lk, p, seed, sid, epoch), H, scale)
    o_ref.backward(do.double())
    return (q, k, v, do), (o_ref, avg_ref, qr.grad, kr.grad, vr.grad), scale


# (B, Lq, Lk, H, dh, want_avg): no averaged weights and Lq <= 8, Lk <= 1024, dh 64 -> thread-per-key kernels; averaged weights (forward)
# or Lq > 8 / dh != 64 -> wave-per-query kernels
SMALL = [(2, 7, 256, 4, 64, False), (2, 8, 1000, 4, 64, False), (1, 1, 64, 4, 64, False), (3, 7, 7, 4, 64, False),
         (2, 7, 256, 4, 64, True), (2, 33, 300, 4, 64, False), (2, 33, 97, 4, 64, True), (3, 49, 49, 2, 12, False)]


@pytest.mark.parametrize("epoch", [None, 5])
@pytest.mark.parametrize("B,Lq,Lk,H,dh,want_avg", SMALL)
def test_attn_small_dropout_against_fp64(B, Lq, Lk, H, dh, want_avg, epoch):
    p, seed, sid = 0.2, 777, 3
    with pinned_epoch(epoch):
        (q, k, v, do), (o_ref, avg_ref, dq_ref, dk_ref, dv_ref), scale = _attn_case(B, Lq, Lk, H, dh, p, seed, sid, epoch, want_avg)
        args = dict(dropout_p=p, seed=seed, stream_id=sid)
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        avg = torch.zeros(B, Lq, Lk, device=DEV) if want_avg else None
        o = Fn.attn_small_fwd(qd, kd, vd, B, Lq, Lk, H, dh, scale, attn_avg=avg, **args)
        dq, dk, dv = Fn.attn_small_bwd(do.to(DEV), qd, kd, vd, B, Lq, Lk, H, dh, scale, **args)
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    if want_avg:
        assert_close(avg, avg_ref, 1e-4, 1e-5, "averaged weights")
    assert_close(dq, dq_ref, 1e-4, 1e-5, "dq")
    assert_close(dk, dk_ref, 1e-4, 1e-5, "dk")
    assert_close(dv, dv_ref, 1e-4, 1e-5, "dv")


@pytest.mark.parametrize("epoch", [None, 5])
@pytest.mark.parametrize("B,Lq,Lk", [(2, 7, 1297), (1, 7, 2304), (1, 14, 2304)])
def test_attn_fq_split_dropout_against_fp64(B, Lq, Lk, epoch):
    p, seed, sid = 0.2, 2 ** 31 - 2, 0
    with pinned_epoch(epoch):
        (q, k, v, do), (o_ref, avg_ref, dq_ref, dk_ref, dv_ref), scale = _attn_case(B, Lq, Lk, 4, 64, p, seed, sid, epoch, True)
        args = dict(dropout_p=p, seed=seed, stream_id=sid)
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        o, lse, avg = Fn.attn_fq_split_fwd(qd, kd, vd, B, Lq, Lk, 4, scale, want_avg=True, **args)
        dq, dk, dv = Fn.attn_fq_split_bwd(do.to(DEV), o, lse, qd, kd, vd, B, Lq, Lk, 4, scale, **args)
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    assert_close(avg, avg_ref, 1e-4, 1e-5, "averaged weights")
    assert_close(dq, dq_ref, 1e-4, 1e-5, "dq")
    assert_close(dk, dk_ref, 1e-4, 1e-5, "dk")
    assert_close(dv, dv_ref, 1e-4, 1e-5, "dv")


@pytest.mark.parametrize("Lk,want_avg,epoch", [(256, False, None), (256, True, 4), (96, False, 4), (1297, True, None), (2304, False, 4)])
def test_attn_small_fn_shared_query_cls_skip_dropout(Lk, want_avg, epoch):
    """The perceiver cross blocks through AttnSmallFn: one [Lq, D] query block for the whole batch (batch stride 0), K | V the column
    halves of a fused [B, Lk + 1, 2D] projection whose CLS row is skipped; dQ summed over the batch, the CLS row's dKV zero."""
    B, Lq, H, dh, p, seed, sid = 3, 7, 4, 64, 0.2, 5150, 0
    D = H * dh
    q, kv, do = rnd(Lq, D, seed=15), rnd(B, Lk + 1, 2 * D, seed=16), rnd(B, Lq, D, seed=17)
    with pinned_epoch(epoch):
        qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
        o_ref, avg_ref = ref_attn_drop(qr.expand(B, -1, -1), kvr[:, 1:, :D], kvr[:, 1:, D:], ms_attn(B, H, Lq, Lk, p, seed, sid, epoch), H,
                                       dh ** -0.5)
        o_ref.backward(do.double())
        qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
        o, avg = A.attn_small(qd, kvd, H, dh ** -0.5, p, seed, sid, 1, want_avg)
        o.backward(do.to(DEV))
    assert_close(o, o_ref, 1e-4, 1e-5, "o")
    if want_avg:
        assert_close(avg, avg_ref, 1e-4, 1e-5, "averaged weights")
    assert_close(qd.grad, qr.grad, 1e-4, 1e-5, "dq")
    assert_close(kvd.grad, kvr.grad, 1e-4, 1e-5, "dkv")
    assert bool((kvd.grad[:, 0] == 0).all())


def _dh16_call(qkv, do, H, p, seed, sid, io16):
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
    return o.float(), dqkv.float()


@pytest.mark.parametrize("io16", [False, True])
@pytest.mark.parametrize("B,N,H,dh,p,epoch", [(7, 49, 2, 12, 0.3, None), (5, 97, 2, 12, 0.1, 6), (2, 130, 1, 16, 0.5, None)])
def test_attn_dh16_train_dropout_against_fp64(B, N, H, dh, p, epoch, io16):
    """DuETT's MFMA attention (bf16 operands): at the tolerances of test_gpu_attention_dh16_train.py, on the bf16-rounded operands."""
    seed, sid = 99, 7
    D = H * dh
    g = torch.Generator().manual_seed(B * N)
    qkv = (torch.randn(B, N, 3 * D, generator=g) * 0.8).bfloat16().float()
    do = torch.randn(B, N, D, generator=g).bfloat16().float()
    with pinned_epoch(epoch):
        o, dqkv = _dh16_call(qkv.to(DEV), do.to(DEV), H, p, seed, sid, io16)
        ms = ms_attn(B, H, N, N, p, seed, sid, epoch)
    x = qkv.double().requires_grad_(True)
    o_ref, _ = ref_attn_drop(x[..., :D], x[..., D:2 * D], x[..., 2 * D:], ms, H, dh ** -0.5)
    o_ref.backward(do.double())
    o_ref, g_ref = o_ref.detach(), x.grad
    assert float((o.cpu().double() - o_ref).abs().max()) <= 1e-2 * float(o_ref.abs().max())
    assert not torch.isnan(dqkv).any()
    for i, name in enumerate(("dq", "dk", "dv")):
        a, b = dqkv[..., i * D:(i + 1) * D].cpu().double(), g_ref[..., i * D:(i + 1) * D]
        err = float((a - b).abs().max())
        assert err <= 2e-2 * float(b.abs().max()), (name, err)
        cos = float(torch.dot(a.flatten(), b.flatten()) / (a.norm() * b.norm()))
        assert cos > 0.9995, (name, cos)


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_draws_the_mask_of_each_epoch():
    """The step's order (graph_step._advance): advance the epoch counter, then the dropout kernels, captured on one stream.  Replay k
    must draw the replica's mask at epoch k, forward and backward, and no two replays may share a mask."""
    shape, p, seed, sid = (64, 512), 0.2, 123456, 41
    x, dy = rnd(*shape, seed=18, scale=2.0), rnd(*shape, seed=19)
    with pinned_epoch(0) as ep:
        xd = x.to(DEV).requires_grad_(True)
        dyd = dy.to(DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                   # warm-up outside the graph (autograd's first-call setup)
            torch.autograd.grad(A.GeluDropoutFn.apply(xd, p, seed, sid), xd, dyd)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            check(lib().medp_counter_advance(ptr(ep), stream()), "counter_advance")
            y = A.GeluDropoutFn.apply(xd, p, seed, sid)
            (dx,) = torch.autograd.grad(y, xd, dyd)
        torch.cuda.synchronize()
        assert int(ep.item()) == 0, "capture ran the counter kernel"
        masks = []
        for k in (1, 2, 3):
            g.replay()
            torch.cuda.synchronize()
            assert int(ep.item()) == k
            ms = ms_flat(shape, p, seed, sid, k).double()
            assert_close(y, gelu64(x) * ms, 1e-6, 1e-6, f"replay {k} forward")
            assert_close(dx, dy.double() * gelu_grad64(x) * ms, 1e-5, 1e-6, f"replay {k} backward")
            masks.append(ms != 0)
        del g
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(masks[a], masks[b]), f"replays {a + 1} and {b + 1} drew the same mask"
