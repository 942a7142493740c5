"""Device-side global-norm clip of `FusedAdamW(max_grad_norm=...)` (medp_grad_sumsq_multi + medp_adamw_multi_dscale) against
`torch.nn.utils.clip_grad_norm_` + `torch.optim.AdamW`: the norm (fp64 reference, 1e-6 relative, bitwise reproducible), three clipped
steps (the tolerance of test_gpu_model.test_fused_adamw_matches_torch_adamw: 2e-6 abs), a clip that never engages (bit-identical to
no clip), zero gradients, and the clip inside a captured graph.  Sizes: 1, 7 (not a multiple of 4: the scalar path), 4096 (exactly
one chunk), 4097 (one element into a second chunk, odd), 100 003 (25 chunks, odd) and a 2-D tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1,), (7,), (4096,), (4097,), (100003,), (300, 257), (64, 64)]
TOL = 2e-6          # tests/test_gpu_model.py::test_fused_adamw_matches_torch_adamw


def tensors(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    gs = [[torch.randn(s, generator=g) * scale for s in SHAPES] for _ in range(3)]
    return ps, gs


def fused(ps, **kw):
    from multimodal_edema_prediction_amd.optim import FusedAdamW
    b = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    return b, FusedAdamW([{"params": b[:2], "lr": 1e-3}, {"params": b[2:], "lr": 3e-4}], weight_decay=5e-2, **kw)


def run_fused(ps, gs, **kw):
    b, ob = fused(ps, **kw)
    norms = []
    for step in range(len(gs)):
        for y, g in zip(b, gs[step]):
            y.grad = g.clone().to(DEV)
        ob.step()
        if ob.last_grad_norm is not None:
            norms.append(ob.last_grad_norm.clone())
    torch.cuda.synchronize()
    return b, ob, norms


def test_norm_matches_fp64_and_is_reproducible():
    ps, gs = tensors()
    _, ob, n1 = run_fused(ps, gs, max_grad_norm=0.5)
    _, _, n2 = run_fused(ps, gs, max_grad_norm=0.5)
    assert ob.last_grad_norm.is_cuda and ob.last_grad_norm.shape == (1,)
    for step in range(3):
        ref = torch.sqrt(sum((g.double() ** 2).sum() for g in gs[step])).item()
        got = float(n1[step])
        print("norm", step, got, ref, abs(got - ref) / ref)
        assert abs(got - ref) <= 1e-6 * ref
        assert torch.equal(n1[step], n2[step])


def test_three_clipped_steps_match_clip_grad_norm_and_torch_adamw():
    ps, gs = tensors()
    a = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    oa = torch.optim.AdamW([{"params": a[:2], "lr": 1e-3}, {"params": a[2:], "lr": 3e-4}], weight_decay=5e-2)
    for step in range(3):
        for x, g in zip(a, gs[step]):
            x.grad = g.clone().to(DEV)
        torch.nn.utils.clip_grad_norm_(a, 0.5)
        oa.step()
    b, ob, _ = run_fused(ps, gs, max_grad_norm=0.5)
    for x, y, g in zip(a, b, gs[2]):
        assert float((x - y).detach().abs().max()) < TOL
        assert torch.equal(y.grad.cpu(), g), "the gradients themselves are not rewritten"


def test_a_clip_that_never_engages_is_bit_identical_to_no_clip():
    ps, gs = tensors()
    a, oa, _ = run_fused(ps, gs)
    b, ob, _ = run_fused(ps, gs, max_grad_norm=1e9)
    assert oa.last_grad_norm is None
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k])


def test_zero_gradients_give_scale_one_and_no_nan():
    ps, gs = tensors(scale=0.0)
    b, ob, norms = run_fused(ps, gs, max_grad_norm=1.0)
    assert float(norms[-1]) == 0.0 and float(ob._clip[1]) == 1.0
    a, _, _ = run_fused(ps, gs)                              # weight decay only, same as without the clip
    for x, y in zip(a, b):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)


def test_clip_inside_a_captured_graph_replays_with_new_gradients():
    ps, gs = tensors()
    ref, _, ref_norms = run_fused(ps, gs, max_grad_norm=0.5)
    b, ob = fused(ps, max_grad_norm=0.5)
    static = [torch.zeros_like(p) for p in b]
    for y, s in zip(b, static):
        y.grad = s
    snap = [p.detach().clone() for p in b]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ob.step()                                            # warm-up: builds the table, the partials and the clip buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.no_grad():                                    # undo the warm-up step
        for p, v in zip(b, snap):
            p.copy_(v)
            ob.state[p]["exp_avg"].zero_()
            ob.state[p]["exp_avg_sq"].zero_()
        ob.dev_step.zero_()
        ob._step = 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ob.step()
    for step in range(3):
        for sbuf, gr in zip(static, gs[step]):
            sbuf.copy_(gr)
        ob.refresh_lrs()
        g.replay()
        assert torch.equal(ob.last_grad_norm, ref_norms[step])
    torch.cuda.synchronize()
    for x, y in zip(ref, b):
        assert torch.equal(x, y)
