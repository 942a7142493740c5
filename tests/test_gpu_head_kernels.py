"""The pathology-head and pooling kernels of csrc/fusion_ops.hip on their own — `medp_rowdot_*`, `medp_fusion_logits_*`,
`medp_meanpool_*` — through RowDotFn / FusionLogitsFn / MeanPoolFn (through the C ABI where a wrapper cannot state the case: a
leading dimension, an absent incoming gradient) against the same operation in float64 with float64 autograd, at shapes where the
row-lane, column-block and grid-stride loops take a second trip.  Bounds: tests/test_gpu_gmlp.py's (fp32, short summation chains)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL, GRAD_TOL = 2e-5, 2e-4


def _close(a, b, tol, what, floor=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"{what}: max err {err:.3e} of max|ref| {scale:.3e}")
    if floor is not None:
        assert scale > floor, (what, "the reference gradient is trivially small", scale)
    assert a.shape == b.shape and bool(torch.isfinite(a).all()) and err <= tol * max(scale, 1e-6), (what, err, scale)


# ------------------------------------------------------------------------------------------------ RowDotFn
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,D,ldx", [(1, 64, 64), (5, 64, 64), (17, 64, 80), (448, 64, 64), (33, 100, 100), (1100, 130, 130)])
def test_rowdot(rows, D, ldx, bias):
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    from multimodal_edema_prediction_amd.autograd_ops import RowDotFn
    g = torch.Generator().manual_seed(rows * 7 + D)
    xp = torch.full((rows, ldx), 1e30)                              # the padding columns of a strided operand must never be read
    xp[:, :D] = torch.randn(rows, D, generator=g)
    w, b, dy = torch.randn(1, D, generator=g) / D ** 0.5, torch.randn(1, generator=g), torch.randn(rows, generator=g)
    xr, wr = xp[:, :D].double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    yr = (xr * wr).sum(1) + (br if bias else 0.0)
    yr.backward(dy.double())
    if ldx == D:
        xd, wd = xp.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        bd = b.to(DEV).requires_grad_(True) if bias else None
        y = RowDotFn.apply(xd, wd, bd)
        y.backward(dy.to(DEV))
        dx, dw, db = xd.grad, wd.grad, bd.grad if bias else None
    else:                                                           # the wrapper makes its operand contiguous: ldx > D through the C ABI
        xd, wd, bd, dyd = xp.to(DEV), w.to(DEV), b.to(DEV) if bias else None, dy.to(DEV)
        y, dx, dw = torch.empty(rows, device=DEV), torch.full((rows, D), float("nan"), device=DEV), torch.empty(1, D, device=DEV)
        db = torch.empty(1, device=DEV) if bias else None
        check(lib().medp_rowdot_fwd(ptr(xd), ldx, ptr(wd), ptr(bd), ptr(y), rows, D, stream()), "rowdot_fwd")
        check(lib().medp_rowdot_bwd(ptr(dyd), ptr(xd), ldx, ptr(wd), ptr(dx), ptr(dw), ptr(db), rows, D, stream()), "rowdot_bwd")
        torch.cuda.synchronize()
    _close(y, yr, FWD_TOL, "y")
    _close(dx, xr.grad, GRAD_TOL, "dx", floor=1e-4)
    _close(dw, wr.grad, GRAD_TOL, "dw", floor=1e-4)
    if bias:
        _close(db, br.grad, GRAD_TOL, "db", floor=1e-4)


# ------------------------------------------------------------------------------------------------ FusionLogitsFn
def _fusion_inputs(B, K):
    g = torch.Generator().manual_seed(B * 10 + K)
    r = lambda *s: torch.randn(*s, generator=g)
    return [r(B, K), r(B, K), r(B, K), 0.3 * r(K), 0.3 * r(K), 1 + 0.3 * r(K)], [r(B, K) for _ in range(4)]


def _fusion_ref(inputs, douts):
    """float64 autograd; douts: the four incoming gradients (img, ts, scaled, fus), None = that output takes no part"""
    hi, ht, hc, ib, tb, beta = leaves = [t.double().requires_grad_(True) for t in inputs]
    img, ts = hi + ib, ht + tb
    scaled = beta * hc
    fus = img.detach() + scaled
    outs = (img, ts, scaled, fus)
    loss = sum((o * d.double()).sum() for o, d in zip(outs, douts) if d is not None)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [o.detach() for o in outs], [torch.zeros_like(l) if gr is None else gr for l, gr in zip(leaves, grads)]


GRAD_NAMES = ("d_hi", "d_ht", "d_hc", "d_img_bias", "d_ts_bias", "d_beta")


@pytest.mark.parametrize("B,K", [(1, 1), (4, 7), (300, 7), (37, 64), (1000, 3)])
def test_fusion_logits(B, K):
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    from multimodal_edema_prediction_amd.autograd_ops import FusionLogitsFn
    inputs, douts = _fusion_inputs(B, K)
    outs_ref, grads_ref = _fusion_ref(inputs, douts)
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    outs = FusionLogitsFn.apply(*leaves)
    for name, o, r in zip(("img", "ts", "scaled", "fus"), outs, outs_ref):
        _close(o, r, FWD_TOL, name)
    torch.autograd.backward(outs, [d.to(DEV) for d in douts])
    for name, l, r in zip(GRAD_NAMES, leaves, grads_ref):
        _close(l.grad, r, GRAD_TOL, name, floor=1e-4)
    # each incoming gradient absent in turn, and fus alone (autograd hands the wrapper zeros, never a null pointer: the C ABI)
    dd = [d.to(DEV) for d in douts]
    hc, beta = leaves[2].detach(), leaves[5].detach()
    for present in ([False, True, True, True], [True, False, True, True], [True, True, False, True], [True, True, True, False],
                    [False, False, False, True]):
        got = [torch.full((B, K), float("nan"), device=DEV) for _ in range(3)] + [torch.full((K,), float("nan"), device=DEV) for _ in range(3)]
        check(lib().medp_fusion_logits_bwd(*(ptr(d) if p else None for d, p in zip(dd, present)), ptr(hc), ptr(beta), *(ptr(t) for t in got), B, K,
                                           stream()), "fusion_logits_bwd")
        torch.cuda.synchronize()
        _, ref = _fusion_ref(inputs, [d if p else None for d, p in zip(douts, present)])
        for name, a, r in zip(GRAD_NAMES, got, ref):
            _close(a, r, GRAD_TOL, f"{name} with {present}")
        if not present[0]:                                          # img receives nothing through fus (fus = img.detach() + scaled)
            assert bool((got[0] == 0).all()) and bool((got[3] == 0).all())
        if not present[1]:
            assert bool((got[1] == 0).all()) and bool((got[4] == 0).all())


def test_fusion_logits_backward_refuses_more_than_64_labels():
    from multimodal_edema_prediction_amd.abi import lib, ptr, stream
    from multimodal_edema_prediction_amd.autograd_ops import FusionLogitsFn
    B, K = 3, 65
    inputs, douts = _fusion_inputs(B, K)
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    outs = FusionLogitsFn.apply(*leaves)                            # the forward has no such limit
    outs_ref, _ = _fusion_ref(inputs, douts)
    _close(outs[3], outs_ref[3], FWD_TOL, "fus")
    with pytest.raises(ValueError):
        torch.autograd.backward(outs, [d.to(DEV) for d in douts])
    dd = [d.to(DEV) for d in douts]
    got = [torch.full((B, K), 7.0, device=DEV) for _ in range(3)] + [torch.full((K,), 7.0, device=DEV) for _ in range(3)]
    rc = lib().medp_fusion_logits_bwd(*(ptr(d) for d in dd), ptr(leaves[2].detach()), ptr(leaves[5].detach()), *(ptr(t) for t in got), B, K, stream())
    torch.cuda.synchronize()
    assert rc < 0 and all(bool((t == 7.0).all()) for t in got)      # refused before any launch: no partial sums written


# ------------------------------------------------------------------------------------------------ MeanPoolFn
@pytest.mark.parametrize("B,T,T1,D", [(1, 1, 1, 4), (3, 5, 6, 24), (2, 33, 34, 100), (70, 7, 9, 130), (2, 3, 4, 270000)])
def test_meanpool(B, T, T1, D):
    from multimodal_edema_prediction_amd.autograd_ops import MeanPoolFn
    g = torch.Generator().manual_seed(B + T * 3 + D)
    x = torch.randn(B, T1, D, generator=g)
    x[:, T:] = 1e30                                                 # tokens past T (the REP row) take no part
    dy = torch.randn(B, D, generator=g)
    xr = x.double().requires_grad_(True)
    yr = xr[:, :T].mean(1)
    yr.backward(dy.double())
    xd = x.to(DEV).requires_grad_(True)
    y = MeanPoolFn.apply(xd, T)
    y.backward(dy.to(DEV))
    _close(y, yr, FWD_TOL, "y")
    _close(xd.grad, xr.grad, GRAD_TOL, "dx", floor=1e-4)
    assert bool((xd.grad[:, T:] == 0).all()) and bool((xr.grad[:, T:] == 0).all())
