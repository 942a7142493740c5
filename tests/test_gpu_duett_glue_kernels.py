"""The DuETT training glue of csrc/duett_train.hip one kernel family at a time — grouped Linear, grouped BatchNorm, activations,
embedding inputs, psi assembly, the axis swaps and broadcast adds — through the autograd Functions of duett_train.py (through the C ABI
where a Function cannot state the case: no bias) against the same operation in float64 with float64 autograd, at the smallest shapes
where every loop (256 threads over elements, 4 row-lanes, row chunks, 64-column blocks, cell slices, grid strides) takes a second trip.
Bounds: tests/test_gpu_gmlp.py's (fp32, short summation chains); copies and single adds are compared for equality."""
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL, GRAD_TOL = 2e-5, 2e-4
BN_EPS, BN_MOM = 1e-5, 0.1


def _close(a, b, tol, what, floor=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"{what}: max err {err:.3e} of max|ref| {scale:.3e}")
    if floor is not None:
        assert scale > floor, (what, "the reference gradient is trivially small", scale)
    assert a.shape == b.shape and bool(torch.isfinite(a).all()) and err <= tol * max(scale, 1e-6), (what, err, scale)


# ------------------------------------------------------------------------------------------------ GLinearFn
GLINEAR_SHAPES = [(1, 1, 1, 1), (3, 7, 2, 64), (2, 300, 64, 24), (7, 5, 64, 1), (7, 64, 256, 64), (2, 700, 8, 128), (1, 6200, 2, 64),
                  (2, 1100, 256, 64), (1, 9, 139, 255),
                  (7, 128, 256, 64), (7, 191, 256, 64), (7, 287, 256, 64), (7, 383, 256, 64)]    # the grouped heads at batch sizes once refused


def _glinear_run(x, W, b, dy):
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    from multimodal_edema_prediction_amd.duett_train import GLinearFn
    if b is not None:
        xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, W, b))
        y = GLinearFn.apply(xd, Wd, bd)
        y.backward(dy.to(DEV))
        return y.detach(), xd.grad, Wd.grad, bd.grad
    (G, R, K), N = x.shape, W.shape[1]                              # no bias: the Function always has one
    xd, Wd, dyd = x.to(DEV), W.to(DEV), dy.to(DEV)
    y, dx, dW = torch.empty((G, R, N), device=DEV), torch.empty_like(xd), torch.empty_like(Wd)
    db = torch.empty((G, N), device=DEV)
    ws = torch.empty(lib().medp_glinear_bwd_workspace_bytes(G, R, K, N) // 4, device=DEV)
    check(lib().medp_glinear_fwd(ptr(xd), ptr(Wd), None, ptr(y), G, R, K, N, stream()), "glinear_fwd")
    check(lib().medp_glinear_bwd(ptr(dyd), ptr(xd), ptr(Wd), ptr(dx), ptr(dW), ptr(db), ptr(ws), G, R, K, N, stream()), "glinear_bwd")
    torch.cuda.synchronize()
    return y, dx, dW, db


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("G,R,K,N", GLINEAR_SHAPES)
def test_glinear(G, R, K, N, bias):
    g = torch.Generator().manual_seed(G * 1000 + R + K + N)
    x, W = torch.randn(G, R, K, generator=g), torch.randn(G, N, K, generator=g) / K ** 0.5
    b, dy = (0.3 * torch.randn(G, N, generator=g) if bias else None), torch.randn(G, R, N, generator=g)
    xr, Wr = x.double().requires_grad_(True), W.double().requires_grad_(True)
    br = torch.zeros(G, N, dtype=torch.float64, requires_grad=True) if b is None else b.double().requires_grad_(True)
    yr = torch.einsum("grk,gnk->grn", xr, Wr) + br[:, None]
    yr.backward(dy.double())
    got = _glinear_run(x, W, b, dy)
    _close(got[0], yr, FWD_TOL, "y")
    for name, a, r in zip(("dx", "dW", "db"), got[1:], (xr.grad, Wr.grad, br.grad)):
        _close(a, r, GRAD_TOL, name, floor=1e-4)
    again = _glinear_run(x, W, b, dy)                               # ordered partial sums: the same bits
    assert all(torch.equal(a, c) for a, c in zip(got, again))


def test_glinear_refuses_weights_that_do_not_fit_lds():
    from multimodal_edema_prediction_amd.duett_train import GLinearFn
    with pytest.raises(ValueError):
        GLinearFn.apply(torch.zeros(1, 9, 139, device=DEV), torch.zeros(1, 256, 139, device=DEV), torch.zeros(1, 256, device=DEV))


# ------------------------------------------------------------------------------------------------ GBatchNormFn
def _gbn_case(G, R, C, batch_stats, x):
    from multimodal_edema_prediction_amd.duett_train import GBatchNormFn
    g = torch.Generator().manual_seed(G * 100 + R + C)
    r = lambda *s: torch.randn(*s, generator=g)
    w, b, rm, rv, dy = 1 + 0.2 * r(G, C), 0.2 * r(G, C), 0.1 * r(G, C), 0.5 + torch.rand(G, C, generator=g), r(G, R, C)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    if batch_stats:
        mu, var = xr.mean(1), xr.var(1, unbiased=False)
        rm_ref = (1 - BN_MOM) * rm.double() + BN_MOM * mu.detach()
        rv_ref = (1 - BN_MOM) * rv.double() + BN_MOM * var.detach() * R / max(R - 1, 1)          # the running variance is unbiased
    else:
        mu, var, rm_ref, rv_ref = rm.double(), rv.double(), rm.double(), rv.double()
    yr = (xr - mu[:, None]) / torch.sqrt(var[:, None] + BN_EPS) * wr[:, None] + br[:, None]
    yr.backward(dy.double())
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    y = GBatchNormFn.apply(xd, wd, bd, rmd, rvd, batch_stats)
    _, _, sm, sv = y.grad_fn.saved_tensors
    y.backward(dy.to(DEV))
    tag = f"[{G},{R},{C}] batch_stats={batch_stats} "
    _close(y, yr, FWD_TOL, tag + "y")
    _close(sm, mu, FWD_TOL, tag + "saved mean")
    _close(sv, var, FWD_TOL, tag + "saved var")
    _close(rmd, rm_ref, FWD_TOL, tag + "running mean")
    _close(rvd, rv_ref, FWD_TOL, tag + "running var")
    if not batch_stats:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    for name, a, ref in (("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad), ("db", bd.grad, br.grad)):
        _close(a, ref, GRAD_TOL, tag + name, floor=1e-4)


@pytest.mark.parametrize("batch_stats", [True, False])
@pytest.mark.parametrize("G,R,C", [(1, 2, 1), (3, 7, 64), (2, 128, 64), (2, 129, 64), (5, 300, 24), (1, 2, 200), (2, 1000, 130)])
def test_gbatchnorm(G, R, C, batch_stats):
    g = torch.Generator().manual_seed(R * 10 + C)
    # Two rows: x_hat = +-d / sqrt(d^2 + eps) and the true dx is dy scaled by eps / (d^2 + eps).  Unit-variance inputs would make that
    # ~1e-5 of dy (a vacuous check, lost in fp32 cancellation); a spread of sqrt(eps) keeps it of order one and puts eps on the scale.
    x = torch.randn(G, R, C, generator=g) * (3e-3 if R == 2 else 1.0)
    _gbn_case(G, R, C, batch_stats, x)


@pytest.mark.parametrize("batch_stats", [True, False])
def test_gbatchnorm_activations_far_from_zero(batch_stats):
    """mean >> spread: the case the pivot of the statistics kernel exists for (E[x^2] - E[x]^2 would lose every digit)"""
    g = torch.Generator().manual_seed(31)
    _gbn_case(2, 129, 64, batch_stats, 30 + 0.5 * torch.randn(2, 129, 64, generator=g))


# ------------------------------------------------------------------------------------------------ ActFn
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 1_100_000])
def test_act(n, mode):
    from multimodal_edema_prediction_amd.duett_train import ActFn
    g = torch.Generator().manual_seed(n + mode)
    x, dy = 2 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n > 1:
        x[0], x[n // 2] = 0.0, -0.0
    else:
        x[0] = 0.7
    xr = x.double().requires_grad_(True)
    yr = torch.relu(xr) if mode == 0 else torch.tanh(xr)
    yr.backward(dy.double())
    xd = x.to(DEV).requires_grad_(True)
    y = ActFn.apply(xd, mode)
    y.backward(dy.to(DEV))
    _close(y, yr, FWD_TOL, "y")
    _close(xd.grad, xr.grad, GRAD_TOL, "dx", floor=1e-4)
    if mode == 0:
        assert torch.equal(y.detach().cpu(), torch.relu(x))
        if n > 1:                                                   # the ReLU gradient at +-0 is 0
            assert float(xd.grad[0]) == 0.0 and float(xd.grad[n // 2]) == 0.0 and float(xr.grad[0]) == 0.0


# ------------------------------------------------------------------------------------------------ EmbedInputsFn
@pytest.mark.parametrize("B,T,V", [(1, 1, 1), (2, 5, 3), (4, 32, 16), (3, 33, 70), (4, 64, 300)])
def test_embed_inputs(B, T, V):
    from multimodal_edema_prediction_amd.duett_train import EmbedInputsFn
    g = torch.Generator().manual_seed(B * 100 + T + V)
    xs = KR.ssl_like_inputs(B, T, V, g)                                # counts: -1, -0.5, 2.7, 15.9, above 15, 1e6
    table = torch.randn(16, 1, generator=g)
    dxin = torch.randn(V, B * T, 2, generator=g)
    xin_ref = KR.embed_inputs(xs, table)                            # == duett_ref.build_psi's pairing (test_kernel_refs_cpu.py)
    idx = KR.embed_indices(xs, 16)
    dtab_ref = torch.zeros(16, dtype=torch.float64).index_add_(0, idx.reshape(-1), dxin[..., 1].double().reshape(-1)).view(16, 1)

    def run():
        td = table.to(DEV).requires_grad_(True)
        xin = EmbedInputsFn.apply(xs.to(DEV), td)
        xin.backward(dxin.to(DEV))
        return xin.detach(), td.grad
    xin, dtab = run()
    assert torch.equal(xin.cpu(), xin_ref)                          # copies and a table look-up: exact
    _close(dtab, dtab_ref, GRAD_TOL, "d_table", floor=1e-4)
    xin2, dtab2 = run()
    assert torch.equal(xin, xin2) and torch.equal(dtab, dtab2)


# ------------------------------------------------------------------------------------------------ PsiAssembleFn
@pytest.mark.parametrize("B,T,V,E", [(1, 1, 1, 4), (2, 5, 3, 24), (4, 32, 16, 24), (3, 7, 5, 64), (2, 9, 4, 84), (40, 6, 3, 24), (600, 2, 2, 8)])
def test_psi_assemble(B, T, V, E):
    from multimodal_edema_prediction_amd import duett_train as DT
    g = torch.Generator().manual_seed(B * 100 + T * 10 + V + E)
    xs = KR.ssl_like_inputs(B, T, V, g)            # masked timesteps, masked events, both in one cell, the static column under a masked timestep
    r = lambda *s: torch.randn(*s, generator=g)
    var_out, tab_out, special, dpsi = r(V, B * T, E), r(B, E), r(2, E), r(B, T + 1, V + 1, E)
    leaves = [t.double().requires_grad_(True) for t in (var_out, tab_out, special)]
    psi_ref = KR.psi_assemble(xs.double(), *leaves)
    psi_ref.backward(dpsi.double())
    dl = [t.to(DEV).requires_grad_(True) for t in (var_out, tab_out, special)]
    psi = DT.PsiAssembleFn.apply(xs.to(DEV), *dl)
    psi.backward(dpsi.to(DEV))
    assert torch.equal(psi.detach().cpu().double(), psi_ref.detach())                      # cell by cell: copies
    d_var, d_tab, d_special = (t.grad for t in dl)
    assert bool(torch.isfinite(d_var).all())
    overridden = leaves[0].grad == 0
    assert bool(overridden.view(V, B, T, E).all(-1).any()) and bool((d_var.cpu()[overridden] == 0).all())       # exact zeros under an override
    kept = ~overridden
    assert torch.equal(d_var.cpu()[kept].double(), leaves[0].grad[kept])
    _close(d_tab, leaves[1].grad, GRAD_TOL, "d_tab", floor=1e-4 if B * T > 1 else None)
    _close(d_special[0], leaves[2].grad[0], GRAD_TOL, "d_special[MASKED]", floor=1e-4)
    _close(d_special[1], leaves[2].grad[1], GRAD_TOL, "d_special[REP]", floor=1e-4)
    # every cell of d_var is written, the overridden ones with zeros: the same call on a buffer full of NaN
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    S = lib().medp_psi_assemble_bwd_slices(B, T, V)
    xd, dd = xs.to(DEV), dpsi.to(DEV)
    nan_var = torch.full((V, B * T, E), float("nan"), device=DEV)
    tab_part, part = torch.empty((B, S, E), device=DEV), torch.empty((B * S, 2 * E), device=DEV)
    check(lib().medp_psi_assemble_bwd(ptr(xd), ptr(dd), ptr(nan_var), ptr(tab_part), ptr(part), B, T, V, E, stream()), "psi_assemble_bwd")
    torch.cuda.synchronize()
    assert torch.equal(nan_var, d_var)


def test_psi_assemble_backward_refuses_wide_embeddings():
    from multimodal_edema_prediction_amd.duett_train import PsiAssembleFn
    B, T, V, E = 2, 3, 2, 88                                        # 3 * E > 256: the backward's three sums per thread block do not fit
    xs = torch.zeros(B, T, 2 * V + 1, device=DEV)
    leaves = [torch.randn(*s, device=DEV).requires_grad_(True) for s in ((V, B * T, E), (B, E), (2, E))]
    psi = PsiAssembleFn.apply(xs, *leaves)
    assert torch.equal(psi[:, :T, :V], leaves[0].detach().view(V, B, T, E).permute(1, 2, 0, 3))
    with pytest.raises(ValueError):
        psi.sum().backward()


# ------------------------------------------------------------------------------------------------ AxisSwapFn, SwapAddFn, AddBcastFn
SWAP_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 24), (3, 33, 17, 24), (2, 17, 33, 64)]


def _fwd_bwd(fn, tensors, ref_fn, dout):
    """-> the Function's result and gradients, the float64 result and gradients, and the fp32 torch expression on the CPU"""
    dl = [t.to(DEV).requires_grad_(True) for t in tensors]
    y = fn(*dl)
    y.backward(dout.to(DEV))
    rl = [t.double().requires_grad_(True) for t in tensors]
    yr = ref_fn(*rl)
    yr.backward(dout.double())
    return y.detach().cpu(), [t.grad for t in dl], [t.grad for t in rl], ref_fn(*tensors)


@pytest.mark.parametrize("B,A1,A2,E", SWAP_SHAPES)
def test_axis_swap(B, A1, A2, E):
    from multimodal_edema_prediction_amd.duett_train import AxisSwapFn
    g = torch.Generator().manual_seed(A1 * 10 + A2)
    x, dout = torch.randn(B, A1, A2, E, generator=g), torch.randn(B, A2, A1, E, generator=g)
    y, grads, grads_ref, y32 = _fwd_bwd(AxisSwapFn.apply, [x], lambda t: t.transpose(1, 2).contiguous(), dout)
    assert torch.equal(y, y32)
    _close(grads[0], grads_ref[0], GRAD_TOL, "dx", floor=1e-4)
    assert torch.equal(grads[0].cpu(), dout.transpose(1, 2).contiguous())


@pytest.mark.parametrize("B,A1,A2,E", SWAP_SHAPES)
def test_swap_add_shared_table(B, A1, A2, E):
    """mode 1: out[b][a2][a1] = in[b][a1][a2] + add[a2][a1] (full_event_embedding)"""
    from multimodal_edema_prediction_amd.duett_train import SwapAddFn
    g = torch.Generator().manual_seed(A1 * 10 + A2 + 1)
    x, add = torch.randn(B, A1, A2, E, generator=g), torch.randn(A2, A1 * E, generator=g)
    dout = torch.randn(B, A2, A1 * E, generator=g)
    ref = lambda t, a: t.transpose(1, 2).reshape(B, A2, A1 * E) + a
    y, grads, grads_ref, y32 = _fwd_bwd(lambda t, a: SwapAddFn.apply(t, a, None), [x, add], ref, dout)
    assert torch.equal(y, y32)                                      # one fp32 add
    _close(grads[0], grads_ref[0], GRAD_TOL, "dx", floor=1e-4)
    _close(grads[1], grads_ref[1], GRAD_TOL, "d_add", floor=1e-4)


@pytest.mark.parametrize("B,A1,A2,E", SWAP_SHAPES[1:] + [(3, 5, 2, 24)])
def test_swap_add_per_sample_rows_and_last_row(B, A1, A2, E):
    """mode 3: the first A2 - 1 rows come from add[b], the last one from add_last (time embedding rows and the REP row)"""
    from multimodal_edema_prediction_amd.duett_train import SwapAddFn
    g = torch.Generator().manual_seed(A1 * 10 + A2 + 2)
    x, add, last = torch.randn(B, A1, A2, E, generator=g), torch.randn(B, A2 - 1, A1 * E, generator=g), torch.randn(A1 * E, generator=g)
    dout = torch.randn(B, A2, A1 * E, generator=g)
    ref = lambda t, a, l: t.transpose(1, 2).reshape(B, A2, A1 * E) + torch.cat((a, l.view(1, 1, -1).expand(B, -1, -1)), 1)
    y, grads, grads_ref, y32 = _fwd_bwd(SwapAddFn.apply, [x, add, last], ref, dout)
    assert torch.equal(y, y32)
    for name, a, r in zip(("dx", "d_add", "d_add_last"), grads, grads_ref):
        _close(a, r, GRAD_TOL, name, floor=1e-4)


@pytest.mark.parametrize("broadcast", [True, False])
@pytest.mark.parametrize("B,A1,A2,E", SWAP_SHAPES)
def test_add_bcast(B, A1, A2, E, broadcast):
    from multimodal_edema_prediction_amd.duett_train import AddBcastFn
    g = torch.Generator().manual_seed(A1 * 10 + A2 + 3)
    a, dout = torch.randn(B, A2, A1 * E, generator=g), torch.randn(B, A2, A1 * E, generator=g)
    b = torch.randn(A2, A1 * E, generator=g) if broadcast else torch.randn(B, A2, A1 * E, generator=g)
    y, grads, grads_ref, y32 = _fwd_bwd(AddBcastFn.apply, [a, b], lambda p, q: p + q, dout)
    assert torch.equal(y, y32)
    _close(grads[0], grads_ref[0], GRAD_TOL, "da", floor=1e-4)
    _close(grads[1], grads_ref[1], GRAD_TOL, "db", floor=1e-4)
