"""The stacked trajectory encoder (n_layers > 1) on the HIP kernels: the bf16 hand-over the recurrence kernel writes for the next
layer (medp_gru_fwd_h16, dropout mask drawn in the kernel), an upper layer against the fp32 recurrence, the stack's autograd node, the module against the fixtures the reference's own class produced (tests/golden/trajectory_layers*.npz), and the probe
on top of it, eager and captured.
Bounds are the one-layer tests' (tests/test_gpu_trajectory.py): recurrence forward 2e-2 abs; tokens 3e-2 abs; parameter gradients
cosine >= 0.995 and max error <= 5 % of the reference's max; fp32 kernel mode 1e-4 abs.  Shapes: S = 37 (ragged against the 16
sequences of a workgroup) and 16; T = 1 (only the zeroed LDS tile is read), 2 (both LDS buffers), 24."""
import os

import numpy as np
import pytest
import torch

import dropout_twin as twin

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = 128
F32, BF16 = torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ helpers
def cpu_gru_layer(gi, w_hh, b_hh):
    """fp32 torch recurrence, written out step by step; gi [S,T,3d] given -> hseq, gates (r|z|n), hn."""
    S, T, _ = gi.shape
    d = w_hh.shape[1]
    h = torch.zeros(S, d)
    hs, gates, hns = [], [], []
    for t in range(T):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, t, :d] + gh[:, :d])
        z = torch.sigmoid(gi[:, t, d:2 * d] + gh[:, d:2 * d])
        n = torch.tanh(gi[:, t, 2 * d:] + r * gh[:, 2 * d:])
        h = (1 - z) * n + z * h
        hs.append(h); gates.append(torch.cat([r, z, n], 1)); hns.append(gh[:, 2 * d:])
    return torch.stack(hs, 1), torch.stack(gates, 1), torch.stack(hns, 1)


def layer_params(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [dict(w_ih=torch.randn(3 * D, D, generator=g) * 0.08, w_hh=torch.randn(3 * D, D, generator=g) * 0.08,
                 b_ih=torch.randn(3 * D, generator=g) * 0.1, b_hh=torch.randn(3 * D, generator=g) * 0.1) for _ in range(n)]


def gpu_composition(x16, q, S, T, p=0.0, seed=0, sid=0, want16=False):
    """An upper layer as the stack runs it: A.linear's GEMM (bf16 operands, fp32 result) into the recurrence kernel."""
    from multimodal_edema_prediction_amd import functional as Fn
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    gi = Fn.gemm(x16.view(S * T, D), q["w_ih"].cuda().to(BF16).contiguous(), bias=q["b_ih"].cuda()).view(S, T, 3 * D)
    hseq, gates, hn = (torch.empty((S, T, n), device="cuda") for n in (D, 3 * D, D))
    whh, bhh = q["w_hh"].cuda().to(BF16).contiguous(), q["b_hh"].cuda()
    h16 = torch.empty((S, T, D), device="cuda", dtype=BF16) if want16 else None
    if want16:
        check(lib().medp_gru_fwd_h16(ptr(gi), ptr(whh), ptr(bhh), ptr(hseq), ptr(gates), ptr(hn), ptr(h16), p, seed, sid, S, T, D, stream()),
              "gru_fwd_h16")
    else:
        check(lib().medp_gru_fwd(ptr(gi), ptr(whh), ptr(bhh), ptr(hseq), ptr(gates), ptr(hn), S, T, D, stream()), "gru_fwd")
    torch.cuda.synchronize()
    return hseq, gates, hn, h16


def grad_check(name, got, ref):
    got, ref = got.detach().cpu().float(), ref.detach().float()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
    err, top = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{name}: cosine {cos:.5f}  max error {err:.3e} of {top:.3e}")
    assert cos >= 0.995, (name, cos)
    assert err <= 5e-2 * top, (name, err, top)


# ------------------------------------------------------------------------------------------------------------------ upper layer
@pytest.mark.parametrize("S,T", [(37, 24), (16, 24), (37, 1), (37, 2), (16, 1)])
def test_upper_layer_matches_the_fp32_recurrence(S, T):
    """x and W_ih reach the GEMM rounded to bf16 exactly as A.linear rounds them (the fp32 reference keeps them unrounded), so the
    one-layer forward bound, 2e-2 abs, applies to hseq, gates and hn; the hand-over variant of the kernel writes the same three."""
    q = layer_params(11, 1)[0]
    x = torch.randn(S, T, D, generator=torch.Generator().manual_seed(S * 100 + T))
    ref, ref_gates, ref_hn = cpu_gru_layer(x @ q["w_ih"].t() + q["b_ih"], q["w_hh"], q["b_hh"])
    x16 = x.cuda().to(BF16)
    hseq, gates, hn, _ = gpu_composition(x16, q, S, T, want16=True)
    e = (hseq.cpu() - ref).abs().max().item()
    eg, eh = (gates.cpu() - ref_gates).abs().max().item(), (hn.cpu() - ref_hn).abs().max().item()
    print(f"S {S} T {T}: against fp32: hseq {e:.3e} gates {eg:.3e} hn {eh:.3e}")
    assert e <= 2e-2 and eg <= 2e-2 and eh <= 2e-2


# ------------------------------------------------------------------------------------------------------------------ hand-over (b)
@pytest.mark.parametrize("S,T", [(37, 24), (16, 2), (37, 1)])
def test_handover_is_the_rounded_hidden_state_times_the_twins_mask(S, T):
    q = layer_params(12, 1)[0]
    x16 = torch.randn(S, T, D, generator=torch.Generator().manual_seed(5)).cuda().to(BF16)
    run = gpu_composition
    hseq, _, _, h16 = run(x16, q, S, T, want16=True)
    assert torch.equal(h16, hseq.to(BF16)), "p = 0: hseq16 is hseq rounded to bf16"
    seed, sid, p = 1234567, 81, 0.5
    for epoch in (None, 5):
        with twin.pinned_epoch(epoch):
            hseq, _, _, h16 = run(x16, q, S, T, p=p, seed=seed, sid=sid, want16=True)
        mask = torch.from_numpy(twin.mask_scale(seed, sid, twin.flat_index((S, T, D)), p, epoch))
        want = (hseq.cpu() * mask).to(BF16)
        assert 0.4 < float((mask == 0).float().mean()) < 0.6
        assert torch.equal(h16.cpu().view(torch.int16), want.view(torch.int16)), epoch


def test_null_handover_leaves_the_one_layer_path_bit_for_bit(monkeypatch):
    """medp_gru_fwd (no hand-over) and medp_gru_fwd_h16 write the same hseq / gates / hn; an n_layers = 1 module never enters the
    stack's node and its tokens are those of a direct call of the one-layer path (GruFn) on the same seed."""
    from multimodal_edema_prediction_amd import autograd_ops as A
    from multimodal_edema_prediction_amd import trajectory as TR
    S, T = 37, 24
    q = layer_params(13, 1)[0]
    x16 = torch.randn(S, T, D, generator=torch.Generator().manual_seed(6)).cuda().to(BF16)
    a, b = gpu_composition(x16, q, S, T), gpu_composition(x16, q, S, T, p=0.5, seed=3, sid=80, want16=True)
    assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))

    def forbidden(*args, **kw):
        raise AssertionError("n_layers = 1 must not take the stack's node")
    monkeypatch.setattr(TR.GruStackFn, "apply", forbidden)
    torch.manual_seed(21)
    m = TR.LocalTrajectoryEncoder(n_vars=5, n_timesteps=24, d_model=D, n_layers=1, dropout=0.1).cuda().train()
    x = torch.cat([torch.randn(3, 24, 5), torch.poisson(torch.full((3, 24, 5), 0.5))], dim=2).cuda()
    torch.manual_seed(22)
    tokens = m(tuple(x))
    # the same stages called directly: the module's own input path, then GruFn, pooling and norm as forward() does them
    torch.manual_seed(22)
    B, V, d = 3, 5, D
    h = A.linear(TR.traj_features(x, V).view(B * V * T, 8), torch.nn.functional.pad(m.input_proj[0].weight, (0, 3)), m.input_proj[0].bias)
    h = A.layer_norm(A.gelu_dropout(h, 0.0, 0, 0), m.input_proj[2].weight, m.input_proj[2].bias, m.input_proj[2].eps).view(B, V, T, d)
    h = h + m.variable_embedding.weight.view(1, V, 1, d) + m.hour_embedding.weight[:T].view(1, 1, T, d)
    h = A.DropoutFn.apply(h.contiguous().view(-1, d), m.p_drop, A.next_seed(), 0)
    gi = A.linear(h, m.temporal.weight_ih_l0, m.temporal.bias_ih_l0).view(B * V, T, 3 * d)
    hs = TR.GruFn.apply(gi, m.temporal.weight_hh_l0, m.temporal.bias_hh_l0)
    pooled, prev = [], 0
    for wi, boundary in enumerate(m.recency_windows):
        pooled.append(hs[:, T - boundary:T - prev, :].mean(dim=1) + m.window_embedding.weight[wi])
        prev = boundary
    direct = A.layer_norm(torch.stack(pooled, dim=1).reshape(-1, d), m.output_norm.weight, m.output_norm.bias, m.output_norm.eps)
    assert torch.equal(tokens[:, :-1].reshape(-1, d), direct)


# ------------------------------------------------------------------------------------------------------------------ module
def _npz(name):
    z = np.load(os.path.join(GOLD, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def gold():
    g = _npz("trajectory_layers.npz")
    g["sd"] = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    g["grads"] = {k[2:]: v for k, v in _npz("trajectory_layers_grads.npz").items()}
    l3 = _npz("trajectory_layers_l3.npz")
    g["sd3"] = {**g["sd"], **{k[2:]: v for k, v in l3.items() if k.startswith("p_")}}
    g["tokens3"] = l3["tokens"]
    return g


def build(g, layers=2):
    from multimodal_edema_prediction_amd.main_architecture_duett import LocalTrajectoryEncoder
    B, T, V, d, *windows = [int(v) for v in g["cfg"]]
    m = LocalTrajectoryEncoder(n_vars=V, n_timesteps=T, d_model=d, n_layers=layers, dropout=0.1, recency_windows=tuple(windows))
    m.load_state_dict(g["sd"] if layers == 2 else g["sd3"], strict=True)
    return m.cuda().eval()


def test_two_layer_module_matches_the_reference_fixture_forward_and_backward(gold):
    m = build(gold)
    xs = tuple(t.cuda() for t in gold["x"])
    tokens, pad = m(xs, return_padding_mask=True)
    assert torch.equal(pad.cpu(), gold["pad"])
    e = (tokens.cpu() - gold["tokens"]).abs().max().item()
    print(f"tokens {e:.3e}")
    assert e <= 3e-2
    (tokens * gold["wgt"].cuda()).sum().backward()
    for k, p in m.named_parameters():
        grad_check(k, p.grad, gold["grads"][k])


def test_three_layer_module_matches_the_reference_fixture_forward(gold):
    m = build(gold, 3)
    with torch.no_grad():
        tokens, pad = m(tuple(t.cuda() for t in gold["x"]), return_padding_mask=True)
    assert torch.equal(pad.cpu(), gold["pad"])
    e = (tokens.cpu() - gold["tokens3"]).abs().max().item()
    print(f"tokens {e:.3e}")
    assert e <= 3e-2


def test_fp32_kernel_mode_matches_the_fixture(gold):
    from multimodal_edema_prediction_amd import functional as Fn
    m = build(gold)
    with Fn.precision_mode("fp32"), torch.no_grad():
        tokens, pad = m(tuple(t.cuda() for t in gold["x"]), return_padding_mask=True)
    e = (tokens.cpu() - gold["tokens"]).abs().max().item()
    print(f"fp32 mode: tokens {e:.3e}")
    assert torch.equal(pad.cpu(), gold["pad"]) and e <= 1e-4


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_backward_applies_the_twins_masks_between_the_layers(mode):
    """A train-mode two-layer stack with p = 0.5 and an explicit seed against CPU autograd through the same recurrence with the host
    replica's mask between the layers: a backward that forgets the mask, or indexes it differently, misses every bound."""
    from multimodal_edema_prediction_amd import functional as Fn
    from multimodal_edema_prediction_amd import trajectory as TR
    S, T, p, seed = 37, 24, 0.5, 424242
    q = layer_params(14, 2)
    g = torch.Generator().manual_seed(15)
    gi, wgt = torch.randn(S, T, 3 * D, generator=g), torch.randn(S, T, D, generator=g)
    mask = torch.from_numpy(twin.mask_scale(seed, TR._SID_GRU_LAYER, twin.flat_index((S, T, D)), p, None))
    leaves = [gi.clone().requires_grad_(True), q[0]["w_hh"].clone().requires_grad_(True), q[0]["b_hh"].clone().requires_grad_(True)] + \
             [q[1][k].clone().requires_grad_(True) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    h0, _, _ = cpu_gru_layer(leaves[0], leaves[1], leaves[2])
    x1 = h0 * mask
    h1, _, _ = cpu_gru_layer(x1 @ leaves[3].t() + leaves[5], leaves[4], leaves[6])
    (h1 * wgt).sum().backward()
    dev = [t.detach().clone().cuda().requires_grad_(True) for t in leaves]
    with twin.pinned_epoch(None), Fn.precision_mode(mode):
        out = TR.GruStackFn.apply(dev[0], p, seed, *dev[1:])
        (out * wgt.cuda()).sum().backward()
        torch.cuda.synchronize()
    assert (out.detach().cpu() - h1.detach()).abs().max().item() <= 2e-2
    for name, a, r in zip(("dgi (layer 0)", "dW_hh_l0", "db_hh_l0", "dW_ih_l1", "dW_hh_l1", "db_ih_l1", "db_hh_l1"), dev, leaves):
        grad_check(name, a.grad, r.grad)


# ------------------------------------------------------------------------------------------------------------------ probe
def _probe(dropout=0.1):
    from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe
    torch.manual_seed(31)
    return TrajectoryPathologyProbe(n_vars=6, n_pathologies=7, n_timesteps=24, d_model=D, gru_layers=2, n_heads=4, dropout=dropout,
                                    recency_windows=(6, 12, 24)).cuda()


def _batch():
    g = torch.Generator().manual_seed(32)
    x = torch.cat([torch.randn(5, 24, 6, generator=g), torch.poisson(torch.full((5, 24, 6), 0.6), generator=g)], dim=2)
    return {"x_ts": x.cuda(), "y": (torch.rand(5, 7, generator=g) < 0.4).float().cuda(), "mask": (torch.rand(5, 7, generator=g) < 0.8).float().cuda()}


def _optimizer(m):
    from multimodal_edema_prediction_amd.optim import FusedAdamW
    return FusedAdamW(m.parameters(), lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0)


def test_two_layer_probe_captured_step_equals_the_eager_step():
    from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce, train_probe_batch
    b = _batch()
    me = _probe().eval()
    oe = _optimizer(me)
    eager = [float(train_probe_batch(me, b, oe)["loss"]) for _ in range(3)]
    mg = _probe().eval()
    og = _optimizer(mg)
    gs = GraphedTrajectoryProbeStep(mg, masked_bce, og, b["x_ts"], b["y"], b["mask"], torch.device("cuda"), warmup=1)
    graphed = [float(gs.step(b["x_ts"], b["y"], b["mask"])["loss"]) for _ in range(3)]
    print("eager", eager, "captured", graphed)
    assert all(np.isfinite(eager))
    for a, r in zip(graphed, eager):
        assert abs(a - r) <= 1e-6
    assert og._step == oe._step == 3
    assert all(p.grad is not None and bool(p.grad.any()) for k, p in me.named_parameters() if "temporal" in k)


def test_two_layer_probe_captures_replay_bit_identically_with_dropout():
    from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce
    b = _batch()

    def run():
        m = _probe().train()
        torch.manual_seed(7)                                    # the dropout seeds are drawn from the CPU generator
        opt = _optimizer(m)
        gs = GraphedTrajectoryProbeStep(m, masked_bce, opt, b["x_ts"], b["y"], b["mask"], torch.device("cuda"), warmup=1)
        losses = [gs.step(b["x_ts"], b["y"], b["mask"])["loss"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in m.parameters()]

    l1, p1 = run()
    l2, p2 = run()
    assert len({float(v) for v in l1}) == 3, "dropout must differ between replays (device epoch)"
    assert all(torch.equal(a, c) for a, c in zip(l1, l2))
    assert all(torch.equal(a, c) for a, c in zip(p1, p2))


def test_training_driver_trains_and_reloads_a_two_layer_probe(tmp_path):
    import math
    from multimodal_edema_prediction_amd import train_synthetic
    d = str(tmp_path / "p2")
    out = train_synthetic.main(["trajectory_probe", "--ckpt_dir", d, "--gru_layers", "2", "--n_train", "256", "--n_val", "64", "--n_test", "64",
                                "--epochs", "1", "--limit_batches", "2"])
    assert math.isfinite(out["history"][-1]["train_loss"])
    state = torch.load(os.path.join(d, "best.pt"), map_location="cpu", weights_only=False)
    assert state["args"]["gru_layers"] == 2
    m = train_synthetic.build_trajectory_probe_from_ckpt(state)
    assert m.encoder.n_layers == 2 and m.encoder.temporal.num_layers == 2
    assert torch.equal(m.encoder.temporal.weight_ih_l1, state["model"]["encoder.temporal.weight_ih_l1"])
