"""`TrajectoryPathologyProbe`, `masked_bce`, `train_probe_batch` and `GraphedTrajectoryProbeStep` against the fixture the reference's
own class produced (tests/golden/trajectory_probe*.npz, make_golden_trajectory_probe.py: 4 observed samples + 1 without any
observation, T 24, V 6, d 128, 4 heads, 7 labels, windows 6 / 12 / 24).
Bounds: fp32 kernel mode — logits 1e-4 abs, loss 1e-5 rel, averaged attention 1e-5 (the project's fp32-mode bounds); bf16 mode —
logits 3e-2, gradient cosine 0.995 (what test_gpu_trajectory uses behind the GRU), three training losses 1e-2 rel; captured against
eager 1e-6; two captures bit-identical."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _npz(name):
    z = np.load(os.path.join(GOLD, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def gold():
    g = _npz("trajectory_probe.npz")
    g["sd"] = {**_npz("trajectory_probe_params_encoder.npz"), **_npz("trajectory_probe_params_readout.npz")}
    g["grads"] = {**_npz("trajectory_probe_grads_encoder.npz"), **_npz("trajectory_probe_grads_readout.npz")}
    return g


def build(g, dropout=0.1):
    from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe
    B, T, V, d, H, K, *windows = [int(v) for v in g["cfg"]]
    m = TrajectoryPathologyProbe(n_vars=V, n_pathologies=K, n_timesteps=T, d_model=d, gru_layers=1, n_heads=H, dropout=dropout,
                                 recency_windows=tuple(windows))
    m.load_state_dict(g["sd"], strict=True)
    return m.cuda().eval()


def batch(g):
    return {"x_ts": g["x"].cuda(), "y": g["y"].cuda(), "mask": g["mask"].cuda()}


def test_state_dict_is_the_reference_modules(gold):
    from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe
    B, T, V, d, H, K, *windows = [int(v) for v in gold["cfg"]]
    m = TrajectoryPathologyProbe(V, K, T, d, 1, H, 0.1, tuple(windows))
    assert sorted(m.state_dict()) == sorted(gold["sd"])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in gold["sd"].items()}
    m.load_state_dict(gold["sd"], strict=True)


def test_fp32_mode_matches_the_reference(gold):
    """fp32 mode runs the GRU forward in fp32 too (medp_gru_fwd_f32): with the bf16 recurrence the averaged attention was 1.15e-5,
    above its bound.  Measured with the fp32 recurrence: logits 2.7e-7, attention 3.0e-8, loss equal to the last bit."""
    from multimodal_edema_prediction_amd import functional as Fn
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce
    m, b = build(gold), batch(gold)
    with Fn.precision_mode("fp32"), torch.no_grad():
        logits, attn = m(tuple(b["x_ts"]), return_attn=True)
        _, pad = m.encoder(tuple(b["x_ts"]), return_padding_mask=True)
        loss = masked_bce(logits, b["y"], b["mask"])
    assert torch.equal(pad[:, :-1].cpu(), gold["pad"])
    n = gold["attn"].shape[0]                                   # the observed samples (the reference's weights are NaN for the other)
    dl = (logits.cpu() - gold["logits"]).abs().max().item()
    da = (attn[:n].cpu() - gold["attn"]).abs().max().item()
    dloss = abs(float(loss) - float(gold["loss"])) / float(gold["loss"])
    print(f"fp32 mode: max|dlogit| {dl:.3e}  max|dattn| {da:.3e}  rel dloss {dloss:.3e}")
    assert bool((attn[n:] == 0).all()), "a fully masked sample attends to nothing"
    assert bool((attn.cpu()[:n][gold["pad"][:n, None, :].expand(-1, attn.shape[1], -1)] == 0).all())
    assert dl <= 1e-4 and da <= 1e-5 and dloss <= 1e-5


def test_bf16_mode_logits_and_gradients(gold):
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce
    m, b = build(gold), batch(gold)
    logits = m(b["x_ts"])
    dl = (logits.detach().cpu() - gold["logits"]).abs().max().item()
    print(f"bf16 mode: max|dlogit| {dl:.3e}")
    assert dl <= 3e-2
    masked_bce(logits, b["y"], b["mask"]).backward()
    cos = {}
    for k, p in m.named_parameters():
        ref = gold["grads"][k]
        if not bool(ref.any()):                                 # encoder.rep_token: the probe drops the REP token, its gradient is zero
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        cos[k] = torch.nn.functional.cosine_similarity(p.grad.cpu().flatten(), ref.flatten(), dim=0).item()
    print("bf16 mode: worst gradient cosine", min((v, k) for k, v in cos.items()))
    for k, v in cos.items():
        assert v >= 0.995, (k, v)


def test_fully_masked_sample_is_finite_and_equals_the_reference(gold):
    m, b = build(gold), batch(gold)
    n = gold["attn"].shape[0]
    assert bool(gold["pad"][n:].all())
    with torch.no_grad():
        z = m(b["x_ts"])[n:].cpu()
    assert bool(torch.isfinite(z).all())
    assert (z - gold["logits"][n:]).abs().max().item() <= 3e-2


def test_masked_bce_of_an_empty_mask_is_zero(gold):
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce
    z = gold["logits"].cuda().requires_grad_(True)
    loss = masked_bce(z, gold["y"].cuda(), torch.zeros_like(gold["mask"]).cuda())
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((z.grad == 0).all())


def _optimizer(m):
    from multimodal_edema_prediction_amd.optim import FusedAdamW
    return FusedAdamW(m.parameters(), lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0)


def test_three_training_steps_track_the_reference_losses(gold):
    from multimodal_edema_prediction_amd.trajectory_probe import train_probe_batch
    m, b = build(gold), batch(gold)                             # eval(): dropout off, as the fixture's steps
    opt = _optimizer(m)
    losses, norms = [], []
    for _ in range(3):
        losses.append(float(train_probe_batch(m, b, opt)["loss"]))
        norms.append(float(opt.last_grad_norm))
    ref = [float(v) for v in gold["step_losses"]]
    print("losses", losses, "reference", ref, "grad norms", norms, "reference's first", float(gold["grad_norm"]))
    for a, r in zip(losses, ref):
        assert abs(a - r) <= 1e-2 * abs(r)
    # the clip engages on the first step (norm above 1.0); 5 % is test_gpu_trajectory's bound on gradient magnitudes behind the GRU
    assert norms[0] > 1.0 and abs(norms[0] - float(gold["grad_norm"])) <= 5e-2 * float(gold["grad_norm"])


def test_captured_step_equals_the_eager_step(gold):
    from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce, train_probe_batch
    b = batch(gold)
    me = build(gold)
    oe = _optimizer(me)
    eager = [float(train_probe_batch(me, b, oe)["loss"]) for _ in range(3)]
    mg = build(gold)
    og = _optimizer(mg)
    gs = GraphedTrajectoryProbeStep(mg, masked_bce, og, b["x_ts"], b["y"], b["mask"], torch.device("cuda"), warmup=1)
    graphed = [float(gs.step(b["x_ts"], b["y"], b["mask"])["loss"]) for _ in range(3)]
    print("eager", eager, "captured", graphed)
    for a, r in zip(graphed, eager):
        assert abs(a - r) <= 1e-6
    assert og._step == oe._step == 3


def test_two_captures_replay_bit_identically_with_dropout(gold):
    from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
    from multimodal_edema_prediction_amd.trajectory_probe import masked_bce
    b = batch(gold)

    def run():
        torch.manual_seed(7)                                    # the dropout seeds are drawn from the CPU generator
        m = build(gold, dropout=0.1).train()
        opt = _optimizer(m)
        gs = GraphedTrajectoryProbeStep(m, masked_bce, opt, b["x_ts"], b["y"], b["mask"], torch.device("cuda"), warmup=1)
        losses = [gs.step(b["x_ts"], b["y"], b["mask"])["loss"].clone() for _ in range(3)]
        norm = opt.last_grad_norm.clone()
        torch.cuda.synchronize()
        return losses, norm, [p.detach().clone() for p in m.parameters()]

    l1, n1, p1 = run()
    l2, n2, p2 = run()
    assert len({float(v) for v in l1}) == 3, "dropout must differ between replays (device epoch)"
    assert all(torch.equal(a, c) for a, c in zip(l1, l2)) and torch.equal(n1, n2)
    assert all(torch.equal(a, c) for a, c in zip(p1, p2))
