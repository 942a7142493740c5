"""Gradient-flow diagnostics end to end on the GPU: the one-pass report against what the reference's own functions returned
(tests/golden/grad_flow_small.npz on a tiny perceiver, tests/golden/grad_flow_cfg1.npz on the cfg1 teacher), against the looped form
(4K + 4 calls of autograd.grad on the public teacher forward), its side effects, the chunked pass and the CLI.

Deviations are measured per class of value (tests/grad_flow_refs.py: compare_reports): losses, gradient norms / sensitivities, cosines
and fractions in absolute terms, the *_over_ts ratios in relative terms.  Each bound below is 4x the worst deviation measured on an
MI355X (cosines of nearly orthogonal 1792-vectors amplify rounding); the measured values stand next to the constants and in DESIGN.md
§6.G.  A norm or loss further from the golden than the element-wise fp32-mode gradient tolerance of tests/test_gpu_fp32_mode.py
(2e-4 of the largest value) would be a bug, not a tolerance: asserted separately."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import grad_flow_refs as R
from helpers import load_npz

pytestmark = pytest.mark.gpu

from multimodal_edema_prediction_amd import functional as Fn  # noqa: E402
from multimodal_edema_prediction_amd import grad_flow_diagnostics as G  # noqa: E402
from multimodal_edema_prediction_amd.cohort import make_batch  # noqa: E402
from multimodal_edema_prediction_amd.losses_duett import DualPathologyLoss  # noqa: E402
from multimodal_edema_prediction_amd.main_architecture_duett import PatchDualPathologyPerceiver  # noqa: E402

DEV = "cuda"
ABS, REL = 0, 1
FP32_GRAD_TOL = 2e-4             # tests/test_gpu_fp32_mode.py::_grad_close, relative to the largest value

# worst deviation measured on an MI355X -> the asserted bound is 4x that                     measured
SMALL_FP32 = {"loss": 4 * 3.080e-7, "norm": 4 * 7.754e-8, "cos": 4 * 2.249e-7, "fraction": 4 * 1.271e-7, "ratio": 4 * 3.050e-8}
CFG1_FP32 = {"loss": 4 * 6.557e-7, "norm": 4 * 8.573e-7, "cos": 4 * 2.384e-7, "fraction": 4 * 1.193e-7, "ratio": 4 * 2.050e-7}
# the one-pass report against the looped form; "dq": q_rep.grad[g] and the token gradients element-wise against the looped
# autograd.grad, relative to the largest element (bf16 mode: both forms round their GEMM operands to bf16, on other batch shapes)
ONE_PASS_VS_LOOP = {"fp32": {"loss": 4 * 4.768e-7, "norm": 4 * 5.786e-8, "cos": 4 * 2.107e-8, "fraction": 4 * 5.922e-9, "ratio": 4 * 1.252e-8,
                             "dq": 4 * 5.228e-7},
                    "bf16": {"loss": 4 * 2.384e-7, "norm": 4 * 8.920e-7, "cos": 4 * 2.830e-6, "fraction": 4 * 1.470e-7, "ratio": 4 * 7.375e-8,
                             "dq": 4 * 2.201e-3}}
# recorded, not asserted: bf16 mode against the cfg1 golden: loss 4.4e-2, norm 1.7e-2, cos 1.6e-3, fraction 5.0e-4, ratio 3.6e-3 (relative);
# one replica per pass against all replicas in one pass (fp32 mode): loss 0, norm 2.5e-8, cos 2.8e-8, fraction 5.5e-9, ratio 4.1e-9


def deviation(worst, cls):
    return worst[cls][REL if cls in R.RELATIVE_CLASSES else ABS]


def within(worst, bounds, what):
    print(what, {cls: f"{deviation(worst, cls):.3e}" for cls in worst})
    for cls in worst:
        assert deviation(worst, cls) <= bounds[cls], (what, cls, deviation(worst, cls), bounds[cls])


# ---- the tiny perceiver of grad_flow_small.npz ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_problem():
    g = load_npz("grad_flow_small.npz")
    K, d_ts, D, heads = (int(v) for v in g["cfg"][:4])
    pc = PatchDualPathologyPerceiver(n_pathologies=K, d_ts=d_ts, d_latent=D, n_heads=heads, dropout=0.0, head_dropout=0.0)
    pc.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}, strict=True)
    pc = pc.to(DEV)
    f = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    batches = [(f(g[f"b{i}_ts_tokens"])[:, :-1].contiguous(), f(g[f"b{i}_img_patches_proj"]), 0, f(g[f"b{i}_y"]), f(g[f"b{i}_mask"]))
               for i in range(len(g["batch_sizes"]))]
    loss_fn = DualPathologyLoss(torch.from_numpy(g["label_weights"]), torch.from_numpy(g["pos_weight"]), *g["alphas"].tolist()).to(DEV)
    return g, pc, batches, loss_fn, json.loads(str(g["report_json"]))


def small_report(mode, collect=None):
    g, pc, batches, loss_fn, _ = small_problem()
    with Fn.precision_mode(mode):
        return G.perceiver_gradient_diagnostics(pc, batches, loss_fn, label_names=[str(s) for s in g["labels"]], _collect=collect)


def test_small_golden_fp32():
    g, _, _, _, want = small_problem()
    collected = []
    got = small_report("fp32", collected)
    worst = R.compare_reports(got, want)
    within(worst, SMALL_FP32, "small golden, fp32 mode")
    assert worst["loss"][REL] <= FP32_GRAD_TOL and worst["norm"][REL] <= FP32_GRAD_TOL, worst
    assert G.format_gradient_diagnostics(got).splitlines()[0] == str(g["format_text"]).splitlines()[0]
    # the replicated backward against the reference's own per-label `_grads` results, element-wise
    for i, (dq, dT) in enumerate(collected):
        for got_t, key in ((dq, f"b{i}_dq"), (dT, f"b{i}_dT")):
            err = float((got_t.cpu() - torch.from_numpy(g[key])).abs().max())
            assert err <= FP32_GRAD_TOL * float(np.abs(g[key]).max()) + 1e-7, (key, err)
    assert not collected[1][0][:, 1].any() and not collected[1][1][:, 1].any()          # the fully masked label of batch 1: exact zeros


# ---- the cfg1 teacher ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg1():
    import test_gpu_model as Tm
    teacher = Tm.build_teacher()
    batches = [make_batch(Tm.CCFG, start, 8, mode="teacher") for start in (100, 101)]
    loss_fn = DualPathologyLoss(torch.ones(Tm.K), None, 0.5, 0.5, 1.0).to(DEV)
    want = json.loads(str(load_npz("grad_flow_cfg1.npz")["report_json"]))
    cache = {}

    def report(mode, kind="one_pass", **kw):
        key = (mode, kind) + tuple(sorted(kw))
        if key not in cache:
            collected = []
            with Fn.precision_mode(mode):
                fn = G.run_dual_gradient_diagnostics if kind == "one_pass" else G._looped_reference
                cache[key] = (fn(teacher, batches, loss_fn, DEV, max_batches=2, _collect=collected, **kw), collected)
        return cache[key]

    return teacher, batches, loss_fn, want, report


def test_cfg1_golden_fp32(cfg1):
    _, _, _, want, report = cfg1
    worst = R.compare_reports(report("fp32")[0], want)
    within(worst, CFG1_FP32, "cfg1 golden, fp32 mode")
    assert worst["loss"][REL] <= FP32_GRAD_TOL and worst["norm"][REL] <= FP32_GRAD_TOL, worst


def test_cfg1_golden_bf16_recorded(cfg1):
    """bf16 kernel mode: the deviation from the golden is printed and recorded, not asserted; the report must be
    complete and finite."""
    _, _, _, want, report = cfg1
    worst = R.compare_reports(report("bf16")[0], want)
    print("cfg1 golden, bf16 mode", {cls: f"{deviation(worst, cls):.3e}" for cls in worst})
    assert all(np.isfinite(v[0]) for v in worst.values())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_one_pass_equals_the_loop(cfg1, mode):
    _, _, _, _, report = cfg1
    (one, one_t), (loop, loop_t) = report(mode), report(mode, "loop")
    worst = R.compare_reports(one, loop)
    dq_dev = 0.0
    for (dq, dT), (dq_l, dT_l, totals, _) in zip(one_t, loop_t):
        scale = float(dq_l.abs().max())
        dq_dev = max(dq_dev, float((dq - dq_l).abs().max()) / scale, float((dT - dT_l).abs().max()) / float(dT_l.abs().max()))
        # linearity: the loop's separately computed branch totals are the label sums of the replicas' gradients
        dq_dev = max(dq_dev, float((dq.sum(1) - totals).abs().max()) / float(totals.abs().max()))
    worst["dq"] = (dq_dev, dq_dev)
    within(worst, ONE_PASS_VS_LOOP[mode], f"one pass vs loop, {mode} mode (dq: element-wise, relative to the largest element)")


def test_side_effects(cfg1):
    from multimodal_edema_prediction_amd import engine
    teacher, batches, loss_fn, _, report = cfg1
    engine._set_train_with_frozen_eval(teacher)
    modes = [m.training for m in teacher.modules()]
    assert teacher.training and not teacher.cxr.training
    before = {k: v.detach().clone() for k, v in teacher.named_parameters()}
    flags = [p.requires_grad for p in teacher.parameters()]
    teacher.zero_grad(set_to_none=True)
    with Fn.precision_mode("fp32"):
        first = G.run_dual_gradient_diagnostics(teacher, batches, loss_fn, DEV, max_batches=2)
        second = G.run_dual_gradient_diagnostics(teacher, batches, loss_fn, DEV, max_batches=2)
    assert [m.training for m in teacher.modules()] == modes
    assert [p.requires_grad for p in teacher.parameters()] == flags
    assert all(p.grad is None for p in teacher.parameters())
    assert all(torch.equal(p.detach(), before[k]) for k, p in teacher.named_parameters())
    assert first == second == report("fp32")[0]
    # ... also when the pass fails half way
    with pytest.raises(ValueError, match="label_names"):
        G.run_dual_gradient_diagnostics(teacher, batches, loss_fn, DEV, label_names=["a"])
    broken = [batches[0], {k: v for k, v in batches[1].items() if k != "y_multi"}]
    with pytest.raises(KeyError):
        G.run_dual_gradient_diagnostics(teacher, broken, loss_fn, DEV, max_batches=2)
    assert [m.training for m in teacher.modules()] == modes and [p.requires_grad for p in teacher.parameters()] == flags
    with pytest.raises(RuntimeError, match="yielded no batches"):
        G.run_dual_gradient_diagnostics(teacher, [], loss_fn, DEV)
    teacher.eval()


def test_chunked_pass(cfg1):
    """One replica per pass (the route of more than 1536 keys, forced): the unchunked report within the one-pass-vs-loop bound."""
    _, _, _, _, report = cfg1
    worst = R.compare_reports(report("fp32", _chunk=1)[0], report("fp32")[0])
    within(worst, ONE_PASS_VS_LOOP["fp32"], "one replica per pass vs all replicas in one pass, fp32 mode")
    assert G._replicas_per_pass(1369, 7, None) is None and G._replicas_per_pass(1600, 7, None) == 4 and G._replicas_per_pass(256, 7, 1) == 1


def test_cli_on_a_train_synthetic_checkpoint(tmp_path):
    from multimodal_edema_prediction_amd import train_synthetic
    import test_gpu_train_synthetic as Ts
    t = train_synthetic.main(["teacher", "--ckpt_dir", str(tmp_path / "t"), "--epochs", "1", "--freeze_duett"] + Ts.TINY)
    out = G.main(["--ckpt", t["ckpt"], "--outdir", str(tmp_path / "diag"), "--split", "val", "--batch_size", "8", "--max_batches", "2",
                  "--num_workers", "0"])
    assert os.path.isfile(out["txt"]) and os.path.isfile(out["json"])
    with open(out["json"]) as f:
        assert json.load(f) == out["report"]
    with open(out["txt"]) as f:
        assert f.read() == G.format_gradient_diagnostics(out["report"]) + "\n"
    assert out["report"]["batches"] == 2 and out["report"]["samples"] == 16 and len(out["report"]["per_label"]) == 7
    assert out["report"]["query_parameter"] == "perceiver.shared_queries" and out["report"]["query_layout"] == "shared"
