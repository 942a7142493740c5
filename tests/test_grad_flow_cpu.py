"""Gradient-flow diagnostics without a GPU: the fp64 numpy replica of the kernels (tests/grad_flow_refs.py) against what the
reference's own functions returned on tests/golden/grad_flow_small.npz, the host-only restatements against the reference's recorded
text, and the errors that are raised before anything reaches a kernel."""
import json

import numpy as np
import pytest
import torch

import grad_flow_refs as R
from helpers import load_npz
from multimodal_edema_prediction_amd import grad_flow_diagnostics as G
from multimodal_edema_prediction_amd.main_architecture_duett import DualPathologyPerceiver, PatchDualPathologyPerceiver

# The reference accumulates in fp32; the replica takes the SAME fp32 per-batch tensors (the reference's own `_grads` results) and
# sums in fp64.  A reported norm or loss then carries the reference's roundings only: <= 3 batch additions and the division by the
# batch count per element, a pairwise fp32 sum over <= 3 * 3 * 32 = 288 squares (<= 9 levels), the square root and the products with
# alpha / label weights: about 16 roundings of <= 2^-24 relative each.  Cosines divide by two such norms, ratios divide two such
# values: twice that, 32 * 2^-24 = 1.9e-6, absolute for cosines and fractions (|cos| <= 1), relative for everything else.
# Observed here on the CPU: relative 8.1e-8 (loss), 1.1e-7 (norm), 3.2e-8 (ratio); absolute 8.5e-8 (cos), 9.5e-8 (fraction).
BOUND = 32 * 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return load_npz("grad_flow_small.npz")


@pytest.fixture(scope="module")
def want(gold):
    return json.loads(str(gold["report_json"]))


def replica_report(gold):
    K, _, D = (int(v) for v in gold["cfg"][:3])
    state = R.new_state(K, D)
    for i in range(len(gold["batch_sizes"])):
        R.accumulate(state, gold[f"b{i}_dq"], None, gold[f"b{i}_dT"], gold[f"b{i}_I"], gold[f"b{i}_T"], gold[f"b{i}_mask"], gold[f"b{i}_losses"])
    w = {k[2:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("w:")}
    q = w["shared_queries"]

    def effective(block):
        n = torch.nn.functional.layer_norm(q, (D,), w[f"{block}.norm_q.weight"], w[f"{block}.norm_q.bias"])
        return torch.nn.functional.linear(n, w[f"{block}.attn.in_proj_weight"][:D], w[f"{block}.attn.in_proj_bias"][:D])

    rows = torch.stack([q, effective("img_cross"), effective("ts_cross")]).numpy()
    vec = np.concatenate([R.report(state, gold["alphas"], K, D), R.query_geometry(rows)])
    return G.report_from_vector(vec.tolist(), K, [str(s) for s in gold["labels"]], gold["alphas"].tolist(), "perceiver.shared_queries")


def test_replica_reproduces_the_reference_report(gold, want):
    got = replica_report(gold)
    worst = R.compare_reports(got, want)                     # also: same keys in the same order, same types, equal integers
    print({k: (f"{a:.2e}", f"{r:.2e}") for k, (a, r) in worst.items()})
    for cls in ("loss", "norm", "ratio"):
        assert worst[cls][1] <= BOUND, (cls, worst[cls])
    for cls in ("cos", "fraction"):
        assert worst[cls][0] <= BOUND, (cls, worst[cls])
    assert want["pairwise_gradient_cosine"]["img_ts_negative_batch_fraction"] == pytest.approx(2 / 3, abs=1e-7)
    masked = want["per_label"][1]
    assert masked["valid_samples"] == got["per_label"][1]["valid_samples"] < 16 * 0.8


def test_replica_seeds_match_the_reference_losses(gold):
    """The seeds replica's losses are the reference's lw_k per_k; its cotangents are zero outside column k of replica (branch, k), and
    in the batch whose label 1 is fully masked that label's cotangent is zero everywhere."""
    K = int(gold["cfg"][0])
    rng = np.random.default_rng(0)
    for i, B in enumerate(gold["batch_sizes"]):
        logits = [rng.standard_normal((B, K)).astype(np.float32) for _ in range(3)]
        losses, cot_img, cot_ts, cot_fus = R.seeds(*logits, gold[f"b{i}_y"], gold[f"b{i}_mask"], gold["label_weights"], gold["pos_weight"], 1e-6)
        y, m = torch.from_numpy(gold[f"b{i}_y"]).double(), torch.from_numpy(gold[f"b{i}_mask"]).double()
        for r, l in enumerate(logits):
            z = torch.from_numpy(l).double().requires_grad_(True)
            bce = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none", pos_weight=torch.from_numpy(gold["pos_weight"]).double())
            per = torch.from_numpy(gold["label_weights"]).double() * (bce * m).sum(0) / (m.sum(0) + 1e-6)
            np.testing.assert_allclose(losses[r], per.detach().numpy(), rtol=1e-9, atol=1e-12)
            for k in range(K):
                (g,) = torch.autograd.grad(per[k], z, retain_graph=True)
                cot = (cot_img[:, k], cot_ts[:, k], cot_fus[:, K + k])[r]
                np.testing.assert_allclose(cot, g.numpy(), rtol=1e-9, atol=1e-12)
        assert np.count_nonzero(cot_ts[:, K:]) == 0 and np.count_nonzero(cot_fus[:, :K]) == 0
        if i == 1:
            assert np.count_nonzero(cot_img[:, 1]) == 0 and losses[0, 1] == 0.0


def test_format_equals_the_recorded_text(gold, want):
    assert G.format_gradient_diagnostics(want) == str(gold["format_text"])
    independent = dict(want, query_layout="independent")
    assert "disjoint parameter banks" in G.format_gradient_diagnostics(independent)


def test_log_dict_equals_the_recorded_items(gold, want):
    log = G.gradient_diagnostics_to_log_dict(want)
    assert list(log) == [str(k) for k in gold["log_keys"]]
    assert list(log.values()) == gold["log_values"].tolist()
    assert all(k.startswith("x/") for k in G.gradient_diagnostics_to_log_dict(want, prefix="x"))


def test_report_has_the_reference_key_set(gold, want):
    got = replica_report(gold)

    def keys(node):
        if isinstance(node, dict):
            return {k: keys(v) for k, v in node.items()}
        if isinstance(node, list):
            return [keys(v) for v in node]
        return type(node).__name__

    assert keys(got) == keys(want)
    assert got["query_layout"] == "shared" and got["query_parameter"] == "perceiver.shared_queries"


class _Holder(torch.nn.Module):
    def __init__(self, perceiver):
        super().__init__()
        self.perceiver = perceiver


def test_bank_lookup():
    patch = _Holder(PatchDualPathologyPerceiver(3, 24, 32, 4, 0.0))
    names, params = G._find_pathology_query_banks(patch)
    assert names == ("perceiver.shared_queries",) and params[0] is patch.perceiver.shared_queries
    wrapped = torch.nn.Module()
    wrapped.module = patch
    assert G._unwrap_model(wrapped) is patch
    dual = _Holder(DualPathologyPerceiver(3, 24, 32, 4, 0.0))
    with pytest.raises(RuntimeError, match=r"Expected image_queries \+ temporal_queries, or one legacy pathology_queries; "
                                           r"found image=0, temporal=1, shared=0"):
        G._find_pathology_query_banks(dual)
    with pytest.raises(RuntimeError, match="found image=0, temporal=0, shared=0"):
        G.run_dual_gradient_diagnostics(torch.nn.Linear(2, 2), [], None, "cpu")


def test_errors_before_any_kernel():
    patch = _Holder(PatchDualPathologyPerceiver(3, 24, 32, 4, 0.0))
    with pytest.raises(NotImplementedError, match="accelerator"):
        G.run_dual_gradient_diagnostics(patch, [], None, "cpu", accelerator=object())
    with pytest.raises(ValueError, match="max_batches must be positive"):
        G.run_dual_gradient_diagnostics(patch, [], None, "cpu", max_batches=0)
    patch.perceiver.shared_queries.requires_grad_(False)
    with pytest.raises(RuntimeError, match="perceiver.shared_queries does not require gradients"):
        G.run_dual_gradient_diagnostics(patch, [], None, "cpu")


def test_cli_arguments():
    args = G.parse_args(["--ckpt", "a.pt", "--outdir", "o"])
    assert (args.split, args.batch_size, args.max_batches, args.num_workers) == ("train", 16, 16, 2)
