"""CPU: the host side of probe_stats.py, what the analysis probes share: the row fields and the `evidence` rule, the small host
helpers and the order of the conditional-shuffle draws.  `draw_bootstrap_indices` and `draw_cluster_bootstrap_indices` are pinned on
the reference's fixtures by tests/test_cond_probe_refs_cpu.py and tests/test_raw_probe_refs_cpu.py; what reaches the metrics kernel
is in tests/test_gpu_raw_probe_kernels.py."""
import numpy as np

from multimodal_edema_prediction_amd import conditional_information_probe as cip
from multimodal_edema_prediction_amd import evaluator, probe_stats as ps

BASE = {"bce": 0.60, "auroc": 0.70, "auprc": 0.50}
PROBE = {"bce": 0.50, "auroc": 0.75, "auprc": 0.58}
CONFIDENCE = {"bce_gain_ci_low": 0.02, "bce_gain_ci_high": 0.18, "auroc_gain_ci_low": -0.01, "auroc_gain_ci_high": 0.11,
              "auprc_gain_ci_low": 0.01, "auprc_gain_ci_high": 0.15}
PERMUTATION = {"perm_bce_mean": 0.58, "perm_bce_low": 0.55, "perm_bce_high": 0.61, "perm_auroc_mean": 0.71, "perm_auroc_low": 0.69,
               "perm_auroc_high": 0.73, "perm_auprc_mean": 0.52, "perm_auprc_low": 0.49, "perm_auprc_high": 0.55}


def test_inference_fields_are_the_shared_row_keys_in_the_references_order():
    fields, evidence = ps.inference_fields(BASE, PROBE, CONFIDENCE, 0.25, PERMUTATION)
    keys = cip.ROW_KEYS
    assert tuple(fields) == keys[keys.index("image_cal_bce"):keys.index("perm_auroc_drop") + 1] and keys[-1] == "evidence"
    assert evidence == "supported"
    assert fields["image_cal_bce"] == 0.60 and fields["probe_auprc"] == 0.58 and fields["corr_residual"] == 0.25
    assert fields["bce_gain"] == 0.60 - 0.50 and fields["auroc_gain"] == 0.75 - 0.70 and fields["auprc_gain"] == 0.58 - 0.50
    assert fields["perm_bce_increase"] == 0.58 - 0.50 and fields["perm_auroc_drop"] == 0.75 - 0.71
    assert all(fields[k] == v for k, v in {**CONFIDENCE, **PERMUTATION}.items())


def test_evidence_rule():
    verdict = lambda probe, confidence, permutation: ps.inference_fields(BASE, probe, confidence, 0.0, permutation)[1]  # noqa: E731
    assert verdict(PROBE, CONFIDENCE, PERMUTATION) == "supported"        # gain > 0, CI low > 0, permutation increase > 0
    for low in (0.0, -0.02, float("nan")):                               # one condition changed: the interval reaches zero
        assert verdict(PROBE, {**CONFIDENCE, "bce_gain_ci_low": low}, PERMUTATION) == "suggestive"
    assert verdict(PROBE, CONFIDENCE, {**PERMUTATION, "perm_bce_mean": 0.50}) == "suggestive"       # the permutation does not hurt
    for bce in (0.60, 0.65):                                             # gain <= 0, whatever the interval and the permutation say
        assert verdict({**PROBE, "bce": bce}, CONFIDENCE, {**PERMUTATION, "perm_bce_mean": 0.9}) == "not_detected"


def test_host_helpers():
    low, high = ps.ci95(np.zeros(0))
    assert np.isnan(low) and np.isnan(high)
    assert ps.ci95(np.arange(101.0)) == (2.5, 97.5)
    assert np.isnan(ps.pearson(np.ones(4), np.arange(4.0))) and np.isnan(ps.pearson(np.arange(4.0), np.full(4, 2.5)))
    assert np.isnan(ps.pearson(np.ones(1), np.ones(1)))
    assert abs(ps.pearson(np.arange(5.0), 3.0 - 2.0 * np.arange(5.0)) + 1.0) < 1e-15
    assert evaluator._pearson is ps.pearson
    s = np.array([-800.0, -1.0, 0.0, 1.0, 800.0])
    np.testing.assert_allclose(ps.expit(s), [0.0, 1.0 / (1.0 + np.e), 0.5, 1.0 / (1.0 + np.exp(-1.0)), 1.0], rtol=4e-16, atol=0)
    assert ps.expit(s)[0] == 0.0 and ps.expit(s)[2] == 0.5 and ps.expit(s)[4] == 1.0          # no overflow at either end
    # StandardScaler's rule: a constant column keeps scale 1, in the numpy form and in the torch form
    import torch
    z = np.array([[3.0, 1.0], [3.0, 2.0], [3.0, 4.0]])
    mean, var = z.mean(0), z.var(0)
    assert ps.unit_or_sd(var[0], mean[0], 3) == 1.0 and ps.unit_or_sd(var[1], mean[1], 3) == np.sqrt(var[1])
    assert np.array_equal(ps.unit_or_sd(torch.as_tensor(var), torch.as_tensor(mean), 3).numpy(), [1.0, np.sqrt(var[1])])


def test_conditional_shuffles_are_the_old_sequence_of_draws():
    image_logit = np.round(np.random.default_rng(3).normal(size=40), 1)  # ties, also across the quantile edges
    assert len(np.unique(image_logit)) < 40
    got = ps.draw_conditional_shuffles(image_logit, 4, 3, seed=7)
    bins = ps.image_risk_bins(image_logit, 4)                            # the old sequence: the bins, ONE generator, three calls
    rng = np.random.default_rng(7)
    want = [ps.conditional_shuffle_indices(bins, rng) for _ in range(3)]
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert len(np.unique(bins)) == 4 and not np.array_equal(got[0], got[1])
    for shuffle in got:                                                  # a permutation that stays within its image-risk bin
        assert np.array_equal(np.sort(shuffle), np.arange(40)) and np.array_equal(bins[shuffle], bins)
    assert ps.draw_conditional_shuffles(image_logit, 4, 0, seed=7) == []
