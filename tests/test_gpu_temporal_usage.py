"""GPU: the temporal-usage diagnostics end to end.

Against the reference's fixture (tests/golden/temporal_usage.npz: the reference's own `_metrics_by_label`, `_cluster_bootstrap_delta` and
the expressions of its sections [3] / [4] on one seeded `pred`, tests/golden/make_golden_temporal_usage.py):
  rank metrics, every bootstrap output   1e-10, the bound tests/test_gpu_cond_probe.py uses for the metrics kernel: AUROC / AUPRC are
                                         functions of the ORDER of the probabilities, which cannot differ (the fixture asserts that
                                         distinct logits give distinct fp32 probabilities, and its logits stay inside +-6, far from
                                         the clip at 1e-7); means and quantiles of such values inherit the bound;
  sensitivity, entropy                   1e-5: the reference accumulates them in fp32.
Against the public path: for `dual` and `dual_patch` every gathered tensor is `torch.equal` to the public `teacher(...)` called on the
host-transformed tuples of the same draws; the image encoder runs once per batch.
End to end: `main` on a saved synthetic checkpoint writes the reference's archive, which `residual_by_confidence.main` then reads."""
import argparse
import os

import numpy as np
import pytest
import torch

from temporal_usage_refs import CONDITIONS, golden, golden_pred, host_conditions
from tests_dual_common import cxr_head_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
_state = {}


def _dtu():
    from multimodal_edema_prediction_amd import diagnose_temporal_usage
    return diagnose_temporal_usage


def _summary():
    if "summary" not in _state:
        g = golden()
        _state["summary"] = _dtu().summarise(golden_pred(g), [str(s) for s in g["labels"]], int(g["cfg"][5]), int(g["cfg"][6]))
    return _state["summary"]


def test_summarise_rank_metrics_equal_the_references():
    g, s = golden(), _summary()
    labels = [str(x) for x in g["labels"]]
    assert list(s) == ["labels", "baseline", "conditions", "sensitivity", "entropy", "audit", "n_boot", "bootstrap"]
    base = s["baseline"]
    assert [r["label"] for r in base] == labels
    got = np.array([[r["n"], r["pos_frac"], r["img_auroc"], r["img_auprc"]] for r in base])
    np.testing.assert_allclose(got, g["metrics_img"], rtol=0, atol=1e-10)
    got = np.array([[r["n"], r["pos_frac"], r["ts_auroc"], r["ts_auprc"]] for r in base])
    np.testing.assert_allclose(got, g["metrics_ts_full"], rtol=0, atol=1e-10)
    rows = s["conditions"]
    assert [(r["condition"], r["label"]) for r in rows] == [(c, l) for c in CONDITIONS for l in labels]
    got = np.array([[r["auroc"], r["auprc"]] for r in rows]).reshape(5, 3, 2)
    worst = np.abs(got - g["metrics_fus"][:, :, 2:]).max()
    print(f"fusion AUROC / AUPRC per condition and label: largest deviation {worst:.3e} (bound 1e-10)")
    assert worst <= 1e-10
    deltas = np.array([[r["d_auroc"], r["d_auprc"]] for r in rows]).reshape(5, 3, 2)
    np.testing.assert_allclose(deltas, g["metrics_fus"][:, :, 2:] - g["metrics_fus"][:1, :, 2:], rtol=0, atol=2e-10)
    np.testing.assert_allclose([[r["fus_auroc"], r["fus_auprc"]] for r in base], g["metrics_fus"][0, :, 2:], rtol=0, atol=1e-10)
    assert s["audit"] == {"same_subject": int(g["shuffle"][0]), "total": int(g["shuffle"][1])}


def test_summarise_bootstrap_equals_the_references():
    g, s = golden(), _summary()
    boot = s["bootstrap"]
    assert [(r["condition"], r["metric"]) for r in boot] == [(c, m) for c in CONDITIONS[1:] for m in ("AUROC", "AUPRC")]
    got = np.array([[r["mean_delta"], r["ci_low"], r["ci_high"], r["n_valid"]] for r in boot]).reshape(4, 2, 4)
    want = g["bootstrap"]
    print("n_valid:", got[:, :, 3].astype(int).tolist(), f"largest deviation {np.abs(got - want).max():.3e} (bound 1e-10)")
    assert np.array_equal(got[:, :, 3], want[:, :, 3])
    assert ((want[:, :, 3] > 0) & (want[:, :, 3] < s["n_boot"])).any()                    # some replicates hold one class only
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)


def test_summarise_sensitivity_and_entropy_equal_the_references(capsys):
    g, s = golden(), _summary()
    got = np.array([[r["mean_abs_dp_fus"], r["corr_fus"], r["mean_abs_dp_ts"]] for r in s["sensitivity"]])
    want = g["sens"][:, 0, :]                                                             # the report's label 0
    entropy = np.array([r["mean_entropy"] for r in s["entropy"]["per_label"]])
    print(f"sensitivity {np.abs(got - want).max():.3e}, entropy {np.abs(entropy - g['entropy']).max():.3e} (bound 1e-5)")
    assert [r["condition"] for r in s["sensitivity"]] == list(CONDITIONS[1:]) and all(r["max_abs_d_img"] == 0.0 for r in s["sensitivity"])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    np.testing.assert_allclose(entropy, g["entropy"], rtol=0, atol=1e-5)
    assert s["entropy"]["axis_size"] == int(g["cfg"][3])
    capsys.readouterr()
    _dtu().print_results(s, attention_axis="time tokens")
    text = capsys.readouterr().out
    for needle in ("[1] Original checkpoint under FULL input", "[2] Fusion logits under counterfactual TS inputs", "[3] Sensitivity to TS corruption",
                   "[4] Full-condition TS attention (time tokens, N=24)", "Cross-patient shuffle audit: same-subject pairs=3/240 (1.2500%)",
                   "[5] Main label (idx 0) subject-cluster paired bootstrap (200 replicates)"):
        assert needle in text, needle


def test_single_class_replicates_return_the_references_nan_tuple():
    dtu = _dtu()
    subject_ids = np.array([1, 1, 2, 3, 3, 4])
    y = np.zeros(6)                                                                       # every replicate holds one class
    valid = np.array([True, True, False, True, True, True])
    p_full, p_abl = np.linspace(0.1, 0.9, 6), np.linspace(0.9, 0.1, 6)
    for metric in ("AUROC", "AUPRC"):
        out = dtu.cluster_bootstrap_delta(subject_ids, y, valid, p_full, p_abl, metric, 25, 3)
        assert out[3] == 0 and isinstance(out[3], int) and all(np.isnan(v) for v in out[:3])
    none_valid = dtu.cluster_bootstrap_delta(subject_ids, y, np.zeros(6, bool), p_full, p_abl, "AUROC", 5, 3)
    assert none_valid[3] == 0 and np.isnan(none_valid[0])
    assert dtu.cluster_bootstrap_delta(subject_ids, y, valid, p_full, p_abl, "AUROC", 0, 3)[3] == 0
    y[[0, 3]] = 1.0                                                                       # two classes: replicates count again
    mean, lo, hi, n = dtu.cluster_bootstrap_delta(subject_ids, y, valid, p_full, p_abl, "AUROC", 25, 3)
    assert 0 < n <= 25 and lo <= mean <= hi
    with pytest.raises(ValueError, match="metric"):
        dtu.cluster_bootstrap_delta(subject_ids, y, valid, p_full, p_abl, "BCE", 5, 3)
    big = 16385                                                                           # one subject with more rows than the metrics kernel sorts
    with pytest.raises(ValueError, match="METRICS_MAX_LEN"):
        dtu.cluster_bootstrap_delta(np.zeros(big, np.int64), np.zeros(big), np.ones(big, bool), np.zeros(big), np.zeros(big), "AUROC", 2, 0)


# ------------------------------------------------------------------------------------------------------------------------------
def _teacher_args(tmp, perceiver_type):
    from multimodal_edema_prediction_amd import train_synthetic
    head = os.path.join(str(tmp), "cxr_head.pt")
    torch.save(cxr_head_state(), head)
    return train_synthetic.parse_args(["teacher", "--ckpt_dir", str(tmp), "--perceiver_type", perceiver_type, "--n_timesteps", "32",
                                       "--n_vars", "16", "--d_static", "8", "--n_train", "8", "--n_val", "40", "--n_test", "40",
                                       "--pretrained_cxr_head_ckpt", head, "--perceiver_dropout", "0.0", "--head_dropout", "0.0",
                                       "--freeze_duett"])


def _batches(B, n, subjects):
    from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch
    cfg = CohortCfg(n_timesteps=32, n_vars=16, d_static=8, image_size=224, n_labels=7, seed=1234)
    out = []
    for i in range(n):
        batch = make_batch(cfg, 100 + i * B, B, mode="teacher")
        batch["_subject_id"] = torch.tensor(subjects, dtype=torch.long)
        out.append(batch)
    return out


@pytest.mark.parametrize("perceiver_type", ["dual", "dual_patch"])
def test_collect_predictions_equals_the_public_path(tmp_path, perceiver_type):
    from multimodal_edema_prediction_amd import train_synthetic
    dtu = _dtu()
    seed, subjects = 2026, [1, 1, 2, 3]
    torch.manual_seed(0)
    teacher = train_synthetic.build_teacher(_teacher_args(tmp_path, perceiver_type), torch.device(DEV)).eval()
    loader = _batches(4, 2, subjects)
    calls = []
    encoder_entry = "forward" if perceiver_type == "dual" else "forward_bf16"
    original = getattr(teacher.cxr, encoder_entry)

    def counted(*a, **k):
        calls.append(1)
        return original(*a, **k)

    setattr(teacher.cxr, encoder_entry, counted)
    got = dtu.collect_predictions(teacher, loader, torch.device(DEV), perceiver_type, seed)
    assert len(calls) == len(loader)                                                      # the image encoder ran once per batch
    delattr(teacher.cxr, encoder_entry)
    assert set(got) == {"fus", "ts", "img", "y", "mask", "subject_ids", "attention", "shuffle_same_subject", "shuffle_total"}
    want = {"fus": {c: [] for c in CONDITIONS}, "ts": {c: [] for c in CONDITIONS}, "img": {c: [] for c in CONDITIONS}, "attention": []}
    same = 0
    with torch.no_grad():
        for batch_idx, batch in enumerate(loader):
            rng = np.random.default_rng(seed + 10007 * batch_idx)
            perm = dtu.different_subject_permutation(np.array(subjects), rng)
            same += int(np.sum(np.array(subjects)[perm] == np.array(subjects)))
            tperms = dtu.time_permutations([32] * 4, rng)
            pixels = batch["pixel_values"].to(DEV)
            for cond, (x_ts, x_static, bin_ends) in host_conditions(batch["x_ts"], batch["x_static"], batch["bin_ends"], perm, tperms).items():
                out = teacher(x_ts, x_static, bin_ends, pixels, return_attn=(cond == "full"))
                want["fus"][cond].append(out["fusion_logits"].float())
                want["ts"][cond].append(out["ts_logits"].float())
                want["img"][cond].append(out["img_logits"].float())
                if cond == "full":
                    want["attention"].append(out["ts_attn"].float())
    for cond in CONDITIONS:
        for half in ("fus", "ts"):
            g = got[half][cond]
            assert g.dtype == torch.float32 and g.is_cuda and g.shape == (8, 7)
            assert torch.equal(g, torch.cat(want[half][cond])), (half, cond)
    assert torch.equal(got["img"], torch.cat(want["img"]["full"]))
    assert got["attention"].shape == (8, 7, 32) and torch.equal(got["attention"], torch.cat(want["attention"]))
    assert torch.equal(got["y"], torch.cat([b["y_multi"] for b in loader]).to(DEV)) and got["mask"].is_cuda
    assert got["subject_ids"].tolist() == subjects * 2
    assert got["shuffle_same_subject"] == same and got["shuffle_total"] == 8
    for cond in ("patient_shuffle", "time_reverse", "time_permute"):                       # the corruptions reach the logits
        assert not torch.equal(got["ts"][cond], got["ts"]["full"]), cond


def test_main_writes_the_references_archive(tmp_path, capsys):
    from multimodal_edema_prediction_amd import checkpoint, residual_by_confidence, train_synthetic
    dtu = _dtu()
    args = _teacher_args(tmp_path, "dual")
    torch.manual_seed(0)
    teacher = train_synthetic.build_teacher(args, torch.device(DEV))
    ckpt = os.path.join(str(tmp_path), "best.pt")
    checkpoint.save_ckpt(ckpt, teacher, argparse.Namespace(state_dict=lambda: {}), 1, 0.5, args)
    npz = str(tmp_path / "out" / "temporal_usage.npz")
    result = dtu.main(["--teacher_ckpt", ckpt, "--split", "val", "--batch_size", "8", "--num_workers", "0", "--bootstrap", "20",
                       "--seed", "5", "--output_npz", npz])
    text = capsys.readouterr().out
    assert "perceiver_type=dual" in text and "[5] Main label (idx 0) subject-cluster paired bootstrap (20 replicates)" in text
    assert "Cross-patient shuffle audit: same-subject pairs=" in text and f"saved raw predictions: {npz}" in text
    assert len(result["summary"]["bootstrap"]) == 8 and result["summary"]["audit"]["total"] == 40
    with np.load(npz) as z:
        assert set(z.files) == {"subject_ids", "labels", "y", "mask", "img_full", "ts_attention_full"} | {
            f"{h}_{c}" for h in ("fus", "ts") for c in CONDITIONS}
        assert z["subject_ids"].shape == (40,) and z["labels"].shape == (7,) and z["ts_attention_full"].shape == (40, 7, 32)
        assert all(z[k].shape == (40, 7) and z[k].dtype == np.float32 for k in z.files if k not in ("subject_ids", "labels", "ts_attention_full"))
        ids = z["subject_ids"]
        assert sorted(ids.tolist()) == sorted(((10_000_000 + i) // 2) for i in range(40))  # two stays per subject, the whole split, shuffled
        assert ids.tolist() != sorted(ids.tolist())
    table = residual_by_confidence.main(["--input_npz", npz])
    assert len(table) == 7 and "Label: label_edema" in capsys.readouterr().out
