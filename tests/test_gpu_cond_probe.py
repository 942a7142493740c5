"""GPU: the conditional-information probe end to end on the reference's fixture (tests/golden/cond_probe.npz: the reference's own
functions on one seeded problem, tests/golden/make_golden_cond_probe.py).  The fixture holds two restatements of the reference's loop:
R, the reference as shipped (L-BFGS stopped at sklearn's tol = 1e-4, on fp32 features), and T, the same pipeline solved to
tol = 1e-12 (the optimum of the reference's own objective).

Bounds
  fitted parameters vs T   10 ||H^-1||_2 (1e-10 + max|g_T|) per fit, from the values the fixture stores (tests/test_cond_probe_refs_cpu.py
                           derives it): ~1e-8.
  row values vs T          1e-8: a parameter shift of ~1e-9 moves a probability by as much, a BCE (a mean) by no more; AUROC / AUPRC
                           are step functions of the ORDER of the probabilities, which cannot change (the fixture asserts distinct T
                           probabilities >= 1e-6 apart); percentiles and means of such values inherit the bound.
  row values vs R          |dev - R| <= 2 |T - R| + 1e-8 per value: the reference's own optimiser slack, measured between two
                           reference-side runs only, bounds how far its optimum may sit from what it printed.
  per-replicate metrics    1e-10 on the stored T probabilities (the kernel tests' bound for the metrics kernel).
Every test prints its figures."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from cond_probe_refs import FIT_NAMES, PROBE_NAMES, fit_bound, golden, split_of
from raw_probe_refs import binary_metrics_ref
from tests_dual_common import cxr_head_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 3
_state = {}


def _cip():
    from multimodal_edema_prediction_amd import conditional_information_probe
    return conditional_information_probe


def _data(split):
    if split not in _state:
        _state[split] = {k: torch.as_tensor(np.array(v), device=DEV) for k, v in split_of(golden(), split).items()}
    return _state[split]


def _cfg():
    g = golden()
    c = g["cfg"]
    return dict(logit_c=float(g["logit_c"]), token_c=float(g["token_c"]), bootstrap=int(c[6]), perm_repeats=int(c[7]), perm_bins=int(c[8]),
                seed=int(c[5]))


def _run():
    if "run" not in _state:
        _state["run"] = _cip().run_probe(_data("train"), _data("test"), [str(s) for s in golden()["labels"]], (0, 1, 2), verbose=False,
                                         **_cfg())
    return _state["run"]


def _known(split, k):
    g = golden()
    return np.flatnonzero(g[f"{split}_mask"][:, k].astype(bool))


def test_fit_probes_reaches_the_reference_optimum_in_one_call():
    g, cip = golden(), _cip()
    problems = [(k, name) for k in range(K) for name in FIT_NAMES]
    fits = cip.fit_probes(_data("train"), problems, logit_c=float(g["logit_c"]), token_c=float(g["token_c"]))
    assert len(fits) == 12
    for (k, name), m in zip(problems, fits):
        p = f"T_{k}_{name}_"
        bound = fit_bound(g, k, name)
        dev = max(np.abs(m.coef - g[p + "coef"]).max(), abs(m.intercept - float(g[p + "intercept"])))
        ref_gap = max(np.abs(g["R" + p[1:] + "coef"] - g[p + "coef"]).max(), abs(float(g["R" + p[1:] + "intercept"]) - float(g[p + "intercept"])))
        print(f"{p}: {m.n_iter} Newton iterations, max|g| {m.max_gradient:.2e}, |theta - T| {dev:.2e} (bound {bound:.2e}; |R - T| {ref_gap:.2e})")
        assert (m.label_index, m.probe) == (k, name) and m.C == (float(g["token_c"]) if name == "token_linear" else float(g["logit_c"]))
        assert dev <= bound
        assert 1 <= m.n_iter <= cip.MAX_ITER and m.max_gradient <= cip.GTOL
        np.testing.assert_allclose(m.mean, g[p + "mean"], rtol=1e-10, atol=1e-10)            # the moments kernel's bound
        np.testing.assert_allclose(m.scale, g[p + "scale"], rtol=1e-10, atol=1e-10)
    with pytest.raises(RuntimeError, match="max_iter"):
        cip.fit_probes(_data("train"), problems[:4], max_iter=1)


def test_run_probe_against_the_reference_at_its_optimum():
    g = golden()
    rows, summary, archive = _run()
    cip = _cip()
    assert [r["label"] for r in rows] == [str(s) for s in g["row_label"]] and [r["probe"] for r in rows] == [str(s) for s in g["row_probe"]]
    assert all(list(r) == [str(k) for k in g["row_keys"]] for r in rows)
    numeric = [str(k) for k in g["row_numeric_keys"]]
    got = np.array([[float(r[k]) for k in numeric] for r in rows])
    dev_T = np.abs(got - g["T_rows"])
    worst = np.unravel_index(np.nanargmax(dev_T), dev_T.shape)
    print(f"run_probe vs T: largest deviation {np.nanmax(dev_T):.3e} at row {worst[0]} ({numeric[worst[1]]}); bound 1e-8")
    assert np.array_equal(np.isnan(got), np.isnan(g["T_rows"]))
    assert np.nanmax(dev_T) <= 1e-8
    assert [r["evidence"] for r in rows] == [str(e) for e in g["evidence"]]
    for k in range(K):
        for name in PROBE_NAMES:
            stored = archive[f"{cip._slug(str(g['labels'][k]))}_{name}_probability"]
            assert stored.dtype == np.float32 and np.abs(stored - g[f"T_{k}_{name}_test_prob"]).max() <= 1e-7     # fp32 rounding of p <= 1
    assert set(archive) >= {"test_img_logits", "test_ts_logits", "test_fusion_logits", "test_y", "test_mask"}
    assert list(summary["labels"]) == [str(s) for s in g["labels"]] and len(summary["fits"]) == 12
    assert summary["labels"]["label_edema"]["probes"]["token_linear"] is rows[2]
    print("Newton iterations per fit:", [f["n_iter"] for f in summary["fits"]])


def test_run_probe_against_the_reference_as_shipped():
    g = golden()
    rows, _, _ = _run()
    numeric = [str(k) for k in g["row_numeric_keys"]]
    got = np.array([[float(r[k]) for k in numeric] for r in rows])
    dev_R, slack = np.abs(got - g["R_rows"]), np.abs(g["T_rows"] - g["R_rows"])
    print(f"run_probe vs R: largest deviation {np.nanmax(dev_R):.3e}; the reference's distance from its own optimum {np.nanmax(slack):.3e}")
    assert (dev_R <= 2 * slack + 1e-8)[~np.isnan(dev_R)].all()
    assert [r["evidence"] for r in rows] == [str(e) for e in g["evidence"]]


def test_per_replicate_metrics_equal_the_references():
    g, cip = golden(), _cip()
    from multimodal_edema_prediction_amd.probe_stats import resampled_binary_metrics
    d = lambda a: torch.as_tensor(np.array(a), device=DEV)  # noqa: E731
    y_test = g["test_y"][_known("test", 0), 0].astype(np.uint8)
    n, idx = len(y_test), g["boot_idx"].astype(np.int32)
    offsets = d(np.arange(0, (len(idx) + 1) * n, n, dtype=np.int64))
    for name, want in (("image_cal", g["boot_metrics_base"]), ("token_linear", g["boot_metrics_probe"])):
        got = resampled_binary_metrics(d(y_test), d(g[f"T_0_{name}_test_prob"][None]), d(idx.reshape(-1)), offsets, n).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)
    # the permutation replicates, rebuilt on the device from the score parts of T's model
    p = "T_0_token_linear_"
    model = cip.FittedProbe(0, "token_linear", g[p + "mean"], g[p + "scale"], g[p + "coef"], float(g[p + "intercept"]), 1.0, 0, 0.0)
    parts = cip.score_parts(_data("test"), [model])[0]
    np.testing.assert_allclose(parts["score"].cpu().numpy(), g[p + "test_score"], rtol=1e-9, atol=1e-9)
    known = d(_known("test", 0))
    prob = cip.permuted_probabilities(model, parts, _data("test")["img"][known, 0], _data("test")["ts"][known, 0], g["perm_idx"])
    got = resampled_binary_metrics(d(y_test), prob).cpu().numpy()
    print(f"permutation replicates: largest deviation {np.abs(got - g['perm_metrics']).max():.3e}")
    np.testing.assert_allclose(got, g["perm_metrics"], rtol=1e-10, atol=1e-10)
    # the interaction column img_i * ts_pi(i): against the host model on explicitly rebuilt features
    p = "T_0_logit_interaction_"
    model = cip.FittedProbe(0, "logit_interaction", g[p + "mean"], g[p + "scale"], g[p + "coef"], float(g[p + "intercept"]), 100.0, 0, 0.0)
    parts = cip.score_parts(_data("test"), [model])[0]
    img, ts = g["test_img"][_known("test", 0), 0], g["test_ts"][_known("test", 0), 0]
    prob = cip.permuted_probabilities(model, parts, d(img), d(ts), g["perm_idx"][:5]).cpu().numpy()
    for r in range(5):
        sh = ts[g["perm_idx"][r]]
        want, _ = model.predict(np.column_stack([img, sh, img * sh]))
        np.testing.assert_allclose(prob[r], want, rtol=1e-12, atol=1e-12)


def test_single_class_replicates_leave_the_rank_metrics_only():
    cip = _cip()
    y = np.array([0, 1, 0, 1, 1, 0])
    base, probe = np.array([0.2, 0.6, 0.4, 0.7, 0.5, 0.3]), np.array([0.1, 0.8, 0.3, 0.9, 0.6, 0.2])
    index = np.array([[0, 1, 2, 3, 4, 5], [0, 2, 5, 5, 0, 2], [1, 3, 4, 4, 1, 3], [5, 4, 3, 2, 1, 0], [0, 0, 1, 1, 2, 3]])    # 2 single-class
    got = cip.bootstrap_differences(y, base, probe, 5, 0, index=index)
    mb = np.array([binary_metrics_ref(y[i], base[i]) for i in index])
    mp = np.array([binary_metrics_ref(y[i], probe[i]) for i in index])
    both = np.array([len(np.unique(y[i])) == 2 for i in index])
    assert both.tolist() == [True, False, False, True, True]
    want = {}
    for name, v in (("bce_gain", mb[:, 0] - mp[:, 0]), ("auroc_gain", (mp[:, 1] - mb[:, 1])[both]), ("auprc_gain", (mp[:, 2] - mb[:, 2])[both])):
        want[f"{name}_ci_low"], want[f"{name}_ci_high"] = np.percentile(v, [2.5, 97.5])
    assert list(got) == list(want)
    np.testing.assert_allclose(list(got.values()), list(want.values()), rtol=1e-10, atol=1e-10)
    empty = cip.bootstrap_differences(y, base, probe, 0, 0)
    assert all(np.isnan(v) for v in empty.values()) and list(empty) == list(want)


def test_cases_that_skip_or_raise(capsys):
    g, cip = golden(), _cip()
    labels = [str(s) for s in g["labels"]]
    test = dict(_data("test"))
    test["y"] = test["y"].clone()
    test["y"][:, 1] = 0.0                                                 # label 1 has one class in the test split: skipped
    rows, summary, _ = cip.run_probe(_data("train"), test, labels, (1, 2), bootstrap=5, perm_repeats=3, logit_c=100.0, token_c=1.0)
    assert "skip label_cardiomegaly: one split has only one class" in capsys.readouterr().out
    assert {r["label"] for r in rows} == {"label_effusion"} and list(summary["labels"]) == ["label_effusion"]
    train = dict(_data("train"))
    train["y"] = torch.ones_like(train["y"])
    with pytest.raises(ValueError, match="only one class"):
        cip.fit_probes(train, [(0, "logit_add")])
    with pytest.raises(ValueError, match="Unknown probe_name"):
        cip.fit_probes(_data("train"), [(0, "nope")])
    n = 16385                                                             # more known test rows than the metrics kernel sorts
    rng = np.random.default_rng(0)
    big = {"img": torch.zeros((n, 1), device=DEV), "ts": torch.zeros((n, 1), device=DEV), "fus": torch.zeros((n, 1), device=DEV),
           "token": torch.zeros((n, 1, 2), device=DEV), "y": torch.as_tensor((rng.random((n, 1)) < 0.5).astype(np.float32), device=DEV),
           "mask": torch.ones((n, 1), device=DEV)}
    with pytest.raises(ValueError, match="METRICS_MAX_LEN"):
        cip.run_probe(big, big, ["label_x"], (0,))


class _FakeTeacher(torch.nn.Module):
    def __init__(self, drop=None, rank2=False):
        super().__init__()
        self.drop, self.rank2 = drop, rank2

    def forward(self, x_ts, x_static, bin_ends, pixel_values, return_attn=False):
        B = len(x_ts)
        out = {"img_logits": torch.zeros(B, 2, device=DEV), "ts_logits": torch.zeros(B, 2, device=DEV),
               "fusion_logits": torch.zeros(B, 2, device=DEV), "ts_tokens": torch.zeros((B, 4) if self.rank2 else (B, 2, 4), device=DEV)}
        if self.drop:
            del out[self.drop]
        return out


def _batches(T, V, DS, K_, B, n):
    from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch
    cfg = CohortCfg(n_timesteps=T, n_vars=V, d_static=DS, image_size=224, n_labels=K_, seed=1234)
    return [make_batch(cfg, 100 + i * B, B, mode="teacher") for i in range(n)]


def test_gather_raises_as_the_reference_does():
    cip = _cip()
    loader = _batches(8, 4, 2, 2, 2, 1)
    with pytest.raises(RuntimeError, match="missing=\\['ts_tokens'\\]"):
        cip.gather(_FakeTeacher(drop="ts_tokens"), loader, DEV)
    with pytest.raises(ValueError, match="Expected pathology-wise ts_tokens"):
        cip.gather(_FakeTeacher(rank2=True), loader, DEV)
    with pytest.raises(RuntimeError, match="no batches"):
        cip.gather(_FakeTeacher(), [], DEV)
    out = cip.gather(_FakeTeacher(), loader, DEV)
    assert set(out) == {"img", "ts", "fus", "token", "y", "mask"} and out["token"].shape == (2, 2, 4) and out["y"].is_cuda


def _teacher_args(tmp, perceiver_type):
    from multimodal_edema_prediction_amd import train_synthetic
    head = os.path.join(str(tmp), "cxr_head.pt")
    torch.save(cxr_head_state(), head)
    return train_synthetic.parse_args(["teacher", "--ckpt_dir", str(tmp), "--perceiver_type", perceiver_type, "--n_timesteps", "32",
                                       "--n_vars", "16", "--d_static", "8", "--n_train", "8", "--n_val", "40", "--n_test", "40",
                                       "--pretrained_cxr_head_ckpt", head, "--perceiver_dropout", "0.0", "--head_dropout", "0.0",
                                       "--freeze_duett"])


@pytest.mark.parametrize("perceiver_type", ["dual", "dual_patch"])
def test_gather_equals_direct_forwards(tmp_path, perceiver_type):
    from multimodal_edema_prediction_amd import engine, train_synthetic
    cip = _cip()
    torch.manual_seed(0)
    teacher = train_synthetic.build_teacher(_teacher_args(tmp_path, perceiver_type), torch.device(DEV)).eval()
    loader = _batches(32, 16, 8, 7, 3, 2)
    got = cip.gather(teacher, loader, torch.device(DEV))
    want = {k: [] for k in got}
    with torch.no_grad():
        for batch in loader:
            b = engine._move_lists(batch, DEV)
            out = teacher(b["x_ts"], b["x_static"], b["bin_ends"], b["pixel_values"], return_attn=True)
            for k, v in zip(("img", "ts", "fus", "token", "y", "mask"), (out["img_logits"], out["ts_logits"], out["fusion_logits"],
                                                                        out["ts_tokens"], b["y_multi"], b["y_multi_mask"])):
                want[k].append(v.float())
    for k in got:
        assert got[k].dtype == torch.float32 and got[k].is_cuda and got[k].is_contiguous()
        assert torch.equal(got[k], torch.cat(want[k])), k
    assert got["token"].shape == (6, 7, 256) and got["img"].shape == (6, 7)


def test_main_writes_the_references_files(tmp_path):
    from multimodal_edema_prediction_amd import checkpoint, train_synthetic
    cip = _cip()
    args = _teacher_args(tmp_path, "dual")
    torch.manual_seed(0)
    teacher = train_synthetic.build_teacher(args, torch.device(DEV))
    ckpt = os.path.join(str(tmp_path), "best.pt")
    checkpoint.save_ckpt(ckpt, teacher, argparse.Namespace(state_dict=lambda: {}), 1, 0.5, args)
    outdir = tmp_path / "out"
    result = cip.main(["--ckpt", ckpt, "--outdir", str(outdir), "--labels", "cardiomegaly", "--batch_size", "8", "--num_workers", "0",
                       "--bootstrap", "20", "--perm_repeats", "5"])
    assert sorted(os.listdir(outdir)) == ["conditional_probe.csv", "conditional_probe.json", "conditional_probe_predictions.npz"]
    header = open(outdir / "conditional_probe.csv").readline().strip().split(",")
    assert header == list(cip.ROW_KEYS) and len(result["rows"]) == 3
    summary = json.load(open(outdir / "conditional_probe.json"))
    assert {"checkpoint", "mode", "probe_train_split", "test_split", "configuration", "labels"} <= set(summary) and summary["mode"] == "dual"
    assert set(summary["labels"]["label_cardiomegaly"]) == {"n_test", "n_positive", "prevalence", "image_cal", "probes"}
    assert list(summary["labels"]["label_cardiomegaly"]["probes"]) == list(cip.PROBE_NAMES)
    with np.load(outdir / "conditional_probe_predictions.npz") as z:
        assert set(z.files) == {"test_img_logits", "test_ts_logits", "test_fusion_logits", "test_y", "test_mask"} | {
            f"label_cardiomegaly_{p}_probability" for p in cip.PROBE_NAMES}
        assert z["test_img_logits"].shape == (40, 7) and z["label_cardiomegaly_token_linear_probability"].dtype == np.float32
    with pytest.raises(SystemExit):
        cip.main(["--ckpt", ckpt, "--outdir", str(outdir), "--probe_train_split", "test"])
