#!/usr/bin/env python3
"""Golden fixture for the temporal-usage diagnostics (analysis/diagnose_temporal_usage.py and its consumer
analysis/residual_by_confidence.py): runs the REFERENCE'S OWN functions (`_different_subject_permutation`, `_time_permuted`, `_prob`,
`_metrics_by_label`, `_cluster_bootstrap_delta`, and `residual_by_confidence.main`; stubs as in make_golden.py) and stores numbers and
recorded text only in tests/golden/temporal_usage.npz.

At the reference's HEAD the diagnostics module does not import: it names `DualPathologyPerceiver`, which the model file has commented
out.  The model file is imported first and given a placeholder attribute of that name; none of the functions used here touches it.

Stored
  draws     four batches (subject ids, series lengths, batch index): the permutation `_different_subject_permutation` returns from
            `default_rng(seed + 10007 * batch_idx)` and, drawn next from the same generator, the time permutations of `_time_permuted`
            (read off series whose rows are numbered).  [1, 1, 1, 2, 3] reaches the cyclic fallback with one same-subject pair; one
            batch has a single sample; one is ragged.
  pred      a synthetic `collect_predictions` result: N = 240 rows of 120 subjects (1 - 3 rows each), K = 3 labels, C = 5 conditions,
            S = 24 attention weights, ~85 % of the labels known, logits on a grid of 1/64 inside (-6, 6) (so some are exactly equal,
            and distinct ones give distinct fp32 probabilities: asserted), with everything the report derives from it:
            `_metrics_by_label` of img / ts / every fusion condition, sections [3] and [4] (the expressions of `_print_results`, which
            prints but does not return them, on the reference's `_prob`), and `_cluster_bootstrap_delta` for the 4 conditions x 2
            metrics at n_boot = 200.  Label 0 has two known positives, so some replicates hold one class: 0 < n_valid < n_boot
            (asserted).
  text      the stdout of the reference's `residual_by_confidence.main()` on the archive built from that `pred`.
Build container only.

Usage:  python tests/golden/make_golden_temporal_usage.py [output directory]"""
from __future__ import annotations

import contextlib
import io
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

N, K, C, S, N_SUBJECTS, N_BOOT, SEED, DATA_SEED = 240, 3, 5, 24, 120, 200, 2026, 7
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
DRAW_CASES = (                       # (subject ids, series lengths, batch index)
    ([1, 1, 2, 3], [32, 32, 32, 32], 0),
    ([1, 1, 1, 2, 3], [50, 64, 50, 64, 50], 1),
    ([4, 5, 6], [5, 9, 3], 2),
    ([7], [1], 3),
)


def import_reference():
    install_stubs()
    sys.path.insert(0, REF)
    for name in ("tqdm", "tqdm.auto"):                       # progress bars only
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                m = types.ModuleType(name)
                m.tqdm = lambda it, **kw: it
                sys.modules[name] = m
    import models.main_architecture_duett as model_file
    if not hasattr(model_file, "DualPathologyPerceiver"):
        model_file.DualPathologyPerceiver = type("DualPathologyPerceiver", (), {})      # placeholder: commented out at HEAD
    import analysis.diagnose_temporal_usage as ref
    import analysis.residual_by_confidence as ref_residual
    return ref, ref_residual


def synth_pred(rng):
    rows_per_subject = np.array([1, 2, 3] * (N_SUBJECTS // 3))
    assert rows_per_subject.sum() == N
    subject_ids = rng.permutation(np.repeat(1000 + np.arange(N_SUBJECTS), rows_per_subject))
    grid = lambda a: np.clip(np.round(a * 64.0) / 64.0, -5.984375, 5.984375).astype(np.float32)  # noqa: E731
    signal = rng.standard_normal((N, K))
    img = grid(1.3 * signal + 0.8 * rng.standard_normal((N, K)))
    ts_full = 0.9 * signal + 0.9 * rng.standard_normal((N, K))
    noise = {"full": 0.0, "patient_shuffle": 1.5, "ts_shuffle": 1.2, "time_reverse": 0.4, "time_permute": 0.7}
    ts, fus = {}, {}
    for cond, s in noise.items():
        t = ts_full if s == 0.0 else (1.0 - 0.4 * s) * ts_full + s * rng.standard_normal((N, K))
        ts[cond] = grid(t)
        fus[cond] = grid(img + 0.6 * t)
    y = (rng.random((N, K)) < 1.0 / (1.0 + np.exp(-(signal - 0.8)))).astype(np.float32)
    mask = (rng.random((N, K)) < 0.85).astype(np.float32)
    # label 0: exactly two known positives, in two different subjects
    y[:, 0] = 0.0
    known0 = np.flatnonzero(mask[:, 0] > 0)
    order = known0[np.argsort(-signal[known0, 0])]
    first = order[0]
    second = next(i for i in order[1:] if subject_ids[i] != subject_ids[first])
    y[[first, second], 0] = 1.0
    attention = rng.random((N, K, S)) ** 3
    attention = (attention / attention.sum(-1, keepdims=True)).astype(np.float32)
    attention[:, 1, :] = np.float32(1.0 / S)                                       # a uniform label: entropy 1
    return {"fus": fus, "ts": ts, "img": img, "y": y, "mask": mask, "subject_ids": subject_ids.astype(np.int64), "attention": attention,
            "shuffle_same_subject": 3, "shuffle_total": N}


def main(out_dir=HERE):
    ref, ref_residual = import_reference()
    from sklearn.metrics import average_precision_score, roc_auc_score
    assert tuple(ref.CONDITIONS) == ("full", "patient_shuffle", "ts_shuffle", "time_reverse", "time_permute")
    out = {"conditions": np.array(ref.CONDITIONS), "labels": np.array(LABELS), "cfg": np.array([N, K, C, S, N_SUBJECTS, N_BOOT, SEED])}

    # ---- draws
    out["draws_n"] = np.array(len(DRAW_CASES))
    for i, (subjects, lengths, batch_idx) in enumerate(DRAW_CASES):
        rng = np.random.default_rng(SEED + 10007 * batch_idx)
        subjects = np.asarray(subjects, dtype=np.int64)
        perm = ref._different_subject_permutation(subjects, rng)
        numbered = tuple(torch.arange(n, dtype=torch.float32).view(n, 1) for n in lengths)
        tperm = [x[:, 0].numpy().astype(np.int64) for x in ref._time_permuted(numbered, rng)]
        assert all(sorted(t.tolist()) == list(range(n)) for t, n in zip(tperm, lengths))
        out.update({f"draws_{i}_subjects": subjects, f"draws_{i}_lengths": np.asarray(lengths), f"draws_{i}_batch_idx": np.array(batch_idx),
                    f"draws_{i}_perm": np.asarray(perm, dtype=np.int64), f"draws_{i}_tperm": np.concatenate(tperm),
                    f"draws_{i}_same_subject": np.array(int(np.sum(subjects[perm] == subjects)))})
    assert int(out["draws_1_same_subject"]) == 1 and np.array_equal(out["draws_1_perm"], np.roll(np.arange(5), 2)), "the cyclic fallback case"
    assert int(out["draws_0_same_subject"]) == 0

    # ---- the synthetic pred and everything the report derives from it
    pred = synth_pred(np.random.default_rng(DATA_SEED))
    for cond in ref.CONDITIONS:
        out[f"fus_{cond}"], out[f"ts_{cond}"] = pred["fus"][cond], pred["ts"][cond]
    out.update(img=pred["img"], y=pred["y"], mask=pred["mask"], subject_ids=pred["subject_ids"], attention=pred["attention"],
               shuffle=np.array([pred["shuffle_same_subject"], pred["shuffle_total"]]))
    n_equal = 0
    for name, z in [("img", pred["img"])] + [(f"{h}_{c}", pred[h][c]) for h in ("fus", "ts") for c in ref.CONDITIONS]:
        assert z.dtype == np.float32 and np.abs(z).max() < 6.0
        p = ref._prob(z)
        assert p.dtype == np.float32
        for k in range(K):
            assert np.unique(p[:, k]).size == np.unique(z[:, k]).size, f"{name}[{k}]: distinct logits must give distinct fp32 probabilities"
            assert np.diff(np.unique(p[:, k].astype(np.float64))).min() > 1e-6
            n_equal += N - np.unique(z[:, k]).size
    assert n_equal > 0, "the fixture wants some exactly equal logits"

    def table(rows):
        return np.array([[r["n"], r["pos_frac"], r["auroc"], r["auprc"]] for r in rows], dtype=np.float64)

    y, mask = pred["y"], pred["mask"]
    out["metrics_img"] = table(ref._metrics_by_label(pred["img"], y, mask, LABELS))
    out["metrics_ts_full"] = table(ref._metrics_by_label(pred["ts"]["full"], y, mask, LABELS))
    out["metrics_fus"] = np.stack([table(ref._metrics_by_label(pred["fus"][c], y, mask, LABELS)) for c in ref.CONDITIONS])
    assert np.isfinite(out["metrics_fus"]).all()
    # section [3], for EVERY label (the report prints label 0): mean |dp fus|, corr fus, mean |dp ts|
    sens = np.zeros((C - 1, K, 3))
    for ci, cond in enumerate(ref.CONDITIONS[1:]):
        for k in range(K):
            p_full_fus, p_full_ts = ref._prob(pred["fus"]["full"][:, k]), ref._prob(pred["ts"]["full"][:, k])
            p_cond_fus, p_cond_ts = ref._prob(pred["fus"][cond][:, k]), ref._prob(pred["ts"][cond][:, k])
            sens[ci, k] = (np.mean(np.abs(p_full_fus - p_cond_fus)), np.corrcoef(p_full_fus, p_cond_fus)[0, 1],
                           np.mean(np.abs(p_full_ts - p_cond_ts)))
    out["sens"] = sens
    # section [4]
    attn = pred["attention"]
    normalized_attn = attn / np.clip(attn.sum(axis=-1, keepdims=True), 1e-12, None)
    entropy = -(normalized_attn * np.log(np.clip(normalized_attn, 1e-12, None))).sum(axis=-1)
    entropy = entropy / max(math.log(normalized_attn.shape[-1]), 1e-12)
    out["entropy"] = np.array([entropy[:, k].mean() for k in range(K)], dtype=np.float64)
    # section [5]
    valid, y0 = mask[:, 0].astype(bool), y[:, 0]
    p_full = ref._prob(pred["fus"]["full"][:, 0])
    boot = np.zeros((C - 1, 2, 4))
    for ci, cond in enumerate(ref.CONDITIONS[1:], start=1):
        pc = ref._prob(pred["fus"][cond][:, 0])
        for mi, fn in enumerate((roc_auc_score, average_precision_score)):
            boot[ci - 1, mi] = ref._cluster_bootstrap_delta(pred["subject_ids"], y0, valid, p_full, pc, fn, n_boot=N_BOOT, seed=SEED + 1000 * ci + mi)
    out["bootstrap"] = boot
    assert ((boot[:, :, 3] > 0) & (boot[:, :, 3] < N_BOOT)).any(), boot[:, :, 3]
    print("n_valid per condition x metric:\n", boot[:, :, 3])

    # ---- recorded text of the consumer
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pred.npz")
        payload = {"subject_ids": pred["subject_ids"], "labels": np.asarray(LABELS), "y": y, "mask": mask, "img_full": pred["img"],
                   "ts_attention_full": attn}
        for cond in ref.CONDITIONS:
            payload[f"fus_{cond}"], payload[f"ts_{cond}"] = pred["fus"][cond], pred["ts"][cond]
        np.savez_compressed(path, **payload)
        argv, sys.argv = sys.argv, ["residual_by_confidence", "--input_npz", path]
        buffer = io.StringIO()
        try:
            with contextlib.redirect_stdout(buffer):
                ref_residual.main()
        finally:
            sys.argv = argv
    out["residual_stdout"] = np.array(buffer.getvalue())
    print(buffer.getvalue())

    path = os.path.join(out_dir, "temporal_usage.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote temporal_usage.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
