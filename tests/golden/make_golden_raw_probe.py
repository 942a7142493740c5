#!/usr/bin/env python3
"""Golden fixture for the raw-trajectory conditional probe (analysis/raw_trajectory_conditional_probe.py): runs the REFERENCE'S OWN
functions (`_summarize_one_variable`, `_fit_model`, `_fit_offset_correction`, `_safe_metrics`, `_cluster_bootstrap_differences`,
`_conditional_permutation_offset`; stubs as in make_golden.py) on ONE seeded problem, restating the body of its `main()` label / block
loop (:927-1075) for one label, and stores numbers only in tests/golden/raw_probe.npz.

The problem: n_train = 240, n_test = 160 windows (two per subject), T = 24, V = 3, recent_hours = 6; un-normalised values; variable 2
never observed in some windows, single-observation windows, observed-but-NaN values; the label depends on the image logit and on the
LEVEL of variable 0 (the planted effect).  Besides the five default blocks a pure-noise block is fitted: the reference selects the
exact null candidate for it (NOISE_SEED is chosen so that it does so by more than the whole `null_tolerance`, asserted below).

Stored: the x_ts arrays, the per-(window, variable) summaries, labels / image logits / subjects, the StratifiedKFold index lists of
the calibration and of every block's correction fit, the calibration result, per block `cv_results`, `selected_l2`, weights,
`transformed_names`, test probabilities, metrics, bootstrap (200) and permutation (50) outputs; for the `level` block also the drawn
index arrays and the reference's per-replicate metrics, and (captured from inside `_fit_offset_weights`) the reference objective's
value and gradient at a fixed probe point.  Build container only.

Usage:  python tests/golden/make_golden_raw_probe.py [output directory]"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

N_TRAIN, N_TEST, T, V, RECENT = 240, 160, 24, 3, 6
VARS = ("hr", "map", "lact")
L2_GRID = (0.0001, 0.001, 0.01, 0.1, 1.0, 10.0, 100.0)
C_GRID = (0.001, 0.01, 0.1, 1.0, 10.0)
CV_FOLDS, MAX_ITER, NULL_TOL, SEED, N_BOOT, N_PERM, PERM_BINS = 5, 3000, 5e-4, 42, 200, 50, 10
BLOCKS = ("level", "trajectory", "observation", "physiologic", "all", "noise")
DATA_SEED, NOISE_SEED = 7, 100


def synth_split(rng, n):
    """[n, T, 2V] fp32 values | counts, subjects (two windows each), image logits, labels."""
    x = np.zeros((n, T, 2 * V), np.float32)
    centre, spread = np.array([85.0, 72.0, 2.2]), np.array([14.0, 11.0, 1.1])
    base = centre + spread * rng.standard_normal((n, V))
    drift = 0.04 * spread * rng.standard_normal((n, V))
    rate = np.array([0.7, 0.45, 0.12])
    for i in range(n):
        for v in range(V):
            seen = rng.random(T) < rate[v]
            cnt = np.where(seen, 1 + rng.poisson(0.6, T), 0)
            val = base[i, v] + drift[i, v] * np.arange(T) + 0.25 * spread[v] * rng.standard_normal(T)
            x[i, :, v] = np.where(seen, val, 0.0)
            x[i, :, V + v] = cnt
    never = rng.random(n) < 0.15                       # variable 2 never observed
    x[never, :, 2] = 0.0
    x[never, :, V + 2] = 0.0
    single = np.flatnonzero(rng.random(n) < 0.10)      # variable 1 observed exactly once
    for i in single:
        t = int(rng.integers(T))
        keep_v, keep_c = x[i, t, 1], max(x[i, t, V + 1], 1.0)
        x[i, :, 1] = 0.0
        x[i, :, V + 1] = 0.0
        x[i, t, 1], x[i, t, V + 1] = (keep_v if keep_v != 0 else 70.0), keep_c
    for i in np.flatnonzero(rng.random(n) < 0.10):     # an observed hour whose value is NaN
        hours = np.flatnonzero(x[i, :, V] > 0)
        if hours.size:
            x[i, hours[int(rng.integers(hours.size))], 0] = np.nan
    subjects = np.repeat(np.arange(n // 2), 2) + 1000
    image = 1.3 * rng.standard_normal(n)
    logit = -0.4 + 0.9 * image + 1.4 * (base[:, 0] - centre[0]) / spread[0]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.int64)
    return x, subjects, image.astype(np.float32), y


def main(out_dir=HERE):
    install_stubs()
    sys.path.insert(0, REF)
    import pandas as pd
    import analysis.raw_trajectory_conditional_probe as ref
    warnings.filterwarnings("ignore", message="Skipping features without any observed values")

    rng = np.random.default_rng(DATA_SEED)
    x_tr, subj_tr, img_tr, y_tr = synth_split(rng, N_TRAIN)
    x_te, subj_te, img_te, y_te = synth_split(rng, N_TEST)
    subj_te = subj_te + 5000
    noise_rng = np.random.default_rng(NOISE_SEED)
    noise_tr, noise_te = noise_rng.standard_normal((N_TRAIN, 4)), noise_rng.standard_normal((N_TEST, 4))

    def summaries(x):
        out = np.empty((x.shape[0], V, 14))
        for i in range(x.shape[0]):
            cols = {VARS[v]: x[i, :, v].astype(np.float64) for v in range(V)}
            cols.update({VARS[v] + "_count": x[i, :, V + v].astype(np.float64) for v in range(V)})
            cols["slot_idx"] = np.arange(T)
            window = pd.DataFrame(cols)
            for v in range(V):
                lv, tr, ob = ref._summarize_one_variable(window, VARS[v], VARS[v] + "_count", T, RECENT)
                out[i, v] = lv + tr + ob
        return out

    s_tr, s_te = summaries(x_tr), summaries(x_te)
    assert np.isnan(s_tr[:, 2, 0]).any() and (s_tr[:, 2, 11] == T).any()          # never observed
    assert (np.isnan(s_tr[:, 1, 5]) & ~np.isnan(s_tr[:, 1, 0])).any()             # one valid point: delta NaN, last finite

    def blocks_of(s, noise):
        level, traj, obs = (s[:, :, a:b].reshape(len(s), -1) for a, b in ((0, 5), (5, 9), (9, 14)))
        phys = np.column_stack([level, traj])
        return {"level": level, "trajectory": traj, "observation": obs, "physiologic": phys, "all": np.column_stack([phys, obs]),
                "noise": noise}

    names = {"level": tuple(f"{v}__{s}" for v in VARS for s in ref.LEVEL_STATS),
             "trajectory": tuple(f"{v}__{s}" for v in VARS for s in ref.TRAJECTORY_STATS),
             "observation": tuple(f"{v}__{s}" for v in VARS for s in ref.OBSERVATION_STATS)}
    names["physiologic"] = names["level"] + names["trajectory"]
    names["all"] = names["physiologic"] + names["observation"]
    names["noise"] = tuple(f"noise{i}" for i in range(4))
    b_tr, b_te = blocks_of(s_tr, noise_tr), blocks_of(s_te, noise_te)

    out = dict(x_train=x_tr, x_test=x_te, summary_train=s_tr, summary_test=s_te, y_train=y_tr, y_test=y_te, image_train=img_tr,
               image_test=img_te, subject_test=subj_te, noise_train=noise_tr, noise_test=noise_te,
               cfg=np.array([N_TRAIN, N_TEST, T, V, RECENT, CV_FOLDS, MAX_ITER, SEED, N_BOOT, N_PERM, PERM_BINS]),
               l2_grid=np.array(L2_GRID), c_grid=np.array(C_GRID), null_tolerance=np.array(NULL_TOL), var_names=np.array(VARS))

    # ---- image calibration (:940-954), label_index = 0 ----
    base_train, base_test = ref._design_frame(img_tr, None), ref._design_frame(img_te, None)
    base_model = ref._fit_model("logistic", base_train, y_tr, C_GRID, CV_FOLDS, MAX_ITER, 1, SEED)
    _, base_train_score = ref._predict(base_model, base_train)
    base_prob, base_score = ref._predict(base_model, base_test)
    base_metrics = ref._safe_metrics(y_te, base_prob)
    cal_folds = list(ref._cv_splitter(y_tr, CV_FOLDS, SEED).split(base_train, y_tr))
    out.update(cal_best_c=np.array(base_model.best_params_["model__C"]), cal_cv_bce=-base_model.cv_results_["mean_test_score"],
               cal_train_score=base_train_score, cal_test_score=base_score, cal_test_prob=base_prob,
               cal_metrics=np.array([base_metrics[k] for k in ("bce", "auroc", "auprc")]))
    for k, (a, b) in enumerate(cal_folds):
        out[f"cal_fold{k}_train"], out[f"cal_fold{k}_valid"] = a.astype(np.int16), b.astype(np.int16)

    # ---- the reference objective's own value / gradient at a probe point, captured from inside _fit_offset_weights ----
    captured = {}
    real_minimize = ref.minimize

    def capture(objective, x0, **kw):
        if "fun" not in captured and x0.size:
            w = 0.05 * np.random.default_rng(1).standard_normal(x0.size)
            loss, grad = objective(w)
            captured.update(w=w, fun=loss, grad=np.array(grad))
        return real_minimize(objective, x0, **kw)

    evidence = []
    for probe_offset, block in enumerate(BLOCKS):
        train_frame = pd.DataFrame(b_tr[block], columns=list(names[block]))
        test_frame = pd.DataFrame(b_te[block], columns=list(names[block]))
        fit_seed = SEED + probe_offset + 1
        folds = list(ref._cv_splitter(y_tr, CV_FOLDS, fit_seed).split(train_frame, y_tr))
        if block == "level":
            # a single-candidate fit on the full training rows: the captured point belongs to this design matrix
            ref.minimize = capture
            imputer = ref.SimpleImputer(strategy="median", add_indicator=True)
            design = ref.StandardScaler().fit_transform(imputer.fit_transform(train_frame))
            ref._fit_offset_weights(design, y_tr, base_train_score, 0.01, MAX_ITER)
            ref.minimize = real_minimize
            out.update(obj_design=design, obj_w=captured["w"], obj_fun=np.array(captured["fun"]), obj_grad=captured["grad"],
                       obj_l2=np.array(0.01))
        fitted = ref._fit_offset_correction(train_frame, y_tr, base_train_score, L2_GRID, CV_FOLDS, MAX_ITER, NULL_TOL, fit_seed)
        prob, score = fitted.predict(base_score, test_frame)
        metrics = ref._safe_metrics(y_te, prob)
        boot = ref._cluster_bootstrap_differences(y_te, base_prob, prob, subj_te, N_BOOT, SEED + probe_offset)
        perm = ref._conditional_permutation_offset(fitted, y_te, img_te, base_score, b_te[block], names[block], N_PERM, PERM_BINS,
                                                   SEED + probe_offset)
        cv = np.array([fitted.cv_results["null"]] + [fitted.cv_results[f"l2={v:g}"] for v in L2_GRID])
        gain = base_metrics["bce"] - metrics["bce"]
        ev = ("supported" if gain > 0 and boot["bce_gain_ci_low"] > 0 and perm["perm_bce_mean"] - metrics["bce"] > 0
              else "suggestive" if gain > 0 else "not_detected")
        evidence.append(ev)
        p = f"{block}_"
        out.update({p + "cv_results": cv, p + "selected_l2": np.array(np.nan if fitted.selected_l2 is None else fitted.selected_l2),
                    p + "weights": fitted.weights, p + "names": np.array(fitted.transformed_names), p + "test_prob": prob,
                    p + "test_score": score, p + "metrics": np.array([metrics[k] for k in ("bce", "auroc", "auprc")]),
                    p + "boot_keys": np.array(list(boot)), p + "boot": np.array(list(boot.values())),
                    p + "perm_keys": np.array(list(perm)), p + "perm": np.array(list(perm.values()))})
        for k, (a, b) in enumerate(folds):
            out[f"{p}fold{k}_train"], out[f"{p}fold{k}_valid"] = a.astype(np.int16), b.astype(np.int16)
        margin = cv[1:].min() + NULL_TOL - cv[0]
        print(f"{block:12s} selected_l2={fitted.selected_l2}  null margin {margin:+.5f}  gain {gain:+.5f}  {ev}")
        if block == "noise":
            # not marginal: no non-null candidate even beats the null one, so the decision `null <= best + null_tolerance` holds by
            # more than the whole tolerance (it cannot hold by much more: the l2 = 100 candidate is the null one to within 1e-4)
            assert fitted.null_selected and margin >= NULL_TOL, margin
        if block == "level":
            assert not fitted.null_selected and -margin > 2e-3, margin      # the planted effect is found, not marginally
            # the drawn indices (:771-777, :816-820) and the reference's metrics on every replicate
            uniq = np.unique(subj_te)
            members = {s: np.flatnonzero(subj_te == s) for s in uniq}
            g = np.random.default_rng(SEED + probe_offset)
            idx = [np.concatenate([members[s] for s in g.choice(uniq, size=len(uniq), replace=True)]) for _ in range(N_BOOT)]
            m_base = np.array([[ref._safe_metrics(y_te[i], base_prob[i])[k] for k in ("bce", "auroc", "auprc")] for i in idx])
            m_probe = np.array([[ref._safe_metrics(y_te[i], prob[i])[k] for k in ("bce", "auroc", "auprc")] for i in idx])
            lo, hi = np.percentile(m_base[:, 0] - m_probe[:, 0], [2.5, 97.5])
            assert lo == boot["bce_gain_ci_low"] and hi == boot["bce_gain_ci_high"]      # the draws ARE the reference's
            bins = ref._image_risk_bins(img_te, PERM_BINS)
            g = np.random.default_rng(SEED + probe_offset)
            shuf = np.stack([ref._conditional_shuffle_indices(bins, g) for _ in range(N_PERM)])
            m_perm = np.array([[ref._safe_metrics(y_te, fitted.predict(base_score, pd.DataFrame(b_te[block][s], columns=list(
                names[block])))[0])[k] for k in ("bce", "auroc", "auprc")] for s in shuf])
            assert m_perm[:, 0].mean() == perm["perm_bce_mean"]
            out.update(boot_idx=np.concatenate(idx).astype(np.int16), boot_offsets=np.cumsum([0] + [len(i) for i in idx]),
                       boot_metrics_base=m_base, boot_metrics_probe=m_probe, perm_bins=bins.astype(np.int16),
                       perm_idx=shuf.astype(np.int16), perm_metrics=m_perm)
    out["evidence"] = np.array(evidence)

    path = os.path.join(out_dir, "raw_probe.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote raw_probe.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
