#!/usr/bin/env python3
"""Golden fixture for the conditional-information probe (analysis/conditional_information_probe.py): runs the REFERENCE'S OWN functions
(`_features`, `_fit_probe`, `_predict`, `_safe_metrics`, `_pearson`, `_bootstrap_differences`, `_conditional_permutation`,
`_image_risk_bins`, `_conditional_shuffle_indices`; stubs as in make_golden.py) on ONE seeded problem, restating the body of its
`main()` label / probe loop (:440-574), and stores numbers only in tests/golden/cond_probe.npz.

The problem: n_train = 240, n_test = 160 gathered rows, K = 3 labels, D = 16 token channels, 85 % of the labels known; the label
depends on the image logit and on token channel 0 (the planted effect), the ts logit is a noisy view of that channel.

The loop is restated twice:
  R  as the reference is: `_fit_probe` = Pipeline(StandardScaler, LogisticRegression(C, lbfgs)) on the fp32 arrays of `_gather`;
  T  with `_fit_probe` replaced by the same pipeline on float64 features with solver="newton-cholesky", tol=1e-12: the optimum of
     the reference's own objective, which its L-BFGS (sklearn's default tol = 1e-4) stops short of.
Stored: the inputs; per fit the R and T coefficients (standardised space), intercepts, means, scales, test probabilities and scores;
every row value of both loops; for one probe (label 0, token_linear, T) the drawn bootstrap and shuffle indices with the per-replicate
metrics; the row-key list; per fit ||H^-1||_2 at T's optimum and T's gradient max-norm, both evaluated here in fp64 by the numpy
restatement (tests/cond_probe_refs.py).  Build container only.

Usage:  python tests/golden/make_golden_cond_probe.py [output directory]"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from cond_probe_refs import FIT_NAMES, PROBE_NAMES, terms_ref  # noqa: E402  (tests/ is on the path through make_golden)

N_TRAIN, N_TEST, K, D = 240, 160, 3, 16
LOGIT_C, TOKEN_C, MAX_ITER, SEED, N_BOOT, N_PERM, PERM_BINS = 100.0, 1.0, 3000, 42, 200, 50, 10
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
DATA_SEED = 1


def synth_split(rng, n):
    """What `_gather` returns for n rows, fp32: img, ts, fus [n, K], token [n, K, D], y, mask [n, K]."""
    token = rng.standard_normal((n, K, D))
    img = 1.2 * rng.standard_normal((n, K))
    ts = 0.8 * token[:, :, 0] + 0.6 * rng.standard_normal((n, K)) + 0.2
    logit = -0.3 + 0.9 * img + 1.1 * token[:, :, 0] + 0.25 * token[:, :, 1]
    y = (rng.random((n, K)) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    mask = (rng.random((n, K)) < 0.85).astype(np.float32)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return {"img": f32(img), "ts": f32(ts), "fus": f32(img + 0.5 * ts), "token": f32(token), "y": y, "mask": mask}


def main(out_dir=HERE):
    install_stubs()
    sys.path.insert(0, REF)
    import analysis.conditional_information_probe as ref
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    warnings.filterwarnings("error", category=UserWarning, module="sklearn")          # a solver fall-back or non-convergence is an error here

    rng = np.random.default_rng(DATA_SEED)
    train, test = synth_split(rng, N_TRAIN), synth_split(rng, N_TEST)
    out = {f"{split}_{k}": v for split, d in (("train", train), ("test", test)) for k, v in d.items()}
    out.update(cfg=np.array([N_TRAIN, N_TEST, K, D, MAX_ITER, SEED, N_BOOT, N_PERM, PERM_BINS]), logit_c=np.array(LOGIT_C),
               token_c=np.array(TOKEN_C), labels=np.array(LABELS))

    def fit_T(features, y, c_value, max_iter):
        if len(np.unique(y)) < 2:
            raise ValueError("Probe-training labels contain only one class")
        model = Pipeline([("scale", StandardScaler()), ("logistic", LogisticRegression(C=float(c_value), penalty="l2",
                         solver="newton-cholesky", tol=1e-12, max_iter=int(max_iter), class_weight=None, random_state=0))])
        return model.fit(np.asarray(features, dtype=np.float64), y)

    def loop(fit, version, cast):
        """The reference's loop (:440-574) with `fit` for `_fit_probe`; `cast` the feature dtype handed to fit / predict."""
        rows = []
        for k, label in enumerate(LABELS):
            tm, sm = train["mask"][:, k].astype(bool), test["mask"][:, k].astype(bool)
            y_train, y_test = train["y"][tm, k].astype(np.int64), test["y"][sm, k].astype(np.int64)
            assert len(np.unique(y_train)) == 2 and len(np.unique(y_test)) == 2
            a_tr = (train["img"][tm, k], train["ts"][tm, k], train["token"][tm, k, :])
            a_te = (test["img"][sm, k], test["ts"][sm, k], test["token"][sm, k, :])
            feats = lambda name, a: ref._features(name, *a).astype(cast)  # noqa: E731
            base_model = fit(feats("image_cal", a_tr), y_train, LOGIT_C, MAX_ITER)
            base_p, base_s = ref._predict(base_model, feats("image_cal", a_te))
            base_metrics = ref._safe_metrics(y_test, base_p)
            models = {"image_cal": (base_model, base_p, base_s)}
            for probe_offset, name in enumerate(PROBE_NAMES):
                c_value = TOKEN_C if name == "token_linear" else LOGIT_C
                model = fit(feats(name, a_tr), y_train, c_value, MAX_ITER)
                prob, score = ref._predict(model, feats(name, a_te))
                models[name] = (model, prob, score)
                metrics = ref._safe_metrics(y_test, prob)
                gains = {"bce_gain": base_metrics["bce"] - metrics["bce"], "auroc_gain": metrics["auroc"] - base_metrics["auroc"],
                         "auprc_gain": metrics["auprc"] - base_metrics["auprc"]}
                confidence = ref._bootstrap_differences(y_test, base_p, prob, N_BOOT, SEED + 1000 * k + probe_offset)
                corr = ref._pearson(score - base_s, y_test.astype(np.float64) - base_p)
                # the reference permutes the arrays and rebuilds `_features` from them; the model sees them in `cast`
                perm_model = model if cast == np.float32 else _Cast64(model)
                perm = ref._conditional_permutation(perm_model, name, y_test, a_te[0], a_te[1], a_te[2], N_PERM, PERM_BINS,
                                                    SEED + 10000 * k + probe_offset)
                inc, drop = perm["perm_bce_mean"] - metrics["bce"], metrics["auroc"] - perm["perm_auroc_mean"]
                ev = ("supported" if gains["bce_gain"] > 0 and confidence["bce_gain_ci_low"] > 0 and inc > 0
                      else "suggestive" if gains["bce_gain"] > 0 else "not_detected")
                rows.append({"label": label, "probe": name, "n_test": int(len(y_test)), "n_positive": int(y_test.sum()),
                             "prevalence": float(y_test.mean()), "image_cal_bce": base_metrics["bce"],
                             "image_cal_auroc": base_metrics["auroc"], "image_cal_auprc": base_metrics["auprc"],
                             "probe_bce": metrics["bce"], "probe_auroc": metrics["auroc"], "probe_auprc": metrics["auprc"], **gains,
                             **confidence, "corr_residual": corr, **perm, "perm_bce_increase": inc, "perm_auroc_drop": drop,
                             "evidence": ev})
                if version == "T" and k == 0 and name == "token_linear":
                    # the drawn indices (:234-238, :323-327) and the reference's metrics on every replicate
                    g = np.random.default_rng(SEED + 1000 * k + probe_offset)
                    idx = np.stack([g.integers(0, len(y_test), size=len(y_test)) for _ in range(N_BOOT)])
                    three = lambda yy, pp: [ref._safe_metrics(yy, pp)[m] for m in ("bce", "auroc", "auprc")]  # noqa: E731
                    m_base = np.array([three(y_test[i], base_p[i]) for i in idx])
                    m_probe = np.array([three(y_test[i], prob[i]) for i in idx])
                    lo, hi = np.percentile(m_base[:, 0] - m_probe[:, 0], [2.5, 97.5])
                    assert abs(lo - confidence["bce_gain_ci_low"]) < 1e-12 and abs(hi - confidence["bce_gain_ci_high"]) < 1e-12
                    bins = ref._image_risk_bins(a_te[0], PERM_BINS)
                    g = np.random.default_rng(SEED + 10000 * k + probe_offset)
                    shuf = np.stack([ref._conditional_shuffle_indices(bins, g) for _ in range(N_PERM)])
                    m_perm = np.array([three(y_test, ref._predict(perm_model, ref._features(name, a_te[0], a_te[1][s], a_te[2][s]))[0])
                                       for s in shuf])
                    assert m_perm[:, 0].mean() == perm["perm_bce_mean"]
                    out.update(boot_idx=idx.astype(np.int16), boot_metrics_base=m_base, boot_metrics_probe=m_probe,
                               perm_bins=bins.astype(np.int16), perm_idx=shuf.astype(np.int16), perm_metrics=m_perm)
            for name, (model, prob, score) in models.items():
                p = f"{version}_{k}_{name}_"
                scaler, logistic = model.named_steps["scale"], model.named_steps["logistic"]
                out.update({p + "coef": logistic.coef_[0].astype(np.float64), p + "intercept": np.float64(logistic.intercept_[0]),
                            p + "mean": scaler.mean_.astype(np.float64), p + "scale": scaler.scale_.astype(np.float64),
                            p + "test_prob": prob, p + "test_score": score})
                assert prob.min() > 1e-7 and prob.max() < 1 - 1e-7, (p, prob.min(), prob.max())   # clipped and unclipped log-loss agree
                if version == "T":
                    X = ref._features(name, *a_tr).astype(np.float64)
                    theta = np.r_[logistic.coef_[0], logistic.intercept_[0]]
                    _, grad, H = terms_ref(X, y_train, theta, scaler.mean_, scaler.scale_, 1.0 / (float(logistic.C) * len(y_train)))
                    out[p + "hinv"], out[p + "gmax"] = np.float64(1.0 / np.linalg.eigvalsh(H).min()), np.float64(np.abs(grad).max())
                    assert out[p + "gmax"] < 1e-9, (p, out[p + "gmax"])
                    distinct = np.unique(prob)
                    assert distinct.size < 2 or np.diff(distinct).min() >= 1e-6, (p, np.diff(distinct).min())
            if version == "T":
                for probe_offset in range(len(PROBE_NAMES)):                 # every bootstrap replicate has both classes
                    g = np.random.default_rng(SEED + 1000 * k + probe_offset)
                    for _ in range(N_BOOT):
                        assert len(np.unique(y_test[g.integers(0, len(y_test), size=len(y_test))])) == 2
        return rows

    class _Cast64:
        """Hands a fitted pipeline float64 features, as the T fit received them."""

        def __init__(self, model):
            self.model = model

        def predict_proba(self, X):
            return self.model.predict_proba(np.asarray(X, dtype=np.float64))

        def decision_function(self, X):
            return self.model.decision_function(np.asarray(X, dtype=np.float64))

    rows_R = loop(ref._fit_probe, "R", np.float32)
    rows_T = loop(fit_T, "T", np.float64)
    keys = list(rows_R[0])
    numeric = [k for k in keys if k not in ("label", "probe", "evidence")]
    assert [r["evidence"] for r in rows_R] == [r["evidence"] for r in rows_T]
    out.update(row_keys=np.array(keys), row_numeric_keys=np.array(numeric), row_label=np.array([r["label"] for r in rows_R]),
               row_probe=np.array([r["probe"] for r in rows_R]), evidence=np.array([r["evidence"] for r in rows_R]),
               R_rows=np.array([[float(r[k]) for k in numeric] for r in rows_R]),
               T_rows=np.array([[float(r[k]) for k in numeric] for r in rows_T]))
    for r, t in zip(rows_R, rows_T):
        print(f"{r['label']:20s} {r['probe']:18s} {r['evidence']:13s} bce_gain R {r['bce_gain']:+.6f} T {t['bce_gain']:+.6f}")
    print("max |T - R| over the row values:", np.nanmax(np.abs(out["R_rows"] - out["T_rows"])))

    path = os.path.join(out_dir, "cond_probe.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote cond_probe.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
