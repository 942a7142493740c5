"""GPU: the raw-trajectory conditional probe end to end on the reference's fixture (tests/golden/raw_probe.npz: the reference's own
functions on one seeded problem, tests/golden/make_golden_raw_probe.py), with the recorded StratifiedKFold index lists.

Exact: NaN patterns and the accumulation-free summaries, `transformed_names`, `selected_l2` / the null selection, the evidence strings.
Optimality: the returned weights satisfy max|gradient| <= 1e-7 (the reference's `gtol`) under the RESTATED gradient
(tests/raw_probe_refs.py), and their restated objective does not exceed the one at the reference's weights by more than rounding.
Against the reference's numbers: `cv_results`, weights, test probabilities, bootstrap CIs and permutation statistics cannot agree to
rounding: the reference's L-BFGS-B also stops on `ftol = 1e-11`, usually before `gtol`, so its weights sit ~1e-5 from the optimum
this module reaches.  As the issue prescribes, each quantity's largest deviation from the fixture over the six blocks was measured on
an MI355X and the test asserts at 8x that figure (both are in DESIGN.md, "Raw-trajectory probe"); every test prints its figures."""
import numpy as np
import pytest
import torch

from raw_probe_refs import EXACT_STATS, STATS, golden, golden_folds, offset_logistic_valgrad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCKS = ("level", "trajectory", "observation", "physiologic", "all", "noise")       # probe_offset = position, as in the fixture
# quantity: (largest deviation from the fixture measured over the six blocks, on an MI355X); asserted at 8x
MEASURED = {"cv_results": 1.590e-5, "weights": 1.502e-5, "test_prob": 5.676e-6, "boot": 3.945e-7, "perm": 3.611e-5}
RUN_PROBE_MEASURED = 1.224e-6              # run_probe rows (own image calibration instead of the recorded one) against the fixture
_state = {}


def _rp():
    from multimodal_edema_prediction_amd import raw_trajectory_probe
    return raw_trajectory_probe


def _ps():
    from multimodal_edema_prediction_amd import probe_stats
    return probe_stats


def _blocks():
    """Summaries of both splits on the device, once; the noise block rides along."""
    if "blocks" not in _state:
        g, rp = golden(), _rp()
        out = {}
        for split in ("train", "test"):
            x = torch.as_tensor(np.array(g[f"x_{split}"]), device=DEV)
            blocks, names = rp.raw_summary_blocks(x, [str(v) for v in g["var_names"]], int(g["cfg"][4]))
            blocks["noise"] = torch.as_tensor(np.array(g[f"noise_{split}"]), device=DEV)
            names["noise"] = tuple(f"noise{i}" for i in range(4))
            out[split] = blocks
        _state["blocks"] = (out["train"], out["test"], names)
    return _state["blocks"]


def _fit(block):
    if ("fit", block) not in _state:
        g, rp = golden(), _rp()
        train, _, names = _blocks()
        cfg = g["cfg"]
        _state[("fit", block)] = rp.fit_offset_correction(
            train[block], g["y_train"], g["cal_train_score"], tuple(g["l2_grid"]), int(cfg[5]), int(cfg[6]), float(g["null_tolerance"]),
            int(cfg[7]) + BLOCKS.index(block) + 1, folds=golden_folds(g, block + "_"), input_names=names[block])
    return _state[("fit", block)]


def _check(quantity, got, want):
    dev = float(np.nanmax(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)))) if np.size(want) else 0.0
    print(f"{quantity}: largest deviation {dev:.3e}  (measured bound {MEASURED[quantity]:.3e}, asserted at 8x)")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert dev <= 8 * MEASURED[quantity], (quantity, dev)


@pytest.mark.parametrize("split", ["train", "test"])
def test_summary_blocks_match_the_reference(split):
    g = golden()
    train, test, names = _blocks()
    blocks = train if split == "train" else test
    want = g[f"summary_{split}"]
    n = want.shape[0]
    got = torch.cat([blocks["level"].reshape(n, 3, 5), blocks["trajectory"].reshape(n, 3, 4), blocks["observation"].reshape(n, 3, 5)],
                    2).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for k, name in enumerate(STATS):
        if name in EXACT_STATS:
            assert np.array_equal(got[..., k], want[..., k], equal_nan=True), name
        else:                                                            # fp64 summation order over T = 24 hours (see the kernel tests)
            np.testing.assert_allclose(got[..., k], want[..., k], rtol=1e-9, atol=1e-9, equal_nan=True, err_msg=name)
    assert names["level"][:6] == ("hr__last", "hr__mean", "hr__std", "hr__min", "hr__max", "map__last")
    assert names["all"] == names["level"] + names["trajectory"] + names["observation"] == names["physiologic"] + names["observation"]
    assert torch.equal(blocks["all"][:, :27].nan_to_num(1e300), blocks["physiologic"].nan_to_num(1e300))
    assert blocks["all"].shape == (n, 42) and len(names["all"]) == 42


@pytest.mark.parametrize("block", BLOCKS)
def test_fit_offset_correction(block):
    g, rp = golden(), _rp()
    train, test, names = _blocks()
    model = _fit(block)
    want_l2 = float(g[block + "_selected_l2"])
    assert model.null_selected == np.isnan(want_l2)
    assert model.null_selected or model.selected_l2 == want_l2
    assert model.transformed_names == tuple(str(n) for n in g[block + "_names"])
    assert list(model.cv_results) == ["null"] + [f"l2={v:g}" for v in g["l2_grid"]]
    assert model.cv_bce == model.cv_results["null" if model.null_selected else f"l2={model.selected_l2:g}"]
    _check("cv_results", np.array(list(model.cv_results.values())), g[block + "_cv_results"])
    _check("weights", model.weights, g[block + "_weights"])
    if not model.null_selected:
        X = model.preprocessor.transform(train[block]).cpu().numpy()
        l2 = np.array([model.selected_l2])
        obj, grad = offset_logistic_valgrad_ref(X, g["y_train"], g["cal_train_score"], model.weights[:, None], l2)
        ref_obj, ref_grad = offset_logistic_valgrad_ref(X, g["y_train"], g["cal_train_score"], g[block + "_weights"][:, None], l2)
        print(f"max|grad| {np.abs(grad).max():.3e} (reference's weights: {np.abs(ref_grad).max():.3e})  objective {obj[0]:.15f} "
              f"reference's {ref_obj[0]:.15f}")
        assert np.abs(grad).max() <= 1e-7 * (1 + 1e-6)                   # gtol; the slack is the kernel-vs-numpy gradient rounding
        assert obj[0] <= ref_obj[0] + 3e-13                              # rounding of a mean of 240 terms of magnitude <= 10: 240 * 1.1e-16 * 10
        assert [n for n, _ in model.standardized_coefficients()][0] == model.transformed_names[int(np.abs(model.weights).argmax())]
    else:
        assert not model.weights.any() and model.best_params_ == {"correction": "null", "correction_l2": None}
    prob, score = model.predict(g["cal_test_score"], test[block])
    _check("test_prob", prob, g[block + "_test_prob"])
    po = BLOCKS.index(block)
    boot = rp.cluster_bootstrap_differences(g["y_test"], g["cal_test_prob"], prob, g["subject_test"], int(g["cfg"][8]), int(g["cfg"][7]) + po)
    assert list(boot) == [str(k) for k in g[block + "_boot_keys"]]
    _check("boot", np.array(list(boot.values())), g[block + "_boot"])
    perm = rp.conditional_permutation_offset(model, g["y_test"], g["image_test"], g["cal_test_score"], test[block], int(g["cfg"][9]),
                                             int(g["cfg"][10]), int(g["cfg"][7]) + po)
    assert list(perm) == [str(k) for k in g[block + "_perm_keys"]]
    _check("perm", np.array(list(perm.values())), g[block + "_perm"])


def test_a_pure_noise_block_selects_the_null_candidate():
    g = golden()
    assert np.isnan(float(g["noise_selected_l2"]))                       # the reference does on this fixture
    model = _fit("noise")
    assert model.null_selected and model.selected_l2 is None and not model.weights.any()
    margin = min(v for k, v in model.cv_results.items() if k != "null") + float(g["null_tolerance"]) - model.cv_results["null"]
    assert margin >= float(g["null_tolerance"])                          # as far from the decision boundary as the reference is
    _, test, _ = _blocks()
    prob, _ = model.predict(g["cal_test_score"], test["noise"])
    assert np.array_equal(prob, _ps().expit(g["cal_test_score"]))       # the exact null: the calibrated image predictor, untouched


def test_the_metrics_kernel_reproduces_the_reference_on_every_replicate():
    """The drawn replicates are the reference's (CPU test); scored on the device they give the reference's per-replicate metrics to
    fp64 summation order (bound: the kernel tests' 1e-10)."""
    g, rp = golden(), _rp()
    d = lambda a: torch.as_tensor(np.array(a), device=DEV)  # noqa: E731
    y = d(g["y_test"].astype(np.uint8))
    idx, offsets = d(g["boot_idx"].astype(np.int32)), d(g["boot_offsets"].astype(np.int64))
    for p, want in ((g["cal_test_prob"], g["boot_metrics_base"]), (g["level_test_prob"], g["boot_metrics_probe"])):
        got = _ps().resampled_binary_metrics(y, d(p[None]), idx, offsets).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)
    assert rp.safe_metrics(g["y_test"], g["level_test_prob"]) == pytest.approx(dict(zip(("bce", "auroc", "auprc"), g["level_metrics"])), abs=1e-10)


def test_run_probe_restates_the_reference_loop():
    g, rp = golden(), _rp()
    train, test, names = _blocks()
    cfg = g["cfg"]
    use = ("level", "trajectory")                                        # probe_offset 0 and 1, as in the fixture
    rows, fitted = rp.run_probe(train, test, names, g["y_train"], g["y_test"], g["image_train"], g["image_test"], g["subject_test"],
                                label="label_edema", blocks=use, c_grid=tuple(g["c_grid"]), correction_l2_grid=tuple(g["l2_grid"]),
                                null_tolerance=float(g["null_tolerance"]), cv_folds=int(cfg[5]), max_iter=int(cfg[6]), bootstrap=int(cfg[8]),
                                perm_repeats=int(cfg[9]), perm_bins=int(cfg[10]), seed=int(cfg[7]), calibration_folds=golden_folds(g, "cal_"),
                                correction_folds={b: golden_folds(g, b + "_") for b in use})
    assert [r["block"] for r in rows] == list(use) and [r["evidence"] for r in rows] == [str(g["evidence"][BLOCKS.index(b)]) for b in use]
    assert fitted["image_cal"].best_params_ == {"model__C": float(g["cal_best_c"])}
    for row, block in zip(rows, use):
        assert row["null_selected"] == bool(np.isnan(float(g[block + "_selected_l2"])))
        for key in ("bce_gain_ci_low", "auprc_gain_ci_high", "perm_bce_mean", "perm_auroc_high", "inner_cv_bce", "corr_residual",
                    "perm_bce_increase", "perm_auroc_drop", "best_params", "correction_cv_results", "n_input_features"):
            assert key in row
        got = np.array([row["image_cal_bce"], row["image_cal_auroc"], row["image_cal_auprc"], row["probe_bce"], row["probe_auroc"],
                        row["probe_auprc"]])
        want = np.concatenate([g["cal_metrics"], g[block + "_metrics"]])
        dev = np.abs(got - want).max()
        print(f"run_probe {block}: largest metric deviation {dev:.3e}  (measured bound {RUN_PROBE_MEASURED:.3e}, asserted at 8x)")
        assert dev <= 8 * RUN_PROBE_MEASURED


def test_fit_raises_when_max_iter_is_reached():
    g, rp = golden(), _rp()
    train, _, names = _blocks()
    with pytest.raises(RuntimeError, match="max_iter"):
        rp.fit_offset_correction(train["level"], g["y_train"], g["cal_train_score"], (0.01,), 5, 3, 5e-4, 1, folds=golden_folds(g, "level_"))
    with pytest.raises(ValueError, match="Not enough samples"):
        rp.fit_offset_correction(train["level"][:4], np.array([0, 0, 0, 1]), np.zeros(4), (0.01,), 5, 50, 5e-4, 1)
