"""CPU: the numpy restatement of the raw-trajectory-probe kernels (tests/raw_probe_refs.py) is pinned on the reference's own outputs
(tests/golden/raw_probe.npz, written by tests/golden/make_golden_raw_probe.py), and the host-side index draws of
multimodal_edema_prediction_amd.probe_stats equal the reference's.

Tolerances.  The restatement and the reference both work in fp64 and differ only in summation order (numpy's pairwise / blocked sums
against hour-by-hour sums; BLAS dot products against numpy's), so the bound is the fp64 rounding of sums of <= 240 terms of magnitude
<= a few hundred: 240 * 2.2e-16 * 1e2 ~ 5e-12 absolute on the sums, which the centred slope / std forms amplify by their condition
number (<= 1e3 here): RTOL = ATOL = 1e-9."""
import numpy as np
import pytest

from raw_probe_refs import (EXACT_STATS, STATS, binary_metrics_ref, golden, offset_logistic_valgrad_ref, raw_traj_summary_ref,
                            resampled_binary_metrics_ref)

RTOL = ATOL = 1e-9


@pytest.mark.parametrize("split", ["train", "test"])
def test_summary_restatement_matches_the_reference(split):
    g = golden()
    T, recent = int(g["cfg"][2]), int(g["cfg"][4])
    want, got = g[f"summary_{split}"], raw_traj_summary_ref(g[f"x_{split}"], recent)
    assert got.shape == want.shape == (g[f"x_{split}"].shape[0], 3, 14)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for k, name in enumerate(STATS):
        if name in EXACT_STATS:
            assert np.array_equal(got[..., k], want[..., k], equal_nan=True), name
        else:
            np.testing.assert_allclose(got[..., k], want[..., k], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=name)
    # the fixture does hold the edge cases the NaN rules are about
    assert np.isnan(want[:, 2, 0]).any() and (want[:, 2, 11] == T).any()
    assert (np.isnan(want[:, 1, 5]) & ~np.isnan(want[:, 1, 0])).any()
    assert np.isnan(g[f"x_{split}"][:, :, 0]).any()


def test_objective_restatement_matches_the_reference_closure():
    g = golden()
    obj, grad = offset_logistic_valgrad_ref(g["obj_design"], g["y_train"], g["cal_train_score"], g["obj_w"][:, None], g["obj_l2"][None])
    np.testing.assert_allclose(obj[0], float(g["obj_fun"]), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad[:, 0], g["obj_grad"], rtol=RTOL, atol=ATOL)


def test_metrics_restatement_matches_the_reference_on_every_replicate():
    g = golden()
    y = g["y_test"]
    for p, want in ((g["cal_test_prob"], g["boot_metrics_base"]), (g["level_test_prob"], g["boot_metrics_probe"])):
        got = resampled_binary_metrics_ref(y, p[None], g["boot_idx"], g["boot_offsets"])
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(binary_metrics_ref(y, g["level_test_prob"]), g["level_metrics"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(binary_metrics_ref(y, g["cal_test_prob"]), g["cal_metrics"], rtol=RTOL, atol=ATOL)


def test_metrics_restatement_on_ties_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    for n, levels in ((2, 2), (17, 4), (200, 4), (1000, 7), (333, 1)):
        y = (rng.random(n) < 0.4).astype(np.int64)
        y[:2] = (0, 1)
        p = rng.integers(0, levels, n) / max(levels, 2) + 0.05           # heavy exact ties
        got = binary_metrics_ref(y, p)
        q = np.clip(p, 1e-7, 1 - 1e-7)
        want = (metrics.log_loss(y, q, labels=[0, 1]), metrics.roc_auc_score(y, q), metrics.average_precision_score(y, q))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    one_class = binary_metrics_ref(np.ones(5, np.int64), rng.random(5))
    assert np.isfinite(one_class[0]) and np.isnan(one_class[1:]).all()
    assert np.isnan(binary_metrics_ref(np.zeros(0, np.int64), np.zeros(0))).all()


def test_host_index_draws_equal_the_reference():
    from multimodal_edema_prediction_amd import probe_stats as rp
    g = golden()
    boot_seed = perm_seed = int(g["cfg"][7])                            # the level block is probe_offset 0
    idx, offsets = rp.draw_cluster_bootstrap_indices(g["subject_test"], int(g["cfg"][8]), boot_seed)
    assert np.array_equal(offsets, g["boot_offsets"]) and np.array_equal(idx, g["boot_idx"])
    bins = rp.image_risk_bins(g["image_test"], int(g["cfg"][10]))
    assert np.array_equal(bins, g["perm_bins"])
    rng = np.random.default_rng(perm_seed)
    shuf = np.stack([rp.conditional_shuffle_indices(bins, rng) for _ in range(int(g["cfg"][9]))])
    assert np.array_equal(shuf, g["perm_idx"])
    assert np.array_equal(rp.image_risk_bins(g["image_test"], 1), np.zeros(len(bins), np.int64))


def test_calibration_matches_the_reference_pipeline():
    """Exact 2 x 2 Newton against sklearn's lbfgs at its default tol = 1e-4 (a gradient-norm stop): sklearn's own solution is only
    that close to the optimum, which bounds the comparison, not fp64.  Largest deviations measured on this fixture: scores 4.45e-5, CV BCE 2.21e-6; asserted at 8x."""
    from multimodal_edema_prediction_amd import raw_trajectory_probe as rp
    from raw_probe_refs import golden_folds
    g = golden()
    cal = rp.calibrate_image_logit(g["image_train"], g["y_train"], tuple(g["c_grid"]), int(g["cfg"][5]), int(g["cfg"][7]),
                                   folds=golden_folds(g, "cal_"))
    assert cal.best_params_ == {"model__C": float(g["cal_best_c"])}
    d_cv = np.abs(cal.cv_bce - g["cal_cv_bce"]).max()
    d_tr = np.abs(cal.decision_function(g["image_train"]) - g["cal_train_score"]).max()
    d_te = np.abs(cal.decision_function(g["image_test"]) - g["cal_test_score"]).max()
    print(f"calibration deviations: cv_bce {d_cv:.3e}  train score {d_tr:.3e}  test score {d_te:.3e}")
    assert d_cv <= 8 * 2.21e-6 and max(d_tr, d_te) <= 8 * 4.45e-5


def test_default_folds_are_stratified_and_seeded():
    from multimodal_edema_prediction_amd import raw_trajectory_probe as rp
    y = golden()["y_train"]
    a, b = rp.stratified_folds(y, 5, 3), rp.stratified_folds(y, 5, 3)
    assert len(a) == 5 and all(np.array_equal(u[1], v[1]) for u, v in zip(a, b))
    assert np.array_equal(np.sort(np.concatenate([v for _, v in a])), np.arange(len(y)))
    pos = [int(y[v].sum()) for _, v in a]
    assert max(pos) - min(pos) <= 1
    for tr, va in a:
        assert np.intersect1d(tr, va).size == 0 and tr.size + va.size == len(y)
    with pytest.raises(ValueError, match="Not enough samples"):
        rp.stratified_folds(np.array([0, 0, 0, 1]), 5, 0)
    assert len(rp.stratified_folds(np.array([0, 0, 0, 1, 1, 0]), 5, 0)) == 2       # min(requested, smallest class)
