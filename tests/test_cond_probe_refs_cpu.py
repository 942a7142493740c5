"""CPU: the numpy restatement of the conditional-information probe (tests/cond_probe_refs.py) pinned on the reference's fixture
(tests/golden/cond_probe.npz, written by tests/golden/make_golden_cond_probe.py: loop R = the reference as shipped, loop T = the same
pipeline solved to tol = 1e-12), and the host-side pieces of the module that need no GPU: the index draws, the row keys, the
argument checks of the three entry points (made before anything is launched) and the refusal to run without a GPU.

Fitted parameters are compared with T within the issue's bound 10 ||H^-1||_2 (1e-10 + max|g_T|) per fit: both sides stop at a
gradient of at most 1e-10 resp. g_T, and a gradient g displaces the optimum of a strongly convex objective by at most ||H^-1|| |g|
(the factor 10 covers the max-norm / 2-norm gap for F + 1 <= 18 parameters and the change of H between the two points)."""
import ctypes

import numpy as np
import pytest
import torch

from cond_probe_refs import (FIT_NAMES, PROBE_NAMES, draw_bootstrap_ref, features, fit_bound, golden, moments_ref, newton_fit_ref,
                             scores_ref, split_of, terms_ref)

K = 3


def _cip():
    from multimodal_edema_prediction_amd import conditional_information_probe
    return conditional_information_probe


def _label(g, split, k):
    d = split_of(g, split)
    m = d["mask"][:, k].astype(bool)
    return d["img"][m, k], d["ts"][m, k], d["token"][m, k, :], d["y"][m, k].astype(np.int64)


@pytest.mark.parametrize("k", range(K))
def test_newton_restatement_reaches_the_reference_optimum(k):
    g = golden()
    img, ts, token, y = _label(g, "train", k)
    for probe in FIT_NAMES:
        C = float(g["token_c"]) if probe == "token_linear" else float(g["logit_c"])
        fit = newton_fit_ref(features(probe, img, ts, token), y, C)
        p = f"T_{k}_{probe}_"
        bound = fit_bound(g, k, probe)
        dev = max(np.abs(fit["coef"] - g[p + "coef"]).max(), abs(fit["intercept"] - float(g[p + "intercept"])))
        print(f"{p}: {fit['n_iter']} iterations, max|g| {fit['gmax']:.2e}, |theta - T| {dev:.2e} (bound {bound:.2e}); "
              f"|T - R| {np.abs(g[p + 'coef'] - g['R' + p[1:] + 'coef']).max():.2e}")
        assert dev <= bound
        assert fit["n_iter"] <= 50 and fit["gmax"] <= 1e-10
        np.testing.assert_allclose(fit["mean"], g[p + "mean"], rtol=1e-12, atol=1e-12)      # sums of <= 240 terms of size <= ~10
        np.testing.assert_allclose(fit["scale"], g[p + "scale"], rtol=1e-12, atol=1e-12)


def test_terms_are_the_derivatives_of_the_objective():
    g = golden()
    img, ts, token, y = _label(g, "train", 0)
    X = features("logit_interaction", img, ts, token)
    mean, scale = moments_ref(X)
    theta = np.array([0.4, -0.7, 0.2, 0.1])
    f, grad, H = terms_ref(X, y, theta, mean, scale, 1e-3)
    h = 1e-5
    for j in range(4):
        e = np.zeros(4)
        e[j] = h
        fp, gp, _ = terms_ref(X, y, theta + e, mean, scale, 1e-3)
        fm, gm, _ = terms_ref(X, y, theta - e, mean, scale, 1e-3)
        assert abs((fp - fm) / (2 * h) - grad[j]) < 1e-9                  # central differences: h^2 |f'''| ~ 1e-10
        np.testing.assert_allclose((gp - gm) / (2 * h), H[:, j], atol=1e-9)
    assert np.abs(H - H.T).max() <= 4 * np.finfo(np.float64).eps * np.abs(H).max()     # a dense product: symmetric to rounding only


def test_scores_restatement_gives_the_reference_scores():
    g = golden()
    for k in range(K):
        img, ts, token, _ = _label(g, "test", k)
        for probe in FIT_NAMES:
            p = f"T_{k}_{probe}_"
            X = features(probe, img, ts, token)
            theta = np.r_[g[p + "coef"], float(g[p + "intercept"])]
            full = scores_ref(X, theta, g[p + "mean"], g[p + "scale"], 0, X.shape[1], True)
            np.testing.assert_allclose(full, g[p + "test_score"], rtol=1e-12, atol=1e-12)
            parts = scores_ref(X, theta, g[p + "mean"], g[p + "scale"], 0, 1, True) + scores_ref(X, theta, g[p + "mean"], g[p + "scale"],
                                                                                                 1, X.shape[1], False)
            np.testing.assert_allclose(parts, full, rtol=1e-12, atol=1e-12)
            model = _cip().FittedProbe(k, probe, g[p + "mean"], g[p + "scale"], g[p + "coef"], float(g[p + "intercept"]), 1.0, 0, 0.0)
            prob, score = model.predict(X)
            np.testing.assert_allclose(score, g[p + "test_score"], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(prob, g[p + "test_prob"], rtol=1e-12, atol=1e-12)


def test_index_draws_are_the_references():
    from multimodal_edema_prediction_amd.probe_stats import conditional_shuffle_indices, draw_bootstrap_indices, image_risk_bins
    g = golden()
    cfg = g["cfg"]
    seed, n_boot, n_perm, bins_n = int(cfg[5]), int(cfg[6]), int(cfg[7]), int(cfg[8])
    img, _, _, y = _label(g, "test", 0)
    probe_offset = PROBE_NAMES.index("token_linear")
    idx = draw_bootstrap_indices(len(y), n_boot, seed + probe_offset)
    assert idx.dtype == np.int32 and np.array_equal(idx, g["boot_idx"]) and np.array_equal(idx, draw_bootstrap_ref(len(y), n_boot, seed + probe_offset))
    assert draw_bootstrap_indices(len(y), 0, 1).shape == (0, len(y))
    bins = image_risk_bins(img, bins_n)
    assert np.array_equal(bins, g["perm_bins"])
    rng = np.random.default_rng(seed + probe_offset)
    assert np.array_equal(np.stack([conditional_shuffle_indices(bins, rng) for _ in range(n_perm)]), g["perm_idx"])


def test_row_keys_and_names_are_the_references():
    g, cip = golden(), _cip()
    assert list(cip.ROW_KEYS) == [str(k) for k in g["row_keys"]]
    assert cip.PROBE_NAMES == PROBE_NAMES == tuple(dict.fromkeys(str(p) for p in g["row_probe"]))
    labels = [str(s) for s in g["labels"]]
    assert cip.resolve_label_indices("all", labels) == (0, 1, 2)
    assert cip.resolve_label_indices("effusion, label_edema", labels) == (2, 0)
    with pytest.raises(ValueError, match="Unknown labels"):
        cip.resolve_label_indices("nope", labels)
    with pytest.raises(ValueError, match="Duplicate"):
        cip.resolve_label_indices("edema,label_edema", labels)


def test_the_fixture_states_the_references_distance_from_its_optimum():
    g = golden()
    assert [str(e) for e in g["evidence"]] and g["R_rows"].shape == g["T_rows"].shape == (9, len(g["row_numeric_keys"]))
    gap = np.nanmax(np.abs(g["R_rows"] - g["T_rows"]))
    assert 1e-6 < gap < 1e-2                                            # the reference's L-BFGS stops short of the optimum (tol = 1e-4)


def test_bad_arguments_are_refused_before_any_launch():
    from multimodal_edema_prediction_amd import abi
    L = abi.lib()
    Pb = abi.MedpProbeProblem
    assert ctypes.sizeof(Pb) == 40
    good = Pb(0, 0, 4, 2, 0, 0, 2, 0)
    q = 4096                                                             # a non-null token: nothing is dereferenced on a refusal

    def calls(table, P=1, Fmax=3, ldx=3, rows_total=4, nulls=False):
        t = (Pb * len(table))(*table)
        x = None if nulls else q
        return (L.medp_probe_moments(x, ldx, 10, t, q, q, rows_total, q, q, P, Fmax, None),
                L.medp_logistic_newton_terms(x, ldx, 10, q, 1, t, q, q, rows_total, q, q, q, q, q, q, q, q, 1 << 20, P, Fmax, None),
                L.medp_probe_scores(x, ldx, 10, t, q, q, rows_total, q, q, q, q, P, Fmax, 1, None))

    bad = {"null": dict(table=[good], nulls=True), "P": dict(table=[good], P=0), "F=0": dict(table=[Pb(0, 0, 4, 0, 0, 0, 0, 0)]),
           "F>Fmax": dict(table=[Pb(0, 0, 4, 4, 0, 0, 4, 0)], ldx=8), "one row": dict(table=[Pb(0, 0, 1, 2, 0, 0, 2, 0)]),
           "columns": dict(table=[Pb(2, 0, 4, 2, 0, 0, 2, 0)]), "rows": dict(table=[Pb(0, 2, 4, 2, 0, 0, 2, 0)]),
           "overlap": dict(table=[good, Pb(0, 2, 4, 2, 0, 0, 2, 0)], P=2, rows_total=8)}
    for name, kw in bad.items():
        for rc in calls(**kw):
            assert rc < 0, name
        assert L.medp_last_error()
    assert L.medp_logistic_newton_terms(q, 3, 10, q, 1, (Pb * 1)(Pb(0, 0, 4, 2, 1, 0, 2, 0)), q, q, 4, q, q, q, q, q, q, q, q, 1 << 20, 1, 3, None) < 0
    assert L.medp_logistic_newton_terms(q, 3, 10, q, 1, (Pb * 1)(good), q, q, 4, q, q, q, q, q, q, q, q, 8, 1, 3, None) < 0   # workspace
    assert L.medp_probe_scores(q, 3, 10, (Pb * 1)(Pb(0, 0, 4, 2, 0, 1, 3, 0)), q, q, 4, q, q, q, q, 1, 3, 1, None) < 0       # j1 > F
    assert L.medp_probe_terms_ws_bytes(0, 3, 4, 4) == 0 and L.medp_probe_terms_ws_bytes(1, 0, 4, 4) == 0
    assert L.medp_probe_terms_ws_bytes(1, 3, 1, 4) == 0 and L.medp_probe_terms_ws_bytes(1, 3, 8, 4) == 0
    assert L.medp_probe_terms_ws_bytes(2, 3, 65, 100) == (2 * 2 * 5 + 100) * 8


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_there_is_no_cpu_fallback():
    g, cip = golden(), _cip()
    data = {k: torch.as_tensor(np.array(v)) for k, v in split_of(g, "train").items()}
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        cip.fit_probes(data, [(0, "image_cal")])
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        cip.run_probe(data, data, ["a", "b", "c"], (0,))
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        cip.bootstrap_differences(np.array([0, 1]), np.array([0.2, 0.6]), np.array([0.3, 0.7]), 2, 0)
