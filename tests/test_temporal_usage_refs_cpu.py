"""CPU: the host half of the temporal-usage diagnostics against the reference's fixture (tests/golden/temporal_usage.npz, written by the
reference's own functions: tests/golden/make_golden_temporal_usage.py).

  the ported draws equal the reference's permutations exactly;
  the fp64 restatements of the summary kernel's formulas (tests/temporal_usage_refs.py) reproduce the reference's sections [3] / [4]:
    correlation to 1e-10 (numpy's corrcoef runs in fp64 on the fp32 probabilities: the same numbers, other summation order);
    means and entropies to 1e-5: the reference accumulates those in fp32, <= (S + log2 N) 2^-24 relative (~2e-6 at S = 24, N = 240);
  `residual_by_confidence` prints the reference's text character for character;
  the assembly wrapper refuses a ragged `ts_shuffle` pairing before it needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from temporal_usage_refs import CONDITIONS, entropy_ref, golden, golden_draws, golden_pred, make_batch, prob_ref, sens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dtu():
    from multimodal_edema_prediction_amd import diagnose_temporal_usage
    return diagnose_temporal_usage


def test_conditions_and_limits_agree_with_the_fixture_and_the_header():
    dtu = _dtu()
    assert dtu.CONDITIONS == CONDITIONS == tuple(str(c) for c in golden()["conditions"])
    header = open(os.path.join(ROOT, "include", "medp_hip.h")).read()
    defined = {k: v for k, v in re.findall(r"#define (MEDP_\w+) (\(1 << \d+\)|\d+)", header)}
    assert int(defined["MEDP_COUNTERFACTUAL_CONDITIONS"]) == len(dtu.CONDITIONS)
    assert eval(defined["MEDP_TEMPORAL_USAGE_MAX_N"]) == dtu.SUMMARY_MAX_N and int(defined["MEDP_TEMPORAL_USAGE_MAX_S"]) == dtu.SUMMARY_MAX_S


def test_the_draws_are_the_references():
    dtu = _dtu()
    seed = int(golden()["cfg"][6])
    cases = golden_draws()
    assert len(cases) == 4
    for case in cases:
        rng = np.random.default_rng(seed + dtu.BATCH_SEED_STRIDE * case["batch_idx"])
        perm = dtu.different_subject_permutation(case["subjects"], rng)
        tperms = dtu.time_permutations(case["lengths"], rng)
        assert np.array_equal(perm, case["perm"]), case["subjects"]
        assert len(tperms) == len(case["tperm"]) and all(np.array_equal(a, b) for a, b in zip(tperms, case["tperm"]))
        assert int(np.sum(case["subjects"][perm] == case["subjects"])) == case["same_subject"]
    fallback = [c for c in cases if c["subjects"].tolist() == [1, 1, 1, 2, 3]][0]
    assert fallback["same_subject"] == 1 and np.array_equal(fallback["perm"], np.roll(np.arange(5), 2))      # no derangement exists: cyclic shift
    single = [c for c in cases if len(c["subjects"]) == 1][0]
    assert single["perm"].tolist() == [0] and single["tperm"][0].tolist() == [0]
    assert any(len(set(c["lengths"])) > 1 for c in cases)                                                 # a ragged batch


def test_restatements_reproduce_the_references_sensitivity_and_entropy():
    g = golden()
    p_fus = np.stack([prob_ref(g[f"fus_{c}"]).T for c in CONDITIONS])                    # [C, K, N]
    p_ts = np.stack([prob_ref(g[f"ts_{c}"]).T for c in CONDITIONS])
    assert p_fus.dtype == np.float32
    sens = sens_ref(p_fus, p_ts)
    want = g["sens"]
    d_mean = max(np.abs(sens[..., 0] - want[..., 0]).max(), np.abs(sens[..., 2] - want[..., 2]).max())
    d_corr = np.abs(sens[..., 1] - want[..., 1]).max()
    entropy = entropy_ref(g["attention"])
    d_entropy = np.abs(entropy - g["entropy"]).max()
    print(f"sensitivity means {d_mean:.3e} (bound 1e-5), correlation {d_corr:.3e} (bound 1e-10), entropy {d_entropy:.3e} (bound 1e-5)")
    assert d_mean <= 1e-5 and d_corr <= 1e-10 and d_entropy <= 1e-5
    assert abs(entropy[1] - 1.0) <= 1e-6                                                  # the fixture's uniform label
    # the rules the kernel shares: constant column, a single row, a single weight
    flat = np.stack([np.full((1, 5), 0.25), np.linspace(0.1, 0.9, 5)[None]])
    assert np.isnan(sens_ref(flat, flat)[0, 0, 1]) and np.isnan(sens_ref(flat[:, :, :1], flat[:, :, :1])[0, 0, 1])
    assert entropy_ref(np.ones((3, 2, 1), np.float32)).tolist() == [0.0, 0.0]


def test_residual_by_confidence_prints_the_references_text(tmp_path, capsys):
    from multimodal_edema_prediction_amd import residual_by_confidence
    g = golden()
    labels = [str(s) for s in g["labels"]]
    path = str(tmp_path / "pred.npz")
    np.savez_compressed(path, **_dtu().npz_payload(golden_pred(g), labels))
    with np.load(path) as z:
        assert set(z.files) == {"subject_ids", "labels", "y", "mask", "img_full", "ts_attention_full"} | {
            f"{h}_{c}" for h in ("fus", "ts") for c in CONDITIONS}
    capsys.readouterr()
    table = residual_by_confidence.main(["--input_npz", path])
    assert capsys.readouterr().out == str(g["residual_stdout"])
    assert [t["label"] for t in table] == labels and all(len(t["quartiles"]) == 4 for t in table)
    known = g["mask"].astype(bool).sum(0)
    assert [sum(q["n"] for q in t["quartiles"]) for t in table] == known.tolist()


def test_ragged_ts_shuffle_pairing_raises_before_a_gpu_is_needed():
    dtu = _dtu()
    x_ts, x_static, bin_ends = make_batch([5, 9, 3])
    tperms = [np.arange(n) for n in (5, 9, 3)]
    with pytest.raises(ValueError, match="ts_shuffle"):
        dtu.counterfactual_inputs(None, x_ts, x_static, bin_ends, [1, 2, 0], tperms)
    with pytest.raises(ValueError, match="one entry per step"):
        dtu.counterfactual_inputs(None, x_ts, x_static, bin_ends, [0, 1, 2], tperms[::-1])
    with pytest.raises(ValueError, match="unknown conditions"):
        dtu.counterfactual_inputs(None, x_ts, x_static, bin_ends, [0, 1, 2], tperms, conditions=("full", "image_shuffle"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
            dtu.summarise(golden_pred(), [str(s) for s in golden()["labels"]], 0, 0)
