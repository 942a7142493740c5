"""CPU: the numpy restatement of the trajectory-availability audit (tests/trajectory_availability_refs.py) and the host half of
multimodal_edema_prediction_amd/trajectory_availability.py (layout of the summary, the CSV files, the command line) against the
reference's own output, tests/golden/trajectory_availability.npz.

Every column compares == (NaN matching NaN) except `median_within_patient_std_if_2plus`: the restatement and the kernel compute that std
in fp64 and round once, the reference in fp32, so it compares within 16 * 2^-24 * max|value of that variable| (refs.std_bounds)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from trajectory_availability_refs import (PS_COLUMNS, PV_COLUMNS, assert_csv, assert_tables, audit_ref, cells_ref, golden_cases, median_ref,
                                          std_bounds)

from multimodal_edema_prediction_amd import trajectory_availability as ta

CASES = golden_cases()
IDS = [f"N{c['x'].shape[0]}_T{c['x'].shape[1]}_V{c['x'].shape[2] // 2}_nt{c['n_timesteps']}" for c in CASES]


def test_fixture_holds_the_cases_the_audit_can_get_wrong():
    shapes = [(c["x"].shape[0], c["x"].shape[1], c["x"].shape[2] // 2, c["n_timesteps"]) for c in CASES]
    assert shapes == [(37, 24, 6, 24), (40, 24, 6, 30), (5, 3, 4, 3), (1, 2, 3, 2), (130, 96, 5, 96)]
    keys = [list(zip(c["per_variable"]["trajectory_2plus_rate"], c["per_variable"]["any_observed_rate"])) for c in CASES]
    assert any(len(set(k)) < len(k) for k in keys), "no tied sort keys"
    assert any(np.isnan(c["per_variable"]["median_recency_h_if_observed"]).any() for c in CASES), "no all-NaN median"
    assert any((c["per_variable"]["median_within_patient_std_if_2plus"] == 0.0).any() for c in CASES), "no constant variable"
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "trajectory_availability.npz")) < 512 * 1024


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_the_reference(case):
    got = audit_ref(case["x"], case["names"], case["n_timesteps"])
    assert_tables(got, (case["per_variable"], case["per_sample"]), std_bounds(case), "restatement")


def test_restatement_ignores_values_at_unobserved_cells():
    case = CASES[0]
    x = case["x"].copy()
    v = x.shape[2] // 2
    hidden = x[:, :, v:] <= 0
    x[:, :, :v][hidden] = np.where(np.arange(hidden.sum()) % 2 == 0, np.nan, np.inf).astype(np.float32)
    a, b = cells_ref(case["x"], case["n_timesteps"]), cells_ref(x, case["n_timesteps"])
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
def test_median_rule_is_numpys(dtype):
    rng = np.random.default_rng(3)
    for m in (1, 2, 3, 4, 7, 10, 255, 256):
        col = (rng.standard_normal(m) * 9).astype(dtype)
        want = float(np.median(col)) if dtype == np.int32 else float(np.nanmedian(col))
        assert median_ref(col) == (want, m)
        assert median_ref(col, take_abs=True)[0] == float(np.median(np.abs(col)))
    if dtype == np.float32:
        col = np.array([np.nan, 3.0, np.nan, 1.0, 2.0, 8.0], dtype=np.float32)
        assert median_ref(col) == (2.5, 4)
        assert np.isnan(median_ref(np.full(5, np.nan, dtype=np.float32))[0]) and median_ref(np.full(5, np.nan, dtype=np.float32))[1] == 0
        big = np.array([3e38, 3e38, 3e38], dtype=np.float32)
        with np.errstate(over="ignore"):
            assert median_ref(big)[0] == float(np.median(big)) == float(np.float32(3e38))    # an odd count averages one element: no overflow
            assert median_ref(big[:2])[0] == float(np.median(big[:2])) == float("inf")       # an even one adds in fp32, as numpy does


@pytest.mark.parametrize("c", range(len(CASES)), ids=IDS)
def test_print_summary_character_for_character(c):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ta.print_summary(CASES[c]["per_variable"], CASES[c]["per_sample"], f"case{c}")
    assert out.getvalue() == CASES[c]["stdout"]


def test_print_summary_tables_of_more_than_15_rows_and_long_names():
    """The layout rule on what the fixture's small V cannot show: head and tail differ, a long name widens its column (`to_string` cuts
    no cell), a negative figure."""
    V = 17
    pv = {k: np.linspace(1.0, 0.0, V) for k in PV_COLUMNS[1:]}
    pv["variable"] = np.array(["v" * (60 if j == 2 else j + 1) for j in range(V)], dtype=object)
    pv["median_recency_h_if_observed"] = np.where(np.arange(V) > 12, np.nan, -np.arange(V) - 0.5)
    ps = {k: np.arange(4, dtype=np.int64) * (i + 1) for i, k in enumerate(PS_COLUMNS)}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ta.print_summary(pv, ps, "train")
    lines = out.getvalue().split("\n")
    assert lines[3] == "Per patient median: observed variables=3, >=2h variables=4, >=3h variables=6"
    top, tail = lines[6:22], lines[24:40]
    assert lines[5] == "Top variables with usable trajectories" and lines[23] == "Variables with little/no usable trajectory"
    assert len({len(s) for s in top}) == 1 and len({len(s) for s in tail}) == 1
    assert top[3].startswith("v" * 60 + "  ") and top[0].startswith(" " * 52 + "variable  any_observed_rate")
    assert top[1].endswith(" -0.500") and tail[-1].endswith(" NaN") and tail[2].lstrip().startswith("vvvv ")
    assert lines[41] == "Verdict: SPARSE: trajectory modeling is plausible for only a small variable subset."


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_csv_files_are_the_references(case, tmp_path):
    pv, ps = str(tmp_path / "a.csv"), str(tmp_path / "a_per_sample.csv")
    ta.save_csv(case["per_variable"], pv)
    ta.save_csv(case["per_sample"], ps)
    assert open(pv).read() == case["csv_pv"]                       # the golden tables themselves: every field, the std column too
    assert open(ps).read() == case["csv_ps"]
    assert_csv(open(pv).read(), case["csv_pv"], std_bounds(case), "per_variable csv")


def test_command_line_names_and_defaults():
    a = ta.parse_args([])
    assert (a.split, a.max_samples, a.out_csv, a.n_timesteps) == ("train", 0, "trajectory_availability.csv", 24)
    assert ta.parse_args(["--split", "all", "--max_samples", "7"]).max_samples == 7
    with pytest.raises(SystemExit):
        ta.parse_args(["--split", "holdout"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_cpu_fallback():
    from multimodal_edema_prediction_amd import probe_stats
    case = CASES[2]
    with pytest.raises(RuntimeError):
        ta.audit_dataset(torch.from_numpy(case["x"]), case["names"], case["n_timesteps"])
    with pytest.raises(RuntimeError):
        ta.trajectory_cells(torch.from_numpy(case["x"]), case["n_timesteps"])
    with pytest.raises(RuntimeError):
        probe_stats.column_medians(torch.zeros(2, 5))
    with pytest.raises(RuntimeError):
        ta.main(["--n_train", "8"])
