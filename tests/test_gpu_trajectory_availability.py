"""GPU: the trajectory-availability audit end to end (multimodal_edema_prediction_amd/trajectory_availability.py) against the reference's
own `audit_dataset`, `_print_summary` and CSV files, recorded in tests/golden/trajectory_availability.npz.

Bounds (those of tests/test_trajectory_availability_refs_cpu.py): every column == with NaN matching NaN, row order included, except
`median_within_patient_std_if_2plus`, which the kernel computes in fp64 and the reference in fp32: within 16 * 2^-24 * max|value of that
variable|.  The summary prints none of the std column, so its text must equal the recorded text."""
import contextlib
import io

import numpy as np
import pytest
import torch

from trajectory_availability_refs import PS_COLUMNS, PV_COLUMNS, assert_csv, assert_tables, golden_cases, parse_csv, std_bounds

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = golden_cases()
IDS = [f"N{c['x'].shape[0]}_T{c['x'].shape[1]}_V{c['x'].shape[2] // 2}_nt{c['n_timesteps']}" for c in CASES]
_audits = {}


def _ta():
    from multimodal_edema_prediction_amd import trajectory_availability
    return trajectory_availability


def _audit(c):
    """The audit of case c from a device tensor, run once and shared."""
    if c not in _audits:
        _audits[c] = _ta().audit_dataset(torch.as_tensor(CASES[c]["x"], device=DEV), CASES[c]["names"], CASES[c]["n_timesteps"])
    return _audits[c]


def _want(c):
    return CASES[c]["per_variable"], CASES[c]["per_sample"]


@pytest.mark.parametrize("c", range(len(CASES)), ids=IDS)
def test_audit_of_a_tensor_against_the_reference(c):
    assert_tables(_audit(c), _want(c), std_bounds(CASES[c]), "tensor")


@pytest.mark.parametrize("c", range(len(CASES)), ids=IDS)
def test_audit_of_a_dataset_and_of_a_tuple_against_the_reference(c, monkeypatch):
    ta, case = _ta(), CASES[c]
    monkeypatch.setattr(ta, "CHUNK", 16)                                            # several chunks, a ragged last one
    items = [torch.from_numpy(case["x"][i]) for i in range(len(case["x"]))]
    dataset = [{"x_ts": x, "y": torch.zeros(())} for x in items]
    from_dataset = ta.audit_dataset(dataset, case["names"], case["n_timesteps"])
    from_tuple = ta.audit_dataset(tuple(items), case["names"], case["n_timesteps"])
    assert_tables(from_dataset, _want(c), std_bounds(case), "dataset")
    for got in (from_dataset, from_tuple):                                          # chunked or not: the same bits, the std column too
        for table, whole in zip(got, _audit(c)):
            for k in table:
                assert np.array_equal(table[k], whole[k], equal_nan=np.asarray(whole[k]).dtype.kind == "f"), k


def test_max_samples_and_ragged_windows():
    ta, case = _ta(), CASES[0]
    x = torch.as_tensor(case["x"], device=DEV)
    head = ta.audit_dataset(x, case["names"], case["n_timesteps"], max_samples=20)
    alone = ta.audit_dataset(x[:20], case["names"], case["n_timesteps"])
    assert len(head[1]["sample_index"]) == 20 and (head[0]["n_samples"] == 20).all()
    for table, want in zip(head, alone):
        for k in table:
            assert np.array_equal(table[k], want[k], equal_nan=np.asarray(want[k]).dtype.kind == "f"), k
    items = [torch.from_numpy(case["x"][i]) for i in range(4)]
    items[2] = items[2][:-1]
    with pytest.raises(ValueError, match="one length"):
        ta.audit_dataset(items, case["names"], case["n_timesteps"])
    with pytest.raises(ValueError):
        ta.audit_dataset(x, case["names"][:-1], case["n_timesteps"])


@pytest.mark.parametrize("c", range(len(CASES)), ids=IDS)
def test_print_summary_is_the_recorded_text(c):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _ta().print_summary(*_audit(c), f"case{c}")
    assert out.getvalue() == CASES[c]["stdout"]


@pytest.mark.parametrize("c", range(len(CASES)), ids=IDS)
def test_csv_files_against_the_references(c, tmp_path):
    ta = _ta()
    pv, ps = str(tmp_path / "audit.csv"), str(tmp_path / "audit_per_sample.csv")
    ta.save_csv(_audit(c)[0], pv)
    ta.save_csv(_audit(c)[1], ps)
    assert_csv(open(pv).read(), CASES[c]["csv_pv"], std_bounds(CASES[c]), "per_variable csv")
    assert open(ps).read() == CASES[c]["csv_ps"]


def test_main_on_a_tiny_synthetic_cohort(tmp_path, capsys):
    ta = _ta()
    out_csv = str(tmp_path / "avail.csv")
    result = ta.main(["--n_train", "64", "--n_timesteps", "24", "--n_vars", "6", "--out_csv", out_csv])
    text = capsys.readouterr().out
    assert "=== 24 h trajectory availability: split=train, n=64 ===" in text and "\nVerdict: " in text
    assert text.endswith(f"\nSaved: {out_csv}\nSaved: {str(tmp_path / 'avail_per_sample.csv')}\n")
    header, rows = parse_csv(open(out_csv).read())
    assert tuple(header) == PV_COLUMNS and len(rows) == 6 and sorted(r[0] for r in rows) == [f"var_{i}" for i in range(6)]
    assert all(r[1] == "64" for r in rows)
    rates = [float(r[3]) for r in rows]
    assert rates == sorted(rates, reverse=True) and all(0.0 < v <= 1.0 for v in rates)     # 24 hours at p = 0.2: trajectories exist
    header, rows = parse_csv(open(str(tmp_path / "avail_per_sample.csv")).read())
    assert tuple(header) == PS_COLUMNS and [int(r[0]) for r in rows] == list(range(64))
    # against the restatement, on the very windows main() read
    from multimodal_edema_prediction_amd.cohort import CohortCfg, make_item
    from trajectory_availability_refs import audit_ref
    cfg = CohortCfg(n_timesteps=24, n_vars=6, d_static=8, image_size=0, n_labels=7, seed=1234, learnable=False)
    x = np.stack([make_item(cfg, i, with_image=False)["x_ts"].numpy() for i in range(64)])
    want = audit_ref(x, [f"var_{i}" for i in range(6)], 24)
    bounds = std_bounds({"x": x, "names": [f"var_{i}" for i in range(6)]})
    assert_tables((result["per_variable"], result["per_sample"]), want, bounds, "main")
