"""GPU: the modality complementarity analysis end to end on the reference's fixture (tests/golden/complementarity.npz: the reference's
own `_derive_thresholds`, `_binarize`, `_analyze_pathology`, `_print_report`, `_save_csv` and `_plot_venn` on one seeded val / test
pair, tests/golden/make_golden_complementarity.py) and on a small saved `train_synthetic` teacher.

Bounds
  thresholds, every integer field, the Venn counts   exact.
  derived floats                                      1e-12 absolute: quotients of the same integers in the same order; only
                                                      `err_corr` sums its rows in another order (cell after cell), which moves it by a
                                                      few n 2^-53 at n = 300.
  NaN where the reference has NaN; the report text equals the recorded text."""
import argparse
import contextlib
import csv
import io
import os

import numpy as np
import pytest
import torch

from complementarity_refs import HEADS, VENN_IDS, assert_rows_match, golden, golden_rows, golden_split, same_bits
from tests_dual_common import cxr_head_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
_state = {}


def _comp():
    from multimodal_edema_prediction_amd import complementarity
    return complementarity


def _labels():
    return [str(s) for s in golden()["labels"]]


def _data(split, mask_key="mask"):
    key = (split, mask_key)
    if key not in _state:
        d = dict(golden_split(split))
        d["mask"] = golden()[f"{split}_{mask_key}"]
        _state[key] = {k: torch.as_tensor(np.array(v), device=DEV) for k, v in d.items()}
    return _state[key]


@pytest.mark.parametrize("rows_key,mask_key", [("rows", "mask"), ("rows_alt", "mask_alt")])
def test_run_complementarity_against_the_reference(rows_key, mask_key):
    g, comp = golden(), _comp()
    rows, thresholds, archive = comp.run_complementarity(_data("val"), _data("test", mask_key), _labels())
    for i, h in enumerate(HEADS):
        print(f"{h}: thresholds {thresholds[h].tolist()} (reference {g['thresholds'][i].tolist()})")
        assert all(same_bits(a, b) for a, b in zip(thresholds[h], g["thresholds"][i]))
        assert all(same_bits(a, b) for a, b in zip(archive["thresholds"][i], g["thresholds"][i]))
    assert np.isinf(thresholds["ts"][0]) and np.isnan(archive["thresholds"][:, 2]).all()
    want = golden_rows(rows_key)
    worst = assert_rows_match(rows, want, 1e-12)
    strip = lambda rs: [{k: v for k, v in r.items() if k != "err_corr"} for r in rs]  # noqa: E731
    assert_rows_match(strip(rows), strip(want), 0.0)
    print(f"{rows_key}: largest float deviation {worst:.3e} (err_corr; bound 1e-12)")
    buffer = io.StringIO()
    with contextlib.redirect_stdout(buffer):
        comp.print_report(rows, thresholds, _labels())
    assert buffer.getvalue() == str(g[f"{rows_key}_stdout"])
    stored = g[f"{rows_key}_venn"]
    for k in range(3):
        assert archive["venn"][k].tolist() == (stored[k].tolist() if stored[k, 0] >= 0 else [0] * 7)
    mask = g[f"test_{mask_key}"]
    assert archive["cells"].shape == (3, 16) and np.array_equal(archive["cells"].sum(1), (mask != 0).sum(0))
    assert np.array_equal(archive["val_counts"][:, 0], (g["val_mask"] != 0).sum(0)) and archive["val_counts"][2, 1] == 0
    assert archive["youden_j"][1, 0] == 0.0 and np.isnan(archive["youden_j"][:, 2]).all()
    assert [str(s) for s in archive["venn_ids"]] == list(VENN_IDS)


def test_filter_fixed_thresholds_and_the_two_entry_points():
    g, comp = golden(), _comp()
    rows, thresholds, archive = comp.run_complementarity(_data("val"), _data("test"), _labels(), labels="label_effusion, LABEL_EDEMA")
    want = golden_rows("rows")
    assert_rows_match(rows, [want[2], want[0]], 1e-12)                          # the request's order; thresholds of all labels in the archive
    assert all(same_bits(a, b) for a, b in zip(thresholds["img"], g["thresholds"][0][[2, 0]])) and archive["thresholds"].shape == (3, 3)
    with pytest.raises(SystemExit):
        comp.run_complementarity(_data("val"), _data("test"), _labels(), labels="label_nope")
    with pytest.raises(ValueError, match="Unknown threshold method"):
        comp.run_complementarity(_data("val"), _data("test"), _labels(), threshold="median")
    derived = comp.derive_thresholds(_data("val"), "youden")
    assert list(derived) == list(HEADS) and all(same_bits(a, b) for i, h in enumerate(HEADS) for a, b in zip(derived[h], g["thresholds"][i]))
    cells = comp.contingency_cells(_data("test"), derived)
    assert np.array_equal(cells, archive["cells"])
    fixed = comp.derive_thresholds(_data("val"), "fixed")
    assert all(np.array_equal(fixed[h], np.zeros(3)) for h in HEADS)
    rows_fixed, thr_fixed, arch_fixed = comp.run_complementarity(_data("val"), _data("test"), _labels(), threshold="fixed")
    test = golden_split("test")
    known = test["mask"][:, 0] != 0
    agree = ((test["img"][known, 0] > 0) == (test["y"][known, 0] != 0)).mean()
    assert rows_fixed[0]["img_acc"] == float(agree) and (thr_fixed["fus"] == 0).all() and np.isnan(arch_fixed["youden_j"]).all()


def _teacher_args(tmp, perceiver_type):
    from multimodal_edema_prediction_amd import train_synthetic
    head = os.path.join(str(tmp), "cxr_head.pt")
    torch.save(cxr_head_state(), head)
    return train_synthetic.parse_args(["teacher", "--ckpt_dir", str(tmp), "--perceiver_type", perceiver_type, "--n_timesteps", "32",
                                       "--n_vars", "16", "--d_static", "8", "--n_train", "8", "--n_val", "40", "--n_test", "40",
                                       "--pretrained_cxr_head_ckpt", head, "--perceiver_dropout", "0.0", "--head_dropout", "0.0",
                                       "--freeze_duett"])


def test_main_writes_both_files(tmp_path):
    from multimodal_edema_prediction_amd import checkpoint, train_synthetic
    from multimodal_edema_prediction_amd.conditional_information_probe import gather
    comp = _comp()
    args = _teacher_args(tmp_path, "dual")
    torch.manual_seed(0)
    teacher = train_synthetic.build_teacher(args, torch.device(DEV))
    ckpt = os.path.join(str(tmp_path), "best.pt")
    checkpoint.save_ckpt(ckpt, teacher, argparse.Namespace(state_dict=lambda: {}), 1, 0.5, args)
    outdir = tmp_path / "out"
    common = ["--ckpt", ckpt, "--batch_size", "8", "--num_workers", "0"]
    result = comp.main(common + ["--outdir", str(outdir)])
    assert sorted(os.listdir(outdir)) == ["complementarity.csv", "complementarity.npz"]
    labels = [s.strip() for s in args.pathology_labels.split(",")]
    K = len(labels)
    table = list(csv.DictReader(open(outdir / "complementarity.csv", newline="")))
    assert [r["label"] for r in table] == labels and list(table[0]) == list(result["rows"][0])
    datasets = dict(zip(("train", "val", "test"), train_synthetic._datasets(args)))
    loader = lambda split: train_synthetic.make_loader(datasets[split], 8, False, 0, "teacher", 0, 1)  # noqa: E731
    teacher.eval()
    val, test = gather(teacher, loader("val"), torch.device(DEV)), gather(teacher, loader("test"), torch.device(DEV))
    again = comp.derive_thresholds(val, "youden")
    with np.load(outdir / "complementarity.npz") as z:
        assert set(z.files) == {"labels", "heads", "venn_ids", "thresholds", "youden_j", "val_counts", "cells", "venn"}
        assert z["thresholds"].shape == (3, K) and z["cells"].shape == (K, 16) and z["venn"].shape == (K, 7)
        known = (test["mask"] != 0).sum(0).cpu().numpy()
        print("known test rows per label", known.tolist(), "thresholds", z["thresholds"].tolist())
        assert np.array_equal(z["cells"].sum(1), known) and z["cells"].sum() > 0
        for i, h in enumerate(HEADS):
            assert all(same_bits(a, b) for a, b in zip(z["thresholds"][i], again[h]))
        assert np.array_equal(z["venn"].sum(1), z["cells"][:, 3::2].sum(1))        # positives any head catches: the odd cells but cell 1
    assert [int(r["n"]) for r in table] == known.tolist()
    out2 = tmp_path / "out2"
    picked = comp.main(common + ["--outdir", str(out2), "--labels", labels[1], "--threshold", "fixed"])
    assert [r["label"] for r in picked["rows"]] == [labels[1]] and (picked["archive"]["thresholds"] == 0).all()
    with pytest.raises(SystemExit):
        comp.main(common + ["--outdir", str(out2), "--labels", "label_nope"])
    with pytest.raises(SystemExit):
        comp.main(common + ["--outdir", str(out2), "--val_split", "dev"])
    with pytest.raises(SystemExit):
        comp.main(common + ["--outdir", str(out2), "--test_split", "holdout"])


def test_main_refuses_a_teacher_that_is_not_dual(tmp_path):
    from multimodal_edema_prediction_amd import checkpoint
    comp = _comp()
    args = _teacher_args(tmp_path, "dual")
    args.perceiver_type = "single"
    ckpt = os.path.join(str(tmp_path), "single.pt")
    checkpoint.save_ckpt(ckpt, torch.nn.Linear(1, 1), argparse.Namespace(state_dict=lambda: {}), 1, 0.5, args)
    with pytest.raises(SystemExit, match="dual"):
        comp.main(["--ckpt", ckpt, "--outdir", str(tmp_path / "o")])
