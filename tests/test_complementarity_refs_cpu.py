"""CPU: the numpy restatement of the complementarity kernels and of the 16-cell derivation (tests/complementarity_refs.py) pinned on the
reference's fixture (tests/golden/complementarity.npz, written by tests/golden/make_golden_complementarity.py from the reference's own
functions), and the host half of the module: `analyze_pathology` from the cells, the report text, the CSV, the options, the argument
checks made before any launch and the refusal to run without a GPU.

Thresholds, J and every integer compare exactly: the restatement performs the IEEE operations sklearn performs.  Derived floats are
quotients of the same integers in the same order, so they are equal too; only `err_corr` sums its rows in another order (cell after
cell, not patient after patient), which moves it by a few n 2^-53 at n = 300: bound 1e-12."""
import contextlib
import csv
import io
import json
import os

import numpy as np
import pytest
import torch

from complementarity_refs import (HEADS, VENN_IDS, assert_rows_match, cells_ref, expand_cells, golden, golden_cases, golden_rows, golden_split,
                                  rows_from_predictions, same_bits, venn_ref, youden_ref, youden_table_ref)

VARIANTS = (("rows", "mask"), ("rows_alt", "mask_alt"))


def _comp():
    from multimodal_edema_prediction_amd import complementarity
    return complementarity


def _labels():
    return [str(s) for s in golden()["labels"]]


def _cells(mask_key):
    g = golden()
    test = golden_split("test")
    scores = np.stack([test[h] for h in HEADS])
    return cells_ref(scores, test["y"], g[f"test_{mask_key}"], g["thresholds"])


def test_youden_restatement_gives_the_reference_threshold_on_every_case():
    cases = golden_cases()
    assert len(cases) >= 50
    n_inf = n_nan = 0
    for i, c in enumerate(cases):
        thr, j, L, P = youden_ref(c["z"], c["y"], c["mask"])
        assert same_bits(thr, c["thr"]) and same_bits(j, c["j"]), (i, thr, c["thr"], j, c["j"])
        assert L == int((c["mask"] != 0).sum()) and P == int(((c["mask"] != 0) & (c["y"] != 0)).sum())
        n_inf += np.isinf(thr)
        n_nan += np.isnan(thr)
    assert n_inf >= 2 and n_nan >= 4
    print(f"{len(cases)} cases, {n_inf} at +inf, {n_nan} NaN")


def test_the_cases_tell_the_wrong_variants_apart():
    cases = golden_cases()
    a, b = cases[0], cases[1]
    assert a["thr"] == 1.5 and youden_ref(a["z"], a["y"], a["mask"], drop=False)[0] == 0.5           # drop_intermediate decides
    assert b["thr"] == 0.5 and youden_ref(b["z"], b["y"], b["mask"], exact=True)[0] == 1.0           # the fp64 rounding of J decides
    differ = lambda c, **kw: not same_bits(youden_ref(c["z"], c["y"], c["mask"], **kw)[0], c["thr"])  # noqa: E731
    assert sum(differ(c, drop=False) for c in cases) >= 1 and sum(differ(c, exact=True) for c in cases) >= 1


def test_thresholds_of_the_pair():
    g, val = golden(), golden_split("val")
    thr, j, counts = youden_table_ref(np.stack([val[h] for h in HEADS]), val["y"], val["mask"])
    assert all(same_bits(a, b) for a, b in zip(thr.ravel(), g["thresholds"].ravel()))
    assert np.isinf(thr[1, 0]) and j[1, 0] == 0.0 and np.isnan(thr[:, 2]).all() and np.isnan(j[:, 2]).all()
    assert np.array_equal(counts[:, 0], (val["mask"] != 0).sum(0)) and counts[2, 1] == 0


@pytest.mark.parametrize("rows_key,mask_key", VARIANTS)
def test_analyze_pathology_from_the_cells_gives_the_reference_rows(rows_key, mask_key):
    g, comp = golden(), _comp()
    cells = _cells(mask_key)
    want = golden_rows(rows_key)
    assert np.array_equal(cells.sum(1), (g[f"test_{mask_key}"] != 0).sum(0))
    got = [comp.analyze_pathology(label, cells[k]) for k, label in enumerate(_labels())]
    worst = assert_rows_match(got, want, 1e-12)
    restated = [rows_from_predictions(label, *expand_cells(cells[k])) for k, label in enumerate(_labels())]
    assert_rows_match(restated, want, 1e-12)
    exact = [{k: v for k, v in r.items() if k != "err_corr"} for r in got]
    assert_rows_match(exact, [{k: v for k, v in r.items() if k != "err_corr"} for r in want], 0.0)      # same integers, same quotients
    print(f"{rows_key}: largest float deviation {worst:.3e} (err_corr; bound 1e-12)")
    if rows_key == "rows":
        assert got[1]["n"] == 0 and "both_agree_broken" in got[1] and "both_agree_broken_rate" not in got[1]
    for k in range(len(want)):
        stored = g[f"{rows_key}_venn"][k]
        for counts in (comp.venn_counts(cells[k]), venn_ref(cells[k])):
            assert list(counts) == list(VENN_IDS)
            if stored[0] < 0:                                                    # `_plot_venn` draws nothing: no known positive
                assert sum(counts.values()) == 0
            else:
                assert [counts[r] for r in VENN_IDS] == stored.tolist()


@pytest.mark.parametrize("rows_key,mask_key", VARIANTS)
def test_report_and_csv_are_the_references(rows_key, mask_key, tmp_path):
    g, comp = golden(), _comp()
    cells = _cells(mask_key)
    rows = [comp.analyze_pathology(label, cells[k]) for k, label in enumerate(_labels())]
    thresholds = {h: g["thresholds"][i] for i, h in enumerate(HEADS)}
    buffer = io.StringIO()
    with contextlib.redirect_stdout(buffer):
        comp.print_report(rows, thresholds, _labels())
    assert buffer.getvalue() == str(g[f"{rows_key}_stdout"])
    path = os.path.join(str(tmp_path), "c.csv")
    with contextlib.redirect_stdout(io.StringIO()):
        comp.save_csv(rows, path)
    got = list(csv.DictReader(open(path, newline="")))
    want = list(csv.DictReader(io.StringIO(str(g[f"{rows_key}_csv"]), newline="")))
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert list(a) == list(b)
        for key in b:
            if key == "err_corr" and b[key] not in ("", "nan"):
                assert abs(float(a[key]) - float(b[key])) <= 1e-12
            else:
                assert a[key] == b[key], (key, a[key], b[key])


def test_options_are_the_references():
    comp = _comp()
    want = json.loads(str(golden()["options_json"]))
    got = vars(comp.parse_args(["--ckpt", "best.pt", "--outdir", "out"]))
    assert got == want and list(got) == list(want)
    assert comp.parse_args(["--ckpt", "a", "--outdir", "b", "--threshold", "fixed", "--labels", "edema"]).threshold == "fixed"
    with pytest.raises(SystemExit):
        comp.parse_args(["--ckpt", "a", "--outdir", "b", "--threshold", "median"])
    labels = _labels()
    assert comp.resolve_labels("", labels) == (0, 1, 2) and comp.resolve_labels(" Label_Effusion,label_edema", labels) == (2, 0)
    with pytest.raises(SystemExit):
        comp.resolve_labels("edema", labels)                                     # the reference takes full names only


def test_bad_arguments_are_refused_before_any_launch():
    from multimodal_edema_prediction_amd import abi
    L = abi.lib()
    q = 4096                                                                     # a non-null token: nothing is dereferenced on a refusal
    assert L.medp_youden_thresholds(None, q, q, q, q, q, 3, 8, 2, None) < 0 and b"null" in L.medp_last_error()
    assert L.medp_youden_thresholds(q, q, q, q, q, None, 3, 8, 2, None) < 0
    for H, N, K in ((0, 8, 2), (3, 0, 2), (3, 8, 0), (-1, 8, 2)):
        assert L.medp_youden_thresholds(q, q, q, q, q, q, H, N, K, None) < 0
    assert L.medp_complementarity_cells(q, q, q, None, q, 8, 2, None) < 0 and b"null" in L.medp_last_error()
    for N, K in ((0, 2), (8, 0), (8, -3)):
        assert L.medp_complementarity_cells(q, q, q, q, q, N, K, None) < 0
    comp = _comp()
    assert comp.YOUDEN_MAX_LEN == 16384
    with pytest.raises(ValueError, match="16 counts"):
        comp.analyze_pathology("x", np.zeros(8))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_there_is_no_cpu_fallback(tmp_path):
    comp = _comp()
    val = {k: torch.as_tensor(np.array(v)) for k, v in golden_split("val").items()}
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        comp.main(["--ckpt", os.path.join(str(tmp_path), "best.pt"), "--outdir", os.path.join(str(tmp_path), "out")])
    assert not os.path.exists(os.path.join(str(tmp_path), "out"))
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        comp.run_complementarity(val, val, _labels())
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        comp.derive_thresholds(val, "youden")
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        comp.contingency_cells(val, {h: np.zeros(3) for h in HEADS})
