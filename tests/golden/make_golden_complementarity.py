#!/usr/bin/env python3
"""Golden fixture for the modality complementarity analysis (analysis/complementarity.py): runs the REFERENCE'S OWN functions
(`_youden_threshold`, `_derive_thresholds`, `_binarize`, `_analyze_pathology`, `_print_report`, `_save_csv`, `_plot_venn`, `parse_args`;
stubs as in make_golden.py) and stores numbers and recorded text only in tests/golden/complementarity.npz.

`matplotlib_venn` is not installed: a recording stand-in of `venn3` is installed before the import, so `_plot_venn` runs and the seven
counts it writes into the diagram's labels are read back from it.

Stored
  cases     threshold cases (scores fp32, labels, mask; concatenated, `case_len` splits them) with the threshold the reference derives
            (`_derive_thresholds`' rule: fewer than two known rows -> NaN, else `_youden_threshold`) and max(tpr - fpr) of sklearn's
            `roc_curve`.  The first two are the issue's: one where `drop_intermediate` decides (1.5, without the drop rule 0.5), one
            where the fp64 rounding of tp / P - fp / N decides (0.5, as rationals 1.0).  Then hand-made edge cases (one distinct score,
            anti-predictive, one class, one row, masked-out class, -0.0 against +0.0) and seeded random ones on small grids.  Asserted:
            some case separates the no-drop variant and some the exact-rational variant (tests/complementarity_refs.youden_ref).
  pair      val (250 rows) and test (300 rows), K = 3, ~85 % known, logits on a 1/16 grid (ties).  Label 0: the TS head is
            anti-predictive in val (threshold +inf).  Label 1: no known test rows (the reference's empty row).  Label 2: one class
            in val (NaN thresholds) but analysed in test.  `test_mask_alt` is the test mask with label 1 known again: a second set
            of rows where every label is analysed.
  results   thresholds, the rows (JSON text; NaN as the token NaN), the CSV text, the stdout of `_print_report`, the Venn counts
            ([K, 7] in the order of VENN_IDS, -1 where `_plot_venn` draws nothing), for both test masks; `parse_args` names and defaults.
Asserted as well: no reported ratio within 1e-9 of a rounding boundary of the report's 3-decimal format; the file stays under 512 KiB.
Build container only.

Usage:  python tests/golden/make_golden_complementarity.py [output directory]"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ.setdefault("MPLBACKEND", "Agg")
from make_golden import REF, install_stubs  # noqa: E402
from complementarity_refs import HEADS, VENN_IDS, youden_ref  # noqa: E402

K, N_VAL, N_TEST, DATA_SEED, CASE_SEED, N_RANDOM = 3, 250, 300, 11, 5, 48
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
ISSUE_CASES = (
    ([0.5, -1, -0.0, -0.5, 1, 1.5, -0.5, -2, 0.5, 1, -0.0, -1.5], [1, 1, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0]),          # the drop rule decides
    ([-0.5, 1.5, 0.5, -0.5, 1.5, -1, 1, -0.5, 0.5, -1], [1, 1, 1, 0, 1, 0, 1, 0, 0, 0]),                           # the fp64 rounding decides
)
PRINTED = ("img_acc", "ts_acc", "ts_unique_gain", "ts_redundancy", "kappa_img_ts", "err_corr", "fus_acc", "ts_gain_retention",
           "fusion_harm_rate", "emergent_gain")                  # what `_print_report` formats with three decimals
VENN_LOG = []


def import_reference():
    install_stubs()
    sys.path.insert(0, REF)
    venn = types.ModuleType("matplotlib_venn")

    class _Label:
        def __init__(self, log, region):
            self.log, self.region = log, region

        def set_text(self, text):
            self.log[self.region] = int(text)

    class _Diagram:
        def __init__(self):
            self.counts = {}
            VENN_LOG.append(self.counts)

        def get_label_by_id(self, region):
            return _Label(self.counts, region)

    venn.venn3 = lambda subsets, set_labels, ax: _Diagram()
    sys.modules["matplotlib_venn"] = venn
    import analysis.complementarity as ref
    assert ref.HAS_VENN
    return ref


def grid(a, step):
    return (np.round(np.asarray(a, dtype=np.float64) / step) * step).astype(np.float32)


def threshold_cases(rng):
    cases = [(np.array(z, dtype=np.float32), np.array(y, dtype=np.float32), np.ones(len(z), dtype=np.float32)) for z, y in ISSUE_CASES]
    f = lambda *a: np.array(a, dtype=np.float32)  # noqa: E731
    cases += [
        (f(0.25, 0.25, 0.25, 0.25), f(1, 0, 1, 0), f(1, 1, 1, 1)),                      # one distinct score: +inf
        (f(-1, -2, 1, 2, 0.5, -0.5), f(1, 1, 0, 0, 0, 1), f(1, 1, 1, 1, 1, 1)),         # anti-predictive: +inf
        (f(1, 2, 3), f(1, 1, 1), f(1, 1, 1)),                                           # one class
        (f(1, 2, 3), f(1, 0, 1), f(0, 1, 0)),                                           # one known row
        (f(1, 2, 3, 4), f(1, 0, 1, 0), f(0, 0, 0, 0)),                                  # nothing known
        (f(1, 2, 3, 4, 5), f(1, 0, 1, 0, 0), f(1, 0, 1, 1, 0)),                         # the mask leaves both classes
        (f(1, 2, 3, 4, 5), f(1, 0, 1, 0, 0), f(1, 0, 1, 0, 0)),                         # the mask removes a whole class
        (f(-0.0, 0.0, -1, 1, -0.0, 0.0), f(1, 0, 0, 1, 1, 0), f(1, 1, 1, 1, 1, 1)),     # -0.0 and +0.0: one tie group
        (f(0.0, -0.0, -1, -0.0), f(1, 1, 0, 0), f(1, 1, 1, 1)),
        (f(2, 1), f(1, 0), f(1, 1)), (f(1, 2), f(1, 0), f(1, 1)),                       # two rows
    ]
    for i in range(N_RANDOM):
        n = int(rng.integers(4, 41))
        step = (0.5, 0.25, 1.0)[i % 3]
        y = (rng.random(n) < (0.5 if i % 4 else 0.3)).astype(np.float32)
        if i % 5 == 0:
            y[: n // 2], y[n // 2:] = 1.0, 0.0                                          # a half / half split
            rng.shuffle(y)
        sign = -1.0 if i % 7 == 3 else 1.0
        z = grid(np.clip(sign * (y - 0.5) * rng.uniform(0.0, 2.0) + rng.standard_normal(n), -2.5, 2.5), step)
        mask = (rng.random(n) < (0.8 if i % 2 else 1.0)).astype(np.float32)
        cases.append((z, y, mask))
    return cases


def synth_pair(rng):
    def split(n):
        signal = rng.standard_normal((n, K))
        y = (rng.random((n, K)) < 1.0 / (1.0 + np.exp(-1.5 * signal))).astype(np.float32)
        img = grid(np.clip(1.2 * signal + 1.0 * rng.standard_normal((n, K)), -3.9, 3.9), 1 / 16)
        ts = grid(np.clip(0.8 * signal + 1.2 * rng.standard_normal((n, K)), -3.9, 3.9), 1 / 16)
        fus = grid(np.clip(img + 0.5 * ts + 0.3 * rng.standard_normal((n, K)), -3.9, 3.9), 1 / 16)
        mask = (rng.random((n, K)) < 0.85).astype(np.float32)
        return {"img": img, "ts": ts, "fus": fus, "y": y, "mask": mask}

    val, test = split(N_VAL), split(N_TEST)
    # label 0, TS head, val: every known positive strictly below every known negative -> no point with J > 0
    val["ts"][:, 0] = grid(np.where(val["y"][:, 0] > 0, -1.0, 1.0) * (0.25 + np.abs(val["ts"][:, 0])), 1 / 16)
    val["y"][:, 2] = 0.0                                                                 # label 2: one class in val
    test_mask_alt = test["mask"].copy()
    test["mask"][:, 1] = 0.0                                                             # label 1: nothing known in test
    return val, test, test_mask_alt


def report_of(ref, test, thresholds):
    preds = ref._binarize(test, thresholds, K)
    rows = [ref._analyze_pathology(k, LABELS[k], test, preds) for k in range(K)]
    buffer = io.StringIO()
    with contextlib.redirect_stdout(buffer):
        ref._print_report(rows, thresholds, LABELS)
    venn = np.full((K, len(VENN_IDS)), -1, dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        with contextlib.redirect_stdout(io.StringIO()):
            ref._save_csv(rows, os.path.join(tmp, "c.csv"))
        csv_text = open(os.path.join(tmp, "c.csv"), newline="").read()
        for k in range(K):
            del VENN_LOG[:]
            if ref._plot_venn(k, LABELS[k], test, preds, os.path.join(tmp, f"v{k}.png")):
                assert len(VENN_LOG) == 1 and sorted(VENN_LOG[0]) == sorted(VENN_IDS)
                venn[k] = [VENN_LOG[0][r] for r in VENN_IDS]
    for r in rows:                                                                       # the report's 3-decimal fields, away from .5 of the last digit
        for key in PRINTED:
            v = r[key]
            if isinstance(v, float) and np.isfinite(v):
                frac = v * 1000.0 - np.floor(v * 1000.0)
                assert abs(frac - 0.5) > 1e-9, (r["label"], key, v)
    return rows, buffer.getvalue(), csv_text, venn


def main(out_dir=HERE):
    ref = import_reference()
    from sklearn.metrics import roc_curve
    out = {"labels": np.array(LABELS), "heads": np.array(HEADS), "venn_ids": np.array(VENN_IDS)}

    # ---- threshold cases
    cases = threshold_cases(np.random.default_rng(CASE_SEED))
    thr, js, sep_drop, sep_exact = [], [], 0, 0
    for z, y, mask in cases:
        data = {mod: z[:, None] for mod in HEADS}
        data.update(y=y[:, None], mask=mask[:, None])
        t = float(ref._derive_thresholds(data, 1, "youden")["img"][0])
        m = mask.astype(bool)
        if m.sum() >= 2 and len(np.unique(y[m])) == 2:
            fpr, tpr, _ = roc_curve(y[m], z[m])
            j = float(np.max(tpr - fpr))
        else:
            j = float("nan")
        mine = youden_ref(z, y, mask)
        assert (np.isnan(t) and np.isnan(mine[0])) or (t == mine[0] and j == mine[1]), (z, y, mask, t, j, mine)
        no_drop, rational = youden_ref(z, y, mask, drop=False)[0], youden_ref(z, y, mask, exact=True)[0]
        sep_drop += not (no_drop == t or (np.isnan(no_drop) and np.isnan(t)))
        sep_exact += not (rational == t or (np.isnan(rational) and np.isnan(t)))
        thr.append(t)
        js.append(j)
    assert thr[0] == 1.5 and youden_ref(*cases[0], drop=False)[0] == 0.5
    assert thr[1] == 0.5 and youden_ref(*cases[1], exact=True)[0] == 1.0
    assert sep_drop >= 1 and sep_exact >= 1
    print(f"{len(cases)} threshold cases: {sep_drop} separate the no-drop variant, {sep_exact} the exact-rational variant; "
          f"{int(np.isinf(thr).sum())} give +inf, {int(np.isnan(thr).sum())} NaN")
    out.update(case_len=np.array([len(c[0]) for c in cases]), case_z=np.concatenate([c[0] for c in cases]),
               case_y=np.concatenate([c[1] for c in cases]), case_mask=np.concatenate([c[2] for c in cases]),
               case_thr=np.array(thr, dtype=np.float64), case_j=np.array(js, dtype=np.float64))

    # ---- the val / test pair
    val, test, test_mask_alt = synth_pair(np.random.default_rng(DATA_SEED))
    for split, d in (("val", val), ("test", test)):
        for key, v in d.items():
            assert v.dtype == np.float32
            out[f"{split}_{key}"] = v
    out["test_mask_alt"] = test_mask_alt
    assert sum(N_VAL + N_TEST - np.unique(d[h][:, k]).size > 0 for d in (val, test) for h in HEADS for k in range(K)), "ties wanted"
    thresholds = ref._derive_thresholds(val, K, "youden")
    table = np.stack([thresholds[h] for h in HEADS])
    print("thresholds\n", table)
    assert np.isinf(table[1, 0]) and np.isfinite(table[[0, 2], 0]).all() and np.isfinite(table[:, 1]).all() and np.isnan(table[:, 2]).all()
    out["thresholds"] = table
    fixed = ref._derive_thresholds(val, K, "fixed")
    assert all(np.array_equal(fixed[h], np.zeros(K)) for h in HEADS)
    for name, mask in (("rows", test["mask"]), ("rows_alt", test_mask_alt)):
        rows, text, csv_text, venn = report_of(ref, dict(test, mask=mask), thresholds)
        out[f"{name}_json"], out[f"{name}_stdout"], out[f"{name}_csv"], out[f"{name}_venn"] = (np.array(json.dumps(rows)), np.array(text),
                                                                                              np.array(csv_text), venn)
        print(text)
    rows = json.loads(str(out["rows_json"]))
    assert rows[1]["n"] == 0 and "both_agree_broken" in rows[1] and rows[2]["n"] > 0 and rows[0]["n"] > 0
    assert all(r["n"] > 0 for r in json.loads(str(out["rows_alt_json"])))

    # ---- the command line
    argv, sys.argv = sys.argv, ["complementarity", "--ckpt", "best.pt", "--outdir", "out"]
    try:
        out["options_json"] = np.array(json.dumps(vars(ref.parse_args())))
    finally:
        sys.argv = argv
    print(str(out["options_json"]))

    path = os.path.join(out_dir, "complementarity.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 2 ** 19, os.path.getsize(path)
    print(f"wrote complementarity.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
