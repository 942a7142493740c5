"""Restatements for the modality complementarity analysis (multimodal_edema_prediction_amd/complementarity.py, csrc/complementarity.hip).

  `youden_ref`   `medp_youden_thresholds` for one (head, label) in numpy: sklearn's `roc_curve` + first `argmax(tpr - fpr)` with its
                 three deciding properties spelt out (the (0, 0) start point at +inf, J as two rounded fp64 quotients and a difference,
                 `drop_intermediate`'s second-difference rule).  `drop=False` and `exact=True` are the two WRONG variants (every point
                 kept; J compared as a rational): the fixture's maker uses them to prove its cases tell the variants apart.
  `cells_ref`    `medp_complementarity_cells`: the 16 counts per label.
  `rows_from_predictions`  the reference's `_analyze_pathology` expressions on boolean prediction arrays (the 16-cell derivation is
                 checked against it), `venn_ref` its `_plot_venn` counts.
  `golden()`     tests/golden/complementarity.npz (tests/golden/make_golden_complementarity.py: the reference's own functions)."""
from __future__ import annotations

import json
import os
from fractions import Fraction

import numpy as np

HEADS = ("img", "ts", "fus")
VENN_IDS = ("100", "010", "110", "001", "101", "011", "111")
_GOLDEN = {}


def golden():
    if not _GOLDEN:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "complementarity.npz")
        with np.load(path, allow_pickle=False) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def golden_cases(g=None) -> list:
    """The fixture's threshold cases: dicts of z (fp32), y, mask, thr, j."""
    g = golden() if g is None else g
    edges = np.r_[0, np.cumsum(g["case_len"])]
    return [{"z": g["case_z"][a:b], "y": g["case_y"][a:b], "mask": g["case_mask"][a:b], "thr": float(g["case_thr"][i]), "j": float(g["case_j"][i])}
            for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


def golden_split(split: str, g=None) -> dict:
    g = golden() if g is None else g
    return {k: g[f"{split}_{k}"] for k in ("img", "ts", "fus", "y", "mask")}


def golden_rows(variant: str = "rows", g=None) -> list:
    g = golden() if g is None else g
    return json.loads(str(g[f"{variant}_json"]))


def same_bits(a, b) -> bool:
    """Equal as IEEE values with NaN equal to NaN, and zeros of the same sign (the recorded report text prints a zero threshold's sign)."""
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


def youden_ref(z, y, mask=None, drop: bool = True, exact: bool = False):
    """One (head, label) -> (thr, J, known rows, known positives); z fp32 [N], y, mask [N]."""
    z, y = np.asarray(z, dtype=np.float32), np.asarray(y)
    known = np.ones(len(z), dtype=bool) if mask is None else np.asarray(mask) != 0
    raw, pos = z[known], y[known] != 0
    s = raw + np.float32(0.0)                                                # -0.0 + 0.0 = +0.0: one tie group
    zero = float(raw[np.flatnonzero(raw == 0)[0]]) if (raw == 0).any() else 0.0      # the zero a stable descending sort ends the group with
    L, P = int(known.sum()), int(pos.sum())
    Nn = L - P
    if L < 2 or P == 0 or Nn == 0 or not np.isfinite(s).all():
        return float("nan"), float("nan"), L, P
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], pos[order]
    ends = np.r_[np.flatnonzero(s[1:] != s[:-1]), L - 1]                      # one point per DISTINCT score, at the end of its tie group
    tps = np.cumsum(pos)[ends].astype(np.int64)
    fps = 1 + ends - tps
    keep = np.ones(len(ends), dtype=bool)
    if drop and len(ends) > 2:                                               # drop_intermediate, before the start point is prepended
        keep[1:-1] = (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0)
    tps, fps, thr = tps[keep], fps[keep], s[ends][keep].astype(np.float64)
    if exact:
        J = [Fraction(int(t), P) - Fraction(int(f), Nn) for t, f in zip(tps, fps)]
        best, best_j = -1, Fraction(0)
        for i, j in enumerate(J):
            if j > best_j:
                best, best_j = i, j
        return (float("inf"), 0.0, L, P) if best < 0 else (float(thr[best]) or zero, float(best_j), L, P)
    J = np.r_[0.0, tps.astype(np.float64) / np.float64(P) - fps.astype(np.float64) / np.float64(Nn)]
    best = int(np.argmax(J))                                                 # the FIRST maximum: the highest threshold
    return (float("inf") if best == 0 else float(thr[best - 1]) or zero), float(J[best]), L, P


def youden_table_ref(scores, y, mask):
    """scores [H, N, K], y, mask [N, K] -> (thr [H, K], J [H, K], counts [K, 2])."""
    H, N, K = scores.shape
    thr, J, counts = np.zeros((H, K)), np.zeros((H, K)), np.zeros((K, 2), dtype=np.int32)
    for h in range(H):
        for k in range(K):
            thr[h, k], J[h, k], counts[k, 0], counts[k, 1] = youden_ref(scores[h, :, k], y[:, k], mask[:, k])
    return thr, J, counts


def cells_ref(scores, y, mask, thr):
    """scores [3, N, K] fp32, thr [3, K] fp64 -> [K, 16] int32 counts of (y != 0) | ip << 1 | tp << 2 | fp << 3 over the known rows."""
    scores, thr = np.asarray(scores, dtype=np.float32), np.asarray(thr, dtype=np.float64)
    K = scores.shape[2]
    with np.errstate(invalid="ignore"):
        pred = scores.astype(np.float64) > thr[:, None, :]                   # NaN and +inf thresholds: False
    code = (np.asarray(y) != 0).astype(np.int64) | pred[0].astype(np.int64) << 1 | pred[1].astype(np.int64) << 2 | pred[2].astype(np.int64) << 3
    known = np.asarray(mask) != 0
    return np.stack([np.bincount(code[known[:, k], k], minlength=16) for k in range(K)]).astype(np.int32)


def expand_cells(cells_row):
    """16 counts -> the boolean columns (y, ip, tp, fp) of as many rows, cell after cell."""
    code = np.repeat(np.arange(16), np.asarray(cells_row, dtype=np.int64))
    return tuple(((code >> b) & 1).astype(bool) for b in range(4))


def rows_from_predictions(label, y, ip, tp, fp) -> dict:
    """The reference's `_analyze_pathology` on the known rows' boolean columns, expression for expression."""
    y, ip, tp, fp = (np.asarray(a, dtype=bool) for a in (y, ip, tp, fp))
    n = len(y)
    nan = float("nan")
    if n == 0:
        row = {"label": label, "n": 0, "pos_frac": nan}
        row.update({k: nan for k in ("img_acc", "ts_acc", "fus_acc", "ts_unique_gain", "ts_redundancy", "coverage_gain", "kappa_img_ts",
                                     "err_corr", "ts_gain_retention", "fusion_harm_rate", "emergent_gain", "both_agree_broken")})
        row.update({k: 0 for k in ("both_correct", "image_only_correct", "ts_only_correct", "both_wrong", "ts_only_and_fus_ok",
                                   "ts_only_but_fus_lost_it", "image_only_and_fus_ok", "image_only_but_fus_lost_it",
                                   "both_wrong_but_fus_saved", "all_three_wrong", "both_correct_and_fus_ok", "both_correct_but_fus_broke_it")})
        return row
    ic, tc, fc = ip == y, tp == y, fp == y
    count = lambda a: int(a.sum())  # noqa: E731
    ratio = lambda num, den: num / den if den > 0 else nan  # noqa: E731
    po, px, py = float((ic == tc).mean()), float(ic.mean()), float(tc.mean())
    pe = px * py + (1 - px) * (1 - py)
    a, b = (~ic).astype(float), (~tc).astype(float)
    corr = nan if (a.size < 2 or a.std() == 0 or b.std() == 0) else float(np.corrcoef(a, b)[0, 1])
    c = {"both_correct": count(ic & tc), "image_only_correct": count(ic & ~tc), "ts_only_correct": count(~ic & tc), "both_wrong": count(~ic & ~tc)}
    d = {"ts_only_and_fus_ok": count(~ic & tc & fc), "ts_only_but_fus_lost_it": count(~ic & tc & ~fc),
         "image_only_and_fus_ok": count(ic & ~tc & fc), "image_only_but_fus_lost_it": count(ic & ~tc & ~fc),
         "both_wrong_but_fus_saved": count(~ic & ~tc & fc), "all_three_wrong": count(~ic & ~tc & ~fc),
         "both_correct_and_fus_ok": count(ic & tc & fc), "both_correct_but_fus_broke_it": count(ic & tc & ~fc)}
    return {"label": label, "n": n, "pos_frac": float(y.mean()), "img_acc": float(ic.mean()), "ts_acc": float(tc.mean()), "fus_acc": float(fc.mean()),
            **c, "ts_unique_gain": c["ts_only_correct"] / n, "ts_redundancy": ratio(c["both_correct"], c["both_correct"] + c["ts_only_correct"]),
            "coverage_gain": (c["both_correct"] + c["image_only_correct"] + c["ts_only_correct"]) / n,
            "kappa_img_ts": nan if 1 - pe == 0 else (po - pe) / (1 - pe), "err_corr": corr, **d,
            "ts_gain_retention": ratio(d["ts_only_and_fus_ok"], d["ts_only_and_fus_ok"] + d["ts_only_but_fus_lost_it"]),
            "fusion_harm_rate": ratio(d["image_only_but_fus_lost_it"], d["image_only_and_fus_ok"] + d["image_only_but_fus_lost_it"]),
            "emergent_gain": ratio(d["both_wrong_but_fus_saved"], d["both_wrong_but_fus_saved"] + d["all_three_wrong"]),
            "both_agree_broken_rate": ratio(d["both_correct_but_fus_broke_it"], d["both_correct_and_fus_ok"] + d["both_correct_but_fus_broke_it"])}


def venn_ref(cells_row) -> dict:
    """`_plot_venn`'s seven counts over the known positives: region ids are (image, TS, fusion) digits."""
    y, ip, tp, fp = expand_cells(cells_row)
    return {r: int((y & (ip == (r[0] == "1")) & (tp == (r[1] == "1")) & (fp == (r[2] == "1"))).sum()) for r in VENN_IDS}


def assert_rows_match(got: list, want: list, float_tol: float = 0.0):
    """Same keys in the same order; integers and strings equal; floats NaN where the reference has NaN, else within float_tol."""
    assert len(got) == len(want)
    worst = 0.0
    for g_row, w_row in zip(got, want):
        assert list(g_row) == list(w_row), (list(g_row), list(w_row))
        for key, w in w_row.items():
            v = g_row[key]
            if isinstance(w, float):
                assert isinstance(v, float), (key, v)
                assert np.isnan(v) == np.isnan(w), (key, v, w)
                if not np.isnan(w):
                    worst = max(worst, abs(v - w))
                    assert abs(v - w) <= float_tol, (key, v, w)
            else:
                assert type(v) is type(w) and v == w, (key, v, w)
    return worst
