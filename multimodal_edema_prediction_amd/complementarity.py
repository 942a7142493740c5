"""Modality complementarity of a trained dual teacher (reference analysis/complementarity.py) on the HIP kernels of
csrc/complementarity.hip: do the image head and the time-series head get different patients right, and does the fusion head keep what
the TS head alone got right?

    python -m multimodal_edema_prediction_amd.complementarity --ckpt runs/t0/best.pt --outdir runs/t0/complementarity

The reference's names without the leading underscore.  Per label and head a threshold is set on the val split by Youden's J
(`thr[argmax(tpr - fpr)]` of sklearn's `roc_curve`, reproduced bit for bit: DESIGN.md "Modality complementarity"), the test split is
binarised with it, and every figure of the report follows from 16 integers per label: the counts of (y, image says 1, TS says 1,
fusion says 1) over the known rows.

What runs where
  device, HIP   `youden_thresholds` (one launch: all heads and labels) and `contingency_cells` (one launch), on the fp32 logits
                `conditional_information_probe.gather` leaves on the device.
  host          two small reads per run (thresholds with J and counts; the cells), then `analyze_pathology` in the reference's key and
                expression order, the report, the CSV and the archive.  Nothing synchronises per label.
sklearn and matplotlib are not dependencies; the Venn diagrams are not drawn, their seven counts go into the archive.  Without a GPU
every entry point that touches data raises (no CPU fallback)."""
from __future__ import annotations

import argparse
import csv
import math
import os
from typing import Dict, Mapping, Sequence

import numpy as np
import torch

from .abi import check, lib, ptr, require_gpu, stream
from .probe_stats import METRICS_MAX_LEN, pearson

HEADS = ("img", "ts", "fus")
YOUDEN_MAX_LEN = METRICS_MAX_LEN   # MEDP_YOUDEN_MAX_LEN: the known rows of one label the threshold kernel sorts in LDS (one bound)
VENN_IDS = ("100", "010", "110", "001", "101", "011", "111")      # (image, TS, fusion) digits, the reference's `_plot_venn` order
CELL_KEYS = ("ts_only_and_fus_ok", "ts_only_but_fus_lost_it", "image_only_and_fus_ok", "image_only_but_fus_lost_it",
             "both_wrong_but_fus_saved", "all_three_wrong", "both_correct_and_fus_ok", "both_correct_but_fus_broke_it")
PAIR_KEYS = ("both_correct", "image_only_correct", "ts_only_correct", "both_wrong")


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _stacked(data: Mapping[str, torch.Tensor]):
    """(scores [3, N, K], y [N, K], mask [N, K]) fp32 contiguous on the device."""
    parts = [data[h] for h in HEADS]
    for t in parts + [data["y"], data["mask"]]:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("complementarity operates on GPU tensors (the output of `gather`); there is no CPU fallback")
        if t.dtype != torch.float32 or t.shape != parts[0].shape or t.ndim != 2:
            raise TypeError("complementarity: img, ts, fus, y and mask are fp32 [N, K]")
    return torch.stack(parts).contiguous(), data["y"].contiguous(), data["mask"].contiguous()


def youden_thresholds(scores: torch.Tensor, y: torch.Tensor, mask: torch.Tensor):
    """scores [H, N, K], y, mask [N, K] fp32 -> device tensors (thr [H, K] fp64, youden_j [H, K] fp64, counts [K, 2] int32 = known
    rows, known positives).  +inf: no point of the curve has J > 0; NaN: fewer than two known rows, one class, or a non-finite score.
    More than YOUDEN_MAX_LEN known rows of a label: ValueError, nothing is sorted."""
    require_gpu()
    if scores.dtype != torch.float32 or y.dtype != torch.float32 or mask.dtype != torch.float32:
        raise TypeError("youden_thresholds reads fp32")
    scores, y, mask = scores.contiguous(), y.contiguous(), mask.contiguous()
    if scores.ndim != 3 or y.shape != scores.shape[1:] or mask.shape != y.shape:
        raise ValueError("youden_thresholds: scores [H, N, K], y and mask [N, K]")
    H, N, K = scores.shape
    thr = torch.empty((H, K), dtype=torch.float64, device=scores.device)
    j = torch.empty_like(thr)
    counts = torch.empty((K, 2), dtype=torch.int32, device=scores.device)
    check(lib().medp_youden_thresholds(ptr(scores), ptr(y), ptr(mask), ptr(thr), ptr(j), ptr(counts), H, N, K, stream()), "youden_thresholds")
    return thr, j, counts


def complementarity_cells(scores: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    """scores [3, N, K] fp32, thr [3, K] fp64 -> cells [K, 16] int32 on the device: over the known rows the count of every
    (y != 0) | ip << 1 | tp << 2 | fp << 3 with ip / tp / fp = score > thr of the image / TS / fusion head."""
    require_gpu()
    if scores.dtype != torch.float32 or y.dtype != torch.float32 or mask.dtype != torch.float32 or thr.dtype != torch.float64:
        raise TypeError("complementarity_cells reads fp32 scores and fp64 thresholds")
    scores, y, mask, thr = scores.contiguous(), y.contiguous(), mask.contiguous(), thr.contiguous()
    if scores.ndim != 3 or scores.shape[0] != 3 or y.shape != scores.shape[1:] or mask.shape != y.shape or thr.shape != (3, y.shape[1]):
        raise ValueError("complementarity_cells: scores [3, N, K], y and mask [N, K], thr [3, K]")
    _, N, K = scores.shape
    cells = torch.empty((K, 16), dtype=torch.int32, device=scores.device)
    check(lib().medp_complementarity_cells(ptr(scores), ptr(y), ptr(mask), ptr(thr), ptr(cells), N, K, stream()), "complementarity_cells")
    return cells


# ------------------------------------------------------------------------------------------------------------------------------
# thresholds, cells
# ------------------------------------------------------------------------------------------------------------------------------
def _derive(val_data: Mapping[str, torch.Tensor], method: str):
    """-> (thr [3, K], youden_j [3, K], counts [K, 2]) on the host, ONE read."""
    K = val_data["img"].shape[1]
    if method == "fixed":
        return np.zeros((3, K)), np.full((3, K), np.nan), np.zeros((K, 2), dtype=np.int32)
    if method != "youden":
        raise ValueError(f"Unknown threshold method {method!r}")
    thr, j, counts = youden_thresholds(*_stacked(val_data))
    flat = torch.cat([thr.reshape(-1), j.reshape(-1), counts.to(torch.float64).reshape(-1)]).cpu().numpy()
    thr, j, counts = flat[:3 * K].reshape(3, K), flat[3 * K:6 * K].reshape(3, K), flat[6 * K:].reshape(K, 2).astype(np.int32)
    curve = (counts[:, 0] >= 2) & (counts[:, 1] > 0) & (counts[:, 1] < counts[:, 0])
    if (np.isnan(thr) & curve[None, :]).any():
        raise ValueError("Input contains NaN or infinity: a logit of a known val row is not finite")
    return thr, j, counts


def derive_thresholds(val_data: Mapping[str, torch.Tensor], method: str = "youden") -> Dict[str, np.ndarray]:
    """`_derive_thresholds` (:111-123) -> {"img", "ts", "fus"}: [K] fp64 each.  "youden": one kernel launch; "fixed": zeros."""
    thr, _, _ = _derive(val_data, method)
    return {h: thr[i].copy() for i, h in enumerate(HEADS)}


def contingency_cells(test_data: Mapping[str, torch.Tensor], thresholds: Mapping[str, np.ndarray]) -> np.ndarray:
    """`_binarize` (:126-135) and every count of `_analyze_pathology` at once -> [K, 16] int64 on the host (one launch, one read)."""
    scores, y, mask = _stacked(test_data)
    thr = torch.as_tensor(np.stack([np.asarray(thresholds[h], dtype=np.float64) for h in HEADS]), device=scores.device)
    return complementarity_cells(scores, y, mask, thr).cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# per-pathology analysis, from the 16 integers
# ------------------------------------------------------------------------------------------------------------------------------
def _cell_sum(cells_row, y=None, ip=None, tp=None, fp=None, ic=None, tc=None, fc=None) -> int:
    """Sum of the cells whose bits match the given values; ic / tc / fc: the head is correct (its prediction equals y)."""
    total = 0
    for c in range(16):
        b = (c & 1, (c >> 1) & 1, (c >> 2) & 1, (c >> 3) & 1)
        ok = all(want is None or bool(want) == bool(got) for want, got in ((y, b[0]), (ip, b[1]), (tp, b[2]), (fp, b[3])))
        ok = ok and all(want is None or bool(want) == (got == b[0]) for want, got in ((ic, b[1]), (tc, b[2]), (fc, b[3])))
        total += int(cells_row[c]) if ok else 0
    return total


def _ratio(num, den):
    return num / den if den > 0 else float("nan")


def _cohens_kappa(n: int, agree: int, x_true: int, y_true: int) -> float:
    """`_cohens_kappa` (:141-150) from counts: a mean of n booleans IS count / n."""
    if n == 0:
        return float("nan")
    po = agree / n
    px, py = x_true / n, y_true / n
    pe = px * py + (1 - px) * (1 - py)
    if 1 - pe == 0:
        return float("nan")
    return (po - pe) / (1 - pe)


def analyze_pathology(label: str, cells_row) -> dict:
    """`_analyze_pathology` (:159-237) from one label's 16 counts: the reference's keys in its order, its expressions in its order
    (every mean of booleans there is an exact count divided by n).  `err_corr` is `probe_stats.pearson` of the two error indicators
    expanded cell after cell.  A label without known rows gets the reference's empty row, `both_agree_broken` key included."""
    cells_row = np.asarray(cells_row, dtype=np.int64)
    if cells_row.shape != (16,):
        raise ValueError("analyze_pathology: 16 counts per label")
    n = int(cells_row.sum())
    if n == 0:
        empty = {"label": label, "n": 0, "pos_frac": float("nan")}
        for key in ("img_acc", "ts_acc", "fus_acc", "ts_unique_gain", "ts_redundancy", "coverage_gain", "kappa_img_ts", "err_corr",
                    "ts_gain_retention", "fusion_harm_rate", "emergent_gain", "both_agree_broken"):
            empty[key] = float("nan")
        for key in PAIR_KEYS + CELL_KEYS:
            empty[key] = 0
        return empty
    s = lambda **kw: _cell_sum(cells_row, **kw)  # noqa: E731
    both_correct, image_only_correct = s(ic=1, tc=1), s(ic=1, tc=0)
    ts_only_correct, both_wrong = s(ic=0, tc=1), s(ic=0, tc=0)
    ts_only_and_fus_ok, ts_only_but_fus_lost_it = s(ic=0, tc=1, fc=1), s(ic=0, tc=1, fc=0)
    image_only_and_fus_ok, image_only_but_fus_lost_it = s(ic=1, tc=0, fc=1), s(ic=1, tc=0, fc=0)
    both_wrong_but_fus_saved, all_three_wrong = s(ic=0, tc=0, fc=1), s(ic=0, tc=0, fc=0)
    both_correct_and_fus_ok, both_correct_but_fus_broke_it = s(ic=1, tc=1, fc=1), s(ic=1, tc=1, fc=0)
    code = np.repeat(np.arange(16), cells_row)
    wrong = lambda bit: (((code >> bit) & 1) != (code & 1)).astype(float)  # noqa: E731
    return {
        "label": label, "n": n, "pos_frac": s(y=1) / n,
        "img_acc": s(ic=1) / n, "ts_acc": s(tc=1) / n, "fus_acc": s(fc=1) / n,
        "both_correct": both_correct, "image_only_correct": image_only_correct,
        "ts_only_correct": ts_only_correct, "both_wrong": both_wrong,
        "ts_unique_gain": ts_only_correct / n,
        "ts_redundancy": _ratio(both_correct, both_correct + ts_only_correct),
        "coverage_gain": (both_correct + image_only_correct + ts_only_correct) / n,
        "kappa_img_ts": _cohens_kappa(n, both_correct + both_wrong, s(ic=1), s(tc=1)),
        "err_corr": pearson(wrong(1), wrong(2)),
        "ts_only_and_fus_ok": ts_only_and_fus_ok, "ts_only_but_fus_lost_it": ts_only_but_fus_lost_it,
        "image_only_and_fus_ok": image_only_and_fus_ok, "image_only_but_fus_lost_it": image_only_but_fus_lost_it,
        "both_wrong_but_fus_saved": both_wrong_but_fus_saved, "all_three_wrong": all_three_wrong,
        "both_correct_and_fus_ok": both_correct_and_fus_ok, "both_correct_but_fus_broke_it": both_correct_but_fus_broke_it,
        "ts_gain_retention": _ratio(ts_only_and_fus_ok, ts_only_and_fus_ok + ts_only_but_fus_lost_it),
        "fusion_harm_rate": _ratio(image_only_but_fus_lost_it, image_only_and_fus_ok + image_only_but_fus_lost_it),
        "emergent_gain": _ratio(both_wrong_but_fus_saved, both_wrong_but_fus_saved + all_three_wrong),
        "both_agree_broken_rate": _ratio(both_correct_but_fus_broke_it, both_correct_and_fus_ok + both_correct_but_fus_broke_it),
    }


def venn_counts(cells_row) -> Dict[str, int]:
    """The seven regions of `_plot_venn` (:305-326): known positives caught by exactly that combination of (image, TS, fusion)."""
    return {r: _cell_sum(cells_row, y=1, ip=int(r[0]), tp=int(r[1]), fp=int(r[2])) for r in VENN_IDS}


# ------------------------------------------------------------------------------------------------------------------------------
# the run
# ------------------------------------------------------------------------------------------------------------------------------
def resolve_labels(requested: str, pathology_labels: Sequence[str]) -> tuple:
    """The reference's `--labels` rule (:384-390): case-insensitive full names, empty = all; an unknown name ends the program."""
    label_to_idx = {lbl.lower(): i for i, lbl in enumerate(pathology_labels)}
    names = [s.strip().lower() for s in requested.split(",") if s.strip()]
    unknown = [n for n in names if n not in label_to_idx]
    if unknown:
        raise SystemExit(f"--labels: unknown pathology {unknown}. available: {list(label_to_idx)}")
    return tuple(label_to_idx[n] for n in names) if names else tuple(range(len(pathology_labels)))


def run_complementarity(val_data: Mapping[str, torch.Tensor], test_data: Mapping[str, torch.Tensor], pathology_labels: Sequence[str],
                        threshold: str = "youden", labels: str = ""):
    """The body of the reference's `main()` after its two gathers (:380-398) -> (rows of the requested labels, their thresholds
    {"img", "ts", "fus"}, archive).  Thresholds and cells are derived for ALL labels (two launches, two host reads); `labels` filters the
    rows and the returned thresholds only.  The archive holds, for all labels: thresholds and youden_j [3, K], val_counts [K, 2], cells
    [K, 16], venn [K, 7] (VENN_IDS order) and the label names."""
    require_gpu()
    pathology_labels = [str(s) for s in pathology_labels]
    analyze_idx = resolve_labels(labels, pathology_labels)
    thr, j, counts = _derive(val_data, threshold)
    cells = contingency_cells(test_data, {h: thr[i] for i, h in enumerate(HEADS)})
    rows = [analyze_pathology(pathology_labels[k], cells[k]) for k in analyze_idx]
    thresholds = {h: thr[i][list(analyze_idx)] for i, h in enumerate(HEADS)}
    archive = {"labels": np.array(pathology_labels), "heads": np.array(HEADS), "venn_ids": np.array(VENN_IDS), "thresholds": thr,
               "youden_j": j, "val_counts": counts, "cells": cells,
               "venn": np.array([[venn_counts(cells[k])[r] for r in VENN_IDS] for k in range(len(pathology_labels))], dtype=np.int64)}
    return rows, thresholds, archive


# ------------------------------------------------------------------------------------------------------------------------------
# outputs, command line
# ------------------------------------------------------------------------------------------------------------------------------
def _fmt(v, spec="7.3f"):
    width = spec.split(".")[0].lstrip("+")
    try:
        if math.isnan(float(v)):
            return f"{'--':>{width}s}"
    except (TypeError, ValueError):
        return f"{'--':>{width}s}"
    return f"{v:{spec}}"


def print_report(rows, thresholds, pathology_labels) -> None:
    """`_print_report` (:254-288), character for character."""
    print("\n=== Per-pathology thresholds (logit units) ===")
    print(f"{'':>4s}  " + "  ".join(f"{lbl[:12]:>12s}" for lbl in pathology_labels))
    for mod in HEADS:
        line = "  ".join(_fmt(t, "12.4f") for t in thresholds[mod])
        print(f"{mod:>4s}  {line}")

    print("\n=== Level 1: image vs TS  (does complementarity exist?) ===")
    print(f"{'label':<14s} {'n':>5s} {'img_acc':>7s} {'ts_acc':>7s} "
          f"{'both_ok':>7s} {'img_only':>8s} {'ts_only':>7s} {'both_wr':>7s} "
          f"{'ts_gain':>7s} {'ts_redun':>8s} {'kappa':>6s} {'err_r':>6s}")
    for r in rows:
        print(f"{r['label'][:14]:<14s} {r['n']:>5d} "
              f"{_fmt(r['img_acc'], '7.3f')} {_fmt(r['ts_acc'], '7.3f')} "
              f"{r['both_correct']:>7d} {r['image_only_correct']:>8d} "
              f"{r['ts_only_correct']:>7d} {r['both_wrong']:>7d} "
              f"{_fmt(r['ts_unique_gain'], '7.3f')} "
              f"{_fmt(r['ts_redundancy'], '8.3f')} "
              f"{_fmt(r['kappa_img_ts'], '6.3f')} "
              f"{_fmt(r['err_corr'], '6.3f')}")

    print("\n=== Level 2: 3-way with fusion  (does fusion capture it?) ===")
    print("cells: fus_ok / fus_bad")
    print(f"{'label':<14s} {'fus_acc':>7s} "
          f"{'ts_retain':>9s} {'fus_harm':>8s} {'emergent':>8s} "
          f"{'ts_only':>9s} {'img_only':>9s} {'both_wr':>9s} {'both_ok':>9s}")
    for r in rows:
        print(f"{r['label'][:14]:<14s} {_fmt(r['fus_acc'], '7.3f')} "
              f"{_fmt(r['ts_gain_retention'], '9.3f')} "
              f"{_fmt(r['fusion_harm_rate'], '8.3f')} "
              f"{_fmt(r['emergent_gain'], '8.3f')} "
              f"{r['ts_only_and_fus_ok']:>4d}/{r['ts_only_but_fus_lost_it']:<4d} "
              f"{r['image_only_and_fus_ok']:>4d}/{r['image_only_but_fus_lost_it']:<4d} "
              f"{r['both_wrong_but_fus_saved']:>4d}/{r['all_three_wrong']:<4d} "
              f"{r['both_correct_and_fus_ok']:>4d}/{r['both_correct_but_fus_broke_it']:<4d}")


def save_csv(rows, path) -> None:
    """`_save_csv` (:291-298): the first row's keys are the columns; a key another row lacks stays empty, one it adds is ignored."""
    fieldnames = list(rows[0].keys())
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=fieldnames, extrasaction="ignore")
        w.writeheader()
        for r in rows:
            w.writerow(r)
    print(f"[complementarity] csv -> {path}")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser("Modality complementarity analysis")
    p.add_argument("--ckpt", type=str, required=True, help="dual teacher best.pt written by train_synthetic")
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--val_split", type=str, default="val", help="the split the thresholds are set on")
    p.add_argument("--test_split", type=str, default="test", help="the split the contingency counts are taken on")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--threshold", type=str, default="youden", choices=["youden", "fixed"],
                   help="youden: the point of largest TPR - FPR on the val split; fixed: logit 0 (probability 0.5)")
    p.add_argument("--labels", type=str, default="",
                   help="comma-separated pathology names to report; empty: all.  Thresholds are derived for every label either way")
    return p.parse_args(argv)


def main(argv=None) -> dict:
    """The reference's `main()` (:347-414) on a `train_synthetic` teacher checkpoint; the splits are slices of its synthetic cohort."""
    from . import checkpoint, train_synthetic
    from .conditional_information_probe import gather
    args = parse_args(argv)
    require_gpu()
    os.makedirs(args.outdir, exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"[complementarity] device={device}")
    state = checkpoint.load_ckpt(args.ckpt)
    t_args = argparse.Namespace(**state["args"])
    mode = state["args"].get("perceiver_type")
    pathology_labels = tuple(s.strip() for s in state["args"]["pathology_labels"].split(","))
    print(f"[complementarity] loaded ckpt: {args.ckpt}  mode={mode}")
    print(f"[complementarity] pathology_labels: {pathology_labels}")
    if mode not in ("dual", "dual_patch"):
        raise SystemExit(f"complementarity needs a dual / dual_patch teacher, got mode={mode!r}")
    datasets = dict(zip(("train", "val", "test"), train_synthetic._datasets(t_args)))
    if args.val_split not in datasets:
        raise SystemExit(f"val_split '{args.val_split}' not in datasets: {list(datasets)}")
    if args.test_split not in datasets:
        raise SystemExit(f"test_split '{args.test_split}' not in datasets: {list(datasets)}")
    analyze_idx = resolve_labels(args.labels, pathology_labels)                     # before the forwards: a typo costs nothing
    teacher = train_synthetic.build_teacher_from_ckpt(state, t_args.d_static, t_args.n_vars, t_args.duett_ckpt, t_args.n_timesteps,
                                                      t_args.cxr_model_name).to(device)
    loader = lambda split: train_synthetic.make_loader(datasets[split], args.batch_size, False, args.num_workers, "teacher", 0, 1)  # noqa: E731
    print(f"[complementarity] gathering {args.val_split} for thresholds...")
    val_data = gather(teacher, loader(args.val_split), device)
    print(f"[complementarity] gathering {args.test_split} for evaluation...")
    test_data = gather(teacher, loader(args.test_split), device)
    print(f"[complementarity] threshold method: {args.threshold}")
    rows, thresholds, archive = run_complementarity(val_data, test_data, pathology_labels, args.threshold, args.labels)
    if args.labels.strip():
        print(f"[complementarity] --labels filter: {[pathology_labels[i] for i in analyze_idx]}")
    print_report(rows, thresholds, tuple(pathology_labels[i] for i in analyze_idx))
    csv_path, npz_path = os.path.join(args.outdir, "complementarity.csv"), os.path.join(args.outdir, "complementarity.npz")
    save_csv(rows, csv_path)
    np.savez_compressed(npz_path, **archive)
    print(f"[complementarity] npz -> {npz_path}")
    print(f"\n[complementarity] done -> {args.outdir}")
    return {"rows": rows, "thresholds": thresholds, "archive": archive, "csv": csv_path, "npz": npz_path}


if __name__ == "__main__":
    main()
