"""Where does the fusion residual help?  The consumer of the archive `diagnose_temporal_usage --output_npz` writes: the counterpart of the
reference's `analysis/residual_by_confidence.py`.  Per label the known rows are cut into quartiles of the image branch's confidence
|img logit| (equal counts), and each quartile reports n, prevalence, mean |residual| (residual = fusion logit - image logit), how
often the residual points towards the label, how often fusion lowers the BCE, and the mean BCE change; then the overall line.

    python -m multimodal_edema_prediction_amd.residual_by_confidence --input_npz runs/t0/temporal_usage.npz

Host numpy in fp64, like the reference: 4 x K rows, no hot path.  The printed text is the reference's, character for character
(tests/golden/temporal_usage.npz records it)."""
from __future__ import annotations

import argparse
import warnings
from typing import Sequence

import numpy as np

QUARTILE_NOTES = ("(uncertain)", "", "", "(confident)")


def binary_bce_with_logits(logits, targets):
    """Stable element-wise BCEWithLogits without pos_weight."""
    return np.logaddexp(0.0, logits) - targets * logits


def confidence_table(labels: Sequence[str], y, mask, img, fus) -> list:
    """y, mask, img, fus [N, K] -> per label {"label", "quartiles": four of {n, pos, mean_abs_r, correct_r, helped, mean_dbce},
    "overall": {helped, correct_direction, mean_delta_bce}}.  An empty quartile reports NaN means, as numpy does."""
    y, mask = np.asarray(y, dtype=np.float64), np.asarray(mask).astype(bool)
    img, fus = np.asarray(img, dtype=np.float64), np.asarray(fus, dtype=np.float64)
    residual = fus - img
    table = []
    for k, label in enumerate(labels):
        valid = mask[:, k]
        yy, zi, zf, rr = y[valid, k], img[valid, k], fus[valid, k], residual[valid, k]
        confidence = np.abs(zi)
        edges = np.quantile(confidence, [0.0, 0.25, 0.50, 0.75, 1.0])      # equal counts per quartile
        edges[0], edges[-1] = -np.inf, np.inf
        delta_loss = binary_bce_with_logits(zi, yy) - binary_bce_with_logits(zf, yy)      # positive: fusion lowers the loss
        helpful_direction = (2.0 * yy - 1.0) * rr > 0                                      # y = 1 wants r > 0, y = 0 wants r < 0
        quartiles = []
        for q in range(4):
            upper = confidence < edges[q + 1] if q < 3 else confidence <= edges[q + 1]
            selected = (confidence >= edges[q]) & upper
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", category=RuntimeWarning)      # an empty quartile: numpy's "Mean of empty slice", the table says NaN
                quartiles.append({"n": int(selected.sum()), "pos": float(yy[selected].mean()), "mean_abs_r": float(np.abs(rr[selected]).mean()),
                                  "correct_r": float(helpful_direction[selected].mean()), "helped": float((delta_loss[selected] > 0).mean()),
                                  "mean_dbce": float(delta_loss[selected].mean())})
        table.append({"label": str(label), "quartiles": quartiles,
                      "overall": {"helped": float((delta_loss > 0).mean()), "correct_direction": float(helpful_direction.mean()),
                                  "mean_delta_bce": float(delta_loss.mean())}})
    return table


def print_table(table: list) -> None:
    for entry in table:
        print(f"\nLabel: {entry['label']}")
        print(f"{'confidence':<18s} {'n':>6s} {'pos':>7s} {'mean|r|':>10s} {'correct_r':>10s} {'helped':>9s} {'mean_dBCE':>11s}")
        for q, row in enumerate(entry["quartiles"]):
            print(f"Q{q + 1} {QUARTILE_NOTES[q]:<13s} {row['n']:>6d} {row['pos']:>7.4f} {row['mean_abs_r']:>10.5f} {row['correct_r']:>10.4f} "
                  f"{row['helped']:>9.4f} {row['mean_dbce']:>+11.6f}")
        o = entry["overall"]
        print(f"Overall: helped={o['helped']:.4f}, correct_direction={o['correct_direction']:.4f}, mean_delta_BCE={o['mean_delta_bce']:+.6f}")


def main(argv=None) -> list:
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_npz", required=True)
    args = parser.parse_args(argv)
    with np.load(args.input_npz, allow_pickle=False) as data:
        labels = [x.decode() if isinstance(x, bytes) else str(x) for x in data["labels"].tolist()]
        table = confidence_table(labels, data["y"], data["mask"], data["img_full"], data["fus_full"])
    print_table(table)
    return table


if __name__ == "__main__":
    main()
