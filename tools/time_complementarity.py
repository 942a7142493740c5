#!/usr/bin/env python3
"""Time the modality complementarity analysis (`multimodal_edema_prediction_amd.complementarity`) on synthetic logits at K = 3 labels
and N = 2 048, 8 192 and 16 384 rows per split (val and test alike, every row known, logits on a 1/64 grid so ties exist):

  youden   `youden_thresholds`, one launch for 3 heads x K labels, by device events;
  cells    `complementarity_cells`, one launch, by device events;
  run      `run_complementarity` end to end (two launches, two host reads, the host rows), wall clock around a device synchronise;
  host     the path the reference takes on the same device arrays: their copy to the host, `sklearn.metrics.roc_curve` + argmax per
           head and label, numpy comparisons and the 16 counts, wall clock.

Each figure is the median of REPEATS windows of INNER calls after a warm-up, printed with the smallest and largest window, so the
machine's spread is on the page next to the value.  No ratio is promised; the tool prints both sides.  sklearn is needed by this tool
only, for the host side.

Usage:  python tools/time_complementarity.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from sklearn.metrics import roc_curve
from multimodal_edema_prediction_amd import complementarity as comp
from complementarity_refs import cells_ref

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER, K, SIZES = 20, 3, (2048, 8192, 16384)
LABELS = [f"label_{k}" for k in range(K)]
dev = torch.device("cuda")


def events(fn):
    """ms per call: REPEATS windows of INNER calls between two device events."""
    for _ in range(3): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / INNER)
    return out


def wall(fn, inner):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(inner): fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e3)
    return out


def show(v):
    return f"{np.median(v):9.4f} ms [{min(v):.4f} .. {max(v):.4f}]"


def split(rng, n):
    signal = rng.standard_normal((n, K))
    y = (rng.random((n, K)) < 1.0 / (1.0 + np.exp(-signal))).astype(np.float32)
    grid = lambda a: (np.round(np.clip(a, -5.9, 5.9) * 64.0) / 64.0).astype(np.float32)  # noqa: E731
    img, ts = grid(1.2 * signal + rng.standard_normal((n, K))), grid(0.8 * signal + 1.2 * rng.standard_normal((n, K)))
    d = {"img": img, "ts": ts, "fus": grid(img + 0.5 * ts), "y": y, "mask": np.ones((n, K), np.float32)}
    return {k: torch.as_tensor(v, device=dev) for k, v in d.items()}


def host_path(val, test):
    """What the reference does once its logits are gathered: everything on the host, sklearn per head and label."""
    v, t = ({k: x.cpu().numpy() for k, x in d.items()} for d in (val, test))
    thr = np.full((3, K), np.nan)
    for h, head in enumerate(comp.HEADS):
        for k in range(K):
            m = v["mask"][:, k].astype(bool)
            yy = v["y"][m, k]
            if m.sum() >= 2 and len(np.unique(yy)) == 2:
                fpr, tpr, th = roc_curve(yy, v[head][m, k])
                thr[h, k] = th[int(np.argmax(tpr - fpr))]
    return thr, cells_ref(np.stack([t[h] for h in comp.HEADS]), t["y"], t["mask"], thr)


print(f"device {torch.cuda.get_device_name(0)}; K = {K}; {REPEATS} windows of {INNER} calls (host path: of 3); median [min .. max]")
for n in SIZES:
    rng = np.random.default_rng(n)
    val, test = split(rng, n), split(rng, n)
    scores_v, y_v, mask_v = comp._stacked(val)
    scores_t, y_t, mask_t = comp._stacked(test)
    thr, _, _ = comp.youden_thresholds(scores_v, y_v, mask_v)
    want_thr, want_cells = host_path(val, test)
    rows, _, archive = comp.run_complementarity(val, test, LABELS)
    assert np.array_equal(archive["thresholds"], want_thr) and np.array_equal(archive["cells"], want_cells), "the two paths disagree"
    print(f"N = {n:6d}  youden {show(events(lambda: comp.youden_thresholds(scores_v, y_v, mask_v)))}")
    print(f"            cells  {show(events(lambda: comp.complementarity_cells(scores_t, y_t, mask_t, thr)))}")
    print(f"            run    {show(wall(lambda: comp.run_complementarity(val, test, LABELS), INNER))}")
    print(f"            host   {show(wall(lambda: host_path(val, test), 3))}")
