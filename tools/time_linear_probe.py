#!/usr/bin/env python3
"""The linear-head trainer (csrc/head_probe.hip) at N = 20 000 train / 4 000 val rows, L = 7 labels, bs 128, 90 % of the labels
known, for the feature widths F = 768 (CLS / REP), 1176 (hourly tokens of the benchmark DuETT) and 4704 (multiscale):
  * HIP-event time of one `medp_head_train_epoch` launch (156 sequential steps) for P = 1 per width and for the three widths in
    one launch (P = 3), with the per-step time and the bytes a step streams (bs F 4 B, read in phase A and again in phase B);
  * the per-epoch selection chain (scores of the validation rows, the metrics launch, keep-best) per head;
  * wall clock of a whole `train_linear_head` (default 300 epochs) around ONE synchronise;
  * beside them the eager fallback loop (`head_probe.eager_fit`, torch autograd on the same device and data) for 3 epochs,
    scaled to the same number of epochs.  The eager loop is the comparator because nothing else trains these heads.

Usage:  python tools/time_linear_probe.py [epochs]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodal_edema_prediction_amd import head_probe, probe_stats, unimodal_linear_probe as ulp

EPOCHS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
N_TR, N_VA, L, BS, WIDTHS = 20_000, 4_000, 7, 128, (768, 1176, 4704)
dev = torch.device("cuda")
LABELS = [f"label_{i}" for i in range(L)]


def synth(n, F, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, F, generator=g)
    logit = -1.0 + X[:, :2 * L:2] + 0.5 * X[:, 1:2 * L:2]
    Y = (torch.rand(n, L, generator=g) < torch.sigmoid(logit)).float()
    M = (torch.rand(n, L, generator=g) < 0.9).float()
    return X.to(dev), Y.to(dev), M.to(dev)


def timed(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


data = {F: (synth(N_TR, F, F), synth(N_VA, F, F + 1)) for F in WIDTHS}
S = N_TR // BS
perm = torch.as_tensor(np.random.default_rng(0).permutation(N_TR)[:S * BS].astype(np.int32), device=dev)


def problem(F):
    (X, Y, M), _ = data[F]
    torch.manual_seed(0)
    head = ulp.LinearHead(F, L).head[1]
    return head_probe.HeadProblem(X, Y, M, head.weight, head.bias, bs=BS, lr=1e-4, weight_decay=1e-4, dropout=0.1, seed=1)


print(f"N = {N_TR} train / {N_VA} val, L = {L}, bs = {BS}: {S} steps per epoch")
for F in WIDTHS:
    pb = problem(F)
    t = timed(lambda: head_probe.head_train_epoch([pb], [perm]))
    where = "LDS" if head_probe.onchip(F, L, 0, BS) else "global (L2)"
    print(f"  head_train_epoch P = 1, F = {F:5d} (W, m, v in {where:11s}): {t:8.3f} ms per epoch = {t / S * 1e3:7.1f} us per step; "
          f"a step streams {BS * F * 4 / 1e6:.2f} MB twice")
pbs = [problem(F) for F in WIDTHS]
t = timed(lambda: head_probe.head_train_epoch(pbs, [perm] * 3))
print(f"  head_train_epoch P = 3, the three widths in one launch  : {t:8.3f} ms per epoch (the widest problem sets the time)")
for F in WIDTHS:
    pb = problem(F)
    _, (Xv, Yv, Mv) = data[F]
    metrics = probe_stats.LabelMetrics(Yv, Mv)
    best = {"v": torch.full((), -float("inf"), dtype=torch.float64, device=dev), "W": pb.W.clone()}

    def select():
        _, probs = head_probe.head_scores(Xv, pb.W, pb.b)
        macro = probe_stats.nan_mean(metrics(probs)[:, 1])
        better = macro > best["v"]
        best["v"] = torch.where(better, macro, best["v"])
        best["W"] = torch.where(better, pb.W, best["W"])

    print(f"  selection chain (scores, metrics, keep-best), F = {F:5d}  : {timed(select):8.3f} ms per epoch")

for F in WIDTHS:
    (X, Y, M), (Xv, Yv, Mv) = data[F]
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, ep, val = ulp.train_linear_head(X, Y, M, Xv, Yv, Mv, LABELS, dev, epochs=EPOCHS, batch_size=BS, verbose=False, seed=1)
    torch.cuda.synchronize()
    t_hip = time.perf_counter() - t0
    torch.manual_seed(0)
    model = ulp.LinearHead(F, L).to(dev)
    perms = head_probe.draw_epoch_permutations(N_TR, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    head_probe.eager_fit(model, lambda m, x: m(x), [X], Y, M, [Xv], Yv, Mv, epochs=3, batch_size=BS, lr=1e-4, weight_decay=1e-4, perms=perms)
    torch.cuda.synchronize()
    t_eager = (time.perf_counter() - t0) / 3 * EPOCHS
    print(f"  train_linear_head, {EPOCHS} epochs, F = {F:5d}: {t_hip:7.2f} s wall (best epoch {ep}, val macro AUROC {val:.4f}); "
          f"eager loop, 3 epochs scaled to {EPOCHS}: {t_eager:7.2f} s  ({t_eager / t_hip:.1f} x)")
