#!/usr/bin/env python3
"""The linear-head trainer (csrc/head_probe.hip) at N = 20 000 train / 4 000 val rows, L = 7 labels, bs 128, 90 % of the labels
known, for the feature widths F = 768 (CLS / REP), 1176 (hourly tokens of the benchmark DuETT) and 4704 (multiscale):
  * HIP-event time of one `medp_head_train_epoch` launch (156 sequential steps) for P = 1 per width and for the three widths in
    one launch (P = 3), with the per-step time and the bytes a step streams (bs F 4 B, read in phase A and again in phase B);
  * the per-epoch selection chain (scores of the validation rows, the metrics launch, keep-best) per head;
  * wall clock of a whole `train_linear_head` (default 300 epochs) around ONE synchronise;
  * beside them the eager fallback loop (`head_probe.eager_fit`, torch autograd on the same device and data) for 3 epochs,
    scaled to the same number of epochs.  The eager loop is the comparator because nothing else trains these heads;
  * the two heads with a hidden stage (csrc/pool_head_probe.hip), each beside `eager=True` on the same inputs in the same process:
    attention pooling at N 20 000 / T 24 / d 1176 (tokens in LDS) and d 2328 (re-read from global memory) / L 7 / bs 128: one
    `medp_pool_head_train_epoch` call (156 steps, two launches each) and the validation scores by HIP events, then
    `train_linear_head(use_attn_pool=True)` for a few epochs by wall clock, device path and eager; the mlp fusion head at
    L 7 / H 32 the same way.  `--hidden-heads` runs this part alone.

Usage:  python tools/time_linear_probe.py [epochs] [--hidden-heads]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodal_edema_prediction_amd import head_probe, logit_fusion_probe as lfp, probe_stats, unimodal_linear_probe as ulp

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
EPOCHS = int(ARGS[0]) if ARGS else 300
HIDDEN_ONLY = "--hidden-heads" in sys.argv
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


def hidden_heads():
    """Attention pooling and the mlp fusion head: device path next to eager=True, per epoch."""
    T, H, E_DEV, E_EAGER = 24, 32, 5, 2
    S = N_TR // BS
    g = torch.Generator(device=dev).manual_seed(0)
    Y, M = (torch.rand(N_TR, L, generator=g, device=dev) < 0.3).float(), (torch.rand(N_TR, L, generator=g, device=dev) < 0.9).float()
    Yv, Mv = (torch.rand(N_VA, L, generator=g, device=dev) < 0.3).float(), (torch.rand(N_VA, L, generator=g, device=dev) < 0.9).float()
    perm = np.random.default_rng(0).permutation(N_TR)[:S * BS].astype(np.int32)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print(f"hidden-stage heads: N = {N_TR} train / {N_VA} val, L = {L}, bs = {BS}: {S} steps per epoch")
    for d in (1176, 2328):
        X, Xv = torch.randn(N_TR, T, d, generator=g, device=dev), torch.randn(N_VA, T, d, generator=g, device=dev)
        torch.manual_seed(0)
        m = ulp.LinearHead(d, L, use_attn_pool=True)
        pb = head_probe.PoolHeadProblem(X, Y, M, m.attn_query, m.head[1].weight, m.head[1].bias, bs=BS, lr=1e-4, weight_decay=1e-4, dropout=0.1, seed=1)
        t = timed(lambda: head_probe.pool_head_train_epoch(pb, perm), n=5)
        where = "LDS" if head_probe.pool_rows_onchip(T, d) else "global / L2"
        print(f"  pool_head_train_epoch T = {T}, d = {d} (row tokens in {where}): {t:8.3f} ms per epoch = {t / S * 1e3:7.1f} us per step of two launches; "
              f"a step reads {BS * T * d * 4 / 1e6:.1f} MB of tokens")
        ts = timed(lambda: head_probe.pool_head_scores(Xv, pb.q, pb.W, pb.b), n=5)
        print(f"  pool_head_scores, {N_VA} rows, d = {d}: {ts:8.3f} ms")
        kw = dict(batch_size=BS, verbose=False, use_attn_pool=True, seed=1)
        for eager in (False, True):                                         # first-use costs of either path stay out of the clock
            ulp.train_linear_head(X, Y, M, Xv, Yv, Mv, LABELS, dev, epochs=1, eager=eager, **kw)
        torch.manual_seed(0)
        t_dev = wall(lambda: ulp.train_linear_head(X, Y, M, Xv, Yv, Mv, LABELS, dev, epochs=E_DEV, eager=False, **kw)) / E_DEV
        torch.manual_seed(0)
        t_eag = wall(lambda: ulp.train_linear_head(X, Y, M, Xv, Yv, Mv, LABELS, dev, epochs=E_EAGER, eager=True, **kw)) / E_EAGER
        print(f"  train_linear_head(use_attn_pool=True), d = {d}: device path {t_dev * 1e3:8.1f} ms per epoch ({E_DEV} epochs, wall); "
              f"eager=True {t_eag * 1e3:8.1f} ms per epoch ({E_EAGER} epochs, wall)  ({t_eag / t_dev:.1f} x)")
        del X, Xv, pb
    img, ts_, imgv, tsv = (torch.randn(n, L, generator=g, device=dev) for n in (N_TR, N_TR, N_VA, N_VA))
    torch.manual_seed(0)
    f = lfp.LogitFusionHead(L, "mlp", hidden=H)
    pb = head_probe.MlpHeadProblem(torch.cat([img, ts_], -1), Y, M, f.head[0].weight, f.head[0].bias, f.head[3].weight, f.head[3].bias, bs=BS,
                                   dropout=0.1, seed=1)
    t = timed(lambda: head_probe.mlp_head_train_epoch([pb], [perm]))
    print(f"  mlp_head_train_epoch L = {L}, H = {H}: {t:8.3f} ms per epoch = {t / S * 1e3:7.1f} us per step (one launch per epoch)")
    kw = dict(fusion_type="mlp", hidden=H, batch_size=BS, verbose=False, seed=1)
    for eager in (False, True):
        lfp.train_fusion_head(img, ts_, Y, M, imgv, tsv, Yv, Mv, LABELS, dev, epochs=1, eager=eager, **kw)
    torch.manual_seed(0)
    t_dev = wall(lambda: lfp.train_fusion_head(img, ts_, Y, M, imgv, tsv, Yv, Mv, LABELS, dev, epochs=4 * E_DEV, eager=False, **kw)) / (4 * E_DEV)
    torch.manual_seed(0)
    t_eag = wall(lambda: lfp.train_fusion_head(img, ts_, Y, M, imgv, tsv, Yv, Mv, LABELS, dev, epochs=E_EAGER, eager=True, **kw)) / E_EAGER
    print(f"  train_fusion_head(fusion_type='mlp'), H = {H}: device path {t_dev * 1e3:8.1f} ms per epoch ({4 * E_DEV} epochs, wall); "
          f"eager=True {t_eag * 1e3:8.1f} ms per epoch ({E_EAGER} epochs, wall)  ({t_eag / t_dev:.1f} x)")


if HIDDEN_ONLY:
    hidden_heads()
    sys.exit(0)

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

hidden_heads()
