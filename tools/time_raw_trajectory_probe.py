#!/usr/bin/env python3
"""The raw-trajectory conditional probe on a synthetic split (N = 4096 windows per split, two per subject, T = 96, V = 48; the
reference's defaults otherwise: recent_hours 6, 7 L2 strengths + the null candidate, 5 folds, 1000 bootstrap replicates, 100
conditional permutations): the three kernels of csrc/raw_probe.hip by HIP events after warm-up (the loop of tools/time_trajectory.py)
and the whole `run_probe` by wall clock.  For the objective/gradient kernel the time per evaluation is printed beside
bytes(X) / peak HBM bandwidth (8 TB/s), the floor of a kernel that reads X once.

Usage:  python tools/time_raw_trajectory_probe.py [N]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodal_edema_prediction_amd import probe_stats, raw_trajectory_probe as rp

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T, V, RECENT, HBM_PEAK = 96, 48, 6, 8.0e12
dev = torch.device("cuda")


def synth_split(n, seed):
    """x [n,T,2V] fp32 (values | counts), subjects, image logits, labels: un-normalised values, per-variable observation rates from
    hourly vitals to rare labs, some variables never observed in a window; the label depends on the image and on two variables' level."""
    pop = np.random.default_rng(0)                                        # the population is the same for every split
    centre, spread = pop.uniform(1.0, 120.0, V), pop.uniform(0.5, 15.0, V)
    rate = np.concatenate([pop.uniform(0.5, 0.95, V // 3), pop.uniform(0.02, 0.3, V - V // 3)])
    rng = np.random.default_rng(seed)
    base = centre + spread * rng.standard_normal((n, V))
    seen = rng.random((n, T, V)) < rate
    seen &= ~(rng.random((n, 1, V)) < 0.1)                                # never observed in this window
    val = base[:, None, :] + 0.3 * spread * rng.standard_normal((n, T, V))
    cnt = np.where(seen, 1 + rng.poisson(0.5, (n, T, V)), 0)
    x = np.concatenate([np.where(seen, val, 0.0), cnt], 2).astype(np.float32)
    image = 1.3 * rng.standard_normal(n)
    logit = -0.5 + 0.9 * image + 0.8 * (base[:, 0] - centre[0]) / spread[0] - 0.6 * (base[:, 1] - centre[1]) / spread[1]
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.int64)
    return x, np.repeat(np.arange(n // 2), 2), image, y


def timed(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


names = [f"v{i:02d}" for i in range(V)]
x_tr, _, img_tr, y_tr = synth_split(N, 1)
x_te, subj_te, img_te, y_te = synth_split(N, 2)
xd_tr, xd_te = torch.as_tensor(x_tr, device=dev), torch.as_tensor(x_te, device=dev)
print(f"split: N = {N} windows, T = {T}, V = {V}; positives {int(y_tr.sum())} / {int(y_te.sum())}")
print(f"raw_traj_summary         : {timed(lambda: rp.raw_traj_summary(xd_tr, RECENT)):9.3f} ms   ({N} x {V} (window, variable) scans)")

train, block_names = rp.raw_summary_blocks(xd_tr, names, RECENT)
test, _ = rp.raw_summary_blocks(xd_te, names, RECENT)
X = rp.Preprocessor.fit(train["all"]).transform(train["all"])
n, F = X.shape
G = len(rp.DEFAULT_L2_GRID)
yd, off = torch.as_tensor(y_tr, dtype=torch.float64, device=dev), torch.as_tensor(img_tr, dtype=torch.float64, device=dev)
W = 0.01 * torch.randn((F, G), dtype=torch.float64, device=dev)
l2 = torch.tensor(rp.DEFAULT_L2_GRID, dtype=torch.float64, device=dev)
ws = rp.valgrad_workspace(n, F, G, dev)
ms = timed(lambda: rp.offset_logistic_valgrad(X, yd, off, W, l2, ws), 50)
floor_ms = n * F * 8 / HBM_PEAK * 1e3
print(f"offset_logistic_valgrad  : {ms:9.4f} ms per evaluation  (n = {n}, F = {F}, G = {G}; bytes(X) = {n * F * 8 / 1e6:.1f} MB, "
      f"bytes(X) / 8 TB/s = {floor_ms:.4f} ms, ratio {ms / floor_ms:.1f}; workspace {ws.numel() * 8 / 1e6:.1f} MB)")

idx, offsets = probe_stats.draw_cluster_bootstrap_indices(subj_te, 1000, 42)
yu, idx_d, off_d = torch.as_tensor(y_te.astype(np.uint8), device=dev), torch.as_tensor(idx, device=dev), torch.as_tensor(offsets, device=dev)
p = torch.sigmoid(torch.as_tensor(img_te, dtype=torch.float64, device=dev))[None]
longest = int(np.diff(offsets).max())
print(f"resampled_binary_metrics : {timed(lambda: probe_stats.resampled_binary_metrics(yu, p, idx_d, off_d, longest), 10):9.3f} ms   "
      f"(1000 bootstrap replicates, longest {longest})")

torch.cuda.synchronize()
t0 = time.perf_counter()
rows, _ = rp.run_probe(train, test, block_names, y_tr, y_te, img_tr, img_te, subj_te)
torch.cuda.synchronize()
print(f"run_probe, five blocks   : {time.perf_counter() - t0:9.2f} s wall  (calibration, 5 x (6 batched fits, 1000 bootstrap, 100 permutations))")
for r in rows:
    print(f"  {r['block']:12s} {r['best_params']:58s} BCE gain {r['bce_gain']:+.5f} [{r['bce_gain_ci_low']:+.5f}, {r['bce_gain_ci_high']:+.5f}]  {r['evidence']}")
