#!/usr/bin/env python3
"""The trajectory-probe training step at the reference's defaults (B=128, V=48, T=24, d=128, 4 heads, 7 labels, windows 6/12/24,
dropout 0.1, AdamW with the 1.0 global-norm clip): eager `train_probe_batch` and the captured `GraphedTrajectoryProbeStep`,
HIP events after warm-up (the loop of tools/time_trajectory.py)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch
from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
from multimodal_edema_prediction_amd.optim import FusedAdamW
from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe, masked_bce, move_batch, train_probe_batch

torch.manual_seed(0)
B, T, V, d = 128, 24, 48, 128
dev = torch.device("cuda")
b = move_batch(make_batch(CohortCfg(n_timesteps=T, n_vars=V, n_labels=7), 0, B, mode="student"), dev)
def timed(fn, n=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
def build():
    m = TrajectoryPathologyProbe(V, 7, T, d, 1, 4, 0.1, (6, 12, 24)).to(dev).train()
    return m, FusedAdamW(m.parameters(), lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0)
m, opt = build()
print(f"parameters               : {sum(p.numel() for p in m.parameters()):,}")
print(f"eager step               : {timed(lambda: train_probe_batch(m, b, opt)):7.3f} ms")
m, opt = build()
gs = GraphedTrajectoryProbeStep(m, masked_bce, opt, b["x_ts"], b["y"], b["mask"], dev)
print(f"captured step            : {timed(lambda: gs.step(b['x_ts'], b['y'], b['mask'])):7.3f} ms")
print(f"last loss {float(gs.out['loss']):.4f}  last gradient norm {float(opt.last_grad_norm):.4f}")
del gs  # release the RNG-epoch registration before interpreter teardown
