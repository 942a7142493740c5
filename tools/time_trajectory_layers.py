#!/usr/bin/env python3
"""Stacked trajectory encoder at the probe's shape (B 128, V 48, T 24, d 128: 6144 sequences, 147 456 rows): forward + backward of the
one- and the two-layer encoder and of the stack's node alone, and the one-layer probe step (eager and captured), timed in the SAME
process, interleaved, one pair of HIP events per call.  Prints median, 10th / 90th percentile and minimum of every series.

  python tools/time_trajectory_layers.py [--n 60] [--only-one-layer]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multimodal_edema_prediction_amd import trajectory as TR
from multimodal_edema_prediction_amd.graph_step import GraphedTrajectoryProbeStep
from multimodal_edema_prediction_amd.optim import FusedAdamW
from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe, masked_bce, train_probe_batch

B, T, V, D = 128, 24, 48, 128


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(name, ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]
    print(f"{name:52s} median {statistics.median(ts):8.3f} ms   p10 {q(0.1):8.3f}   p90 {q(0.9):8.3f}   min {ts[0]:8.3f}   n {len(ts)}", flush=True)


def interleaved(variants, n, warm=10):
    """variants: {name: fn}; every round runs each once, in turn."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(n):
        for k, fn in variants.items():
            out[k].append(once(fn))
    for k, ts in out.items():
        report(k, ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60)
    ap.add_argument("--only-one-layer", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    x = torch.cat([torch.randn(B, T, V), torch.poisson(torch.full((B, T, V), 0.5))], dim=2).cuda()
    y, mask = (torch.rand(B, 7) < 0.4).float().cuda(), (torch.rand(B, 7) < 0.8).float().cuda()
    batch = {"x_ts": x, "y": y, "mask": mask}

    def probe(layers):
        torch.manual_seed(1)
        m = TrajectoryPathologyProbe(n_vars=V, n_pathologies=7, n_timesteps=T, d_model=D, gru_layers=layers, n_heads=4, dropout=0.1,
                                     recency_windows=(6, 12, 24)).cuda().train()
        return m, FusedAdamW(m.parameters(), lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0)

    if not a.only_one_layer:
        xs = tuple(x)
        encs = {L: TR.LocalTrajectoryEncoder(n_vars=V, n_timesteps=T, d_model=D, n_layers=L, dropout=0.1).cuda().train() for L in (1, 2)}

        def fwdbwd(enc):
            def run():
                enc.zero_grad(set_to_none=True)
                enc(xs).square().mean().backward()
            return run
        print(f"encoder, forward + backward, B {B} V {V} T {T} (train mode, dropout 0.1)")
        interleaved({"  one layer": fwdbwd(encs[1]), "  two layers": fwdbwd(encs[2])}, a.n)

        S = B * V
        gi = torch.randn(S, T, 3 * D, device="cuda", requires_grad=True)
        g = encs[2].temporal
        params = [g.weight_hh_l0, g.bias_hh_l0, g.weight_ih_l1, g.weight_hh_l1, g.bias_ih_l1, g.bias_hh_l1]
        dh = torch.randn(S, T, D, device="cuda")

        def stack(bwd):
            def run():
                if bwd:
                    TR.GruStackFn.apply(gi, 0.1, 17, *params).backward(dh)
                else:
                    with torch.no_grad():
                        TR.GruStackFn.apply(gi, 0.1, 17, *params)
            return run
        print("the stack's node alone (two layers)")
        interleaved({"  forward": stack(False), "  forward + backward": stack(True)}, a.n)

    print(f"one-layer probe step, B {B} V {V} T {T} (train mode, dropout 0.1, clip 1.0)")
    me, oe = probe(1)
    mg, og = probe(1)
    gs = GraphedTrajectoryProbeStep(mg, masked_bce, og, x, y, mask, torch.device("cuda"))
    interleaved({"  eager step": lambda: train_probe_batch(me, batch, oe), "  captured step": lambda: gs.step(x, y, mask)}, a.n)


if __name__ == "__main__":
    main()
