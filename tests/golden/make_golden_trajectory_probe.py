#!/usr/bin/env python3
"""Golden fixture for `TrajectoryPathologyProbe` and `masked_bce` (analysis/train_trajectory_probe.py:98-174): runs the
REFERENCE'S OWN CLASS and loss (stubs as in make_golden.py) on seeded weights and the inputs of make_golden_trajectory.py, plus one
sample without any observation (all 18 (variable, window) keys masked), and stores inputs, weights, eval-mode logits / head-averaged
attention (observed samples) / padding mask, the loss, every parameter's gradient, the total gradient norm (above the 1.0 clip) and
the losses of three consecutive steps (clip_grad_norm_ 1.0 + AdamW lr 3e-4, wd 1e-2; dropout off).  Numbers only.  Parameters and gradients go to four
side files (encoder / read-out) so that every file stays under the 1 MiB limit for committed files.  Build container only.

Usage:  python tests/golden/make_golden_trajectory_probe.py [output directory]"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from make_golden_trajectory import synth_inputs  # noqa: E402

B, T, V, D, HEADS, K, WINDOWS = 4, 24, 6, 128, 4, 7, (6, 12, 24)
FILES = ("trajectory_probe.npz", "trajectory_probe_params_encoder.npz", "trajectory_probe_params_readout.npz",
         "trajectory_probe_grads_encoder.npz", "trajectory_probe_grads_readout.npz")


def _save(out_dir, name, arrays):
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 2 ** 20, (name, os.path.getsize(path))
    print(f"wrote {name}: {os.path.getsize(path) / 1e6:.2f} MB")


def main(out_dir=HERE):
    torch.set_num_threads(4)
    install_stubs()
    sys.path.insert(0, REF)
    from analysis.train_trajectory_probe import TrajectoryPathologyProbe, masked_bce

    torch.manual_seed(3)
    m = TrajectoryPathologyProbe(n_vars=V, n_pathologies=K, n_timesteps=T, d_model=D, gru_layers=1, n_heads=HEADS, dropout=0.1,
                                 recency_windows=WINDOWS)
    with torch.no_grad():
        for _, p in m.named_parameters():                   # livelier than the defaults (LayerNorm 1/0, zero biases)
            if p.ndim == 1:
                p.add_(0.1 * torch.randn_like(p))
    m.eval()                                                # dropout off: the parity form
    xs = synth_inputs(B + 1, T, V, seed=11)
    xs[B][:, V:] = 0.0                                      # a sample that was never observed: every key masked
    g = torch.Generator().manual_seed(5)
    y = (torch.rand(B + 1, K, generator=g) < 0.3).float()
    mask = (torch.rand(B + 1, K, generator=g) < 0.9).float()
    params = {k: p.detach().clone() for k, p in m.named_parameters()}

    _, pad = m.encoder(tuple(xs), return_padding_mask=True)
    assert bool(pad[B, :-1].all()) and not bool(pad[:B, :-1].all(dim=1).any())
    # nn.MultiheadAttention keeps the fully masked sample finite (zero attention output) on its default path only; with
    # need_weights=True its own softmax over 18 x -inf is NaN.  So: logits from the default call (all samples), the averaged
    # weights from the return_attn call for the B observed samples.
    logits = m(tuple(xs))
    attn = m(tuple(xs), return_attn=True)[1][:B]
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(attn).all())
    loss = masked_bce(logits, y, mask)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    norm = torch.sqrt(sum((v.double() ** 2).sum() for v in grads.values()))
    assert float(norm) > 1.0, float(norm)                   # so that the 1.0 clip engages

    opt = torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=1e-2)
    step_losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        ls = masked_bce(m(tuple(xs)), y, mask)
        ls.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        step_losses.append(float(ls.detach()))

    _save(out_dir, FILES[0], dict(x=torch.stack(xs), y=y, mask=mask, logits=logits, attn=attn, pad=pad[:, :-1], loss=loss,
                                  grad_norm=norm, step_losses=np.array(step_losses),
                                  cfg=np.array([B + 1, T, V, D, HEADS, K] + list(WINDOWS))))
    enc = lambda d, yes: {k: v for k, v in d.items() if k.startswith("encoder.") == yes}  # noqa: E731
    _save(out_dir, FILES[1], enc(params, True))
    _save(out_dir, FILES[2], enc(params, False))
    _save(out_dir, FILES[3], enc(grads, True))
    _save(out_dir, FILES[4], enc(grads, False))
    print(f"loss {float(loss):.6f}  grad norm {float(norm):.4f}  step losses {step_losses}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
