#!/usr/bin/env python3
"""Golden fixture for the STACKED `LocalTrajectoryEncoder` (n_layers > 1; models/main_architecture_duett.py:1242-1391, the
`nn.GRU(num_layers=n_layers, dropout=...)` of :1296-1302): runs the REFERENCE'S OWN CLASS (stubs as in make_golden.py) in eval()
on seeded weights and inputs that include unobserved windows.  Build container only.

Three files, each below the 1 MiB limit of a committed file:
  trajectory_layers.npz        n_layers = 2: cfg, x, tokens, pad, wgt and the state_dict (`p_<name>`)
  trajectory_layers_grads.npz  n_layers = 2: the gradient of sum(tokens * wgt) with respect to every parameter (`g_<name>`)
  trajectory_layers_l3.npz     n_layers = 3, forward only: the same inputs and the same weights for everything the two-layer model
                               has; only the third GRU layer's four tensors are new and stored (`p_temporal.*_l2`), and the tokens.

Usage:  python tests/golden/make_golden_trajectory_layers.py [out_dir]"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

B, T, V, D, WINDOWS = 2, 24, 3, 128, (6, 12, 24)


def synth_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(B, T, V, generator=g)
    counts = torch.poisson(torch.full((B, T, V), 0.7), generator=g)
    counts[:, :, 0] = 0.0                     # a variable that is never observed
    counts[0, :, 1] = 0.0                     # ... and one unobserved in one sample only
    counts[:, -6:, 2] = 0.0                   # nothing in the most recent window
    counts[1, 3, 1] = -1.0                    # negative count (clamped by the module)
    return [torch.cat([vals[b], counts[b]], dim=1) for b in range(B)]


def _save(out_dir, name, arrays):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(out_dir, name), **out)
    print(f"wrote {name}: {os.path.getsize(os.path.join(out_dir, name)) / 2 ** 20:.2f} MiB")


def main(out_dir=HERE):
    torch.set_num_threads(4)
    install_stubs()
    sys.path.insert(0, REF)
    from models.main_architecture_duett import LocalTrajectoryEncoder

    def build(n_layers, seed):
        torch.manual_seed(seed)
        m = LocalTrajectoryEncoder(n_vars=V, n_timesteps=T, d_model=D, n_layers=n_layers, dropout=0.1, recency_windows=WINDOWS)
        with torch.no_grad():
            for k, p in m.named_parameters():             # livelier than the defaults (LayerNorm 1/0, small embeddings)
                if p.ndim == 1:
                    p.add_(0.1 * torch.randn_like(p))
        return m.eval()                                   # dropout off: the parity form

    xs = synth_inputs(seed=123)
    wgt = torch.randn((B, V * len(WINDOWS) + 1, D), generator=torch.Generator().manual_seed(56))
    cfg = np.array([B, T, V, D] + list(WINDOWS))

    m2 = build(2, 202)
    tokens, pad = m2(tuple(xs), return_padding_mask=True)
    (tokens * wgt).sum().backward()
    main_file = {"cfg": cfg, "x": torch.stack(xs), "tokens": tokens, "pad": pad, "wgt": wgt}
    main_file.update({f"p_{k}": v for k, v in m2.state_dict().items()})
    _save(out_dir, "trajectory_layers.npz", main_file)
    _save(out_dir, "trajectory_layers_grads.npz", {f"g_{k}": p.grad for k, p in m2.named_parameters()})

    m3 = build(3, 303)
    m3.load_state_dict(m2.state_dict(), strict=False)     # layers 0 and 1 and everything around the GRU: the two-layer model's
    tokens3, pad3 = m3(tuple(xs), return_padding_mask=True)
    assert torch.equal(pad3, pad)
    l3 = {"cfg": cfg, "tokens": tokens3}
    l3.update({f"p_{k}": v for k, v in m3.state_dict().items() if k.endswith("_l2")})
    _save(out_dir, "trajectory_layers_l3.npz", l3)


if __name__ == "__main__":
    main(*sys.argv[1:2])
