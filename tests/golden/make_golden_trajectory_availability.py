#!/usr/bin/env python3
"""Golden fixture for the trajectory-availability audit (analysis/trajectory_availability.py): runs the REFERENCE'S OWN `audit_dataset`
and `_print_summary` (stubs as in make_golden.py; pandas is needed here, and only here) and stores numbers and recorded text only in
tests/golden/trajectory_availability.npz.

Cases (N, T, V, n_timesteps): (37, 24, 6, 24), (40, 24, 6, 30), (5, 3, 4, 3), (1, 2, 3, 2), (130, 96, 5, 96).  Every variable draws
its hours with its own probability from {0, 0.04, 0.15, 0.5, 0.9, 1}: never-observed variables (all-NaN medians), fully observed ones,
tied sort keys.  Counts are integers 1-3 at observed cells and 0 elsewhere; values are N(0, 1) plus a per-variable offset of up to about
+-15 at observed cells and 0 elsewhere; one variable per case is held constant at 0.25 (its std is exactly 0).

Stored per case c: c<c>_x [N, T, 2V] fp32, c<c>_names, c<c>_n_timesteps, both tables column by column in the reference's row order
(c<c>_pv_<column>, c<c>_ps_<column>), the two CSV texts (`to_csv(index=False)`, what the reference's `main` writes) and the stdout of
`_print_summary`.
Asserted: no printed figure lies within 1e-6 of a rounding boundary of the 3-decimal format; some case has tied sort keys; some case
has an all-NaN median; every exact column equals tests/trajectory_availability_refs.audit_ref; the file stays under 512 KiB.
Build container only.

Usage:  python tests/golden/make_golden_trajectory_availability.py [output directory]"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from trajectory_availability_refs import PS_COLUMNS, PV_COLUMNS, STD_COLUMN, assert_tables, audit_ref, std_bounds  # noqa: E402

SEED = 23
NAMES = ("heart_rate", "sbp", "glucose, serum", "respiratory_rate_total", "spo2", "lactate")
CASES = (   # N, T, V, n_timesteps, observation probability per variable, the constant variable
    (37, 24, 6, 24, (1.0, 0.9, 0.5, 0.15, 0.04, 0.0), 1),
    (40, 24, 6, 30, (0.5, 0.0, 1.0, 0.15, 1.0, 0.04), 3),
    (5, 3, 4, 3, (0.5, 0.9, 0.0, 0.5), 1),
    (1, 2, 3, 2, (1.0, 0.5, 0.0), 0),
    (130, 96, 5, 96, (0.04, 0.15, 0.5, 0.9, 1.0), 2),
)
PRINTED = ("any_observed_rate", "trajectory_2plus_rate", "trajectory_3plus_rate", "median_observed_hours", "median_recency_h_if_observed")


def make_input(rng, N, T, V, probs, constant):
    observed = rng.random((N, T, V)) < np.asarray(probs)[None, None, :]
    offsets = rng.uniform(-15.0, 15.0, size=V)
    values = rng.standard_normal((N, T, V)) + offsets[None, None, :]
    values[:, :, constant] = 0.25
    counts = rng.integers(1, 4, size=(N, T, V))
    return np.concatenate([np.where(observed, values, 0.0), np.where(observed, counts, 0)], axis=2).astype(np.float32)


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else HERE
    install_stubs()
    sys.path.insert(0, REF)
    import analysis.trajectory_availability as ref
    rng = np.random.default_rng(SEED)
    out = {"n_cases": np.int64(len(CASES))}
    tied = all_nan = False
    for c, (N, T, V, n_timesteps, probs, constant) in enumerate(CASES):
        x = make_input(rng, N, T, V, probs, constant)
        names = list(NAMES[:V])
        dataset = [{"x_ts": torch.from_numpy(x[i])} for i in range(N)]
        per_variable, per_sample = ref.audit_dataset(dataset, names, n_timesteps)
        stdout = io.StringIO()
        with contextlib.redirect_stdout(stdout):
            ref._print_summary(per_variable, per_sample, f"case{c}")
        assert tuple(per_variable.columns) == PV_COLUMNS and tuple(per_sample.columns) == PS_COLUMNS
        p = f"c{c}_"
        out.update({p + "x": x, p + "names": np.array(names), p + "n_timesteps": np.int64(n_timesteps),
                    p + "csv_pv": np.array(per_variable.to_csv(index=False)), p + "csv_ps": np.array(per_sample.to_csv(index=False)),
                    p + "stdout": np.array(stdout.getvalue())})
        for k in PV_COLUMNS:
            col = per_variable[k].to_numpy()
            out[p + "pv_" + k] = np.array([str(s) for s in col]) if k == "variable" else col
        for k in PS_COLUMNS:
            out[p + "ps_" + k] = per_sample[k].to_numpy()
        for k in PRINTED:
            for v in per_variable[k].to_numpy():
                if np.isfinite(v):
                    frac = (abs(float(v)) * 1000.0) % 1.0
                    assert abs(frac - 0.5) > 1e-6 * 1000.0, f"case {c}: {k} = {v!r} sits on a rounding boundary of %.3f"
        keys = list(zip(per_variable["trajectory_2plus_rate"], per_variable["any_observed_rate"]))
        tied |= len(set(keys)) < len(keys)
        all_nan |= bool(np.isnan(per_variable["median_recency_h_if_observed"].to_numpy()).any())
        # the restatement the GPU tests lean on, against the reference, column by column
        case = {"x": x, "names": names}
        want = ({k: out[p + "pv_" + k].astype(object) if k == "variable" else out[p + "pv_" + k] for k in PV_COLUMNS},
                {k: out[p + "ps_" + k] for k in PS_COLUMNS})
        assert_tables(audit_ref(x, names, n_timesteps), want, std_bounds(case), f"case {c}")
        gap = np.nanmax(np.abs(audit_ref(x, names, n_timesteps)[0][STD_COLUMN] - want[0][STD_COLUMN]), initial=0.0)
        print(f"case {c}: N={N} T={T} V={V}: largest std-median gap restatement vs reference {gap:.3e}")
    assert tied, "no case has tied sort keys"
    assert all_nan, "no case has an all-NaN median"
    path = os.path.join(outdir, "trajectory_availability.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"wrote {path}: {size} bytes")


if __name__ == "__main__":
    main()
