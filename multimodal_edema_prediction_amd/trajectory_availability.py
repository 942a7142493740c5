"""Do the pre-CXR windows hold per-variable trajectories at all (reference analysis/trajectory_availability.py)?  A data audit, not a
model: a variable can only contribute a slope when it is observed in at least two hours of the window, a shape from three.  Its verdict
is the reason to train, or not to train, the `LocalTrajectoryEncoder` and the trajectory probes.

    python -m multimodal_edema_prediction_amd.trajectory_availability --split train --out_csv trajectory_availability_train.csv

The reference's names (`_print_summary` without its underscore).  pandas is not a dependency: both tables are column dictionaries
(name -> numpy array) with the reference's column names, dtypes and row order, and `print_summary` / `save_csv` lay them out as
`DataFrame.to_string` / `to_csv` do.

What runs where
  device, HIP   `trajectory_cells` (csrc/trajectory_audit.hip): per (sample, variable) observed hours, count total, recency, within-patient
                std, endpoint change, and the per-sample / per-variable counts; a dataset streams through it in chunks.
                `probe_stats.column_medians`: the five per-variable medians and the three per-sample ones of the summary line, by exact
                radix selection over the full columns (four launches).
  host          rates and the mean as integer / N in fp64, the sort, the text.  ONE synchronisation, at the end of `audit_dataset`.
Without a GPU `audit_dataset` and `main` raise (no CPU fallback)."""
from __future__ import annotations

import argparse
import csv
import math
import os
from typing import Dict, Sequence

import numpy as np
import torch

from .abi import check, lib, ptr, require_gpu, stream
from .probe_stats import column_medians

CHUNK = 256                        # samples per `trajectory_cells` launch when a dataset is streamed (a DataLoader-sized batch)
PRINTED = ("variable", "any_observed_rate", "trajectory_2plus_rate", "trajectory_3plus_rate", "median_observed_hours",
           "median_recency_h_if_observed")
SAMPLE_COUNTS = ("n_variables_observed", "n_variables_with_trajectory_2plus", "n_variables_with_trajectory_3plus",
                 "n_observed_variable_hours")


class SampleTable(dict):
    """The per-sample columns; `medians` carries the device medians of the first three count columns for the summary line."""
    medians: tuple | None = None


# ------------------------------------------------------------------------------------------------------------------------------
# kernel
# ------------------------------------------------------------------------------------------------------------------------------
class CellPlanes:
    """The output of `trajectory_cells` for `capacity` samples: variable-major planes [V, capacity], per_sample [capacity, 4] int32,
    var_counts [V, 4] int64 (zeroed here, the kernel adds).  The fp32 planes share one buffer, so one launch takes three medians."""

    def __init__(self, V: int, capacity: int, device):
        self.V, self.capacity = V, capacity
        self.obs_hours = torch.empty((V, capacity), dtype=torch.int32, device=device)
        self.f32 = torch.empty((4, V, capacity), dtype=torch.float32, device=device)
        self.total, self.recency, self.within_std, self.endpoint_change = self.f32[0], self.f32[1], self.f32[2], self.f32[3]
        self.per_sample = torch.empty((capacity, 4), dtype=torch.int32, device=device)
        self.var_counts = torch.zeros((V, 4), dtype=torch.int64, device=device)


def trajectory_cells(x: torch.Tensor, n_timesteps: int, planes: CellPlanes | None = None, n0: int = 0) -> CellPlanes:
    """x [n, T, 2V] fp32 on the device (values | counts) -> the planes of samples n0 .. n0 + n - 1 (`medp_trajectory_cells`).  Without
    `planes` a fresh set for exactly n samples; with it, a chunk of a stream: the planes end bit-identical to those of one call."""
    require_gpu()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("trajectory_cells operates on GPU tensors; there is no CPU fallback")
    if x.dtype != torch.float32 or x.ndim != 3 or x.shape[2] % 2 or 0 in x.shape:
        raise TypeError("trajectory_cells: x is fp32 [n, T, 2V]")
    x = x.contiguous()
    n, T, V = x.shape[0], x.shape[1], x.shape[2] // 2
    if planes is None:
        planes = CellPlanes(V, n0 + n, x.device)
    if planes.V != V:
        raise ValueError(f"trajectory_cells: the planes hold {planes.V} variables, x has {V}")
    check(lib().medp_trajectory_cells(ptr(x), n, T, V, int(n_timesteps), int(n0), planes.capacity, ptr(planes.obs_hours), ptr(planes.total),
                                      ptr(planes.recency), ptr(planes.within_std), ptr(planes.endpoint_change), ptr(planes.per_sample),
                                      ptr(planes.var_counts), stream()), "trajectory_cells")
    return planes


# ------------------------------------------------------------------------------------------------------------------------------
# the audit
# ------------------------------------------------------------------------------------------------------------------------------
def _item_x(item) -> torch.Tensor:
    return item["x_ts"] if isinstance(item, dict) else item


def _stream_cells(source, n: int, V: int, n_timesteps: int, device) -> CellPlanes:
    """Items `source[0 .. n)` (dicts with x_ts, or the x_ts tensors of a collated tuple) through the kernel in chunks of CHUNK."""
    planes, shape = CellPlanes(V, n, device), None
    for n0 in range(0, n, CHUNK):
        items = [_item_x(source[i]) for i in range(n0, min(n0 + CHUNK, n))]
        for x in items:
            shape = tuple(x.shape) if shape is None else shape
            if tuple(x.shape) != shape:
                raise ValueError(f"trajectory availability audits windows of one length: x_ts {tuple(x.shape)} after {shape}")
        if len(shape) != 2 or shape[1] != 2 * V:
            raise ValueError(f"x_ts is [T, 2V] with V = {V} variable names, got {shape}")
        trajectory_cells(torch.stack(items).to(device=device, dtype=torch.float32), n_timesteps, planes, n0)
    return planes


def audit_dataset(dataset, variable_names: Sequence[str], n_timesteps: int, max_samples: int = 0):
    """`audit_dataset` (:56-109) -> (per_variable, per_sample): column dictionaries with the reference's columns, dtypes and row order
    (per_variable sorted by trajectory_2plus_rate, then any_observed_rate, descending, ties in input order; per_sample in sample order).
    `dataset`: items with `x_ts` [T, 2V]; a collated tuple / list of such tensors; or a device tensor [N, T, 2V].  One window length
    only (ValueError otherwise).  within-patient std is fp64 arithmetic rounded once to fp32, a little MORE accurate than the
    reference's fp32 numpy arithmetic; every other figure is the reference's bit for bit.  (One corner is not reproduced: a column whose
    valid entries are all infinite has that infinity for its median here, NaN in the reference's `_nanmedian`.)"""
    require_gpu()
    variable_names = [str(s) for s in variable_names]
    V = len(variable_names)
    n = len(dataset) if max_samples <= 0 else min(len(dataset), int(max_samples))
    if n < 1 or V < 1:
        raise ValueError("audit_dataset: no sample or no variable to audit")
    if isinstance(dataset, torch.Tensor):
        if dataset.ndim != 3 or dataset.shape[2] != 2 * V:
            raise ValueError(f"x is [N, T, 2V] with V = {V} variable names, got {tuple(dataset.shape)}")
        planes = trajectory_cells(dataset[:n], n_timesteps)
    else:
        planes = _stream_cells(dataset, n, V, n_timesteps, torch.device("cuda", torch.cuda.current_device()))
    # eight medians, four launches: int32 hours; total | recency | std in one; |endpoint change|; the per-sample counts
    med_hours, _ = column_medians(planes.obs_hours)
    med_f32, valid_f32 = column_medians(planes.f32[:3].reshape(3 * V, n))
    med_abs, _ = column_medians(planes.endpoint_change, take_abs=True)
    med_sample, _ = column_medians(planes.per_sample.t()[:3].contiguous())
    flat = torch.cat([planes.var_counts.reshape(-1).to(torch.float64), med_hours, med_f32, med_abs, med_sample,
                      valid_f32[:V].to(torch.float64)])                     # integers far below 2^53: exact in fp64
    host_flat = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
    host_rows = torch.empty(planes.per_sample.shape, dtype=torch.int32, pin_memory=True)
    host_flat.copy_(flat, non_blocking=True)
    host_rows.copy_(planes.per_sample, non_blocking=True)
    torch.cuda.current_stream().synchronize()                                # the audit's one synchronisation
    flat, rows = host_flat.numpy().copy(), host_rows.numpy().astype(np.int64)
    counts, flat = flat[:4 * V].reshape(V, 4), flat[4 * V:]
    med_hours, med_total, med_recency, med_std, med_abs = (flat[i * V:(i + 1) * V] for i in range(5))
    med_sample, total_valid = flat[5 * V:5 * V + 3], flat[5 * V + 3:]
    med_total = np.where(total_valid < n, np.nan, med_total)                 # np.median, not nanmedian: a NaN count makes it NaN
    columns = {
        "variable": np.array(variable_names, dtype=object), "n_samples": np.full(V, n, dtype=np.int64),
        "any_observed_rate": counts[:, 0] / n, "trajectory_2plus_rate": counts[:, 1] / n, "trajectory_3plus_rate": counts[:, 2] / n,
        "median_observed_hours": med_hours, "mean_observed_hours": counts[:, 3] / n, "median_total_measurements": med_total,
        "median_recency_h_if_observed": med_recency, "median_within_patient_std_if_2plus": med_std,
        "median_abs_endpoint_change_if_2plus": med_abs,
    }
    order = sorted(range(V), key=lambda j: (-columns["trajectory_2plus_rate"][j], -columns["any_observed_rate"][j]))   # stable
    per_variable = {name: col[order] for name, col in columns.items()}
    per_sample = SampleTable({"sample_index": np.arange(n, dtype=np.int64)})
    per_sample.update({name: rows[:, i].copy() for i, name in enumerate(SAMPLE_COUNTS)})
    per_sample.medians = tuple(float(m) for m in med_sample)
    return per_variable, per_sample


# ------------------------------------------------------------------------------------------------------------------------------
# outputs
# ------------------------------------------------------------------------------------------------------------------------------
def _to_string(table: Dict[str, np.ndarray], names: Sequence[str], rows: slice) -> str:
    """`DataFrame[names].iloc[rows].to_string(index=False, float_format="%.3f")`: right-justified columns one space apart, the header of
    a numeric column with a space in front, NaN as NaN, no cell cut short."""
    strcols = []
    for name in names:
        col = np.asarray(table[name])[rows]
        numeric = col.dtype.kind in "fiu"
        header = " " + name if numeric else name
        if col.dtype.kind == "f":
            cells = ["NaN" if math.isnan(v) else f"{v:.3f}" for v in col.tolist()]
        else:
            cells = [str(v) for v in col.tolist()]
        width = max([len(header)] + [len(c) for c in cells])
        strcols.append([s.rjust(width) for s in [header] + cells])
    return "\n".join(" ".join(line) for line in zip(*strcols))


def print_summary(per_variable, per_sample, split: str) -> None:
    """`_print_summary` (:112-139), character for character.  The three per-patient medians are the device's where `per_sample` comes
    from `audit_dataset`; for plain columns (a table read back from its CSV) they are numpy's, the same numbers."""
    medians = getattr(per_sample, "medians", None) or tuple(float(np.median(per_sample[c])) for c in SAMPLE_COUNTS[:3])
    print(f"\n=== 24 h trajectory availability: split={split}, n={len(per_sample['sample_index'])} ===")
    print("Definition: >=2 observed hours can express a change; >=3 can express a shape.")
    print("Per patient median: "
          f"observed variables={medians[0]:.0f}, "
          f">=2h variables={medians[1]:.0f}, "
          f">=3h variables={medians[2]:.0f}")
    V = len(per_variable["variable"])
    print("\nTop variables with usable trajectories")
    print(_to_string(per_variable, PRINTED, slice(0, 15)))
    print("\nVariables with little/no usable trajectory")
    print(_to_string(per_variable, PRINTED, slice(max(V - 15, 0), V)))
    median_two = medians[1]
    if median_two < 3:
        verdict = "VERY SPARSE: most inputs contain levels/missingness, not multivariable trajectories."
    elif median_two < 8:
        verdict = "SPARSE: trajectory modeling is plausible for only a small variable subset."
    else:
        verdict = "TRAJECTORY-RICH: an encoder that preserves variable-wise temporal structure is justified."
    print(f"\nVerdict: {verdict}")


def save_csv(table: Dict[str, np.ndarray], path: str) -> None:
    """`DataFrame.to_csv(path, index=False)`: floats as their shortest round-trip text, NaN as an empty field, integers plain."""
    def field(v):
        if isinstance(v, float):
            return "" if math.isnan(v) else repr(v)
        return v
    names = list(table)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(names)
        for row in zip(*(np.asarray(table[name]).tolist() for name in names)):
            w.writerow([field(v) for v in row])


# ------------------------------------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser("Audit pre-CXR trajectory availability")
    p.add_argument("--n_timesteps", type=int, default=24)
    p.add_argument("--n_vars", type=int, default=48)
    p.add_argument("--d_static", type=int, default=8)
    p.add_argument("--n_train", type=int, default=4096)
    p.add_argument("--n_val", type=int, default=1024)
    p.add_argument("--n_test", type=int, default=1024)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--learnable_labels", action="store_true", help="the cohort whose labels depend on the inputs (same x_ts either way)")
    p.add_argument("--split", choices=["train", "val", "test", "all"], default="train")
    p.add_argument("--max_samples", type=int, default=0,
                   help="0=all samples; positive values are useful for a quick check")
    p.add_argument("--out_csv", default="trajectory_availability.csv")
    return p.parse_args(argv)


def main(argv=None) -> dict:
    """The reference's `main()` (:142-171) on the splits of `train_synthetic`'s synthetic cohort (time series only, no images)."""
    from . import train_synthetic
    args = parse_args(argv)
    require_gpu()
    args.image_size = 0
    splits = dict(zip(("train", "val", "test"), train_synthetic._datasets(args, mode="student")))
    if args.split == "all":
        dataset = torch.utils.data.ConcatDataset([splits[s] for s in ("train", "val", "test")])
    else:
        dataset = splits[args.split]
    ts_vars = [f"var_{i}" for i in range(args.n_vars)]
    per_variable, per_sample = audit_dataset(dataset, ts_vars, args.n_timesteps, args.max_samples)
    print_summary(per_variable, per_sample, args.split)
    save_csv(per_variable, args.out_csv)
    sample_path = os.path.splitext(args.out_csv)[0] + "_per_sample.csv"
    save_csv(per_sample, sample_path)
    print(f"\nSaved: {args.out_csv}")
    print(f"Saved: {sample_path}")
    return {"per_variable": per_variable, "per_sample": per_sample, "csv": args.out_csv, "per_sample_csv": sample_path}


if __name__ == "__main__":
    main()
