#!/usr/bin/env python3
"""Time the trajectory-availability audit (`multimodal_edema_prediction_amd.trajectory_availability`) on the synthetic cohort's windows
(observed with probability 0.2, counts 1-3, drawn on the device from a seed) at the driver's default size N = 4 096, T = 96, V = 48 and
at N = 65 536, T = 24, V = 48:

  cells    `trajectory_cells`, one launch over the whole [N, T, 2V] tensor, by device events; with it the bytes of x per second the
           launch reaches (N T 2V 4 bytes over its time) next to the 8.0 TB/s HBM peak and the 6.3 TB/s a plain copy achieves;
  medians  the audit's four `column_medians` launches (int32 hours; total | recency | std; |endpoint change|; the per-sample counts),
           together, by device events;
  audit    `audit_dataset` on the device tensor end to end (five launches, the one synchronisation, the host tables), wall clock;
  host     the per-sample loop of tests/trajectory_availability_refs.py (`audit_ref`) on the same windows on the host, wall clock,
           once (at the large size on the first 4 096 samples, scaled by N / 4 096 and labelled so).

Each device figure is the median of REPEATS windows of INNER calls after a warm-up, printed with the smallest and largest window.  No
ratio is promised; the tool prints both sides.  Before timing, the audit's exact columns are compared with the restatement's.

Usage:  python tools/time_trajectory_availability.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from multimodal_edema_prediction_amd import trajectory_availability as ta
from multimodal_edema_prediction_amd.probe_stats import column_medians
from trajectory_availability_refs import STD_COLUMN, audit_ref

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER, HOST_ROWS = 20, 4096
SIZES = ((4096, 96, 48), (65536, 24, 48))
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12
ta.require_gpu()
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


def windows(N, T, V, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    obs = torch.rand((N, T, V), generator=g, device=dev) < 0.2
    values = torch.randn((N, T, V), generator=g, device=dev) * obs
    counts = obs.float() * torch.randint(1, 4, (N, T, V), generator=g, device=dev).float()
    return torch.cat((values, counts), dim=2).contiguous()


def medians(planes, n):
    V = planes.V
    column_medians(planes.obs_hours)
    column_medians(planes.f32[:3].reshape(3 * V, n))
    column_medians(planes.endpoint_change, take_abs=True)
    column_medians(planes.per_sample.t()[:3].contiguous())


print(f"device {torch.cuda.get_device_name(0)}; {REPEATS} windows of {INNER} calls; median [min .. max]")
for N, T, V in SIZES:
    x = windows(N, T, V, N)
    names = [f"var_{i}" for i in range(V)]
    rows = min(N, HOST_ROWS)
    xh = x[:rows].cpu().numpy()
    t0 = time.perf_counter()
    want = audit_ref(xh, names, T)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = ta.audit_dataset(x[:rows], names, T)
    for table, ref in zip(got, want):
        for k in ref:
            if k != STD_COLUMN:
                assert np.array_equal(table[k], ref[k], equal_nan=np.asarray(ref[k]).dtype.kind == "f"), f"the two paths disagree on {k}"
    planes = ta.trajectory_cells(x, T)
    cells = events(lambda: ta.trajectory_cells(x, T, planes, 0))
    rate = x.numel() * 4 / (np.median(cells) * 1e-3)
    print(f"N = {N:6d} T = {T:3d} V = {V}  cells   {show(cells)}   x: {x.numel() * 4 / 1e6:.1f} MB, {rate / 1e12:.3f} TB/s "
          f"({100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:.1f} % of a 6.3 TB/s copy)")
    print(f"{'':28s}medians {show(events(lambda: medians(planes, N)))}   (four launches, {5 * V + 3} columns of {N})")
    print(f"{'':28s}audit   {show(wall(lambda: ta.audit_dataset(x, names, T), INNER))}")
    scaled = "" if rows == N else f"   ({rows} samples timed: {host_ms:.0f} ms, scaled by {N // rows})"
    print(f"{'':28s}host    {host_ms * N / rows:9.1f} ms, one run{scaled}")
