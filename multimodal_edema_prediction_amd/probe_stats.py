"""What the analysis probes share (raw_trajectory_probe.py, conditional_information_probe.py, head_probe.py, unimodal_linear_probe.py):
the wrapper of the metrics kernel (csrc/binary_metrics.hip), the index draws that depend on no model (`default_rng(seed)` in the
reference's call order, so the replicates ARE the reference's), the paired bootstrap and the permutation summary over replicates, the
inference rule and the row keys of both conditional probes.  Without a GPU whatever reaches the metrics kernel raises (no CPU fallback)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .abi import check, lib, ptr, stream

F64 = torch.float64
METRICS_MAX_LEN = 16384        # MEDP_LDS_SORT_MAX_LEN (= MEDP_RESAMPLED_METRICS_MAX_LEN): the longest replicate one workgroup sorts in LDS


def to_host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def to_device(a, dtype, device) -> torch.Tensor:
    """A host vector, copied (read-only inputs stay untouched) and converted, on the device."""
    return torch.as_tensor(np.array(to_host(a), dtype=dtype), device=device)


def expit(s: np.ndarray) -> np.ndarray:
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ci95(values: np.ndarray):
    if values.size:
        low, high = np.percentile(values, [2.5, 97.5])
        return float(low), float(high)
    return float("nan"), float("nan")


def pearson(a: np.ndarray, b: np.ndarray) -> float:
    """The reference's `_pearson` (evaluator.py:186-194 and both analysis probes): NaN for fewer than two points or a constant side."""
    a, b = np.asarray(a), np.asarray(b)
    if a.size < 2 or a.std() == 0 or b.std() == 0:
        return float("nan")
    return float(np.corrcoef(a, b)[0, 1])


def unit_or_sd(var, mean, n: int):
    """`StandardScaler`'s scale of a column with population variance `var` over n rows: 1 where sklearn's test calls it constant."""
    eps = torch.finfo(F64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    return torch.where(constant, torch.ones_like(var), var.sqrt()) if isinstance(var, torch.Tensor) else (1.0 if constant else np.sqrt(var))


# ------------------------------------------------------------------------------------------------------------------------------
# the metrics kernel
# ------------------------------------------------------------------------------------------------------------------------------
def resampled_binary_metrics(y, p, idx=None, offsets=None, max_len=None) -> torch.Tensor:
    """y [N] u8, p [Rp,N] fp64, idx int32 / offsets int64 [R+1] (device) -> [R,3] fp64 = BCE, AUROC, AUPRC per replicate.
    idx None: R = Rp identity replicates.  `max_len`: the longest replicate (known to the caller, who drew the indices)."""
    Rp, N = p.shape
    if idx is None:
        R, max_len = Rp, N
    else:
        R = offsets.numel() - 1
        if max_len is None:
            max_len = int((offsets[1:] - offsets[:-1]).max())
    if y.dtype != torch.uint8 or p.dtype != F64 or (idx is not None and (idx.dtype != torch.int32 or offsets.dtype != torch.int64)):
        raise TypeError("resampled_binary_metrics: y u8, p fp64, idx int32, offsets int64")
    y, p = y.contiguous(), p.contiguous()
    out = torch.empty((R, 3), dtype=F64, device=p.device)
    check(lib().medp_resampled_binary_metrics(ptr(y), ptr(p), ptr(idx), ptr(offsets), ptr(out), N, Rp, R, int(max_len), stream()),
          "resampled_binary_metrics")
    return out


def placement(args, device=None):
    """-> (device, put): the device of the first of `args` that is on a GPU already, else `device`, else cuda; `put(a, host_t, dev_t)`
    leaves a device tensor where it is (as dev_t) and copies anything else there through a host array of host_t."""
    held = [a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda]
    device = held[0] if held else torch.device("cuda") if device is None else device
    return device, lambda a, host_t, dev_t: a.to(dev_t) if isinstance(a, torch.Tensor) and a.is_cuda else to_device(a, host_t, device)


def binary_metrics(y, probability, device=None) -> Dict[str, float]:
    """The reference's `_safe_metrics` through the metrics kernel (one identity replicate).  `y`, `probability`: host arrays or device
    tensors; what is on the device already stays there, `device` places the rest."""
    _, put = placement((probability, y), device)
    m = resampled_binary_metrics(put(y, np.uint8, torch.uint8), put(probability, np.float64, F64)[None]).cpu().numpy()[0]
    return {"bce": float(m[0]), "auroc": float(m[1]), "auprc": float(m[2])}


def paired_replicate_metrics(y, p_a, p_b, idx, offsets, max_len: int, device=None):
    """Two probability vectors (host or device) scored on the same replicates idx[offsets[r] : offsets[r + 1]] (int32 / int64 [R+1], host
    or device) -> two host [R, 3] arrays of BCE, AUROC, AUPRC: both launches of the metrics kernel, then the two copies."""
    device, put = placement((p_a, p_b), device)
    yd, idx_d, off_d = put(y, np.uint8, torch.uint8), torch.as_tensor(idx, device=device), torch.as_tensor(offsets, device=device)
    m = [resampled_binary_metrics(yd, put(p, np.float64, F64).reshape(1, -1), idx_d, off_d, max_len) for p in (p_a, p_b)]
    return m[0].cpu().numpy(), m[1].cpu().numpy()


class LabelMetrics:
    """AUROC / AUPRC / BCE of every label over its known rows, in ONE `medp_resampled_binary_metrics` launch: y and p are flattened
    to [L n] (label-major) and replicate l is the index list of label l's known rows, offset by l n."""

    def __init__(self, Y: torch.Tensor, M: torch.Tensor):
        dev = Y.device
        self.n, self.L = Y.shape
        known = M.detach().to("cpu").numpy().astype(bool)                              # once, before the first launch
        self.counts = known.sum(0)
        if self.counts.max(initial=0) > METRICS_MAX_LEN:
            raise ValueError(f"a label has {int(self.counts.max())} known rows: more than the metrics kernel's "
                             f"MEDP_RESAMPLED_METRICS_MAX_LEN = {METRICS_MAX_LEN}")
        idx = [np.flatnonzero(known[:, l]).astype(np.int32) + l * self.n for l in range(self.L)]
        self.idx = torch.as_tensor(np.concatenate(idx) if idx else np.zeros(0, np.int32), device=dev)
        self.offsets = torch.as_tensor(np.concatenate(([0], np.cumsum(self.counts))).astype(np.int64), device=dev)
        self.y = (Y.detach().t() > 0.5).to(torch.uint8).contiguous().reshape(-1)
        self.max_len = max(int(self.counts.max(initial=0)), 1)
        if self.idx.numel() == 0:                                                      # nothing known at all: a valid (empty) index list
            self.idx = torch.zeros(1, dtype=torch.int32, device=dev)

    def __call__(self, probs: torch.Tensor) -> torch.Tensor:
        """probs [L, n] fp64 -> [L, 3] fp64 = BCE, AUROC, AUPRC per label (NaN: fewer than two known rows, or one class)."""
        return resampled_binary_metrics(self.y, probs.reshape(1, -1), self.idx, self.offsets, self.max_len)


def column_medians(planes: torch.Tensor, take_abs: bool = False):
    """planes [C, N] fp32 or int32 on the device (rows may be strided: a view `buf[:, :N]` of wider planes is read in place) ->
    (median [C] fp64, n_valid [C] int32), device tensors, no synchronisation.  numpy's median of every row after `take_abs`, NaNs
    dropped (`np.nanmedian`; a row without a valid entry: NaN): exact selection by radix (csrc/trajectory_audit.hip), any N up to
    MEDP_COLUMN_MEDIAN_MAX_N, none of the 16384-row limit of the kernels that sort in LDS."""
    if not isinstance(planes, torch.Tensor) or planes.dtype not in (torch.float32, torch.int32):
        raise TypeError("column_medians reads fp32 or int32 planes")
    if planes.ndim != 2 or planes.shape[0] < 1 or planes.shape[1] < 1:
        raise ValueError("column_medians: planes [C >= 1, N >= 1]")
    C, N = planes.shape
    if planes.stride(1) != 1 or (C > 1 and planes.stride(0) < N):
        planes = planes.contiguous()
    ld = planes.stride(0) if C > 1 else max(planes.stride(0), N)
    median = torch.empty(C, dtype=F64, device=planes.device)
    n_valid = torch.empty(C, dtype=torch.int32, device=planes.device)
    check(lib().medp_column_medians(ptr(planes), ld, C, N, int(planes.dtype == torch.int32), int(bool(take_abs)), ptr(median), ptr(n_valid),
                                    stream()), "column_medians")
    return median, n_valid


def nan_mean(v: torch.Tensor) -> torch.Tensor:
    """Mean of the entries that are not NaN; NaN when there is none (a device scalar, no synchronisation)."""
    ok = ~torch.isnan(v)
    return torch.where(ok, v, torch.zeros_like(v)).sum() / ok.sum()


# ------------------------------------------------------------------------------------------------------------------------------
# index draws
# ------------------------------------------------------------------------------------------------------------------------------
def image_risk_bins(image_logit: np.ndarray, n_bins: int) -> np.ndarray:
    """`_image_risk_bins` (raw-trajectory probe :130-138; the conditional-information probe's is the same)."""
    if n_bins <= 1:
        return np.zeros(len(image_logit), dtype=np.int64)
    edges = np.unique(np.quantile(image_logit, np.linspace(0.0, 1.0, int(n_bins) + 1)))
    if len(edges) <= 2:
        return np.zeros(len(image_logit), dtype=np.int64)
    return np.digitize(image_logit, edges[1:-1], right=True).astype(np.int64)


def conditional_shuffle_indices(bins: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """`_conditional_shuffle_indices` (:141-149): the same draws from `rng`."""
    shuffled = np.arange(len(bins))
    for value in np.unique(bins):
        members = np.flatnonzero(bins == value)
        if len(members) > 1:
            shuffled[members] = rng.permutation(members)
    return shuffled


def draw_conditional_shuffles(image_logit: np.ndarray, n_bins: int, repeats: int, seed: int) -> list:
    """The `repeats` within-image-risk shuffles of both conditional permutations: the bins, ONE `default_rng(seed)`, then the draws."""
    bins = image_risk_bins(image_logit, n_bins)
    rng = np.random.default_rng(seed)
    return [conditional_shuffle_indices(bins, rng) for _ in range(max(int(repeats), 0))]


def draw_bootstrap_indices(n: int, n_bootstrap: int, seed: int) -> np.ndarray:
    """The draws of the conditional-information probe's `_bootstrap_differences` (:234-238) -> [n_bootstrap, n] int32."""
    rng = np.random.default_rng(seed)
    draws = [rng.integers(0, n, size=n) for _ in range(max(int(n_bootstrap), 0))]
    return np.stack(draws).astype(np.int32) if draws else np.zeros((0, n), np.int32)


def draw_cluster_bootstrap_indices(subject_ids: np.ndarray, n_bootstrap: int, seed: int):
    """The patient-cluster draws of `_cluster_bootstrap_differences` (:771-777) -> (idx int32 concatenated, offsets int64 [R+1])."""
    unique_subjects = np.unique(subject_ids)
    members = {subject: np.flatnonzero(subject_ids == subject) for subject in unique_subjects}
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(max(int(n_bootstrap), 0)):
        drawn = rng.choice(unique_subjects, size=len(unique_subjects), replace=True)
        parts.append(np.concatenate([members[subject] for subject in drawn]))
    offsets = np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
    idx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return idx, offsets


# ------------------------------------------------------------------------------------------------------------------------------
# replicates -> intervals -> the inference rule
# ------------------------------------------------------------------------------------------------------------------------------
def paired_bootstrap_gains(y, base_probability, probe_probability, idx, offsets, max_len: int, device) -> Dict[str, float]:
    """95 % intervals of the (BCE, AUROC, AUPRC) gains of the probe over the base on the replicates idx[offsets[r] : offsets[r + 1]] (int32 /
    int64 [R+1], host or device), two metrics launches; one-class replicates leave the AUROC / AUPRC lists only; no replicate: six NaN."""
    samples = {"bce_gain": np.zeros(0), "auroc_gain": np.zeros(0), "auprc_gain": np.zeros(0)}
    if len(offsets) > 1:
        base, probe = paired_replicate_metrics(y, base_probability, probe_probability, idx, offsets, max_len, device)
        both = ~np.isnan(base[:, 1])                                     # replicates with both classes present
        samples = {"bce_gain": base[:, 0] - probe[:, 0], "auroc_gain": (probe[:, 1] - base[:, 1])[both],
                   "auprc_gain": (probe[:, 2] - base[:, 2])[both]}
    return {f"{metric}_ci_{side}": v for metric, values in samples.items() for side, v in zip(("low", "high"), ci95(values))}


def permutation_summary(y, probabilities: torch.Tensor | None) -> Dict[str, float]:
    """The nine `perm_*` values: mean and 95 % interval of BCE / AUROC / AUPRC over the rows of `probabilities` [R, n] (device; None: R = 0)."""
    samples = np.zeros((0, 3))
    if probabilities is not None and len(probabilities):
        samples = resampled_binary_metrics(to_device(y, np.uint8, probabilities.device), probabilities).cpu().numpy()
    output: Dict[str, float] = {}
    for k, metric in enumerate(("bce", "auroc", "auprc")):
        finite = samples[:, k][np.isfinite(samples[:, k])]
        output[f"perm_{metric}_mean"] = float(finite.mean()) if finite.size else float("nan")
        output[f"perm_{metric}_low"], output[f"perm_{metric}_high"] = ci95(finite)
    return output


def inference_fields(base_metrics, metrics, confidence, corr_residual: float, permutation):
    """(fields, evidence): the part of a row both conditional probes share, `image_cal_bce` ... `perm_auroc_drop` in the reference's order,
    and its verdict: `supported` = a positive BCE gain, its interval above zero AND a worse BCE under the permutation."""
    gains = {"bce_gain": base_metrics["bce"] - metrics["bce"], "auroc_gain": metrics["auroc"] - base_metrics["auroc"],
             "auprc_gain": metrics["auprc"] - base_metrics["auprc"]}
    perm_bce_increase, perm_auroc_drop = permutation["perm_bce_mean"] - metrics["bce"], metrics["auroc"] - permutation["perm_auroc_mean"]
    supported = gains["bce_gain"] > 0 and confidence["bce_gain_ci_low"] > 0 and perm_bce_increase > 0
    evidence = "supported" if supported else "suggestive" if gains["bce_gain"] > 0 else "not_detected"
    fields = {"image_cal_bce": base_metrics["bce"], "image_cal_auroc": base_metrics["auroc"], "image_cal_auprc": base_metrics["auprc"],
              "probe_bce": metrics["bce"], "probe_auroc": metrics["auroc"], "probe_auprc": metrics["auprc"],
              **gains, **confidence, "corr_residual": corr_residual, **permutation,
              "perm_bce_increase": perm_bce_increase, "perm_auroc_drop": perm_auroc_drop}
    return fields, evidence
