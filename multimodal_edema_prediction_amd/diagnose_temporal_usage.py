"""Temporal-usage diagnostics of a trained dual teacher: the device-side counterpart of the reference's
`analysis/diagnose_temporal_usage.py`.  Does the teacher use the time series at all, and does it use their ORDER?  Every batch is re-run
on five arrangements of its EHR input (`CONDITIONS`: full, another patient's whole EHR package, another patient's measurements only,
time reversed, time permuted within the sample); reported are AUROC / AUPRC per condition, the sensitivity of the probabilities, the
entropy of the temporal attention and a subject-cluster paired bootstrap of full - ablated.  `--output_npz` writes the file that
`residual_by_confidence.py` reads.

    python -m multimodal_edema_prediction_amd.diagnose_temporal_usage --teacher_ckpt runs/t0/best.pt --split val --bootstrap 2000

The contract is THE SCRIPT'S ARITHMETIC AND DRAWS, ON THE MODEL AS THE REFERENCE'S MODEL FILE DEFINES IT and as this package mirrors
it.  At the reference's HEAD the script itself does not import (it names `DualPathologyPerceiver`, which is commented out there, expects
`encode` to return a pair and the patch perceiver to return `event_attn`; the model file of the same checkout does neither).  So: both
perceiver types take `ts_tokens` with `ts_ablation="hourly_only"`, and the attention of the full condition is `ts_attn` in both modes.
Its pure functions do run and are restated here name for name: `different_subject_permutation`, `time_permutations` (the draws of
`_time_permuted`), `metrics_by_label`, `cluster_bootstrap_delta`, `print_results`; tests/golden/temporal_usage.npz holds what the
reference's own functions return on one seeded problem.

Where the work runs
  counterfactual_inputs   ONE launch of `medp_counterfactual_feats` assembles all five arrangements (the reference: five host loops).
  collect_predictions     the image encoder runs ONCE per batch; the DuETT encoder and the time-series half of the perceiver run per
                          condition on views of the stacked buffer; everything gathered stays on the device in fp32.  The logits are
                          bit-equal to five calls of the public `teacher(...)` on host-transformed tuples.  (For `dual_patch` the image
                          half of the PERCEIVER runs twice: `return_attn` selects another attention kernel, and the public forward of the
                          full condition has it on.)
  summarise               `medp_temporal_usage_summary` (fp32 sigmoid widened, sensitivity, entropy), `LabelMetrics` for the rank
                          metrics and two launches of the metrics kernel per bootstrap.

One documented divergence: the metrics kernel clips probabilities to [1e-7, 1 - 1e-7], which ties logits beyond about +-16; the
reference's fp32 sigmoid ties them beyond about +-17.  Rank metrics of a teacher whose logits leave +-16 can differ by those ties.
Without a GPU everything that reaches a kernel raises (no CPU fallback)."""
from __future__ import annotations

import argparse
import os
from typing import Dict, Sequence

import numpy as np
import torch

from .abi import check, lib, ptr, require_gpu, stream
from .probe_stats import F64, METRICS_MAX_LEN, LabelMetrics, draw_cluster_bootstrap_indices, paired_replicate_metrics, placement, to_host

CONDITIONS = ("full", "patient_shuffle", "ts_shuffle", "time_reverse", "time_permute")
BATCH_SEED_STRIDE = 10007           # the batch's generator: default_rng(seed + 10007 * batch_idx)
SUMMARY_MAX_N, SUMMARY_MAX_S = 1 << 22, 4096          # MEDP_TEMPORAL_USAGE_MAX_N / _MAX_S
_METRIC_COLUMN = {"AUROC": 1, "AUPRC": 2}


# ------------------------------------------------------------------------------------------------------------------------------
# the draws (host numpy, the reference's call order)
# ------------------------------------------------------------------------------------------------------------------------------
def different_subject_permutation(subject_ids: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """`_different_subject_permutation`: up to 100 tries for a permutation that pairs no sample with its own subject, then the cyclic
    shift with the fewest same-subject pairs (repeated stays can make a derangement impossible)."""
    subject_ids = np.asarray(subject_ids)
    n = len(subject_ids)
    if n <= 1:
        return np.arange(n)
    for _ in range(100):
        perm = rng.permutation(n)
        if np.all(subject_ids[perm] != subject_ids):
            return perm
    best_perm = np.roll(np.arange(n), 1)
    best_matches = int(np.sum(subject_ids[best_perm] == subject_ids))
    for shift in range(2, n):
        candidate = np.roll(np.arange(n), shift)
        matches = int(np.sum(subject_ids[candidate] == subject_ids))
        if matches < best_matches:
            best_perm, best_matches = candidate, matches
            if matches == 0:
                break
    return best_perm


def time_permutations(lengths: Sequence[int], rng: np.random.Generator) -> list:
    """The draws of `_time_permuted`: one `rng.permutation(T_b)` per sample, in batch order."""
    return [rng.permutation(int(n)) for n in lengths]


# ------------------------------------------------------------------------------------------------------------------------------
# kernel 1: the five arrangements of one batch
# ------------------------------------------------------------------------------------------------------------------------------
def counterfactual_inputs(duett, x_ts, x_static, bin_ends, sample_perm, time_perms, conditions: Sequence[str] = CONDITIONS):
    """-> (xs_static [5, B, Ds], xs_ts [5, B, Tpad, 2V+1], xs_times [5, B, Tpad], n_timesteps: one list per condition), condition-major
    in the order of `CONDITIONS`: what `feats_to_input` returns for the reference's host-transformed tuples (flip / index_select /
    tuple permutation of the RAW series, THEN the truncation to the last max_len steps), in one launch.  Inputs as `feats_to_input`
    takes them (host tensors, separate device tensors or rows of one stacked buffer); they are never modified.  `sample_perm` [B] and
    `time_perms` (one permutation of [0, T_b) per sample) are host integers.  An entry outside its range is never dereferenced: the
    output rows that depend on it are NaN.  `ts_shuffle` has no meaning where lengths[perm[b]] != lengths[b] (the reference's padding
    goes negative): ValueError before anything is launched, unless `conditions` leaves it out — its block is then written but
    meaningless and its `n_timesteps` is None."""
    unknown = [c for c in conditions if c not in CONDITIONS]
    if unknown:
        raise ValueError(f"counterfactual_inputs: unknown conditions {unknown}; expected a subset of {CONDITIONS}")
    lens = [int(f.shape[0]) for f in x_ts]
    B = len(lens)
    perm = np.asarray(sample_perm, dtype=np.int64).reshape(-1)
    if len(perm) != B or len(time_perms) != B:
        raise ValueError(f"counterfactual_inputs: {B} samples, {len(perm)} sample_perm entries, {len(time_perms)} time permutations")
    if any(len(tp) != n for tp, n in zip(time_perms, lens)):
        raise ValueError("counterfactual_inputs: time_perms[b] must have one entry per step of sample b")
    inside = (perm >= 0) & (perm < B)
    paired = np.where(inside, np.asarray(lens, dtype=np.int64)[np.where(inside, perm, 0)], -1)
    if "ts_shuffle" in conditions and np.any(inside & (paired != np.asarray(lens))):
        b = int(np.flatnonzero(inside & (paired != np.asarray(lens)))[0])
        raise ValueError(f"counterfactual_inputs: condition 'ts_shuffle' pairs sample {b} (length {lens[b]}) with sample {int(perm[b])} "
                         f"(length {int(paired[b])}); the measurements of another patient fit the sample's own bin times only at equal length")
    where, lens, keep, (B, V, Ds) = duett._locate_batch((x_ts, x_static, bin_ends), "counterfactual_inputs")
    dev = duett.device
    max_len = int(duett.max_len)
    n_own = [min(n, max_len) for n in lens]
    Tpad, Tmax = max(n_own), max(lens)
    table = np.zeros((B, Tmax), dtype=np.int32)
    for b, tp in enumerate(time_perms):
        table[b, :lens[b]] = np.asarray(tp, dtype=np.int64).astype(np.int32)
    tables = torch.as_tensor(np.concatenate((perm.astype(np.int32), table.reshape(-1))), device=dev)           # one upload
    out_ts = torch.empty((len(CONDITIONS), B, Tpad, 2 * V + 1), dtype=torch.float32, device=dev)
    out_tm = torch.empty((len(CONDITIONS), B, Tpad), dtype=torch.float32, device=dev)
    out_st = torch.empty((len(CONDITIONS), B, Ds), dtype=torch.float32, device=dev)
    check(lib().medp_counterfactual_feats(*where, ptr(tables), tables.data_ptr() + 4 * B, ptr(out_ts), ptr(out_tm), ptr(out_st), B, V, Ds,
                                          max_len, Tpad, Tmax, stream()), "counterfactual_feats")
    del keep
    n_shuffled = [n_own[int(j)] if ok else 0 for j, ok in zip(perm, inside)]
    n_timesteps = [n_own, n_shuffled, n_own if "ts_shuffle" in conditions else None, n_own, n_own]
    return out_st, out_ts, out_tm, n_timesteps


# ------------------------------------------------------------------------------------------------------------------------------
# the gather
# ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def collect_predictions(teacher, loader, device, perceiver_type: str, seed: int) -> dict:
    """The reference's `collect_predictions`: per batch one assembly launch, the image side once, the DuETT encoder and the time-series
    side per condition, `return_attn` for the full condition only.  -> {"fus", "ts": {condition: [N, K]}, "img", "y", "mask" [N, K],
    "attention" [N, K, S] (device, fp32), "subject_ids" [N] (host), "shuffle_same_subject", "shuffle_total"}.  Batches carry
    `_subject_id` (`SubjectAnnotatedDataset` / `diagnostic_collate`)."""
    from . import autograd_ops as A
    from .engine import _move_lists
    from .main_architecture_duett import _BroadcastRowsFn
    require_gpu()
    if perceiver_type not in ("dual", "dual_patch"):
        raise NotImplementedError(f"perceiver_type={perceiver_type!r}: only dual / dual_patch teachers are diagnosed")
    teacher.eval()
    fus = {c: [] for c in CONDITIONS}
    ts = {c: [] for c in CONDITIONS}
    img_full, y_all, mask_all, attn_all, subject_all = [], [], [], [], []
    same_subject = total = 0
    pc = teacher.perceiver
    for batch_idx, batch in enumerate(loader):
        subject_ids = to_host(batch["_subject_id"]).astype(np.int64)
        subject_all.append(subject_ids.copy())
        b = _move_lists(batch, device)
        B = len(b["x_ts"])
        rng = np.random.default_rng(seed + BATCH_SEED_STRIDE * batch_idx)
        cross_perm = different_subject_permutation(subject_ids, rng)
        same_subject += int(np.sum(subject_ids[cross_perm] == subject_ids))
        total += B
        time_perms = time_permutations([int(x.shape[0]) for x in b["x_ts"]], rng)
        xs_static, xs_ts, xs_times, n_timesteps = counterfactual_inputs(teacher.duett, b["x_ts"], b["x_static"], b["bin_ends"], cross_perm,
                                                                        time_perms)
        # ---- the image side, once per batch
        if perceiver_type == "dual":
            img_logits = teacher._kept_head_logits(b["pixel_values"])
        else:
            q0 = _BroadcastRowsFn.apply(pc.shared_queries, B)
            tokens16 = teacher.cxr.forward_bf16(b["pixel_values"])
            img_proj_full = A.linear(tokens16, teacher.img_proj.weight, teacher.img_proj.bias)
            image = {True: pc._img_branch(img_proj_full, q0, 0, True, 1), False: pc._img_branch(img_proj_full, q0, 0, False, 1)}
        # ---- the time-series side, per condition on views of the stacked buffer
        for c, cond in enumerate(CONDITIONS):
            need_attn = cond == "full"
            tokens = teacher.duett.encode((xs_static[c], xs_ts[c], xs_times[c], n_timesteps[c]))
            if perceiver_type == "dual":
                out = pc(tokens, img_logits, return_attn=need_attn, ts_ablation="hourly_only")
            else:
                out = pc._fuse(image[need_attn], pc._ts_branch(pc._select_ts(tokens, "hourly_only"), q0, 0, need_attn), need_attn)
            fus[cond].append(out["fusion_logits"].detach().float())
            ts[cond].append(out["ts_logits"].detach().float())
            if need_attn:
                img_full.append(out["img_logits"].detach().float())
                attn_all.append(out["ts_attn"].detach().float())
        y_all.append(b["y_multi"].float())
        mask_all.append(b["y_multi_mask"].float())
    if not y_all:
        raise RuntimeError("temporal diagnostics: the loader yielded no batches")
    cat = lambda parts: torch.cat(parts).contiguous()  # noqa: E731
    return {"fus": {c: cat(v) for c, v in fus.items()}, "ts": {c: cat(v) for c, v in ts.items()}, "img": cat(img_full), "y": cat(y_all),
            "mask": cat(mask_all), "subject_ids": np.concatenate(subject_all), "attention": cat(attn_all),
            "shuffle_same_subject": same_subject, "shuffle_total": total}


# ------------------------------------------------------------------------------------------------------------------------------
# kernel 2 and the report
# ------------------------------------------------------------------------------------------------------------------------------
def temporal_usage_summary(fus: torch.Tensor, ts: torch.Tensor, attention: torch.Tensor | None = None, entropy: torch.Tensor | None = None):
    """fus, ts [C, N, K] fp32 logits (condition 0 = full), attention [N, K, S] fp32 or None -> (prob [2, C, K, N] fp64: the fp32 sigmoid
    of fus then ts, widened, label-major as `LabelMetrics` reads it; sens [C-1, K, 3] fp64 = mean |dp fus|, corr fus, mean |dp ts|;
    entropy [K] fp64 or None).  `entropy`: a buffer to write into (left untouched without attention)."""
    if fus.dtype != torch.float32 or ts.dtype != torch.float32 or fus.shape != ts.shape or fus.dim() != 3:
        raise TypeError("temporal_usage_summary: fus and ts are fp32 [C, N, K]")
    fus, ts = fus.contiguous(), ts.contiguous()
    C, N, K = fus.shape
    S = 0
    if attention is not None:
        if attention.dtype != torch.float32 or attention.dim() != 3 or tuple(attention.shape[:2]) != (N, K):
            raise TypeError("temporal_usage_summary: attention is fp32 [N, K, S]")
        attention = attention.contiguous()
        S = int(attention.shape[2])
        if entropy is None:
            entropy = torch.empty(K, dtype=F64, device=fus.device)
    prob = torch.empty((2, C, K, N), dtype=F64, device=fus.device)
    sens = torch.empty((max(C - 1, 0), K, 3), dtype=F64, device=fus.device)
    check(lib().medp_temporal_usage_summary(ptr(fus), ptr(ts), ptr(attention), ptr(prob), ptr(sens) if C > 1 else None, ptr(entropy) if entropy is not None else None,
                                            C, N, K, S, stream()), "temporal_usage_summary")
    return prob, sens, entropy


def metrics_by_label(prob: torch.Tensor, y, mask, labels: Sequence[str], label_metrics: LabelMetrics | None = None) -> list:
    """`_metrics_by_label` on probabilities: prob [K, N] fp64 (device, label-major), y / mask [N, K] -> one row per label:
    label, n, pos_frac, auroc, auprc (NaN: fewer than two known rows or one class), all labels in ONE launch of the metrics kernel."""
    y_host, known = to_host(y).astype(np.float32), to_host(mask).astype(bool)
    if label_metrics is None:
        label_metrics = LabelMetrics(torch.as_tensor(y_host, device=prob.device), torch.as_tensor(known, device=prob.device))
    m = label_metrics(prob.contiguous()).cpu().numpy()
    rows = []
    for k, label in enumerate(labels):
        yk = y_host[known[:, k], k]
        rows.append({"label": label, "n": int(known[:, k].sum()), "pos_frac": float(yk.mean()) if len(yk) else float("nan"),
                     "auroc": float(m[k, 1]), "auprc": float(m[k, 2])})
    return rows


def cluster_bootstrap_delta(subject_ids, y, valid, p_full, p_ablated, metric: str, n_boot: int, seed: int, device=None):
    """`_cluster_bootstrap_delta`: subject-cluster bootstrap of metric(full) - metric(ablated) -> (mean, q2.5, q97.5, n_valid).  The
    draws are `draw_cluster_bootstrap_indices`' (the reference's); rows with `valid == False` leave every replicate on the host; two
    launches of the metrics kernel; a replicate counts iff both values are finite (an empty or one-class replicate is NaN there)."""
    if metric not in _METRIC_COLUMN:
        raise ValueError(f"cluster_bootstrap_delta: metric {metric!r}; expected one of {tuple(_METRIC_COLUMN)}")
    nothing = (float("nan"), float("nan"), float("nan"), 0)
    subject_ids, valid = np.asarray(to_host(subject_ids)), to_host(valid).astype(bool)
    idx, offsets = draw_cluster_bootstrap_indices(subject_ids, n_boot, seed)
    if len(offsets) < 2:
        return nothing
    keep = valid[idx]
    offsets = np.concatenate(([0], np.cumsum(keep)))[offsets].astype(np.int64)
    idx = idx[keep]
    longest = int(np.diff(offsets).max())
    if longest > METRICS_MAX_LEN:
        raise ValueError(f"cluster_bootstrap_delta: a replicate has {longest} rows: more than the metrics kernel's "
                         f"MEDP_RESAMPLED_METRICS_MAX_LEN = METRICS_MAX_LEN = {METRICS_MAX_LEN}")
    if idx.size == 0:
        return nothing
    full, ablated = (m[:, _METRIC_COLUMN[metric]]
                     for m in paired_replicate_metrics(to_host(y) > 0.5, p_full, p_ablated, idx, offsets, max(longest, 1), device))
    both = np.isfinite(full) & np.isfinite(ablated)
    if not both.any():
        return nothing
    deltas = (full - ablated)[both]
    return float(deltas.mean()), float(np.quantile(deltas, 0.025)), float(np.quantile(deltas, 0.975)), int(deltas.size)


def summarise(pred: dict, labels: Sequence[str], n_boot: int, seed: int) -> dict:
    """The five sections of the reference's report as a plain dict: "baseline" [1], "conditions" [2], "sensitivity" [3] (label 0),
    "entropy" [4] (None without a [N, K, S > 0] attention), "audit", "bootstrap" [5] (empty when n_boot <= 0).  `pred`: what
    `collect_predictions` returns (device tensors or host arrays)."""
    require_gpu()
    _, put = placement((pred["y"], pred["img"]))
    f32 = lambda a: put(a, np.float32, torch.float32)  # noqa: E731
    fus = torch.stack([f32(pred["fus"][c]) for c in CONDITIONS])
    ts = torch.stack([f32(pred["ts"][c]) for c in CONDITIONS])
    img, y, mask = f32(pred["img"]), f32(pred["y"]), f32(pred["mask"])
    C, N, K = fus.shape
    attention = pred.get("attention")
    attention = None if attention is None else f32(attention)
    if attention is not None and not (attention.dim() == 3 and attention.numel() > 0):
        attention = None
    prob, sens, entropy = temporal_usage_summary(fus, ts, attention)
    prob_img = temporal_usage_summary(img[None], img[None])[0][0, 0]                        # [K, N]
    lm = LabelMetrics(y, mask)
    y_host, mask_host = to_host(y), to_host(mask)
    rows = lambda p: metrics_by_label(p, y_host, mask_host, labels, lm)  # noqa: E731
    img_m, ts_m = rows(prob_img), rows(prob[1, 0])
    fus_by_cond = {c: rows(prob[0, i]) for i, c in enumerate(CONDITIONS)}
    baseline = [{"label": ri["label"], "n": ri["n"], "pos_frac": ri["pos_frac"], "img_auroc": ri["auroc"], "ts_auroc": rt["auroc"],
                 "fus_auroc": rf["auroc"], "img_auprc": ri["auprc"], "ts_auprc": rt["auprc"], "fus_auprc": rf["auprc"]}
                for ri, rt, rf in zip(img_m, ts_m, fus_by_cond["full"])]
    conditions = [{"condition": c, "label": row["label"], "auroc": row["auroc"], "d_auroc": row["auroc"] - base["auroc"],
                   "auprc": row["auprc"], "d_auprc": row["auprc"] - base["auprc"]}
                  for c in CONDITIONS for row, base in zip(fus_by_cond[c], fus_by_cond["full"])]
    sens_host = sens.cpu().numpy()
    sensitivity = [{"condition": c, "mean_abs_dp_fus": float(sens_host[i, 0, 0]), "corr_fus": float(sens_host[i, 0, 1]),
                    "mean_abs_dp_ts": float(sens_host[i, 0, 2]), "max_abs_d_img": 0.0} for i, c in enumerate(CONDITIONS[1:])]
    entropy_section = None
    if entropy is not None:
        e = entropy.cpu().numpy()
        entropy_section = {"axis_size": int(attention.shape[-1]), "per_label": [{"label": label, "mean_entropy": float(e[k])}
                                                                                for k, label in enumerate(labels)]}
    bootstrap = []
    if n_boot > 0:
        valid, y0 = mask_host[:, 0].astype(bool), y_host[:, 0]
        for ci, condition in enumerate(CONDITIONS[1:], start=1):
            for offset, metric in enumerate(("AUROC", "AUPRC")):
                mean_d, lo, hi, n_valid = cluster_bootstrap_delta(pred["subject_ids"], y0, valid, prob[0, 0, 0], prob[0, ci, 0], metric,
                                                                  n_boot, seed + 1000 * ci + offset)
                bootstrap.append({"condition": condition, "metric": metric, "mean_delta": mean_d, "ci_low": lo, "ci_high": hi,
                                  "n_valid": n_valid})
    return {"labels": list(labels), "baseline": baseline, "conditions": conditions, "sensitivity": sensitivity, "entropy": entropy_section,
            "audit": {"same_subject": int(pred["shuffle_same_subject"]), "total": int(pred["shuffle_total"])}, "n_boot": int(n_boot),
            "bootstrap": bootstrap}


def print_results(summary: dict, attention_axis: str = "time tokens") -> None:
    """`_print_results`: the sections of `summarise` in the reference's layout."""
    print("\n[1] Original checkpoint under FULL input: img / ts / fus per-label")
    print(f"{'label':<24s} {'n':>6s} {'pos':>7s} {'img_roc':>8s} {'ts_roc':>8s} {'fus_roc':>8s}  {'img_prc':>8s} {'ts_prc':>8s} {'fus_prc':>8s}")
    for r in summary["baseline"]:
        print(f"{r['label']:<24s} {r['n']:>6d} {r['pos_frac']:>7.4f} {r['img_auroc']:>8.4f} {r['ts_auroc']:>8.4f} {r['fus_auroc']:>8.4f}  "
              f"{r['img_auprc']:>8.4f} {r['ts_auprc']:>8.4f} {r['fus_auprc']:>8.4f}")
    print("\n[2] Fusion logits under counterfactual TS inputs (delta = ablated - full; negative = 성능 하락)")
    print(f"{'condition':<18s} {'label':<24s} {'AUROC':>9s} {'d_ROC':>9s} {'AUPRC':>9s} {'d_PRC':>9s}")
    for r in summary["conditions"]:
        print(f"{r['condition']:<18s} {r['label']:<24s} {r['auroc']:>9.4f} {r['d_auroc']:>+9.4f} {r['auprc']:>9.4f} {r['d_auprc']:>+9.4f}")
    print("\n[3] Sensitivity to TS corruption (label=Edema, idx 0)")
    print(f"{'condition':<18s} {'mean|dp fus|':>14s} {'corr fus':>10s} {'mean|dp ts|':>13s} {'max|d img|':>12s}")
    for r in summary["sensitivity"]:
        print(f"{r['condition']:<18s} {r['mean_abs_dp_fus']:>14.6f} {r['corr_fus']:>10.6f} {r['mean_abs_dp_ts']:>13.6f} {r['max_abs_d_img']:>12.6g}")
    print("img logits는 TS 무관 → invariance는 항상 0 (perceiver 입력에서 image branch가 TS와 분리)")
    if summary["entropy"] is not None:
        print(f"\n[4] Full-condition TS attention ({attention_axis}, N={summary['entropy']['axis_size']}): normalized entropy per label")
        print(f"{'label':<24s} {'mean entropy':>14s}")
        for r in summary["entropy"]["per_label"]:
            print(f"{r['label']:<24s} {r['mean_entropy']:>14.6f}")
    same, total = summary["audit"]["same_subject"], summary["audit"]["total"]
    print(f"\nCross-patient shuffle audit: same-subject pairs={same}/{total} ({same / max(total, 1):.4%})")
    if summary["n_boot"] <= 0:
        return
    print(f"\n[5] Main label (idx 0) subject-cluster paired bootstrap ({summary['n_boot']} replicates)")
    print("Delta = full - ablated; positive → 원본 TS 사용이 유리")
    print(f"{'condition':<18s} {'metric':<7s} {'mean delta':>11s} {'95% CI':>24s} {'valid':>7s}")
    for r in summary["bootstrap"]:
        print(f"{r['condition']:<18s} {r['metric']:<7s} {r['mean_delta']:>+11.5f} [{r['ci_low']:>+9.5f}, {r['ci_high']:>+9.5f}] {r['n_valid']:>7d}")


# ------------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------------
class SubjectAnnotatedDataset(torch.utils.data.Dataset):
    """`_SubjectAnnotatedDataset` for the synthetic cohort, which has no patients: stay i of the cohort belongs to subject
    (dataset.offset + i) // stays_per_subject."""

    def __init__(self, base_dataset, stays_per_subject: int = 2):
        if stays_per_subject < 1:
            raise ValueError("stays_per_subject must be at least 1")
        self.base, self.stays_per_subject = base_dataset, int(stays_per_subject)

    def __len__(self):
        return len(self.base)

    def __getitem__(self, index):
        item = self.base[index]
        item["_subject_id"] = (int(getattr(self.base, "offset", 0)) + int(index)) // self.stays_per_subject
        return item


def diagnostic_collate(items: list) -> dict:
    from .cohort import collate
    out = collate(items, "teacher")
    out["_subject_id"] = torch.tensor([item["_subject_id"] for item in items], dtype=torch.long)
    return out


def npz_payload(pred: dict, labels: Sequence[str]) -> Dict[str, np.ndarray]:
    """The reference's archive, key for key: subject_ids, labels, y, mask, img_full, ts_attention_full, fus_<cond>, ts_<cond>."""
    payload = {"subject_ids": to_host(pred["subject_ids"]), "labels": np.asarray(labels), "y": to_host(pred["y"]), "mask": to_host(pred["mask"]),
               "img_full": to_host(pred["img"]), "ts_attention_full": to_host(pred["attention"])}
    for condition in CONDITIONS:
        payload[f"fus_{condition}"] = to_host(pred["fus"][condition])
        payload[f"ts_{condition}"] = to_host(pred["ts"][condition])
    return payload


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser("Dual/DualPatch teacher temporal-usage diagnostics")
    p.add_argument("--teacher_ckpt", required=True, help="teacher best.pt written by train_synthetic")
    p.add_argument("--split", choices=("train", "val", "test"), default="val")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--bootstrap", type=int, default=2000, help="subject-cluster paired bootstrap replicates; 0 disables")
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--output_npz", default=None, help="optional path for raw aligned predictions")
    p.add_argument("--stays_per_subject", type=int, default=2, help="synthetic cohort: consecutive stays that share a subject id")
    return p.parse_args(argv)


def build_model_and_loader(args, state: dict, device):
    """-> (teacher, loader, labels, perceiver_type): the teacher restored from its own checkpoint, the split of its synthetic cohort
    shuffled ONCE by a fixed generator (so the within-batch shuffles pair stays from the whole split), last partial batch kept."""
    from . import checkpoint, train_synthetic
    t_args = argparse.Namespace(**state["args"])
    perceiver_type = state["args"].get("perceiver_type")
    if perceiver_type not in ("dual", "dual_patch"):
        raise NotImplementedError(f"perceiver_type={perceiver_type!r} is not supported: dual / dual_patch only")
    teacher = checkpoint.load_model_state(train_synthetic.build_teacher(t_args, device), state, freeze=True)
    labels = tuple(s.strip() for s in state["args"]["pathology_labels"].split(","))
    datasets = dict(zip(("train", "val", "test"), train_synthetic._datasets(t_args)))
    dataset = SubjectAnnotatedDataset(datasets[args.split], args.stays_per_subject)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=True, generator=torch.Generator().manual_seed(args.seed),
                                         num_workers=args.num_workers, pin_memory=True, collate_fn=diagnostic_collate, drop_last=False)
    return teacher, loader, labels, perceiver_type


def main(argv=None) -> dict:
    """The reference's `main()` on a `train_synthetic` teacher checkpoint."""
    from . import checkpoint
    args = parse_args(argv)
    if args.split == "test":
        print("WARNING: use val for model diagnosis/selection. Reserve test for the final locked evaluation.")
    require_gpu()
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"device={device}  split={args.split}")
    state = checkpoint.load_ckpt(args.teacher_ckpt)
    teacher, loader, labels, perceiver_type = build_model_and_loader(args, state, device)
    print(f"perceiver_type={perceiver_type}  labels={labels}")
    pred = collect_predictions(teacher, loader, device, perceiver_type, args.seed)
    summary = summarise(pred, labels, args.bootstrap, args.seed)
    print_results(summary, attention_axis="time tokens")
    if args.output_npz:
        os.makedirs(os.path.dirname(os.path.abspath(args.output_npz)), exist_ok=True)
        np.savez_compressed(args.output_npz, **npz_payload(pred, labels))
        print(f"saved raw predictions: {args.output_npz}")
    return {"pred": pred, "summary": summary, "npz": args.output_npz}


if __name__ == "__main__":
    main()
