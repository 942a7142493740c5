"""Conditional-information probe of a trained dual teacher (reference analysis/conditional_information_probe.py) on the HIP kernels of
csrc/cond_probe.hip: does the temporal branch (`ts_logits`, `ts_tokens`) say anything about a label once `img_logits` is known?

The reference's names without the leading underscore and its return shapes; `run_probe` is the body of its `main()` label / probe
loop (:440-574); `bootstrap_differences`, `conditional_permutation` and `safe_metrics` are this probe's own draw or probability
construction followed by a call into probe_stats.py, which all analysis probes share.  Per label four models are fitted on the
probe-training split and scored on the test split:
    image_cal          sigmoid(a img + b)                              the control
    logit_add          sigmoid(a img + b ts + c)
    logit_interaction  logit_add + d img ts
    token_linear       sigmoid(a img + w.token + b)
each a `Pipeline(StandardScaler, LogisticRegression(C))` with a free, unpenalised intercept.  The reference stops its L-BFGS at
sklearn's `tol = 1e-4`; this module reports the optimum of the same objective (max|gradient| <= 1e-10), reached by a damped Newton
iteration in well under ten steps.  All fit arithmetic is fp64; `functional.precision()` is not consulted.

What runs where
  device, HIP   `probe_moments` (mean / scale of every column of every problem), `logistic_newton_terms` (objective, gradient and
                Hessian of ALL problems of a width group in one launch group, standardising the teacher's fp32 outputs on the fly:
                no standardised copy of the tokens exists), `probe_scores` (decision-function parts over any row list) and
                `probe_stats.resampled_binary_metrics` (BCE / AUROC / AUPRC of every bootstrap / permutation replicate).
  device, torch the teacher forwards of `gather`, the [N, K, 3] logit feature tensor (the product in fp32, as the reference takes it),
                the sigmoid of the scores and the gather that builds the permuted probability vectors.
  host, numpy   the Newton driver: per iteration ONE copy of (f, g, H) and one batched `numpy.linalg.solve` (<= 10 iterations of a few
                MB; no device solver library is needed), step halving, the index draws (`default_rng(seed)` in the reference's call
                order, so the replicates ARE the reference's), percentiles, Pearson correlation and the result rows.
sklearn, scipy and pandas are not dependencies.  Without a GPU every entry point raises (no CPU fallback)."""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Mapping, Sequence

import numpy as np
import torch

from .abi import MedpProbeProblem, check, fp32_matrix, lib, ptr, require_gpu, stream, table_bytes
from .probe_stats import (METRICS_MAX_LEN, binary_metrics, draw_bootstrap_indices, draw_conditional_shuffles, expit, inference_fields,
                          paired_bootstrap_gains, pearson, permutation_summary)

F64 = torch.float64
PROBE_NAMES = ("logit_add", "logit_interaction", "token_linear")
NARROW_WIDTH = {"image_cal": 1, "logit_add": 2, "logit_interaction": 3}       # columns of the (img, ts, img * ts) tensor a probe reads
ROW_KEYS = ("label", "probe", "n_test", "n_positive", "prevalence", "image_cal_bce", "image_cal_auroc", "image_cal_auprc", "probe_bce",
            "probe_auroc", "probe_auprc", "bce_gain", "auroc_gain", "auprc_gain", "bce_gain_ci_low", "bce_gain_ci_high",
            "auroc_gain_ci_low", "auroc_gain_ci_high", "auprc_gain_ci_low", "auprc_gain_ci_high", "corr_residual", "perm_bce_mean",
            "perm_bce_low", "perm_bce_high", "perm_auroc_mean", "perm_auroc_low", "perm_auroc_high", "perm_auprc_mean", "perm_auprc_low",
            "perm_auprc_high", "perm_bce_increase", "perm_auroc_drop", "evidence")          # the reference's row, in its order (:533-552)
GTOL = 1e-10           # max|gradient| of the mean-scaled objective at which a problem has converged
MAX_ITER = 50
MAX_HALVINGS = 40


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
class ProblemTable:
    """The problem table of one launch group, on both sides.  `entries`: per problem (col_off, F, row indices (host int array),
    y_col[, j0, j1]).  Every problem gets its own stretch of the concatenated row list (per-row outputs live at those positions)."""

    def __init__(self, entries: Sequence[tuple], device, Fmax: int | None = None):
        self.P = len(entries)
        self.host = (MedpProbeProblem * max(self.P, 1))()
        offset, parts = 0, []
        for p, e in enumerate(entries):
            col_off, F, rows, y_col = e[:4]
            j0, j1 = (e[4], e[5]) if len(e) > 4 else (0, F)
            rows = np.asarray(rows, dtype=np.int32).reshape(-1)
            self.host[p] = MedpProbeProblem(int(col_off), offset, int(rows.size), int(F), int(y_col), int(j0), int(j1), 0)
            parts.append(rows)
            offset += rows.size
        self.Fmax = int(max([e[1] for e in entries] + [1]) if Fmax is None else Fmax)
        self.rows_total = offset
        self.max_rows = max([r.size for r in parts] + [0])
        self.row_off = np.cumsum([0] + [r.size for r in parts])
        self.dev = torch.as_tensor(table_bytes(self.host, self.P), device=device)
        self.rows = torch.as_tensor(np.concatenate(parts) if parts else np.zeros(0, np.int32), device=device)

    def with_ranges(self, ranges: Sequence[tuple]) -> "ProblemTable":
        """The same problems and rows with other column ranges (j0, j1) for `probe_scores`."""
        t = object.__new__(ProblemTable)
        t.__dict__.update(self.__dict__)
        t.host = (MedpProbeProblem * max(self.P, 1))()
        for p, (j0, j1) in enumerate(ranges):
            q = self.host[p]
            t.host[p] = MedpProbeProblem(q.col_off, q.row_off, q.n_rows, q.F, q.y_col, int(j0), int(j1), 0)
        t.dev = torch.as_tensor(table_bytes(t.host, self.P), device=self.dev.device)
        return t


def probe_moments(X: torch.Tensor, table: ProblemTable):
    """(mean, scale) [P, Fmax] fp64: `StandardScaler.fit` of every problem's columns over its rows."""
    X, N, ldx = fp32_matrix(X, "X")
    mean = torch.empty((table.P, table.Fmax), dtype=F64, device=X.device)
    scale = torch.empty_like(mean)
    check(lib().medp_probe_moments(ptr(X), ldx, N, table.host, ptr(table.dev), ptr(table.rows), table.rows_total, ptr(mean), ptr(scale),
                                   table.P, table.Fmax, stream()), "probe_moments")
    return mean, scale


def terms_workspace(table: ProblemTable) -> torch.Tensor:
    nbytes = lib().medp_probe_terms_ws_bytes(table.P, table.Fmax, table.max_rows, table.rows_total)
    if nbytes == 0:
        raise ValueError(f"logistic_newton_terms: bad table (P={table.P}, Fmax={table.Fmax}, longest problem {table.max_rows} rows)")
    return torch.empty(nbytes // 8, dtype=F64, device=table.dev.device)


def logistic_newton_terms(X, y, table: ProblemTable, theta, mean, scale, l2, hessian: bool = True, ws=None):
    """theta [P, Fmax+1] (standardised space, intercept last), l2 [P] -> (f [P], g [P, Fmax+1], H [P, Fmax+1, Fmax+1] or None)."""
    X, N, ldx = fp32_matrix(X, "X")
    y, Ny, ldy = fp32_matrix(y, "y")
    if Ny != N:
        raise ValueError(f"logistic_newton_terms: X has {N} rows, y {Ny}")
    for t in (theta, mean, scale, l2):
        if t.dtype != F64:
            raise TypeError("logistic_newton_terms is fp64 only")
    theta, mean, scale, l2 = theta.contiguous(), mean.contiguous(), scale.contiguous(), l2.contiguous()
    S = table.Fmax + 1
    if theta.shape != (table.P, S) or mean.shape != (table.P, table.Fmax) or scale.shape != mean.shape or l2.numel() != table.P:
        raise ValueError("logistic_newton_terms: theta [P, Fmax+1], mean / scale [P, Fmax], l2 [P]")
    ws = terms_workspace(table) if ws is None else ws
    f = torch.empty(table.P, dtype=F64, device=X.device)
    g = torch.empty((table.P, S), dtype=F64, device=X.device)
    H = torch.empty((table.P, S, S), dtype=F64, device=X.device) if hessian else None
    check(lib().medp_logistic_newton_terms(ptr(X), ldx, N, ptr(y), ldy, table.host, ptr(table.dev), ptr(table.rows), table.rows_total,
                                           ptr(theta), ptr(mean), ptr(scale), ptr(l2), ptr(f), ptr(g), ptr(H), ptr(ws), ws.numel() * 8,
                                           table.P, table.Fmax, stream()), "logistic_newton_terms")
    return f, g, H


def probe_scores(X, table: ProblemTable, theta, mean, scale, intercept: bool = True) -> torch.Tensor:
    """Ragged scores [rows_total] fp64: problem p's rows sit at table.row_off[p] : table.row_off[p+1]; columns [j0, j1) of its table entry."""
    X, N, ldx = fp32_matrix(X, "X")
    out = torch.empty(table.rows_total, dtype=F64, device=X.device)
    check(lib().medp_probe_scores(ptr(X), ldx, N, table.host, ptr(table.dev), ptr(table.rows), table.rows_total, ptr(theta.contiguous()),
                                  ptr(mean.contiguous()), ptr(scale.contiguous()), ptr(out), table.P, table.Fmax, int(bool(intercept)),
                                  stream()), "probe_scores")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def gather(teacher, loader, device) -> Dict[str, torch.Tensor]:
    """The reference's `_gather` (:104-147) with the six arrays left on the device in fp32: img, ts, fus [N, K], token [N, K, D],
    y, mask [N, K]."""
    from .engine import _move_lists
    require_gpu()
    keys = ("img", "ts", "fus", "token", "y", "mask")
    parts: Dict[str, list] = {k: [] for k in keys}
    teacher.eval()
    for batch in loader:
        moved = _move_lists(batch, device)
        output = teacher(moved["x_ts"], moved["x_static"], moved["bin_ends"], moved["pixel_values"], return_attn=True)
        required = {"img_logits", "ts_logits", "fusion_logits", "ts_tokens"}
        missing = sorted(required.difference(output))
        if missing:
            raise RuntimeError("Conditional probe requires a dual teacher exposing "
                               f"{sorted(required)} with return_attn=True; missing={missing}")
        tokens = output["ts_tokens"]
        if tokens.ndim != 3:
            raise ValueError(f"Expected pathology-wise ts_tokens [B, K, D], got shape={tuple(tokens.shape)}")
        for k, v in zip(keys, (output["img_logits"], output["ts_logits"], output["fusion_logits"], tokens, moved["y_multi"],
                               moved["y_multi_mask"])):
            parts[k].append(v.detach().float())
    if not parts["img"]:
        raise RuntimeError("Probe loader yielded no batches")
    return {k: torch.cat(v).contiguous() for k, v in parts.items()}


def resolve_label_indices(requested: str, pathology_labels: Sequence[str]) -> tuple:
    """`_resolve_label_indices` (:150-167)."""
    if requested.strip().lower() == "all":
        return tuple(range(len(pathology_labels)))
    normalized = {name.lower(): i for i, name in enumerate(pathology_labels)}
    for i, name in enumerate(pathology_labels):
        normalized[name.lower().removeprefix("label_")] = i
    names = [item.strip().lower() for item in requested.split(",") if item.strip()]
    unknown = [name for name in names if name not in normalized]
    if unknown:
        raise ValueError(f"Unknown labels {unknown}; checkpoint labels={list(pathology_labels)}")
    indices = tuple(normalized[name] for name in names)
    if len(set(indices)) != len(indices):
        raise ValueError(f"Duplicate labels requested: {requested!r}")
    return indices


# ------------------------------------------------------------------------------------------------------------------------------
# the fit
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class FittedProbe:
    """A fitted `Pipeline(StandardScaler, LogisticRegression(C))`: the coefficients act on the standardised features."""
    label_index: int
    probe: str
    mean: np.ndarray
    scale: np.ndarray
    coef: np.ndarray
    intercept: float
    C: float
    n_iter: int
    max_gradient: float          # max|gradient| of the mean-scaled objective where the iteration stopped

    def decision_function(self, features) -> np.ndarray:
        x = features.detach().cpu().numpy() if isinstance(features, torch.Tensor) else np.asarray(features)
        x = x.astype(np.float64).reshape(len(x), -1)
        return ((x - self.mean) / self.scale) @ self.coef + self.intercept

    def predict(self, features):
        score = self.decision_function(features)
        return expit(score), score


def _feature_tensors(data: Mapping[str, torch.Tensor]):
    """(logit features [N, K, 3] = (img, ts, img * ts), the product in fp32 as `_features` takes it; token features [N, K, 1 + D])."""
    img, ts = data["img"].float(), data["ts"].float()
    feats = torch.stack([img, ts, img * ts], dim=2).contiguous()
    tok = torch.cat([img[:, :, None], data["token"].float()], dim=2).contiguous()
    return feats, tok


def _known_rows(mask_host: np.ndarray, label_index: int) -> np.ndarray:
    return np.flatnonzero(mask_host[:, label_index].astype(bool)).astype(np.int32)


def _group_entries(problems, mask_host, D):
    """Split (label, probe) problems into the narrow group (Fmax = 3, the [N, K, 3] tensor) and the token group ([N, K, 1 + D])."""
    narrow, token = [], []
    for pos, (k, name) in enumerate(problems):
        rows = _known_rows(mask_host, k)
        if name in NARROW_WIDTH:
            narrow.append((pos, (3 * k, NARROW_WIDTH[name], rows, k)))
        elif name == "token_linear":
            token.append((pos, ((1 + D) * k, 1 + D, rows, k)))
        else:
            raise ValueError(f"Unknown probe_name={name!r}")
    return narrow, token


def _newton(X, y, table: ProblemTable, l2_host: np.ndarray, max_iter: int):
    """Damped Newton on all problems of one table together -> (theta [P, S], mean, scale, n_iter [P], gmax [P]) on the host."""
    dev = X.device
    P, S = table.P, table.Fmax + 1
    mean, scale = probe_moments(X, table)
    l2 = torch.as_tensor(l2_host, dtype=F64, device=dev)
    ws = terms_workspace(table)
    eps = np.finfo(np.float64).eps

    def evaluate(theta, hessian):
        f, g, H = logistic_newton_terms(X, y, table, torch.as_tensor(theta, device=dev), mean, scale, l2, hessian, ws)
        flat = torch.cat([f, g.reshape(-1)] + ([H.reshape(-1)] if hessian else [])).cpu().numpy()    # ONE copy to the host
        f, g = flat[:P], flat[P:P + P * S].reshape(P, S)
        return f, g, (flat[P + P * S:].reshape(P, S, S) if hessian else None)

    theta = np.zeros((P, S))
    f, g, H = evaluate(theta, True)
    n_iter = np.zeros(P, dtype=np.int64)
    for _ in range(int(max_iter)):
        gmax = np.abs(g).max(1)
        if not np.isfinite(gmax).all():
            raise RuntimeError("Probe fit: non-finite gradient (a row index outside the feature matrix, or non-finite features)")
        active = gmax > GTOL
        if not active.any():
            break
        step = np.zeros_like(theta)
        step[active] = np.linalg.solve(H[active], -g[active][:, :, None])[:, :, 0]
        slope = (g * step).sum(1)                                        # < 0: H is positive definite
        t = np.ones(P)
        trial = theta + step
        ft, gt, Ht = evaluate(trial, True)                               # the full step is the rule: its terms serve the next iteration
        # sufficient decrease; at the rounding floor of f its differences are below a few ulp
        accept = lambda ft, t: ~active | (ft <= f + 1e-4 * t * slope + 8 * eps * np.abs(f))  # noqa: E731
        ok = accept(ft, t)
        if not ok.all():
            for _h in range(MAX_HALVINGS):                               # step halving in the value-only mode, converged problems masked
                t = np.where(ok, t, 0.5 * t)
                trial = theta + t[:, None] * step
                ft, gt, _ = evaluate(trial, False)
                ok = accept(ft, t)
                if ok.all():
                    break
            else:
                raise RuntimeError(f"Probe fit: the line search failed after {MAX_HALVINGS} halvings")
            ft, gt, Ht = evaluate(trial, True)
        theta, f, g, H = trial, ft, gt, Ht
        n_iter += active
    gmax = np.abs(g).max(1)
    if (gmax > GTOL).any():
        raise RuntimeError(f"Probe fit did not converge: max|gradient| = {gmax.max():.3e} > {GTOL:g} after max_iter = {max_iter} Newton "
                           "iterations")
    return theta, mean.cpu().numpy(), scale.cpu().numpy(), n_iter, gmax


def fit_probes(data: Mapping[str, torch.Tensor], problems: Sequence[tuple], *, logit_c: float = 100.0, token_c: float = 1.0,
               max_iter: int = MAX_ITER) -> list:
    """Fit every (label_index, probe_name) of `problems` on the gathered split `data` -> [FittedProbe] in the same order.  The
    narrow probes (image_cal, logit_add, logit_interaction) of all labels go as ONE group (Fmax = 3), the token probes as one."""
    require_gpu()
    dev = data["img"].device
    feats, tok = _feature_tensors(data)
    D = data["token"].shape[2]
    mask_host, y_host = data["mask"].cpu().numpy(), data["y"].cpu().numpy()
    for k in sorted({k for k, _ in problems}):
        known = mask_host[:, k].astype(bool)
        if len(np.unique(y_host[known, k].astype(np.int64))) < 2:
            raise ValueError("Probe-training labels contain only one class")
    fitted: list = [None] * len(problems)
    narrow, token = _group_entries(problems, mask_host, D)
    for group, X, Fmax in ((narrow, feats, 3), (token, tok, 1 + D)):
        if not group:
            continue
        table = ProblemTable([e for _, e in group], dev, Fmax)
        Cs = np.array([token_c if problems[pos][1] == "token_linear" else logit_c for pos, _ in group], dtype=np.float64)
        n = np.array([q.n_rows for q in table.host], dtype=np.float64)
        theta, mean, scale, n_iter, gmax = _newton(X, data["y"], table, 1.0 / (Cs * n), max_iter)
        for p, (pos, entry) in enumerate(group):
            F = entry[1]
            fitted[pos] = FittedProbe(problems[pos][0], problems[pos][1], mean[p, :F].copy(), scale[p, :F].copy(), theta[p, :F].copy(),
                                      float(theta[p, Fmax]), float(Cs[p]), int(n_iter[p]), float(gmax[p]))
    return fitted


def _padded(fits: Sequence[FittedProbe], Fmax: int, device):
    P = len(fits)
    theta, mean, scale = np.zeros((P, Fmax + 1)), np.zeros((P, Fmax)), np.ones((P, Fmax))
    for p, m in enumerate(fits):
        F = m.coef.size
        theta[p, :F], theta[p, Fmax], mean[p, :F], scale[p, :F] = m.coef, m.intercept, m.mean, m.scale
    return tuple(torch.as_tensor(a, device=device) for a in (theta, mean, scale))


def score_parts(data: Mapping[str, torch.Tensor], fits: Sequence[FittedProbe]) -> list:
    """Scores of fitted probes over the known rows of their label in the split `data` -> per probe a dict of device vectors
    {"score": full decision function, "image": intercept + image column, "ts": the remaining columns of the SAME table}: for the
    interaction probe "ts" is the ts column alone (its third column mixes both modalities)."""
    dev = data["img"].device
    feats, tok = _feature_tensors(data)
    D = data["token"].shape[2]
    mask_host = data["mask"].cpu().numpy()
    out: list = [None] * len(fits)
    narrow, token = _group_entries([(m.label_index, m.probe) for m in fits], mask_host, D)
    for group, X, Fmax in ((narrow, feats, 3), (token, tok, 1 + D)):
        if not group:
            continue
        table = ProblemTable([e for _, e in group], dev, Fmax)
        theta, mean, scale = _padded([fits[pos] for pos, _ in group], Fmax, dev)
        Fs = [e[1] for _, e in group]
        ts_hi = [min(F, 2) for F in Fs] if Fmax == 3 else Fs
        full = probe_scores(X, table, theta, mean, scale, True)
        image = probe_scores(X, table.with_ranges([(0, 1)] * len(Fs)), theta, mean, scale, True)
        ts = probe_scores(X, table.with_ranges([(min(F, 1), hi) for F, hi in zip(Fs, ts_hi)]), theta, mean, scale, False)
        for p, (pos, _) in enumerate(group):
            a, b = int(table.row_off[p]), int(table.row_off[p + 1])
            out[pos] = {"score": full[a:b], "image": image[a:b], "ts": ts[a:b]}
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# resampling
# ------------------------------------------------------------------------------------------------------------------------------
def safe_metrics(y, probability: torch.Tensor) -> Dict[str, float]:
    """`_safe_metrics` (:205-215) through the metrics kernel (one identity replicate); `probability`: a device vector."""
    return binary_metrics(y, probability)


def bootstrap_differences(y, base_probability, probe_probability, n_bootstrap: int, seed: int, device=None, index=None) -> Dict[str, float]:
    """Paired bootstrap; positive differences mean the probe is better (`_bootstrap_differences` :226-264).  The draws are the
    reference's; two launches of the metrics kernel score both probability vectors on every replicate.  Replicates with one class
    drop out of the AUROC / AUPRC lists only.  `index` [R, n] overrides the draws."""
    require_gpu()
    device = torch.device("cuda") if device is None else device
    y = np.asarray(y)
    n = len(y)
    if n > METRICS_MAX_LEN:
        raise ValueError(f"bootstrap_differences: {n} rows exceed METRICS_MAX_LEN = {METRICS_MAX_LEN}")
    index = draw_bootstrap_indices(n, n_bootstrap, seed) if index is None else np.asarray(index, dtype=np.int32).reshape(-1, n)
    offsets = torch.arange(0, (len(index) + 1) * n, n, dtype=torch.int64, device=device)
    return paired_bootstrap_gains(y, base_probability, probe_probability, index.reshape(-1), offsets, n, device)


def permuted_probabilities(model: FittedProbe, parts: Mapping[str, torch.Tensor], image_logit: torch.Tensor, ts_logit: torch.Tensor,
                           shuffles: np.ndarray) -> torch.Tensor:
    """[R, n] fp64 on the device: the model's probabilities with the TS inputs of row i taken from row shuffles[r, i].  The image part
    of the score stays, the TS part is gathered; the interaction column img_i * ts_pi(i) is rebuilt in fp32 and standardised with
    the training moments."""
    dev = parts["image"].device
    pi = torch.as_tensor(np.asarray(shuffles, dtype=np.int64), device=dev)
    score = parts["image"][None, :] + parts["ts"][pi]
    if model.probe == "logit_interaction":
        product = (image_logit.float()[None, :] * ts_logit.float()[pi]).to(F64)
        score = score + float(model.coef[2]) * ((product - float(model.mean[2])) / float(model.scale[2]))
    return torch.sigmoid(score)


def conditional_permutation(model: FittedProbe, parts, y, image_logit: torch.Tensor, ts_logit: torch.Tensor, repeats: int, n_bins: int,
                            seed: int, shuffles=None) -> Dict[str, float]:
    """Shuffle TS within image-risk bins and summarise the resulting metrics (`_conditional_permutation` :311-351): the reference's
    bins and draws; all `repeats` probability vectors are built on the device and scored by one launch of the metrics kernel."""
    if shuffles is None:
        shuffles = draw_conditional_shuffles(image_logit.cpu().numpy(), n_bins, repeats, seed)
    prob = permuted_probabilities(model, parts, image_logit, ts_logit, np.stack(shuffles)) if len(shuffles) else None
    return permutation_summary(y, prob)


# ------------------------------------------------------------------------------------------------------------------------------
# the label / probe loop
# ------------------------------------------------------------------------------------------------------------------------------
def _slug(value: str) -> str:
    return re.sub(r"[^0-9A-Za-z._-]+", "_", value).strip("_") or "label"


def _fmt(value: float, digits: int = 4, signed: bool = False) -> str:
    if not np.isfinite(value):
        return "--"
    return f"{value:{'+' if signed else ''}.{digits}f}"


def run_probe(train_data: Mapping[str, torch.Tensor], test_data: Mapping[str, torch.Tensor], pathology_labels: Sequence[str],
              selected: Sequence[int], *, logit_c: float = 100.0, token_c: float = 1.0, max_iter: int = MAX_ITER, bootstrap: int = 1000,
              perm_repeats: int = 100, perm_bins: int = 10, seed: int = 42, verbose: bool = True):
    """The reference's `main()` loop (:440-574) -> (rows, summary["labels"], prediction_archive).  All fits of all labels run as two
    launch groups before the loop; the loop scores, resamples and writes the reference's row keys with its `evidence` rule and seeds."""
    require_gpu()
    say = print if verbose else (lambda *a, **k: None)
    masks = {"train": train_data["mask"].cpu().numpy(), "test": test_data["mask"].cpu().numpy()}
    ys = {"train": train_data["y"].cpu().numpy(), "test": test_data["y"].cpu().numpy()}
    kept = []
    for k in selected:
        label = pathology_labels[k]
        y_train = ys["train"][masks["train"][:, k].astype(bool), k].astype(np.int64)
        y_test = ys["test"][masks["test"][:, k].astype(bool), k].astype(np.int64)
        if len(np.unique(y_train)) < 2 or len(np.unique(y_test)) < 2:
            say(f"[conditional-probe] skip {label}: one split has only one class")
            continue
        if len(y_test) > METRICS_MAX_LEN:
            raise ValueError(f"{label}: {len(y_test)} known test rows exceed METRICS_MAX_LEN = {METRICS_MAX_LEN}, the longest replicate "
                             "the metrics kernel sorts")
        kept.append((k, y_test))
    names = ("image_cal",) + PROBE_NAMES
    problems = [(k, name) for k, _ in kept for name in names]
    fits = fit_probes(train_data, problems, logit_c=logit_c, token_c=token_c, max_iter=max_iter) if problems else []
    parts = score_parts(test_data, fits) if fits else []
    rows: list = []
    label_summaries: Dict[str, object] = {}
    archive: Dict[str, np.ndarray] = {"test_img_logits": test_data["img"].cpu().numpy(), "test_ts_logits": test_data["ts"].cpu().numpy(),
                                      "test_fusion_logits": test_data["fus"].cpu().numpy(), "test_y": ys["test"], "test_mask": masks["test"]}
    for li, (k, y_test) in enumerate(kept):
        label = pathology_labels[k]
        known = torch.as_tensor(_known_rows(masks["test"], k).astype(np.int64), device=test_data["img"].device)
        image_test, ts_test = test_data["img"][known, k], test_data["ts"][known, k]
        base = parts[li * len(names)]
        base_probability_d = torch.sigmoid(base["score"])
        base_probability, base_score = base_probability_d.cpu().numpy(), base["score"].cpu().numpy()
        base_metrics = safe_metrics(y_test, base_probability_d)
        label_summary: Dict[str, object] = {"n_test": int(len(y_test)), "n_positive": int(y_test.sum()), "prevalence": float(y_test.mean()),
                                            "image_cal": base_metrics, "probes": {}}
        say(f"\n[{label}] n={len(y_test)} pos={int(y_test.sum())} image-cal BCE={base_metrics['bce']:.5f} "
            f"AUROC={base_metrics['auroc']:.4f} AUPRC={base_metrics['auprc']:.4f}")
        say("probe                 BCE   BCEgain [95% CI]       AUROC  dROC    AUPRC  dPRC   corr_r  perm_dBCE  evidence")
        say("-" * 117)
        for probe_offset, probe_name in enumerate(PROBE_NAMES):
            model, part = fits[li * len(names) + 1 + probe_offset], parts[li * len(names) + 1 + probe_offset]
            probability_d = torch.sigmoid(part["score"])
            probability, score = probability_d.cpu().numpy(), part["score"].cpu().numpy()
            metrics = safe_metrics(y_test, probability_d)
            confidence = bootstrap_differences(y_test, base_probability, probability, bootstrap, seed + 1000 * k + probe_offset,
                                               probability_d.device)
            corr_residual = pearson(score - base_score, y_test.astype(np.float64) - base_probability)
            permutation = conditional_permutation(model, part, y_test, image_test, ts_test, perm_repeats, perm_bins,
                                                  seed + 10000 * k + probe_offset)
            fields, evidence = inference_fields(base_metrics, metrics, confidence, corr_residual, permutation)
            row = {"label": label, "probe": probe_name, "n_test": int(len(y_test)), "n_positive": int(y_test.sum()),
                   "prevalence": float(y_test.mean()), **fields, "evidence": evidence}
            assert tuple(row) == ROW_KEYS
            rows.append(row)
            label_summary["probes"][probe_name] = row
            archive[f"{_slug(label)}_{probe_name}_probability"] = probability.astype(np.float32)
            say(f"{probe_name:<20} {metrics['bce']:.5f} {_fmt(row['bce_gain'], 5, True):>8} "
                f"[{_fmt(confidence['bce_gain_ci_low'], 5, True):>8},{_fmt(confidence['bce_gain_ci_high'], 5, True):>8}] "
                f"{metrics['auroc']:.4f} {_fmt(row['auroc_gain'], 4, True):>7} {metrics['auprc']:.4f} "
                f"{_fmt(row['auprc_gain'], 4, True):>7} {_fmt(corr_residual, 3, True):>7} {_fmt(row['perm_bce_increase'], 5, True):>10}  {evidence}")
        label_summaries[label] = label_summary
    summary = {"labels": label_summaries, "fits": [{"label": pathology_labels[m.label_index], "probe": m.probe, "C": m.C, "n_iter": m.n_iter,
                                                     "max_gradient": m.max_gradient} for m in fits]}
    return rows, summary, archive


# ------------------------------------------------------------------------------------------------------------------------------
# outputs, command line
# ------------------------------------------------------------------------------------------------------------------------------
def _json_ready(value):
    if isinstance(value, dict):
        return {str(key): _json_ready(item) for key, item in value.items()}
    if isinstance(value, (list, tuple)):
        return [_json_ready(item) for item in value]
    if isinstance(value, np.generic):
        return _json_ready(value.item())
    if isinstance(value, float) and not math.isfinite(value):
        return None
    return value


def write_outputs(outdir, rows: Sequence[Mapping[str, object]], summary: Mapping[str, object], archive: Mapping[str, np.ndarray]):
    """conditional_probe.csv / .json / _predictions.npz with the reference's keys (:576-582) -> the three paths."""
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    csv_path, json_path, npz_path = (outdir / "conditional_probe.csv", outdir / "conditional_probe.json",
                                     outdir / "conditional_probe_predictions.npz")
    if rows:
        with csv_path.open("w", newline="") as handle:
            writer = csv.DictWriter(handle, fieldnames=list(rows[0].keys()))
            writer.writeheader()
            writer.writerows(rows)
    with json_path.open("w") as handle:
        json.dump(_json_ready(dict(summary)), handle, indent=2, ensure_ascii=False)
    np.savez_compressed(npz_path, **archive)
    return csv_path, json_path, npz_path


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser("Probe image-conditional information in TS logits and pathology tokens")
    parser.add_argument("--ckpt", required=True, help="dual teacher best.pt written by train_synthetic")
    parser.add_argument("--outdir", required=True)
    parser.add_argument("--labels", default="all", help="comma-separated checkpoint labels, with or without 'label_'; default: all")
    parser.add_argument("--probe_train_split", default="val")
    parser.add_argument("--test_split", default="test")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("--logit_c", type=float, default=100.0, help="inverse L2 strength for image/logit probes")
    parser.add_argument("--token_c", type=float, default=1.0, help="inverse L2 strength for the high-dimensional token probe")
    parser.add_argument("--max_iter", type=int, default=MAX_ITER, help="Newton iterations (the reference's L-BFGS takes 3000 here)")
    parser.add_argument("--bootstrap", type=int, default=1000)
    parser.add_argument("--perm_repeats", type=int, default=100)
    parser.add_argument("--perm_bins", type=int, default=10)
    parser.add_argument("--seed", type=int, default=42)
    return parser.parse_args(argv)


def main(argv=None) -> dict:
    """The reference's `main()` (:386-592) on a `train_synthetic` teacher checkpoint; the splits are slices of its synthetic cohort."""
    from . import checkpoint, train_synthetic
    args = parse_args(argv)
    if args.probe_train_split == args.test_split:
        raise SystemExit("probe_train_split and test_split must be different")
    require_gpu()
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"[conditional-probe] device={device}")
    state = checkpoint.load_ckpt(args.ckpt)
    t_args = argparse.Namespace(**state["args"])
    mode = state["args"].get("perceiver_type")
    if mode not in ("dual", "dual_patch"):
        raise SystemExit(f"Expected a dual teacher checkpoint, got mode={mode!r}")
    teacher = train_synthetic.build_teacher_from_ckpt(state, t_args.d_static, t_args.n_vars, t_args.duett_ckpt, t_args.n_timesteps,
                                                      t_args.cxr_model_name).to(device)
    pathology_labels = tuple(s.strip() for s in state["args"]["pathology_labels"].split(","))
    datasets = dict(zip(("train", "val", "test"), train_synthetic._datasets(t_args)))
    for split in (args.probe_train_split, args.test_split):
        if split not in datasets:
            raise SystemExit(f"Unknown split={split!r}; available={list(datasets)}")
    selected = resolve_label_indices(args.labels, pathology_labels)
    print(f"[conditional-probe] mode={mode} labels={[pathology_labels[i] for i in selected]}")
    loader = lambda split: train_synthetic.make_loader(datasets[split], args.batch_size, False, args.num_workers, "teacher", 0, 1)  # noqa: E731
    print(f"[conditional-probe] gathering probe-train={args.probe_train_split} ...")
    train_data = gather(teacher, loader(args.probe_train_split), device)
    print(f"[conditional-probe] gathering test={args.test_split} ...")
    test_data = gather(teacher, loader(args.test_split), device)
    rows, probe_summary, archive = run_probe(train_data, test_data, pathology_labels, selected, logit_c=args.logit_c, token_c=args.token_c,
                                             max_iter=args.max_iter, bootstrap=args.bootstrap, perm_repeats=args.perm_repeats,
                                             perm_bins=args.perm_bins, seed=args.seed)
    summary = {"checkpoint": os.path.abspath(args.ckpt), "mode": mode, "probe_train_split": args.probe_train_split,
               "test_split": args.test_split, "configuration": vars(args), **probe_summary}
    csv_path, json_path, npz_path = write_outputs(args.outdir, rows, summary, archive)
    print(f"\n[conditional-probe] CSV  -> {csv_path}\n[conditional-probe] JSON -> {json_path}\n[conditional-probe] NPZ  -> {npz_path}")
    print("[interpretation] BCEgain > 0 is better. 'supported' requires a paired bootstrap BCE-gain CI above zero and worse BCE after "
          "within-image-risk TS permutation. This is evidence about the current representation, not proof that the raw TS data do or do "
          "not contain all possible signal.")
    return {"rows": rows, "summary": summary, "csv": str(csv_path), "json": str(json_path), "npz": str(npz_path)}


if __name__ == "__main__":
    main()
