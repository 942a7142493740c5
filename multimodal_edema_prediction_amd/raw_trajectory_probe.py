"""Raw-trajectory conditional probe (reference analysis/raw_trajectory_conditional_probe.py, its default path: the `offset_logistic`
model on the `level`, `trajectory`, `observation`, `physiologic` and `all` blocks) on the HIP kernels of csrc/raw_probe.hip.

The reference's names without the leading underscore and its return shapes, so that the body of its `main()` label / block loop
(:927-1075) restates on top of this module; `run_probe` is that restatement for one label.  All arithmetic is fp64, as in the
reference: there is no bf16 mode and `functional.precision()` is not consulted.  The resampling functions that carry the reference's
names are this probe's own draw or probability construction followed by a call into probe_stats.py, which all analysis probes share.

What runs where
  device, HIP   `raw_traj_summary` (the 14 statistics per (window, variable)), `offset_logistic_valgrad` (objective + gradient of G
                candidates per launch; also the held-out BCE of a fold), `probe_stats.resampled_binary_metrics` (csrc/binary_metrics.hip:
                BCE / AUROC / AUPRC of every bootstrap or permutation replicate in one launch).
  device, torch median imputation + missing indicators + standardisation (fp64), the batched L-BFGS two-loop recursion and its
                masked line search (no host round trip but ONE convergence flag per evaluation), the final X.w of a prediction.
  host, numpy   the index draws (`default_rng(seed)`, the reference's call order, so the replicates ARE the reference's), the fold
                split, percentiles, the two-parameter image calibration (a closed 2 x 2 Newton iteration) and the result rows.
sklearn, scipy and pandas are not dependencies.  Without a GPU every device entry point raises (no CPU fallback)."""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Dict, Mapping, Sequence

import numpy as np
import torch

from .abi import check, lib, ptr, stream
from .probe_stats import (binary_metrics, draw_cluster_bootstrap_indices, draw_conditional_shuffles, expit, inference_fields,
                          paired_bootstrap_gains, pearson, permutation_summary, to_device, to_host, unit_or_sd)

F64 = torch.float64
LEVEL_STATS = ("last", "mean", "std", "min", "max")
TRAJECTORY_STATS = ("delta", "slope24", "slope_recent", "recent_shift")
OBSERVATION_STATS = ("observed_fraction", "log_total_count", "time_since_last", "recent_observed_fraction", "log_recent_count")
DEFAULT_BLOCKS = ("level", "trajectory", "observation", "physiologic", "all")
DEFAULT_L2_GRID = (0.0001, 0.001, 0.01, 0.1, 1.0, 10.0, 100.0)
DEFAULT_C_GRID = (0.001, 0.01, 0.1, 1.0, 10.0)
MAX_CANDIDATES = 8             # MEDP_OFFSET_LOGISTIC_MAX_G
GTOL = 1e-7                    # the reference's L-BFGS-B `gtol` (max-norm of the gradient)


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
def raw_traj_summary(x: torch.Tensor, recent_hours: int) -> torch.Tensor:
    """x [B,T,2V] fp32 (values | counts) -> [B,V,14] fp64 in the order LEVEL_STATS, TRAJECTORY_STATS, OBSERVATION_STATS."""
    B, T, C = x.shape
    if C % 2:
        raise ValueError(f"x_ts has {C} channels: expected values | counts")
    xc = x.detach().to(torch.float32).contiguous()
    out = torch.empty((B, C // 2, 14), dtype=F64, device=x.device)
    check(lib().medp_raw_traj_summary(ptr(xc), ptr(out), B, T, C // 2, int(recent_hours), stream()), "raw_traj_summary")
    return out


def offset_logistic_valgrad(X, y, offset, W, l2, ws=None):
    """X [n,F] (row-major, any row stride), y [n], offset [n], W [F,G], l2 [G], all fp64 on the device -> (objective [G], gradient [F,G])
    of `_fit_offset_weights` (:578-584) for the G <= 8 columns of W, one launch.  `ws`: a reusable workspace from `valgrad_workspace`."""
    n, F = X.shape
    G = W.shape[1]
    for t in (X, y, offset, W, l2):
        if t.dtype != F64:
            raise TypeError("offset_logistic_valgrad is fp64 only")
    if X.stride(1) != 1:
        X = X.contiguous()
    y, offset, W, l2 = y.contiguous(), offset.contiguous(), W.contiguous(), l2.contiguous()
    if ws is None:
        ws = valgrad_workspace(n, F, G, X.device)
    obj = torch.empty(G, dtype=F64, device=X.device)
    grad = torch.empty((F, G), dtype=F64, device=X.device)
    check(lib().medp_offset_logistic_valgrad(ptr(X), X.stride(0), ptr(y), ptr(offset), ptr(W), ptr(l2), ptr(obj), ptr(grad), ptr(ws),
                                             ws.numel() * 8, n, F, G, stream()), "offset_logistic_valgrad")
    return obj, grad


def valgrad_workspace(n: int, F: int, G: int, device) -> torch.Tensor:
    nbytes = lib().medp_offset_logistic_ws_bytes(n, F, G)
    if nbytes == 0:
        raise ValueError(f"offset_logistic_valgrad: bad shape n={n} F={F} G={G} (1 <= G <= {MAX_CANDIDATES})")
    return torch.empty(nbytes // 8, dtype=F64, device=device)


# ------------------------------------------------------------------------------------------------------------------------------
# summaries
# ------------------------------------------------------------------------------------------------------------------------------
def raw_summary_blocks(x_ts, ts_vars: Sequence[str], recent_hours: int):
    """(blocks, names) of `_raw_summary_blocks` (:423-476): x_ts is a device tensor [N,T,2V] or the collated tuple of [T,2V] tensors;
    blocks maps level / trajectory / observation / physiologic / all to fp64 device matrices [N, V*k], names to `var__stat` tuples."""
    if isinstance(x_ts, (tuple, list)):
        x_ts = torch.stack(list(x_ts))
    N, T, C = x_ts.shape
    if C != 2 * len(ts_vars):
        raise ValueError(f"x_ts has {C} channels for {len(ts_vars)} variables (expected values | counts)")
    if recent_hours < 1 or recent_hours > T:
        raise ValueError(f"recent_hours must be within [1, {T}], got {recent_hours}")
    s = raw_traj_summary(x_ts, recent_hours)
    level, trajectory, observation = s[:, :, 0:5].reshape(N, -1), s[:, :, 5:9].reshape(N, -1), s[:, :, 9:14].reshape(N, -1)
    physiologic = torch.cat([level, trajectory], 1)
    blocks = {"level": level, "trajectory": trajectory, "observation": observation, "physiologic": physiologic,
              "all": torch.cat([physiologic, observation], 1)}
    n_level = tuple(f"{v}__{st}" for v in ts_vars for st in LEVEL_STATS)
    n_traj = tuple(f"{v}__{st}" for v in ts_vars for st in TRAJECTORY_STATS)
    n_obs = tuple(f"{v}__{st}" for v in ts_vars for st in OBSERVATION_STATS)
    names = {"level": n_level, "trajectory": n_traj, "observation": n_obs, "physiologic": n_level + n_traj,
             "all": n_level + n_traj + n_obs}
    return blocks, names


# ------------------------------------------------------------------------------------------------------------------------------
# folds, pre-processing
# ------------------------------------------------------------------------------------------------------------------------------
def stratified_folds(y, requested_folds: int, seed: int):
    """[(train_idx, valid_idx)]: a stratified shuffled split drawn from `numpy.random.default_rng(seed)`.  NOT sklearn's
    `StratifiedKFold(shuffle=True, random_state=seed)` sequence (pass recorded `folds` to reproduce one); the fold count follows
    `_cv_splitter` (:504-509): min(requested, smallest class count), at least 2."""
    y = np.asarray(y, dtype=np.int64)
    counts = np.bincount(y, minlength=2)
    k = min(int(requested_folds), int(counts.min()))
    if k < 2:
        raise ValueError(f"Not enough samples in both classes for CV: counts={counts}")
    rng = np.random.default_rng(seed)
    fold_of = np.empty(len(y), dtype=np.int64)
    start = 0
    for cls in np.unique(y):
        members = rng.permutation(np.flatnonzero(y == cls))
        fold_of[members] = (start + np.arange(len(members))) % k          # the classes deal round-robin where the last one stopped
        start = (start + len(members)) % k
    everyone = np.arange(len(y))
    return [(everyone[fold_of != f], everyone[fold_of == f]) for f in range(k)]


def _check_folds(y, folds, requested_folds):
    counts = np.bincount(np.asarray(y, dtype=np.int64), minlength=2)
    if min(int(requested_folds), int(counts.min())) < 2:
        raise ValueError(f"Not enough samples in both classes for CV: counts={counts}")
    return [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in folds]


@dataclass
class Preprocessor:
    """`SimpleImputer(strategy="median", add_indicator=True)` followed by `StandardScaler`, fitted on the device in fp64."""
    keep: torch.Tensor           # input columns with at least one observed fitting row
    medians: torch.Tensor        # [len(keep)]
    indicator: torch.Tensor      # input columns with a NaN in the fitting rows (all-NaN ones included, as in sklearn)
    mean: torch.Tensor
    scale: torch.Tensor

    @staticmethod
    def fit(X: torch.Tensor) -> "Preprocessor":
        nan = torch.isnan(X)
        n_obs = (~nan).sum(0)
        keep = torch.nonzero(n_obs > 0).flatten()
        indicator = torch.nonzero(nan.any(0)).flatten()
        srt = torch.sort(X[:, keep], dim=0).values                        # NaN sorts last
        cnt = n_obs[keep]
        lo = srt.gather(0, ((cnt - 1) // 2)[None, :])[0]
        hi = srt.gather(0, (cnt // 2)[None, :])[0]
        pre = Preprocessor(keep, (lo + hi) / 2.0, indicator, None, None)  # even count: the mean of the middle two
        Z = pre._impute(X)
        n = Z.shape[0]
        mean = Z.mean(0)
        var = ((Z - mean) ** 2).mean(0)                                   # population variance
        pre.mean, pre.scale = mean, unit_or_sd(var, mean, n)              # a constant column keeps scale 1
        return pre

    def _impute(self, X):
        Z = X[:, self.keep]
        Z = torch.where(torch.isnan(Z), self.medians.expand_as(Z), Z)
        return torch.cat([Z, torch.isnan(X[:, self.indicator]).to(F64)], 1)

    def transform(self, X: torch.Tensor) -> torch.Tensor:
        return ((self._impute(X) - self.mean) / self.scale).contiguous()

    def names(self, input_names: Sequence[str]) -> tuple:
        return tuple([input_names[i] for i in self.keep.tolist()] + [f"missingindicator_{input_names[i]}" for i in self.indicator.tolist()])


# ------------------------------------------------------------------------------------------------------------------------------
# the fit
# ------------------------------------------------------------------------------------------------------------------------------
def bce_from_scores(y: torch.Tensor, score: torch.Tensor) -> torch.Tensor:
    """Stable mean binary cross-entropy from logits (`_bce_from_scores` :556-560), on the device."""
    return (torch.logaddexp(torch.zeros_like(score), score) - y * score).mean()


def fit_offset_weights(features, y, fixed_offset, l2_strengths, max_iter: int, history: int = 10) -> torch.Tensor:
    """argmin_w mean BCE(fixed_offset + X w) + 0.5 l2 w.w for every l2 in `l2_strengths` at once -> W [F, G] (`_fit_offset_weights`
    :563-598 for G strengths).  A batched L-BFGS: the G columns advance together, one `offset_logistic_valgrad` launch per
    evaluation; the two-loop recursion and the Armijo backtracking are masked torch arithmetic on the device, so the only host
    round trip per evaluation is the convergence flag.  A column stops when max|gradient| <= 1e-7 (the reference's `gtol`; the
    reference may stop earlier on its `ftol`, further from the optimum).  Raises when `max_iter` evaluations did not get there."""
    n, F = features.shape
    dev = features.device
    l2 = torch.as_tensor(l2_strengths, dtype=F64, device=dev).reshape(-1)
    G = l2.numel()
    if F == 0:
        return torch.zeros((0, G), dtype=F64, device=dev)
    if G > MAX_CANDIDATES:
        return torch.cat([fit_offset_weights(features, y, fixed_offset, l2[i:i + MAX_CANDIDATES], max_iter, history)
                          for i in range(0, G, MAX_CANDIDATES)], 1)
    ws = valgrad_workspace(n, F, G, dev)
    evaluate = lambda W: offset_logistic_valgrad(features, y, fixed_offset, W, l2, ws)  # noqa: E731
    W = torch.zeros((F, G), dtype=F64, device=dev)
    f, g = evaluate(W)
    S = torch.zeros((history, F, G), dtype=F64, device=dev)
    Y = torch.zeros_like(S)
    rho = torch.zeros((history, G), dtype=F64, device=dev)               # 0: an empty (or skipped) slot drops out of the recursion
    gamma = torch.ones(G, dtype=F64, device=dev)
    d = -g
    step = 1.0 / g.abs().sum(0).clamp_min(1e-300)                        # first trial, as L-BFGS-B scales it; afterwards 1
    slope = (g * d).sum(0)
    tiny = 4 * torch.finfo(F64).eps
    for _ in range(int(max_iter)):
        gmax = g.abs().amax(0)
        active = gmax > GTOL
        if not bool(active.any()):                                       # the one host synchronisation of this evaluation
            return W
        Wt = W + torch.where(active, step, torch.zeros_like(step)) * d
        ft, gt = evaluate(Wt)
        slope_t = (gt * d).sum(0)
        # sufficient decrease; at the rounding floor of f (differences below a few ulp) a flatter directional derivative decides
        ok = (ft <= f + 1e-4 * step * slope) | ((ft <= f + tiny * f.abs()) & (slope_t.abs() <= 0.9 * slope.abs()))
        ok &= active
        s, yv = Wt - W, gt - g
        sy, yy = (s * yv).sum(0), (yv * yv).sum(0)
        push = ok & (sy > 1e-10 * yy) & (yy > 0)                         # curvature condition: otherwise the pair is skipped
        S = torch.where(ok, torch.cat([S[1:], s[None]]), S)              # an accepted column shifts its history by one slot
        Y = torch.where(ok, torch.cat([Y[1:], yv[None]]), Y)
        rho = torch.where(ok, torch.cat([rho[1:], torch.where(push, 1.0 / sy.clamp_min(1e-300), torch.zeros_like(sy))[None]]), rho)
        gamma = torch.where(push, sy / yy.clamp_min(1e-300), gamma)
        W, f, g = torch.where(ok, Wt, W), torch.where(ok, ft, f), torch.where(ok, gt, g)
        # two-loop recursion for every column (rho = 0 slots contribute nothing)
        q = g.clone()
        alpha = []
        for i in range(history - 1, -1, -1):
            a = rho[i] * (S[i] * q).sum(0)
            q = q - a * Y[i]
            alpha.append(a)
        r = gamma * q
        for i in range(history):
            b = rho[i] * (Y[i] * r).sum(0)
            r = r + S[i] * (alpha[history - 1 - i] - b)
        d = torch.where(ok, -r, d)
        slope = torch.where(ok, (g * d).sum(0), slope)
        step = torch.where(ok, torch.ones_like(step), 0.5 * step)
    if bool((g.abs().amax(0) > GTOL).any()):
        raise RuntimeError(f"Offset correction optimization failed: max|gradient| = {float(g.abs().amax()):.3e} > {GTOL:g} after "
                           f"max_iter = {max_iter} evaluations")
    return W


@dataclass
class OffsetCorrectionModel:
    """Preprocessed TS correction added to an externally fixed image score (the reference class, :601-652)."""
    preprocessor: Preprocessor
    weights: np.ndarray
    input_names: tuple
    transformed_names: tuple
    selected_l2: float | None
    cv_bce: float
    cv_results: Mapping[str, float]

    @property
    def null_selected(self) -> bool:
        return self.selected_l2 is None

    @property
    def best_params_(self) -> Dict[str, object]:
        if self.null_selected:
            return {"correction": "null", "correction_l2": None}
        return {"correction": "offset_logistic", "correction_l2": float(self.selected_l2)}

    def correction(self, raw_features: torch.Tensor) -> torch.Tensor:
        """X.w on the device, [n] fp64."""
        w = torch.as_tensor(self.weights, dtype=F64, device=raw_features.device)
        return self.preprocessor.transform(raw_features.to(F64)) @ w

    def decision_function(self, fixed_image_score, raw_features: torch.Tensor) -> np.ndarray:
        return np.asarray(fixed_image_score, dtype=np.float64) + self.correction(raw_features).cpu().numpy()

    def predict(self, fixed_image_score, raw_features: torch.Tensor):
        score = self.decision_function(fixed_image_score, raw_features)
        return expit(score), score

    def standardized_coefficients(self):
        return sorted([(name, float(c)) for name, c in zip(self.transformed_names, self.weights)], key=lambda item: abs(item[1]),
                      reverse=True)


def fit_offset_correction(raw_train, y_train, fixed_image_score, l2_grid: Sequence[float], cv_folds: int, max_iter: int,
                          null_tolerance: float, seed: int, folds=None, input_names: Sequence[str] | None = None) -> OffsetCorrectionModel:
    """Inner-CV selection with an exact zero-correction candidate (`_fit_offset_correction` :655-747).  raw_train: fp64 device matrix
    [n, F] with NaN for missing; y_train, fixed_image_score: host or device vectors.  `folds` = [(train_idx, valid_idx)] overrides the
    default `stratified_folds(y_train, cv_folds, seed)`."""
    if null_tolerance < 0:
        raise ValueError("null_tolerance must be non-negative")
    dev = raw_train.device
    raw_train = raw_train.to(F64)
    y_host = to_host(y_train).astype(np.int64)
    folds = stratified_folds(y_host, cv_folds, seed) if folds is None else _check_folds(y_host, folds, cv_folds)
    y, offset = to_device(y_host, np.float64, dev), to_device(fixed_image_score, np.float64, dev)
    input_names = tuple(f"x{i}" for i in range(raw_train.shape[1])) if input_names is None else tuple(str(n) for n in input_names)
    candidate_names = ["null"] + [f"l2={value:g}" for value in l2_grid]
    zeros = torch.zeros(len(l2_grid), dtype=F64, device=dev)
    fold_losses = []
    for train_index, valid_index in folds:
        tr, va = torch.as_tensor(train_index, device=dev), torch.as_tensor(valid_index, device=dev)
        pre = Preprocessor.fit(raw_train[tr])
        W = fit_offset_weights(pre.transform(raw_train[tr]), y[tr], offset[tr], l2_grid, max_iter)
        # held-out BCE of every candidate: the same kernel with zero penalty (its objective IS the mean BCE)
        held_out = _chunked_objective(pre.transform(raw_train[va]), y[va], offset[va], W, zeros)
        fold_losses.append(torch.cat([bce_from_scores(y[va], offset[va])[None], held_out]))
    mean_losses_v = torch.stack(fold_losses).mean(0).cpu().numpy()
    mean_losses = {name: float(v) for name, v in zip(candidate_names, mean_losses_v)}
    best_non_null = min((name for name in candidate_names if name != "null"), key=mean_losses.__getitem__)
    if mean_losses["null"] <= mean_losses[best_non_null] + null_tolerance:
        selected_name, selected_l2 = "null", None
    else:
        selected_name, selected_l2 = best_non_null, float(best_non_null.split("=", 1)[1])
    final = Preprocessor.fit(raw_train)
    transformed = final.transform(raw_train)
    if selected_l2 is None:
        weights = np.zeros(transformed.shape[1], dtype=np.float64)
    else:
        weights = fit_offset_weights(transformed, y, offset, [selected_l2], max_iter)[:, 0].cpu().numpy()
    return OffsetCorrectionModel(final, weights, input_names, final.names(input_names), selected_l2, mean_losses[selected_name],
                                 mean_losses)


def _chunked_objective(X, y, offset, W, l2):
    if X.shape[1] == 0:
        return bce_from_scores(y, offset).expand(W.shape[1])
    return torch.cat([offset_logistic_valgrad(X, y, offset, W[:, i:i + MAX_CANDIDATES], l2[i:i + MAX_CANDIDATES])[0]
                      for i in range(0, W.shape[1], MAX_CANDIDATES)])


# ------------------------------------------------------------------------------------------------------------------------------
# resampling
# ------------------------------------------------------------------------------------------------------------------------------
def cluster_bootstrap_differences(y, base_probability, probe_probability, subject_ids, n_bootstrap: int, seed: int,
                                  device=None) -> Dict[str, float]:
    """Paired patient-cluster bootstrap; positive values favor the probe (`_cluster_bootstrap_differences` :760-801).  The draws are
    the reference's; both probability vectors are scored on every replicate by two launches of the metrics kernel."""
    device = torch.device("cuda") if device is None else device
    idx, offsets = draw_cluster_bootstrap_indices(np.asarray(subject_ids), n_bootstrap, seed)
    max_len = int(np.diff(offsets).max()) if len(offsets) > 1 else 0
    return paired_bootstrap_gains(np.asarray(y), base_probability, probe_probability, idx, offsets, max_len, device)


def conditional_permutation_offset(model: OffsetCorrectionModel, y, image_logit, fixed_image_score, raw_features: torch.Tensor,
                                   repeats: int, n_bins: int, seed: int) -> Dict[str, float]:
    """Shuffle the whole raw-TS feature row among similar image-risk samples (`_conditional_permutation_offset` :804-840).  The
    pre-processing is row-wise, so shuffling the rows shuffles the corrections X.w: one gather builds all `repeats` probability
    vectors on the device and one launch of the metrics kernel scores them."""
    dev = raw_features.device
    shuffles = draw_conditional_shuffles(np.asarray(image_logit), n_bins, repeats, seed)
    if not shuffles:
        return permutation_summary(y, None)
    fixed = to_device(fixed_image_score, np.float64, dev)
    corr = model.correction(raw_features)
    return permutation_summary(y, torch.sigmoid(fixed[None, :] + corr[torch.as_tensor(np.stack(shuffles), device=dev)]))


def safe_metrics(y, probability, device=None) -> Dict[str, float]:
    """`_safe_metrics` (:109-119) through the metrics kernel (one identity replicate)."""
    return binary_metrics(y, probability, device)


# ------------------------------------------------------------------------------------------------------------------------------
# image calibration (host)
# ------------------------------------------------------------------------------------------------------------------------------
def _newton_logistic(z, y, C, iters=100):
    """argmin C sum BCE(w z + b) + 0.5 w^2 (intercept unpenalised): sklearn's `LogisticRegression(C=C)` objective on one feature."""
    w = b = 0.0

    def value(w, b):
        s = w * z + b
        return C * np.sum(np.logaddexp(0.0, s) - y * s) + 0.5 * w * w

    f = value(w, b)
    for _ in range(iters):
        p = expit(w * z + b)
        r, h = p - y, p * (1.0 - p)
        g = np.array([C * np.sum(r * z) + w, C * np.sum(r)])
        if np.abs(g).max() <= 1e-12 * max(1.0, C * len(y)):
            break
        H = np.array([[C * np.sum(h * z * z) + 1.0, C * np.sum(h * z)], [C * np.sum(h * z), C * np.sum(h)]])
        dw, db = np.linalg.solve(H, -g)
        t = 1.0
        while t > 1e-12 and not value(w + t * dw, b + t * db) <= f:      # the objective is convex: halve until it does not rise
            t *= 0.5
        w, b = w + t * dw, b + t * db
        f = value(w, b)
    return w, b


@dataclass
class ImageCalibration:
    """The fitted `Pipeline(impute, scale, LogisticRegression)` of the reference's image calibration, two parameters."""
    mean: float
    scale: float
    coef: float
    intercept: float
    best_params_: Dict[str, float]
    best_score_: float           # -CV log-loss of the selected C, sklearn's sign convention
    cv_bce: np.ndarray           # mean CV log-loss per C of the grid

    def decision_function(self, image_logit) -> np.ndarray:
        return self.coef * (np.asarray(image_logit, np.float64) - self.mean) / self.scale + self.intercept

    def predict(self, image_logit):
        score = self.decision_function(image_logit)
        return expit(score), score


def _fit_scaled_logistic(z, y, C):
    mean, var = z.mean(), z.var()
    scale = unit_or_sd(var, mean, len(z))
    w, b = _newton_logistic((z - mean) / scale, y, C)
    return mean, scale, w, b


def calibrate_image_logit(image_train, y_train, c_grid: Sequence[float] = DEFAULT_C_GRID, cv_folds: int = 5, seed: int = 42,
                          folds=None) -> ImageCalibration:
    """The two-parameter L2 logistic of :940-953 (`_fit_model("logistic", ...)` on the image logit alone): the scaler sits inside the
    pipeline (refitted per fold), the intercept is unpenalised, C is selected by mean CV log-loss (the first of equal ones)."""
    z, y = np.asarray(image_train, np.float64).reshape(-1), np.asarray(y_train, np.float64).reshape(-1)
    if not np.isfinite(z).all():
        raise ValueError("image logits must be finite")
    folds = stratified_folds(y, cv_folds, seed) if folds is None else _check_folds(y, folds, cv_folds)
    cv = np.zeros(len(c_grid))
    for k, C in enumerate(c_grid):
        losses = []
        for tr, va in folds:
            mean, scale, w, b = _fit_scaled_logistic(z[tr], y[tr], float(C))
            s = w * (z[va] - mean) / scale + b
            losses.append(np.mean(np.logaddexp(0.0, s) - y[va] * s))
        cv[k] = np.mean(losses)
    best = int(np.argmin(cv))
    mean, scale, w, b = _fit_scaled_logistic(z, y, float(c_grid[best]))
    return ImageCalibration(float(mean), float(scale), float(w), float(b), {"model__C": float(c_grid[best])}, float(-cv[best]), cv)


# ------------------------------------------------------------------------------------------------------------------------------
# the label / block loop
# ------------------------------------------------------------------------------------------------------------------------------
def run_probe(train_blocks: Mapping[str, torch.Tensor], test_blocks: Mapping[str, torch.Tensor], block_names: Mapping[str, Sequence[str]],
              y_train, y_test, image_train, image_test, subject_test, *, label: str = "label", label_index: int = 0,
              blocks: Sequence[str] = DEFAULT_BLOCKS, c_grid: Sequence[float] = DEFAULT_C_GRID,
              correction_l2_grid: Sequence[float] = DEFAULT_L2_GRID, null_tolerance: float = 5e-4, cv_folds: int = 5,
              max_iter: int = 3000, bootstrap: int = 1000, perm_repeats: int = 100, perm_bins: int = 10, seed: int = 42,
              calibration_folds=None, correction_folds: Mapping[str, list] | None = None):
    """One label of the reference's `main()` loop (:927-1075) -> (rows, fitted): a result row per block with the reference's keys
    (metrics, gains, cluster-bootstrap CIs, conditional-permutation statistics, `evidence`), and the fitted models
    {"image_cal": ImageCalibration, block: OffsetCorrectionModel}.  Blocks are fp64 device matrices (`raw_summary_blocks`); labels,
    image logits and subject ids are host vectors of the rows where the label is known.  Seeds follow the reference
    (`seed + label_index * 1000 + probe_offset + 1` for the fit, `* 10000` / `* 100000` for the bootstrap / permutation draws)."""
    y_train, y_test = np.asarray(y_train).astype(np.int64), np.asarray(y_test).astype(np.int64)
    image_train, image_test, subject_test = np.asarray(image_train), np.asarray(image_test), np.asarray(subject_test)
    if np.unique(y_train).size < 2 or np.unique(y_test).size < 2:
        raise ValueError(f"{label}: one split has one class")
    dev = next(iter(train_blocks.values())).device
    cal = calibrate_image_logit(image_train, y_train, c_grid, cv_folds, seed + label_index * 1000, folds=calibration_folds)
    base_train_score = cal.decision_function(image_train)
    base_probability, base_score = cal.predict(image_test)
    base_metrics = safe_metrics(y_test, base_probability, dev)
    rows, fitted_models = [], {"image_cal": cal}
    for probe_offset, block in enumerate(blocks):
        names = tuple(block_names[block])
        raw_train, raw_test = train_blocks[block], test_blocks[block]
        fitted = fit_offset_correction(raw_train, y_train, base_train_score, correction_l2_grid, cv_folds, max_iter, null_tolerance,
                                       seed + label_index * 1000 + probe_offset + 1,
                                       folds=None if correction_folds is None else correction_folds.get(block), input_names=names)
        probability, score = fitted.predict(base_score, raw_test)
        metrics = safe_metrics(y_test, probability, dev)
        confidence = cluster_bootstrap_differences(y_test, base_probability, probability, subject_test, bootstrap,
                                                   seed + label_index * 10000 + probe_offset, dev)
        corr_residual = pearson(score - base_score, y_test.astype(np.float64) - base_probability)
        permutation = conditional_permutation_offset(fitted, y_test, image_test, base_score, raw_test, perm_repeats, perm_bins,
                                                     seed + label_index * 100000 + probe_offset)
        fields, evidence = inference_fields(base_metrics, metrics, confidence, corr_residual, permutation)
        rows.append({
            "label": label, "model": "offset_logistic", "block": block, "n_test": int(len(y_test)), "n_positive": int(y_test.sum()),
            "prevalence": float(y_test.mean()), "n_input_features": int(raw_train.shape[1]), **fields, "inner_cv_bce": fitted.cv_bce,
            "best_params": json.dumps(fitted.best_params_, sort_keys=True),
            "correction_cv_results": json.dumps(fitted.cv_results, sort_keys=True),
            "null_selected": fitted.null_selected, "evidence": evidence})
        fitted_models[block] = fitted
    return rows, fitted_models
