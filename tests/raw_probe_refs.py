"""Numpy restatement of the three raw-trajectory-probe kernels (csrc/raw_probe.hip, csrc/binary_metrics.hip), pinned on
tests/golden/raw_probe.npz by tests/test_raw_probe_refs_cpu.py and compared with the kernels by tests/test_gpu_raw_probe_kernels.py.  Written from the reference's
definitions (analysis/raw_trajectory_conditional_probe.py), not from the kernels: the summaries walk the hours in order with the
reference's centred two-pass formulas, AUROC is the Mann-Whitney statistic on tie-averaged ranks and AUPRC the step sum over distinct
thresholds."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_probe.npz")
STATS = ("last", "mean", "std", "min", "max", "delta", "slope24", "slope_recent", "recent_shift",
         "observed_fraction", "log_total_count", "time_since_last", "recent_observed_fraction", "log_recent_count")
EXACT_STATS = ("last", "min", "max", "delta", "observed_fraction", "time_since_last", "recent_observed_fraction")   # no accumulation
METRICS_MAX_LEN = 16384          # MEDP_RESAMPLED_METRICS_MAX_LEN (include/medp_hip.h)

_cache = {}


def golden():
    """The fixture, loaded once and shared (read-only) by every test that needs it."""
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
        for v in _cache["g"].values():
            v.setflags(write=False)
    return _cache["g"]


def golden_folds(g, prefix):
    k, folds = 0, []
    while f"{prefix}fold{k}_train" in g:
        folds.append((g[f"{prefix}fold{k}_train"].astype(np.int64), g[f"{prefix}fold{k}_valid"].astype(np.int64)))
        k += 1
    return folds


def raw_traj_summary_ref(x, recent_hours):
    """x [B,T,2V] (values | counts) -> [B,V,14] float64, _summarize_one_variable (:329-405) with one row per hour."""
    x = np.asarray(x)
    B, T, C = x.shape
    V = C // 2
    assert 1 <= recent_hours <= T
    val, cnt = x[:, :, :V].astype(np.float64), x[:, :, V:].astype(np.float64)
    tt = np.arange(T, dtype=np.float64)[None, :, None]
    start = max(T - recent_hours, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        observed = np.isfinite(cnt) & (cnt > 0)
        valid = observed & np.isfinite(val)
        recent = np.broadcast_to(tt >= start, valid.shape)

        def seqsum(a):                        # hour by hour, as the reference's sorted-by-time arrays are
            s = np.zeros((B, V))
            for t in range(T):
                s = s + a[:, t]
            return s

        def wmean(sel, q):
            w = np.where(sel, cnt, 0.0)
            return seqsum(np.where(sel, cnt * q, 0.0)) / seqsum(w)          # 0 / 0 = NaN where nothing is selected

        def slope(sel):
            n = sel.sum(1)
            tm, ym = wmean(sel, np.broadcast_to(tt, val.shape)), wmean(sel, val)
            ct = tt - tm[:, None]
            den = seqsum(np.where(sel, cnt * (ct * ct), 0.0))
            num = seqsum(np.where(sel, cnt * ct * (val - ym[:, None]), 0.0))
            return np.where((n >= 2) & (den > 0), num / den, np.nan)

        n_valid = valid.sum(1)
        has = n_valid > 0
        first_t, last_t = valid.argmax(1), T - 1 - valid[:, ::-1].argmax(1)
        take = lambda idx: np.take_along_axis(val, idx[:, None, :], 1)[:, 0]  # noqa: E731
        first, last = np.where(has, take(first_t), np.nan), np.where(has, take(last_t), np.nan)
        mean = wmean(valid, val)
        std = np.sqrt(np.maximum(seqsum(np.where(valid, cnt * (val - mean[:, None]) ** 2, 0.0)) / seqsum(np.where(valid, cnt, 0.0)), 0.0))
        mn = np.where(has, np.where(valid, val, np.inf).min(1), np.nan)
        mx = np.where(has, np.where(valid, val, -np.inf).max(1), np.nan)
        delta = np.where(n_valid >= 2, last - first, np.nan)
        rv, ev = valid & recent, valid & ~recent
        shift = np.where(rv.any(1) & ev.any(1), wmean(rv, val) - wmean(ev, val), np.nan)
        n_obs = observed.sum(1)
        last_obs = T - 1 - observed[:, ::-1].argmax(1)
        since = np.where(n_obs > 0, np.maximum((T - 1) - last_obs, 0), T).astype(np.float64)
        ro = observed & recent
        out = np.stack([last, mean, std, mn, mx, delta, slope(valid), slope(rv), shift,
                        n_obs / T, np.log1p(np.maximum(seqsum(np.where(observed, cnt, 0.0)), 0.0)), since,
                        ro.sum(1) / max(T - start, 1), np.log1p(np.maximum(seqsum(np.where(ro, cnt, 0.0)), 0.0))], axis=-1)
    return out


def expit(s):
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def offset_logistic_valgrad_ref(X, y, offset, W, l2):
    """objective [G] and gradient [F,G] of _fit_offset_weights (:578-584) for the G columns of W."""
    X, W, l2 = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(l2, np.float64)
    y, offset = np.asarray(y, np.float64), np.asarray(offset, np.float64)
    s = offset[:, None] + X @ W
    obj = np.mean(np.logaddexp(0.0, s) - y[:, None] * s, axis=0) + 0.5 * l2 * np.sum(W * W, axis=0)
    grad = X.T @ (expit(s) - y[:, None]) / X.shape[0] + l2[None, :] * W
    return obj, grad


def binary_metrics_ref(y, p):
    """(BCE, AUROC, AUPRC) of _safe_metrics (:109-119): sklearn's tie-aware definitions.  Empty input: three NaN."""
    y = np.asarray(y).astype(np.int64)
    if y.size == 0:
        return np.full(3, np.nan)
    q = np.clip(np.asarray(p, np.float64), 1e-7, 1 - 1e-7)
    bce = float(np.mean(-np.where(y == 1, np.log(q), np.log(1.0 - q))))
    P, N = int(y.sum()), int(y.size - y.sum())
    if P == 0 or N == 0:
        return np.array([bce, np.nan, np.nan])
    order = np.argsort(q, kind="stable")
    qs = q[order]
    starts = np.flatnonzero(np.r_[True, qs[1:] != qs[:-1]])
    ends = np.r_[starts[1:], qs.size]
    ranks = np.empty(qs.size)
    for a, b in zip(starts, ends):
        ranks[a:b] = 0.5 * (a + 1 + b)                                   # tie-averaged 1-based ranks
    auroc = (ranks[y[order] == 1].sum() - P * (P + 1) / 2.0) / (P * N)
    yd = y[order][::-1]                                                  # descending score
    tp = np.cumsum(yd)
    last = np.flatnonzero(np.r_[qs[::-1][1:] != qs[::-1][:-1], True])    # last position of every distinct threshold
    tps = tp[last]
    recall, precision = tps / P, tps / (last + 1.0)
    auprc = float(np.sum(np.diff(np.r_[0.0, recall]) * precision))
    return np.array([bce, auroc, auprc])


def resampled_binary_metrics_ref(y, p, idx=None, offsets=None, R=None):
    """[R,3]: replicate r is y[idx[offsets[r]:offsets[r+1]]] against p[0 or r] at the same positions; idx None = identity."""
    p = np.atleast_2d(np.asarray(p, np.float64))
    R = (len(offsets) - 1 if idx is not None else p.shape[0]) if R is None else R
    out = np.empty((R, 3))
    for r in range(R):
        pr = p[0 if p.shape[0] == 1 else r]
        sel = np.arange(len(y)) if idx is None else np.asarray(idx[offsets[r]:offsets[r + 1]], np.int64)
        out[r] = binary_metrics_ref(np.asarray(y)[sel], pr[sel])
    return out
