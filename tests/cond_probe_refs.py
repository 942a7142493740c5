"""Numpy restatement of the conditional-information probe's device pieces (csrc/cond_probe.hip: moments, Newton terms, scores) and of
the damped Newton fit built on them, pinned on tests/golden/cond_probe.npz by tests/test_cond_probe_refs_cpu.py and compared with the
kernels by tests/test_gpu_cond_probe_kernels.py.  Written from the definitions (the issue text and sklearn's objective
C sum BCE + 0.5 w.w divided by C n), not from the kernels: dense matrix products, `np.logaddexp`, p (1 - p)."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_probe.npz")
FIT_NAMES = ("image_cal", "logit_add", "logit_interaction", "token_linear")
PROBE_NAMES = FIT_NAMES[1:]
GTOL = 1e-10

_cache = {}


def golden():
    """The fixture, loaded once and shared (read-only) by every test that needs it."""
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
        for v in _cache["g"].values():
            v.setflags(write=False)
    return _cache["g"]


def split_of(g, split):
    return {k: g[f"{split}_{k}"] for k in ("img", "ts", "fus", "token", "y", "mask")}


def features(probe, img, ts, token):
    """`_features` (:288-308) on one label's fp32 columns, widened to float64 (the product is taken in fp32 first)."""
    img, ts = np.asarray(img, np.float32).reshape(-1), np.asarray(ts, np.float32).reshape(-1)
    cols = {"image_cal": [img], "logit_add": [img, ts], "logit_interaction": [img, ts, img * ts],
            "token_linear": [img] + list(np.asarray(token, np.float32).T)}[probe]
    return np.column_stack(cols).astype(np.float64)


def expit(s):
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def moments_ref(X):
    """X [n, F] -> (mean, scale): population variance, centred; a constant column keeps scale 1 (StandardScaler's test)."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    mean = X.sum(0) / n
    var = ((X - mean) ** 2).sum(0) / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    return mean, np.where(constant, 1.0, np.sqrt(var))


def terms_ref(X, y, theta, mean, scale, l2):
    """theta [F + 1] (intercept last) -> (f, g [F + 1], H [F + 1, F + 1]) of mean BCE + 0.5 l2 w.w, intercept unpenalised."""
    X, y, theta = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(theta, np.float64)
    n, F = X.shape
    A = np.column_stack([(X - mean) / scale, np.ones(n)])
    s = A @ theta
    p = expit(s)
    pen = np.r_[np.ones(F), 0.0]
    f = np.mean(np.logaddexp(0.0, s) - y * s) + 0.5 * l2 * np.sum(pen * theta * theta)
    g = A.T @ (p - y) / n + l2 * pen * theta
    H = (A * (p * (1.0 - p))[:, None]).T @ A / n + l2 * np.diag(pen)
    return f, g, H


def scores_ref(X, theta, mean, scale, j0, j1, intercept):
    A = (np.asarray(X, np.float64) - mean) / scale
    return A[:, j0:j1] @ np.asarray(theta)[j0:j1] + (theta[-1] if intercept else 0.0)


def pad_terms(f, g, H, F, Fmax):
    """The kernel's padded layout: entries [F, Fmax) zero with 1 on H's diagonal, the intercept at index Fmax."""
    S = Fmax + 1
    src = np.r_[np.arange(F), Fmax]
    gp, Hp = np.zeros(S), np.zeros((S, S))
    gp[src] = g
    Hp[np.ix_(src, src)] = H
    pad = np.arange(F, Fmax)
    Hp[pad, pad] = 1.0
    return f, gp, Hp


def newton_fit_ref(X, y, C, max_iter=50):
    """Damped Newton on the objective of Pipeline(StandardScaler, LogisticRegression(C)) -> dict(mean, scale, coef, intercept,
    n_iter, gmax).  Stops at max|gradient| <= 1e-10; halves the step until the objective does not rise."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    if len(np.unique(y)) < 2:
        raise ValueError("Probe-training labels contain only one class")
    n, F = X.shape
    mean, scale = moments_ref(X)
    l2 = 1.0 / (C * n)
    theta = np.zeros(F + 1)
    f, g, H = terms_ref(X, y, theta, mean, scale, l2)
    it = 0
    while np.abs(g).max() > GTOL:
        if it >= max_iter:
            raise RuntimeError(f"no convergence after max_iter = {max_iter}")
        step = np.linalg.solve(H, -g)
        t = 1.0
        while True:
            ft, gt, Ht = terms_ref(X, y, theta + t * step, mean, scale, l2)
            if ft <= f + 1e-4 * t * (g @ step) + 8 * np.finfo(np.float64).eps * abs(f) or t < 1e-12:
                break
            t *= 0.5
        theta, f, g, H = theta + t * step, ft, gt, Ht
        it += 1
    return {"mean": mean, "scale": scale, "coef": theta[:F], "intercept": float(theta[F]), "n_iter": it, "gmax": float(np.abs(g).max())}


def fit_bound(g, k, probe):
    """The issue's bound on |parameter - T's|: 10 ||H^-1||_2 (1e-10 + max|g_T|), from the values the fixture stores per fit."""
    return 10.0 * float(g[f"T_{k}_{probe}_hinv"]) * (1e-10 + float(g[f"T_{k}_{probe}_gmax"]))


def draw_bootstrap_ref(n, n_bootstrap, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n, size=n) for _ in range(n_bootstrap)])
