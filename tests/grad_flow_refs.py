"""fp64 numpy replica of the gradient-flow kernels (csrc/grad_flow.hip; layouts in include/medp_hip.h): `seeds`, `accumulate`,
`report`, `query_geometry`.  Plain loops and numpy sums, no attempt to mirror the kernels' summation order: the kernel tests allow
1e-10, the expected difference of two fp64 orders over <= 1e5 fp32 products is <~ 1e-11."""
from __future__ import annotations

import numpy as np

REPORT_HEAD, REPORT_PER_LABEL = 26, 16
F8 = np.float64


def state_size(K, D):
    return 3 * K * K * D + 11 + 5 * K


def new_state(K, D):
    return np.zeros(state_size(K, D), dtype=F8)


def _cosine(xy, xx, yy):
    den = np.sqrt(xx) * np.sqrt(yy)
    return 0.0 if den <= 1e-12 else float(xy / max(den, 1e-12))


def _softplus_neg(l):
    return np.maximum(-l, 0.0) + np.log1p(np.exp(-np.abs(l)))


def seeds(img, ts, fus, y, mask, lw, pw, eps):
    """-> (losses [3, K], cot_img [B, K, K], cot_ts [B, 2K, K], cot_fus [B, 2K, K]) in fp64 from the fp32 inputs."""
    logits = [np.asarray(a, dtype=F8) for a in (img, ts, fus)]
    y, mask, lw = np.asarray(y, dtype=F8), np.asarray(mask, dtype=F8), np.asarray(lw, dtype=F8)
    B, K = y.shape
    pw = np.ones(K) if pw is None else np.asarray(pw, dtype=F8)
    den = mask.sum(0) + F8(np.float32(eps))
    losses = np.zeros((3, K))
    g = np.zeros((3, B, K))
    for r, l in enumerate(logits):
        coef = 1.0 + (pw[None] - 1.0) * y
        bce = (1.0 - y) * l + coef * _softplus_neg(l)
        losses[r] = lw * ((bce * mask).sum(0) / den)
        sig = 1.0 / (1.0 + np.exp(-l))
        g[r] = lw[None] * mask / den[None] * ((1.0 - y) - coef * (1.0 - sig))
    cot_img = np.zeros((B, K, K))
    cot_ts, cot_fus = np.zeros((B, 2 * K, K)), np.zeros((B, 2 * K, K))
    for k in range(K):
        cot_img[:, k, k] = g[0][:, k]
        cot_ts[:, k, k] = g[1][:, k]
        cot_fus[:, K + k, k] = g[2][:, k]
    return losses, cot_img, cot_ts, cot_fus


def accumulate(state, dq, dI, dT, I, T, mask, losses):
    """One batch into `state` (in place)."""
    dq, dT, I, T = (np.asarray(a, dtype=F8) for a in (dq, dT, I, T))
    mask, losses = np.asarray(mask, dtype=F8), np.asarray(losses, dtype=F8)
    B, K, D = T.shape
    n = 3 * K * K * D
    state[:n] += dq.reshape(-1)
    state[n:n + 3] += losses.reshape(3, K).sum(1)
    a, b = dq[0].sum(0).reshape(-1), dq[1].sum(0).reshape(-1)
    c = _cosine(a @ b, a @ a, b @ b)
    state[n + 3] += c
    state[n + 4] += 1.0 if c < 0 else 0.0
    state[n + 5] += 1.0
    state[n + 6] += B
    state[n + 7:n + 7 + K] += mask.sum(0)
    sens = state[n + 7 + K:n + 11 + K]
    sens_label = state[n + 11 + K:n + 11 + 5 * K].reshape(4, K)
    for m, (g, tok) in enumerate(((dI, I), (dT, T))):
        if g is None:
            continue
        g = np.asarray(g, dtype=F8).reshape(B, K, K * D)
        tok_norm = np.sqrt((tok.reshape(B, -1) ** 2).sum(1))
        total = np.sqrt((g.sum(1) ** 2).sum(1))
        sens[m] += total.sum()
        sens[2 + m] += (total * tok_norm).sum()
        for k in range(K):
            gn = np.sqrt((g[:, k] ** 2).sum(1))
            sens_label[m, k] += gn.sum()
            sens_label[2 + m, k] += (gn * tok_norm).sum()
    return state


def report(state, alphas, K, D):
    """-> the report vector [REPORT_HEAD + REPORT_PER_LABEL K]."""
    n = 3 * K * K * D
    pl = state[:n].reshape(3, K, K * D)
    loss, scal = state[n:n + 3], state[n + 3:n + 7]
    valid, sens = state[n + 7:n + 7 + K], state[n + 7 + K:n + 11 + K]
    sens_label = state[n + 11 + K:n + 11 + 5 * K].reshape(4, K)
    alphas = np.asarray(alphas, dtype=F8)
    nb, ns = max(scal[2], 1.0), max(scal[3], 1.0)
    out = np.zeros(REPORT_HEAD + REPORT_PER_LABEL * K)
    mean = pl.sum(1) / nb
    total = (alphas[:, None] * mean).sum(0)
    for r in range(3):
        w = alphas[r] * mean[r]
        out[4 * r:4 * r + 4] = (loss[r] / nb, np.sqrt(mean[r] @ mean[r]), np.sqrt(w @ w), _cosine(w @ total, w @ w, total @ total))
    for i, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        out[12 + i] = _cosine(mean[a] @ mean[b], mean[a] @ mean[a], mean[b] @ mean[b])
    out[15], out[16] = scal[0] / nb, scal[1] / nb
    out[17] = out[2] / max(out[6], 1e-12)
    out[18:22] = sens / ns
    out[22], out[23] = out[18] / max(out[19], 1e-12), out[20] / max(out[21], 1e-12)
    out[24], out[25] = scal[2], scal[3]
    for k in range(K):
        o = out[REPORT_HEAD + REPORT_PER_LABEL * k:REPORT_HEAD + REPORT_PER_LABEL * (k + 1)]
        g = pl[:, k] / nb
        t = (alphas[:, None] * g).sum(0)
        o[0] = valid[k]
        for r in range(3):
            o[1 + r] = np.sqrt(g[r] @ g[r])
            own = g[r].reshape(K, D)[k]
            o[8 + r] = np.sqrt(own @ own) / max(o[1 + r], 1e-12)
        for i, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
            o[4 + i] = _cosine(g[a] @ g[b], g[a] @ g[a], g[b] @ g[b])
        o[7] = np.sqrt(t @ t)
        o[11:15] = sens_label[:, k] / max(valid[k], 1.0)
        o[15] = o[13] / max(o[14], 1e-12)
    return out


def query_geometry(rows):
    """rows [3, K, D] -> [3 K K + K + 1]: Gram matrices of the normalised rows, prototype norms, ||G_img - G_ts||_F / K."""
    rows = np.asarray(rows, dtype=F8)
    _, K, _ = rows.shape
    norms = np.sqrt((rows ** 2).sum(-1))
    unit = rows / np.maximum(norms, 1e-12)[..., None]
    gram = np.einsum("sid,sjd->sij", unit, unit)
    gap = np.sqrt(((gram[1] - gram[2]) ** 2).sum()) / K
    return np.concatenate([gram.reshape(-1), norms[0], [gap]])


# ---- comparing two report dictionaries ------------------------------------------------------------------------------------------
ABSOLUTE_CLASSES, RELATIVE_CLASSES = ("loss", "norm", "cos", "fraction"), ("ratio",)


def _class_of(path):
    leaf = [p for p in path if isinstance(p, str)][-1]
    if "query_geometry" in path:
        return "norm" if leaf == "prototype_norms" else "cos"
    if leaf.endswith("_over_ts"):
        return "ratio"
    if "fraction" in leaf:
        return "fraction"
    if "cos" in leaf or path[0] == "pairwise_gradient_cosine":
        return "cos"
    if leaf == "loss":
        return "loss"
    return "norm"                                               # gradient norms and token sensitivities


def _walk(got, want, path, out):
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (path, list(got), list(want))
        for key in want:
            _walk(got[key], want[key], path + (key,), out)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _walk(g, w, path + (i,), out)
    elif isinstance(want, (str, int)) and not isinstance(want, bool):
        assert type(got) is type(want) and got == want, (path, got, want)
    else:
        assert isinstance(got, float) and isinstance(want, float), (path, type(got), type(want))
        if path[-1] == "alpha":
            assert got == want, path
            return
        cls = _class_of(path)
        err = abs(got - want)
        a, r = out.setdefault(cls, (0.0, 0.0))
        out[cls] = (max(a, err), max(r, err / max(abs(want), 1e-300) if want != 0.0 else (0.0 if err == 0.0 else float("inf"))))


def compare_reports(got, want):
    """Same keys in the same order, same types, equal strings / integers / alphas; -> {class: (worst absolute, worst relative
    deviation)} over the floats, classes "loss", "norm" (gradient norms, sensitivities, prototype norms), "cos" (cosines, Gram
    entries, the Gram gap), "fraction" (own-row and negative-batch fractions), "ratio" (the *_over_ts values)."""
    out = {}
    _walk(got, want, (), out)
    return out
