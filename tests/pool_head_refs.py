"""numpy restatement of the two probe heads with a hidden stage (a test helper, like head_probe_refs.py): the attention-pooled head
`LinearHead(use_attn_pool=True)` and the MLP fusion head `LogitFusionHead("mlp")`, each with its forward, its ANALYTIC backward, the
masked BCE of the reference (vc = the known labels of the whole minibatch; a minibatch with none still takes its AdamW step with zero
gradients), torch.optim.AdamW on every parameter tensor and the per-epoch validation logits / macro AUROC.  `dtype` float64 is the
yardstick T of the tests; float32 is the same loop in the device's storage precision, whose distance to T measures the rounding
noise a case carries.  `defect` plants one wrong formula (the golden generator proves that each moves the result far beyond that
noise)."""
from __future__ import annotations

import numpy as np
import torch

from head_probe_refs import macro_auroc

POOL_DEFECTS = ("no_sqrt_d", "no_centring", "no_query_wd")
MLP_DEFECTS = ("tanh_gelu", "gelu_grad_no_pdf")
POOL_KEYS = ("attn_query", "head.1.weight", "head.1.bias")
MLP_KEYS = ("head.0.weight", "head.0.bias", "head.3.weight", "head.3.bias")


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


# ---- attention-pooled head ------------------------------------------------------------------------------------------------------
def pool_forward(x, P, mask=None, defect=None):
    """x [n, T, d]; P: {attn_query [d], head.1.weight [L, d], head.1.bias [L]} -> (logits [n, L], cache for the backward)."""
    dt = x.dtype.type
    s = x @ P["attn_query"]
    scale = dt(1.0) if defect == "no_sqrt_d" else dt(1.0) / np.sqrt(dt(x.shape[-1]))
    s = s * scale
    e = np.exp(s - s.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    pooled = (w[:, :, None] * x).sum(axis=1)
    pm = pooled if mask is None else pooled * mask.astype(x.dtype)
    z = pm @ P["head.1.weight"].T + P["head.1.bias"]
    return z.astype(x.dtype), (x, w, pm, mask, scale)


def pool_backward(g, P, cache, defect=None):
    """g = d loss / d logits [n, L] -> the gradients of the three parameter tensors."""
    x, w, pm, mask, scale = cache
    dp = g @ P["head.1.weight"]
    if mask is not None:
        dp = dp * mask.astype(x.dtype)
    dw = np.einsum("bj,btj->bt", dp, x)
    if defect != "no_centring":
        dw = dw - (w * dw).sum(axis=1, keepdims=True)
    ds = w * dw * scale
    return {"attn_query": np.einsum("bt,btj->j", ds, x).astype(x.dtype), "head.1.weight": (g.T @ pm).astype(x.dtype),
            "head.1.bias": g.sum(axis=0).astype(x.dtype)}


# ---- MLP fusion head ------------------------------------------------------------------------------------------------------------
def _gelu(a, defect):
    dt = a.dtype.type
    if defect == "tanh_gelu":
        u = dt(np.sqrt(2.0 / np.pi)) * (a + dt(0.044715) * a ** 3)
        th = np.tanh(u)
        return dt(0.5) * a * (dt(1) + th), dt(0.5) * (dt(1) + th) + dt(0.5) * a * (dt(1) - th * th) * dt(np.sqrt(2.0 / np.pi)) * (
            dt(1) + dt(3 * 0.044715) * a * a)
    cdf = dt(0.5) * (dt(1) + _erf(a * dt(np.sqrt(0.5))))
    pdf = np.exp(-dt(0.5) * a * a) * dt(1.0 / np.sqrt(2.0 * np.pi))
    return a * cdf, (cdf if defect == "gelu_grad_no_pdf" else cdf + a * pdf)


def mlp_forward(x, P, mask=None, defect=None):
    """x [n, K]; P: {head.0.weight [H, K], head.0.bias [H], head.3.weight [L, H], head.3.bias [L]} -> (logits [n, L], cache)."""
    a = (x @ P["head.0.weight"].T + P["head.0.bias"]).astype(x.dtype)
    h, dh = _gelu(a, defect)
    hm = h if mask is None else h * mask.astype(x.dtype)
    z = hm @ P["head.3.weight"].T + P["head.3.bias"]
    return z.astype(x.dtype), (x, hm.astype(x.dtype), dh.astype(x.dtype), mask)


def mlp_backward(g, P, cache, defect=None):
    x, hm, dgelu, mask = cache
    dh = g @ P["head.3.weight"]
    if mask is not None:
        dh = dh * mask.astype(x.dtype)
    da = (dh * dgelu).astype(x.dtype)
    return {"head.0.weight": (da.T @ x).astype(x.dtype), "head.0.bias": da.sum(axis=0).astype(x.dtype),
            "head.3.weight": (g.T @ hm).astype(x.dtype), "head.3.bias": g.sum(axis=0).astype(x.dtype)}


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def bce_grad(z, y, m):
    """(g = d loss / d z, loss, vc) of the masked BCE; zeros when no label of the minibatch is known."""
    vc = m.sum()
    ez = np.exp(-np.abs(z))
    sg = np.where(z >= 0, 1 / (1 + ez), ez / (1 + ez)).astype(z.dtype)
    if vc > 0:
        bce = np.maximum(z, 0) - y * z + np.log1p(ez)
        return ((sg - y) * m / vc).astype(z.dtype), float((bce * m).sum() / vc), float(vc)
    return np.zeros_like(z), 0.0, 0.0


def _train(kind, X, Y, M, params, perms, *, bs, lr, wd, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64, mask_fn=None, state=None,
           defect=None, val=None):
    fwd, bwd, width = (pool_forward, pool_backward, lambda x: x.shape[-1]) if kind == "pool" else (
        mlp_forward, mlp_backward, lambda x: params["head.0.bias"].size)
    assert defect is None or defect in (POOL_DEFECTS if kind == "pool" else MLP_DEFECTS)
    dt = np.dtype(dtype).type
    X, Y, M = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype), np.asarray(M, dtype=dtype)
    P = {k: np.array(v, dtype=dtype) for k, v in params.items()}
    if state is None:
        m1, m2, t = {k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}, 0
    else:
        m1, m2 = ({k: np.array(v, dtype=dtype) for k, v in s.items()} for s in state[:2])
        t = int(state[2])
    S = X.shape[0] // bs
    b1, b2 = betas
    loss_sum, valid_sum, val_logits, curve = [], [], [], []
    for perm in np.asarray(perms):
        run_l = run_v = 0.0
        for s in range(S):
            t += 1
            rows = np.asarray(perm[s * bs:(s + 1) * bs], dtype=np.int64)
            x, y, m = X[rows], Y[rows], M[rows]
            mk = mask_fn(t, bs, width(x)) if mask_fn is not None else None
            z, cache = fwd(x, P, mk, defect)
            g, loss, vc = bce_grad(z, y, m)
            run_l += loss * vc
            run_v += vc
            G = bwd(g, P, cache, defect)
            for k in P:
                decay = not (defect == "no_query_wd" and k == "attn_query")
                P[k] *= dt(1.0 - lr * wd) if decay else dt(1.0)
                m1[k] += dt(1.0 - b1) * (G[k] - m1[k])
                m2[k] *= dt(b2)
                m2[k] += dt(1.0 - b2) * G[k] * G[k]
                denom = np.sqrt(m2[k]) / dt(np.sqrt(1.0 - b2 ** t)) + dt(eps)
                P[k] += dt(-(lr / (1.0 - b1 ** t))) * m1[k] / denom
        loss_sum.append(run_l)
        valid_sum.append(run_v)
        if val is not None:
            zv = fwd(np.asarray(val[0], dtype=dtype), P, None, defect)[0]
            val_logits.append(zv)
            curve.append(macro_auroc(zv, val[1], val[2]))
    return {"params": P, "state": (m1, m2, t), "loss_sum": np.array(loss_sum), "valid_sum": np.array(valid_sum),
            "val_logits": np.array(val_logits), "curve": np.array(curve)}


def train_pool_ref(X, Y, M, params, perms, **kw):
    """X [N, T, d]; params: {attn_query, head.1.weight, head.1.bias}; perms [E, >= S bs].  mask_fn(t, bs, d) -> the fp32 dropout factors
    [bs, d] of step number t (1-based), or None.  state: (first moments, second moments, t) to continue from.  Returns a dict:
    params, state, loss_sum / valid_sum [E], val_logits [E, n, L] and curve [E] when val = (X_va, Y_va, M_va) is given."""
    return _train("pool", X, Y, M, params, perms, **kw)


def train_mlp_ref(X, Y, M, params, perms, **kw):
    """X [N, K] = cat(img, ts); params: {head.0.weight, head.0.bias, head.3.weight, head.3.bias}; mask_fn(t, bs, H) masks the hidden units."""
    return _train("mlp", X, Y, M, params, perms, **kw)


def param_gap(A: dict, B: dict) -> float:
    return max(float(np.abs(np.asarray(A[k], dtype=np.float64).reshape(np.shape(B[k])) - np.asarray(B[k], dtype=np.float64)).max()) for k in B)
