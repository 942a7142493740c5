"""numpy restatement of the linear-head probes' training loop (a test helper, like cond_probe_refs.py): minibatch AdamW on
z = (x o mask) W^T + b with the masked BCE of the reference (vc = the number of known labels of the WHOLE minibatch; a minibatch with
none still takes its AdamW step with zero gradients), torch.optim.AdamW's update on W and b, and the per-epoch validation logits /
macro AUROC.  `dtype` float64 is the yardstick T of the tests; float32 is the same loop in the device's storage precision, whose
distance to T measures the rounding noise a case carries.  `defect` plants one wrong formula (the golden generator proves that each
moves the result far beyond that noise)."""
from __future__ import annotations

import numpy as np

DEFECTS = ("no_wd", "no_bias_wd", "no_bias_correction", "vc_per_label", "eps_in_sqrt")


def forward(x, W, b, label_width=0):
    """x [n, F], W [L, F] or [L, w] -> logits [n, L] in x's dtype."""
    if label_width:
        L = W.shape[0]
        return (x.reshape(x.shape[0], L, label_width) * W[None]).sum(-1) + b
    return x @ W.T + b


def sigmoid32(z):
    """The reference's evaluation: 1 / (1 + exp(-z)) in fp32 on the fp32 logits."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-z))).astype(np.float32)


def auroc(y, s):
    """Tie-aware AUROC (average ranks), what sklearn's roc_auc_score gives; NaN with fewer than two rows or one class."""
    y = np.asarray(y) > 0.5
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    _, inv, cnt = np.unique(np.asarray(s), return_inverse=True, return_counts=True)
    ends = np.cumsum(cnt)
    rank = (ends - (cnt - 1) / 2.0)[inv]
    return float((rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def macro_auroc(logits, Y, M):
    """Mean over the labels whose AUROC is defined, of the AUROC of the fp32 sigmoid over the label's known rows."""
    p = sigmoid32(logits)
    vals = []
    for l in range(Y.shape[1]):
        k = np.asarray(M[:, l]) > 0.5
        a = auroc(Y[k, l], p[k, l]) if k.sum() >= 2 else float("nan")
        if not np.isnan(a):
            vals.append(a)
    return float(np.mean(vals)) if vals else float("nan")


def train_ref(X, Y, M, W, b, perms, *, bs, lr, wd, betas=(0.9, 0.999), eps=1e-8, label_width=0, dtype=np.float64, mask_fn=None,
              state=None, defect=None, val=None):
    """perms [E, >= S bs] (S = N // bs).  mask_fn(t, bs, F) -> the fp32 dropout factors [bs, F] of step number t (1-based), or None.
    state: (mW, vW, mb, vb, t) to continue from.  val = (X_va, Y_va, M_va): per-epoch logits and macro AUROC.
    Returns a dict: W, b, state, loss_sum / valid_sum [E] (sum of loss * vc, sum of vc), val_logits [E, n, L], curve [E]."""
    assert defect is None or defect in DEFECTS
    dt = np.dtype(dtype).type
    X, Y, M = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype), np.asarray(M, dtype=dtype)
    W, b = np.array(W, dtype=dtype), np.array(b, dtype=dtype)
    L, F, N = b.size, X.shape[1], X.shape[0]
    if state is None:
        mW, vW, mb, vb, t = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b), 0
    else:
        mW, vW, mb, vb = (np.array(a, dtype=dtype) for a in state[:4])
        t = int(state[4])
    S = N // bs
    b1, b2 = betas
    loss_sum, valid_sum, val_logits, curve = [], [], [], []

    def adam(p, m, v, g, decay):
        p *= dt(1.0 - lr * wd) if decay else dt(1.0)
        m += dt(1.0 - b1) * (g - m)
        v *= dt(b2)
        v += dt(1.0 - b2) * g * g
        bc1, bc2 = (1.0, 1.0) if defect == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
        if defect == "eps_in_sqrt":
            denom = np.sqrt(v / dt(bc2) + dt(eps))
        else:
            denom = np.sqrt(v) / dt(np.sqrt(bc2)) + dt(eps)
        p += dt(-(lr / bc1)) * m / denom

    for perm in np.asarray(perms):
        run_l = run_v = 0.0
        for s in range(S):
            t += 1
            rows = np.asarray(perm[s * bs:(s + 1) * bs], dtype=np.int64)
            x, y, m = X[rows], Y[rows], M[rows]
            if mask_fn is not None:
                mk = mask_fn(t, bs, F)
                if mk is not None:
                    x = (x.astype(np.float32) * mk).astype(dtype) if dtype == np.float32 else x * mk.astype(dtype)
            z = forward(x, W, b, label_width)
            vc = m.sum()
            sg = np.where(z >= 0, 1 / (1 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1 + np.exp(-np.abs(z)))).astype(dtype)
            bce = np.maximum(z, 0) - y * z + np.log1p(np.exp(-np.abs(z)))
            if vc > 0:
                div = np.maximum(m.sum(0, keepdims=True), 1) if defect == "vc_per_label" else vc
                g = ((sg - y) * m / div).astype(dtype)
                loss = float((bce * m).sum() / vc)
                run_l += loss * float(vc)
                run_v += float(vc)
            else:
                g = np.zeros_like(z)
            if label_width:
                gW = (g[:, :, None] * x.reshape(bs, L, label_width)).sum(0).astype(dtype)
            else:
                gW = (g.T @ x).astype(dtype)
            gb = g.sum(0).astype(dtype)
            adam(W, mW, vW, gW, defect != "no_wd")
            adam(b, mb, vb, gb, defect not in ("no_wd", "no_bias_wd"))
        loss_sum.append(run_l)
        valid_sum.append(run_v)
        if val is not None:
            zv = forward(np.asarray(val[0], dtype=dtype), W, b, label_width)
            val_logits.append(zv)
            curve.append(macro_auroc(zv, val[1], val[2]))
    return {"W": W, "b": b, "state": (mW, vW, mb, vb, t), "loss_sum": np.array(loss_sum), "valid_sum": np.array(valid_sum),
            "val_logits": np.array(val_logits), "curve": np.array(curve)}


def best_epoch(curve):
    """The reference's selection: strict `>` against the running best, NaN never wins; 1-based, -1 when nothing is defined."""
    best, at = -float("inf"), -1
    for e, v in enumerate(curve):
        if v > best:
            best, at = v, e + 1
    return at
