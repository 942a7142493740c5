"""Minibatch AdamW on linear heads over frozen features, on the HIP kernels of csrc/head_probe.hip: the trainer behind
`unimodal_linear_probe.train_linear_head` and `logit_fusion_probe.train_fusion_head` (DESIGN.md "Linear-head probes").

One `medp_head_train_epoch` launch runs every sequential step of an epoch for P independent heads (one workgroup each); the
per-epoch selection on validation macro AUROC stays on the device (`medp_head_scores`, `probe_stats.LabelMetrics`, a few
elementwise torch ops), so a run of E epochs has no device->host copy and no synchronisation until its single copy at the end.

What runs where
  device, HIP   the steps (gather through the permutation, dropout, logits, masked BCE gradient, AdamW on W and b), the scores of
                the validation rows, AUROC / AUPRC / BCE per label.
  device, torch macro AUROC = mean over the labels whose AUROC is not NaN, the strict `>` against the running best and the
                conditional copy of (W, b) into the best slot.
  host          the initial parameters (torch's default CPU generator, the reference's order), every epoch's permutation in the
                DataLoader's draw order, the problem tables (validated before the first launch).
`eager_fit` is the reference's loop through torch autograd for the heads no kernel covers (learned attention pooling, the MLP
fusion head): the same selection rule, NOT accelerated.  Without a GPU every entry point raises (no CPU fallback)."""
from __future__ import annotations

from typing import Callable, Sequence

import numpy as np
import torch

from .abi import MedpHeadProblem, check, fp32_matrix, lib, ptr, require_gpu, stream, table_bytes
from .probe_stats import LabelMetrics, nan_mean

MAX_F, MAX_L, MAX_BS = 32768, 16, 1024          # MEDP_HEAD_MAX_*
BETAS, EPS = (0.9, 0.999), 1e-8                 # torch.optim.AdamW's defaults, which the reference takes


# ------------------------------------------------------------------------------------------------------------------------------
# host draws
# ------------------------------------------------------------------------------------------------------------------------------
def draw_epoch_permutations(n: int, epochs: int) -> np.ndarray:
    """[epochs, n] int32: the row orders `DataLoader(shuffle=True)` visits in `epochs` passes, drawn from torch's default CPU
    generator in the loader's own order.  Per epoch: one int64 `random_()` (the iterator's base seed), one more (the
    RandomSampler's seed), then `randperm(n)` from a private generator seeded with the latter (the sampler's second randperm, for
    the empty remainder, comes from that private generator too and leaves the default one alone)."""
    out = np.empty((epochs, n), dtype=np.int32)
    for e in range(epochs):
        torch.empty((), dtype=torch.int64).random_()
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        out[e] = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
def onchip(F: int, L: int, label_width: int, bs: int) -> bool:
    """True when W and both Adam moments of such a problem live in LDS for the epoch."""
    return bool(lib().medp_head_train_onchip(int(F), int(L), int(label_width), int(bs)))


class HeadProblem:
    """One head: z = (x o dropout) W^T + b over the columns [col0, col0 + F) of X.  `label_width` = 0: W [L, F]; w > 0: label l reads
    columns [l w, (l+1) w) and W is [L, w].  Parameters, Adam moments and the step count live on the device."""

    def __init__(self, X, Y, M, W, b, *, col0: int = 0, F: int | None = None, label_width: int = 0, bs: int = 128, lr: float = 1e-4,
                 weight_decay: float = 1e-4, dropout: float = 0.0, seed: int = 0, stream_id: int = 0, betas=BETAS, eps: float = EPS):
        self.X, self.N, self.ldx = fp32_matrix(X, "X")
        self.Y, ny, self.ldy = fp32_matrix(Y, "Y")
        self.M, nm, ldm = fp32_matrix(M, "M")
        if ny != self.N or nm != self.N or ldm != self.ldy:
            raise ValueError(f"HeadProblem: X has {self.N} rows, Y {ny} x {self.ldy}, M {nm} x {ldm}")
        dev = self.X.device
        self.W = W.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        self.b = b.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        self.L = int(self.b.numel())
        self.label_width = int(label_width)
        self.col0 = int(col0)
        self.F = int(F) if F is not None else (self.ldx - self.col0)
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb, self.vb = torch.zeros_like(self.b), torch.zeros_like(self.b)
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.bs, self.S = int(bs), self.N // max(int(bs), 1)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.dropout, self.seed, self.stream_id = float(dropout), int(seed) & 0xFFFFFFFF, int(stream_id) & 0xFFFFFFFF
        expect = self.L * (self.label_width if self.label_width > 0 else self.F)
        if self.W.numel() != expect:
            raise ValueError(f"HeadProblem: W has {self.W.numel()} elements, L={self.L}, F={self.F}, label_width={self.label_width} need {expect}")

    def entry(self, perm: torch.Tensor | None, loss_out: torch.Tensor | None) -> MedpHeadProblem:
        return MedpHeadProblem(ptr(self.X), ptr(self.Y), ptr(self.M), ptr(self.W), ptr(self.b), ptr(self.mW), ptr(self.vW), ptr(self.mb),
                               ptr(self.vb), ptr(self.t), ptr(perm), ptr(loss_out), self.ldx, self.N, self.ldy, self.col0, self.F, self.L,
                               self.label_width, self.bs, self.S, self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps,
                               self.dropout, self.seed, self.stream_id, 0)


def make_table(entries: Sequence[MedpHeadProblem]):
    """(host ctypes array, the same bytes as a uint8 numpy array)."""
    host = (MedpHeadProblem * max(len(entries), 1))(*entries)
    return host, table_bytes(host, len(entries))


def check_table(entries: Sequence[MedpHeadProblem]) -> None:
    """The library's host-side validation alone (needs no GPU).  Nothing is launched: the device table is null, which the library
    reports last, so a table that passes every other check raises ValueError('... null device table')."""
    host, _ = make_table(entries)
    check(lib().medp_head_train_epoch(host, None, len(entries), None), "head_train_epoch")


def head_train_epoch(problems: Sequence[HeadProblem], perms: Sequence[torch.Tensor], loss_out: torch.Tensor | None = None) -> torch.Tensor:
    """One epoch of every problem in ONE launch.  perms[p]: int32 [S bs] on the device.  Returns loss_out [P, 2] fp64 =
    (sum over the steps of loss * vc, sum of vc); the parameters, moments and step counts of the problems are updated in place."""
    require_gpu()
    dev = problems[0].X.device
    if loss_out is None:
        loss_out = torch.empty((len(problems), 2), dtype=torch.float64, device=dev)
    for pb, perm in zip(problems, perms):
        if perm.dtype != torch.int32 or perm.numel() < pb.S * pb.bs or not perm.is_contiguous():
            raise ValueError("head_train_epoch: a permutation is a contiguous int32 tensor of at least S * bs entries")
    host, raw = make_table([pb.entry(perm, loss_out[p]) for p, (pb, perm) in enumerate(zip(problems, perms))])
    table_dev = torch.as_tensor(raw, device=dev)
    check(lib().medp_head_train_epoch(host, ptr(table_dev), len(problems), stream()), "head_train_epoch")
    return loss_out


def head_scores(X, W, b, *, col0: int = 0, F: int | None = None, label_width: int = 0, rows: torch.Tensor | None = None, logits=None,
                probs=None):
    """(logits [n, L] fp32, probs [L, n] fp64 = the fp32 sigmoid widened) of the rows `rows` (int32, device; None: all rows)."""
    require_gpu()
    X, N, ldx = fp32_matrix(X, "X")
    L = int(b.numel())
    F = ldx - col0 if F is None else F
    n = N if rows is None else int(rows.numel())
    if rows is not None and rows.dtype != torch.int32:
        raise TypeError("head_scores: rows are int32")
    if W.dtype != torch.float32 or b.dtype != torch.float32 or W.numel() != L * (label_width if label_width > 0 else F):
        raise ValueError("head_scores: W fp32 [L, F] (or [L, label_width]), b fp32 [L]")
    logits = torch.empty((n, L), dtype=torch.float32, device=X.device) if logits is None else logits
    probs = torch.empty((L, n), dtype=torch.float64, device=X.device) if probs is None else probs
    check(lib().medp_head_scores(ptr(X), ldx, N, int(col0), int(F), L, int(label_width), ptr(W.contiguous()), ptr(b.contiguous()), ptr(rows),
                                 n, ptr(logits), ptr(probs), stream()), "head_scores")
    return logits, probs


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------------------------------
def train_heads(problems: Sequence[HeadProblem], vals: Sequence[tuple], epochs: int, perms: Sequence[np.ndarray],
                record_val_logits: bool = False) -> list:
    """`epochs` epochs of every problem, one launch group per epoch, best-validation-macro-AUROC selection on the device.
    vals[p] = (X_va, Y_va, M_va) with the problem's column layout; perms[p]: [epochs, >= S bs] int host array.
    One result dict per problem: curve [E], loss_sum / valid_sum [E], best_epoch (1-based), best_val, best_W / best_b, and
    val_logits [E, n, L] when asked for.  Raises ValueError when no epoch has a defined macro AUROC, or a permutation was bad."""
    require_gpu()
    P, E = len(problems), int(epochs)
    dev = problems[0].X.device
    metrics = [LabelMetrics(v[1].to(dev), v[2].to(dev)) for v in vals]                 # raises before the first launch
    Xv = [fp32_matrix(v[0].to(dev), "X_va")[0] for v in vals]
    perm_dev = [torch.as_tensor(np.ascontiguousarray(np.asarray(pm)[:, :pb.S * pb.bs], dtype=np.int32), device=dev)
                for pb, pm in zip(problems, perms)]
    for pb, pd in zip(problems, perm_dev):
        if pd.shape != (E, pb.S * pb.bs):
            raise ValueError(f"train_heads: a problem needs [{E}, {pb.S * pb.bs}] permutation entries, got {tuple(pd.shape)}")
    losses = torch.zeros((E, P, 2), dtype=torch.float64, device=dev)
    # every epoch's table up front: the loop copies nothing to or from the device
    tables = [make_table([pb.entry(perm_dev[p][e], losses[e, p]) for p, pb in enumerate(problems)]) for e in range(E)]
    host0 = tables[0][0] if E else None
    if E:
        rc = lib().medp_head_train_epoch(host0, None, P, None)                         # validate; a null device table is never launched
        if rc != 0 and b"null device table" not in lib().medp_last_error():
            check(rc, "head_train_epoch")
    tables_dev = torch.as_tensor(np.stack([t[1] for t in tables]) if E else np.zeros((0, 1), np.uint8), device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    state = []
    for p, pb in enumerate(problems):
        n = Xv[p].shape[0]
        state.append({"curve": torch.full((E,), float("nan"), **f64), "best": torch.full((), -float("inf"), **f64),
                      "best_epoch": torch.full((), -1, dtype=torch.int64, device=dev), "best_W": pb.W.clone(), "best_b": pb.b.clone(),
                      "logits": torch.empty((E if record_val_logits else 1, n, pb.L), dtype=torch.float32, device=dev),
                      "probs": torch.empty((pb.L, n), **f64)})
    for e in range(E):
        check(lib().medp_head_train_epoch(tables[e][0], ptr(tables_dev[e]), P, stream()), "head_train_epoch")
        for p, pb in enumerate(problems):
            st = state[p]
            head_scores(Xv[p], pb.W, pb.b, col0=pb.col0, F=pb.F, label_width=pb.label_width,
                        logits=st["logits"][e if record_val_logits else 0], probs=st["probs"])
            macro = nan_mean(metrics[p](st["probs"])[:, 1])
            better = macro > st["best"]                                                # strict; NaN never wins
            st["best"] = torch.where(better, macro, st["best"])
            st["best_epoch"] = torch.where(better, torch.full_like(st["best_epoch"], e + 1), st["best_epoch"])
            st["best_W"] = torch.where(better, pb.W, st["best_W"])
            st["best_b"] = torch.where(better, pb.b, st["best_b"])
            st["curve"][e] = macro
    torch.cuda.synchronize(dev)
    losses_h = losses.cpu().numpy()
    out = []
    for p, pb in enumerate(problems):
        st = state[p]
        if np.isnan(losses_h[:, p]).any():
            raise ValueError(f"train_heads: problem {p} has a permutation entry outside [0, {pb.N})")
        best_epoch = int(st["best_epoch"].item())
        if best_epoch < 0:
            raise ValueError("no epoch has a defined validation macro AUROC: no label has two known validation rows of both classes")
        res = {"curve": st["curve"].cpu().numpy(), "loss_sum": losses_h[:, p, 0], "valid_sum": losses_h[:, p, 1], "best_epoch": best_epoch,
               "best_val": float(st["best"].item()), "best_W": st["best_W"], "best_b": st["best_b"]}
        if record_val_logits:
            res["val_logits"] = st["logits"].cpu().numpy()
        out.append(res)
    return out


def history_lines(result: dict, tag: str = "epoch") -> list:
    """The reference's per-epoch line, from a result of `train_heads` (printed after the run: the loop never synchronises)."""
    return [f"  {tag} {e + 1:>2d}  train_loss={result['loss_sum'][e] / max(result['valid_sum'][e], 1):.4f}  "
            f"val_macro_AUROC={result['curve'][e]:.4f}" for e in range(len(result["curve"]))]


# ------------------------------------------------------------------------------------------------------------------------------
# eager fallback (not accelerated)
# ------------------------------------------------------------------------------------------------------------------------------
def masked_bce_loss(logits: torch.Tensor, labels: torch.Tensor, label_mask: torch.Tensor) -> torch.Tensor:
    """Mean BCE-with-logits over the known labels of the batch; an all-unknown batch gives a zero that still has a graph."""
    per = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels, reduction="none")
    mf = label_mask.float()
    vc = mf.sum()
    if vc.item() == 0:
        return logits.sum() * 0.0
    return (per * mf).sum() / vc


def eager_fit(model: torch.nn.Module, forward: Callable, train: Sequence[torch.Tensor], Y_tr, M_tr, val: Sequence[torch.Tensor], Y_va, M_va,
              *, epochs: int, batch_size: int, lr: float, weight_decay: float, perms: np.ndarray) -> dict:
    """The reference's loop through torch autograd on the device, for the heads no kernel covers: `forward(model, *inputs)` gives the
    logits; minibatches follow `perms`; AdamW; per epoch the validation macro AUROC from the metrics kernel and the strict `>`
    selection.  Synchronises every step, as the reference does (`.item()`): this path is NOT accelerated."""
    require_gpu()
    dev = Y_tr.device
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
    metrics = LabelMetrics(Y_va, M_va)
    S = Y_tr.shape[0] // batch_size
    best_val, best_state, best_epoch = -float("inf"), None, -1
    curve, loss_sum, valid_sum = [], [], []
    for e in range(epochs):
        model.train()
        order = torch.as_tensor(np.asarray(perms[e][:S * batch_size], dtype=np.int64), device=dev)
        run_l = run_v = 0.0
        for s in range(S):
            rows = order[s * batch_size:(s + 1) * batch_size]
            opt.zero_grad(set_to_none=True)
            loss = masked_bce_loss(forward(model, *(t[rows] for t in train)), Y_tr[rows], M_tr[rows])
            loss.backward()
            opt.step()
            v = M_tr[rows].float().sum().item()
            run_l += loss.item() * v
            run_v += v
        model.eval()
        with torch.no_grad():
            z = forward(model, *val).float()
            probs = (1.0 / (1.0 + torch.exp(-z))).t().contiguous().double()
            macro = float(nan_mean(metrics(probs)[:, 1]).item())
        curve.append(macro)
        loss_sum.append(run_l)
        valid_sum.append(run_v)
        if macro > best_val:
            best_val, best_epoch = macro, e + 1
            best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if best_state is None:
        raise ValueError("no epoch has a defined validation macro AUROC: no label has two known validation rows of both classes")
    model.load_state_dict(best_state)
    return {"curve": np.array(curve), "loss_sum": np.array(loss_sum), "valid_sum": np.array(valid_sum), "best_epoch": best_epoch,
            "best_val": best_val}
