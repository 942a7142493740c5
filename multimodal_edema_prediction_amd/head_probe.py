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
The two heads with a hidden stage run on csrc/pool_head_probe.hip:
  attention pooling  `PoolHeadProblem`, `train_pool_head`: a step is two launches (a row kernel, one workgroup per minibatch row,
                and a column kernel that sums the rows in order and applies AdamW); `medp_pool_head_train_epoch` enqueues every step
                of an epoch from one call.  Python counts the steps (the kernels keep no device counter).
  MLP fusion    `MlpHeadProblem`, `train_mlp_heads`: every step of an epoch in one launch, a workgroup per problem, parameters,
                moments and activations in LDS.
The three problem classes share one base (`_Problem`: labels, minibatch grid, AdamW and dropout fields), the three scores wrappers
one buffer helper, and the three trainers one epoch loop (`_train`) and one selection rule (`BestSelection`): a trainer says how its
family launches an epoch and scores a problem, nothing else.  `eager_fit` is the reference's loop through torch autograd: the
fallback for a shape outside the kernels' limits, and the baseline the timing tool compares with.  Without a GPU every entry point
raises (no CPU fallback)."""
from __future__ import annotations

import ctypes
from typing import Callable, Sequence

import numpy as np
import torch

from .abi import (MedpHeadProblem, MedpMlpHeadProblem, MedpPoolHeadProblem, check, fp32_matrix, lib, ptr, require_gpu, stream,
                  table_bytes)
from .probe_stats import LabelMetrics, nan_mean

MAX_F, MAX_L, MAX_BS = 32768, 16, 1024          # MEDP_HEAD_MAX_*
MAX_T, MAX_K, MAX_H = 1024, 64, 1024            # MEDP_POOL_HEAD_MAX_T, MEDP_MLP_HEAD_MAX_K / _H
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


class _Problem:
    """What the three problems share, once `X` and `N` are set: the labels Y / M [N, >= L], the minibatch grid (bs, S), AdamW's
    hyper-parameters, the dropout stream, and `own`, the device copy of an initial parameter."""

    def __init__(self, Y, M, bs, lr, weight_decay, dropout, seed, stream_id, betas, eps):
        self.Y, ny, self.ldy = fp32_matrix(Y, "Y")
        self.M, nm, ldm = fp32_matrix(M, "M")
        if ny != self.N or nm != self.N or ldm != self.ldy:
            raise ValueError(f"{type(self).__name__}: X has {self.N} rows, Y {ny} x {self.ldy}, M {nm} x {ldm}")
        self.bs, self.S = int(bs), self.N // max(int(bs), 1)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.dropout, self.seed, self.stream_id = float(dropout), int(seed) & 0xFFFFFFFF, int(stream_id) & 0xFFFFFFFF

    def own(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.X.device, dtype=torch.float32).contiguous().clone()


class HeadProblem(_Problem):
    """One head: z = (x o dropout) W^T + b over the columns [col0, col0 + F) of X.  `label_width` = 0: W [L, F]; w > 0: label l reads
    columns [l w, (l+1) w) and W is [L, w].  Parameters, Adam moments and the step count live on the device."""

    def __init__(self, X, Y, M, W, b, *, col0: int = 0, F: int | None = None, label_width: int = 0, bs: int = 128, lr: float = 1e-4,
                 weight_decay: float = 1e-4, dropout: float = 0.0, seed: int = 0, stream_id: int = 0, betas=BETAS, eps: float = EPS):
        self.X, self.N, self.ldx = fp32_matrix(X, "X")
        super().__init__(Y, M, bs, lr, weight_decay, dropout, seed, stream_id, betas, eps)
        self.W, self.b = self.own(W), self.own(b)
        self.L = int(self.b.numel())
        self.label_width = int(label_width)
        self.col0 = int(col0)
        self.F = int(F) if F is not None else (self.ldx - self.col0)
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb, self.vb = torch.zeros_like(self.b), torch.zeros_like(self.b)
        self.t = torch.zeros(1, dtype=torch.int32, device=self.X.device)
        expect = self.L * (self.label_width if self.label_width > 0 else self.F)
        if self.W.numel() != expect:
            raise ValueError(f"HeadProblem: W has {self.W.numel()} elements, L={self.L}, F={self.F}, label_width={self.label_width} need {expect}")

    def live(self) -> dict:
        return {"best_W": self.W, "best_b": self.b}

    def entry(self, perm: torch.Tensor | None, loss_out: torch.Tensor | None) -> MedpHeadProblem:
        return MedpHeadProblem(ptr(self.X), ptr(self.Y), ptr(self.M), ptr(self.W), ptr(self.b), ptr(self.mW), ptr(self.vW), ptr(self.mb),
                               ptr(self.vb), ptr(self.t), ptr(perm), ptr(loss_out), self.ldx, self.N, self.ldy, self.col0, self.F, self.L,
                               self.label_width, self.bs, self.S, self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps,
                               self.dropout, self.seed, self.stream_id, 0)


def _table(struct, entries: Sequence):
    host = (struct * max(len(entries), 1))(*entries)
    return host, table_bytes(host, len(entries))


def make_table(entries: Sequence[MedpHeadProblem]):
    """(host ctypes array, the same bytes as a uint8 numpy array)."""
    return _table(MedpHeadProblem, entries)


def make_mlp_table(entries: Sequence[MedpMlpHeadProblem]):
    """(host ctypes array, the same bytes as a uint8 numpy array)."""
    return _table(MedpMlpHeadProblem, entries)


def _table_launcher(struct, train_epoch, what: str, entries: Sequence[Sequence], dev) -> Callable:
    """Every epoch's problem table (entries[e]) built and uploaded in one copy; returns launch(e)."""
    tables = [_table(struct, en) for en in entries]
    tables_dev = torch.as_tensor(np.stack([t[1] for t in tables]) if tables else np.zeros((0, 1), np.uint8), device=dev)
    return lambda e: check(train_epoch(tables[e][0], ptr(tables_dev[e]), len(entries[e]), stream()), what)


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
    entries = [pb.entry(perm, loss_out[p]) for p, (pb, perm) in enumerate(zip(problems, perms))]
    _table_launcher(MedpHeadProblem, lib().medp_head_train_epoch, "head_train_epoch", [entries], dev)(0)
    return loss_out


def _score_buffers(who: str, X: torch.Tensor, L: int, rows, logits, probs):
    """(n, logits [n, L] fp32, probs [L, n] fp64) of a scores call over the rows `rows` of X (int32; None: all n = N rows); the two
    buffers are allocated unless given."""
    if rows is not None and rows.dtype != torch.int32:
        raise TypeError(f"{who}: rows are int32")
    n = X.shape[0] if rows is None else int(rows.numel())
    logits = torch.empty((n, L), dtype=torch.float32, device=X.device) if logits is None else logits
    probs = torch.empty((L, n), dtype=torch.float64, device=X.device) if probs is None else probs
    return n, logits, probs


def head_scores(X, W, b, *, col0: int = 0, F: int | None = None, label_width: int = 0, rows: torch.Tensor | None = None, logits=None,
                probs=None):
    """(logits [n, L] fp32, probs [L, n] fp64 = the fp32 sigmoid widened) of the rows `rows` (int32, device; None: all rows)."""
    require_gpu()
    X, N, ldx = fp32_matrix(X, "X")
    L = int(b.numel())
    F = ldx - col0 if F is None else F
    n, logits, probs = _score_buffers("head_scores", X, L, rows, logits, probs)
    if W.dtype != torch.float32 or b.dtype != torch.float32 or W.numel() != L * (label_width if label_width > 0 else F):
        raise ValueError("head_scores: W fp32 [L, F] (or [L, label_width]), b fp32 [L]")
    check(lib().medp_head_scores(ptr(X), ldx, N, int(col0), int(F), L, int(label_width), ptr(W.contiguous()), ptr(b.contiguous()), ptr(rows),
                                 n, ptr(logits), ptr(probs), stream()), "head_scores")
    return logits, probs


# ------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------------------------------
class BestSelection:
    """The reference's per-epoch selection, on the device: macro AUROC of the validation probabilities (`LabelMetrics`, `nan_mean`),
    strict `>` against the running best (NaN never wins), `torch.where` copies of every live parameter tensor into its best slot.
    `live`: {result key: the tensor the kernels update in place}.  Nothing here synchronises; `result` is called after the run's
    one synchronise."""

    def __init__(self, epochs: int, live: dict, metrics: LabelMetrics, n_val: int, L: int, record_val_logits: bool):
        dev = next(iter(live.values())).device
        f64 = dict(dtype=torch.float64, device=dev)
        self.live, self.metrics, self.record = live, metrics, record_val_logits
        self.curve = torch.full((epochs,), float("nan"), **f64)
        self.best = torch.full((), -float("inf"), **f64)
        self.best_epoch = torch.full((), -1, dtype=torch.int64, device=dev)
        self.slots = {k: v.clone() for k, v in live.items()}
        self.logits = torch.empty((epochs if record_val_logits else 1, n_val, L), dtype=torch.float32, device=dev)
        self.probs = torch.empty((L, n_val), **f64)

    def buffers(self, e: int):
        """(logits [n, L], probs [L, n]) the scores kernel of epoch e writes."""
        return self.logits[e if self.record else 0], self.probs

    def update(self, e: int) -> None:
        macro = nan_mean(self.metrics(self.probs)[:, 1])
        better = macro > self.best                                                     # strict; NaN never wins
        self.best = torch.where(better, macro, self.best)
        self.best_epoch = torch.where(better, torch.full_like(self.best_epoch, e + 1), self.best_epoch)
        for k, v in self.live.items():
            self.slots[k] = torch.where(better, v, self.slots[k])
        self.curve[e] = macro

    def result(self, losses_h: np.ndarray) -> dict:
        """losses_h [E, 2] host.  The result dict of the trainers."""
        best_epoch = int(self.best_epoch.item())
        if best_epoch < 0:
            raise ValueError("no epoch has a defined validation macro AUROC: no label has two known validation rows of both classes")
        res = {"curve": self.curve.cpu().numpy(), "loss_sum": losses_h[:, 0], "valid_sum": losses_h[:, 1], "best_epoch": best_epoch,
               "best_val": float(self.best.item()), **self.slots}
        if self.record:
            res["val_logits"] = self.logits.cpu().numpy()
        return res


def _epoch_perms(perms, E: int, count: int, who: str) -> np.ndarray:
    host = np.ascontiguousarray(np.asarray(perms)[:, :count], dtype=np.int32)
    if host.shape != (E, count):
        raise ValueError(f"{who}: [{E}, {count}] permutation entries are needed, got {tuple(host.shape)}")
    return host


def _train(who: str, problems: Sequence, vals: Sequence[tuple], epochs: int, perms: Sequence, record_val_logits: bool, prepare: Callable,
           score: Callable, entry: Callable = lambda pb, perm_dev, perm_host, loss_out: pb.entry(perm_dev, loss_out),
           check_losses: Callable = lambda p, pb, losses_h: None) -> list:
    """The epoch loop of the three trainers.  The order fixes what is raised before the first launch: the metrics, the row orders
    (one upload per problem), every epoch's entries (`entry`), then `prepare(entries [E][P], hosts, dev)`, which uploads what the
    family keeps on the device and returns launch(e).  The loop copies nothing to or from the device: per epoch launch(e), then
    `score(pb, X_va, logits=, probs=)` and the selection of every problem; one synchronise and one copy of the losses at the end."""
    require_gpu()
    P, E = len(problems), int(epochs)
    dev = problems[0].X.device
    metrics = [LabelMetrics(v[1].to(dev), v[2].to(dev)) for v in vals]                 # raises before the first launch
    Xv = [fp32_matrix(v[0].to(dev), "X_va")[0] for v in vals]
    hosts = [_epoch_perms(pm, E, pb.S * pb.bs, who) for pb, pm in zip(problems, perms)]
    perm_dev = [torch.as_tensor(h, device=dev) for h in hosts]
    losses = torch.zeros((E, P, 2), dtype=torch.float64, device=dev)
    launch = prepare([[entry(pb, perm_dev[p][e], hosts[p][e], losses[e, p]) for p, pb in enumerate(problems)] for e in range(E)], hosts, dev)
    sel = [BestSelection(E, pb.live(), metrics[p], Xv[p].shape[0], pb.L, record_val_logits) for p, pb in enumerate(problems)]
    for e in range(E):
        launch(e)
        for p, pb in enumerate(problems):
            logits, probs = sel[p].buffers(e)
            score(pb, Xv[p], logits=logits, probs=probs)
            sel[p].update(e)
    torch.cuda.synchronize(dev)
    losses_h = losses.cpu().numpy()
    out = []
    for p, pb in enumerate(problems):
        check_losses(p, pb, losses_h[:, p])
        out.append(sel[p].result(losses_h[:, p]))
    return out


def train_heads(problems: Sequence[HeadProblem], vals: Sequence[tuple], epochs: int, perms: Sequence[np.ndarray],
                record_val_logits: bool = False) -> list:
    """`epochs` epochs of every problem, one launch group per epoch, best-validation-macro-AUROC selection on the device.
    vals[p] = (X_va, Y_va, M_va) with the problem's column layout; perms[p]: [epochs, >= S bs] int host array.
    One result dict per problem: curve [E], loss_sum / valid_sum [E], best_epoch (1-based), best_val, best_W / best_b, and
    val_logits [E, n, L] when asked for.  Raises ValueError when no epoch has a defined macro AUROC, or a permutation was bad."""
    def prepare(entries, hosts, dev):
        if entries:
            try:
                check_table(entries[0])                                                # a null device table is never launched
            except ValueError as err:
                if "null device table" not in str(err):
                    raise
        return _table_launcher(MedpHeadProblem, lib().medp_head_train_epoch, "head_train_epoch", entries, dev)

    def nan_loss(p, pb, losses_h):                                                     # what the kernel leaves of a bad permutation
        if np.isnan(losses_h).any():
            raise ValueError(f"train_heads: problem {p} has a permutation entry outside [0, {pb.N})")

    return _train("train_heads", problems, vals, epochs, perms, record_val_logits, prepare, check_losses=nan_loss,
                  score=lambda pb, Xv, **out: head_scores(Xv, pb.W, pb.b, col0=pb.col0, F=pb.F, label_width=pb.label_width, **out))


# ------------------------------------------------------------------------------------------------------------------------------
# heads with a hidden stage: attention pooling, the MLP fusion head (csrc/pool_head_probe.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def pool_head_supported(T: int, d: int, L: int, bs: int) -> bool:
    """The limits of `medp_pool_head_train_epoch` (needs no GPU)."""
    return 1 <= T <= MAX_T and 1 <= d <= MAX_F and 1 <= L <= MAX_L and 1 <= bs <= MAX_BS


def pool_rows_onchip(T: int, d: int) -> bool:
    """True when the row kernel keeps a row's T d tokens in LDS; they are re-read from global memory otherwise."""
    return bool(lib().medp_pool_head_rows_onchip(int(T), int(d)))


def mlp_head_supported(L: int, H: int, bs: int, K: int | None = None) -> bool:
    """True when the MLP head's parameters, moments and minibatch activations fit the LDS budget (K inputs, 2 L by default)."""
    return bool(lib().medp_mlp_head_supported(int(2 * L if K is None else K), int(L), int(H), int(bs)))


def _perm_pair(perm, count: int, dev):
    """(host int32 array of `count` entries, its device copy): the kernels read the copy of exactly what the library validates."""
    host = np.ascontiguousarray(np.asarray(perm.cpu() if isinstance(perm, torch.Tensor) else perm).reshape(-1)[:count], dtype=np.int32)
    if host.size < count:
        raise ValueError(f"a permutation has {host.size} entries, {count} are needed")
    return host, (torch.as_tensor(host, device=dev) if dev is not None else None)


class PoolHeadProblem(_Problem):
    """`LinearHead(use_attn_pool=True)` over X [N, T, d]: attn_query q [d], head.1.weight W [L, d], head.1.bias b [L].  Parameters,
    Adam moments and the workspace live on the device; `steps` (host) counts the steps taken."""

    def __init__(self, X, Y, M, q, W, b, *, bs: int = 128, lr: float = 1e-4, weight_decay: float = 1e-4, dropout: float = 0.0, seed: int = 0,
                 stream_id: int = 0, betas=BETAS, eps: float = EPS):
        if X.dtype != torch.float32 or X.ndim != 3:
            raise TypeError("PoolHeadProblem: X is fp32 [N, T, d]")
        self.X = X.contiguous()
        self.N, self.T, self.d = (int(v) for v in self.X.shape)
        super().__init__(Y, M, bs, lr, weight_decay, dropout, seed, stream_id, betas, eps)
        self.q, self.W, self.b = self.own(q), self.own(W), self.own(b)
        self.L = int(self.b.numel())
        if self.q.numel() != self.d or self.W.numel() != self.L * self.d:
            raise ValueError(f"PoolHeadProblem: q has {self.q.numel()} and W {self.W.numel()} elements, d={self.d}, L={self.L}")
        self.mq, self.vq, self.mW, self.vW, self.mb, self.vb = (torch.zeros_like(t) for t in (self.q, self.q, self.W, self.W, self.b, self.b))
        self.steps = 0
        nbytes = int(lib().medp_pool_head_ws_bytes(self.d, min(max(self.L, 1), MAX_L), max(self.bs, 1)))
        self.ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.X.device) if self.X.is_cuda else None

    def live(self) -> dict:
        return {"attn_query": self.q, "head.1.weight": self.W, "head.1.bias": self.b}

    def entry(self, perm_dev, loss_out, addr=ptr) -> MedpPoolHeadProblem:
        a = addr
        return MedpPoolHeadProblem(a(self.X), a(self.Y), a(self.M), a(self.q), a(self.W), a(self.b), a(self.mq), a(self.vq), a(self.mW),
                                   a(self.vW), a(self.mb), a(self.vb), a(perm_dev), a(self.ws), a(loss_out), self.N, self.T, self.d, self.L,
                                   self.ldy, self.bs, self.S, self.steps, self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps,
                                   self.dropout, self.seed, self.stream_id, 0)


def pool_head_train_epoch(pb: PoolHeadProblem, perm, loss_out: torch.Tensor | None = None) -> torch.Tensor:
    """One epoch (S steps, two launches each) enqueued by ONE library call.  perm: at least S bs row indices (host array or tensor);
    the device copy is made from the host array the library validates.  Returns loss_out [2] fp64 = (sum of loss * vc, sum of vc);
    parameters and moments are updated in place and pb.steps advances by S."""
    require_gpu()
    host, dev_perm = _perm_pair(perm, pb.S * pb.bs, pb.X.device)
    if loss_out is None:
        loss_out = torch.empty(2, dtype=torch.float64, device=pb.X.device)
    entry = pb.entry(dev_perm, loss_out)
    check(lib().medp_pool_head_train_epoch(ctypes.byref(entry), host.ctypes.data, stream()), "pool_head_train_epoch")
    pb.steps += pb.S
    return loss_out


def pool_head_scores(X, q, W, b, *, rows: torch.Tensor | None = None, logits=None, probs=None):
    """(logits [n, L] fp32, probs [L, n] fp64 = the fp32 sigmoid widened) of the attention-pooled head over X [N, T, d]."""
    require_gpu()
    if X.dtype != torch.float32 or X.ndim != 3:
        raise TypeError("pool_head_scores: X is fp32 [N, T, d]")
    X = X.contiguous()
    N, T, d = (int(v) for v in X.shape)
    L = int(b.numel())
    n, logits, probs = _score_buffers("pool_head_scores", X, L, rows, logits, probs)
    if any(t.dtype != torch.float32 for t in (q, W, b)) or q.numel() != d or W.numel() != L * d:
        raise ValueError("pool_head_scores: q fp32 [d], W fp32 [L, d], b fp32 [L]")
    check(lib().medp_pool_head_scores(ptr(X), N, T, d, L, ptr(q.contiguous()), ptr(W.contiguous()), ptr(b.contiguous()), ptr(rows), n,
                                      ptr(logits), ptr(probs), stream()), "pool_head_scores")
    return logits, probs


class MlpHeadProblem(_Problem):
    """`LogitFusionHead("mlp")` over the K columns [col0, col0 + K) of X: head.0.weight W1 [H, K], head.0.bias b1 [H], head.3.weight
    W2 [L, H], head.3.bias b2 [L].  Parameters, Adam moments (one buffer: first then second, in the order W1, b1, W2, b2) and the step
    count live on the device."""

    def __init__(self, X, Y, M, W1, b1, W2, b2, *, col0: int = 0, K: int | None = None, bs: int = 128, lr: float = 1e-3,
                 weight_decay: float = 1e-4, dropout: float = 0.0, seed: int = 0, stream_id: int = 0, betas=BETAS, eps: float = EPS):
        self.X, self.N, self.ldx = fp32_matrix(X, "X")
        super().__init__(Y, M, bs, lr, weight_decay, dropout, seed, stream_id, betas, eps)
        self.W1, self.b1, self.W2, self.b2 = self.own(W1), self.own(b1), self.own(W2), self.own(b2)
        self.col0 = int(col0)
        self.K = int(K) if K is not None else self.ldx - self.col0
        self.H, self.L = int(self.b1.numel()), int(self.b2.numel())
        if self.W1.numel() != self.H * self.K or self.W2.numel() != self.L * self.H:
            raise ValueError(f"MlpHeadProblem: W1 has {self.W1.numel()} and W2 {self.W2.numel()} elements, K={self.K}, H={self.H}, L={self.L}")
        self.n_params = self.H * self.K + self.H + self.L * self.H + self.L
        self.mom = torch.zeros(2 * self.n_params, dtype=torch.float32, device=self.X.device)
        self.t = torch.zeros(1, dtype=torch.int32, device=self.X.device)

    def live(self) -> dict:
        return {"head.0.weight": self.W1, "head.0.bias": self.b1, "head.3.weight": self.W2, "head.3.bias": self.b2}

    def entry(self, perm_dev, perm_host: np.ndarray, loss_out, addr=ptr) -> MedpMlpHeadProblem:
        a = addr
        return MedpMlpHeadProblem(a(self.X), a(self.Y), a(self.M), a(self.W1), a(self.b1), a(self.W2), a(self.b2), a(self.mom), a(self.t),
                                  a(perm_dev), None if perm_host is None else perm_host.ctypes.data, a(loss_out), self.ldx, self.N, self.ldy,
                                  self.col0, self.K, self.H, self.L, self.bs, self.S, 0, self.lr, self.weight_decay, self.betas[0],
                                  self.betas[1], self.eps, self.dropout, self.seed, self.stream_id, 0)


def mlp_head_train_epoch(problems: Sequence[MlpHeadProblem], perms: Sequence, loss_out: torch.Tensor | None = None) -> torch.Tensor:
    """One epoch of every problem in ONE launch.  perms[p]: at least S bs row indices (host array or tensor).  Returns loss_out [P, 2]."""
    require_gpu()
    dev = problems[0].X.device
    if loss_out is None:
        loss_out = torch.empty((len(problems), 2), dtype=torch.float64, device=dev)
    pairs = [_perm_pair(pm, pb.S * pb.bs, dev) for pb, pm in zip(problems, perms)]
    entries = [pb.entry(pd, ph, loss_out[p]) for p, (pb, (ph, pd)) in enumerate(zip(problems, pairs))]
    _table_launcher(MedpMlpHeadProblem, lib().medp_mlp_head_train_epoch, "mlp_head_train_epoch", [entries], dev)(0)
    return loss_out


def mlp_head_scores(X, W1, b1, W2, b2, *, col0: int = 0, K: int | None = None, rows: torch.Tensor | None = None, logits=None, probs=None):
    """(logits [n, L] fp32, probs [L, n] fp64 = the fp32 sigmoid widened) of the MLP head, no dropout."""
    require_gpu()
    X, N, ldx = fp32_matrix(X, "X")
    H, L = int(b1.numel()), int(b2.numel())
    K = ldx - col0 if K is None else K
    n, logits, probs = _score_buffers("mlp_head_scores", X, L, rows, logits, probs)
    if any(t.dtype != torch.float32 for t in (W1, b1, W2, b2)) or W1.numel() != H * K or W2.numel() != L * H:
        raise ValueError("mlp_head_scores: W1 fp32 [H, K], b1 fp32 [H], W2 fp32 [L, H], b2 fp32 [L]")
    check(lib().medp_mlp_head_scores(ptr(X), ldx, N, int(col0), int(K), H, L, ptr(W1.contiguous()), ptr(b1.contiguous()), ptr(W2.contiguous()),
                                     ptr(b2.contiguous()), ptr(rows), n, ptr(logits), ptr(probs), stream()), "mlp_head_scores")
    return logits, probs


def train_pool_head(pb: PoolHeadProblem, val: tuple, epochs: int, perms: np.ndarray, record_val_logits: bool = False) -> dict:
    """`train_heads` for the attention-pooled head: per epoch one `medp_pool_head_train_epoch` call and one scores launch, the
    selection of `BestSelection`, one synchronise at the end.  val = (X_va [n, T, d], Y_va, M_va); perms [epochs, >= S bs].
    The result dict of `train_heads` with the best `attn_query`, `head.1.weight`, `head.1.bias` in place of best_W / best_b."""
    def prepare(entries, hosts, dev):
        for e, (entry,) in enumerate(entries):
            entry.step0 += e * pb.S                                                    # the kernels keep no counter of their own

        def launch(e):
            check(lib().medp_pool_head_train_epoch(ctypes.byref(entries[e][0]), hosts[0][e].ctypes.data, stream()), "pool_head_train_epoch")
            pb.steps += pb.S
        return launch

    return _train("train_pool_head", [pb], [val], epochs, [perms], record_val_logits, prepare,
                  score=lambda pb, Xv, **out: pool_head_scores(Xv, pb.q, pb.W, pb.b, **out))[0]


def train_mlp_heads(problems: Sequence[MlpHeadProblem], vals: Sequence[tuple], epochs: int, perms: Sequence[np.ndarray],
                    record_val_logits: bool = False) -> list:
    """`train_heads` for MLP fusion heads: one launch per epoch serves every problem.  vals[p] = (X_va, Y_va, M_va) with the problem's
    column layout.  The result dicts carry the best `head.0.weight`, `head.0.bias`, `head.3.weight`, `head.3.bias`."""
    return _train("train_mlp_heads", problems, vals, epochs, perms, record_val_logits,
                  lambda entries, hosts, dev: _table_launcher(MedpMlpHeadProblem, lib().medp_mlp_head_train_epoch, "mlp_head_train_epoch", entries, dev),
                  score=lambda pb, Xv, **out: mlp_head_scores(Xv, pb.W1, pb.b1, pb.W2, pb.b2, col0=pb.col0, K=pb.K, **out),
                  entry=lambda pb, perm_dev, perm_host, loss_out: pb.entry(perm_dev, perm_host, loss_out))


def history_lines(result: dict, tag: str = "epoch") -> list:
    """The reference's per-epoch line, from a result of `train_heads` (printed after the run: the loop never synchronises)."""
    return [f"  {tag} {e + 1:>2d}  train_loss={result['loss_sum'][e] / max(result['valid_sum'][e], 1):.4f}  "
            f"val_macro_AUROC={result['curve'][e]:.4f}" for e in range(len(result["curve"]))]


# ------------------------------------------------------------------------------------------------------------------------------
# eager fallback and comparison baseline
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
    """The reference's loop through torch autograd on the device, for a head whose shape is outside the kernels' limits, and the
    baseline the device paths are timed against: `forward(model, *inputs)` gives the logits; minibatches follow `perms`; AdamW; per
    epoch the validation macro AUROC from the metrics kernel and the strict `>` selection.  Synchronises every step, as the
    reference does (`.item()`)."""
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
