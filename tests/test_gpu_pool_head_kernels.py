"""Kernel-level tests of csrc/pool_head_probe.hip (the attention-pooled head's row / column kernels, the MLP fusion head's epoch kernel,
both scores kernels) against the numpy restatement tests/pool_head_refs.py.

Tolerance (DESIGN.md "Linear-head probes", the rule of test_gpu_head_probe_kernels.py): the device is an fp32 realisation of the loop
with its own summation order; the restatement run in fp32 numpy is another.  A case's rounding noise is measured as
gap = max|fp32 restatement - fp64 restatement| on that case, and the device must be within 8 gap + 1e-7 of the fp64 restatement.
Masks, guards, copies and repeated launches are exact."""
import math

import numpy as np
import pytest
import torch

import dropout_twin
import pool_head_refs as prefs
from multimodal_edema_prediction_amd import head_probe

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 3e-3, 1e-2
t_ = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731


def _labels(rng, n_used, N, L, ldy_pad=1):
    Y = np.full((N, L + ldy_pad), np.nan, dtype=np.float32)
    M = np.full((N, L + ldy_pad), np.nan, dtype=np.float32)
    Y[:n_used, :L] = rng.random((n_used, L)) < 0.4
    M[:n_used, :L] = rng.random((n_used, L)) < 0.8
    return Y, M


def close(params_dev: dict, loss, T, R32, what):
    gap = prefs.param_gap(R32["params"], T["params"])
    bound = 8 * gap + 1e-7
    errs = {k: float(np.abs(v.cpu().numpy().astype(np.float64).reshape(T["params"][k].shape) - T["params"][k]).max()) for k, v in params_dev.items()}
    print(f"{what}: " + " ".join(f"|{k} - T| {e:.3g}" for k, e in errs.items()) + f" gap {gap:.3g} bound {bound:.3g}")
    assert all(e <= bound for e in errs.values()), errs
    if loss is not None:
        got = loss.cpu().numpy()
        assert abs(got[1] - T["valid_sum"][-1]) == 0
        # the loss is summed in fp64 from fp32-rounded logits: far below 1e-5 per known label
        assert abs(got[0] - T["loss_sum"][-1]) <= 1e-5 * max(T["valid_sum"][-1], 1)


# ---- attention-pooled head ------------------------------------------------------------------------------------------------------
def pool_case(T, d, L, bs, S, seed=0, tail=2):
    """X [N, T, d] with NaN tail rows (never read), Y / M [N, L + 1] with a NaN padding column."""
    rng = np.random.default_rng(seed)
    n_used, tail = S * bs, min(tail, bs - 1)
    N = n_used + tail
    X = np.full((N, T, d), np.nan, dtype=np.float32)
    X[:n_used] = rng.standard_normal((n_used, T, d)).astype(np.float32)
    Y, M = _labels(rng, n_used, N, L)
    P = {"attn_query": rng.standard_normal(d).astype(np.float32), "head.1.weight": (0.1 * rng.standard_normal((L, d))).astype(np.float32),
         "head.1.bias": (0.1 * rng.standard_normal(L)).astype(np.float32)}
    return dict(X=X, Y=Y, M=M, P=P, perm=rng.permutation(n_used).astype(np.int32), T=T, d=d, L=L, bs=bs, S=S, N=N)


def pool_problem(c, *, dropout=0.0, seed=0, sid=0, betas=head_probe.BETAS):
    return head_probe.PoolHeadProblem(t_(c["X"]), t_(c["Y"]), t_(c["M"]), *(t_(c["P"][k]) for k in prefs.POOL_KEYS), bs=c["bs"], lr=LR,
                                      weight_decay=WD, dropout=dropout, seed=seed, stream_id=sid, betas=betas)


def pool_ref(c, dtype, perms=None, mask_fn=None):
    return prefs.train_pool_ref(np.nan_to_num(c["X"]), np.nan_to_num(c["Y"][:, :c["L"]]), np.nan_to_num(c["M"][:, :c["L"]]), c["P"],
                                [c["perm"]] if perms is None else perms, bs=c["bs"], lr=LR, wd=WD, dtype=dtype, mask_fn=mask_fn)


def masks(seed, sid, p):
    return lambda t, bs, F: dropout_twin.mask_scale(seed, sid, np.arange(bs * F, dtype=np.uint32).reshape(bs, F), p, epoch=t)


#           T   d     L   bs  S  on chip
POOL_SHAPES = [(5, 70, 3, 32, 3, True),       # the fixture's shape: a ragged second trip of the lane loops, T no power of two
               (1, 70, 3, 8, 2, True),        # T 1: the softmax is 1, the query's gradient 0
               (24, 130, 7, 16, 2, True),     # the 8-label padding
               (5, 70, 1, 8, 2, True), (3, 33, 16, 8, 2, True), (9, 600, 2, 4, 2, True),   # L 1 / 16 / 2, d over one trip of the column loop
               (24, 1600, 3, 8, 2, False)]    # 154 KB of tokens per row: re-read from global memory


@pytest.mark.parametrize("T, d, L, bs, S, on", POOL_SHAPES)
def test_pool_one_epoch_matches_the_restatement(T, d, L, bs, S, on):
    assert head_probe.pool_rows_onchip(T, d) == on
    c = pool_case(T, d, L, bs, S, seed=T + d + L)
    pb = pool_problem(c)
    loss = head_probe.pool_head_train_epoch(pb, c["perm"])
    assert pb.steps == S
    close(pb.live(), loss, pool_ref(c, np.float64), pool_ref(c, np.float32), f"pool T={T} d={d} L={L} bs={bs} S={S}")
    assert all(torch.isfinite(v).all() for v in pb.live().values())        # the NaN tail rows and the label padding were never read


def test_pool_a_row_repeated_within_a_minibatch_and_an_all_unknown_minibatch():
    c = pool_case(5, 70, 3, 16, 3, seed=7)
    c["perm"][3] = c["perm"][9] = c["perm"][0]                             # the same row three times in step 0
    c["M"][c["perm"][16:32], :] = 0.0                                       # step 1 knows no label
    pb = pool_problem(c)
    loss = head_probe.pool_head_train_epoch(pb, c["perm"])
    T = pool_ref(c, np.float64)
    close(pb.live(), loss, T, pool_ref(c, np.float32), "pool repeat / vc=0")
    known = np.nan_to_num(c["M"][np.r_[c["perm"][:16], c["perm"][32:]], :3]).sum()
    assert T["state"][2] == 3 and T["valid_sum"][-1] == known and float(loss[1]) == known      # valid_sum unchanged by the unknown step
    # the all-unknown step alone: zero gradients, so the moments stay zero and the weights take the decay and nothing else
    one = pool_case(5, 70, 3, 16, 1, seed=7)
    one["M"][:] = np.where(np.isnan(one["M"]), np.nan, 0.0)
    p1 = pool_problem(one)
    loss1 = head_probe.pool_head_train_epoch(p1, one["perm"])
    assert float(loss1[0]) == 0 and float(loss1[1]) == 0
    decay = np.float32(1.0 - LR * WD)
    for k, v in p1.live().items():
        assert torch.equal(v.cpu(), torch.as_tensor(one["P"][k] * decay)), k   # weight decay still applied, nothing else moved
    assert all(float(m.abs().max()) == 0 for m in (p1.mq, p1.vq, p1.mW, p1.vW, p1.mb, p1.vb))


def test_pool_dropout_masks_are_the_twins_exactly():
    """T = 1 makes pooled = x.  beta1 = 0 makes the first moment the gradient itself; with W = b = 0, Y = 0, M = 1 every g[r] is
    0.5 / bs, and with x[r, 0, j] = 1 only where (j + shift) % bs == r the gradient of column j is g times the mask factor of ONE
    element: every factor is read back."""
    bs, d, p, seed, sid = 4, 257, 0.3, 1234, 3
    want = masks(seed, sid, p)(1, bs, d).astype(np.float64) * np.float64(np.float32(0.5 / bs))
    seen = np.zeros((bs, d), dtype=bool)
    for shift in range(bs):
        hot = (np.arange(d)[None, :] + shift) % bs == np.arange(bs)[:, None]
        c = pool_case(1, d, 1, bs, 1, tail=0)
        c["X"][:, 0, :] = hot.astype(np.float32)
        c["Y"][:], c["M"][:] = 0.0, 1.0
        c["P"] = {k: np.zeros_like(v) for k, v in c["P"].items()}
        pb = pool_problem(c, dropout=p, seed=seed, sid=sid, betas=(0.0, 0.999))
        head_probe.pool_head_train_epoch(pb, np.arange(bs))
        assert np.array_equal(pb.mW.cpu().numpy()[0], (want * hot).sum(0).astype(np.float32)), shift
        seen |= hot
    assert seen.all() and (want == 0).mean() > 0.2 and (want > 0).mean() > 0.6


def test_pool_dropout_and_the_step_number_carried_over_two_epoch_calls():
    c = pool_case(5, 70, 3, 32, 3, seed=9)
    second = np.random.default_rng(1).permutation(c["S"] * c["bs"]).astype(np.int32)
    p, seed, sid = 0.1, 77, 1
    pb = pool_problem(c, dropout=p, seed=seed, sid=sid)
    head_probe.pool_head_train_epoch(pb, c["perm"])
    loss = head_probe.pool_head_train_epoch(pb, second)
    assert pb.steps == 6
    both = [c["perm"], second]
    T, R32 = (pool_ref(c, dt, perms=both, mask_fn=masks(seed, sid, p)) for dt in (np.float64, np.float32))   # ONE run of 2 S steps
    close(pb.live(), loss, T, R32, "pool dropout, two epoch calls")
    bound = 8 * prefs.param_gap(R32["params"], T["params"]) + 1e-7
    assert prefs.param_gap(pool_ref(c, np.float64, perms=both)["params"], T["params"]) > 100 * bound      # without the masks T is far away
    # a second epoch that restarted the step count would draw the first epoch's masks again
    again = pool_ref(c, np.float64, perms=both, mask_fn=lambda t, bs, F: masks(seed, sid, p)((t - 1) % 3 + 1, bs, F))
    assert prefs.param_gap(again["params"], T["params"]) > 100 * bound


@pytest.mark.parametrize("T, d", [(5, 70), (24, 1600)])
def test_pool_the_same_call_twice_is_bit_identical_and_nothing_outside_the_buffers_is_written(T, d):
    c = pool_case(T, d, 7, 8, 2, seed=5)
    outs = []
    for _ in range(2):
        pb = pool_problem(c, dropout=0.3, seed=11, sid=2)
        guarded = {}
        for a in ("q", "W", "b", "mq", "vq", "mW", "vW", "mb", "vb"):       # parameters and moments inside sentinel-filled buffers
            v = getattr(pb, a)
            buf = torch.full((v.numel() + 64,), 12345.0, device=DEV)
            buf[32:32 + v.numel()] = v.reshape(-1)
            setattr(pb, a, buf[32:32 + v.numel()].view(v.shape))
            guarded[a] = buf
        nbytes = int(head_probe.lib().medp_pool_head_ws_bytes(d, 7, 8))
        assert nbytes == 8 * 9 + 4 * (8 * 8 + 2 * 8 * d)
        wsbuf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=DEV)
        pb.ws = wsbuf[64:64 + nbytes]
        bystander = torch.full((1024,), 7.0, device=DEV)
        loss = head_probe.pool_head_train_epoch(pb, c["perm"])
        for a, buf in guarded.items():
            assert (buf[:32] == 12345.0).all() and (buf[-32:] == 12345.0).all(), a
        assert (wsbuf[:64] == 0xA5).all() and (wsbuf[-64:] == 0xA5).all() and (bystander == 7.0).all()
        assert torch.equal(t_(c["X"][:16]), pb.X[:16]) and torch.isnan(pb.X[16:]).all()
        outs.append([getattr(pb, a).clone() for a in guarded] + [loss.clone()])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("T, d, L", [(5, 70, 3), (24, 130, 7), (24, 1600, 16), (1, 9, 1)])
def test_pool_scores_match_the_restatements_forward(T, d, L):
    c = pool_case(T, d, L, 8, 5, seed=3)
    rows = np.random.default_rng(2).permutation(40)[:23].astype(np.int32)
    P64 = {k: v.astype(np.float64) for k, v in c["P"].items()}
    for sel, want_rows in ((t_(rows), rows), (None, np.arange(40))):
        X = c["X"] if sel is not None else c["X"][:40]
        logits, probs = head_probe.pool_head_scores(t_(X), *(t_(c["P"][k]) for k in prefs.POOL_KEYS), rows=sel)
        x = c["X"][want_rows]
        z64 = prefs.pool_forward(x.astype(np.float64), P64)[0]
        gap = np.abs(prefs.pool_forward(x, c["P"])[0] - z64).max()
        err = np.abs(logits.cpu().numpy() - z64).max()
        print(f"pool scores T={T} d={d} L={L}: |z - T| {err:.3g} gap {gap:.3g}")
        assert logits.shape == (len(want_rows), L) and probs.shape == (L, len(want_rows)) and err <= 8 * gap + 1e-7
        assert probs.dtype == torch.float64 and torch.equal(probs, torch.sigmoid(logits).t().double())
    bad = np.array([4, c["N"], 0, -1], dtype=np.int32)                       # a row outside the matrix is not dereferenced
    logits, probs = head_probe.pool_head_scores(t_(c["X"]), *(t_(c["P"][k]) for k in prefs.POOL_KEYS), rows=t_(bad))
    assert torch.isfinite(logits[[0, 2]]).all() and torch.isnan(logits[[1, 3]]).all() and torch.isnan(probs[:, [1, 3]]).all()


def test_pool_a_bad_permutation_entry_raises_and_launches_nothing():
    c = pool_case(5, 70, 3, 8, 2, seed=4)
    for bad in (c["N"], -1):
        pb = pool_problem(c)
        perm = c["perm"].copy()
        perm[5] = bad
        with pytest.raises(ValueError, match="permutation entry 5"):
            head_probe.pool_head_train_epoch(pb, perm)
        torch.cuda.synchronize()
        assert pb.steps == 0 and all(torch.equal(v.cpu(), torch.as_tensor(c["P"][k])) for k, v in pb.live().items())


# ---- MLP fusion head ------------------------------------------------------------------------------------------------------------
def mlp_case(K, H, L, bs, S, seed=0, tail=2, pad=3, col0=1):
    rng = np.random.default_rng(seed)
    n_used, tail = S * bs, min(tail, bs - 1)
    N, ldx = n_used + tail, col0 + K + pad
    X = np.full((N, ldx), np.nan, dtype=np.float32)
    X[:n_used, col0:col0 + K] = (1.5 * rng.standard_normal((n_used, K))).astype(np.float32)
    Y, M = _labels(rng, n_used, N, L)
    P = {"head.0.weight": (0.4 * rng.standard_normal((H, K))).astype(np.float32), "head.0.bias": (0.2 * rng.standard_normal(H)).astype(np.float32),
         "head.3.weight": (0.3 * rng.standard_normal((L, H))).astype(np.float32), "head.3.bias": (0.1 * rng.standard_normal(L)).astype(np.float32)}
    return dict(X=X, Y=Y, M=M, P=P, perm=rng.permutation(n_used).astype(np.int32), K=K, H=H, L=L, bs=bs, S=S, N=N, col0=col0)


def mlp_problem(c, *, dropout=0.0, seed=0, sid=0, betas=head_probe.BETAS):
    return head_probe.MlpHeadProblem(t_(c["X"]), t_(c["Y"]), t_(c["M"]), *(t_(c["P"][k]) for k in prefs.MLP_KEYS), col0=c["col0"], K=c["K"],
                                     bs=c["bs"], lr=LR, weight_decay=WD, dropout=dropout, seed=seed, stream_id=sid, betas=betas)


def mlp_ref(c, dtype, perms=None, mask_fn=None):
    X = np.nan_to_num(c["X"][:, c["col0"]:c["col0"] + c["K"]])
    return prefs.train_mlp_ref(X, np.nan_to_num(c["Y"][:, :c["L"]]), np.nan_to_num(c["M"][:, :c["L"]]), c["P"],
                               [c["perm"]] if perms is None else perms, bs=c["bs"], lr=LR, wd=WD, dtype=dtype, mask_fn=mask_fn)


@pytest.mark.parametrize("K, H, L, bs, S", [(6, 32, 3, 32, 3), (2, 5, 1, 7, 3), (32, 32, 16, 7, 2), (14, 64, 7, 128, 1), (1, 1, 1, 1, 2)])
def test_mlp_one_epoch_matches_the_restatement(K, H, L, bs, S):
    assert head_probe.mlp_head_supported(L, H, bs, K)
    c = mlp_case(K, H, L, bs, S, seed=K + H)
    pb = mlp_problem(c)
    loss = head_probe.mlp_head_train_epoch([pb], [c["perm"]])[0]
    assert int(pb.t.item()) == S
    close(pb.live(), loss, mlp_ref(c, np.float64), mlp_ref(c, np.float32), f"mlp K={K} H={H} L={L} bs={bs} S={S}")
    assert all(torch.isfinite(v).all() for v in pb.live().values()) and torch.isfinite(pb.mom).all()


def test_mlp_a_row_repeated_within_a_minibatch_and_an_all_unknown_minibatch():
    c = mlp_case(6, 32, 3, 16, 3, seed=7)
    c["perm"][3] = c["perm"][9] = c["perm"][0]
    c["M"][c["perm"][16:32], :] = 0.0
    pb = mlp_problem(c)
    loss = head_probe.mlp_head_train_epoch([pb], [c["perm"]])[0]
    T = mlp_ref(c, np.float64)
    close(pb.live(), loss, T, mlp_ref(c, np.float32), "mlp repeat / vc=0")
    assert T["state"][2] == 3 and float(loss[1]) == np.nan_to_num(c["M"][np.r_[c["perm"][:16], c["perm"][32:]], :3]).sum()
    one = mlp_case(6, 32, 3, 16, 1, seed=7)
    one["M"][:] = np.where(np.isnan(one["M"]), np.nan, 0.0)
    p1 = mlp_problem(one)
    loss1 = head_probe.mlp_head_train_epoch([p1], [one["perm"]])[0]
    assert float(loss1[0]) == 0 and float(loss1[1]) == 0 and float(p1.mom.abs().max()) == 0
    for k, v in p1.live().items():
        assert torch.equal(v.cpu(), torch.as_tensor(one["P"][k] * np.float32(1.0 - LR * WD))), k


def test_mlp_dropout_masks_on_the_hidden_units_are_the_twins_exactly():
    """One row, W1 = 0, b1 = 1: every hidden unit is gelu(1) times its mask factor.  beta1 = 0, W2 = b2 = 0, Y = 0, M = 1: g = 0.5 and the
    first moment of W2[0, k] is 0.5 h_k, every factor read back."""
    H, p, seed, sid = 257, 0.3, 99, 2
    c = mlp_case(2, H, 1, 1, 1, tail=0)
    c["X"][:] = 1.0
    c["Y"][:], c["M"][:] = 0.0, 1.0
    c["P"] = {k: np.zeros_like(v) for k, v in c["P"].items()}
    c["P"]["head.0.bias"][:] = 1.0
    pb = mlp_problem(c, dropout=p, seed=seed, sid=sid, betas=(0.0, 0.999))
    head_probe.mlp_head_train_epoch([pb], [np.zeros(1, dtype=np.int32)])
    gelu1 = np.float32(0.5 * (1.0 + math.erf(math.sqrt(0.5))))
    want = (np.float64(0.5) * (gelu1 * masks(seed, sid, p)(1, 1, H)[0]).astype(np.float64)).astype(np.float32)
    n0 = H * 2 + H
    assert np.array_equal(pb.mom.cpu().numpy()[n0:n0 + H], want) and (want == 0).mean() > 0.2 and (want > 0).mean() > 0.6


def test_mlp_two_problems_with_their_own_seeds_in_one_launch_and_the_step_count_carried_on():
    cases = [mlp_case(6, 32, 3, 32, 3, seed=1), mlp_case(14, 5, 7, 16, 2, seed=2)]
    seeds, p = (5, 6), 0.1
    second = [np.random.default_rng(s).permutation(c["S"] * c["bs"]).astype(np.int32) for s, c in enumerate(cases)]
    group = [mlp_problem(c, dropout=p, seed=s) for c, s in zip(cases, seeds)]
    alone = [mlp_problem(c, dropout=p, seed=s) for c, s in zip(cases, seeds)]
    bystander = mlp_problem(cases[0])
    head_probe.mlp_head_train_epoch(group, [c["perm"] for c in cases])
    loss = head_probe.mlp_head_train_epoch(group, second)
    for c, pb, solo, sd, pm2, ls in zip(cases, group, alone, seeds, second, loss):
        head_probe.mlp_head_train_epoch([solo], [c["perm"]])
        ls1 = head_probe.mlp_head_train_epoch([solo], [pm2])[0]
        for a in ("W1", "b1", "W2", "b2", "mom", "t"):
            assert torch.equal(getattr(pb, a), getattr(solo, a)), a         # a launch of its own gives the same bits
        assert torch.equal(ls, ls1) and int(pb.t.item()) == 2 * c["S"]
        both = [c["perm"], pm2]
        T, R32 = (mlp_ref(c, dt, perms=both, mask_fn=masks(sd, 0, p)) for dt in (np.float64, np.float32))
        close(pb.live(), ls, T, R32, "mlp P=2, dropout, two launches")
        bound = 8 * prefs.param_gap(R32["params"], T["params"]) + 1e-7
        assert prefs.param_gap(mlp_ref(c, np.float64, perms=both)["params"], T["params"]) > 100 * bound
    assert torch.equal(bystander.W1.cpu(), torch.as_tensor(cases[0]["P"]["head.0.weight"])) and int(bystander.t.item()) == 0


def test_mlp_scores_match_the_restatements_forward():
    for K, H, L in ((6, 32, 3), (2, 5, 1), (32, 33, 16)):
        c = mlp_case(K, H, L, 10, 30, seed=3)
        rows = np.random.default_rng(2).permutation(300)[:270].astype(np.int32)
        P64 = {k: v.astype(np.float64) for k, v in c["P"].items()}
        args = [t_(c["P"][k]) for k in prefs.MLP_KEYS]
        for sel, want_rows in ((t_(rows), rows), (None, np.arange(300))):
            X = c["X"] if sel is not None else c["X"][:300]
            logits, probs = head_probe.mlp_head_scores(t_(X), *args, col0=c["col0"], K=K, rows=sel)
            x = c["X"][want_rows, c["col0"]:c["col0"] + K]
            z64 = prefs.mlp_forward(x.astype(np.float64), P64)[0]
            gap = np.abs(prefs.mlp_forward(x, c["P"])[0] - z64).max()
            err = np.abs(logits.cpu().numpy() - z64).max()
            print(f"mlp scores K={K} H={H} L={L}: |z - T| {err:.3g} gap {gap:.3g}")
            assert logits.shape == (len(want_rows), L) and err <= 8 * gap + 1e-7
            assert torch.equal(probs, torch.sigmoid(logits).t().double())
        bad = np.array([4, c["N"], -1], dtype=np.int32)
        logits, _ = head_probe.mlp_head_scores(t_(c["X"]), *args, col0=c["col0"], K=K, rows=t_(bad))
        assert torch.isfinite(logits[0]).all() and torch.isnan(logits[1:]).all()


def test_mlp_a_bad_permutation_entry_raises_and_launches_nothing():
    c = mlp_case(6, 32, 3, 8, 2, seed=4)
    pb = mlp_problem(c)
    perm = c["perm"].copy()
    perm[5] = c["N"]
    with pytest.raises(ValueError, match="permutation entry 5"):
        head_probe.mlp_head_train_epoch([pb], [perm])
    torch.cuda.synchronize()
    assert int(pb.t.item()) == 0 and torch.equal(pb.W1.cpu(), torch.as_tensor(c["P"]["head.0.weight"]))
