"""Kernel-level tests of csrc/head_probe.hip against the numpy restatement tests/head_probe_refs.py.

Tolerance (DESIGN.md "Linear-head probes"): the device is an fp32 realisation of the loop with its own summation order; the
restatement run in fp32 numpy is another.  A case's rounding noise is measured as gap = max|fp32 restatement - fp64 restatement|
on that case, and the device must be within 8 gap + 1e-7 of the fp64 restatement.  Masks, metrics on the device's own scores and
everything that is copied are exact."""
import numpy as np
import pytest
import torch

import dropout_twin
import head_probe_refs as refs
from multimodal_edema_prediction_amd import evaluator, head_probe, probe_stats

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 3e-3, 1e-2


def make_case(F, L, bs, S, *, width=0, seed=0, tail=3, pad=5, col0=2, ldy_pad=1, w_scale=0.1):
    """Host arrays of one problem: X [N, ldx] with NaN in the tail rows (never read) and in the padding columns, Y / M [N, L + 1]."""
    rng = np.random.default_rng(seed)
    n_used, tail = S * bs, min(tail, bs - 1)                              # N // bs stays S
    N, ldx, ldy = n_used + tail, col0 + F + pad, L + ldy_pad
    X = np.full((N, ldx), np.nan, dtype=np.float32)
    X[:n_used, col0:col0 + F] = rng.standard_normal((n_used, F)).astype(np.float32)
    Y = np.full((N, ldy), np.nan, dtype=np.float32)
    M = np.full((N, ldy), np.nan, dtype=np.float32)
    Y[:n_used, :L] = rng.random((n_used, L)) < 0.4
    M[:n_used, :L] = rng.random((n_used, L)) < 0.8
    W = (w_scale * rng.standard_normal((L, width if width else F))).astype(np.float32)
    b = (w_scale * rng.standard_normal(L)).astype(np.float32)
    perm = rng.permutation(n_used).astype(np.int32)
    return dict(X=X, Y=Y, M=M, W=W, b=b, perm=perm, F=F, L=L, bs=bs, S=S, width=width, col0=col0, N=N)


def problem(c, *, dropout=0.0, seed=0, sid=0, betas=head_probe.BETAS):
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    return head_probe.HeadProblem(t(c["X"]), t(c["Y"]), t(c["M"]), t(c["W"]), t(c["b"]), col0=c["col0"], F=c["F"], label_width=c["width"],
                                  bs=c["bs"], lr=LR, weight_decay=WD, dropout=dropout, seed=seed, stream_id=sid, betas=betas)


def ref(c, dtype, perms=None, mask_fn=None, state=None, W=None, b=None):
    cols = slice(c["col0"], c["col0"] + c["F"])
    X = np.nan_to_num(c["X"][:, cols], nan=0.0)
    return refs.train_ref(X, np.nan_to_num(c["Y"][:, :c["L"]]), np.nan_to_num(c["M"][:, :c["L"]]), c["W"] if W is None else W,
                          c["b"] if b is None else b, [c["perm"]] if perms is None else perms, bs=c["bs"], lr=LR, wd=WD,
                          label_width=c["width"], dtype=dtype, mask_fn=mask_fn, state=state)


def close(c, pb, loss, T, R32, what=""):
    gap = max(np.abs(R32["W"] - T["W"]).max(), np.abs(R32["b"] - T["b"]).max())
    bound = 8 * gap + 1e-7
    dW = np.abs(pb.W.cpu().numpy().astype(np.float64) - T["W"]).max()
    db = np.abs(pb.b.cpu().numpy().astype(np.float64) - T["b"]).max()
    print(f"{what} F={c['F']} L={c['L']} bs={c['bs']} S={c['S']} w={c['width']}: |W - T| {dW:.3g} |b - T| {db:.3g} gap {gap:.3g} bound {bound:.3g}")
    assert dW <= bound and db <= bound
    if loss is not None:
        got = loss.cpu().numpy()
        assert abs(got[1] - T["valid_sum"][-1]) == 0
        # the loss is summed in fp64 from fp32-rounded logits: |z| 2^-24 plus the logit's own noise per known label, far below 1e-5
        assert abs(got[0] - T["loss_sum"][-1]) <= 1e-5 * max(T["valid_sum"][-1], 1)
    assert int(pb.t.item()) == T["state"][4]


SHAPES = [(1, 1, 1, 1, True), (2, 3, 7, 3, True), (63, 16, 64, 1, True), (64, 3, 128, 3, True), (65, 1, 7, 3, True), (257, 3, 64, 3, True),
          (1025, 3, 128, 1, True), (1025, 16, 7, 3, False), (9312, 7, 128, 1, False)]


@pytest.mark.parametrize("F, L, bs, S, on", SHAPES)
def test_one_epoch_matches_the_restatement(F, L, bs, S, on):
    assert head_probe.onchip(F, L, 0, bs) == on                        # both homes of W and the Adam state are covered
    c = make_case(F, L, bs, S, seed=F + L)
    pb = problem(c)
    loss = head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])[0]
    close(c, pb, loss, ref(c, np.float64), ref(c, np.float32))
    assert torch.isfinite(pb.W).all()                                    # the NaN tail rows and padding columns were never read


@pytest.mark.parametrize("L, width", [(3, 2), (16, 2), (3, 5), (1, 7)])
def test_label_width(L, width):
    c = make_case(L * width, L, 7, 3, width=width, seed=L)
    pb = problem(c)
    loss = head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])[0]
    close(c, pb, loss, ref(c, np.float64), ref(c, np.float32), "label_width")


def test_three_problems_of_mixed_width_in_one_launch_equal_their_own_launches():
    cases = [make_case(64, 3, 32, 3, seed=1), make_case(1025, 16, 7, 3, seed=2), make_case(6, 3, 16, 2, width=2, seed=3)]
    group, alone = [problem(c) for c in cases], [problem(c) for c in cases]
    bystander = problem(cases[0])
    perms = [torch.as_tensor(c["perm"], device=DEV) for c in cases]
    loss = head_probe.head_train_epoch(group, perms)
    for c, pb, solo, pm, ls in zip(cases, group, alone, perms, loss):
        ls1 = head_probe.head_train_epoch([solo], [pm])[0]
        for a in ("W", "b", "mW", "vW", "mb", "vb", "t"):
            assert torch.equal(getattr(pb, a), getattr(solo, a)), a
        assert torch.equal(ls, ls1)
        close(c, pb, ls, ref(c, np.float64), ref(c, np.float32), "P=3")
    assert torch.equal(bystander.W.cpu(), torch.as_tensor(cases[0]["W"])) and int(bystander.t.item()) == 0     # a problem outside the launch


def test_two_launches_are_bit_identical_and_the_guards_stay():
    c = make_case(257, 7, 64, 3, seed=5)
    outs = []
    for _ in range(2):
        pb = problem(c, dropout=0.3, seed=11, sid=2)
        guarded = {}
        for a in ("W", "b", "mW", "vW", "mb", "vb"):                      # parameters and moments inside sentinel-filled buffers
            v = getattr(pb, a)
            buf = torch.full((v.numel() + 64,), 12345.0, device=DEV)
            buf[32:32 + v.numel()] = v.reshape(-1)
            setattr(pb, a, buf[32:32 + v.numel()].view(v.shape))
            guarded[a] = buf
        loss = head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])
        for a, buf in guarded.items():
            assert (buf[:32] == 12345.0).all() and (buf[-32:] == 12345.0).all(), a
        outs.append([pb.W.clone(), pb.b.clone(), pb.mW.clone(), pb.vW.clone(), loss.clone()])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_a_row_repeated_within_a_minibatch_and_an_all_unknown_minibatch():
    c = make_case(65, 3, 16, 3, seed=7)
    c["perm"][3] = c["perm"][9] = c["perm"][0]                             # the same row three times in step 0
    c["M"][c["perm"][16:32], :] = 0.0                                       # step 1 knows no label: zero gradients, AdamW still steps
    pb = problem(c)
    loss = head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])[0]
    T = ref(c, np.float64)
    close(c, pb, loss, T, ref(c, np.float32), "repeat / vc=0")
    # the restatement takes its AdamW step on the all-unknown minibatch (decay and momentum move the weights by about lr each);
    # a device that skipped it would miss T by far more than the bound
    assert T["state"][4] == 3 and T["valid_sum"][-1] == np.nan_to_num(c["M"][np.r_[c["perm"][:16], c["perm"][32:]], :3]).sum()


def masks(seed, sid, p):
    return lambda t, bs, F: dropout_twin.mask_scale(seed, sid, np.arange(bs * F, dtype=np.uint32).reshape(bs, F), p, epoch=t)


def test_dropout_masks_are_the_twins_exactly():
    """beta1 = 0 makes the first moment the gradient itself; with W = b = 0, Y = 0, M = 1 every g[r] is 0.5 / bs, and with x[r, j] = 1
    only where (j + shift) % bs == r the gradient of column j is g times the mask factor of ONE element: every factor is read back."""
    bs, F, p, seed, sid = 4, 257, 0.3, 1234, 3
    want = masks(seed, sid, p)(1, bs, F).astype(np.float64) * np.float64(np.float32(0.5 / bs))
    seen = np.zeros((bs, F), dtype=bool)
    for shift in range(bs):
        hot = (np.arange(F)[None, :] + shift) % bs == np.arange(bs)[:, None]
        c = make_case(F, 1, bs, 1, tail=0, pad=0, col0=0, ldy_pad=0)
        c["X"][:] = hot.astype(np.float32)
        c["Y"][:], c["M"][:], c["W"][:], c["b"][:] = 0.0, 1.0, 0.0, 0.0
        c["perm"] = np.arange(bs, dtype=np.int32)
        pb = problem(c, dropout=p, seed=seed, sid=sid, betas=(0.0, 0.999))
        head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])
        got = pb.mW.cpu().numpy()[0]
        exp = (want * hot).sum(0).astype(np.float32)
        assert np.array_equal(got, exp), shift
        seen |= hot
    assert seen.all() and (want == 0).mean() > 0.2 and (want > 0).mean() > 0.6


def test_dropout_and_step_counts_continuing_across_two_launches():
    c = make_case(70, 3, 32, 3, seed=9)
    rng = np.random.default_rng(1)
    second = rng.permutation(c["S"] * c["bs"]).astype(np.int32)
    p, seed, sid = 0.3, 77, 1
    pb = problem(c, dropout=p, seed=seed, sid=sid)
    head_probe.head_train_epoch([pb], [torch.as_tensor(c["perm"], device=DEV)])
    assert int(pb.t.item()) == 3
    loss = head_probe.head_train_epoch([pb], [torch.as_tensor(second, device=DEV)])[0]
    both = [c["perm"], second]
    T, R32 = (ref(c, dt, perms=both, mask_fn=masks(seed, sid, p)) for dt in (np.float64, np.float32))
    close(c, pb, loss, T, R32, "dropout, two launches")
    # without the masks the restatement is far away: the comparison does see them
    assert np.abs(ref(c, np.float64, perms=both)["W"] - T["W"]).max() > 100 * (8 * np.abs(R32["W"] - T["W"]).max() + 1e-7)


def test_a_bad_permutation_entry_gives_nan_and_a_raise_not_a_fault():
    c = make_case(64, 3, 16, 2, seed=4)
    for bad in (c["N"], -1):
        pb, good = problem(c), problem(c)
        perm = c["perm"].copy()
        perm[5] = bad
        loss = head_probe.head_train_epoch([pb, good], [torch.as_tensor(perm, device=DEV), torch.as_tensor(c["perm"], device=DEV)])
        assert torch.isnan(pb.W).all() and torch.isnan(pb.b).all() and torch.isnan(loss[0]).all()
        assert torch.isfinite(good.W).all() and torch.isfinite(loss[1]).all()           # its neighbour in the launch is served
    val = (torch.as_tensor(np.nan_to_num(c["X"]), device=DEV), torch.as_tensor(np.nan_to_num(c["Y"][:, :3]), device=DEV),
           torch.as_tensor(np.nan_to_num(c["M"][:, :3]), device=DEV))
    with pytest.raises(ValueError, match="permutation entry outside"):
        head_probe.train_heads([problem(c)], [val], 1, [perm[None, :]])


@pytest.fixture(scope="module")
def scored():
    """One scoring problem shared by the score / metric tests: (case, rows, logits, probs)."""
    rng = np.random.default_rng(3)
    c = make_case(257, 7, 50, 4, seed=8, w_scale=0.2)
    rows = rng.permutation(c["S"] * c["bs"])[:150].astype(np.int32)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    logits, probs = head_probe.head_scores(t(c["X"]), t(c["W"]), t(c["b"]), col0=c["col0"], F=c["F"], rows=t(rows))
    return c, rows, logits, probs


def test_scores_match_the_restatement(scored):
    c, rows, logits, probs = scored
    x = c["X"][rows, c["col0"]:c["col0"] + c["F"]]
    z64 = refs.forward(x.astype(np.float64), c["W"].astype(np.float64), c["b"].astype(np.float64))
    gap = np.abs(refs.forward(x, c["W"], c["b"]) - z64).max()
    err = np.abs(logits.cpu().numpy() - z64).max()
    print(f"scores: |z - T| {err:.3g} gap {gap:.3g}")
    assert logits.shape == (150, 7) and probs.shape == (7, 150) and err <= 8 * gap + 1e-7


def test_probabilities_are_torchs_fp32_sigmoid_of_the_devices_logits(scored):
    _, _, logits, probs = scored
    assert probs.dtype == torch.float64 and torch.equal(probs, torch.sigmoid(logits).t().double())


def test_scores_with_label_width_and_a_row_outside_the_matrix():
    c = make_case(6, 3, 10, 2, width=2, seed=2)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    rows = np.array([4, 0, c["N"], 7, -1], dtype=np.int32)
    logits, probs = head_probe.head_scores(t(c["X"]), t(c["W"]), t(c["b"]), col0=c["col0"], F=6, label_width=2, rows=t(rows))
    x = c["X"][[4, 0, 7], c["col0"]:c["col0"] + 6].astype(np.float64)
    z64 = refs.forward(x, c["W"].astype(np.float64), c["b"].astype(np.float64), 2)
    got = logits.cpu().numpy()
    assert np.abs(got[[0, 1, 3]] - z64).max() <= 1e-6 and np.isnan(got[[2, 4]]).all() and torch.isnan(probs[:, 2]).all()


def test_device_metrics_equal_the_host_evaluator_on_the_same_probabilities(scored):
    c, rows, logits, probs = scored
    Y, M = np.nan_to_num(c["Y"][rows, :7]), np.nan_to_num(c["M"][rows, :7])
    M[:, 5] = 0.0                                                           # a label without a known row: NaN, skipped by the macro mean
    Y[:, 6] = 1.0                                                           # one class only: NaN too
    m = probe_stats.LabelMetrics(torch.as_tensor(Y, device=DEV), torch.as_tensor(M, device=DEV))(probs).cpu().numpy()
    p = probs.cpu().numpy()
    for l in range(5):
        k = M[:, l] > 0.5
        assert abs(m[l, 1] - evaluator.auroc(Y[k, l], p[l, k])) <= 1e-12 and abs(m[l, 2] - evaluator.average_precision(Y[k, l], p[l, k])) <= 1e-12
    assert np.isnan(m[5, 1]) and np.isnan(m[6, 1])
    macro = float(probe_stats.nan_mean(torch.as_tensor(m[:, 1], device=DEV)).item())
    assert abs(macro - np.mean(m[:5, 1])) <= 1e-15
    assert abs(macro - refs.macro_auroc(logits.cpu().numpy(), Y, M)) <= 1e-12
