"""GPU: the two kernels of csrc/temporal_diag.hip one by one.

`medp_counterfactual_feats` is pure data movement: BIT-EXACT (`torch.equal`) against the reference's host transforms of the raw tuples
(tuple permutation, `torch.flip`, `index_select`) followed by `oracle.duett_ref.feats_to_input` (tests/temporal_usage_refs.py), for
every way a batch can arrive (host tensors, separate device tensors, views of one stacked buffer), at V = 16, Ds = 8, max_len = 32:
equal lengths, over-length series (flip-THEN-truncate keeps other rows than truncate-then-flip), a ragged batch, a batch of one.  The
out-of-range guard is exercised with indices outside the LOGICAL range but inside the allocation, so a broken guard would show as wrong
numbers, never as an out-of-bounds read.

`medp_temporal_usage_summary` at N = 37 and 240, K = 3, S = 1, 7, 24:
  prob      an exactly widened fp32 value, non-decreasing in the logit, within 2 fp32 ulp of numpy's fp32 sigmoid (the reference's
            `_prob`; the kernel runs numpy's own fp32 arithmetic, see `test_prob_within_2_ulp_of_numpys_fp32_sigmoid`) and within
            7.04 fp32 ulp of the sigmoid evaluated in fp64: numpy states 2.52 ulp for its float32 exp, the sum and the quotient add
            half an ulp each, 3.52 * 2^-23 relative in all, and an ulp of p is at least p * 2^-24;
  sens, entropy   1e-12 against the fp64 restatement evaluated on the kernel's OWN prob: <= ~N additions of fp64 roundings of values <= 1,
            N 2^-53 ~ 3e-14, and a log / sqrt of the same order;
  two launches are bit-identical; a constant column gives a NaN correlation; S = 1 gives entropy 0; attn = null leaves `entropy` alone."""
import numpy as np
import pytest
import torch

from temporal_usage_refs import CONDITIONS, entropy_ref, feats_ref, host_conditions, make_batch, prob_ref, sens_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, DS, MAXLEN = 16, 8, 32
_state = {}


def _dtu():
    from multimodal_edema_prediction_amd import diagnose_temporal_usage
    return diagnose_temporal_usage


def _model():
    if "model" not in _state:
        from multimodal_edema_prediction_amd.main_architecture_duett import load_duett_backbone
        torch.manual_seed(0)
        _state["model"] = load_duett_backbone("synthetic", d_static_num=DS, d_time_series_num=V, n_timesteps=MAXLEN, freeze=True).cuda()
    return _state["model"]


def _place(x, where, extra_rows=0, row_len=None):
    """The batch as the caller may hold it.  "stacked": views of ONE padded device buffer per part (rows as long as the longest series, or
    `row_len`, the tail filled with a sentinel; `extra_rows` further rows behind the batch)."""
    if where == "host":
        return x
    if where == "device":
        return tuple(tuple(t.to(DEV) for t in part) for part in x)
    x_ts, x_static, bin_ends = x
    B, L = len(x_ts), row_len or max(t.shape[0] for t in x_ts)
    ts_buf = torch.full((B + extra_rows, L, 2 * V), -777.0)
    tm_buf = torch.full((B + extra_rows, L), -777.0)
    st_buf = torch.full((B + extra_rows, DS), -777.0)
    for b in range(B):
        ts_buf[b, :x_ts[b].shape[0]], tm_buf[b, :x_ts[b].shape[0]], st_buf[b] = x_ts[b], bin_ends[b], x_static[b]
    ts_buf, tm_buf, st_buf = ts_buf.to(DEV), tm_buf.to(DEV), st_buf.to(DEV)
    _state["buffers"] = (ts_buf, tm_buf, st_buf)
    return (tuple(ts_buf[b, :x_ts[b].shape[0]] for b in range(B)), tuple(st_buf[b] for b in range(B)),
            tuple(tm_buf[b, :x_ts[b].shape[0]] for b in range(B)))


def _want(x, perm, tperms, conditions):
    return {c: feats_ref(t, MAXLEN) for c, t in host_conditions(*x, perm, tperms, conditions).items()}


CASES = {
    "equal": ([32, 32, 32, 32], [2, 3, 0, 1], CONDITIONS),
    "over_length": ([50, 64, 50, 64], [2, 3, 0, 1], CONDITIONS),                       # the perm pairs equal lengths
    "ragged": ([5, 9, 3], [1, 2, 0], tuple(c for c in CONDITIONS if c != "ts_shuffle")),
    "single": ([1], [0], CONDITIONS),
}


@pytest.mark.parametrize("where", ["host", "device", "stacked"])
@pytest.mark.parametrize("case", list(CASES))
def test_counterfactual_feats_bit_exact(case, where):
    dtu, m = _dtu(), _model()
    lens, perm, conditions = CASES[case]
    x = make_batch(lens, V, DS, seed=len(lens))
    rng = np.random.default_rng(5)
    tperms = [rng.permutation(n) for n in lens]
    want = _want(x, perm, tperms, conditions)
    xin = _place(x, where)
    before = [[t.clone() for t in part] for part in xin]
    if "ts_shuffle" not in conditions:
        with pytest.raises(ValueError, match="ts_shuffle"):
            dtu.counterfactual_inputs(m, *xin, perm, tperms)
    got_st, got_ts, got_tm, got_n = dtu.counterfactual_inputs(m, *xin, perm, tperms, conditions=conditions)
    Tpad = min(max(lens), MAXLEN)
    assert got_ts.shape == (5, len(lens), Tpad, 2 * V + 1) and got_tm.shape == (5, len(lens), Tpad) and got_st.shape == (5, len(lens), DS)
    assert got_ts.dtype == got_tm.dtype == got_st.dtype == torch.float32 and got_ts.is_contiguous()
    for c, cond in enumerate(CONDITIONS):
        if cond not in conditions:
            assert got_n[c] is None
            continue
        w_st, w_ts, w_tm, w_n = want[cond]
        assert got_n[c] == w_n, cond
        assert torch.equal(got_st[c].cpu(), w_st), cond
        assert torch.equal(got_ts[c].cpu(), w_ts), cond
        assert torch.equal(got_tm[c].cpu(), w_tm), cond
    full = m.feats_to_input(xin, len(lens))                                           # the `full` block is feats_to_input's output
    assert torch.equal(got_st[0], full[0]) and torch.equal(got_ts[0], full[1]) and torch.equal(got_tm[0], full[2]) and got_n[0] == full[3]
    for part_before, part in zip(before, xin):
        for a, b in zip(part_before, part):
            assert torch.equal(a, b)                                                  # the caller's tensors are left alone
    if case == "over_length":                                                         # flip-then-truncate is not truncate-then-flip
        truncated_then_flipped = torch.flip(x[0][0][-MAXLEN:], dims=(0,))
        assert not torch.equal(got_ts[3, 0, :, :2 * V].cpu(), truncated_then_flipped)
        assert torch.equal(got_ts[3, 0, :, :2 * V].cpu(), torch.flip(x[0][0], dims=(0,))[-MAXLEN:])


def test_out_of_range_sample_perm_gives_nan_rows_only():
    """sample_perm = B names the row BEHIND the batch in a stacked buffer of B + 1 rows: logically out of range, physically allocated."""
    dtu, m = _dtu(), _model()
    lens, B = [32, 32, 32], 3
    x = make_batch(lens, V, DS, seed=11)
    tperms = [np.random.default_rng(b).permutation(n) for b, n in enumerate(lens)]
    xin = _place(x, "stacked", extra_rows=1)
    got_st, got_ts, got_tm, got_n = dtu.counterfactual_inputs(m, *xin, [1, B, 0], tperms)
    want = _want(x, [1, 1, 0], tperms, CONDITIONS)                                    # any valid stand-in for the bad entry: its rows are not compared
    for c, cond in enumerate(CONDITIONS):
        w_st, w_ts, w_tm, _ = want[cond]
        bad_ts = cond in ("patient_shuffle", "ts_shuffle")
        bad_rest = cond == "patient_shuffle"
        for b in range(B):
            affected = b == 1
            for got, w, bad, name in ((got_ts[c, b], w_ts[b], bad_ts, "xs_ts"), (got_tm[c, b], w_tm[b], bad_rest, "xs_times"),
                                      (got_st[c, b], w_st[b], bad_rest, "xs_static")):
                if affected and bad:
                    assert bool(torch.isnan(got).all()), (cond, b, name)
                else:
                    assert torch.equal(got.cpu(), w), (cond, b, name)
    assert got_n[1] == [32, 0, 32]


def test_out_of_range_time_perm_gives_one_nan_row():
    """time_perm = T_b for series of 20 steps that live in stacked rows of 40: the entry points at allocated memory behind the series."""
    dtu, m = _dtu(), _model()
    lens = [20, 20]
    x = make_batch(lens, V, DS, seed=12)
    tperms = [np.random.default_rng(b + 7).permutation(n) for b, n in enumerate(lens)]
    broken = [tperms[0].copy(), tperms[1]]
    broken[0][4] = 20
    stand_in = [tperms[0].copy(), tperms[1]]
    stand_in[0][4] = 0
    xin = _place(x, "stacked", row_len=40)
    got_st, got_ts, got_tm, _ = dtu.counterfactual_inputs(m, *xin, [1, 0], broken)
    want = _want(x, [1, 0], stand_in, CONDITIONS)
    for c, cond in enumerate(CONDITIONS):
        w_st, w_ts, w_tm, _ = want[cond]
        assert torch.equal(got_st[c].cpu(), w_st) and torch.equal(got_tm[c].cpu(), w_tm), cond
        g = got_ts[c].cpu()
        if cond == "time_permute":
            assert bool(torch.isnan(g[0, 4]).all())                                   # the whole output step, mask column included
            g, w_ts = g.clone(), w_ts.clone()
            g[0, 4], w_ts[0, 4] = 0.0, 0.0
        assert torch.equal(g, w_ts), cond


def test_counterfactual_feats_refuses_bad_arguments():
    from multimodal_edema_prediction_amd.abi import lib
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, q = t.data_ptr(), i.data_ptr()
    L = lib()
    assert L.medp_counterfactual_feats(None, None, 0, None, p, 1, None, 2, p, q, q, p, p, p, 1, 1, 1, 2, 2, 2, None) < 0       # no series
    assert L.medp_counterfactual_feats(None, p, 4, None, p, 2, None, 2, p, None, q, p, p, p, 1, 1, 1, 2, 2, 2, None) < 0        # no sample_perm
    assert L.medp_counterfactual_feats(None, p, 4, None, p, 2, None, 2, p, q, q, p, p, p, 0, 1, 1, 2, 2, 2, None) < 0           # B = 0
    assert L.medp_counterfactual_feats(None, p, 4, None, p, 2, None, 2, p, q, q, p, p, p, 1, 1, 1, 2, 3, 2, None) < 0           # Tpad > max_len
    assert L.medp_counterfactual_feats(None, p, 4, None, p, 2, None, 3, p, q, q, p, p, p, 1, 1, 1, 2, 2, 2, None) < 0           # T_uniform > Tmax


# ------------------------------------------------------------------------------------------------------------------------------
def _logits(N, K, C, seed):
    rng = np.random.default_rng(seed)
    fus = (2.5 * rng.standard_normal((C, N, K))).astype(np.float32)
    ts = (2.5 * rng.standard_normal((C, N, K))).astype(np.float32)
    fus[:, 0, :], fus[:, 1, :], fus[:, 2, :], fus[:, 3, :] = 60.0, -60.0, 50.0, -50.0      # beyond and at the clip
    fus[:, 4, :] = fus[:, 5, :]                                                            # exactly equal logits
    fus[2, :, 1] = 0.375                                                                   # a constant column
    return fus, ts


@pytest.mark.parametrize("S", [1, 7, 24])
@pytest.mark.parametrize("N", [37, 240])
def test_temporal_usage_summary(N, S):
    dtu = _dtu()
    K, C = 3, 5
    fus, ts = _logits(N, K, C, N + S)
    rng = np.random.default_rng(S)
    attn = (rng.random((N, K, S)) ** 2).astype(np.float32)
    attn[0, 0, :] = 0.0                                                                    # an all-zero row: the 1e-12 floors
    d = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    prob, sens, entropy = dtu.temporal_usage_summary(d(fus), d(ts), d(attn))
    prob2, sens2, entropy2 = dtu.temporal_usage_summary(d(fus), d(ts), d(attn))
    assert prob.shape == (2, C, K, N) and sens.shape == (C - 1, K, 3) and entropy.shape == (K,) and prob.dtype == torch.float64
    for a, b in ((prob, prob2), (sens, sens2), (entropy, entropy2)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))                      # bit-identical, NaN included
    p = prob.cpu().numpy()
    for h, z in enumerate((fus, ts)):
        exact = (1.0 / (1.0 + np.exp(-np.clip(z.astype(np.float64), -50.0, 50.0)))).transpose(0, 2, 1)      # [C, K, N]
        got32 = p[h].astype(np.float32)
        assert np.array_equal(got32.astype(np.float64), p[h])                              # an fp32 value, widened
        ulps = np.abs(p[h] - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
        print(f"N={N} S={S} half {h}: prob within {ulps.max():.3f} fp32 ulp of the fp64 sigmoid (bound 7.04)")
        assert ulps.max() <= 7.04
        order = np.argsort(z.transpose(0, 2, 1), axis=-1, kind="stable")
        assert (np.diff(np.take_along_axis(p[h], order, -1), axis=-1) >= 0).all()          # non-decreasing in the logit
    assert np.array_equal(p[0][:, :, 4], p[0][:, :, 5]) and np.array_equal(p[0][:, :, 0], p[0][:, :, 2])     # equal logits, clipped logits
    want_sens, want_entropy = sens_ref(p[0], p[1]), entropy_ref(attn)
    s, e = sens.cpu().numpy(), entropy.cpu().numpy()
    assert np.isnan(s[1, 1, 1]) and np.isnan(want_sens[1, 1, 1])                           # the constant column: NaN correlation
    assert np.array_equal(np.isnan(s), np.isnan(want_sens))
    print(f"N={N} S={S}: sens {np.nanmax(np.abs(s - want_sens)):.3e}, entropy {np.abs(e - want_entropy).max():.3e} (bound 1e-12)")
    np.testing.assert_allclose(s, want_sens, rtol=0, atol=1e-12)
    np.testing.assert_allclose(e, want_entropy, rtol=0, atol=1e-12)
    if S == 1:
        assert (e == 0.0).all()                                                            # max(log S, 1e-12): 0 / 1e-12
    # attn = null: the entropy buffer is left alone
    sentinel = torch.full((K,), -3.0, dtype=torch.float64, device=DEV)
    prob3, sens3, same = dtu.temporal_usage_summary(d(fus), d(ts), None, entropy=sentinel)
    assert same is sentinel and (sentinel == -3.0).all() and torch.equal(prob3, prob)
    assert torch.equal(sens3.view(torch.int64), sens.view(torch.int64))


@pytest.mark.parametrize("N", [37, 240])
def test_prob_within_2_ulp_of_numpys_fp32_sigmoid(N):
    """The bound the feature's issue sets: `prob` within 2 fp32 ulp of numpy's fp32 sigmoid 1 / (1 + exp(-clip(z))), the reference's `_prob`.
    numpy's float32 `exp` is itself up to 2.52 ulp from the exact exponential, so neither the device library's expf (measured 3.00 ulp
    from numpy's sigmoid) nor an fp64 evaluation rounded once (3.00 ulp at N = 240, 1 of 7200 values beyond 2) meets it.  The kernel
    therefore runs numpy's own algorithm (reduction by ln 2 in two pieces, a 5 / 2 rational in fused multiply-adds, IEEE quotient,
    sum and quotient in fp32): where numpy takes its SIMD loop (x86 with FMA) the values are numpy's bit for bit, which a numpy
    restatement of that loop confirms on 6 million logits; elsewhere numpy calls the C library's expf, within an ulp of it."""
    K, C = 3, 5
    fus, ts = _logits(N, K, C, N + 1)
    d = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    p = _dtu().temporal_usage_summary(d(fus), d(ts))[0].cpu().numpy()
    worst = 0.0
    for h, z in enumerate((fus, ts)):
        want = prob_ref(z).transpose(0, 2, 1)
        ulps = np.abs(p[h] - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        print(f"N={N} half {h}: prob within {ulps.max():.2f} fp32 ulp of numpy's fp32 sigmoid ({int((ulps > 0).sum())} of {ulps.size} differ at all)")
        worst = max(worst, float(ulps.max()))
    assert worst <= 2.0


def test_temporal_usage_summary_single_row_and_limits():
    dtu = _dtu()
    from multimodal_edema_prediction_amd.abi import lib
    z = torch.tensor([[[0.5, -1.0]], [[0.25, 2.0]]], device=DEV)                           # C = 2, N = 1, K = 2
    prob, sens, _ = dtu.temporal_usage_summary(z, z)
    assert bool(torch.isnan(sens[0, :, 1]).all())                                          # N < 2: no correlation
    want = (prob[0, 0, :, 0] - prob[0, 1, :, 0]).abs()
    assert torch.equal(sens[0, :, 0], want) and torch.equal(sens[0, :, 2], want)          # one row: the mean is the value
    only = dtu.temporal_usage_summary(z[:1], z[:1])                                        # C = 1: probabilities only
    assert only[0].shape == (2, 1, 2, 1) and only[1].shape == (0, 2, 3) and torch.equal(only[0][:, 0], prob[:, 0])
    p, q = z.data_ptr(), prob.data_ptr()
    L = lib()
    assert L.medp_temporal_usage_summary(p, p, None, q, q, None, 2, dtu.SUMMARY_MAX_N + 1, 2, 0, None) < 0
    assert L.medp_temporal_usage_summary(p, p, p, q, q, q, 2, 1, 2, dtu.SUMMARY_MAX_S + 1, None) < 0
    assert L.medp_temporal_usage_summary(p, p, p, q, q, None, 2, 1, 2, 1, None) < 0       # attention without an entropy buffer
    assert L.medp_temporal_usage_summary(None, p, None, q, q, None, 2, 1, 2, 0, None) < 0
    assert L.medp_temporal_usage_summary(p, p, None, q, q, None, 2, 0, 2, 0, None) < 0
    with pytest.raises(TypeError):
        dtu.temporal_usage_summary(z.double(), z.double())
