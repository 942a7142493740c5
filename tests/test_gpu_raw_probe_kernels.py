"""GPU: the two kernels of csrc/raw_probe.hip and the metrics kernel of csrc/binary_metrics.hip against their numpy restatement
(tests/raw_probe_refs.py, itself pinned on the reference's outputs by tests/test_raw_probe_refs_cpu.py), and the shared resampling
of probe_stats.py on top of the metrics kernel.

Tolerances (fp64 everywhere; kernel and restatement differ in summation order and in libm's exp / log / log1p by an ulp or two):
  summaries  sums of T <= 96 terms of magnitude <= ~1e3 (count * value): 96 * 1.1e-16 * 1e3 ~ 1e-11 absolute, amplified by the
             condition of the centred std / slope forms (<= 1e2 on this data): RTOL = 1e-9, ATOL = 1e-9.  NaN positions and the
             statistics without accumulation (last, min, max, delta, the two fractions, time_since_last) are exact.
  valgrad    scores are dot products of F <= 20000 terms with sum |x w| <= ~1e2, objectives / gradients means over n <= 333 rows of
             terms <= ~1e2: (F + n) * 1.1e-16 * 1e2 ~ 2e-10: RTOL = ATOL = 1e-9.  Two runs are bit-identical.
  metrics    BCE is a mean of L <= 16384 terms <= 16.2 (= -log 1e-7): L * 1.1e-16 * 16.2 ~ 3e-11; AUPRC a sum of <= L terms <= 1
             (2e-12); AUROC is an exact integer ratio in the kernel, a half-integer rank sum in the restatement (ulps):
             RTOL = ATOL = 1e-10."""
import numpy as np
import pytest
import torch

from raw_probe_refs import (EXACT_STATS, METRICS_MAX_LEN, STATS, binary_metrics_ref, offset_logistic_valgrad_ref, raw_traj_summary_ref,
                            resampled_binary_metrics_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rp():
    from multimodal_edema_prediction_amd import raw_trajectory_probe
    return raw_trajectory_probe


def _ps():
    from multimodal_edema_prediction_amd import probe_stats
    return probe_stats


def _abi():
    from multimodal_edema_prediction_amd import abi
    return abi


# ---------------------------------------------------------------------------------------------------------------------------
def _synth_x(B, T, V, seed):
    rng = np.random.default_rng(seed)
    val = (80.0 + 25.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    cnt = np.where(rng.random((B, T, V)) < 0.5, 1 + rng.poisson(0.7, (B, T, V)), 0).astype(np.float32)
    val[rng.random((B, T, V)) < 0.05] = np.nan                        # observed-but-NaN (where the count is positive) or plain junk
    val[rng.random((B, T, V)) < 0.02] = np.inf
    cnt[rng.random((B, T, V)) < 0.02] = np.nan
    cnt[rng.random((B, T, V)) < 0.02] = -1.0
    if V > 1:
        cnt[0, :, 1] = 0.0                                               # never observed
    if V > 2 and T > 1:
        cnt[0, :, 2] = 0.0
        cnt[0, T // 2, 2], val[0, T // 2, 2] = 2.0, 71.5                 # a single observation
    return np.concatenate([val, cnt], axis=2)


@pytest.mark.parametrize("B,T,V,recent", [(3, 24, 3, 6), (2, 5, 5, 5), (1, 1, 1, 1), (4, 96, 48, 6)])
def test_raw_traj_summary(B, T, V, recent):
    x = _synth_x(B, T, V, seed=B * 1000 + T)
    want = raw_traj_summary_ref(x, recent)
    got = _rp().raw_traj_summary(torch.as_tensor(x, device=DEV), recent).cpu().numpy()
    assert got.shape == (B, V, 14) and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for k, name in enumerate(STATS):
        if name in EXACT_STATS:
            assert np.array_equal(got[..., k], want[..., k], equal_nan=True), name
        else:
            np.testing.assert_allclose(got[..., k], want[..., k], rtol=1e-9, atol=1e-9, equal_nan=True, err_msg=name)


def test_raw_traj_summary_rejects_a_bad_recent_window():
    x = torch.zeros((2, 6, 4), device=DEV)
    for recent in (0, 7, -1):
        with pytest.raises(ValueError, match="recent_hours"):
            _rp().raw_traj_summary(x, recent)
    assert _rp().raw_traj_summary(x, 6).shape == (2, 2, 14)


# ---------------------------------------------------------------------------------------------------------------------------
def _valgrad_case(n, F, G, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)) / np.sqrt(F)
    y = (rng.random(n) < 0.5).astype(np.float64)
    offset = rng.choice([-40.0, 40.0, 0.3, -1.7], size=n)               # +-40: logaddexp / expit must not overflow or cancel
    W = 0.7 * rng.standard_normal((F, G))
    l2 = 10.0 ** rng.integers(-4, 3, G).astype(np.float64)
    return X, y, offset, W, l2


# F = 20000: a row longer than the LDS budget, the unstaged path
@pytest.mark.parametrize("n,F", [(n, F) for n in (1, 5, 64, 333) for F in (1, 7, 130, 1344)] + [(5, 20000), (64, 20000)])
def test_offset_logistic_valgrad(n, F):
    rp = _rp()
    for G in (1, 5, 8):
        X, y, offset, W, l2 = _valgrad_case(n, F, G, seed=n * 7 + F + G)
        want_obj, want_grad = offset_logistic_valgrad_ref(X, y, offset, W, l2)
        d = [torch.as_tensor(a, device=DEV) for a in (X, y, offset, W, l2)]
        obj, grad = rp.offset_logistic_valgrad(*d)
        obj2, grad2 = rp.offset_logistic_valgrad(*d)
        assert torch.equal(obj, obj2) and torch.equal(grad, grad2)        # two-stage reduction in a fixed order: bit-stable
        np.testing.assert_allclose(obj.cpu().numpy(), want_obj, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(grad.cpu().numpy(), want_grad, rtol=1e-9, atol=1e-9)
        assert np.isfinite(want_obj).all() and np.isfinite(want_grad).all()


def test_offset_logistic_valgrad_reads_a_strided_design_matrix():
    rp = _rp()
    X, y, offset, W, l2 = _valgrad_case(37, 19, 3, seed=5)
    wide = torch.full((37, 32), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :19] = torch.as_tensor(X, device=DEV)
    obj, grad = rp.offset_logistic_valgrad(wide[:, :19], *[torch.as_tensor(a, device=DEV) for a in (y, offset, W, l2)])
    want_obj, want_grad = offset_logistic_valgrad_ref(X, y, offset, W, l2)
    np.testing.assert_allclose(obj.cpu().numpy(), want_obj, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(grad.cpu().numpy(), want_grad, rtol=1e-9, atol=1e-9)


def test_offset_logistic_valgrad_rejects_bad_shapes():
    abi = _abi()
    L = abi.lib()
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = abi.ptr(t)
    assert L.medp_offset_logistic_ws_bytes(4, 2, 0) == 0 and L.medp_offset_logistic_ws_bytes(4, 2, 9) == 0
    assert L.medp_offset_logistic_ws_bytes(0, 2, 1) == 0 and L.medp_offset_logistic_ws_bytes(4, 0, 1) == 0
    for n, F, G in ((4, 2, 0), (4, 2, 9), (0, 2, 1), (4, 0, 1)):
        assert L.medp_offset_logistic_valgrad(p, 2, p, p, p, p, p, p, p, 512, n, F, G, abi.stream()) < 0
    assert L.medp_offset_logistic_valgrad(p, 1, p, p, p, p, p, p, p, 512, 4, 2, 1, abi.stream()) < 0          # ldx < F
    assert L.medp_offset_logistic_valgrad(p, 2, p, p, p, p, p, p, p, 8, 4, 2, 1, abi.stream()) < 0            # workspace too small
    with pytest.raises(ValueError):
        _rp().valgrad_workspace(4, 2, 9, DEV)


# ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 1000, 0, METRICS_MAX_LEN, 5, 6)            # 0: the empty replicate; the last two: one class only


def _metrics_case(N, seed, quantised):
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.35).astype(np.uint8)
    p = rng.integers(0, 4, N) / 4.0 + 0.1 if quantised else rng.random(N)
    p[:3] = (0.0, 1.0, 1e-9)                                             # outside the clip
    parts = [rng.integers(0, N, L) for L in LENGTHS[:-2]]
    parts += [rng.choice(np.flatnonzero(y == 1), LENGTHS[-2]), rng.choice(np.flatnonzero(y == 0), LENGTHS[-1])]
    offsets = np.cumsum([0] + [len(a) for a in parts]).astype(np.int64)
    return y, p, np.concatenate(parts).astype(np.int32), offsets


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("per_replicate_p", [False, True])
def test_resampled_binary_metrics_with_a_ragged_gather(quantised, per_replicate_p):
    N, R = 3000, len(LENGTHS)
    y, p, idx, offsets = _metrics_case(N, seed=11 + quantised, quantised=quantised)
    P = np.stack([np.roll(p, r) for r in range(R)]) if per_replicate_p else p[None]
    want = resampled_binary_metrics_ref(y, P, idx, offsets)
    d = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    got = _ps().resampled_binary_metrics(d(y), d(P), d(idx), d(offsets), max_len=max(LENGTHS)).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10, equal_nan=True)
    assert np.isnan(got[LENGTHS.index(0)]).all()                         # the empty replicate: NaN, NaN, NaN by definition
    for r in (R - 2, R - 1):                                             # one class only: AUROC / AUPRC NaN, BCE finite
        assert np.isfinite(got[r, 0]) and np.isnan(got[r, 1:]).all()
    assert np.isnan(got[0, 1]) and np.isfinite(got[0, 0])                # length 1 is one class too
    again = _ps().resampled_binary_metrics(d(y), d(P), d(idx), d(offsets), max_len=max(LENGTHS))
    assert np.array_equal(again.cpu().numpy(), got, equal_nan=True)


@pytest.mark.parametrize("N,Rp", [(1000, 3), (65, 1), (2, 2), (1025, 1), (2049, 2)])   # the last two: L < M, 2 and 4 positions per thread
def test_resampled_binary_metrics_identity(N, Rp):
    rng = np.random.default_rng(N)
    y = (rng.random(N) < 0.5).astype(np.uint8)
    y[:2] = (0, 1)
    P = np.round(rng.random((Rp, N)), 1)                                 # ties
    want = resampled_binary_metrics_ref(y, P)
    got = _ps().resampled_binary_metrics(torch.as_tensor(y, device=DEV), torch.as_tensor(P, device=DEV)).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)


def test_resampled_binary_metrics_limit_and_bad_index():
    abi, rp = _abi(), _ps()
    N = 50
    y = torch.zeros(N, dtype=torch.uint8, device=DEV)
    y[::2] = 1
    p = torch.linspace(0.05, 0.95, N, dtype=torch.float64, device=DEV)[None]
    idx = torch.zeros(METRICS_MAX_LEN + 1, dtype=torch.int32, device=DEV)
    offsets = torch.tensor([0, METRICS_MAX_LEN + 1], dtype=torch.int64, device=DEV)
    out = torch.full((1, 3), 7.0, dtype=torch.float64, device=DEV)
    rc = abi.lib().medp_resampled_binary_metrics(abi.ptr(y), abi.ptr(p), abi.ptr(idx), abi.ptr(offsets), abi.ptr(out), N, 1, 1,
                                                 METRICS_MAX_LEN + 1, abi.stream())
    torch.cuda.synchronize()
    assert rc < 0 and bool((out == 7.0).all())                           # refused before any launch
    with pytest.raises(ValueError, match="limit"):
        rp.resampled_binary_metrics(y, p, idx, offsets)
    with pytest.raises(ValueError):                                      # Rp is neither 1 nor R
        rp.resampled_binary_metrics(y, p.expand(2, N).contiguous(), idx[:6], torch.tensor([0, 2, 4, 6], dtype=torch.int64, device=DEV))
    # an index outside [0, N) is never dereferenced: that replicate is NaN, its neighbour is untouched
    idx = torch.tensor([0, 1, 2, 3, 0, N, 2, 3], dtype=torch.int32, device=DEV)
    offsets = torch.tensor([0, 4, 8], dtype=torch.int64, device=DEV)
    got = rp.resampled_binary_metrics(y, p, idx, offsets).cpu().numpy()
    assert np.isfinite(got[0]).all() and np.isnan(got[1]).all()
    # a replicate longer than the max_len the caller declared is refused on the device, not sorted past the staged size
    got = rp.resampled_binary_metrics(y, p, idx, offsets, max_len=2).cpu().numpy()
    assert np.isnan(got).all()


# ---------------------------------------------------------------------------------------------------------------------------
CI_KEYS = [f"{m}_gain_ci_{side}" for m in ("bce", "auroc", "auprc") for side in ("low", "high")]
PERM_KEYS = [f"perm_{m}_{s}" for m in ("bce", "auroc", "auprc") for s in ("mean", "low", "high")]


def _stats_case():
    """n = 65 rows (one past a wave; 128 sort keys), R = 5 replicates: y has both classes, rows 10 / 20 / 30 tie in both probability
    vectors, replicate 4 draws positives only."""
    n, R = 65, 5
    rng = np.random.default_rng(65)
    y = (rng.random(n) < 0.4).astype(np.int64)
    y[:2] = (0, 1)
    base, probe = rng.random(n), rng.random(n)
    base[[10, 20, 30]], probe[[10, 20, 30]] = 0.5, 0.625
    index = np.stack([rng.integers(0, n, n) for _ in range(R)]).astype(np.int32)
    index[1, :2] = (0, 1)                                                # both classes in the two rows the ragged form keeps of it
    index[2] = rng.permutation(n)                                        # holds the whole tie group
    index[4] = rng.choice(np.flatnonzero(y == 1), n)
    return y, base, probe, index


def _gains_ref(y, base, probe, replicates):
    mb = np.array([binary_metrics_ref(y[i], base[i]) for i in replicates])
    mp = np.array([binary_metrics_ref(y[i], probe[i]) for i in replicates])
    both = ~np.isnan(mb[:, 1])
    want = {}
    for name, v in (("bce_gain", mb[:, 0] - mp[:, 0]), ("auroc_gain", (mp[:, 1] - mb[:, 1])[both]), ("auprc_gain", (mp[:, 2] - mb[:, 2])[both])):
        want[f"{name}_ci_low"], want[f"{name}_ci_high"] = np.percentile(v, [2.5, 97.5])
    return want, both


def test_shared_resampling_statistics():
    """probe_stats on the metrics kernel.  `paired_bootstrap_gains` returns intervals only, so the two forms of the index matrix are
    compared on the replicates they share in two ways: the per-replicate kernel outputs at the shared positions of the two tables,
    and the intervals of the shared replicates alone in either encoding.  Bounds: 1e-12 for one triple of 65 terms <= 16.2
    (65 * 1.1e-16 * 16.2 ~ 1e-13), 1e-10 for the intervals (the bound of the metrics-kernel tests; percentiles interpolate linearly)."""
    ps = _ps()
    y, base, probe, index = _stats_case()
    n, R = index.shape[1], len(index)
    dev = torch.device(DEV)
    d = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    # one triple: host array and device tensor
    for p in (base, probe):
        host, device = ps.binary_metrics(y, p, dev), ps.binary_metrics(y, d(p))
        want = binary_metrics_ref(y, p)
        print("binary_metrics", host, "deviation from the restatement", np.abs(np.array(list(host.values())) - want).max())
        assert list(host) == list(device) == ["bce", "auroc", "auprc"]
        assert all(host[k] == device[k] for k in host) and np.isfinite(list(host.values())).all()
        np.testing.assert_allclose(list(host.values()), want, rtol=1e-12, atol=1e-12)
    one = ps.binary_metrics(y[index[4]], d(base[index[4]]))                # one class: BCE only, NaN at the same places in both forms
    assert np.isfinite(one["bce"]) and np.isnan(one["auroc"]) and np.isnan(one["auprc"])
    assert np.array_equal(np.isnan(list(ps.binary_metrics(y[index[4]], base[index[4]], dev).values())), [False, True, True])
    # the intervals: rectangular and ragged index tables
    rect_off = torch.arange(0, (R + 1) * n, n, dtype=torch.int64, device=dev)
    rect = ps.paired_bootstrap_gains(y, base, probe, index.reshape(-1), rect_off, n, dev)
    ragged_rows = [index[0][:64], index[1][:2], index[2], index[3], index[4]]
    ragged_idx = np.concatenate(ragged_rows)
    ragged_off = np.cumsum([0] + [len(r) for r in ragged_rows]).astype(np.int64)
    ragged = ps.paired_bootstrap_gains(y, base, probe, ragged_idx, ragged_off, 65, dev)
    for name, got, replicates in (("rectangular", rect, list(index)), ("ragged", ragged, ragged_rows)):
        want, both = _gains_ref(y, base, probe, replicates)
        assert both.tolist() == [True, True, True, True, False] and list(got) == list(want) == CI_KEYS
        print(name, got, "largest deviation", np.abs(np.array(list(got.values())) - np.array(list(want.values()))).max())
        np.testing.assert_allclose(list(got.values()), list(want.values()), rtol=1e-10, atol=1e-10)
    shared = slice(2, 5)
    for p in (base, probe):                                               # the shared replicates, at other offsets beside other neighbours
        a = ps.resampled_binary_metrics(d(y.astype(np.uint8)), d(p[None]), d(index.reshape(-1)), rect_off, n).cpu().numpy()
        b = ps.resampled_binary_metrics(d(y.astype(np.uint8)), d(p[None]), d(ragged_idx), d(ragged_off), 65).cpu().numpy()
        assert np.array_equal(a[shared], b[shared], equal_nan=True) and np.isnan(a[4, 1:]).all() and np.isfinite(a[:4]).all()
    shared_rect = ps.paired_bootstrap_gains(y, base, probe, index[shared].reshape(-1), rect_off[:4], n, dev)
    shared_ragged = ps.paired_bootstrap_gains(y, base, probe, ragged_idx[ragged_off[2]:], ragged_off[2:] - ragged_off[2], 65, dev)
    assert list(shared_rect.values()) == list(shared_ragged.values()) and np.isfinite(list(shared_rect.values())).all()
    # no replicate
    for nothing in (None, torch.empty((0, n), dtype=torch.float64, device=dev)):
        empty = ps.permutation_summary(y, nothing)
        assert list(empty) == PERM_KEYS and all(np.isnan(v) for v in empty.values())
    none = ps.paired_bootstrap_gains(y, base, probe, np.zeros(0, np.int32), np.zeros(1, np.int64), 0, dev)
    assert list(none) == CI_KEYS and all(np.isnan(v) for v in none.values())
