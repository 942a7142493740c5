"""GPU: the two kernels of csrc/complementarity.hip against the reference's fixture (tests/golden/complementarity.npz) and, at the
sizes the fixture has no entry for, against the numpy restatement the CPU suite pins on that fixture (tests/complementarity_refs.py).

Every comparison is EXACT: thresholds are one of the input scores (or +inf / NaN), J is the same two fp64 quotients and one difference
sklearn computes, counts are integers.  A tolerance would hide exactly the tie cases the kernel exists to get right.  A zero threshold
is compared with its sign: the kernel reports the zero of the first known row, as sklearn's stable sort does, and the recorded report
text prints it."""
import numpy as np
import pytest
import torch

from complementarity_refs import cells_ref, golden_cases, same_bits, youden_ref, youden_table_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _comp():
    from multimodal_edema_prediction_amd import complementarity
    return complementarity


def _d(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _launch(scores, y, mask):
    thr, j, counts = _comp().youden_thresholds(_d(scores), _d(y), _d(mask))
    return thr.cpu().numpy(), j.cpu().numpy(), counts.cpu().numpy()


def _assert_table(got, want, what):
    for name, a, b in zip(("thr", "youden_j"), got[:2], want[:2]):
        bad = [(i, x, w) for i, (x, w) in enumerate(zip(a.ravel(), b.ravel())) if not same_bits(x, w)]
        assert not bad, f"{what}: {name} differs at (flat index, got, want) {bad[:5]}"
    assert np.array_equal(got[2], want[2]), f"{what}: counts"


def test_every_fixture_case_in_one_launch():
    """All cases side by side as labels of one launch (padding rows masked out); head 1 holds the negated scores."""
    cases = golden_cases()
    N, K = max(len(c["z"]) for c in cases), len(cases)
    z, y, mask = np.zeros((N, K), np.float32), np.zeros((N, K), np.float32), np.zeros((N, K), np.float32)
    for k, c in enumerate(cases):
        n = len(c["z"])
        z[:n, k], y[:n, k], mask[:n, k] = c["z"], c["y"], c["mask"]
    thr, j, counts = _launch(np.stack([z, -z]), y, mask)
    for k, c in enumerate(cases):
        print(f"case {k}: thr {thr[0, k]} (reference {c['thr']}), J {j[0, k]} (reference {c['j']})")
        assert same_bits(thr[0, k], c["thr"]) and same_bits(j[0, k], c["j"]), k
        assert counts[k, 0] == int((c["mask"] != 0).sum())
    _assert_table((thr, j, counts), youden_table_ref(np.stack([z, -z]), y, mask), "fixture cases, both signs")
    assert thr[0, 0] == 1.5 and thr[0, 1] == 0.5                                  # the drop rule and the fp64 rounding, the issue's two cases


def test_every_fixture_case_alone():
    for k, c in enumerate(golden_cases()[:16]):                                   # the issue's and the hand-made ones, N as small as 2
        thr, j, counts = _launch(c["z"][None, :, None], c["y"][:, None], c["mask"][:, None])
        assert same_bits(thr[0, 0], c["thr"]) and same_bits(j[0, 0], c["j"]), k


@pytest.mark.parametrize("known", [1, 2, 1023, 1024, 1025, 2049, 16384])
def test_padding_and_range_edges_with_long_tie_groups(known):
    """~8 distinct scores: tie groups span many threads' ranges; 37 masked rows are interleaved, so N differs from the sorted length
    (at 16384 known rows N is above the sort limit and the known rows are counted first)."""
    rng = np.random.default_rng(known)
    N, K = known + 37, 2
    mask = np.ones((N, K), np.float32)
    for k in range(K):
        mask[rng.choice(N, 37, replace=False), k] = 0.0
    y = (rng.random((N, K)) < 0.4).astype(np.float32)
    levels = np.array([-1.5, -0.75, -0.0, 0.0, 0.25, 0.5, 1.0, 2.0, 3.5], np.float32)
    scores = np.stack([levels[np.clip(np.round(2.0 * y + h + 1.5 * rng.standard_normal((N, K))).astype(int) + 3, 0, 8)] for h in range(3)])
    scores[2] = -scores[2]                                                        # an anti-predictive head
    got, want = _launch(scores, y, mask), youden_table_ref(scores, y, mask)
    print(f"known = {known}: thr {got[0].tolist()} J {got[1].tolist()}")
    _assert_table(got, want, f"known = {known}")
    assert (got[2][:, 0] == known).all()
    if known >= 1023:
        assert np.isfinite(got[0][:2]).all() and np.isinf(got[0][2]).all() and (got[1][2] == 0.0).all()
    if known == 1:
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all()


def test_many_distinct_scores_across_thread_ranges():
    """Gridded scores with a few hundred distinct values at a length that is no multiple of anything: group ends whose neighbours
    (the drop rule) lie in other threads' ranges."""
    rng = np.random.default_rng(3)
    N, K = 5003, 3
    y = (rng.random((N, K)) < 0.5).astype(np.float32)
    mask = (rng.random((N, K)) < 0.9).astype(np.float32)
    scores = np.stack([(np.round((0.4 * y + rng.standard_normal((N, K))) * g) / g).astype(np.float32) for g in (4.0, 32.0, 4096.0)])
    _assert_table(_launch(scores, y, mask), youden_table_ref(scores, y, mask), "N = 5003")


def test_degenerate_inputs():
    f = lambda *a: np.array(a, dtype=np.float32)  # noqa: E731
    one = np.ones(6, np.float32)
    table = {
        "single distinct score": (f(.25, .25, .25, .25, .25, .25), f(1, 0, 1, 0, 0, 1), one, float("inf"), 0.0),
        "anti-predictive": (f(-1, 1, -2, 2, -3, 3), f(1, 0, 1, 0, 1, 0), one, float("inf"), 0.0),
        "mask removes a class": (f(1, 2, 3, 4, 5, 6), f(1, 0, 1, 0, 1, 0), f(1, 0, 1, 0, 1, 0), float("nan"), float("nan")),
        "signed zeros": (f(-0.0, 0.0, -1, -1, -0.0, 0.0), f(1, 1, 0, 0, 1, 0), one, -0.0, 1.0 - 1 / 3),      # the first zero row is -0.0
        "NaN score": (f(1, 2, np.nan, 4, 5, 6), f(1, 0, 1, 0, 1, 0), one, float("nan"), float("nan")),
        "infinite score": (f(1, 2, np.inf, 4, 5, 6), f(1, 0, 1, 0, 1, 0), one, float("nan"), float("nan")),
        "NaN score masked out": (f(1, 2, np.nan, 4, 5, 6), f(0, 0, 1, 1, 1, 0), f(1, 1, 0, 1, 1, 1), 4.0, 1.0 - 1 / 3),
    }
    for name, (z, y, mask, thr_want, j_want) in table.items():
        thr, j, _ = _launch(z[None, :, None], y[:, None], mask[:, None])
        ref = youden_ref(z, y, mask)
        print(f"{name}: thr {thr[0, 0]} J {j[0, 0]}")
        assert same_bits(thr[0, 0], thr_want) and same_bits(j[0, 0], j_want), name
        assert same_bits(ref[0], thr_want) and same_bits(ref[1], j_want), name
    comp = _comp()
    z, y, mask = table["NaN score"][:3]
    data = {"img": _d(z[:, None]), "ts": _d(np.zeros((6, 1), np.float32)), "fus": _d(np.zeros((6, 1), np.float32)), "y": _d(y[:, None]),
            "mask": _d(mask[:, None])}
    with pytest.raises(ValueError, match="NaN or infinity"):
        comp.derive_thresholds(data, "youden")


def test_over_the_sort_limit_is_refused_without_a_launch():
    comp = _comp()
    n = comp.YOUDEN_MAX_LEN + 1
    rng = np.random.default_rng(0)
    scores, y = _d(rng.standard_normal((1, n, 1)).astype(np.float32)), _d((rng.random((n, 1)) < 0.5).astype(np.float32))
    with pytest.raises(ValueError, match="sort limit"):
        comp.youden_thresholds(scores, y, torch.ones((n, 1), device=DEV))
    mask = torch.ones((n, 1), device=DEV)
    mask[5, 0] = 0.0                                                              # one row fewer known: the same N is served
    thr, j, counts = comp.youden_thresholds(scores, y, mask)
    want = youden_ref(scores.cpu().numpy()[0, :, 0], y.cpu().numpy()[:, 0], mask.cpu().numpy()[:, 0])
    assert same_bits(thr.item(), want[0]) and same_bits(j.item(), want[1]) and counts.cpu().numpy().tolist() == [[n - 1, want[3]]]


def test_two_launches_are_bit_identical():
    rng = np.random.default_rng(9)
    N, K = 3000, 4
    scores = _d((np.round(rng.standard_normal((3, N, K)) * 8) / 8).astype(np.float32))
    y, mask = _d((rng.random((N, K)) < 0.3).astype(np.float32)), _d((rng.random((N, K)) < 0.8).astype(np.float32))
    a, b = _comp().youden_thresholds(scores, y, mask), _comp().youden_thresholds(scores, y, mask)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v)


@pytest.mark.parametrize("N", [1, 257, 4099])
def test_cells_are_the_exact_counts(N):
    rng = np.random.default_rng(N)
    K = 5
    scores = (np.round(rng.standard_normal((3, N, K)) * 4) / 4).astype(np.float32)
    y = (rng.random((N, K)) < 0.45).astype(np.float32)
    mask = (rng.random((N, K)) < 0.8).astype(np.float32)
    mask[:, 3] = 0.0                                                              # a label without known rows
    thr = np.array([[0.25, float("nan"), -0.5, 0.0, float("inf")], [float("inf"), 0.3, 0.25, 1.0, float("nan")],
                    [0.1, -0.25, float("nan"), 0.5, -float("inf")]])              # ties with the grid (0.25, -0.5, 0.0), NaN, both infinities
    got = _comp().complementarity_cells(_d(scores), _d(y), _d(mask), _d(thr)).cpu().numpy()
    want = cells_ref(scores, y, mask, thr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(got.sum(1), (mask != 0).sum(0)) and got[3].sum() == 0
    again = _comp().complementarity_cells(_d(scores), _d(y), _d(mask), _d(thr)).cpu().numpy()
    assert np.array_equal(got, again)
