"""The host replica of the kernels' dropout masks (tests/dropout_twin.py), without a GPU: keep rates, independence between
neighbouring indices, stream ids, seeds and RNG epochs, and between the 15 dropout sites of one perceiver forward.  Every bound
is 5 sigma of a binomial count.  test_gpu_dropout.py checks that the kernels draw these very masks."""
import itertools
import math

import numpy as np
import pytest

import dropout_twin as T

N = 1 << 22
PAIRS = [(0, 0), (123, 5), (2 ** 31 - 2, 42), (987654321, 100), (7, 255)]


def _within(k: int, n: int, q: float, what: str):
    sigma = math.sqrt(q * (1 - q) / n)
    assert abs(k / n - q) <= 5 * sigma, f"{what}: rate {k / n:.6f}, expected {q:.6f} +- 5 x {sigma:.2e}"


def test_scale_is_the_launchers_fp32_value():
    for p in (0.1, 0.2, 0.25, 0.5):
        assert T.scale(p) == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(p))
        assert T.scale(p).dtype == np.float32
    assert T.scale(0.0) == np.float32(1.0)


def test_replica_matches_a_hand_evaluated_hash():
    """The C expressions of common.h evaluated on Python integers reduced modulo 2^32, so a numpy promotion cannot slip in."""
    def c_hash(seed, sid, idx):
        m = 0xFFFFFFFF
        x = ((idx * 0x9E3779B1) & m) ^ ((seed + 0x7F4A7C15 * (sid + 1)) & m)
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & m
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & m
        x ^= x >> 16
        x = (x + seed * 0x27D4EB2F) & m
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & m
        x ^= x >> 12
        return x

    idx = np.array([0, 1, 977, 2 ** 31 + 5, 2 ** 32 - 1], dtype=np.int64)
    for seed, sid in PAIRS:
        for ep in (None, 0, 1, 7, 2 ** 31 - 1):
            s = seed if ep is None else (seed + ep * 0x9E3779B9) & 0xFFFFFFFF
            assert int(T.mix_epoch(seed, ep)) == s
            got = T.medp_hash(T.mix_epoch(seed, ep), sid, idx)
            assert got.dtype == np.uint32
            assert [int(v) for v in got] == [c_hash(s, sid, int(i)) for i in idx]


def test_p_zero_keeps_everything():
    idx = T.flat_index((1 << 16,))
    for seed, sid in PAIRS:
        assert T.keep_mask(seed, sid, idx, 0.0).all()
        assert (T.mask_scale(seed, sid, idx, 0.0) == 1.0).all()


@pytest.mark.parametrize("seed,sid", PAIRS)
def test_keep_rate(seed, sid):
    u = T.uniform(seed, sid, T.flat_index((N,)))
    for p in (0.1, 0.2, 0.5):
        _within(int((u >= np.float32(p)).sum()), N, 1 - p, f"keep rate p={p} seed={seed} sid={sid}")


@pytest.mark.parametrize("seed,sid", PAIRS[1:4])
def test_joint_keep_rates(seed, sid):
    """Pairs that a weak hash would correlate: adjacent indices, neighbouring stream ids, neighbouring seeds, neighbouring epochs."""
    idx = T.flat_index((N,))
    u = T.uniform(seed, sid, idx)
    others = {"sid, sid + 1": T.uniform(seed, sid + 1, idx), "seed, seed + 1": T.uniform(seed + 1, sid, idx)}
    ue = [T.uniform(seed, sid, idx, e) for e in range(3)]
    for p in (0.1, 0.2, 0.5):
        q, pf = (1 - p) ** 2, np.float32(p)
        a = u >= pf
        _within(int((a[1:] & a[:-1]).sum()), N - 1, q, f"adjacent indices p={p}")
        for what, v in others.items():
            _within(int((a & (v >= pf)).sum()), N, q, f"{what} p={p}")
        for e in range(2):
            _within(int(((ue[e] >= pf) & (ue[e + 1] >= pf)).sum()), N, q, f"epoch {e}, {e + 1} p={p}")


def perceiver_sites(B=64, K=7, d=256, H=4, Lk_img=256, Lk_ts=48, hidden=128):
    """(name, sid, index array) of the 15 dropout sites of one PatchDualPathologyPerceiver forward (main_architecture_duett.py)."""
    from multimodal_edema_prediction_amd.main_architecture_duett import _SID
    sites = []
    for blk, Lk in (("img_cross", Lk_img), ("img_self", K), ("ts_cross", Lk_ts), ("ts_self", K)):
        s = _SID[blk]
        sites += [(blk + ".attn", s, T.attn_index(B, H, K, Lk)), (blk + ".ff_gelu", s + 1, T.flat_index((B * K, 4 * d))),
                  (blk + ".ff_out", s + 2, T.flat_index((B * K, d)))]
    for head in ("image_head", "temporal_head", "correction_head"):
        sites.append((head, _SID[head], T.flat_index((B * K, hidden))))
    return sites


def test_perceiver_sites_draw_pairwise_independent_masks():
    sites = perceiver_sites()
    assert len(sites) == 15 and len({s[1] for s in sites}) == 15, "two sites of one forward share a stream id"
    p, seed = 0.2, 1234567
    masks = {name: T.keep_mask(seed, sid, idx.ravel(), p) for name, sid, idx in sites}
    for (na, ma), (nb, mb) in itertools.combinations(masks.items(), 2):
        n = min(ma.size, mb.size)
        _within(int((ma[:n] & mb[:n]).sum()), n, (1 - p) ** 2, f"{na} x {nb}")


def test_oracle_drop_hook_sees_the_15_sites():
    """oracle.fusion_ref's `drop=` hook is called once per dropout site of the perceiver, with the tensor the site's kernel masks (its
    layout is what the GPU comparison maps to a stream id); without a hook the oracle draws F.dropout's masks as before."""
    import torch
    import torch.nn.functional as F
    from multimodal_edema_prediction_amd.main_architecture_duett import PatchDualPathologyPerceiver
    from oracle import fusion_ref

    Bs, K, d, H, hid, Lk_img, Lk_ts = 2, 7, 32, 4, 16, 9, 5
    torch.manual_seed(0)
    sd = PatchDualPathologyPerceiver(K, 24, d_latent=d, n_heads=H, head_hidden=hid).state_dict()
    ts, img = torch.randn(Bs, Lk_ts + 1, 24), torch.randn(Bs, Lk_img, d)
    seen = {}

    def drop(t, p, site):
        assert site not in seen, f"site {site} called twice"
        seen[site] = (tuple(t.shape), p)
        return t
    kw = dict(dropout=0.2, head_dropout=0.1, training=True)
    fusion_ref.perceiver_forward(sd, ts, img, H, drop=drop, **kw)
    want = {name: idx.size for name, _, idx in perceiver_sites(Bs, K, d, H, Lk_img, Lk_ts, hid)}
    assert set(seen) == set(want)
    for name, (shape, p) in seen.items():
        assert int(np.prod(shape)) == want[name], name
        assert p == (0.1 if name.endswith("_head") else 0.2), name
        if name.endswith(".attn"):
            assert shape[1] == H and shape[2] == K, name
    torch.manual_seed(5)
    a = fusion_ref.perceiver_forward(sd, ts, img, H, **kw)
    torch.manual_seed(5)
    b = fusion_ref.perceiver_forward(sd, ts, img, H, drop=lambda t, p, site: F.dropout(t, p, True), **kw)
    for k in ("img_logits", "ts_logits", "fusion_logits"):
        assert torch.equal(a[k], b[k])
