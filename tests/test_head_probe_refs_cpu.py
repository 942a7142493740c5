"""CPU checks of what the linear-head probes' GPU tests rest on (no GPU needed): the float64 restatement of the training loop
(tests/head_probe_refs.py) against the fixture of tests/golden/make_golden_linear_probe.py (R = the reference's own run, T = the
restatement), the package's replay of the DataLoader's draw order, the mirrored names / signatures / state-dict keys, the token
poolings, and the library's host-side validation of the problem table."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import head_probe_refs as refs
from multimodal_edema_prediction_amd import head_probe, logit_fusion_probe as lfp, unimodal_linear_probe as ulp
from multimodal_edema_prediction_amd.abi import MedpHeadProblem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("lin", "fus_linear", "fus_per_label")


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLDEN, "linear_probe.npz")))


def inputs(G, kind):
    """(X_tr, X_va, label_width) of a head of the fixture."""
    if kind == "lin":
        return G["train_X"], G["val_X"], 0
    if kind == "fus_per_label":
        il = lambda a, b: np.stack([a, b], -1).reshape(len(a), -1)  # noqa: E731
        return il(G["train_img"], G["train_ts"]), il(G["val_img"], G["val_ts"]), 2
    return np.concatenate([G["train_img"], G["train_ts"]], -1), np.concatenate([G["val_img"], G["val_ts"]], -1), 0


def run_T(G, kind, **kw):
    Xtr, Xva, width = inputs(G, kind)
    bs = int(G["cfg"][5])
    return refs.train_ref(Xtr, G["train_Y"], G["train_M"], G[f"{kind}_W0"], G[f"{kind}_b0"], G[f"{kind}_perms"], bs=bs, lr=float(G[f"{kind}_lr"]),
                          wd=float(G["wd"]), label_width=width, val=(Xva, G["val_Y"], G["val_M"]), **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_the_restatement_reproduces_T_and_is_within_the_stored_gap_of_R(G, kind):
    T = run_T(G, kind)
    for k in ("W", "b"):
        assert np.abs(T[k] - G[f"{kind}_T_{k}"]).max() <= 1e-12
        assert np.abs(T[k] - G[f"{kind}_R_{k}"].reshape(T[k].shape)).max() <= float(G[f"{kind}_gap_params"])
    assert np.abs(T["val_logits"] - G[f"{kind}_T_val_logits"]).max() <= 1e-12
    assert np.abs(T["curve"] - G[f"{kind}_T_curve"]).max() <= 1e-12
    assert refs.best_epoch(T["curve"]) == int(G[f"{kind}_T_best_epoch"]) == int(G[f"{kind}_R_best_epoch"]) != 1
    # the reference's own curve is T's (the top-2 margin is far above one pair-step)
    assert np.abs(G[f"{kind}_R_curve"] - T["curve"]).max() <= 1e-12


def test_the_stored_conditions_hold(G):
    for kind in KINDS:
        ratios = dict(zip(G["defects"], G[f"{kind}_defect_ratio"]))
        for d, r in ratios.items():
            assert r >= 100 or (d == "eps_in_sqrt" and kind != "lin"), (kind, d, r)
        assert float(G[f"{kind}_margin_steps"]) >= 10
        assert np.abs(G[f"{kind}_T_val_logits"]).max() < 15
    assert (G["train_M"][:int(G["cfg"][5])] == 0).all()                  # the leading block without a known label


def test_a_planted_defect_moves_the_restatement(G):
    T, bad = run_T(G, "lin"), run_T(G, "lin", defect="no_bias_wd")
    assert np.abs(bad["b"] - T["b"]).max() >= 100 * float(G["lin_gap_params"])


@pytest.mark.parametrize("kind", KINDS)
def test_the_package_draws_the_recorded_row_orders(G, kind):
    """Module construction, then the DataLoader's draws: what train_linear_head / train_fusion_head do before the first launch."""
    N, _, F, L, E, _ = (int(v) for v in G["cfg"])
    torch.manual_seed(int(G[f"{kind}_seed"]))
    if kind == "lin":
        model = ulp.LinearHead(F, L, dropout=0.0)
        W0, b0 = model.head[1].weight, model.head[1].bias
    else:
        model = lfp.LogitFusionHead(L, kind[len("fus_"):])
        W0, b0 = (model.per_label_w, model.per_label_b) if kind == "fus_per_label" else (model.head.weight, model.head.bias)
    assert np.array_equal(W0.detach().numpy(), G[f"{kind}_W0"]) and np.array_equal(b0.detach().numpy(), G[f"{kind}_b0"])
    assert np.array_equal(head_probe.draw_epoch_permutations(N, E), G[f"{kind}_perms"])


def _sig(fn):
    return [[n, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def _mirrors(ours, theirs, what):
    """The reference's parameters lead ours, by name, kind and default; what we add has a default (or is keyword-only)."""
    assert ours[:len(theirs)] == theirs, (what, ours, theirs)
    for name, kind, default in ours[len(theirs):]:
        assert kind == "KEYWORD_ONLY" or default is not None, (what, name)


def test_names_signatures_and_state_dict_keys_mirror_the_reference():
    doc = json.load(open(os.path.join(GOLDEN, "linear_probe_signatures.json")))
    mods = {"unimodal_linear_probe": ulp, "logit_fusion_probe": lfp}
    assert len(doc["functions"]) == 11 and len(doc["classes"]) == 2
    for key, theirs in doc["functions"].items():
        mod, name = key.split(".")
        _mirrors(_sig(getattr(mods[mod], name)), theirs, key)
    for key, methods in doc["classes"].items():
        mod, name = key.split(".")
        for m, theirs in methods.items():
            _mirrors(_sig(getattr(getattr(mods[mod], name), m)), theirs, f"{key}.{m}")
    keys = doc["state_dict_keys"]
    assert list(ulp.LinearHead(8, 3).state_dict()) == keys["LinearHead"] == ["head.1.weight", "head.1.bias"]
    assert list(ulp.LinearHead(8, 3, use_attn_pool=True).state_dict()) == keys["LinearHead(use_attn_pool=True)"]
    for ftype in ("linear", "mlp", "per_label"):
        assert list(lfp.LogitFusionHead(3, ftype).state_dict()) == keys[f"LogitFusionHead({ftype})"]
    assert {"attn_query", "per_label_w", "per_label_b", "head.weight", "head.bias"} <= {k for v in keys.values() for k in v}
    w = lfp.LogitFusionHead(3, "per_label")
    assert torch.equal(w.per_label_w, torch.tensor([[1.0, 0.0]] * 3)) and torch.equal(w.per_label_b, torch.zeros(3))


@pytest.mark.parametrize("T", [24, 7])
@pytest.mark.parametrize("feature_type", ["rep", "hourly_mean", "multiscale", "attn_pool"])
def test_pool_duett_tokens_matches_the_reference(G, T, feature_type):
    got = ulp._pool_duett_tokens(torch.from_numpy(G[f"pool_tokens_T{T}"]), feature_type).numpy()
    want = G[f"pool_{feature_type}_T{T}"]
    assert got.shape == want.shape and np.array_equal(got, want)
    with pytest.raises(ValueError, match="unknown feature_type"):
        ulp._pool_duett_tokens(torch.zeros(1, 3, 2), "nope")


def _entry(**kw):
    """A table entry whose pointers are never dereferenced: the host-side checks launch nothing."""
    v = dict(X=64, Y=64, M=64, W=64, b=64, mW=64, vW=64, mb=64, vb=64, t=64, perm=64, loss_out=64, ldx=80, N=100, ldy=3, col0=4, F=70, L=3,
             label_width=0, bs=32, S=3, lr=1e-3, weight_decay=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, dropout_p=0.1, seed=1, stream_id=0,
             reserved_=0)
    v.update(kw)
    return MedpHeadProblem(**v)


@pytest.mark.parametrize("bad, text", [(dict(F=0), "F=0"), (dict(F=head_probe.MAX_F + 1, ldx=10 ** 6), "F="), (dict(L=0), "L=0"),
                                       (dict(L=17, ldy=17), "L=17"), (dict(bs=0), "bs=0"), (dict(bs=1025, N=5000), "bs=1025"),
                                       (dict(label_width=4), "label_width=4"), (dict(ldx=73), "leave a row"), (dict(ldy=2), "ldy=2"),
                                       (dict(S=4), "S=4"), (dict(dropout_p=1.0), "dropout_p"), (dict(W=None), "null pointer"),
                                       (dict(perm=None), "null pointer")])
def test_the_table_is_validated_on_the_host_before_anything_is_launched(bad, text):
    with pytest.raises(ValueError, match=text):
        head_probe.check_table([_entry(), _entry(**bad)])


def test_a_valid_table_passes_every_check_but_the_missing_device_copy():
    with pytest.raises(ValueError, match="null device table"):
        head_probe.check_table([_entry(), _entry(label_width=2, F=6, ldx=10)])
    assert head_probe.onchip(768, 7, 0, 128) and not head_probe.onchip(4704, 7, 0, 128)
