"""CPU checks behind the attention-pool / MLP-fusion head tests: the numpy restatement (tests/pool_head_refs.py) against torch autograd and
torch.optim.AdamW in float64, the conditions the fixture tests/golden/pool_probe.npz was generated under, the host-side argument
checks of the three new training / scoring entry points (driven without a device through the null-device convention), and the
`eager=False` contract of the two trainers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pool_head_refs as prefs
from multimodal_edema_prediction_amd import head_probe, logit_fusion_probe as lfp, unimodal_linear_probe as ulp
from multimodal_edema_prediction_amd.abi import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR, WD = 3e-3, 1e-2


def _problem(kind, seed=0, n=24, L=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 5, 13)) if kind == "pool" else rng.standard_normal((n, 2 * L))
    Y = (rng.random((n, L)) < 0.4).astype(np.float64)
    M = (rng.random((n, L)) < 0.8).astype(np.float64)
    torch.manual_seed(seed)
    model = (ulp.LinearHead(13, L, dropout=0.0, use_attn_pool=True) if kind == "pool" else lfp.LogitFusionHead(L, "mlp", hidden=7, dropout=0.0)).double()
    if kind == "pool":
        with torch.no_grad():
            model.attn_query.mul_(40.0)                                     # a softmax far from uniform
    return X, Y, M, model


@pytest.mark.parametrize("kind", ["pool", "mlp"])
def test_restated_gradients_and_three_adamw_steps_match_torch_in_float64(kind):
    X, Y, M, model = _problem(kind)
    bs = 8
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    fwd, bwd, train = ((prefs.pool_forward, prefs.pool_backward, prefs.train_pool_ref) if kind == "pool" else
                       (prefs.mlp_forward, prefs.mlp_backward, prefs.train_mlp_ref))
    call = (lambda x: model(x)) if kind == "pool" else (lambda x: model(x[:, :3], x[:, 3:]))
    # the gradients of the first minibatch
    z = call(torch.from_numpy(X[:bs]))
    ulp.masked_bce(z, torch.from_numpy(Y[:bs]), torch.from_numpy(M[:bs])).backward()
    zr, cache = fwd(X[:bs], init)
    g, _, _ = prefs.bce_grad(zr, Y[:bs], M[:bs])
    G = bwd(g, init, cache)
    assert np.abs(zr - z.detach().numpy()).max() <= 1e-12
    for k, p in model.named_parameters():
        assert np.abs(G[k] - p.grad.numpy()).max() <= 1e-12, k
        assert np.abs(p.grad.numpy()).max() > 1e-4, k                       # a gradient that is there to be compared
    # three steps of torch.optim.AdamW
    model.zero_grad()
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    for s in range(3):
        rows = slice(s * bs, (s + 1) * bs)
        opt.zero_grad()
        ulp.masked_bce(call(torch.from_numpy(X[rows])), torch.from_numpy(Y[rows]), torch.from_numpy(M[rows])).backward()
        opt.step()
    T = train(X, Y, M, init, [np.arange(24)], bs=bs, lr=LR, wd=WD)
    assert T["state"][2] == 3
    for k, v in model.state_dict().items():
        assert np.abs(T["params"][k] - v.numpy()).max() <= 1e-12, k
    # every planted defect is a different computation
    for d in (prefs.POOL_DEFECTS if kind == "pool" else prefs.MLP_DEFECTS):
        bad = train(X, Y, M, init, [np.arange(24)], bs=bs, lr=LR, wd=WD, defect=d)
        assert prefs.param_gap(bad["params"], T["params"]) > 1e-7, d


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLDEN, "pool_probe.npz")))


@pytest.mark.parametrize("kind", ["pool", "mlp"])
def test_the_fixture_meets_the_conditions_it_was_generated_under(G, kind):
    E = int(G["cfg"][6])
    assert int(G[f"{kind}_R_best_epoch"]) == int(G[f"{kind}_T_best_epoch"]) != 1
    assert len(G[f"{kind}_T_curve"]) == E and G[f"{kind}_T_val_logits"].shape[0] == E
    assert float(G[f"{kind}_margin_steps"]) >= 10 and float(G[f"{kind}_max_abs_logit"]) < 15
    assert float(G[f"{kind}_query_moved"]) >= 100
    ratios = dict(zip((str(d) for d in G[f"{kind}_defects"]), G[f"{kind}_defect_ratio"]))
    print(kind, ratios, "gaps", float(G[f"{kind}_gap_params"]), float(G[f"{kind}_gap_logits"]))
    assert set(ratios) == set(prefs.POOL_DEFECTS if kind == "pool" else prefs.MLP_DEFECTS)
    for d, r in ratios.items():
        assert r >= 100, f"{kind}: defect {d} moves T by {r:.1f} gaps"


def test_the_restatement_reproduces_the_fixtures_T(G):
    """Five epochs of T from the stored initial state and row orders: the helper in the tree is the one the fixture was made with."""
    for kind, keys, train in (("pool", prefs.POOL_KEYS, prefs.train_pool_ref), ("mlp", prefs.MLP_KEYS, prefs.train_mlp_ref)):
        init = {k: G[f"{kind}_init_{k}"] for k in keys}
        Xtr, Xva = ((G["train_X"], G["val_X"]) if kind == "pool" else
                    (np.concatenate([G["train_img"], G["train_ts"]], -1), np.concatenate([G["val_img"], G["val_ts"]], -1)))
        T = train(Xtr, G["train_Y"], G["train_M"], init, G[f"{kind}_perms"][:5], bs=int(G["cfg"][7]), lr=float(G[f"{kind}_lr"]), wd=float(G["wd"]),
                  val=(Xva, G["val_Y"], G["val_M"]))
        assert np.abs(T["val_logits"] - G[f"{kind}_T_val_logits"][:5]).max() <= 1e-12 and np.array_equal(T["curve"], G[f"{kind}_T_curve"][:5])


# ---- host-side checks, no device: every pointer is a fake address that is never dereferenced, the device permutation / table is null
FAKE = 4096


def _pool_entry(**over):
    """A valid problem (N 40, T 5, d 9, L 3, bs 8, S 5) with the struct fields of `over` replaced."""
    N, T, d, L, bs = 40, 5, 9, 3, 8
    pb = head_probe.PoolHeadProblem(torch.zeros(N, T, d), torch.zeros(N, L), torch.zeros(N, L), torch.zeros(d), torch.zeros(L, d), torch.zeros(L), bs=bs)
    e = pb.entry(None, None, addr=lambda t: FAKE)
    e.perm = None
    for k, v in over.items():
        setattr(e, k, v)
    return e


def _pool_rc(entry, perm):
    perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    rc = lib().medp_pool_head_train_epoch(ctypes.byref(entry), None if perm is None else perm.ctypes.data, None)
    return rc, lib().medp_last_error().decode()


POOL_BAD = [(dict(T=0), "T=0"), (dict(T=1025), "T=1025"), (dict(d=0), "d=0"), (dict(d=32769), "d=32769"), (dict(L=0), "L=0"), (dict(L=17), "L=17"),
            (dict(bs=0), "bs=0"), (dict(bs=1025, N=4000, S=1), "bs=1025"), (dict(S=0), "S=0"), (dict(S=6), "S=6 steps of 8 rows with N=40"),
            (dict(dropout_p=1.0), "dropout_p=1"), (dict(dropout_p=-0.1), "dropout_p"), (dict(ldy=2), "ldy=2"), (dict(step0=-1), "step0"),
            (dict(beta1=1.0), "AdamW scalars"), (dict(X=None), "null pointer"), (dict(q=None), "null pointer"), (dict(ws=None), "null pointer"),
            (dict(loss_out=None), "null pointer")]


@pytest.mark.parametrize("over, text", POOL_BAD)
def test_pool_head_train_epoch_reports_every_limit_before_any_launch(over, text):
    rc, msg = _pool_rc(_pool_entry(**over), np.arange(40))
    assert rc < 0 and text in msg, msg


def test_pool_head_train_epoch_checks_the_permutation_on_the_host_and_reports_the_null_device_copy_last():
    good = np.arange(40)
    rc, msg = _pool_rc(_pool_entry(), good)
    assert rc < 0 and "null device permutation" in msg                     # everything else passed
    for bad, where in ((-1, 7), (40, 39), (40, 0)):
        perm = good.copy()
        perm[where] = bad
        rc, msg = _pool_rc(_pool_entry(), perm)
        assert rc < 0 and f"permutation entry {where} = {bad} outside [0, 40)" in msg, msg
    rc, msg = _pool_rc(_pool_entry(), None)
    assert rc < 0 and "null pointer" in msg
    rc = lib().medp_pool_head_train_epoch(None, good.astype(np.int32).ctypes.data, None)
    assert rc < 0 and "null problem" in lib().medp_last_error().decode()
    with pytest.raises(ValueError, match="null device permutation"):
        head_probe.check(_pool_rc(_pool_entry(), good)[0], "pool_head_train_epoch")


SCORES_BAD = [(dict(T=0), "T=0"), (dict(T=1025), "T=1025"), (dict(d=32769), "d=32769"), (dict(L=17), "L=17"), (dict(N=0), "N=0"), (dict(n=0), "n=0"),
              (dict(X=None), "null argument"), (dict(probs=None), "null argument")]


@pytest.mark.parametrize("over, text", SCORES_BAD)
def test_pool_head_scores_reports_every_limit_before_any_launch(over, text):
    a = dict(X=FAKE, N=10, T=5, d=9, L=3, q=FAKE, W=FAKE, b=FAKE, rows=None, n=10, logits=FAKE, probs=FAKE)
    a.update(over)
    rc = lib().medp_pool_head_scores(a["X"], a["N"], a["T"], a["d"], a["L"], a["q"], a["W"], a["b"], a["rows"], a["n"], a["logits"], a["probs"], None)
    assert rc < 0 and text in lib().medp_last_error().decode(), lib().medp_last_error()


def _mlp_table(host_perm, **over):
    """A one-problem table (N 40, K 6, H 5, L 3, bs 8, S 5) with the struct fields of `over` replaced."""
    N, L, H, bs = 40, 3, 5, 8
    pb = head_probe.MlpHeadProblem(torch.zeros(N, 2 * L), torch.zeros(N, L), torch.zeros(N, L), torch.zeros(H, 2 * L), torch.zeros(H), torch.zeros(L, H),
                                   torch.zeros(L), bs=bs)
    e = pb.entry(None, host_perm, None, addr=lambda t: FAKE)
    for k, v in over.items():
        setattr(e, k, v)
    return head_probe.make_mlp_table([e])[0]


MLP_BAD = [(dict(K=0), "K=0"), (dict(K=65, ldx=65), "K=65"), (dict(H=0), "H=0"), (dict(H=1025), "H=1025"), (dict(L=0), "L=0"), (dict(L=17), "L=17"),
           (dict(bs=0), "bs=0"), (dict(bs=1025, N=4000, S=1), "bs=1025"), (dict(S=0), "S=0"), (dict(S=6), "S=6 steps"), (dict(dropout_p=1.0), "dropout_p=1"),
           (dict(ldy=2), "ldy=2"), (dict(ldx=5), "leave a row of 5"), (dict(col0=-1), "columns [-1"), (dict(beta2=1.0), "AdamW scalars"),
           (dict(H=1024, K=64, ldx=64), "bytes of LDS"), (dict(W2=None), "null pointer"), (dict(mom=None), "null pointer"), (dict(perm_host=None), "null pointer"),
           (dict(perm=None), "null pointer")]


@pytest.mark.parametrize("over, text", MLP_BAD)
def test_mlp_head_train_epoch_reports_every_limit_before_any_launch(over, text):
    perm = np.arange(40, dtype=np.int32)
    rc = lib().medp_mlp_head_train_epoch(_mlp_table(perm, **over), None, 1, None)
    assert rc < 0 and text in lib().medp_last_error().decode(), lib().medp_last_error()


def test_mlp_head_train_epoch_checks_the_permutation_on_the_host_and_reports_the_null_device_table_last():
    perm = np.arange(40, dtype=np.int32)
    rc = lib().medp_mlp_head_train_epoch(_mlp_table(perm), None, 1, None)
    assert rc < 0 and "null device table" in lib().medp_last_error().decode()
    for bad in (-1, 40):
        p = perm.copy()
        p[11] = bad
        rc = lib().medp_mlp_head_train_epoch(_mlp_table(p), None, 1, None)
        assert rc < 0 and f"permutation entry 11 = {bad} outside [0, 40)" in lib().medp_last_error().decode()
    for P in (0, 65536):
        assert lib().medp_mlp_head_train_epoch(_mlp_table(perm), None, P, None) < 0 and f"P={P}" in lib().medp_last_error().decode()
    assert lib().medp_mlp_head_train_epoch(None, None, 1, None) < 0 and "null host table" in lib().medp_last_error().decode()


def test_mlp_head_scores_reports_every_limit_before_any_launch():
    def rc(**over):
        a = dict(X=FAKE, ldx=6, N=10, col0=0, K=6, H=5, L=3, W1=FAKE, b1=FAKE, W2=FAKE, b2=FAKE, rows=None, n=10, logits=FAKE, probs=FAKE)
        a.update(over)
        r = lib().medp_mlp_head_scores(*(a[k] for k in ("X", "ldx", "N", "col0", "K", "H", "L", "W1", "b1", "W2", "b2", "rows", "n", "logits", "probs")), None)
        return r, lib().medp_last_error().decode()
    for over, text in ((dict(K=0), "K=0"), (dict(K=65, ldx=70), "K=65"), (dict(H=1025), "H=1025"), (dict(L=17), "L=17"), (dict(ldx=5), "leave a row"),
                       (dict(n=0), "n=0"), (dict(W1=None), "null argument"), (dict(logits=None), "null argument")):
        r, msg = rc(**over)
        assert r < 0 and text in msg, msg


def test_the_shape_queries():
    L = lib()
    assert L.medp_pool_head_rows_onchip(24, 1176) == 1 and L.medp_pool_head_rows_onchip(24, 2328) == 0
    assert L.medp_pool_head_rows_onchip(5, 70) == 1 and L.medp_pool_head_rows_onchip(0, 70) == 0 and L.medp_pool_head_rows_onchip(1025, 1) == 0
    assert L.medp_pool_head_rows_onchip(1024, 32) == 1 and L.medp_pool_head_rows_onchip(1024, 33) == 0      # 16 T + 4 T d against 144 KiB
    assert L.medp_pool_head_ws_bytes(70, 3, 32) == 8 * 33 + 4 * (32 * 8 + 2 * 32 * 70) and L.medp_pool_head_ws_bytes(70, 17, 32) == 0
    assert head_probe.mlp_head_supported(7, 32, 128) and head_probe.mlp_head_supported(16, 32, 1024) is False
    assert L.medp_mlp_head_supported(6, 3, 32, 32) == 1 and L.medp_mlp_head_supported(65, 3, 32, 32) == 0
    # 8 bs H + 4 bs Lpad + 12 (H K + H + L H + L) against 144 KiB
    for K, Lb, H, bs in ((14, 7, 32, 128), (14, 7, 64, 128), (14, 7, 128, 128), (32, 16, 256, 32), (2, 1, 1024, 16)):
        need = 8 * bs * H + 4 * bs * (2 if Lb <= 2 else 8 if Lb <= 8 else 16) + 12 * (H * K + H + Lb * H + Lb)
        assert L.medp_mlp_head_supported(K, Lb, H, bs) == int(need <= 144 * 1024), (K, Lb, H, bs)


def test_eager_false_on_an_unsupported_shape_raises_before_a_device_is_needed():
    z2, z3 = torch.zeros(40, 3), torch.zeros(40, 2, 4)
    names = ["a", "b", "c"]
    with pytest.raises(ValueError, match="outside the attention-pool kernels' limits"):      # batch size over the kernels' 1024
        ulp.train_linear_head(torch.zeros(1100, 2, 4), torch.zeros(1100, 3), torch.ones(1100, 3), z3, z2, z2, names, "cuda", epochs=1,
                              batch_size=1025, use_attn_pool=True, eager=False)
    with pytest.raises(ValueError, match="outside the attention-pool kernels' limits"):      # fewer rows than one minibatch
        ulp.train_linear_head(z3, z2, z2, z3, z2, z2, names, "cuda", epochs=1, batch_size=64, use_attn_pool=True, eager=False)
    with pytest.raises(ValueError, match="outside the mlp kernel's limits"):                 # hidden width beyond the LDS budget
        lfp.train_fusion_head(z2, z2, z2, z2, z2, z2, z2, z2, names, "cuda", fusion_type="mlp", hidden=512, epochs=1, batch_size=32, eager=False)
