"""End-to-end tests of the attention-pooled probe head and the MLP fusion head on the fixture tests/golden/pool_probe.npz (R = the
reference's own run on the CPU, T = its float64 restatement; tests/golden/make_golden_pool_probe.py).

Tolerance, as in test_gpu_linear_probe.py: R and T are two realisations of the same arithmetic (fp32 / fp64); the device is a third.
Every parameter tensor and every epoch's validation logits must be within 8 max|R - T| + 1e-7 of T, with the fixture's stored gaps;
every planted defect moves T by more than 100 gaps (asserted by the generator and by test_pool_head_refs_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import pool_head_refs as prefs
from multimodal_edema_prediction_amd import head_probe, logit_fusion_probe as lfp, unimodal_linear_probe as ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLDEN, "pool_probe.npz")))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _check(G, kind, keys, model, best_epoch, best_val, hist):
    E = int(G["cfg"][6])
    gp, gz = float(G[f"{kind}_gap_params"]), float(G[f"{kind}_gap_logits"])
    T_best = int(G[f"{kind}_T_best_epoch"])
    state = model.state_dict()
    errs = {k: float(np.abs(state[k].detach().cpu().numpy().astype(np.float64) - G[f"{kind}_T_best_{k}"]).max()) for k in keys}
    ez = np.abs(hist["val_logits"].astype(np.float64) - G[f"{kind}_T_val_logits"]).max()
    ec = np.abs(hist["curve"] - G[f"{kind}_T_curve"]).max()
    print(f"{kind}: best epoch {best_epoch} (T {T_best}) " + " ".join(f"|{k} - T| {e:.3g}" for k, e in errs.items()) +
          f" (bound {8 * gp + 1e-7:.3g}) |z - T| {ez:.3g} (bound {8 * gz + 1e-7:.3g}) |curve - T| {ec:.3g}")
    assert best_epoch == T_best == int(G[f"{kind}_R_best_epoch"])
    assert set(state) == set(keys) and all(e <= 8 * gp + 1e-7 for e in errs.values())
    assert hist["val_logits"].shape == G[f"{kind}_T_val_logits"].shape and ez <= 8 * gz + 1e-7
    assert len(hist["curve"]) == E and abs(best_val - hist["curve"][best_epoch - 1]) == 0
    assert all(v.is_cuda for v in state.values()) and np.isfinite(hist["train_loss"]).all() and (hist["valid_sum"] > 0).all()


def _pool(G, **kw):
    E, bs = int(G["cfg"][6]), int(G["cfg"][7])
    torch.manual_seed(int(G["pool_seed"]))
    args = dict(epochs=E, batch_size=bs, lr=float(G["pool_lr"]), weight_decay=float(G["wd"]), dropout=0.0, verbose=False, use_attn_pool=True)
    args.update(kw)
    return ulp.train_linear_head(_t(G["train_X"]), _t(G["train_Y"]), _t(G["train_M"]), _t(G["val_X"]), _t(G["val_Y"]), _t(G["val_M"]),
                                 list(G["labels"]), DEV, **args)


def _mlp(G, **kw):
    E, bs, H = int(G["cfg"][6]), int(G["cfg"][7]), int(G["cfg"][4])
    torch.manual_seed(int(G["mlp_seed"]))
    args = dict(fusion_type="mlp", hidden=H, dropout=0.0, epochs=E, batch_size=bs, lr=float(G["mlp_lr"]), weight_decay=float(G["wd"]), verbose=False)
    args.update(kw)
    return lfp.train_fusion_head(_t(G["train_img"]), _t(G["train_ts"]), _t(G["train_Y"]), _t(G["train_M"]), _t(G["val_img"]), _t(G["val_ts"]),
                                 _t(G["val_Y"]), _t(G["val_M"]), list(G["labels"]), DEV, **args)


def test_train_linear_head_with_attention_pooling_reproduces_the_fixture(G):
    """The module is built from torch's default generator (attn_query before the nn.Linear) and the row orders drawn after it: the
    fixture's initial state and row orders are reproduced from the seed alone."""
    hist = {"record_val_logits": True}
    model, best_epoch, best_val = _pool(G, history=hist, eager=False)
    _check(G, "pool", prefs.POOL_KEYS, model, best_epoch, best_val, hist)
    # the returned module scores as the kernel does, and its table is the curve's best value
    res = ulp._eval_multi(model, _t(G["val_X"]), _t(G["val_Y"]), _t(G["val_M"]), list(G["labels"]), DEV)
    assert abs(res["macro_auroc"] - best_val) <= 1e-12 and set(res["per_label"]) == set(G["labels"])
    z = model(_t(G["val_X"]).to(DEV))                                       # the module computes what the kernels trained
    assert np.abs(z.detach().cpu().numpy() - hist["val_logits"][best_epoch - 1]).max() <= 1e-5


def test_train_fusion_head_mlp_reproduces_the_fixture(G, capsys):
    hist = {"record_val_logits": True}
    model, best_epoch, best_val = _mlp(G, history=hist, eager=False, verbose=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("  ep ")]
    assert len(lines) == int(G["cfg"][6]) and "train_loss=" in lines[0] and "val_macro_AUROC=" in lines[0]
    _check(G, "mlp", prefs.MLP_KEYS, model, best_epoch, best_val, hist)
    z = model(_t(G["val_img"]).to(DEV), _t(G["val_ts"]).to(DEV))
    assert np.abs(z.detach().cpu().numpy() - hist["val_logits"][best_epoch - 1]).max() <= 1e-5


def test_init_state_is_honoured(G):
    init = {k: _t(G[f"pool_init_{k}"]) for k in prefs.POOL_KEYS}
    hist = {"record_val_logits": True}
    _pool(G, history=hist, init_state=init, epochs=3)
    assert np.abs(hist["val_logits"] - G["pool_T_val_logits"][:3]).max() <= 8 * float(G["pool_gap_logits"]) + 1e-7


def test_the_default_call_takes_the_device_path_and_eager_true_the_torch_loop(G, monkeypatch):
    def boom(*a, **k):
        raise RuntimeError("eager_fit was called")

    monkeypatch.setattr(head_probe, "eager_fit", boom)
    model, ep, val = _pool(G, epochs=2)                                     # eager=None
    assert ep in (1, 2) and np.isfinite(val) and model.attn_query.is_cuda
    model, ep, val = _mlp(G, epochs=2, dropout=0.1)
    assert ep in (1, 2) and np.isfinite(val) and model.head[0].weight.is_cuda
    with pytest.raises(RuntimeError, match="eager_fit was called"):
        _pool(G, epochs=2, eager=True)
    with pytest.raises(RuntimeError, match="eager_fit was called"):
        _mlp(G, epochs=2, eager=True)
    with pytest.raises(RuntimeError, match="eager_fit was called"):        # beyond the LDS budget the default falls back
        _mlp(G, epochs=2, hidden=512)


def test_eager_true_still_trains(G):
    model, ep, val = _pool(G, epochs=2, eager=True)
    assert ep in (1, 2) and np.isfinite(val) and "attn_query" in model.state_dict()
    model, ep, val = _mlp(G, epochs=2, eager=True)
    assert ep in (1, 2) and np.isfinite(val)


def test_both_mains_run_with_the_pooled_head_and_the_mlp_fusion(capsys):
    cohort = ["--n_train", "48", "--n_val", "32", "--n_test", "32", "--n_timesteps", "24", "--n_vars", "16", "--d_static", "8",
              "--image_size", "224", "--batch_size", "16"]
    out = ulp.main(["--modality", "duett_attn_pool", "--epochs", "3", "--train_batch_size", "16"] + cohort)
    text = capsys.readouterr().out
    assert "[result] DUETT_ATTN_POOL-only linear probe" in text and "macro average" in text and "pool=attn (T=24)" in text
    assert 1 <= out["best_epoch"] <= 3 and out["model"].attn_query.is_cuda
    out = lfp.main(["--ts_modality", "duett_attn_pool", "--fusion_type", "mlp", "--uni_epochs", "3", "--fus_epochs", "3", "--uni_batch_size", "16",
                    "--fus_batch_size", "16"] + cohort)
    text = capsys.readouterr().out
    assert "[stage 2] DuETT linear probe (duett_attn_pool)" in text and "[result] logit-fusion probe   (fusion_type=mlp)" in text
    assert "fus_roc" in text and all(1 <= e <= 3 for e in out["best_epochs"]) and out["model"].head[0].weight.is_cuda
