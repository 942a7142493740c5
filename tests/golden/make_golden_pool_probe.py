#!/usr/bin/env python3
"""Golden fixture for the probe heads with a hidden stage: runs the REFERENCE'S OWN `train_linear_head(use_attn_pool=True)`
(analysis/unimodal_linear_probe.py) and `train_fusion_head(fusion_type="mlp")` (analysis/logit_fusion_probe.py) on the CPU, fp32,
dropout 0, on ONE seeded problem each (stubs as in make_golden.py) and stores numbers only in tests/golden/pool_probe.npz.

The problems: N_train = 160, N_val = 96, L = 3, 85 % of the labels known, 30 epochs, bs 32, wd 1e-2.
  pool  X [N, T = 5, d = 70]: column 0 is a key that is large at ONE time step per row, and the columns that carry the planted effect
        carry it at that time step only (noise at the others): the head sees the effect only once `attn_query` has learned to follow
        the key, so the query has to move.  d is above 64 and not a multiple of it, T is not a power of two.
  mlp   the two noisy logit matrices of make_golden_linear_probe.py's recipe, H = 32.

Per head:
  R  the reference: per-epoch macro AUROC, per-epoch validation logits, best epoch, best and final state dicts;
  T  the same loop restated in float64 numpy (tests/pool_head_refs.py) from the same initial parameters and row orders.
The row orders are recorded by wrapping `torch.randperm` around the reference's call (the first of each epoch's two calls).

Asserted here, because the tests rest on it; (lr, seed) is searched until all hold:
  1. replaying the DataLoader's draw order reproduces the recorded row orders exactly (`attn_query` is drawn before the nn.Linear);
  2. the best epoch is not the first, R and T agree on it, and the top-2 margin of T's curve is at least 10 pair-steps;
  3. every validation |logit| < 15;
  4. pool: `attn_query` moves by at least 100 gaps (gap = max|R - T| over the parameters);
  5. every planted defect of pool_head_refs moves T's final parameters by at least 100 gaps.  Where no tried (lr, seed) reaches 100
     for a defect the best candidate is kept and the exception is stored with its ratio (`<kind>_defect_ratio`) and printed.
Build container only.

Usage:  python tests/golden/make_golden_pool_probe.py [output directory]"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from head_probe_refs import best_epoch  # noqa: E402  (tests/ is on the path through make_golden)
import pool_head_refs as prefs  # noqa: E402

N_TRAIN, N_VAL, L, T_STEPS, D, H = 160, 96, 3, 5, 70, 32
EPOCHS, BS, WD = 30, 32, 1e-2
LRS = (3e-3, 1e-2, 3e-2, 1e-3)
SEEDS = 24
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
DATA_SEED = 5
KEY = 30.0


def synth(rng, n):
    X = rng.standard_normal((n, T_STEPS, D))
    at = rng.integers(0, T_STEPS, size=n)
    X[:, :, 0] = 0.1 * rng.standard_normal((n, T_STEPS))
    X[np.arange(n), at, 0] = KEY
    sel = X[np.arange(n), at]                                              # the tokens of the key's time step
    logit = np.stack([-0.3 + 1.6 * sel[:, 1 + 2 * l] + 1.2 * sel[:, 2 + 2 * l] for l in range(L)], axis=1)
    Y = (rng.random((n, L)) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    M = (rng.random((n, L)) < 0.85).astype(np.float32)
    img = logit + 1.5 * rng.standard_normal((n, L))
    ts = 0.7 * logit + 1.5 * rng.standard_normal((n, L)) + 0.2
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return {"X": f32(X), "Y": Y, "M": M, "img": f32(img), "ts": f32(ts)}


def replay_perms(n, epochs):
    out = []
    for _ in range(epochs):
        torch.empty((), dtype=torch.int64).random_()
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        out.append(torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy())
    return np.stack(out)


def main(out_dir=HERE):
    install_stubs()
    sys.path.insert(0, REF)
    import analysis.logit_fusion_probe as ref_f
    import analysis.unimodal_linear_probe as ref_u

    rng = np.random.default_rng(DATA_SEED)
    tr, va = synth(rng, N_TRAIN), synth(rng, N_VAL)
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    out = {f"{s}_{k}": v for s, d in (("train", tr), ("val", va)) for k, v in d.items()}
    out.update(cfg=np.array([N_TRAIN, N_VAL, T_STEPS, D, H, L, EPOCHS, BS]), wd=np.array(WD), labels=np.array(LABELS))
    pairs = min(int(((va["Y"][:, l] > 0.5) & (va["M"][:, l] > 0.5)).sum() * ((va["Y"][:, l] < 0.5) & (va["M"][:, l] > 0.5)).sum()) for l in range(L))
    pair_step = 1.0 / (L * pairs)

    real_randperm = torch.randperm
    calls = []

    def spy_randperm(*a, **k):
        r = real_randperm(*a, **k)
        calls.append(r.numpy().copy())
        return r

    def run(kind, seed, lr):
        """One head through the reference (R) and the float64 restatement (T)."""
        calls.clear()
        seen = {"curve": [], "logits": [], "state": []}
        if kind == "pool":
            keys, defects, train_ref = prefs.POOL_KEYS, prefs.POOL_DEFECTS, prefs.train_pool_ref
            Xtr, Xva = tr["X"], va["X"]
            torch.manual_seed(seed)
            init = {k: v.numpy().copy() for k, v in ref_u.LinearHead(D, L, dropout=0.0, use_attn_pool=True).state_dict().items()}
            real_eval = ref_u._eval_multi

            def spy_eval(model, X, Y, M, names, device):
                res = real_eval(model, X, Y, M, names, device)
                with torch.no_grad():
                    seen["logits"].append(model.eval()(X).numpy().copy())
                seen["curve"].append(res["macro_auroc"])
                seen["state"].append({k: v.numpy().copy() for k, v in model.state_dict().items()})
                return res

            ref_u._eval_multi, torch.randperm = spy_eval, spy_randperm
            try:
                torch.manual_seed(seed)
                model, best_ep, _ = ref_u.train_linear_head(t(Xtr), t(tr["Y"]), t(tr["M"]), t(Xva), t(va["Y"]), t(va["M"]), list(LABELS),
                                                            torch.device("cpu"), epochs=EPOCHS, batch_size=BS, lr=lr, weight_decay=WD, dropout=0.0,
                                                            verbose=False, use_attn_pool=True)
            finally:
                ref_u._eval_multi, torch.randperm = real_eval, real_randperm
            torch.manual_seed(seed)
            ref_u.LinearHead(D, L, dropout=0.0, use_attn_pool=True)
        else:
            keys, defects, train_ref = prefs.MLP_KEYS, prefs.MLP_DEFECTS, prefs.train_mlp_ref
            Xtr, Xva = np.concatenate([tr["img"], tr["ts"]], -1), np.concatenate([va["img"], va["ts"]], -1)
            torch.manual_seed(seed)
            init = {k: v.numpy().copy() for k, v in ref_f.LogitFusionHead(L, "mlp", hidden=H, dropout=0.0).state_dict().items()}
            real_eval, real_cls, made = ref_f._eval_from_logits, ref_f.LogitFusionHead, []

            class Spy(real_cls):
                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    made.append(self)

            def spy_eval(logits, Y, M, names):
                res = real_eval(logits, Y, M, names)
                seen["logits"].append(np.array(logits, dtype=np.float32))
                seen["curve"].append(res["macro_auroc"])
                seen["state"].append({k: v.numpy().copy() for k, v in made[-1].state_dict().items()})
                return res

            ref_f._eval_from_logits, ref_f.LogitFusionHead, torch.randperm = spy_eval, Spy, spy_randperm
            try:
                torch.manual_seed(seed)
                model, best_ep, _ = ref_f.train_fusion_head(t(tr["img"]), t(tr["ts"]), t(tr["Y"]), t(tr["M"]), t(va["img"]), t(va["ts"]), t(va["Y"]),
                                                            t(va["M"]), list(LABELS), torch.device("cpu"), fusion_type="mlp", hidden=H, dropout=0.0,
                                                            epochs=EPOCHS, batch_size=BS, lr=lr, weight_decay=WD, verbose=False)
            finally:
                ref_f._eval_from_logits, ref_f.LogitFusionHead, torch.randperm = real_eval, real_cls, real_randperm
            torch.manual_seed(seed)
            real_cls(L, "mlp", hidden=H, dropout=0.0)
        assert len(calls) == 2 * EPOCHS, len(calls)
        perms = np.stack(calls[0::2]).astype(np.int32)
        # 1. the draw order (the default generator stands where the reference's module construction left it)
        assert np.array_equal(replay_perms(N_TRAIN, EPOCHS), perms), "the DataLoader draw order is not what head_probe replays"
        R = {"curve": np.array(seen["curve"]), "val_logits": np.stack(seen["logits"]), "best_epoch": best_ep,
             "best": {k: model.state_dict()[k].numpy().copy() for k in keys}, "final": {k: seen["state"][-1][k] for k in keys}}
        kw = dict(bs=BS, lr=lr, wd=WD)
        val = (Xva, va["Y"], va["M"])
        full = train_ref(Xtr, tr["Y"], tr["M"], init, perms, val=val, **kw)
        T = {"curve": full["curve"], "val_logits": full["val_logits"], "best_epoch": best_epoch(full["curve"]), "final": full["params"]}
        T["best"] = train_ref(Xtr, tr["Y"], tr["M"], init, perms[:max(T["best_epoch"], 1)], **kw)["params"]
        gap_p = max(prefs.param_gap(R["final"], T["final"]), prefs.param_gap(R["best"], T["best"]) if R["best_epoch"] == T["best_epoch"] else 0.0)
        gap_z = np.abs(R["val_logits"] - T["val_logits"]).max()
        report = {"gap_params": gap_p, "gap_logits": gap_z, "defects": {}}
        ok = R["best_epoch"] == T["best_epoch"] and T["best_epoch"] != 1                  # 2.
        top = np.sort(T["curve"])[::-1]
        report["margin_steps"] = (top[0] - top[1]) / pair_step
        ok = ok and report["margin_steps"] >= 10
        report["max_abs_logit"] = max(np.abs(T["val_logits"]).max(), np.abs(R["val_logits"]).max())   # 3.
        ok = ok and report["max_abs_logit"] < 15
        report["query_moved"] = (np.abs(T["final"]["attn_query"] - init["attn_query"]).max() / gap_p) if kind == "pool" else np.inf   # 4.
        ok = ok and report["query_moved"] >= 100
        for d in defects:                                                                # 5.
            bad = train_ref(Xtr, tr["Y"], tr["M"], init, perms, defect=d, **kw)
            report["defects"][d] = prefs.param_gap(bad["params"], T["final"]) / gap_p
        return ok, perms, init, R, T, report

    for kind in ("pool", "mlp"):
        defects = prefs.POOL_DEFECTS if kind == "pool" else prefs.MLP_DEFECTS
        best = None
        for lr, seed in ((lr, seed) for lr in LRS for seed in range(SEEDS)):
            ok, perms, init, R, T, report = run(kind, seed, lr)
            worst = min(report["defects"].values())
            print(f"{kind:5s} lr {lr:g} seed {seed:2d} ok={ok} best R/T {R['best_epoch']}/{T['best_epoch']} gap_params {report['gap_params']:.3g} "
                  f"gap_logits {report['gap_logits']:.3g} margin {report['margin_steps']:.1f} steps max|z| {report['max_abs_logit']:.2f} "
                  f"query moved {report['query_moved']:.0f}x defects/gap {', '.join(f'{k} {v:.0f}x' for k, v in report['defects'].items())}")
            if ok and (best is None or worst > best[0]):
                best = (worst, lr, seed, perms, init, R, T, report)
            if ok and worst >= 100:
                break
        assert best is not None, f"{kind}: no (lr, seed) tried meets the fixture's conditions"
        worst, lr, seed, perms, init, R, T, report = best
        for d, v in report["defects"].items():
            if v < 100:
                print(f"EXCEPTION {kind}: defect {d} moves T by only {v:.1f} gaps at the best (lr, seed) tried; stored in {kind}_defect_ratio")
        out.update({f"{kind}_seed": np.array(seed), f"{kind}_lr": np.array(lr), f"{kind}_perms": perms.astype(np.int16),
                    f"{kind}_gap_params": np.float64(report["gap_params"]), f"{kind}_gap_logits": np.float64(report["gap_logits"]),
                    f"{kind}_margin_steps": np.float64(report["margin_steps"]), f"{kind}_max_abs_logit": np.float64(report["max_abs_logit"]),
                    f"{kind}_query_moved": np.float64(report["query_moved"]),
                    f"{kind}_defect_ratio": np.array([report["defects"][d] for d in defects]), f"{kind}_defects": np.array(defects)})
        for k, v in init.items():
            out[f"{kind}_init_{k}"] = v
        for tag, res in (("R", R), ("T", T)):
            out.update({f"{kind}_{tag}_curve": np.asarray(res["curve"], dtype=np.float64), f"{kind}_{tag}_best_epoch": np.array(res["best_epoch"])})
            for k in res["final"]:
                out[f"{kind}_{tag}_final_{k}"] = res["final"][k]
                out[f"{kind}_{tag}_best_{k}"] = res["best"][k]
        out[f"{kind}_T_val_logits"] = T["val_logits"]
    path = os.path.join(out_dir, "pool_probe.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 3 * 2 ** 18, os.path.getsize(path)
    print(f"wrote pool_probe.npz: {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
