#!/usr/bin/env python3
"""Golden fixture for the linear-head probes (analysis/unimodal_linear_probe.py, analysis/logit_fusion_probe.py): runs the
REFERENCE'S OWN `train_linear_head` and `train_fusion_head` ("linear", "per_label") on the CPU, fp32, dropout 0, on ONE seeded
problem (stubs as in make_golden.py) and stores numbers and names only:

  tests/golden/linear_probe.npz               inputs, initial parameters, every epoch's row order, R, T and their gaps
  tests/golden/linear_probe_signatures.json   names, signatures and state-dict keys of the two reference modules

The problem: N_train = 300, N_val = 160, F = 70, L = 3, 85 % of the labels known, the effect planted in two columns per label; the
first `bs` training rows have no known label at all.  (The reference's loader shuffles, so those rows are spread over the
minibatches and R never meets an all-unknown minibatch; the kernel tests build that step directly.)  30 epochs, bs 32, lr 3e-3
(the fusion heads: the first of FUS_LRS that meets the conditions), wd 1e-2.  The fusion heads train on two seeded logit matrices [N, L].

Per head (`lin`, `fus_linear`, `fus_per_label`):
  R  the reference: per-epoch macro AUROC, per-epoch validation logits, best epoch, best and final parameters;
  T  the same loop restated in float64 numpy (tests/head_probe_refs.py) from the same initial parameters and row orders.
The row orders are recorded by wrapping `torch.randperm` around the reference's call (the first of each epoch's two calls).

Asserted here, because the tests rest on it:
  1. replaying the DataLoader's draw order (one int64 draw, one more, randperm from a private generator seeded with the second)
     reproduces the recorded row orders exactly;
  2. every planted defect of head_probe_refs.DEFECTS moves T's final parameters by at least 100 x max|R - T|.  One exception,
     recorded with its ratio: eps inside the square root on the two fusion heads.  sqrt(v + eps) and sqrt(v) + eps differ by
     eps / (2 v) relatively, which only shows where a gradient entry stays near 1e-4; the 70-column head has such entries (the
     unplanted columns), the six-input fusion heads have none (ratio about 1), and all three heads run the same update code;
  3. the best epoch is not the first, R and T agree on it, and the top-2 margin of T's curve is at least 10 pair-steps,
     10 / (L min_l n_pos n_neg);
  4. every validation |logit| < 15 (the metrics kernel clips probabilities to [1e-7, 1 - 1e-7]).
Build container only.

Usage:  python tests/golden/make_golden_linear_probe.py [output directory]"""
from __future__ import annotations

import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from head_probe_refs import DEFECTS, best_epoch, train_ref  # noqa: E402  (tests/ is on the path through make_golden)

N_TRAIN, N_VAL, F, L = 300, 160, 70, 3
EPOCHS, BS, LR, WD = 30, 32, 3e-3, 1e-2
FUS_LRS = (3e-3, 1e-2, 1e-3, 3e-2)          # the first (lr, seed) that meets the conditions below is taken
LABELS = ("label_edema", "label_cardiomegaly", "label_effusion")
DATA_SEED = 3
NAMES_UNI = ("_pool_duett_tokens", "_extract_cxr", "_extract_duett", "LinearHead", "masked_bce", "_eval_multi", "train_linear_head", "main")
NAMES_FUS = ("LogitFusionHead", "train_fusion_head", "_eval_from_logits", "_head_logits", "main")


def synth(rng, n):
    X = rng.standard_normal((n, F))
    logit = np.stack([-0.3 + 1.2 * X[:, 2 * l] + 0.8 * X[:, 2 * l + 1] for l in range(L)], axis=1)
    Y = (rng.random((n, L)) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    M = (rng.random((n, L)) < 0.85).astype(np.float32)
    img = logit + 1.5 * rng.standard_normal((n, L))                      # two noisy views of the planted logit: the "unimodal logits"
    ts = 0.7 * logit + 1.5 * rng.standard_normal((n, L)) + 0.2
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return {"X": f32(X), "Y": Y, "M": M, "img": f32(img), "ts": f32(ts)}


def sig(fn) -> list:
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self":
            out.append([name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)])
    return out


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
    tr["M"][:BS] = 0.0
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    out = {f"{s}_{k}": v for s, d in (("train", tr), ("val", va)) for k, v in d.items()}
    out.update(cfg=np.array([N_TRAIN, N_VAL, F, L, EPOCHS, BS]), wd=np.array(WD), labels=np.array(LABELS))
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
        epochs_seen = {"curve": [], "logits": [], "state": []}
        torch.manual_seed(seed)
        if kind == "lin":
            init = ref_u.LinearHead(F, L, dropout=0.0).state_dict()
            W0, b0, width = init["head.1.weight"].numpy().copy(), init["head.1.bias"].numpy().copy(), 0
            Xtr, Xva = tr["X"], va["X"]
            real_eval = ref_u._eval_multi

            def spy_eval(model, X, Y, M, names, device):
                res = real_eval(model, X, Y, M, names, device)
                with torch.no_grad():
                    epochs_seen["logits"].append(model.eval()(X).numpy().copy())
                epochs_seen["curve"].append(res["macro_auroc"])
                epochs_seen["state"].append({k: v.numpy().copy() for k, v in model.state_dict().items()})
                return res

            ref_u._eval_multi = spy_eval
            torch.randperm = spy_randperm
            try:
                torch.manual_seed(seed)
                model, best_ep, best_val = ref_u.train_linear_head(t(Xtr), t(tr["Y"]), t(tr["M"]), t(Xva), t(va["Y"]), t(va["M"]), list(LABELS),
                                                                   torch.device("cpu"), epochs=EPOCHS, batch_size=BS, lr=lr, weight_decay=WD,
                                                                   dropout=0.0, verbose=False)
            finally:
                ref_u._eval_multi, torch.randperm = real_eval, real_randperm
            keys = ("head.1.weight", "head.1.bias")
            torch.manual_seed(seed)
            ref_u.LinearHead(F, L, dropout=0.0)
        else:
            ftype = kind[len("fus_"):]
            init = ref_f.LogitFusionHead(L, ftype).state_dict()
            keys = ("per_label_w", "per_label_b") if ftype == "per_label" else ("head.weight", "head.bias")
            W0, b0, width = init[keys[0]].numpy().copy(), init[keys[1]].numpy().copy(), 2 if ftype == "per_label" else 0
            cat = (lambda a, b: np.stack([a, b], -1).reshape(len(a), -1)) if ftype == "per_label" else (lambda a, b: np.concatenate([a, b], -1))
            Xtr, Xva = cat(tr["img"], tr["ts"]), cat(va["img"], va["ts"])
            real_eval, real_cls, made = ref_f._eval_from_logits, ref_f.LogitFusionHead, []

            class Spy(real_cls):
                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    made.append(self)

            def spy_eval(logits, Y, M, names):
                res = real_eval(logits, Y, M, names)
                epochs_seen["logits"].append(np.array(logits, dtype=np.float32))
                epochs_seen["curve"].append(res["macro_auroc"])
                epochs_seen["state"].append({k: v.numpy().copy() for k, v in made[-1].state_dict().items()})
                return res

            ref_f._eval_from_logits, ref_f.LogitFusionHead, torch.randperm = spy_eval, Spy, spy_randperm
            try:
                torch.manual_seed(seed)
                model, best_ep, best_val = ref_f.train_fusion_head(t(tr["img"]), t(tr["ts"]), t(tr["Y"]), t(tr["M"]), t(va["img"]), t(va["ts"]),
                                                                   t(va["Y"]), t(va["M"]), list(LABELS), torch.device("cpu"), fusion_type=ftype,
                                                                   epochs=EPOCHS, batch_size=BS, lr=lr, weight_decay=WD, verbose=False)
            finally:
                ref_f._eval_from_logits, ref_f.LogitFusionHead, torch.randperm = real_eval, real_cls, real_randperm
            torch.manual_seed(seed)
            real_cls(L, ftype)
        assert len(calls) == 2 * EPOCHS, len(calls)
        perms = np.stack(calls[0::2]).astype(np.int32)
        # 1. the draw order (the default generator stands where the reference's module construction left it)
        assert np.array_equal(replay_perms(N_TRAIN, EPOCHS), perms), "the DataLoader draw order is not what head_probe replays"
        R = {"curve": np.array(epochs_seen["curve"]), "val_logits": np.stack(epochs_seen["logits"]), "best_epoch": best_ep,
             "best_W": model.state_dict()[keys[0]].numpy().copy(), "best_b": model.state_dict()[keys[1]].numpy().copy(),
             "W": epochs_seen["state"][-1][keys[0]], "b": epochs_seen["state"][-1][keys[1]]}
        kw = dict(bs=BS, lr=lr, wd=WD, label_width=width, val=(Xva, va["Y"], va["M"]))
        T = train_ref(Xtr, tr["Y"], tr["M"], W0, b0, perms, **kw)
        T["best_epoch"] = best_epoch(T["curve"])
        upto = train_ref(Xtr, tr["Y"], tr["M"], W0, b0, perms[:T["best_epoch"]], **kw)
        T["best_W"], T["best_b"] = upto["W"], upto["b"]
        gap_p = max(np.abs(R[k].reshape(T[k].shape) - T[k]).max() for k in ("W", "b", "best_W", "best_b"))
        gap_z = np.abs(R["val_logits"] - T["val_logits"]).max()
        report = {"gap_params": gap_p, "gap_logits": gap_z, "defects": {}}
        ok = R["best_epoch"] == T["best_epoch"] and T["best_epoch"] != 1
        for d in DEFECTS:                                                                # 2.
            bad = train_ref(Xtr, tr["Y"], tr["M"], W0, b0, perms, defect=d, **{k: v for k, v in kw.items() if k != "val"})
            moved = max(np.abs(bad["W"] - T["W"]).max(), np.abs(bad["b"] - T["b"]).max())
            report["defects"][d] = moved / gap_p
            ok = ok and (moved >= 100 * gap_p or (d == "eps_in_sqrt" and kind != "lin"))
        top = np.sort(T["curve"])[::-1]
        report["margin_steps"] = (top[0] - top[1]) / pair_step                           # 3.
        ok = ok and report["margin_steps"] >= 10
        report["max_abs_logit"] = np.abs(T["val_logits"]).max()                          # 4.
        ok = ok and report["max_abs_logit"] < 15 and np.abs(R["val_logits"]).max() < 15
        return ok, perms, W0, b0, R, T, report

    for kind in ("lin", "fus_linear", "fus_per_label"):
        for lr, seed in ((lr, seed) for lr in ((LR,) if kind == "lin" else FUS_LRS) for seed in range(40)):
            ok, perms, W0, b0, R, T, report = run(kind, seed, lr)
            print(f"{kind:14s} lr {lr:g} seed {seed:2d} ok={ok} best R/T {R['best_epoch']}/{T['best_epoch']} gap_params {report['gap_params']:.3g} "
                  f"gap_logits {report['gap_logits']:.3g} margin {report['margin_steps']:.1f} steps max|z| {report['max_abs_logit']:.2f} "
                  f"defects/gap {', '.join(f'{k} {v:.0f}x' for k, v in report['defects'].items())}")
            if ok:
                break
        assert ok, f"{kind}: no (lr, seed) tried meets the fixture's conditions"
        out.update({f"{kind}_seed": np.array(seed), f"{kind}_lr": np.array(lr), f"{kind}_perms": perms.astype(np.int16), f"{kind}_W0": W0, f"{kind}_b0": b0,
                    f"{kind}_gap_params": np.float64(report["gap_params"]), f"{kind}_gap_logits": np.float64(report["gap_logits"]),
                    f"{kind}_margin_steps": np.float64(report["margin_steps"]),
                    f"{kind}_defect_ratio": np.array([report["defects"][d] for d in DEFECTS])})
        for tag, res in (("R", R), ("T", T)):
            out.update({f"{kind}_{tag}_curve": np.asarray(res["curve"], dtype=np.float64), f"{kind}_{tag}_best_epoch": np.array(res["best_epoch"]),
                        f"{kind}_{tag}_W": res["W"], f"{kind}_{tag}_b": res["b"], f"{kind}_{tag}_best_W": res["best_W"],
                        f"{kind}_{tag}_best_b": res["best_b"]})
        out[f"{kind}_T_val_logits"] = T["val_logits"]
    out["defects"] = np.array(DEFECTS)
    for T_ in (24, 7):                                                               # the reference's poolings on seeded tokens
        tokens = rng.standard_normal((3, T_ + 1, 5)).astype(np.float32)
        out[f"pool_tokens_T{T_}"] = tokens
        for ft in ("rep", "hourly_mean", "multiscale", "attn_pool"):
            out[f"pool_{ft}_T{T_}"] = ref_u._pool_duett_tokens(torch.from_numpy(tokens), ft).numpy().copy()
    path = os.path.join(out_dir, "linear_probe.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 3 * 2 ** 18, os.path.getsize(path)
    print(f"wrote linear_probe.npz: {os.path.getsize(path) / 1e3:.0f} kB")

    doc = {"functions": {}, "classes": {}, "state_dict_keys": {}}
    for mod, names, tag in ((ref_u, NAMES_UNI, "unimodal_linear_probe"), (ref_f, NAMES_FUS, "logit_fusion_probe")):
        for n in names:
            obj = getattr(mod, n)
            if inspect.isclass(obj):
                doc["classes"][f"{tag}.{n}"] = {m: sig(getattr(obj, m)) for m in ("__init__", "forward")}
            else:
                doc["functions"][f"{tag}.{n}"] = sig(obj)
    doc["state_dict_keys"]["LinearHead"] = list(ref_u.LinearHead(8, 3).state_dict())
    doc["state_dict_keys"]["LinearHead(use_attn_pool=True)"] = list(ref_u.LinearHead(8, 3, use_attn_pool=True).state_dict())
    for ftype in ("linear", "mlp", "per_label"):
        doc["state_dict_keys"][f"LogitFusionHead({ftype})"] = list(ref_f.LogitFusionHead(3, ftype).state_dict())
    path = os.path.join(out_dir, "linear_probe_signatures.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(f"wrote {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
