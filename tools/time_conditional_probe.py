#!/usr/bin/env python3
"""The conditional-information probe on synthetic gathered splits (N = 4096 rows per split, K = 7 labels, D = 256 token channels, 90 %
of the labels known; the reference's defaults otherwise: logit_c 100, token_c 1, 1000 bootstrap replicates, 100 conditional
permutations in 10 bins): the entry points of csrc/cond_probe.hip by HIP events after warm-up, `fit_probes` and the whole
`run_probe` by wall clock around a device synchronise.  For the Newton-terms pass of the token group the time is printed beside its
floors: bytes = the fp32 features once (n (F) 4 B per problem), FLOP = n (F + 1)(F + 2) for the upper triangle of the weighted Gram
matrix plus 4 n F for scores and gradient, against 8 TB/s and the 78.6 TFLOP/s vector-fp64 peak.

Usage:  python tools/time_conditional_probe.py [N]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodal_edema_prediction_amd import conditional_information_probe as cip

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K, D, HBM_PEAK, FP64_PEAK = 7, 256, 8.0e12, 78.6e12
dev = torch.device("cuda")
LABELS = [f"label_{i}" for i in range(K)]


def synth_split(n, seed):
    """What `gather` returns: the label depends on the image logit and on two token channels; the ts logit is a noisy view of them."""
    rng = np.random.default_rng(seed)
    token = rng.standard_normal((n, K, D))
    img = 1.2 * rng.standard_normal((n, K))
    signal = 0.8 * token[:, :, 0] - 0.5 * token[:, :, 1]
    ts = signal + 0.7 * rng.standard_normal((n, K))
    y = rng.random((n, K)) < 1 / (1 + np.exp(-(-0.8 + 0.9 * img + signal)))
    mask = rng.random((n, K)) < 0.9
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
    return {"img": f32(img), "ts": f32(ts), "fus": f32(img + 0.5 * ts), "token": f32(token), "y": f32(y), "mask": f32(mask)}


def timed(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


train, test = synth_split(N, 1), synth_split(N, 2)
feats, tok = cip._feature_tensors(train)
mask = train["mask"].cpu().numpy()
problems = [(k, name) for k in range(K) for name in ("image_cal",) + cip.PROBE_NAMES]
narrow, token = cip._group_entries(problems, mask, D)
print(f"split: N = {N} rows, K = {K}, D = {D}; known per label {[int(mask[:, k].sum()) for k in range(K)]}")
for title, group, X, Fmax in (("narrow group (21 problems, Fmax 3)", narrow, feats, 3), (f"token group ({K} problems, F {1 + D})", token, tok, 1 + D)):
    table = cip.ProblemTable([e for _, e in group], dev, Fmax)
    mean, scale = cip.probe_moments(X, table)
    theta = 0.05 * torch.randn((table.P, Fmax + 1), dtype=torch.float64, device=dev)
    l2 = torch.full((table.P,), 1e-4, dtype=torch.float64, device=dev)
    ws = cip.terms_workspace(table)
    t_m = timed(lambda: cip.probe_moments(X, table))
    t_h = timed(lambda: cip.logistic_newton_terms(X, train["y"], table, theta, mean, scale, l2, True, ws))
    t_v = timed(lambda: cip.logistic_newton_terms(X, train["y"], table, theta, mean, scale, l2, False, ws))
    t_s = timed(lambda: cip.probe_scores(X, table, theta, mean, scale))
    rows = table.rows_total
    nbytes = sum(q.n_rows * q.F * 4 for q in table.host[:table.P])
    flop = sum(q.n_rows * ((q.F + 1) * (q.F + 2) + 4 * q.F) for q in table.host[:table.P])
    floor_ms = max(nbytes / HBM_PEAK, flop / FP64_PEAK) * 1e3
    print(f"{title}: {rows} rows in all")
    print(f"  probe_moments                 : {t_m:9.4f} ms")
    print(f"  logistic_newton_terms (f,g,H) : {t_h:9.4f} ms   bytes {nbytes / 1e6:.1f} MB -> {nbytes / HBM_PEAK * 1e3:.4f} ms at 8 TB/s; "
          f"{flop / 1e9:.2f} GFLOP -> {flop / FP64_PEAK * 1e3:.4f} ms at 78.6 TFLOP/s; ratio to the larger floor {t_h / floor_ms:.1f}")
    print(f"  logistic_newton_terms (f,g)   : {t_v:9.4f} ms   (the line search's value-only mode)")
    print(f"  probe_scores                  : {t_s:9.4f} ms")

torch.cuda.synchronize()
t0 = time.perf_counter()
fits = cip.fit_probes(train, problems)
torch.cuda.synchronize()
print(f"fit_probes, 28 problems        : {time.perf_counter() - t0:9.3f} s wall; Newton iterations {sorted({m.n_iter for m in fits})}, "
      f"largest final max|g| {max(m.max_gradient for m in fits):.2e}")
t0 = time.perf_counter()
rows, summary, _ = cip.run_probe(train, test, LABELS, tuple(range(K)), verbose=False)
torch.cuda.synchronize()
print(f"run_probe, {K} labels x 3 probes : {time.perf_counter() - t0:9.3f} s wall  (28 fits, 21 x (1000 bootstrap replicates x 2, 100 permutations))")
for r in rows[:6]:
    print(f"  {r['label']:8s} {r['probe']:18s} BCE gain {r['bce_gain']:+.5f} [{r['bce_gain_ci_low']:+.5f}, {r['bce_gain_ci_high']:+.5f}]  {r['evidence']}")
