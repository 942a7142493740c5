"""The gradient-flow kernels (csrc/grad_flow.hip) one by one against the fp64 numpy replica (tests/grad_flow_refs.py) on identical
fp32 inputs.  Tolerance 1e-10 relative on sums and norms, 1e-10 absolute on cosines and fractions: both sides sum at most ~1e5 fp32
products in fp64 in different orders, expected difference <~ 1e-11.  The seeds kernel's losses and cotangents are fp32 (the loss
kernel's arithmetic): compared at fp32 rounding."""
import numpy as np
import pytest
import torch

import grad_flow_refs as R

pytestmark = pytest.mark.gpu

from multimodal_edema_prediction_amd import grad_flow_diagnostics as G  # noqa: E402
from multimodal_edema_prediction_amd.abi import lib, stream  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 32, 1), (3, 32, 4), (7, 32, 65), (1, 256, 65), (3, 256, 1), (7, 256, 4), (16, 256, 5)]       # (K, D, B)
TOL = 1e-10


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def batch(K, D, B, seed, with_dI=False):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    mask = (rng.random((B, K)) < 0.8).astype(np.float32)
    return {"dq": f(3, K, K, D), "dI": f(B, K, K, D) if with_dI else None, "dT": f(B, K, K, D), "I": f(B, K, D), "T": f(B, K, D),
            "mask": mask, "losses": np.abs(f(3, K))}


def run_accumulate(state, b):
    G.grad_flow_accumulate(state, *(dev(b[k]) for k in ("dq", "dI", "dT", "I", "T", "mask", "losses")))


def ref_accumulate(state, b):
    return R.accumulate(state, *(b[k] for k in ("dq", "dI", "dT", "I", "T", "mask", "losses")))


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert np.all(err <= TOL * np.maximum(np.abs(want), 1.0)), (what, float(err.max()))


def report_close(got, want, K):
    """1e-10 relative on losses, norms, sensitivities, ratios; 1e-10 absolute on cosines and fractions."""
    cos_like = [3, 7, 11, 12, 13, 14, 15, 16] + [R.REPORT_HEAD + R.REPORT_PER_LABEL * k + j for k in range(K) for j in (4, 5, 6, 8, 9, 10)]
    for i, (g, w) in enumerate(zip(got, want)):
        bound = TOL if i in cos_like else TOL * max(abs(w), 1e-300)
        assert abs(g - w) <= bound, (i, g, w)


@pytest.mark.parametrize("K,D,B", SHAPES)
def test_accumulate_and_report(K, D, B):
    state = torch.zeros(G.state_size(K, D), dtype=torch.float64, device=DEV)
    want = R.new_state(K, D)
    assert state.numel() == want.size
    for i, with_dI in enumerate((False, True, False)):
        b = batch(K, D, B, 100 * K + D + B + i, with_dI)
        if i == 2:
            b["mask"][:, K - 1] = 0.0                          # a label without a valid sample in this batch
            b["dq"][:, K - 1] = 0.0
            b["dT"][:, K - 1] = 0.0
        run_accumulate(state, b)
        ref_accumulate(want, b)
        close(state.cpu().numpy(), want, f"state after batch {i}")
    alphas = (0.5, 0.25, 1.0)
    out = torch.empty(R.REPORT_HEAD + R.REPORT_PER_LABEL * K, dtype=torch.float64, device=DEV)
    G.grad_flow_report(state, alphas, out, K, D)
    report_close(out.cpu().numpy(), R.report(want, alphas, K, D), K)
    # the report of the kernel's OWN state equals the replica's report of that state too (report kernel alone)
    report_close(out.cpu().numpy(), R.report(state.cpu().numpy(), alphas, K, D), K)


def test_zero_gradients_and_unseen_label():
    """All-zero gradients: every cosine is 0 by the denominator rule, every fraction and ratio 0, nothing is NaN; a label that never
    has a valid sample divides by max(valid, 1)."""
    K, D, B = 3, 32, 4
    b = batch(K, D, B, 7)
    for key in ("dq", "dT"):
        b[key][:] = 0.0
    b["mask"][:, 1] = 0.0
    state = torch.zeros(G.state_size(K, D), dtype=torch.float64, device=DEV)
    run_accumulate(state, b)
    out = torch.empty(R.REPORT_HEAD + R.REPORT_PER_LABEL * K, dtype=torch.float64, device=DEV)
    G.grad_flow_report(state, (0.5, 0.5, 1.0), out, K, D)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    report_close(got, R.report(ref_accumulate(R.new_state(K, D), b), (0.5, 0.5, 1.0), K, D), K)
    assert got[3] == got[7] == got[11] == 0.0 and not got[12:18].any() and got[24] == 1.0 and got[25] == B
    assert got[R.REPORT_HEAD + R.REPORT_PER_LABEL] == 0.0      # label 1: no valid sample


def test_two_calls_equal_one_call_on_the_concatenation():
    """Where that is defined: the sensitivities, the valid counts and the sample count are sums over samples."""
    K, D = 3, 32
    a, b = batch(K, D, 5, 1, True), batch(K, D, 65, 2, True)
    both = {k: np.concatenate([a[k], b[k]]) for k in ("dI", "dT", "I", "T", "mask")}
    both.update(dq=a["dq"], losses=a["losses"])
    two, one = (torch.zeros(G.state_size(K, D), dtype=torch.float64, device=DEV) for _ in range(2))
    run_accumulate(two, a)
    run_accumulate(two, b)
    run_accumulate(one, both)
    n = 3 * K * K * D
    two, one = two.cpu().numpy(), one.cpu().numpy()
    close(two[n + 6:], one[n + 6:], "sample count, valid counts, sensitivities")
    assert two[n + 5] == 2.0 and one[n + 5] == 1.0


@pytest.mark.parametrize("K,D,B", [(7, 256, 65)])
def test_repeated_run_is_bit_identical(K, D, B):
    outs = []
    for _ in range(2):
        state = torch.zeros(G.state_size(K, D), dtype=torch.float64, device=DEV)
        for i in range(2):
            run_accumulate(state, batch(K, D, B, i, True))
        out = torch.empty(R.REPORT_HEAD + R.REPORT_PER_LABEL * K, dtype=torch.float64, device=DEV)
        G.grad_flow_report(state, (0.5, 0.5, 1.0), out, K, D)
        outs.append((state.cpu(), out.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("K,B", [(1, 1), (3, 4), (7, 65), (16, 5)])
@pytest.mark.parametrize("with_pw", [False, True])
def test_seeds(K, B, with_pw):
    rng = np.random.default_rng(K * 100 + B)
    logits = [(2.0 * rng.standard_normal((B, K))).astype(np.float32) for _ in range(3)]
    y = (rng.random((B, K)) < 0.4).astype(np.float32)
    mask = (rng.random((B, K)) < 0.8).astype(np.float32)
    if K > 1:
        mask[:, 1] = 0.0                                       # a label with zero valid samples: zero loss, zero cotangent
    lw = (0.5 + rng.random(K)).astype(np.float32)
    pw = (0.5 + rng.random(K)).astype(np.float32) if with_pw else None
    got = G.grad_flow_seeds(*(dev(a) for a in logits), dev(y), dev(mask), dev(lw), dev(pw), 1e-6)
    want = R.seeds(*logits, y, mask, lw, pw, 1e-6)
    for g, w, name in zip(got, want, ("losses", "cot_img", "cot_ts", "cot_fus")):
        g = g.cpu().numpy()
        assert g.shape == w.shape
        # fp32 arithmetic of the loss kernel (__expf, log1pf, fp32 sums over B): 1e-5 of the largest value
        assert np.abs(g - w).max() <= 1e-5 * max(np.abs(w).max(), 1e-3), (name, np.abs(g - w).max())
        assert np.array_equal(g == 0.0, w == 0.0) or name == "losses", name          # exact zeros outside column k of replica (., k)
    again = G.grad_flow_seeds(*(dev(a) for a in logits), dev(y), dev(mask), dev(lw), dev(pw), 1e-6)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("K,D", [(1, 32), (3, 32), (7, 256), (16, 256)])
def test_query_geometry(K, D):
    rng = np.random.default_rng(K + D)
    rows = rng.standard_normal((3, K, D)).astype(np.float32)
    if K > 1:
        rows[1, 1] = 0.0                                       # a zero row: clamp_min(1e-12), Gram row and column 0
    out = torch.empty(3 * K * K + K + 1, dtype=torch.float64, device=DEV)
    G.query_geometry(dev(rows), out)
    got, want = out.cpu().numpy(), R.query_geometry(rows)
    assert np.abs(got - want)[:3 * K * K].max() <= TOL and abs(got[-1] - want[-1]) <= TOL
    close(got[3 * K * K:-1], want[3 * K * K:-1], "prototype norms")
    out2 = torch.empty_like(out)
    G.query_geometry(dev(rows), out2)
    assert torch.equal(out, out2)


def test_invalid_arguments_return_negative():
    L = lib()
    K, D, B = 3, 32, 4
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    d = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p, q, s = f.data_ptr(), d.data_ptr(), stream()
    assert L.medp_grad_flow_seeds(None, p, p, p, p, p, None, 1e-6, p, p, p, p, p, B, K, s) < 0
    assert L.medp_grad_flow_seeds(p, p, p, p, p, p, None, 1e-6, p, p, p, p, p, 0, K, s) < 0
    assert L.medp_grad_flow_seeds(p, p, p, p, p, p, None, 1e-6, p, p, p, p, p, B, 17, s) < 0
    assert L.medp_grad_flow_accumulate(p, None, None, p, p, p, p, q, q, B, K, D, s) < 0
    assert L.medp_grad_flow_accumulate(p, None, p, p, p, p, p, q, q, B, 0, D, s) < 0
    assert L.medp_grad_flow_accumulate(p, None, p, p, p, p, p, q, q, -1, K, D, s) < 0
    assert L.medp_grad_flow_accumulate(p, None, p, p, p, p, p, None, q, B, K, D, s) < 0
    assert L.medp_grad_flow_report(None, 0.5, 0.5, 1.0, q, K, D, s) < 0
    assert L.medp_grad_flow_report(q, 0.5, 0.5, 1.0, q, K, 0, s) < 0
    assert L.medp_query_geometry(p, None, K, D, s) < 0
    assert L.medp_query_geometry(p, q, 17, D, s) < 0
    assert L.medp_grad_flow_state_doubles(0, D) == 0 and L.medp_grad_flow_ws_doubles(B, 17) == 0
    assert L.medp_grad_flow_state_doubles(K, D) == R.state_size(K, D)
    torch.cuda.synchronize()
    assert not d.any() and not f.any()                         # nothing was launched
