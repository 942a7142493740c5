"""CPU: the host references of tests/attn_dh64_refs.py hold before tests/test_gpu_attn_dh64_paths.py measures the kernels with them.
  - `twin` (the backward with the kernels' bf16 roundings) stays within 1 % of the fp64 gradients on a nearly uniform softmax;
  - `trace_blocks` sees no later move of the running maximum on randn under the deferred rule, and sees every path that the `ramp` and
    `late_key` inputs exist to force;
  - a one-hot softmax leaves the twin exactly the index map in O, the scatter-add in dV, and dQ / dK inside the derived rounding bound."""
import pytest
import torch

import attn_dh64_refs as R

SCALE = 0.125
ONE_HOT_S = [1, 16, 17, 33, 192, 257, 320, 321, 400, 512, 577, 641, 1370]
KINDS = ["perm", "reverse", "last", "first"]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("S", [64, 257])
def test_twin_against_fp64_on_uniform_inputs(S):
    B, H = 2, 2
    q, k, v = R.uniform_inputs(B, S, H, seed=S)
    dout = torch.randn(B, H, S, 64, generator=torch.Generator().manual_seed(S + 1))
    ref, tw = R.ref64(q, k, v, dout, SCALE), R.twin(q, k, v, dout, SCALE)
    for name in ("dq", "dk", "dv", "o"):
        rel = _rel(tw[name], ref[name])
        print(f"S={S} {name}: twin vs fp64 relative Frobenius error {rel:.3e}")
        assert rel <= 1e-2, (name, rel)
    assert float((tw["lse2"].double() - ref["lse2"]).abs().max()) <= 1e-4


def test_twin_row_sums_of_ds_vanish():
    """D from bf16(dout): sum_j P_ij (dP_ij - D_i) = <dOb_i, P v - O_i>, rounding of O only.  What the kernels' gradients rest on."""
    q, k, v, _ = R.peaked_inputs(1, 257, 1, 3.0, seed=5)
    dout = torch.randn(1, 1, 257, 64, generator=torch.Generator().manual_seed(6))
    tw = R.twin(q, k, v, dout, SCALE)
    s = (q @ k.transpose(-1, -2)).double()
    p = torch.softmax(s * SCALE, dim=-1)
    dp = tw["dob"].double() @ v.double().transpose(-1, -2)
    rowsum = (p * (dp - tw["dsum"].double().unsqueeze(-1))).sum(-1).abs()
    # |<dOb_i, P v - O_i>| <= sum_d |dOb_id| * 2^-8 |O_id| (one bf16 rounding of O, bf16 P before the product adds as much again)
    bound = (tw["dob"].abs() * tw["o"].abs()).sum(-1).double() * 2.0 ** -7
    assert bool((rowsum <= bound + 1e-12).all()), float((rowsum / (bound + 1e-12)).max())


def test_trace_blocks_randn_never_moves_later_under_defer():
    S = 577
    g = torch.Generator().manual_seed(S)
    q, k = [R.bf16(torch.randn(1, 1, S, 64, generator=g)) for _ in range(2)]
    t = R.trace_blocks(q, k, S, defer=True)
    print(t)
    assert t.later_blocks == 37 * 9                     # 37 subtiles, 5 + 5 blocks
    assert t.later_moves == 0 and t.chunk_moves == 0 and t.tail_moves == 0
    assert R.trace_blocks(q, k, S, defer=False).later_moves > 0          # the same walk without the threshold does move


@pytest.mark.parametrize("S", [321, 400, 512, 577, 1370])
def test_trace_blocks_sees_the_forced_paths(S):
    defer = S >= 512
    q, k, _ = R.forcing_inputs(1, S, 1, "ramp", seed=S)
    t = R.trace_blocks(q, k, S, defer)
    print("ramp", S, t)
    assert t.later_moves > 0 and t.chunk_moves > 0
    assert t.deferred > 0 if defer else t.deferred == 0
    q, k, _ = R.forcing_inputs(1, S, 1, "late_key", seed=S)
    t = R.trace_blocks(q, k, S, defer)
    print("late_key", S, t)
    assert t.later_moves > 0 and t.chunk_moves > 0
    assert t.tail_moves > 0 if S % 64 else t.tail_moves == 0


def test_late_keys_lie_where_they_are_meant_to():
    assert R.late_keys(321) == [256 + 37, 320]              # chunk 1 holds one key: the full block is chunk 0's last
    assert R.late_keys(400) == [320 + 37, 320, 399]
    assert R.late_keys(512) == [320 + 128 + 37, 320, 511]
    assert R.late_keys(577) == [320 + 192 + 37, 320, 576]
    assert R.late_keys(1370) == [1280 + 37, 320, 1369]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", ONE_HOT_S)
def test_one_hot_inputs_and_the_twin(S, kind):
    B = H = 2 if S <= 577 else 1
    q, k, v, pi = R.one_hot_inputs(B, S, H, kind, seed=1000 + S)          # asserts the 40-nat lead itself
    if kind == "perm" and S > 16 and B > 1:
        assert not torch.equal(pi[0, 0], pi[1, 1])
    dout = torch.randn(B, H, S, 64, generator=torch.Generator().manual_seed(S))
    tw, ex = R.twin(q, k, v, dout, SCALE), R.one_hot_expect(q, k, v, pi, dout, SCALE)
    assert torch.equal(tw["o"], ex["o"])
    assert float((tw["lse2"].double() - ex["lse2"]).abs().max()) <= 2e-3 + 1e-4 * float(ex["lse2"].max())
    assert _rel(tw["dv"], ex["dv"]) <= 1e-6
    assert bool(((tw["dv"].double() - ex["dv"]).abs() <= ex["tol_v"]).all())
    rq = float((tw["dq"].abs().double() / ex["bound_q"]).max())
    rk = float((tw["dk"].abs().double() / ex["bound_k"]).max())
    print(f"S={S} {kind}: max |dQ| / bound {rq:.3e}, max |dK| / bound {rk:.3e}")
    assert rq <= 1.0 and rk <= 1.0


def test_one_hot_bound_rejects_an_inconsistent_d():
    """The bound is sharp enough to matter: D formed from the fp32 dout while dP uses bf16(dout) lands far outside it."""
    S = 257
    q, k, v, pi = R.one_hot_inputs(1, S, 1, "perm", seed=1000 + S)
    dout = torch.randn(1, 1, S, 64, generator=torch.Generator().manual_seed(S))
    ex = R.one_hot_expect(q, k, v, pi, dout, SCALE)
    dob = R.bf16(dout)
    d_bad = (dout * ex["o"]).sum(-1, keepdim=True)
    p = torch.softmax((q @ k.transpose(-1, -2)).double() * SCALE, dim=-1).float()
    ds = R.bf16(p * (dob @ v.transpose(-1, -2) - d_bad) * SCALE)
    assert float(((ds @ k).abs().double() / ex["bound_q"]).max()) > 10.0
