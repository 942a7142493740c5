"""tests/gru_refs.py is right, and the bounds built from it can tell (no GPU).

Pinning: the unrounded fp64 forward against torch.nn.GRU (gi fed through an identity W_ih) to 1e-12; the unrounded fp64 backward
against fp64 autograd through that recurrence (dgi, and dghn as the gradient of the W_hn h + b_hn term) to 1e-10; `bf16_rne` of an
fp64 value against the nearer of its two bf16 neighbours found in fp64.

The comparison of tests/test_gpu_gru_kernels.py (gru_refs.forward_distance / backward_distance, bound max(8 x noise, 16 fp32 ulps)),
run here on CPU stand-ins for a kernel, at every (S, T) of gru_refs.CASES with the inputs the GPU file uses.
Passes: the fp32 replica, and an fp32 twin with the kernel's own formulas (sigmoid as 1 / (1 + exp(-x)), tanh as 2 sigmoid(2x) - 1,
bf16 products summed in another order).  Measured: noise 0.5e-7 .. 7e-7 per output, so every bound is its 16-ulp floor or just above
(forward 1.9e-6 .. 5.8e-6, backward 1.9e-6 .. 7.5e-6 on gradients up to 3.9); both stand-ins stay below 0.13 of it.
Rejected, each at least twice the bound away in every output the error reaches (measured: 280x at the least):
  forward, T >= 2   the hidden tile cut to bf16 towards zero instead of rounded            hseq, gates, hn
  backward          h_{t-1} at t = 0 read as hseq[:, 0] instead of 0                       dgi (its z columns at t = 0)
  backward, T >= 2  the n columns of the carried product taken from dnp instead of dgn     dgi, dghn
  backward, T >= 2  the gradient tile cut towards zero instead of rounded: the written dgh16 is then not bf16(dgi | dghn), which the
                    GPU file compares bit for bit; and were only the tile in LDS cut, dgi and dghn move by 2e-3
The same mutants measured with both evaluations running free, as the first draft of these tests had it, are printed beside: there the
truncated hidden tile is 1.1x the bound at T = 24 and the truncated gradient tile is below it (gru_refs' docstring says why).
NOT COVERED by any test here: a kernel that rounds a tile element to the wrong side only at an exact tie (ties to even or away):
ties do not occur in these inputs.

Each case prints its noise, bounds and distances (`pytest -s` shows them)."""
import pytest
import torch

import gru_refs as R

F32, F64 = torch.float32, torch.float64
D = R.D


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


def show(what, names, judged):
    away, bounds, nz = judged
    print(f"    {what}: " + "  ".join(f"{k} {a:.2e} / bound {b:.2e} (noise {n:.1e})" for k, a, b, n in zip(names, away, bounds, nz)))


def passes(judged):
    return all(a <= b for a, b in zip(judged[0], judged[1]))


def kernel_twin_fwd(gi, w_hh, b_hh, round_h=R.bf16_rne):
    """The forward kernels' own formulas in fp32, free running; the bf16 products are exact in fp32 and summed in fp64 (another order
    than the replica's)."""
    def sig(v):
        return 1.0 / (1.0 + torch.exp(-v))
    w, b, d = R.bf16_rne(w_hh), b_hh, D
    h, hs, gates, hns = torch.zeros(gi.shape[0], d), [], [], []
    for t in range(gi.shape[1]):
        gh = (round_h(h).double() @ w.double().t()).float()
        r, z = sig(gi[:, t, :d] + gh[:, :d] + b[:d]), sig(gi[:, t, d:2 * d] + gh[:, d:2 * d] + b[d:2 * d])
        hn = gh[:, 2 * d:] + b[2 * d:]
        n = 2.0 * sig(2.0 * (gi[:, t, 2 * d:] + r * hn)) - 1.0
        h = (1.0 - z) * n + z * h
        hs.append(h); gates.append(torch.cat([r, z, n], 1)); hns.append(hn)
    return torch.stack(hs, 1), torch.stack(gates, 1), torch.stack(hns, 1)


# ---------------------------------------------------------------------------------------------------------------- rounding
def test_bf16_rne_of_fp64_is_the_nearer_bf16_neighbour():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g, dtype=F64) * torch.rand(200000, generator=g, dtype=F64).mul(20).sub(10).exp2()
    # fp64 values that round to fp32 exactly on a bf16 tie: the tie itself, and a little to either side of it
    tie = (torch.randn(4096, generator=g).view(torch.int32) & ~0xFFFF | 0x8000).view(F32).double()
    x = torch.cat([x, tie, tie * (1 + 2.0 ** -40), tie * (1 - 2.0 ** -40)])
    m, e = torch.frexp(x)                                          # x = m 2^e, 0.5 <= |m| < 1: bf16 keeps 8 bits of m
    s = m * 256
    lo, frac = torch.floor(s), s - torch.floor(s)
    want = torch.where(frac > 0.5, lo + 1, torch.where(frac < 0.5, lo, lo + (lo % 2)))
    assert torch.equal(R.bf16_rne(x), torch.ldexp(want / 256, e))
    assert torch.equal(R.bf16_rne(x.float()), x.float().bfloat16().float())
    assert torch.equal(R.bf16_trunc(x), torch.ldexp(torch.trunc(s) / 256, e))


# ---------------------------------------------------------------------------------------------------------------- pinning
def test_unrounded_forward_is_torch_gru():
    S, T, d = 5, 6, D
    x = R.inputs(S, T)
    gru = torch.nn.GRU(3 * d, d, batch_first=True, dtype=F64)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * d, dtype=F64)); gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(x["w_hh"]); gru.bias_hh_l0.copy_(x["b_hh"])
        want, _ = gru(x["gi"].double())
    hseq, gates, hn = R.gru_fwd(x["gi"], x["w_hh"], x["b_hh"], F64, round_operands=False)
    print(f"against torch.nn.GRU: {dist(hseq, want):.3e}")
    assert dist(hseq, want) <= 1e-12
    h_prev = R.entering(hseq)
    assert dist(hn, h_prev @ x["w_hh"].double()[2 * d:].t() + x["b_hh"].double()[2 * d:]) <= 1e-12
    assert dist(hseq, (1 - gates[..., d:2 * d]) * gates[..., 2 * d:] + gates[..., d:2 * d] * h_prev) <= 1e-12
    # restarted at every step from its own states, the replica reproduces itself
    again = R.gru_fwd(x["gi"], x["w_hh"], x["b_hh"], F64, round_operands=False, carried=h_prev)
    assert all(torch.equal(a, c) for a, c in zip(again, (hseq, gates, hn)))


def test_unrounded_backward_is_autograd():
    S, T, d = 5, 6, D
    x = R.inputs(S, T)
    gi, w, b = x["gi"].double().requires_grad_(True), x["w_hh"].double().requires_grad_(True), x["b_hh"].double()
    h, hs, hns = torch.zeros(S, d, dtype=F64), [], []
    for t in range(T):
        gh = h @ w.t()
        hn = gh[:, 2 * d:] + b[2 * d:]
        r, z = torch.sigmoid(gi[:, t, :d] + gh[:, :d] + b[:d]), torch.sigmoid(gi[:, t, d:2 * d] + gh[:, d:2 * d] + b[d:2 * d])
        h = (1 - z) * torch.tanh(gi[:, t, 2 * d:] + r * hn) + z * h
        hs.append(h); hns.append(hn)
    hseq, gates, hn = R.gru_fwd(x["gi"], x["w_hh"], x["b_hh"], F64, round_operands=False)
    assert torch.equal(torch.stack(hs, 1).detach(), hseq)          # the recurrence differentiated here is the pinned one
    grads = torch.autograd.grad((torch.stack(hs, 1) * x["dh"].double()).sum(), [gi] + hns)
    dgi, dghn, dgh, dgi_copy = R.gru_bwd(x["dh"], gates, hn, hseq, x["w_hh"], F64, round_operands=False)
    print(f"against autograd: dgi {dist(dgi, grads[0]):.3e}  dghn {dist(dghn, torch.stack(grads[1:], 1)):.3e}")
    assert dist(dgi, grads[0]) <= 1e-10 and dist(dghn, torch.stack(grads[1:], 1)) <= 1e-10
    assert torch.equal(dgh, torch.cat([dgi[..., :2 * d], dghn], 2)) and torch.equal(dgi_copy, dgi)


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("S,T", R.CASES)
def test_forward_bound_passes_the_twins_and_rejects_a_truncated_hidden_tile(S, T):
    x = R.inputs(S, T)
    args = (x["gi"], x["w_hh"], x["b_hh"])
    names = ("hseq", "gates", "hn")
    print(f"fwd S {S} T {T}")
    for what, got in (("fp32 replica", R.gru_fwd(*args, F32)), ("kernel twin", kernel_twin_fwd(*args))):
        judged = R.forward_distance(x, got)
        show(what, names, judged)
        assert passes(judged), what
    plain = R.forward_distance(x, R.gru_fwd(*args, F32, round_operands=False), round_operands=False)
    show("fp32 plain GRU, running free (medp_gru_fwd_f32's comparison)", names, plain)
    assert passes(plain)
    free = R.noise(R.gru_fwd, *args)
    print("    running free, fp32 against fp64 replica: " + "  ".join(f"{k} {v:.2e}" for k, v in zip(names, free)))
    if T < 2:
        return                                                     # h_0 = 0: nothing is rounded, there is no such mutant
    away, bounds, nz = judged = R.forward_distance(x, kernel_twin_fwd(*args, round_h=R.bf16_trunc))
    show("truncated hidden tile", names, judged)
    for a, bnd in zip(away, bounds):                               # the cap on FACTOR: no bound above half the mutant's distance
        assert a >= 2 * bnd
    cut = [dist(a, c) for a, c in zip(R.gru_fwd(*args, F64, round_h=R.bf16_trunc), R.forward_free(S, T))]
    print("    truncated hidden tile, both running free: " + "  ".join(f"{k} {v:.2e} = {v / R.bound(f, r):.1f}x 8x-free-noise bound"
                                                                       for k, v, f, r in zip(names, cut, free, R.forward_free(S, T))))


# ---------------------------------------------------------------------------------------------------------------- backward
def rounded_copy_is_exact(dgi, dghn, dgh16):
    """the GPU file's bit comparison: dgh16 is bf16(drp | dzp | dgn) of the written fp32 values"""
    return torch.equal(dgh16.float(), R.bf16_rne(torch.cat([dgi[..., :2 * D], dghn], 2).float()))


@pytest.mark.parametrize("S,T", R.CASES)
def test_backward_bound_passes_the_replica_and_rejects_the_mutants(S, T):
    args = R.backward_args(S, T)
    names = ("dgi", "dghn")
    ref = R.gru_bwd(*args, F64)
    print(f"bwd S {S} T {T}: max|dgi| {float(ref[0].abs().max()):.2f} max|dghn| {float(ref[1].abs().max()):.2f}")
    got = R.gru_bwd(*args, F32)
    judged = R.backward_distance(args, got)
    show("fp32 replica", names, judged)
    assert passes(judged) and rounded_copy_is_exact(*got[:3])
    free = R.noise(R.gru_bwd, *args)[:2]
    print("    running free, fp32 against fp64 replica: " + "  ".join(f"{k} {v:.2e}" for k, v in zip(names, free)))

    away, bounds, _ = judged = R.backward_distance(args, R.gru_bwd(*args, F32, mutant="h0"))
    show("h_-1 = hseq[:, 0]", names, judged)
    assert away[0] >= 2 * bounds[0]
    if T < 2:
        return                                                     # nothing is carried
    away, bounds, _ = judged = R.backward_distance(args, R.gru_bwd(*args, F32, mutant="dnp"))
    show("dnp carried for dgn", names, judged)
    assert away[0] >= 2 * bounds[0] and away[1] >= 2 * bounds[1]
    cut = R.gru_bwd(*args, F32, mutant="trunc")
    assert not rounded_copy_is_exact(*cut[:3])                      # the kernel writes the tile it used: the bits give it away
    away, bounds, _ = judged = R.backward_distance(args, (cut[0], cut[1], R.bf16_rne(torch.cat([cut[0][..., :2 * D], cut[1]], 2))))
    show("gradient tile truncated in LDS only", names, judged)
    assert away[0] >= 2 * bounds[0] and away[1] >= 2 * bounds[1]
    cut64 = R.gru_bwd(*args, F64, mutant="trunc")
    print("    truncated gradient tile, both running free: " + "  ".join(f"{k} {dist(c, r):.2e} = {dist(c, r) / R.bound(f, r):.1f}x 8x-free-noise bound"
                                                                         for k, c, r, f in zip(names, cut64, ref, free)))


# ---------------------------------------------------------------------------------------------------------------- saturation
@pytest.mark.parametrize("scale", [30.0, 200.0])
def test_saturated_inputs_stay_finite_and_the_twins_pass(scale):
    """The saturation cases of the GPU file: how many r / z gates are exactly 0 or 1 there, and the same comparison."""
    S, T = 17, 3
    x = R.inputs(S, T, scale)
    ref = R.forward_free(S, T, scale)
    rz = ref[1][..., :2 * D].float()
    pinned = float(((rz == 0) | (rz == 1)).float().mean())
    print(f"gi x {scale:.0f}: r/z exactly 0 or 1 in fp32: {pinned:.0%}")
    assert all(bool(torch.isfinite(t).all()) for t in ref) and pinned > 0.25
    for what, got in (("fp32 replica", R.gru_fwd(x["gi"], x["w_hh"], x["b_hh"], F32)), ("kernel twin", kernel_twin_fwd(x["gi"], x["w_hh"], x["b_hh"]))):
        judged = R.forward_distance(x, got)
        show(what, ("hseq", "gates", "hn"), judged)
        assert passes(judged), what
    args = R.backward_args(S, T, scale)
    got = R.gru_bwd(*args, F32)
    judged = R.backward_distance(args, got)
    show("backward, fp32 replica", ("dgi", "dghn"), judged)
    assert passes(judged) and all(bool(torch.isfinite(t).all()) for t in got)
