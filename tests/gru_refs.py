"""Replica of the GRU kernels of csrc/trajectory.hip (torch on the CPU, the dtype a parameter), the inputs, the bound rule and the
two comparisons that tests/test_gru_refs_cpu.py and tests/test_gpu_gru_kernels.py share.  TEST INFRASTRUCTURE ONLY.

The replica restates what the kernels compute and rounds ONLY where they round: the bf16 weight cast and `pack_bf2` on the tile
that feeds the MFMA, both round-to-nearest-even.  Everything else runs in the dtype asked for, so the same function is the fp64
truth (`dtype=torch.float64`) and, in fp32, a correct kernel's twin up to the order of its sums and the last ulp of exp / tanh.
`noise` is the distance between the two: what a correct fp32 implementation of these formulas is allowed, measured at the test's
own inputs.  The bound is max(FACTOR x noise, 16 fp32 ulps of max(1, max|reference|)).

Why the comparison restarts the replica at every step.  Let both evaluations run free and their distance is no longer fp32
rounding: now and then a tile element lies so close to a bf16 tie that the two round it to different sides (a "flip"), and from
there on one sequence differs by a bf16 ulp of that element times a weight: up to 4e-3 * 0.3.  At (S, T) = (37, 24) twelve seeds
gave a free-running fp32-against-fp64 distance on hseq from 4e-6 to 7e-4 (5 to 700 tile elements flipped), and 2 of 12 seeds flip already
at (33, 3).  A kernel's flips are not the replica's, so a bound of 8 x that number is a lottery in both directions: it fails a correct
kernel where the replica happened not to flip, and where it did flip the bound (3e-3 to 8e-3 at T = 24) no longer rejects the
truncated tile (3e-3).  What a kernel rounds is visible in what it writes: the tile of step t is bf16(hseq[:, t - 1]) and the
backward's tile is dgh16.  So `forward_distance` / `backward_distance` give the fp64 replica, at every step, the state (the tile)
the implementation under test itself carried into that step.  Then no rounding can go two ways, the noise is fp32 rounding alone
(1e-7), every step of every sequence is held to about 2e-6, and by induction from h_0 = 0 (carry_T = 0) so is the whole recurrence.
That the tiles are the correct rounding of the written values is a comparison of bits in the GPU file.

Not part of the replica: the hooks `round_h` and `mutant`.  They exist for tests/test_gru_refs_cpu.py, which shows that the bound
rejects a replica that is wrong in one place."""
from __future__ import annotations

import functools

import torch

D = 128                                   # the only hidden size the kernels are built for
FACTOR = 8                                # bound = max(FACTOR * noise, FLOOR_ULPS fp32 ulps of max(1, max|ref|))
FLOOR_ULPS = 16
F32, F64 = torch.float32, torch.float64
# (sequences, steps): one live lane | one short of, exactly, one past a 16-sequence workgroup | three workgroups, the last with one
# live lane  x  only the zeroed LDS tile | both LDS buffers | a buffer reused; the workload's 24 steps at the two ragged S only
CASES = [(S, T) for S in (1, 15, 16, 17, 33) for T in (1, 2, 3)] + [(17, 24), (33, 24)]


# ---------------------------------------------------------------------------------------------------------------- rounding
def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """x rounded to the nearest bf16 (ties to even), returned in x's dtype.  fp64 goes through fp32 and the one case where two
    roundings differ from one (the fp32 value is exactly a bf16 tie, the fp64 value is not) is decided by the fp64 value."""
    if x.dtype != F64:
        return x.to(torch.bfloat16).to(x.dtype)
    f = x.to(F32)
    bits = f.view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    down = (bits & ~0xFFFF).view(F32)                              # towards zero
    up = ((bits & ~0xFFFF) + 0x10000).view(F32)                    # away from zero (sign-magnitude: the same add for either sign)
    y = f.to(torch.bfloat16).to(F32)
    y = torch.where(tie & (x.abs() > f.double().abs()), up, y)
    y = torch.where(tie & (x.abs() < f.double().abs()), down, y)
    return y.double()


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """x cut to bf16 towards zero: the wrong rounding mode of the mutants."""
    f = x.to(F32)
    over = f.double().abs() > x.double().abs()                     # the fp32 rounding itself went away from zero
    bits = f.view(torch.int32) - over.to(torch.int32)
    return (bits & ~0xFFFF).view(F32).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- forward
def gru_fwd(gi, w_hh, b_hh, dtype, round_operands=True, *, carried=None, round_h=bf16_rne):
    """gi [S,T,3d] (= x_t W_ih^T + b_ih), W_hh [3d,d], b_hh [3d] -> hseq [S,T,d], gates r|z|n [S,T,3d], hn = W_hn h + b_hn [S,T,d];
    h0 = 0.  `round_operands=False` is the plain GRU (torch.nn.GRU's equations): the fp32 kernel's reference.
    `carried` [S,T,d]: the state that enters each step (`entering(hseq)` of an implementation under test) instead of the replica's own."""
    gi, w, b = gi.to(dtype), w_hh.to(dtype), b_hh.to(dtype)
    S, T, d3 = gi.shape
    d = d3 // 3
    if round_operands:
        w = bf16_rne(w)
    h = torch.zeros((S, d), dtype=dtype)
    hs, gates, hns = [], [], []
    for t in range(T):
        if carried is not None:
            h = carried[:, t].to(dtype)
        hb = round_h(h) if round_operands else h                   # h itself is carried unrounded
        gh = hb @ w.t()
        r = torch.sigmoid(gi[:, t, :d] + gh[:, :d] + b[:d])
        z = torch.sigmoid(gi[:, t, d:2 * d] + gh[:, d:2 * d] + b[d:2 * d])
        hn = gh[:, 2 * d:] + b[2 * d:]
        n = torch.tanh(gi[:, t, 2 * d:] + r * hn)
        h = (1 - z) * n + z * h
        hs.append(h); gates.append(torch.cat([r, z, n], 1)); hns.append(hn)
    return torch.stack(hs, 1), torch.stack(gates, 1), torch.stack(hns, 1)


def entering(hseq):
    """The state that enters each step of a run that wrote `hseq`: h_0 = 0, then hseq[:, t - 1]."""
    return torch.cat([torch.zeros_like(hseq[:, :1]), hseq[:, :-1]], 1)


# ---------------------------------------------------------------------------------------------------------------- backward
def gru_bwd(dh, gates, hn, hseq, w_hh, dtype, round_operands=True, *, tiles=None, mutant=""):
    """gru_bwd_kernel step by step, t = T-1 .. 0 -> dgi [S,T,3d] (drp|dzp|dnp), dghn [S,T,d] (dgn), dgh16 = bf16(drp|dzp|dgn),
    dgi16 = bf16(dgi).  `tiles` [S,T,3d]: the gradient tile that goes into each step's carried product (the dgh16 of an implementation
    under test) instead of the replica's own.  `mutant` (tests only): "h0" reads h_{-1} as hseq[:, 0]; "dnp" carries dnp where dgn
    belongs; "trunc" cuts the gradient tile to bf16 instead of rounding it."""
    dh, gates, hn, hseq, w = (x.to(dtype) for x in (dh, gates, hn, hseq, w_hh))
    S, T, d = hseq.shape
    rnd = bf16_rne if round_operands else (lambda x: x)
    w = rnd(w)
    carry = torch.zeros((S, d), dtype=dtype)
    dgi, dghn, dgh16 = [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        r, z, n = gates[:, t, :d], gates[:, t, d:2 * d], gates[:, t, 2 * d:]
        hp = hseq[:, t - 1] if t > 0 else (hseq[:, 0] if mutant == "h0" else torch.zeros((S, d), dtype=dtype))
        dht = dh[:, t] + carry
        dn, dz = dht * (1 - z), dht * (hp - n)
        dnp, dzp = dn * (1 - n * n), dz * z * (1 - z)
        drp, dgn = dnp * hn[:, t] * r * (1 - r), dnp * r
        tile = (bf16_trunc if mutant == "trunc" else rnd)(torch.cat([drp, dzp, dgn], 1))
        sent = tile if tiles is None else tiles[:, t].to(dtype)
        if mutant == "dnp":
            sent = torch.cat([sent[:, :2 * d], rnd(dnp)], 1)
        carry = dht * z + sent @ w
        dgi[t], dghn[t], dgh16[t] = torch.cat([drp, dzp, dnp], 1), dgn, tile
    dgi = torch.stack(dgi, 1)
    return dgi, torch.stack(dghn, 1), torch.stack(dgh16, 1), rnd(dgi)


# ---------------------------------------------------------------------------------------------------------------- noise, bound
def noise(fn, *args, **kw):
    """Largest elementwise distance between fn(..., torch.float32) and fn(..., torch.float64), per output."""
    lo, hi = fn(*args, F32, **kw), fn(*args, F64, **kw)
    return tuple(float((a.double() - b).abs().max()) for a, b in zip(lo, hi))


def bound(noise_, ref, factor=FACTOR):
    """max(factor * noise, 16 fp32 ulps of max(1, max|ref|))"""
    return max(factor * noise_, FLOOR_ULPS * 2.0 ** -23 * max(1.0, float(ref.abs().max())))


def _judge(got, ref, nz):
    return ([float((g.double() - r).abs().max()) for g, r in zip(got, ref)], [bound(n, r) for n, r in zip(nz, ref)], list(nz))


def forward_distance(x, got, round_operands=True):
    """got = (hseq, gates, hn) of an implementation under test on inputs x -> (distance, bound, noise) per output, against the fp64
    replica that enters every step with the state `got` itself carried (round_operands=False: the plain GRU running free)."""
    kw = dict(carried=entering(got[0].float())) if round_operands else {}
    args = (x["gi"], x["w_hh"], x["b_hh"])
    return _judge(got, gru_fwd(*args, F64, round_operands, **kw), noise(gru_fwd, *args, round_operands=round_operands, **kw))


def backward_distance(args, got):
    """got = (dgi, dghn, dgh16) of an implementation under test on args = (dh, gates, hn, hseq, w_hh) -> (distance, bound, noise)
    for dgi and dghn, against the fp64 replica whose carried products use the tiles `got` itself wrote."""
    tiles = got[2].float()
    return _judge(got[:2], gru_bwd(*args, F64, tiles=tiles)[:2], noise(gru_bwd, *args, tiles=tiles)[:2])


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(S, T, gi_scale=1.0):
    """Seeded per (S, T): gi ~ randn (times gi_scale: the saturation cases), W_hh ~ 0.08 randn, b_hh ~ 0.1 randn, dh ~ randn; fp32."""
    g = torch.Generator().manual_seed(1000 * S + T)
    w_hh, b_hh = torch.randn(3 * D, D, generator=g) * 0.08, torch.randn(3 * D, generator=g) * 0.1
    gi, dh = torch.randn(S, T, 3 * D, generator=g) * gi_scale, torch.randn(S, T, D, generator=g)
    return dict(gi=gi, w_hh=w_hh, b_hh=b_hh, dh=dh)


@functools.lru_cache(maxsize=None)
def forward_free(S, T, gi_scale=1.0, round_operands=True):
    """The fp64 replica running free -> (hseq, gates, hn); computed once and shared, never modified."""
    x = inputs(S, T, gi_scale)
    return gru_fwd(x["gi"], x["w_hh"], x["b_hh"], F64, round_operands)


@functools.lru_cache(maxsize=None)
def backward_args(S, T, gi_scale=1.0):
    """The backward kernels' inputs (dh, gates, hn, hseq, w_hh), fp32: gates, hn and hseq are the REPLICA's fp64 forward cast to fp32,
    so that the backward kernels are tested apart from the forward kernels."""
    hseq, gates, hn = forward_free(S, T, gi_scale)
    x = inputs(S, T, gi_scale)
    return x["dh"], gates.float(), hn.float(), hseq.float(), x["w_hh"]
