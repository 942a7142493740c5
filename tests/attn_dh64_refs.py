"""Host references and input builders for the head-dim-64 attention kernels (csrc/attention_dh64.hip, csrc/attention_dh64_bwd.hip).
CPU torch only; tests/test_attn_dh64_refs_cpu.py shows that each one holds, tests/test_gpu_attn_dh64_paths.py compares the kernels with them.

Every operand here is [B, H, S, 64] float32 holding bf16-representable values (`dout` alone may be any fp32); `pack_qkv` / `rows` turn
them into the row-major [B * S, ...] buffers the C ABI takes.
  ref64          fp64 softmax attention with autograd: the truth.
  twin           the backward with the kernels' roundings (bf16 P, dS, dO, O; fp32 elsewhere), in plain fp32 torch.  It is a reference,
                 written from the formulas and not fitted to the kernels: its distance from ref64 is what bf16 operands cost, and the
                 yardstick the kernels' own distance from ref64 is held against.
  trace_blocks   the order in which the general forward kernels meet the keys, walked in fp64: which blocks move the running maximum.
  one_hot_inputs / peaked_inputs / forcing_inputs / uniform_inputs: the cases."""
from __future__ import annotations

import collections
import math

import torch

LOG2E = 1.4426950408889634
DH = 64
# restated from the kernels, so that the tracer does not depend on the library:
KC = 320              # csrc/attention_dh64_tile.h `KC`: keys per LDS chunk, chunks start at key 0
KB = 64               # keys per block of key_block(); a chunk's last block is masked when it holds fewer
QT = 16               # queries per subtile: one running-maximum decision (`moved`) per subtile and block
DEFER_LOG2 = 5.0      # csrc/attention_dh64.hip `DEFER_LOG2`: the 8-wave and S = 257 kernels move the maximum only past this (exp2 units)
GAP_NATS = 40.0       # one_hot_inputs: the hot score leads its row by at least this, so every other weight is < e^-40 < 2^-57
NONHOT = 2.0 ** -57


def bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def rows(x: torch.Tensor) -> torch.Tensor:
    """[B, H, S, 64] -> [B * S, H * 64], the kernels' row layout"""
    B, H, S, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * d).contiguous()


def unrows(x2: torch.Tensor, B: int, S: int, H: int) -> torch.Tensor:
    """[B * S, H * 64] -> [B, H, S, 64]"""
    return x2.reshape(B, S, H, DH).permute(0, 2, 1, 3).contiguous()


def pack_qkv(q, k, v) -> torch.Tensor:
    """-> [B * S, 3 * H * 64] (q | k | v column blocks)"""
    return torch.cat([rows(q), rows(k), rows(v)], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ references
def ref64(q, k, v, dout, scale):
    """fp64 softmax(q k^T scale) v on the given operands -> dict o, lse2 (logsumexp * log2 e, [B, H, S]), dq, dk, dv (autograd)."""
    q, k, v = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    sc = q @ k.transpose(-1, -2) * scale
    o = torch.softmax(sc, dim=-1) @ v
    o.backward(dout.double())
    return {"o": o.detach(), "lse2": (torch.logsumexp(sc, dim=-1) * LOG2E).detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def twin(q, k, v, dout, scale):
    """Forward and backward as the kernels round them, fp32 torch -> dict o, lse2, dq, dk, dv, dob, dsum.
    D is formed from bf16(dout), the operand dP is formed from: then dS = P o (dP - D) has row sums that vanish up to rounding."""
    q, k, v, dout = [t.float() for t in (q, k, v, dout)]
    c = float(scale) * LOG2E
    s = q @ k.transpose(-1, -2)
    m = s.amax(dim=-1, keepdim=True)
    pt = torch.exp2((s - m) * c)
    l = pt.sum(dim=-1, keepdim=True)
    o = bf16((bf16(pt) @ v) / l)
    L = m * c + torch.log2(l)
    p = torch.exp2(s * c - L)
    dob = bf16(dout)
    dp = dob @ v.transpose(-1, -2)
    dsum = (dob * o).sum(dim=-1, keepdim=True)
    ds = bf16(p * (dp - dsum) * float(scale))
    return {"o": o, "lse2": L.squeeze(-1), "dq": ds @ k, "dk": ds.transpose(-1, -2) @ q, "dv": bf16(p).transpose(-1, -2) @ dob,
            "dob": dob, "dsum": dsum.squeeze(-1)}


# ------------------------------------------------------------------------------------------------------------------ the block walk
Trace = collections.namedtuple("Trace", "later_moves deferred chunk_moves tail_moves later_blocks")


def trace_blocks(q, k, S, defer, scale=0.125) -> Trace:
    """The general forward kernels' walk over the keys, in fp64, per (b, h) and 16-query subtile: chunks of KC keys from key 0, KB-key
    blocks inside a chunk, the chunk's last block masked when it holds fewer than KB keys.  Per block
        moved = any query of the subtile has (block maximum - m_run) * scale * log2 e > DEFER_LOG2       (defer; else always True)
    and m_run = max(m_run, block maximum) only when moved.  Counted over every (b, h, subtile, block) but a subtile's first block:
      later_moves  moved, and some query's m_run rose (the alpha rescale of O and l_run did real work)
      deferred     not moved although some query's block maximum exceeds its m_run (growth carried in P instead)
      chunk_moves  the later_moves inside a chunk >= 1
      tail_moves   the later_moves inside a masked block
      later_blocks how many blocks were looked at"""
    assert q.shape[2] == S and k.shape[2] == S
    B, H = q.shape[:2]
    c = float(scale) * LOG2E
    nt = (S + QT - 1) // QT
    cnt = dict.fromkeys(Trace._fields, 0)
    for b in range(B):
        for h in range(H):
            s = q[b, h].double() @ k[b, h].double().T                      # [query, key]
            if nt * QT > S:                                                # a ragged last subtile: its absent queries decide nothing
                s = torch.cat([s, s[-1:].expand(nt * QT - S, S)], dim=0)
            m_run = torch.full((nt, QT), -math.inf, dtype=torch.float64)
            first = True
            for c0 in range(0, S, KC):
                nkeys = min(KC, S - c0)
                for k0 in range(c0, c0 + nkeys, KB):
                    k1 = min(k0 + KB, c0 + nkeys)
                    mx = s[:, k0:k1].amax(dim=1).view(nt, QT)
                    if first:                                              # m_run = -inf: every subtile moves, nothing to rescale
                        m_run, first = mx, False
                        continue
                    grew = (mx > m_run).any(dim=1)
                    moved = ((mx - m_run) * c > DEFER_LOG2).any(dim=1) if defer else torch.ones(nt, dtype=torch.bool)
                    real = moved & grew
                    cnt["later_blocks"] += nt
                    cnt["later_moves"] += int(real.sum())
                    cnt["deferred"] += int((grew & ~moved).sum())
                    if c0 > 0:
                        cnt["chunk_moves"] += int(real.sum())
                    if k1 - k0 < KB:
                        cnt["tail_moves"] += int(real.sum())
                    m_run = torch.where(moved.view(nt, 1), torch.maximum(m_run, mx), m_run)
    return Trace(**cnt)


# ------------------------------------------------------------------------------------------------------------------ inputs
def uniform_inputs(B, S, H, seed, std=0.7):
    """bf16(std * randn) q, k, v: score standard deviation about 8 std^2 / 8, a nearly uniform softmax"""
    g = _gen(seed)
    return tuple(bf16(torch.randn(B, H, S, DH, generator=g) * std) for _ in range(3))


def _pi(B, S, H, kind, g):
    if kind == "perm":
        return torch.stack([torch.stack([torch.randperm(S, generator=g) for _ in range(H)]) for _ in range(B)])
    one = {"reverse": torch.arange(S - 1, -1, -1), "last": torch.full((S,), S - 1), "first": torch.zeros(S, dtype=torch.long)}[kind]
    return one.view(1, 1, S).expand(B, H, S).contiguous()


def one_hot_inputs(B, S, H, kind, seed, scale=0.125):
    """A softmax that is one-hot to far below fp32: k_j = c_j, q_i = 16 c_{pi(i)} with random codes c_j in {+-1}^64 per (b, h), v =
    bf16(randn).  The hot raw score is 1024 for every query (times scale log2 e it is exact in fp32 and the same in every row), another
    key's is 16 <c_pi(i), c_j>.  -> q, k, v, pi ([B, H, S], int64).  Asserts the lead of the hot score: >= GAP_NATS over every key whose
    code differs (a key with the very code of the hot one would share its weight; the assertion refuses that as well)."""
    g = _gen(seed)
    code = (torch.randint(0, 2, (B, H, S, DH), generator=g) * 2 - 1).float()
    pi = _pi(B, S, H, kind, g)
    k = code
    q = 16.0 * torch.gather(code, 2, pi.unsqueeze(-1).expand(B, H, S, DH))
    v = bf16(torch.randn(B, H, S, DH, generator=g))
    sc = (q @ k.transpose(-1, -2)) * scale                                   # exact: integers times a power of two
    hot = torch.gather(sc, 3, pi.unsqueeze(-1))
    assert bool((hot == 16.0 * DH * scale).all())
    rest = sc.scatter(3, pi.unsqueeze(-1), -math.inf)
    gap = float((hot - rest.amax(dim=-1, keepdim=True)).min()) if S > 1 else math.inf
    assert gap >= GAP_NATS, f"one_hot_inputs(S={S}, {kind}, seed={seed}): the hot score leads by {gap} nats only"
    return q, k, v, pi


def peaked_inputs(B, S, H, factor, seed):
    """k = bf16(randn), q_i = bf16(factor k_{pi(i)}) for a random permutation pi, v = bf16(0.7 randn): query i has a dominant key
    (factor |k|^2 / 8 ~ 8 factor nats against a spread of about factor nats) without being one-hot.  -> q, k, v, pi"""
    g = _gen(seed)
    k = bf16(torch.randn(B, H, S, DH, generator=g))
    pi = _pi(B, S, H, "perm", g)
    q = bf16(factor * torch.gather(k, 2, pi.unsqueeze(-1).expand(B, H, S, DH)))
    v = bf16(0.7 * torch.randn(B, H, S, DH, generator=g))
    return q, k, v, pi


def late_keys(S):
    """the keys the `late_key` case makes dominant: one in the last full block of the last chunk (of the chunk before, where the last
    chunk has no full block), key KC (the first key of chunk 1) and key S - 1 (in the masked tail block where S % 64 != 0)"""
    c_last = (S - 1) // KC * KC
    nfull = (S - c_last) // KB
    j_full = c_last + (nfull - 1) * KB + 37 if nfull > 0 else c_last - KB + 37
    return [j for j in dict.fromkeys([j_full, KC, S - 1]) if 0 <= j < S]


def forcing_inputs(B, S, H, case, seed):
    """The data-dependent paths of the online softmax, forced (after test_attn_dh64_s257_rescale_paths):
      late_key  on a bf16(0.5 randn) base, k_j = bf16(30 q_i) for the keys j of late_keys(S), each for a query i of its own per (b, h):
                a score of about 30 |q_i|^2 / 8 ~ 60 nats arrives after the running maximum has settled
      ramp      on a bf16(randn) base, K rows times linspace(0.2, 3.0, S): block maxima that keep growing, below and above the defer
                threshold.  (On the 0.5 randn base the scores spread by 0.25 nats times the ramp and no block maximum ever leads the running
                one by DEFER_LOG2 = 3.5 nats: the walk shows 0 later moves at S = 512, 577 and 1370.  On randn it shows 380 and 1424
                deferred growths at S = 1370.)
    -> q, k, v"""
    q, k, v = uniform_inputs(B, S, H, seed, std=1.0 if case == "ramp" else 0.5)
    if case == "late_key":
        js = late_keys(S)
        for b in range(B):
            for h in range(H):
                for n, j in enumerate(js):
                    i = (7 + 37 * (b * H + h) + (S // 3) * n) % S            # spread over subtiles, another set per (b, h)
                    k[b, h, j] = bf16(30.0 * q[b, h, i])
    elif case == "ramp":
        k = bf16(k * torch.linspace(0.2, 3.0, S).view(1, 1, S, 1))
    else:
        raise ValueError(case)
    return q, k, v


# ------------------------------------------------------------------------------------------------------------------ one-hot bounds
def one_hot_expect(q, k, v, pi, dout, scale):
    """What a one-hot softmax leaves of the backward, and how far a kernel that forms dP and D from the same bf16(dout) may be from it.
    With dOb = bf16(dout) and A[i, d] = |dOb[i, d] v[pi(i), d]|:
      o = v[pi]; lse2 = hot score * scale * log2 e; dV[j] = sum of dOb[i] over pi(i) = j, an fp32 sum of n_j terms (P = 1 exactly);
      dQ = dK = 0 in exact arithmetic; the hot dS is P (dP - D) scale where dP and D are the SAME 64-term dot product summed in two fp32
      orders, each within 64 * 2^-24 * sum_d A of it, so per element
          |dQ[i]| <= bound_q[i] = 2 * 64 * 2^-24 * sum_d A[i, d] * scale * max|k|
          |dK[j]| <= sum over pi(i) = j of 2 * 64 * 2^-24 * sum_d A[i, d] * scale * max|q|
          |dV[j, d] - want| <= n_j 2^-23 * sum over pi(i) = j of |dOb[i, d]|
    The weights off the hot key are below NONHOT = 2^-57 but not zero (2^-57 is an ordinary bf16 number), and for a key no query points at
    the bounds above are exactly 0.  `floor_k` / `floor_v` are what those weights can add at most, per element:
          floor_v[d] = NONHOT * sum_i |dOb[i, d]|        floor_k = NONHOT * scale * max|q| * sum_i 2 * max|v| * sum_d |dOb[i, d]|
    (|dP - D| <= 2 max|v| sum_d |dOb|).  Both are some 2^-30 of a typical gradient element."""
    B, H, S, _ = q.shape
    dob = bf16(dout.float()).double()
    idx = pi.unsqueeze(-1).expand(B, H, S, DH)
    vhot = torch.gather(v.double(), 2, idx)
    a_row = (dob * vhot).abs().sum(dim=-1)                                   # [B, H, S]
    per_q = 2 * 64 * 2.0 ** -24 * a_row * scale
    n = torch.zeros(B, H, S, dtype=torch.float64).scatter_add(2, pi, torch.ones(B, H, S, dtype=torch.float64))
    dv = torch.zeros(B, H, S, DH, dtype=torch.float64).scatter_add(2, idx, dob)
    dv_abs = torch.zeros(B, H, S, DH, dtype=torch.float64).scatter_add(2, idx, dob.abs())
    qmax, kmax, vmax = float(q.abs().max()), float(k.abs().max()), float(v.abs().max())
    bound_k = torch.zeros(B, H, S, dtype=torch.float64).scatter_add(2, pi, per_q * qmax)
    floor_k = NONHOT * scale * qmax * 2 * vmax * dob.abs().sum(dim=(-1, -2))            # [B, H]
    floor_v = NONHOT * dob.abs().sum(dim=2, keepdim=True)                                # [B, H, 1, 64]
    return {"o": vhot.float(), "lse2": torch.full((B, H, S), 16.0 * DH * scale * LOG2E, dtype=torch.float64),
            "dv": dv, "tol_v": n.unsqueeze(-1) * 2.0 ** -23 * dv_abs + floor_v,
            "bound_q": (per_q * kmax).unsqueeze(-1), "bound_k": (bound_k + floor_k.view(B, H, 1)).unsqueeze(-1)}
