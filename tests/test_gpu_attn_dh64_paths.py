"""Head-dim-64 attention (csrc/attention_dh64.hip, csrc/attention_dh64_bwd.hip) where randn inputs never take it: every rescale path of
the general forward kernels, and the backward under a peaked softmax.  References and input builders: tests/attn_dh64_refs.py (shown to
hold by tests/test_attn_dh64_refs_cpu.py).  The shapes alone select the kernels (tests/test_attn_dh64_plan_cpu.py pins which).

  forward rescale paths   On randn the 8-wave kernel (S >= 512, deferred rescale) never moves a running maximum after a subtile's first
                          key block, so its alpha multiply of O and l_run ran in no test.  `late_key` and `ramp` inputs force moves in
                          later chunks and in the masked tail block, and deferred growth; each case first shows, from a host walk of the
                          kernel's block order, that it does.  O and lse against fp64.
  one-hot softmax         q_i = 16 c_pi(i), k_j = c_j on +-1 codes: every weight off key pi(i) is below 2^-57.  O must be v[pi] bit for
                          bit, dV the scatter-add of bf16(dO), and dQ, dK (exactly 0 in exact arithmetic) at most the fp32 reordering
                          error of ONE 64-term dot product: all that separates dP = <dOb, v> from D = <dOb, O> when both are formed from
                          the same bf16(dO).  With D formed from the fp32 dO, as the prep kernel did, dQ and dK carried noise of order
                          2^-9 |dO| |v| scale |q|, growing with the sharpness of the softmax.
  backward against twin   e(x) = x - fp64 truth; the kernel's error may be at most 3 x the error of the host twin, which rounds what the
                          kernels round (bf16 P, dS, dO, O) and is fp32 elsewhere, in Frobenius norm and in the largest element.  Kernel
                          and twin differ in fp32 summation order, hardware exp2, the forward's choice of running maximum, and ties.
                          Measured kernel / twin ratios: Frobenius 0.998-1.003 and max 0.958-1.074 on uniform inputs, 1.000 and 1.000
                          on peaked ones (17.6 and 5.4 before D was formed from bf16(dO)); per case under
                          `test_backward_error_against_the_twins`.
  prep and strides        medp_attn_bwd_dh64_prep alone, and the forward / prep / backward with every row stride wider than its rows,
                          inside NaN padding."""
import pytest
import torch

import attn_dh64_refs as R

pytestmark = pytest.mark.gpu

SCALE = 0.125
DEV = "cuda"
PAD = 4096          # NaN elements before and behind every buffer (a multiple of 8: the views stay 16-byte aligned)


def _fn():
    from multimodal_edema_prediction_amd import functional as Fn
    return Fn


def assert_close(got, want, rtol, atol, what):
    err = (got.detach().cpu().double() - want.double()).abs()
    tol = atol + rtol * want.double().abs()
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e}"


def gpu_forward(q, k, v):
    """-> o [B, H, S, 64] fp32 on the host, lse [B, H, S] on the host, and the device tensors the backward consumes"""
    B, H, S, _ = q.shape
    qkv = R.pack_qkv(q, k, v).to(DEV).bfloat16()
    o, lse = _fn().attn_dh64_lse(qkv, B, S, H, SCALE)
    return R.unrows(o.float().cpu(), B, S, H), lse.cpu(), (qkv, o, lse)


def gpu_backward(dout, state, B, S, H):
    qkv, o, lse = state
    D = H * 64
    dqkv = _fn().attn_dh64_bwd(R.rows(dout).to(DEV), qkv, o, lse, B, S, H, SCALE).cpu()
    return [R.unrows(dqkv[:, i * D:(i + 1) * D], B, S, H) for i in range(3)]


# ------------------------------------------------------------------------------------------------ C.1 forward rescale paths
@pytest.mark.parametrize("case", ["late_key", "ramp"])
@pytest.mark.parametrize("B,S,H", [(1, 321, 2), (2, 400, 2), (1, 512, 1), (2, 577, 2), (1, 1370, 1)])
def test_forward_rescale_paths_of_the_general_kernels(B, S, H, case):
    """4-wave kernel (S < 512: the maximum moves with every growth) and 8-wave kernel (deferred), two and more key chunks."""
    defer = S >= 512
    q, k, v = R.forcing_inputs(B, S, H, case, seed=S)
    t = R.trace_blocks(q, k, S, defer, SCALE)
    print(f"{case} S={S}: {t}")
    assert t.later_moves > 0
    if case == "late_key":
        assert t.chunk_moves > 0, "no move of the running maximum inside a chunk >= 1"
        assert S % 64 == 0 or t.tail_moves > 0, "no move inside the masked tail block"
    if defer and case == "ramp":
        assert t.deferred > 0, "no growth below the defer threshold"
    ref = R.ref64(q, k, v, torch.zeros_like(q), SCALE)
    o, lse, _ = gpu_forward(q, k, v)
    assert_close(o, ref["o"], 1e-2, 1e-2, f"O {case} S={S}")
    o2 = _fn().attn_dh64(R.pack_qkv(q, k, v).to(DEV).bfloat16(), B, S, H, SCALE)
    assert_close(R.unrows(o2.float().cpu(), B, S, H), ref["o"], 1e-2, 1e-2, f"O (no lse) {case} S={S}")
    assert_close(lse, ref["lse2"], 1e-4, 2e-3, f"lse {case} S={S}")


# ------------------------------------------------------------------------------------------------ C.2 one-hot softmax
@pytest.mark.parametrize("kind", ["perm", "reverse", "last", "first"])
@pytest.mark.parametrize("S", [1, 16, 17, 33, 192, 257, 320, 321, 512, 577, 1370])
def test_one_hot_softmax_exact_index_maps(S, kind):
    """Bounds: attn_dh64_refs.one_hot_expect.  For a key that no query points at, the rounding bounds of dK and dV are exactly 0; there
    they carry the floor that the weights below 2^-57 can add (ordinary bf16 numbers, not zeros)."""
    B = H = 2 if S <= 577 else 1
    q, k, v, pi = R.one_hot_inputs(B, S, H, kind, seed=1000 + S)
    dout = torch.randn(B, H, S, 64, generator=torch.Generator().manual_seed(S))
    ex = R.one_hot_expect(q, k, v, pi, dout, SCALE)
    o, lse, state = gpu_forward(q, k, v)
    dq, dk, dv = gpu_backward(dout, state, B, S, H)
    rq = float((dq.abs().double() / ex["bound_q"]).max())
    rk = float((dk.abs().double() / ex["bound_k"]).max())
    ev = (dv.double() - ex["dv"]).abs()
    print(f"one-hot S={S} {kind}: max|dQ| {float(dq.abs().max()):.3e} = {rq:.3e} of its bound, max|dK| {float(dk.abs().max()):.3e} = "
          f"{rk:.3e} of its bound, max dV error {float(ev.max()):.3e}, O exact {torch.equal(o, ex['o'])}")
    assert torch.equal(o, ex["o"]), f"O != v[pi] in {int((o != ex['o']).sum())} elements"
    assert_close(lse, ex["lse2"], 1e-4, 2e-3, "lse")
    assert bool((ev <= ex["tol_v"]).all()), f"dV: {int((ev > ex['tol_v']).sum())} elements outside n_j 2^-23"
    assert rq <= 1.0, f"dQ is {rq:.1f} x the fp32 reordering bound"
    assert rk <= 1.0, f"dK is {rk:.1f} x the fp32 reordering bound"


# ------------------------------------------------------------------------------------------------ C.3 backward against the twin
BWD_CASES = [("uniform", 2, 33, 2), ("uniform", 1, 320, 1), ("uniform", 2, 321, 2), ("uniform", 1, 640, 1), ("uniform", 1, 641, 2),
             ("peaked3", 1, 257, 2), ("peaked3", 2, 400, 2)]


@pytest.mark.parametrize("inputs,B,S,H", BWD_CASES)
def test_backward_error_against_the_twins(inputs, B, S, H):
    """uniform: bf16(0.7 randn) operands; peaked3: peaked_inputs(factor 3).  dout is fp32 randn, not bf16-rounded.  Per tensor
        |e(kernel)|_F <= 3 |e(twin)|_F + 1e-6    and    max|e(kernel)| <= 3 max|e(twin)| + 1e-6.
    Measured on the MI355X, kernel / twin error as Frobenius ratio and max ratio, the extremes over dq, dk, dv:
        uniform  (2, 33, 2) 1.000, 1.000   (1, 320, 1) 0.999-1.003, 0.964-1.019   (2, 321, 2) 1.000-1.002, 0.987-1.000
                 (1, 640, 1) 0.998-1.001, 0.958-1.074   (1, 641, 2) 1.000-1.001, 1.000-1.060
        peaked3  (1, 257, 2) 1.000, 1.000   (2, 400, 2) 1.000, 1.000
    With D formed from the fp32 dout (the prep kernel before it was changed) peaked3 gave 17.6, 5.4 at S = 257 and 8.4, 1.9 at S = 400
    on dq and dk (dv 1.000; uniform 0.992-1.010, 0.937-1.087).  The yardstick itself is coarse where the softmax is peaked: the twin's
    own error is 0.28 (S = 257) and 0.65 (S = 400) of |dq|_F there, against 2.4e-3 on uniform inputs: bf16 dS against gradients that
    nearly cancel."""
    if inputs == "uniform":
        q, k, v = R.uniform_inputs(B, S, H, seed=100 + S)
    else:
        q, k, v, _ = R.peaked_inputs(B, S, H, 3.0, seed=100 + S)
    dout = torch.randn(B, H, S, 64, generator=torch.Generator().manual_seed(200 + S))
    ref, tw = R.ref64(q, k, v, dout, SCALE), R.twin(q, k, v, dout, SCALE)
    o, lse, state = gpu_forward(q, k, v)
    got = dict(zip(("dq", "dk", "dv"), gpu_backward(dout, state, B, S, H)))
    assert_close(o, ref["o"], 1e-2, 1e-2, "O")
    assert_close(lse, ref["lse2"], 1e-4, 2e-3, "lse")
    bad = []
    for name in ("dq", "dk", "dv"):
        ek, et = got[name].double() - ref[name], tw[name].double() - ref[name]
        fro, mx = float(ek.norm() / et.norm()), float(ek.abs().max() / et.abs().max())
        print(f"{inputs} B={B} S={S} H={H} {name}: kernel / twin error  Frobenius {fro:.3f}  max {mx:.3f}   "
              f"(twin: {float(et.norm() / ref[name].norm()):.3e} of |{name}|_F)")
        assert torch.isfinite(got[name]).all()
        if float(ek.norm()) > 3 * float(et.norm()) + 1e-6 or float(ek.abs().max()) > 3 * float(et.abs().max()) + 1e-6:
            bad.append((name, round(fro, 2), round(mx, 2)))
    assert not bad, f"(tensor, Frobenius ratio, max ratio) above 3: {bad}"


# ------------------------------------------------------------------------------------------------ C.4 prep alone, and strides
def _poisoned(nrows, cols, ld, dtype, fill=None):
    """[nrows, cols] view with row stride ld inside a NaN buffer; `fill`: values for the view (default: left NaN)"""
    buf = torch.full((2 * PAD + nrows * ld,), float("nan"), device=DEV, dtype=dtype)
    view = buf[PAD:PAD + nrows * ld].view(nrows, ld)[:, :cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _surroundings_intact(buf, nrows, cols, ld):
    body = buf[PAD:PAD + nrows * ld].view(nrows, ld)
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + nrows * ld:]).all() and torch.isnan(body[:, cols:]).all())


@pytest.mark.parametrize("B,S,H", [(1, 1, 1), (2, 5, 3), (3, 17, 2)])
def test_prep_kernel_alone(B, S, H):
    """dob = bf16(dout) and dsum = sum_d bf16(dout) o: the D of the backward, from the operand dP is made of.  16 lanes per (row, head);
    B S H = 1 / 30 / 102 units end inside a 16-unit workgroup.  fp32 sum of 64 products in a tree: within 64 * 2^-23 of sum |terms|."""
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    D, M = H * 64, B * S
    g = torch.Generator().manual_seed(S)
    dout, o = torch.randn(M, D, generator=g), R.bf16(torch.randn(M, D, generator=g))
    lddout, ldo, lddob = D + 4, D + 8, D + 8
    dbuf, d_v = _poisoned(M, D, lddout, torch.float32, dout)
    obuf, o_v = _poisoned(M, D, ldo, torch.bfloat16, o)
    bbuf, b_v = _poisoned(M, D, lddob, torch.bfloat16)
    sbuf, s_v = _poisoned(1, B * H * S, B * H * S, torch.float32)
    check(lib().medp_attn_bwd_dh64_prep(ptr(d_v), lddout, ptr(o_v), ldo, ptr(b_v), lddob, ptr(s_v), B, S, H, stream()), "prep")
    torch.cuda.synchronize()
    assert _surroundings_intact(bbuf, M, D, lddob) and _surroundings_intact(sbuf, 1, B * H * S, B * H * S), "a store outside dob / dsum"
    assert _surroundings_intact(dbuf, M, D, lddout) and _surroundings_intact(obuf, M, D, ldo)
    assert torch.equal(b_v.cpu(), dout.bfloat16())
    terms = (R.bf16(dout).double() * o.double()).view(B, S, H, 64)
    want, mag = terms.sum(-1).permute(0, 2, 1), terms.abs().sum(-1).permute(0, 2, 1)          # [B, H, S]
    err = (s_v.cpu().view(B, H, S).double() - want).abs()
    print(f"prep B={B} S={S} H={H}: max |dsum - sum bf16(dout) o| / sum|terms| = {float((err / mag).max()):.3e} (bound {64 * 2.0 ** -23:.3e})")
    assert bool((err <= 64 * 2.0 ** -23 * mag).all())


def test_wide_row_strides_give_the_packed_bits():
    """Forward with lse, prep and backward on separate q, k, v, o, dO, dq, dk, dv buffers whose rows are wider than their live columns,
    all inside NaN: every live element has the bits of the packed call through `functional`, nothing else is written."""
    from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream
    B, S, H = 2, 33, 2
    D, M = H * 64, B * S
    q, k, v = R.uniform_inputs(B, S, H, seed=33)
    dout = R.rows(torch.randn(B, H, S, 64, generator=torch.Generator().manual_seed(34)))
    Fn = _fn()
    qkv = R.pack_qkv(q, k, v).to(DEV).bfloat16()
    o_p, lse_p = Fn.attn_dh64_lse(qkv, B, S, H, SCALE)
    dqkv_p = Fn.attn_dh64_bwd(dout.to(DEV), qkv, o_p, lse_p, B, S, H, SCALE)

    ldqkv, lddo, ldd, ldo, lddout = 3 * D + 8, D + 8, 3 * D + 4, D + 4, D + 4
    ins = [_poisoned(M, D, ldqkv, torch.bfloat16, R.rows(t)) for t in (q, k, v)]
    obuf, o_v = _poisoned(M, D, ldo, torch.bfloat16)
    lbuf, l_v = _poisoned(1, B * H * S, B * H * S, torch.float32)
    check(lib().medp_attn_fwd_dh64_lse(ptr(ins[0][1]), ptr(ins[1][1]), ptr(ins[2][1]), ptr(o_v), ptr(l_v), B, S, H, ldqkv, ldqkv, ldqkv,
                                       ldo, SCALE, stream()), "fwd")
    _, d_v = _poisoned(M, D, lddout, torch.float32, dout)
    bbuf, b_v = _poisoned(M, D, lddo, torch.bfloat16)
    sbuf, s_v = _poisoned(1, B * H * S, B * H * S, torch.float32)
    check(lib().medp_attn_bwd_dh64_prep(ptr(d_v), lddout, ptr(o_v), ldo, ptr(b_v), lddo, ptr(s_v), B, S, H, stream()), "prep")
    outs = [_poisoned(M, D, ldd, torch.float32) for _ in range(3)]
    check(lib().medp_attn_bwd_dh64(ptr(ins[0][1]), ptr(ins[1][1]), ptr(ins[2][1]), ldqkv, ptr(b_v), lddo, ptr(l_v), ptr(s_v),
                                   ptr(outs[0][1]), ptr(outs[1][1]), ptr(outs[2][1]), ldd, B, S, H, SCALE, stream()), "bwd")
    torch.cuda.synchronize()
    assert _surroundings_intact(obuf, M, D, ldo) and _surroundings_intact(lbuf, 1, B * H * S, B * H * S), "forward stored outside o / lse"
    assert _surroundings_intact(bbuf, M, D, lddo) and _surroundings_intact(sbuf, 1, B * H * S, B * H * S), "prep stored outside dob / dsum"
    for (buf, _), name in zip(outs, ("dq", "dk", "dv")):
        assert _surroundings_intact(buf, M, D, ldd), f"backward stored outside {name}"
    for (buf, _) in ins:
        assert _surroundings_intact(buf, M, D, ldqkv)
    assert torch.equal(o_v.contiguous().view(torch.int16).cpu(), o_p.view(torch.int16).cpu()), "o"
    assert torch.equal(l_v.view(torch.int32).cpu().view(-1), lse_p.view(torch.int32).cpu().view(-1)), "lse"
    for i, ((_, view), name) in enumerate(zip(outs, ("dq", "dk", "dv"))):
        assert torch.isfinite(view).all(), name
        assert torch.equal(view.contiguous().view(torch.int32).cpu(), dqkv_p[:, i * D:(i + 1) * D].contiguous().view(torch.int32).cpu()), name
