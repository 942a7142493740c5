"""The kernels of csrc/elementwise.hip on their own — the ViT front end (`medp_im2col_patch`, `medp_vit_assemble`,
`medp_pos_embed_bicubic`, `medp_pos_embed_bicubic_bwd`), the bf16 GELU pair, the strided forms of `medp_cast_f32_bf16` /
`medp_transpose_to_bf16` and `medp_weight_operands_multi` — through the C ABI, against tests/vit_front_refs.py in float64 (or, where
the only arithmetic is one rounding, bit for bit against torch).  Every output buffer starts as NaN with a payload of its own, so a
cell the kernel skipped, a gap column it wrote and a guard row past the end all show.

Bounds: the bicubic resize and its backward within 3e-5 of max|reference| (vit_front_refs.BICUBIC_TOL: about 5x the error of an
fp32 replica of the kernel's arithmetic); GELU within one bf16 ulp plus the 1e-6 absolute that the erf formula (A&S 7.1.26) and fp32
rounding are allowed, at every one of the 65 536 bf16 inputs.

Worst observed error / bound on an MI355X (each test prints its own):
  bicubic forward   0.150  (37 -> 48x48: 1.6e-5 on max|ref| 3.6, i.e. 4.5e-6 relative)
  bicubic backward  0.136  (37 <- 48x48)
  adjoint identity  0.069  (5 -> 3x9: 6.9e-7 of the inner product)
  gelu forward      0.484  (x = -0.0327; no input above half of the bound, i.e. above half an ulp)
  gelu backward     0.497  (dy = 1, x = 0.00244), 0.488 (seeded dy); none above half of the bound
Everything else here is compared bit for bit."""
import ctypes

import pytest
import torch

import vit_front_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN16, NAN32 = 0x7FC1, 0x7FC00001                                   # quiet NaNs with a payload no arithmetic produces


def _abi():
    from multimodal_edema_prediction_amd import abi
    return abi


def nan16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(BF16)


def nan32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=DEV).view(F32)


def untouched(t):
    if t.numel() == 0:
        return True
    return bool((t.view(torch.int16) == NAN16).all()) if t.dtype == BF16 else bool((t.view(torch.int32) == NAN32).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def call(name, *args):
    """One C ABI call on the current stream, errors as exceptions, finished before it returns."""
    abi = _abi()
    abi.check(getattr(abi.lib(), name)(*(abi.ptr(a) if isinstance(a, torch.Tensor) else a for a in args), abi.stream()), name)
    torch.cuda.synchronize()


def within(got, ref, tol, what):
    """max|got - ref| <= tol * max|ref|, the observed ratio printed"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max err {err:.3e} of max|ref| {scale:.3e}: {err / (tol * scale):.3f} of the bound")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and err <= tol * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------ medp_im2col_patch
# non-square with K = 588 padded by 4 | remainder rows and columns ignored | K == kpad, C = 1 | a whole 8-column group of zeros | small
@pytest.mark.parametrize("B,C,H,W,patch,kpad", [(2, 3, 28, 42, 14, 592), (1, 3, 37, 30, 14, 592), (3, 1, 16, 24, 8, 64),
                                                (1, 3, 14, 14, 14, 600), (2, 2, 12, 20, 4, 32)])
def test_im2col_patch(B, C, H, W, patch, kpad):
    g = torch.Generator().manual_seed(H * 100 + W)
    pix = torch.randn(B, C, H, W, generator=g)
    rows, K = B * (H // patch) * (W // patch), C * patch * patch
    A = nan16(rows + 1, kpad)
    call("medp_im2col_patch", pix.to(DEV), A, B, C, H, W, patch, kpad)
    want = R.im2col(pix, patch, kpad).bfloat16()                    # the only arithmetic is the rounding
    assert torch.equal(A[:rows].cpu(), want) and torch.equal(bits(A[:rows]), bits(want))
    assert bool((bits(A[:rows, K:]) == 0).all())                    # pad columns: +0.0, never the sentinel
    assert untouched(A[rows:])


def test_im2col_patch_refuses():
    pix, A = torch.zeros(1, 3, 28, 28, device=DEV), nan16(8, 600)
    for B, C, H, W, patch, kpad in [(1, 3, 13, 28, 14, 592), (1, 3, 28, 13, 14, 592), (1, 3, 28, 28, 14, 590), (1, 3, 28, 28, 14, 584),
                                    (1, 1, 28, 28, 14, 192)]:      # H < patch, W < patch, kpad % 8, kpad < C p^2 (twice)
        with pytest.raises(ValueError):
            call("medp_im2col_patch", pix, A, B, C, H, W, patch, kpad)
    assert untouched(A)


# ------------------------------------------------------------------------------------------------ medp_vit_assemble
@pytest.mark.parametrize("B,P,D", [(1, 1, 4), (3, 6, 128), (2, 17, 132), (2, 256, 768)])
def test_vit_assemble(B, P, D):
    g = torch.Generator().manual_seed(P * 10 + D)
    patch, cls, pos = torch.randn(B * P, D, generator=g), torch.randn(D, generator=g), torch.randn(P + 1, D, generator=g)
    x = nan32(B * (P + 1) + 1, D)
    call("medp_vit_assemble", patch.to(DEV), cls.to(DEV), pos.to(DEV), x, B, P, D)
    want = torch.cat((cls.expand(B, 1, D), patch.view(B, P, D)), dim=1) + pos      # one correctly rounded add per element
    assert torch.equal(x[:-1].cpu().view(B, P + 1, D), want)
    assert untouched(x[-1:])


def test_vit_assemble_refuses_a_width_that_is_no_multiple_of_4():
    x = nan32(2 * 3, 6)
    with pytest.raises(ValueError):
        call("medp_vit_assemble", torch.zeros(4, 6, device=DEV), torch.zeros(6, device=DEV), torch.zeros(3, 6, device=DEV), x, 2, 2, 6)
    assert untouched(x)


# ------------------------------------------------------------------------------------------------ medp_pos_embed_bicubic
def _pos(s, D, g):
    return torch.randn(1 + s * s, D, generator=g)                   # unit scale: an error is not hidden behind 0.02


def _bicubic_fwd(pos, s, gh, gw):
    D = pos.shape[1]
    out = nan32(2 + gh * gw, D)
    call("medp_pos_embed_bicubic", pos.to(DEV), out, s, gh, gw, D)
    assert untouched(out[-1:])
    return out[:-1]


@pytest.mark.parametrize("s,gh,gw,D", [c + (8,) for c in R.BICUBIC_CASES] + [(37, 40, 23, 6)])
def test_pos_embed_bicubic(s, gh, gw, D):
    pos = _pos(s, D, torch.Generator().manual_seed(s * 10000 + gh * 100 + gw))
    out = _bicubic_fwd(pos, s, gh, gw)
    within(out, R.pos_bicubic(pos.double(), s, gh, gw), R.BICUBIC_TOL, f"bicubic {s} -> {gh}x{gw}")
    assert torch.equal(out[0].cpu(), pos[0])                        # the class row is a copy


@pytest.mark.parametrize("s", [3, 5, 37])
def test_pos_embed_bicubic_onto_the_same_grid_is_a_copy(s):
    pos = _pos(s, 8, torch.Generator().manual_seed(s))
    assert torch.equal(bits(_bicubic_fwd(pos, s, s, s)), bits(pos))  # t = 0: the taps are exactly (0, 1, 0, 0)


# ------------------------------------------------------------------------------------------------ medp_pos_embed_bicubic_bwd
def _bicubic_bwd(dout, s, gh, gw):
    D = dout.shape[1]
    dpos = nan32(2 + s * s, D)
    call("medp_pos_embed_bicubic_bwd", dout.to(DEV), dpos, s, gh, gw, D)
    assert untouched(dpos[-1:])
    return dpos[:-1]


# 132: the d4 loop's second trip.  37 -> 4 x 5: the 4-tap footprints (source spacing 9.25 and 7.4) leave source cells that no
# destination reads; at 37 -> 16 (spacing 2.3) every source cell is still read
@pytest.mark.parametrize("s,gh,gw,D", [c + (8,) for c in R.BICUBIC_CASES] + [(5, 3, 9, 132), (37, 4, 5, 8)])
def test_pos_embed_bicubic_bwd(s, gh, gw, D):
    g = torch.Generator().manual_seed(s * 10000 + gh * 100 + gw + 1)
    pos, dout = _pos(s, D, g), torch.randn(1 + gh * gw, D, generator=g)
    pr = pos.double().requires_grad_(True)
    (want,) = torch.autograd.grad((R.pos_bicubic(pr, s, gh, gw) * dout.double()).sum(), pr)
    got = _bicubic_bwd(dout, s, gh, gw)
    assert not bool(torch.isnan(got).any())                         # every one of the 1 + s*s rows is written
    within(got, want, R.BICUBIC_TOL, f"bicubic backward {s} <- {gh}x{gw}")
    # source cells that no destination reads (strong down-sampling) get exactly 0.0
    zero = want == 0
    print(f"  {int(zero.sum())} of {zero.numel()} reference entries are exactly zero")
    assert bool((got.cpu()[zero] == 0).all())
    if (s, gh, gw) == (37, 4, 5):
        assert int(zero.sum()) > 37 * 37 * D // 2
    assert torch.equal(bits(got), bits(_bicubic_bwd(dout, s, gh, gw)))              # a gather: two runs agree bit for bit
    # <fwd(p), d> == <p, bwd(d)>, in float64 on the two kernels' outputs, relative to the inner product itself
    lhs = float((_bicubic_fwd(pos, s, gh, gw).double().cpu() * dout.double()).sum())
    rhs = float((pos.double() * got.double().cpu()).sum())
    print(f"  adjoint: {lhs:.9e} against {rhs:.9e}: {abs(lhs - rhs) / (1e-5 * max(abs(lhs), abs(rhs))):.4f} of the bound")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


def test_pos_embed_bicubic_bwd_refuses_a_width_that_is_no_multiple_of_4():
    dpos = nan32(1 + 25, 6)
    with pytest.raises(ValueError):
        call("medp_pos_embed_bicubic_bwd", torch.zeros(1 + 12, 6, device=DEV), dpos, 5, 3, 4, 6)
    assert untouched(dpos)


# ------------------------------------------------------------------------------------------------ medp_gelu_bf16_fwd / _bwd
def _all_bf16():
    """every bf16 bit pattern once: 65 536 values, NaNs and infinities among them"""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)


def test_gelu_bf16_fwd_at_every_bf16_input():
    x = _all_bf16()
    out = nan16(x.numel() + 8)
    call("medp_gelu_bf16_fwd", x.to(DEV), out, x.numel())
    assert untouched(out[-8:])
    fin = torch.isfinite(x.float())
    assert int(fin.sum()) == 65536 - 2 * 128
    xd, got = x.double()[fin], out[:-8].cpu().double()[fin]
    ref = R.gelu(xd)
    assert bool(torch.isfinite(got).all())
    # one bf16 ulp (fp32 error may flip the final rounding) + erf by A&S 7.1.26 (1.5e-7, 0.75e-7 |x| on GELU) and fp32 rounding
    bound = 2.0 ** -7 * ref.abs() + 1e-6 * xd.abs().clamp(min=1.0)
    ratio = (got - ref).abs() / bound
    i = int(ratio.argmax())
    print(f"gelu forward: worst {float(ratio[i]):.3f} of the bound at x = {float(xd[i]):.6g} (got {float(got[i]):.6g}, ref {float(ref[i]):.6g}); "
          f"{int((ratio > 0.5).sum())} of {ratio.numel()} above half of it")
    assert bool((ratio <= 1).all()), int((ratio > 1).sum())


@pytest.mark.parametrize("dy_kind", ["ones", "seeded"])
def test_gelu_bf16_bwd_at_every_bf16_input(dy_kind):
    x = _all_bf16()
    dy = torch.ones(x.numel()).bfloat16() if dy_kind == "ones" else torch.randn(x.numel(), generator=torch.Generator().manual_seed(11)).bfloat16()
    dx = nan16(x.numel() + 8)
    call("medp_gelu_bf16_bwd", dy.to(DEV), x.to(DEV), dx, x.numel())
    assert untouched(dx[-8:])
    fin = torch.isfinite(x.float())
    xd, dyd, got = x.double()[fin], dy.double()[fin], dx[:-8].cpu().double()[fin]
    ref = dyd * R.gelu_grad(xd)
    assert bool(torch.isfinite(got).all())
    bound = 2.0 ** -7 * ref.abs() + 1e-6 * dyd.abs()
    ratio = (got - ref).abs() / bound
    i = int(ratio.argmax())
    print(f"gelu backward ({dy_kind}): worst {float(ratio[i]):.3f} of the bound at x = {float(xd[i]):.6g}, dy = {float(dyd[i]):.6g} "
          f"(got {float(got[i]):.6g}, ref {float(ref[i]):.6g}); {int((ratio > 0.5).sum())} of {ratio.numel()} above half of it")
    assert bool((ratio <= 1).all()), int((ratio > 1).sum())


def test_gelu_bf16_single_thread_and_bad_length():
    x = torch.tensor([-3.0, -0.5, 0.0, 0.25, 1.0, 2.5, -8.0, 6.0]).bfloat16()       # lo and hi halves of four dwords, all different
    dy = torch.tensor([1.0, -2.0, 0.5, 3.0, -1.0, 0.25, 2.0, -0.5]).bfloat16()
    out, dx = nan16(16), nan16(16)
    call("medp_gelu_bf16_fwd", x.to(DEV), out, 8)
    call("medp_gelu_bf16_bwd", dy.to(DEV), x.to(DEV), dx, 8)
    assert untouched(out[8:]) and untouched(dx[8:])
    ref, dref = R.gelu(x.double()), dy.double() * R.gelu_grad(x.double())
    assert bool(((out[:8].cpu().double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-6 * x.double().abs().clamp(min=1.0)).all())
    assert bool(((dx[:8].cpu().double() - dref).abs() <= 2.0 ** -7 * dref.abs() + 1e-6 * dy.double().abs()).all())
    for n in (4, 12):
        with pytest.raises(ValueError):
            call("medp_gelu_bf16_fwd", x.to(DEV), out, n)
        with pytest.raises(ValueError):
            call("medp_gelu_bf16_bwd", dy.to(DEV), x.to(DEV), dx, n)


# ------------------------------------------------------------------------------------------------ medp_cast_f32_bf16, strided
def _padded(rows, cols, ld, g, dtype=F32):
    """[rows, ld] with the matrix in the first `cols` columns and 1e30 in the gap, which must never be read"""
    xp = torch.full((rows, ld), 1e30)
    xp[:, :cols] = torch.randn(rows, cols, generator=g)
    return xp.to(dtype)


@pytest.mark.parametrize("rows,cols,ldx,ldy", [(5, 8, 12, 16), (37, 64, 64, 72), (1, 4, 4, 4)])
def test_cast_strided(rows, cols, ldx, ldy):
    xp = _padded(rows, cols, ldx, torch.Generator().manual_seed(rows))
    y = nan16(rows + 1, ldy)
    call("medp_cast_f32_bf16", xp.to(DEV), ldx, y, ldy, rows, cols)
    assert torch.equal(bits(y[:rows, :cols]), bits(xp[:, :cols].bfloat16()))
    assert untouched(y[:rows, cols:]) and untouched(y[rows:])


def test_cast_refuses():
    x, y = torch.zeros(4, 16, device=DEV), nan16(4, 16)
    # cols % 4, empty, ld % 4, and ldy < cols: rows of the result would overlap and the last one end past rows * ldy elements
    for ldx, ldy, rows, cols in [(16, 16, 4, 6), (16, 16, 4, 0), (16, 16, 0, 8), (14, 16, 4, 8), (16, 10, 4, 8), (16, 4, 4, 8)]:
        with pytest.raises(ValueError):
            call("medp_cast_f32_bf16", x, ldx, y, ldy, rows, cols)
    assert untouched(y)
    call("medp_cast_f32_bf16", x, 16, y, 4, 1, 16)                  # one row: ldy is never used
    assert bool((bits(y[0]) == 0).all()) and untouched(y[1:])


# ------------------------------------------------------------------------------------------------ medp_transpose_to_bf16, strided
TRANSPOSE_CASES = [(1, 1, 1, 8), (63, 65, 80, 64), (65, 63, 63, 72), (130, 129, 136, 136)]


@pytest.mark.parametrize("src", [F32, BF16])
@pytest.mark.parametrize("rows,cols,ldx,ldy", TRANSPOSE_CASES)
def test_transpose_strided(rows, cols, ldx, ldy, src):
    xp = _padded(rows, cols, ldx, torch.Generator().manual_seed(rows + cols), src)
    y = nan16(cols + 1, ldy)
    call("medp_transpose_to_bf16", xp.to(DEV), int(src == BF16), ldx, y, ldy, rows, cols)
    assert torch.equal(bits(y[:cols, :rows]), bits(xp[:, :cols].bfloat16().T))
    assert untouched(y[:cols, rows:]) and untouched(y[cols:])


def test_transpose_refuses():
    x, y = torch.zeros(8, 16, device=DEV), nan16(16, 8)
    for ldx, ldy, rows, cols in [(12, 8, 8, 16), (16, 7, 8, 16), (16, 8, 0, 16), (16, 8, 8, 0)]:       # ldx < cols, ldy < rows, empty
        with pytest.raises(ValueError):
            call("medp_transpose_to_bf16", x, 0, ldx, y, ldy, rows, cols)
    assert untouched(y)


# ------------------------------------------------------------------------------------------------ medp_weight_operands_multi
def test_weight_operands_multi():
    """One launch, fifteen jobs: five shapes (one element, both sides of the 64-tile edge, several tiles, one exact tile), each asked
    for its plain copy only, its transposed copy only, and both; every leading dimension wider than the matrix."""
    abi = _abi()
    g = torch.Generator().manual_seed(3)
    shapes = [(1, 1), (63, 65), (65, 63), (130, 129), (64, 64)]
    jobs, blk_job, blk_tile, held = [], [], [], []
    for rows, cols in shapes:
        for want_plain, want_t in ((True, False), (False, True), (True, True)):
            ld_src, ld_plain, ld_t = cols + 3, cols + 5, rows + 2
            src = _padded(rows, cols, ld_src, g).to(DEV)
            plain, tr = nan16(rows + 1, ld_plain), nan16(cols + 1, ld_t)           # allocated either way: an absent one must stay NaN
            jobs.append(abi.MedpOperandJob(src.data_ptr(), plain.data_ptr() if want_plain else None, tr.data_ptr() if want_t else None,
                                           rows, cols, ld_src, ld_plain, ld_t, 0))
            tiles = ((rows + 63) // 64) * ((cols + 63) // 64)                      # the block map: one block per 64 x 64 tile
            blk_job += [len(jobs) - 1] * tiles
            blk_tile += list(range(tiles))
            held.append((rows, cols, src, plain, tr, want_plain, want_t))
    table = torch.from_numpy(abi.table_bytes((abi.MedpOperandJob * len(jobs))(*jobs), len(jobs))).to(DEV)
    assert table.numel() == len(jobs) * ctypes.sizeof(abi.MedpOperandJob)
    call("medp_weight_operands_multi", table, torch.tensor(blk_job, dtype=torch.int32, device=DEV),
         torch.tensor(blk_tile, dtype=torch.int32, device=DEV), len(blk_job))
    for rows, cols, src, plain, tr, want_plain, want_t in held:
        m = src[:, :cols]
        if want_plain:
            assert torch.equal(bits(plain[:rows, :cols]), bits(m.cpu().bfloat16())), (rows, cols)
            assert untouched(plain[:rows, cols:]) and untouched(plain[rows:])
            if cols % 4 == 0:                                       # the per-tensor cast kernel takes this width
                y = nan16(rows, cols)
                call("medp_cast_f32_bf16", m.contiguous(), cols, y, cols, rows, cols)
                assert torch.equal(bits(plain[:rows, :cols]), bits(y))
        else:
            assert untouched(plain)
        if want_t:
            assert torch.equal(bits(tr[:cols, :rows]), bits(m.cpu().bfloat16().T)), (rows, cols)
            assert untouched(tr[:cols, rows:]) and untouched(tr[cols:])
            y = nan16(cols, rows)
            call("medp_transpose_to_bf16", src, 0, src.shape[1], y, rows, rows, cols)
            assert torch.equal(bits(tr[:cols, :rows]), bits(y))
        else:
            assert untouched(tr)


def test_weight_operands_multi_refuses():
    t = torch.zeros(64, dtype=torch.uint8, device=DEV)
    i = torch.zeros(1, dtype=torch.int32, device=DEV)
    for args in [(None, i, i, 1), (t, None, i, 1), (t, i, None, 1), (t, i, i, 0)]:
        with pytest.raises(ValueError):
            call("medp_weight_operands_multi", *args)
