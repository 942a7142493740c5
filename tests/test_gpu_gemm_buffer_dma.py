"""The buffer-addressed LDS-DMA stream of the 256-tile block GEMMs (csrc/gemm_bf16_v6.hip, csrc/gemm_bf16_v7.hip, csrc/gemm_tile256.h): rows
past M / N are dropped by the descriptors' range check instead of being staged from a zero chunk, so every case here puts A, W and C
INSIDE larger buffers of NaN (before, behind and between the rows): a read past a piece's records that reaches a stored element, and
any element the kernel does not write, shows up as NaN; a store outside C shows up as a hole in the NaN around it.

Shapes are the smallest that reach each path (debug entry medp_dbg_gemm_tile256: the kernels without the dispatcher's grid-size rules):
the persistent kernel with 8 workgroups walking 9 / 27 tiles whose last row-tile holds 2 live rows; the one-tile kernel with 256-row
tiles, with 224-row tiles whose last one holds 112 / 12 / 200 rows (residual in place and out of place), and with a K that is no
multiple of 64 (the per-lane path that stays for it).  References are fp32 products of the bf16 operands, tolerances those of
tools/check_gemm_v7.py and tools/check_gemm_v6_n768.py."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PAD = 4096          # NaN elements before and behind every operand (a multiple of 8: operands stay 16-byte aligned)


def _hook():
    from multimodal_edema_prediction_amd.abi import lib
    L = lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    L.medp_dbg_gemm_tile256.restype = I
    L.medp_dbg_gemm_tile256.argtypes = [I, P, P, P] + [I] * 6 + [P, P, P] + [I] * 3 + [P]
    return L


def _poisoned(rows, cols, ld, dtype, fill=None):
    """[rows, cols] view with row stride ld inside a NaN buffer; `fill`: values for the view (default: left NaN)"""
    import torch
    buf = torch.full((2 * PAD + rows * ld,), float("nan"), device="cuda", dtype=dtype)
    view = buf[PAD:PAD + rows * ld].view(rows, ld)[:, :cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _surroundings_intact(buf, rows, cols, ld):
    """everything of the buffer outside the [rows, cols] view is still NaN"""
    import torch
    body = buf[PAD:PAD + rows * ld].view(rows, ld)
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + rows * ld:]).all() and torch.isnan(body[:, cols:]).all())


def _run(kernel, m, n, k, pad_ld, out_dtype, bias=False, scale=False, residual=None, act=0, seed=0):
    """one launch through the debug entry; returns (result view, fp32 reference, C's buffer) — residual: None / "out" / "inplace" """
    import torch
    from multimodal_edema_prediction_amd.abi import check, ptr, stream
    L = _hook()
    g = torch.Generator(device="cuda").manual_seed(seed)
    lda, ldw, ldc = k + pad_ld, k + 2 * pad_ld, n + (8 if pad_ld else 0)
    _, a = _poisoned(m, k, lda, torch.bfloat16, torch.randn(m, k, device="cuda", generator=g))
    _, w = _poisoned(n, k, ldw, torch.bfloat16, torch.randn(n, k, device="cuda", generator=g))
    b = torch.randn(n, device="cuda", generator=g) if bias else None
    s = torch.rand(n, device="cuda", generator=g) + 0.5 if scale else None
    r0 = torch.randn(m, n, device="cuda", generator=g) if residual else None
    cbuf, c = _poisoned(m, n, ldc, out_dtype, r0 if residual == "inplace" else None)
    r = c if residual == "inplace" else r0
    ref = a.float() @ w.float().T
    if bias:
        ref = ref + b
    if act:
        ref = torch.nn.functional.gelu(ref)
    if scale:
        ref = ref * s
    if residual:
        ref = ref + r0
    check(L.medp_dbg_gemm_tile256(kernel, ptr(a), ptr(w), ptr(c), m, n, k, lda, ldw, ldc, ptr(b), ptr(s), ptr(r), r.stride(0) if residual else 0,
                                  act, int(out_dtype == torch.bfloat16), stream()), "gemm_tile256")
    torch.cuda.synchronize()
    assert _surroundings_intact(cbuf, m, n, ldc), "a store outside C"
    return c, ref


def _rel_to_max(y, ref):
    err = (y.float() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"max error relative to max |ref|: {err:.3e}")
    return err


@pytest.fixture
def eight_workgroups():
    """the persistent kernel on 8 workgroups: 9 / 27 tiles are then two / four rounds"""
    L = _hook()
    prev = L.medp_gemm_persistent_cap(8)
    yield
    L.medp_gemm_persistent_cap(prev)


@pytest.mark.parametrize("n", [768, 2304])
@pytest.mark.parametrize("pad_ld,bias_act", [(0, False), (8, True)])
def test_persistent_kernel_last_row_tile_of_two_rows(eight_workgroups, n, pad_ld, bias_act):
    import torch
    y, ref = _run(7, 514, n, 256, pad_ld, torch.bfloat16, bias=bias_act, act=int(bias_act))
    assert torch.isfinite(y).all(), "NaN: an unwritten element, or a read past the operands reached a stored one"
    assert _rel_to_max(y, ref) <= 2e-2


def test_persistent_kernel_on_the_qkv_shape():
    """the product path (dispatcher, 200 resident workgroups, three rounds) once: M = 64 x 257, N = 2304, K = 768"""
    import torch
    from multimodal_edema_prediction_amd import functional as Fn
    g = torch.Generator(device="cuda").manual_seed(1)
    m, n, k = 16448, 2304, 768
    _, a = _poisoned(m, k, k, torch.bfloat16, torch.randn(m, k, device="cuda", generator=g))
    _, w = _poisoned(n, k, k, torch.bfloat16, torch.randn(n, k, device="cuda", generator=g))
    bias = torch.randn(n, device="cuda", generator=g)
    cbuf, c = _poisoned(m, n, n, torch.bfloat16)
    Fn.gemm(a, w, bias=bias, act=1, out=c)
    torch.cuda.synchronize()
    ref = torch.nn.functional.gelu(a.float() @ w.float().T + bias)
    assert _surroundings_intact(cbuf, m, n, n)
    assert torch.isfinite(c).all()
    assert _rel_to_max(c, ref) <= 2e-2


@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_one_tile_kernel_256_row_tiles(out_dtype):
    import torch
    dt = getattr(torch, out_dtype)
    y, ref = _run(6, 300, 768, 256, 8, dt, bias=True)
    assert torch.isfinite(y).all()
    if dt == torch.float32:
        err = (y - ref).abs().max().item()
        print(f"max abs error {err:.3e}")
        assert err <= 1e-3 * 256 ** 0.5 + 1e-3
    else:
        assert _rel_to_max(y, ref) <= 1e-2


@pytest.mark.parametrize("residual", ["out", "inplace"])
@pytest.mark.parametrize("k", [256, 3072])
@pytest.mark.parametrize("m", [224 + 112, 224 + 12, 224 + 200])
def test_one_tile_kernel_224_row_tiles(m, k, residual):
    """N = 768 with a residual takes 224-row tiles (rows 112-127 of each group's A half: beyond the descriptor of rows 64-111)"""
    import torch
    y, ref = _run(6, m, 768, k, 0, torch.float32, bias=True, scale=True, residual=residual)
    assert torch.isfinite(y).all()
    assert _rel_to_max(y, ref) <= 1e-3


@pytest.mark.parametrize("residual", [None, "out"])
def test_one_tile_kernel_k_tail(residual):
    """K = 200: no multiple of 64, the per-lane path with its zero chunk past K (256- and 224-row tiles)"""
    import torch
    y, ref = _run(6, 300, 768, 200, 8, torch.float32, bias=True, residual=residual)
    assert torch.isfinite(y).all()
    assert _rel_to_max(y, ref) <= 1e-3
