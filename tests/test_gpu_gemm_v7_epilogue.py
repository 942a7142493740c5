"""The epilogue of the persistent block GEMM (csrc/gemm_bf16_v7.hip): full tiles take a straight-line, software-pipelined patch chain
(row block i+1 is packed while row block i's LDS reads are in flight), clipped tiles the serial chain with a test per store.  Whatever
the path, the bits are those of the one-tile kernel (csrc/gemm_bf16_v6.hip) on the same operands, and a workgroup that walks several
tiles runs its 16 output stores into the next tile's counted waits.

Debug entry medp_dbg_gemm_tile256 on 8 workgroups.  Shapes, the smallest that reach each path: M = 2 x 256 + 2 (a last row tile of
2 rows) and 3 x 256 (all full); N = 3 x 256 and 2 x 256 + 8 (a clipped column tile); K = 256 (four K-tiles, the minimum) and 768;
with and without bias and GELU; and N = 9 x 256 (27 tiles: four rounds, a workgroup walks three or four tiles).  A, W and C lie inside
NaN-filled buffers; C's buffer covers whole 256 x 256 tiles plus a guard, so a store to a row >= M or a column >= N lands in it."""
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


def _poisoned(rows, cols, ld, dtype, fill=None, alloc_rows=None):
    """[rows, cols] view with row stride ld at the top of alloc_rows rows inside a NaN buffer; `fill`: values for the view"""
    import torch
    alloc_rows = alloc_rows or rows
    buf = torch.full((2 * PAD + alloc_rows * ld,), float("nan"), device="cuda", dtype=dtype)
    view = buf[PAD:PAD + rows * ld].view(rows, ld)[:, :cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _operands(m, n, k, bias, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    _, a = _poisoned(m, k, k + 8, torch.bfloat16, torch.randn(m, k, device="cuda", generator=g))
    _, w = _poisoned(n, k, k + 16, torch.bfloat16, torch.randn(n, k, device="cuda", generator=g))
    b = torch.randn(n, device="cuda", generator=g) if bias else None
    return a, w, b


def _launch(kernel, a, w, b, m, n, k, act):
    """one launch into a fresh NaN buffer of whole tiles; returns (buffer, [m, n] view, ldc, rows of the buffer)"""
    import torch
    from multimodal_edema_prediction_amd.abi import check, ptr, stream
    L = _hook()
    rows = (m + 255) // 256 * 256
    ldc = (n + 255) // 256 * 256 + 8
    cbuf, c = _poisoned(m, n, ldc, torch.bfloat16, alloc_rows=rows)
    check(L.medp_dbg_gemm_tile256(kernel, ptr(a), ptr(w), ptr(c), m, n, k, a.stride(0), w.stride(0), ldc, ptr(b), None, None, 0,
                                  act, 1, stream()), "gemm_tile256")
    torch.cuda.synchronize()
    return cbuf, c, ldc, rows


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16)


@pytest.fixture
def eight_workgroups():
    """the persistent kernel on 8 workgroups: 9 tiles are two rounds, 27 tiles four"""
    L = _hook()
    prev = L.medp_gemm_persistent_cap(8)
    yield
    L.medp_gemm_persistent_cap(prev)


def _check(m, n, k, bias, act):
    import torch
    a, w, b = _operands(m, n, k, bias)
    buf7, c7, ldc, rows = _launch(7, a, w, b, m, n, k, act)
    _, c6, _, _ = _launch(6, a, w, b, m, n, k, act)
    assert not torch.isnan(c7).any(), "NaN in C: an unwritten element, or a read past the operands reached a stored one"
    assert torch.equal(_bits(c7), _bits(c6)), "the persistent kernel's bits differ from the one-tile kernel's"
    assert torch.isnan(buf7[:PAD]).all() and torch.isnan(buf7[PAD + rows * ldc:]).all(), "the NaN guard around C is broken"
    body = buf7[PAD:PAD + rows * ldc].view(rows, ldc)
    assert torch.isnan(body[m:]).all(), "a row >= M was written"
    assert torch.isnan(body[:, n:]).all(), "a column >= N was written"


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("k", [256, 768])
@pytest.mark.parametrize("n", [3 * 256, 2 * 256 + 8])
@pytest.mark.parametrize("m", [2 * 256 + 2, 3 * 256])
def test_epilogue_bits_equal_the_one_tile_kernel(eight_workgroups, m, n, k, bias, act):
    _check(m, n, k, bias, act)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("m", [2 * 256 + 2, 3 * 256])
def test_epilogue_runs_into_the_next_tiles_counted_waits(eight_workgroups, m, act):
    """27 tiles on 8 workgroups: every workgroup walks three or four tiles, full ones after full and clipped ones"""
    _check(m, 9 * 256, 256, True, act)


def test_dispatcher_qkv_shape_eager_and_replayed():
    """the product path (200 resident workgroups, three rounds) at M = 64 x 257, N = 2304, K = 768: eager and two replays of a
    captured graph give the same bits"""
    import torch
    from multimodal_edema_prediction_amd import functional as Fn
    m, n, k = 16448, 2304, 768
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(m, k, device="cuda", generator=g).bfloat16()
    w = torch.randn(n, k, device="cuda", generator=g).bfloat16()
    bias = torch.randn(n, device="cuda", generator=g)
    eager = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
    Fn.gemm(a, w, bias=bias, act=0, out=eager)
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all()
    ref = a.float() @ w.float().T + bias
    err = (eager.float() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"max error relative to max |ref|: {err:.3e}")
    assert err <= 2e-2                      # the bound of tools/check_gemm_v7.py for a bf16 result
    yg = torch.empty_like(eager)
    graph, sg = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(sg):
        Fn.gemm(a, w, bias=bias, act=0, out=yg)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=sg):
            Fn.gemm(a, w, bias=bias, act=0, out=yg)
    for _ in range(2):
        yg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(yg), _bits(eager))
