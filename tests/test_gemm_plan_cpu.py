"""CPU: which kernel family, how many K slices and whether a ragged-rows launch the bf16 GEMM front end plans for a shape
(csrc/gemm_bf16.hip: gemm_plan, through the debug hook medp_dbg_gemm_plan, which touches no device).

The expected plans were derived BY HAND from the dispatch rules as they stood before the rules were gathered into gemm_plan; the
rule that fires is the comment on each row.  With t128 = ceil(M/128) * ceil(N/64 if N <= 64 else N/128), nkt = ceil(K/64),
t256 = ceil(M/256) * ceil(N/256), tv3 = ceil(M/256) * ceil(N/128), `big` = M >= 2048 and N >= 256, in this order:
  1. split-K, only with a workspace and tag != 1:  t128 >= 128 or nkt < 8: none;  t128 < 64: min(256 // t128, nkt // 4, 16) slices;
     else min(384 // t128, nkt // 8) slices if nkt >= 32, else none.  More than one slice: 128 x 64 tiles for N <= 64, else 128 x 128.
  2. N <= 64: 128 x 64 tiles.
  3. big and t256 >= 160: the 256-tile kernels: v7 if t256 > 256, bf16 result, no residual / scale, K % 128 == 0, K >= 256; else v6.
  4. big and tv3 >= 192: v3.
  5. 128 x 128 tiles.
MEDP_GEMM_VARIANT=3: rule 3 never, rule 4 for every shape that reaches it; =6: rule 3 for every big shape, always v6; rule 4 never.
The children run with every MEDP_* variable removed (the switches are read once per process), so each forced form has its own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T64, T128, V3, V6, V7 = 64, 128, 3, 6, 7
F32, BF16 = 0, 1

# (M, N, K, tag, workspace, residual, scale, out_bf16) -> (kernel, K slices, ragged-rows launch)
DEFAULT = [
    # ---- bench.py --config teacher / student / probe: the frozen CXR encoder (B 64, 224 x 224, ViT-B/14: M = 64 * 257), tag 1, no workspace
    ((16448, 2304, 768, 1, 0, 0, 0, BF16), (V7, 1, 0)),     # qkv: t256 = 65 * 9 = 585 > 256, bf16, K = 6 * 128 -> v7
    ((16448, 768, 768, 1, 0, 1, 1, F32), (V6, 1, 0)),       # proj: t256 = 65 * 3 = 195 >= 160; fp32 + residual -> v6
    ((16448, 3072, 768, 1, 0, 0, 0, BF16), (V7, 1, 0)),     # fc1: t256 = 65 * 12 = 780 -> v7
    ((16448, 768, 3072, 1, 0, 1, 1, F32), (V6, 1, 0)),      # fc2: as proj
    ((16384, 768, 592, 0, 0, 0, 0, F32), (V6, 1, 0)),       # patch embedding (K = 3 * 14 * 14 padded to 8): t256 = 64 * 3 = 192 -> v6
    # ---- the frozen DuETT encoder (duett.hip: workspace, tag 0), event axis M = 64 * 49, D = 24 * 97; time axis M = 64 * 97, D = 24 * 49
    ((3136, 72, 2328, 0, 1, 0, 0, F32), (T128, 9, 0)),      # event qkv: t128 = 25 * 1, nkt = 37: min(256 // 25 = 10, 37 // 4 = 9, 16)
    ((3136, 2328, 24, 0, 1, 1, 0, F32), (V3, 1, 0)),        # event out: t128 = 25 * 19 = 475: no split; t256 = 13 * 10 = 130; tv3 = 13 * 19 = 247
    ((3136, 512, 2328, 0, 1, 0, 0, BF16), (T128, 3, 0)),    # event ff1: t128 = 100, nkt = 37 >= 32: min(384 // 100 = 3, 37 // 8 = 4)
    ((3136, 2328, 512, 0, 1, 1, 0, F32), (V3, 1, 0)),       # event ff2: as out
    ((6208, 72, 1176, 0, 1, 0, 0, F32), (T128, 4, 0)),      # time qkv: t128 = 49, nkt = 19: min(256 // 49 = 5, 19 // 4 = 4, 16)
    ((6208, 1176, 24, 0, 1, 1, 0, F32), (V3, 1, 0)),        # time out: t128 = 49 * 10: no split; t256 = 25 * 5 = 125; tv3 = 25 * 10 = 250
    ((6208, 512, 1176, 0, 1, 0, 0, BF16), (T128, 1, 0)),    # time ff1: t128 = 49 * 4 = 196 >= 128: no split; t256 = 50; tv3 = 100 < 192
    ((6208, 1176, 512, 0, 1, 1, 0, F32), (V3, 1, 0)),       # time ff2: as out
    # ---- every Fn.gemm shape of the three bench.py configurations (trainable heads, the student's DuETT forward / backward; t / s / p =
    #      teacher / student / probe); Fn.gemm passes a workspace exactly where the query asks for one
    ((7, 256, 256, 0, 0, 0, 0, F32), (T128, 1, 0)),             # s/t: t128 = 2, nkt = 4 < 8; not big
    ((8, 768, 64, 0, 0, 0, 0, F32), (T128, 1, 0)),              # p: t128 = 6, nkt = 1
    ((64, 8, 768, 0, 1, 0, 0, F32), (T64, 3, 0)),               # p: t128 = 1, nkt = 12: min(256, 12 // 4 = 3, 16); N <= 64
    ((64, 128, 1176, 0, 1, 0, 0, F32), (T128, 4, 0)),           # s: t128 = 1, nkt = 19: min(256, 19 // 4 = 4, 16)
    ((64, 1176, 128, 0, 0, 0, 0, F32), (T128, 1, 0)),           # s: t128 = 10, nkt = 2
    ((448, 64, 256, 0, 0, 0, 0, F32), (T64, 1, 0)),             # s/t: t128 = 4, nkt = 4; N <= 64
    ((448, 256, 64, 0, 0, 0, 0, F32), (T128, 1, 0)),            # t: t128 = 8, nkt = 1
    ((448, 256, 256, 0, 0, 1, 0, F32), (T128, 1, 0)),           # s/t: t128 = 8, nkt = 4
    ((448, 256, 512, 0, 1, 0, 0, F32), (T128, 2, 0)),           # t: t128 = 8, nkt = 8: min(32, 8 // 4 = 2, 16)
    ((448, 256, 1024, 0, 1, 1, 0, F32), (T128, 4, 0)),          # s/t: t128 = 8, nkt = 16: min(32, 4, 16)
    ((448, 512, 256, 0, 0, 0, 0, F32), (T128, 1, 0)),           # s/t: t128 = 16, nkt = 4
    ((448, 1024, 256, 0, 0, 0, 0, F32), (T128, 1, 0)),          # s/t: t128 = 32, nkt = 4
    ((3136, 24, 2328, 0, 1, 0, 0, BF16), (T64, 9, 0)),          # s: t128 = 25, nkt = 37: min(10, 9, 16); N <= 64
    ((3136, 72, 2328, 0, 1, 0, 0, BF16), (T128, 9, 0)),         # s: as the frozen encoder's event qkv
    ((3136, 512, 2328, 0, 1, 0, 0, F32), (T128, 3, 0)),         # s: as the frozen encoder's event ff1
    ((3136, 2328, 24, 0, 0, 1, 0, F32), (V3, 1, 0)),            # s: as the frozen encoder's event out
    ((3136, 2328, 72, 0, 0, 0, 0, F32), (V3, 1, 0)),            # s: t128 = 475; t256 = 130; tv3 = 13 * 19 = 247
    ((3136, 2328, 512, 0, 0, 1, 0, F32), (V3, 1, 0)),           # s: the same grid
    ((6144, 40, 1176, 0, 1, 0, 0, F32), (T64, 4, 0)),           # s: t128 = 48, nkt = 19: min(256 // 48 = 5, 4, 16); N <= 64
    ((6144, 256, 512, 0, 0, 0, 0, F32), (T128, 1, 0)),          # t: t128 = 96, nkt = 8 < 32; t256 = 24; tv3 = 48
    ((6144, 256, 1176, 0, 0, 0, 0, F32), (T128, 1, 0)),         # s/t: ts_proj: t128 = 96, nkt = 19 < 32
    ((6144, 512, 256, 0, 0, 0, 0, F32), (T128, 1, 0)),          # s/t: t128 = 192; t256 = 48; tv3 = 96
    ((6144, 1176, 40, 0, 0, 0, 0, F32), (V3, 1, 0)),            # s: t128 = 480; t256 = 24 * 5 = 120; tv3 = 24 * 10 = 240
    ((6208, 24, 1176, 0, 1, 0, 0, BF16), (T64, 4, 0)),          # s: t128 = 49, nkt = 19: min(5, 4, 16); N <= 64
    ((6208, 72, 1176, 0, 1, 0, 0, BF16), (T128, 4, 0)),         # s: as the frozen encoder's time qkv
    ((6208, 512, 1176, 0, 0, 0, 0, F32), (T128, 1, 0)),         # s: as the frozen encoder's time ff1
    ((6208, 1176, 24, 0, 0, 1, 0, F32), (V3, 1, 0)),            # s: as the frozen encoder's time out
    ((6208, 1176, 72, 0, 0, 0, 0, F32), (V3, 1, 0)),            # s: the same grid
    ((6208, 1176, 512, 0, 0, 1, 0, F32), (V3, 1, 0)),           # s: the same grid
    ((16448, 256, 512, 0, 0, 0, 0, F32), (T128, 1, 0)),         # t: t128 = 129 * 2 = 258; t256 = 65; tv3 = 130 < 192
    ((16448, 256, 768, 0, 0, 0, 0, F32), (T128, 1, 0)),         # s/t: img_proj: the same grid
    ((16448, 512, 256, 0, 0, 0, 0, F32), (V3, 1, 0)),           # s/t: t256 = 65 * 2 = 130; tv3 = 65 * 4 = 260
    # ---- tests/test_gpu_kernels.py::test_gemm_split_k_small_grids (Fn.gemm passes the workspace the query asks for)
    ((777, 100, 1160, 0, 1, 0, 0, F32), (T128, 4, 0)),      # t128 = 7, nkt = 19: min(36, 4, 16)   (its other three shapes: DuETT rows above)
    ((3136, 72, 1176, 0, 1, 0, 0, F32), (T128, 4, 0)),      # t128 = 25, nkt = 19: min(10, 4, 16)
    # ---- tests/test_gpu_kernels.py::test_gemm_v3_ragged_tiles
    ((8130, 772, 72, 0, 0, 0, 0, F32), (V3, 1, 0)),         # t256 = 32 * 4 = 128 < 160; tv3 = 32 * 7 = 224 >= 192
    ((8130, 772, 32, 0, 0, 0, 1, F32), (V3, 1, 0)),         # the same grid; the epilogue does not enter rule 4
    ((2048, 256, 72, 0, 0, 0, 0, F32), (T128, 1, 0)),       # big, but t256 = 8 and tv3 = 16
    # ---- both sides of every threshold
    ((13568, 768, 768, 0, 0, 0, 0, F32), (V3, 1, 0)),       # t256 = 53 * 3 = 159; tv3 = 53 * 6 = 318
    ((8192, 1280, 768, 0, 0, 0, 0, F32), (V6, 1, 0)),       # t256 = 32 * 5 = 160
    ((24320, 256, 768, 0, 0, 0, 0, F32), (T128, 1, 0)),     # t256 = 95; tv3 = 95 * 2 = 190 (191 is prime and N >= 256 makes tv3 a multiple of >= 2)
    ((8192, 768, 768, 0, 0, 0, 0, F32), (V3, 1, 0)),        # t256 = 96; tv3 = 32 * 6 = 192
    ((4096, 4096, 768, 0, 0, 0, 0, BF16), (V6, 1, 0)),      # t256 = 16 * 16 = 256: one round of workgroups -> v6
    ((65792, 256, 768, 0, 0, 0, 0, BF16), (V7, 1, 0)),      # t256 = 257 * 1
    ((65792, 256, 768, 0, 0, 0, 0, F32), (V6, 1, 0)),       # ... but an fp32 result is not v7's
    ((4096, 64, 256, 0, 0, 0, 0, F32), (T64, 1, 0)),        # N <= 64
    ((4096, 68, 256, 0, 0, 0, 0, F32), (T128, 1, 0)),       # N = 68
    ((8064, 128, 1024, 0, 1, 0, 0, F32), (T128, 4, 0)),     # t128 = 63, nkt = 16: min(256 // 63 = 4, 4, 16)
    ((8192, 128, 1024, 0, 1, 0, 0, F32), (T128, 1, 0)),     # t128 = 64, nkt = 16 < 32
    ((16256, 128, 2048, 0, 1, 0, 0, F32), (T128, 3, 0)),    # t128 = 127, nkt = 32: min(384 // 127 = 3, 4)
    ((16384, 128, 2048, 0, 1, 0, 0, F32), (T128, 1, 0)),    # t128 = 128
    ((1024, 128, 448, 0, 1, 0, 0, F32), (T128, 1, 0)),      # t128 = 8, nkt = 7
    ((1024, 128, 512, 0, 1, 0, 0, F32), (T128, 2, 0)),      # t128 = 8, nkt = 8: min(32, 8 // 4 = 2, 16)
    ((8192, 128, 1984, 0, 1, 0, 0, F32), (T128, 1, 0)),     # t128 = 64, nkt = 31
    ((8192, 128, 2048, 0, 1, 0, 0, F32), (T128, 4, 0)),     # t128 = 64, nkt = 32: min(384 // 64 = 6, 32 // 8 = 4)
    # ---- the workspace and the tag gate the split
    ((3136, 72, 2328, 0, 0, 0, 0, F32), (T128, 1, 0)),      # no workspace: no split
    ((3136, 72, 2328, 1, 1, 0, 0, F32), (T128, 1, 0)),      # tag 1: no split
    ((3136, 64, 2328, 0, 1, 0, 0, F32), (T64, 9, 0)),       # split decided BEFORE the N <= 64 rule: 128 x 64 tiles, 9 slices
]
FORCED = {
    "3": [((4096, 68, 256, 0, 0, 0, 0, F32), (V3, 1, 0)),           # v3 for any N > 64 ...
          ((16448, 2304, 768, 1, 0, 0, 0, BF16), (V3, 1, 0))],      # ... and the 256-tile kernels never
    "6": [((2048, 256, 768, 0, 0, 0, 0, BF16), (V6, 1, 0)),         # every big shape (t256 = 8) ...
          ((16448, 2304, 768, 1, 0, 0, 0, BF16), (V6, 1, 0)),       # ... and v7 switched off
          ((2040, 256, 768, 0, 0, 0, 0, BF16), (T128, 1, 0))],      # M < 2048 is not forced (and v3 is off: 128 x 128 tiles)
}

CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.medp_gemm_nt_workspace_bytes.restype = ctypes.c_size_t
out = []
for row in json.loads(sys.argv[2]):
    o = (ctypes.c_int * 3)(-1, -1, -1)
    M, N, K, tag, ws, res, scale, ob = row
    rc = L.medp_dbg_gemm_plan(tag, M, N, K, ws, res, scale, ob, o)
    out.append([rc, list(o), L.medp_gemm_nt_workspace_bytes(M, N, K)])
print(json.dumps(out))
"""


def plans(rows, variant=None):
    from multimodal_edema_prediction_amd.abi import LIB_PATH
    env = {k: v for k, v in os.environ.items() if not k.startswith("MEDP_")}
    if variant is not None:
        env["MEDP_GEMM_VARIANT"] = variant
    r = subprocess.run([sys.executable, "-c", CHILD, LIB_PATH, json.dumps([list(k) for k, _ in rows])], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_default_plans_and_workspace_query():
    got = plans(DEFAULT)
    bad = [(k, want, g[1]) for (k, want), g in zip(DEFAULT, got) if g[0] != 0 or tuple(g[1]) != want]
    assert not bad, "(M, N, K, tag, ws, res, scale, bf16), expected, planned: " + "; ".join(map(str, bad))
    for (k, (kernel, nsplit, _)), g in zip(DEFAULT, got):
        M, N, K, tag, ws = k[:5]
        if ws and tag != 1:                               # the query answers for exactly these launches: nsplit * M * N fp32, or nothing
            assert g[2] == (nsplit * M * N * 4 if nsplit > 1 else 0), (k, g[2])
        assert g[2] % (M * N * 4) == 0 and g[2] != M * N * 4, (k, g[2])


@pytest.mark.parametrize("variant", sorted(FORCED))
def test_forced_variant(variant):
    rows = FORCED[variant]
    got = plans(rows, variant)
    bad = [(k, want, g[1]) for (k, want), g in zip(rows, got) if g[0] != 0 or tuple(g[1]) != want]
    assert not bad, f"MEDP_GEMM_VARIANT={variant}: " + "; ".join(map(str, bad))

