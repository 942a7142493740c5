"""CPU: which kernel, grid, workgroup size, dynamic LDS and image rows the head-dim-64 attention launchers plan for a shape
(csrc/attention_dh64.hip: attn_dh64_plan; csrc/attention_dh64_bwd.hip: attn_dh64_bwd_plan), through the debug hook
medp_dbg_attn_dh64_plan, which touches no device.

The expected plans were derived BY HAND from the launch rules as they stood before they were gathered into the plan functions.
With ntile = ceil(S / 16) and crows = min(320, S rounded up to 32), LDS = 2 * crows * 128 bytes (two images of 128-byte rows):
  forward   S = 257 (unless MEDP_ATTN_S257=0): the S = 257 kernel, B * H workgroups of 512 threads, 2 * 288 * 128 + 8 * 68 * 4 bytes;
            S >= MEDP_ATTN_W8_MIN_S (default 512; 0: never): the 8-wave kernel, ceil(ntile / 16) workgroups of 512 threads per (b, h);
            else the 4-wave kernel, floor(ntile / 8) workgroups of 256 threads per (b, h), but at least ceil(ntile / 12);
  backward  ceil(ntile / 8) workgroups of 256 threads per (b, h), LDS + 2 * crows * 4 bytes (L and D of the image rows).
The general kernels deal the ntile subtiles over the nwave waves of a (b, h): wave gw takes ntile // nwave, one more if gw < ntile % nwave,
and branches on that count: 0..3 in the 4-wave kernel, 0..2 in the 8-wave kernel and in the backward.  A larger count would fall into the
idle branch and leave queries unwritten, so the sweep below holds the plans to those limits for every S up to 4096.  (It found one:
max(1, floor(ntile / 8)), the rule as first gathered, is ONE workgroup at ntile = 13..15, S = 193..240, and a wave with 4 subtiles;
hence the ceil(ntile / 12).  Every hand-derived row below is the same under both rules.)
The children run with every MEDP_* variable removed (the switches are read once per process), so each setting has its own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W4, W8, S257, BWD = 4, 8, 257, 2
KERNEL, GX, GY, GZ, THREADS, LDS, CROWS, MOST, SUM = range(9)

# (B, S, H) -> (kernel, grid x, threads, crows (None: not a quantity of that kernel), LDS bytes); grid y, z = H, B for the general kernels
FORWARD = [
    ((2, 257, 3), (S257, 6, 512, None, 2 * 288 * 128 + 8 * 68 * 4)),      # one workgroup per (b, h): 75904 bytes
    ((2, 1, 3), (W4, 1, 256, 32, 8192)),
    ((2, 64, 3), (W4, 1, 256, 64, 16384)),
    ((2, 192, 3), (W4, 1, 256, 192, 49152)),                               # ntile = 12: three subtiles per wave
    ((2, 193, 3), (W4, 2, 256, 224, 57344)),                               # ntile = 13: ceil(13 / 12) workgroups
    ((2, 240, 3), (W4, 2, 256, 256, 65536)),                               # ntile = 15
    ((2, 241, 3), (W4, 2, 256, 256, 65536)),                               # ntile = 16: floor(16 / 8)
    ((2, 400, 3), (W4, 25 // 8, 256, 320, 81920)),
    ((2, 511, 3), (W4, 4, 256, 320, 81920)),                               # ntile = 32
    ((2, 512, 3), (W8, (32 + 15) // 16, 512, 320, 81920)),
    ((2, 513, 3), (W8, 3, 512, 320, 81920)),                               # ntile = 33
    ((2, 1297, 3), (W8, 6, 512, 320, 81920)),                              # ntile = 82
    ((2, 1370, 3), (W8, 6, 512, 320, 81920)),                              # ntile = 86
]
SWITCHED = {
    "MEDP_ATTN_S257": [((2, 257, 3), (W4, 17 // 8, 256, 288, 73728))],
    "MEDP_ATTN_W8_MIN_S": [((2, 1297, 3), (W4, 82 // 8, 256, 320, 81920))],
}
BACKWARD = [
    ((2, 257, 3), (BWD, (17 + 7) // 8, 256, 288, 73728 + 2304)),
    ((2, 1370, 3), (BWD, 11, 256, 320, 81920 + 2560)),
    ((2, 17, 3), (BWD, 1, 256, 32, 8192 + 256)),
]

CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
out = []
for backward, B, S, H in json.loads(sys.argv[2]):
    o = (ctypes.c_int * 9)(*([-1] * 9))
    rc = L.medp_dbg_attn_dh64_plan(backward, B, S, H, o)
    out.append([rc] + list(o))
print(json.dumps(out))
"""


def plans(queries, switch=None):
    """[(backward, B, S, H)] -> [[out[0..8]]], in a fresh process with `switch`=0 (or no switch) set"""
    from multimodal_edema_prediction_amd.abi import LIB_PATH
    env = {k: v for k, v in os.environ.items() if not k.startswith("MEDP_")}
    if switch is not None:
        env[switch] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD, LIB_PATH, json.dumps(queries)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert all(g[0] == 0 for g in got), [q for q, g in zip(queries, got) if g[0] != 0]
    return [g[1:] for g in got]


def check_rows(rows, backward, switch=None):
    got = plans([[backward, *shape] for shape, _ in rows], switch)
    bad = []
    for (shape, (kernel, gx, threads, crows, lds)), g in zip(rows, got):
        B, _, H = shape
        want_yz = [1, 1] if kernel == S257 else [H, B]
        ok = g[KERNEL] == kernel and g[GX] == gx and [g[GY], g[GZ]] == want_yz and g[THREADS] == threads and g[LDS] == lds
        if not ok or (crows is not None and g[CROWS] != crows):
            bad.append((shape, (kernel, gx, threads, crows, lds), g))
    assert not bad, "(B, S, H), expected (kernel, grid x, threads, crows, LDS), planned out[0..8]: " + "; ".join(map(str, bad))


def test_forward_plans():
    check_rows(FORWARD, 0)


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_forward_plans_with_a_switch_off(switch):
    check_rows(SWITCHED[switch], 0, switch)


def test_backward_plans():
    check_rows(BACKWARD, 1)


SWEEP = [("forward", 0, None), ("forward, 8-wave kernel off", 0, "MEDP_ATTN_W8_MIN_S"), ("backward", 1, None)]


@pytest.mark.parametrize("name,backward,switch", SWEEP, ids=[s[0] for s in SWEEP])
def test_every_wave_gets_a_share_its_kernel_has_a_branch_for(name, backward, switch):
    sizes = range(1, 4097)
    got = plans([[backward, 1, S, 1] for S in sizes], switch)
    limit = {W4: 3, W8: 2, S257: 2, BWD: 2}
    bad = [(S, g) for S, g in zip(sizes, got) if g[SUM] != (S + 15) // 16 or not 1 <= g[MOST] <= limit[g[KERNEL]]]
    assert not bad, f"{name}: S, out[0..8] where the shares do not sum to ceil(S / 16) or a wave gets too many: {bad[:10]}"
    kernels = {g[KERNEL] for g in got}
    assert kernels == ({BWD} if backward else {W4, S257} if switch else {W4, W8, S257}), kernels
