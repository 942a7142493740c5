"""CPU checks of the split-key few-query attention (attention_fq_split.hip): every kernel compiles for gfx950 without scratch or
VGPR spills (its backward keeps a key's scores, dP and dS in registers and reads the query rows from LDS step by step — the
compiler sinks the score sums past later steps otherwise), and bad arguments are refused through the C ABI before any launch."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from multimodal_edema_prediction_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_edema_prediction_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ["attn_fqs_fwd_kernel", "attn_fqs_combine_kernel", "attn_fqs_avg_kernel", "attn_fqs_bwd_kernel", "attn_fqs_dq_kernel"]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="needs hipcc")
def test_split_kernels_do_not_spill():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-x", "hip", "-I", CSRC,
               "-I", os.path.join(ROOT, "include"), "-Wno-unused-result", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(CSRC, "attention_fq_split.hip"), "-o", os.path.join(tmp, "a.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    usage, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    for family in KERNELS:
        found = {k: v for k, v in usage.items() if family in k}
        assert found, f"no resource-usage remark for {family}"
        for k, v in found.items():
            assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0, f"{k} spills: {v}"


def _fwd(L, B=1, Lq=7, Lk=2304, dh=64, k=4096, ldkv=512, ws_bytes=None):
    ws = L.medp_attn_fq_split_ws_bytes(B, 4, Lq, Lk, 0) if ws_bytes is None else ws_bytes
    return L.medp_attn_fq_split_fwd(4096, 256, 0, k, k + 1024, ldkv, Lk * ldkv, 4096, 256, 0, 4096, None, 4096, ws, B, Lq, Lk, 4, dh,
                                    0.125, 0.0, 0, 0, None)


def test_workspace_bytes():
    L = abi.lib()
    # forward: (O row of 64 + m, l) per (batch, head, key slice of 256, query); backward: a dQ row of 64
    assert L.medp_attn_fq_split_ws_bytes(32, 4, 7, 1296, 0) == 32 * 4 * 6 * 7 * 66 * 4
    assert L.medp_attn_fq_split_ws_bytes(32, 4, 7, 1296, 1) == 32 * 4 * 6 * 7 * 64 * 4
    assert L.medp_attn_fq_split_ws_bytes(1, 1, 1, 1, 0) == 66 * 4


@pytest.mark.parametrize("bad,msg", [(dict(dh=32), b"head dim"), (dict(Lq=33), b"Lq 33"), (dict(k=4100), b"aligned"),
                                     (dict(ldkv=510), b"aligned"), (dict(ws_bytes=16), b"workspace"),
                                     (dict(B=64, Lq=32, Lk=(1 << 19) + 1), b"32 bits")])
def test_bad_arguments_are_refused_before_launch(bad, msg):
    L = abi.lib()
    rc = _fwd(L, **bad)
    assert rc < 0 and msg in L.medp_last_error(), L.medp_last_error()


def test_bad_backward_gradient_alignment_is_refused():
    L = abi.lib()
    Lk = 2304
    ws = L.medp_attn_fq_split_ws_bytes(1, 4, 7, Lk, 1)
    rc = L.medp_attn_fq_split_bwd(4096, 256, 4096, 256, 4096, 4096, 256, 0, 4096, 5120, 512, Lk * 512, 4096, 256, 4100, 5124, 512,
                                  Lk * 512, 4096, ws, 1, 7, Lk, 4, 64, 0.125, 0.0, 0, 0, None)
    assert rc < 0 and b"dK / dV" in L.medp_last_error()
