"""Kernels whose `s_waitcnt vmcnt(N)` waits are counted by hand (the LDS-DMA pieces and loads of a phase, in issue order) must keep
every value in registers: a VGPR spill adds scratch loads and stores to the vector-memory counter and silently shifts those counts.
Compiles the sources for gfx950 with the resource-usage remarks and fails on any scratch or VGPR spill in those kernels.
The counted K-tile body of the two 256-tile GEMMs is written once, in csrc/gemm_tile256.h (tile256_ktile); it is compiled into the kernels of
gemm_bf16_v6.hip and gemm_bf16_v7.hip, which are what is checked here."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_edema_prediction_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# source -> the kernels in it with hand-counted vmcnt waits (a substring of the mangled name); the waits of the two GEMMs live in gemm_tile256.h
HAND_COUNTED = {
    "gemm_bf16_v6.hip": ["gemm_bf16_nt_v6_kernel"],
    "gemm_bf16_v7.hip": ["gemm_bf16_nt_v7_kernel"],
    "attention_dh64.hip": ["attn_fwd_dh64_s257_kernel"],
}


def _resource_usage(src: str, tmp: str) -> dict:
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-x", "hip", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), "-Wno-unused-result", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, src + ".o")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    usage, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return usage


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(HAND_COUNTED))
def test_hand_counted_vmcnt_kernels_do_not_spill(src):
    with tempfile.TemporaryDirectory() as tmp:
        usage = _resource_usage(src, tmp)
    for family in HAND_COUNTED[src]:
        kernels = {k: v for k, v in usage.items() if family in k}
        assert kernels, f"{src}: no resource-usage remark for {family} (remark format changed?)"
        for k, v in kernels.items():
            assert "ScratchSize [bytes/lane]" in v and "VGPRs Spill" in v, (k, v)
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, f"{k} spills: {v}"
