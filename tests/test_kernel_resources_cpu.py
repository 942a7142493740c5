"""Kernels whose `s_waitcnt vmcnt(N)` waits are counted by hand (the LDS-DMA pieces and loads of a phase, in issue order) must keep
every value in registers: a VGPR spill adds scratch loads and stores to the vector-memory counter and silently shifts those counts.
Compiles the sources for gfx950 with the resource-usage remarks and fails on any scratch or VGPR spill in those kernels.
The counted K-tile body of the two 256-tile GEMMs is written once, in csrc/gemm_tile256.h (tile256_ktile); it is compiled into the kernels of
gemm_bf16_v6.hip and gemm_bf16_v7.hip, which are what is checked here.
The two forward kernels of csrc/attention_dh16.hip (one algorithm: whoever merges or edits them) may not take more registers than they did as
two files (fewer VGPRs is more waves per SIMD on the time axis of every step)."""
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
    "attention_dh64.hip": ["attn_fwd_dh64_s257_kernel"],          # one plain kernel (its LDS-image helpers: csrc/attention_dh64_tile.h)
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


# attention_dh16.hip, the forward kernels: (family, NT, element types in -> out) -> most VGPRs.  The caps are the figures of the parent's
# kernels at commit f05a412, from the same remarks: attn_dh16_fwd_kernel<NT> (then attention_dh16.hip) and dh16_train_fwd_kernel<NT, T>
# (then attention_dh16_train.hip).
DH16_FWD_VGPR_CAPS = {
    **{("inference", nt, "f32->bf16"): v for nt, v in zip((2, 4, 7, 10, 17), (26, 40, 60, 86, 120))},
    **{("training", nt, "f32->f32"): v for nt, v in zip((2, 4, 7, 10, 17), (38, 51, 77, 128, 212))},
    **{("training", nt, "bf16->bf16"): v for nt, v in zip((2, 4, 7, 10, 17), (32, 50, 82, 127, 211))},
}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="needs hipcc")
def test_dh16_forward_instantiations_stay_within_the_registers_of_the_parent():
    with tempfile.TemporaryDirectory() as tmp:
        usage = _resource_usage("attention_dh16.hip", tmp)
    elem = {"f": "f32->f32", "t": "bf16->bf16"}                          # Itanium mangling: float, unsigned short (bf16_t)
    seen = {}
    for k, v in usage.items():
        m = re.search(r"attn_dh16_fwd_kernelILi(\d+)EEE", k)
        if m:
            seen[("inference", int(m.group(1)), "f32->bf16")] = v
        m = re.search(r"dh16_train_fwd_kernelILi(\d+)E([ft])EE", k)
        if m:
            seen[("training", int(m.group(1)), elem[m.group(2)])] = v
    assert set(seen) == set(DH16_FWD_VGPR_CAPS), sorted(set(seen) ^ set(DH16_FWD_VGPR_CAPS))
    for key, v in sorted(seen.items()):
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, f"{key} spills: {v}"
        assert v["VGPRs"] <= DH16_FWD_VGPR_CAPS[key], f"{key}: {v['VGPRs']} VGPRs > {DH16_FWD_VGPR_CAPS[key]}"
