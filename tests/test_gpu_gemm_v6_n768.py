"""The 224 x 256 tiles of the one-tile-per-workgroup GEMM (csrc/gemm_bf16_v6.hip, GR = 112: proj / fc2 of the CXR encoder, N = 768
with a residual) against its 256 x 256 tiles: BIT-identical results on the step's shapes and on ragged last tiles, both also against
an fp32 product.  The check runs three child processes (MEDP_V6_N768 = 1 / 0 / 2; the switch is read once per process)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_224_row_tiles_are_bit_identical_to_256_row_tiles():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_gemm_v6_n768.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:]
