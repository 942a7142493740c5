"""CPU-side checks of the trajectory probe's plumbing: the fixture generator reproduces its files' keys from the reference (where the
reference is present), the new C symbols are declared and tabled, `FusedAdamW` takes `max_grad_norm`, the model has the reference
class's parameter names, and the training driver has the stage."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = ("trajectory_probe.npz", "trajectory_probe_params_encoder.npz", "trajectory_probe_params_readout.npz",
         "trajectory_probe_grads_encoder.npz", "trajectory_probe_grads_readout.npz")
sys.path.insert(0, GOLD)
from make_golden import REF  # noqa: E402  (where the generator scripts look for the reference checkout)

SYMBOLS = ("medp_attn_small_masked_fwd", "medp_attn_small_masked_bwd", "medp_grad_sumsq_multi", "medp_adamw_multi_dscale")
STATE_KEYS = ("pathology_queries", "label_bias", "norm_q.weight", "norm_kv.bias", "norm_ff.weight", "cross_attn.in_proj_weight",
              "cross_attn.in_proj_bias", "cross_attn.out_proj.weight", "cross_attn.out_proj.bias", "ff.0.weight", "ff.3.bias",
              "head.0.weight", "head.1.weight", "head.4.bias", "encoder.rep_token", "encoder.temporal.weight_hh_l0")


def test_fixture_files_are_small_and_hold_the_expected_keys():
    main = np.load(os.path.join(GOLD, FILES[0]))
    assert set(main.files) == {"x", "y", "mask", "logits", "attn", "pad", "loss", "grad_norm", "step_losses", "cfg"}
    assert float(main["grad_norm"]) > 1.0 and main["step_losses"].shape == (3,)
    assert bool(main["pad"][-1].all()) and np.isfinite(main["logits"]).all()
    params = set(np.load(os.path.join(GOLD, FILES[1])).files) | set(np.load(os.path.join(GOLD, FILES[2])).files)
    grads = set(np.load(os.path.join(GOLD, FILES[3])).files) | set(np.load(os.path.join(GOLD, FILES[4])).files)
    assert params == grads and set(STATE_KEYS) <= params
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLD, f)) < 2 ** 20, f


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not on this machine")
def test_fixture_regenerates_with_the_committed_keys(tmp_path):
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_trajectory_probe.py"), str(tmp_path)], check=True, timeout=300,
                   stdout=subprocess.DEVNULL)
    for f in FILES:
        new, old = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(GOLD, f))
        assert sorted(new.files) == sorted(old.files), f
        for k in old.files:
            assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype, (f, k)
    new, old = np.load(os.path.join(tmp_path, FILES[0])), np.load(os.path.join(GOLD, FILES[0]))
    assert np.array_equal(new["x"], old["x"]) and np.array_equal(new["pad"], old["pad"])
    assert np.allclose(new["logits"], old["logits"], atol=1e-4)          # same seeds; CPU summation order may differ between hosts


def test_new_symbols_are_declared_and_tabled():
    from multimodal_edema_prediction_amd import abi
    header = open(os.path.join(ROOT, "include", "medp_hip.h")).read()
    for s in SYMBOLS:
        assert s in abi.SIGNATURES, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    n = len(abi.SIGNATURES["medp_attn_small_fwd"][1])
    assert len(abi.SIGNATURES["medp_attn_small_masked_fwd"][1]) == n + 2          # + key_mask, mask_batch_stride
    assert len(abi.SIGNATURES["medp_attn_small_masked_bwd"][1]) == len(abi.SIGNATURES["medp_attn_small_bwd"][1]) + 2
    assert len(abi.SIGNATURES["medp_adamw_multi_dscale"][1]) == len(abi.SIGNATURES["medp_adamw_multi"][1])


def test_fused_adamw_accepts_max_grad_norm():
    from multimodal_edema_prediction_amd.optim import FusedAdamW
    sig = inspect.signature(FusedAdamW.__init__)
    assert sig.parameters["max_grad_norm"].default is None
    p = torch.nn.Parameter(torch.zeros(3))
    assert FusedAdamW([p], max_grad_norm=1.0).max_grad_norm == 1.0
    assert FusedAdamW([p]).max_grad_norm is None and FusedAdamW([p]).last_grad_norm is None
    with pytest.raises(ValueError):
        FusedAdamW([p], max_grad_norm=-1.0)


def test_model_has_the_reference_parameter_names_and_refuses_the_cpu():
    from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe
    m = TrajectoryPathologyProbe(n_vars=6, n_pathologies=7, n_timesteps=24, d_model=128, gru_layers=1, n_heads=4, dropout=0.1,
                                 recency_windows=(6, 12, 24))
    params = set(np.load(os.path.join(GOLD, FILES[1])).files) | set(np.load(os.path.join(GOLD, FILES[2])).files)
    assert set(m.state_dict()) == params
    with pytest.raises(RuntimeError):
        m(tuple(torch.zeros(2, 24, 12)))


def test_training_driver_has_the_stage_with_the_reference_defaults():
    from multimodal_edema_prediction_amd import train_synthetic
    for argv in (["--stage", "trajectory_probe", "--ckpt_dir", "x"], ["trajectory_probe", "--ckpt_dir", "x"]):
        a = train_synthetic.parse_args(argv)
        assert (a.stage, a.batch_size, a.lr, a.weight_decay, a.grad_clip, a.trajectory_windows, a.patience) == \
               ("trajectory_probe", 128, 3e-4, 1e-2, 1.0, "6,12,24", 5)
        assert a.graph
