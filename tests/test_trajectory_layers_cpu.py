"""CPU-side checks of the stacked trajectory encoder (n_layers > 1): construction, the state_dict of torch's stacked GRU under
`temporal.` (names and shapes, also those the reference's own class stored in tests/golden/trajectory_layers*.npz), torch's error for
n_layers = 0, the unchanged d_model = 64 behaviour, and the new C symbols."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _encoder(**kw):
    from multimodal_edema_prediction_amd.trajectory import LocalTrajectoryEncoder
    return LocalTrajectoryEncoder(n_vars=3, n_timesteps=24, **kw)


def test_two_layers_construct_with_torchs_gru_as_the_container():
    m = _encoder(d_model=128, n_layers=2, dropout=0.1)
    assert m.temporal.num_layers == 2 and m.temporal.dropout == 0.1 and m.temporal.batch_first
    assert _encoder(d_model=128, n_layers=1, dropout=0.1).temporal.dropout == 0.0        # reference :1301


@pytest.mark.parametrize("layers", [2, 3])
def test_state_dict_is_torchs_stacked_gru(layers):
    m = _encoder(d_model=128, n_layers=layers)
    ref = torch.nn.GRU(128, 128, layers).state_dict()
    ours = {k[len("temporal."):]: v for k, v in m.state_dict().items() if k.startswith("temporal.")}
    assert list(ours) == list(ref)
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in ref.items()}


def test_state_dict_equals_the_fixtures():
    z = np.load(os.path.join(GOLD, "trajectory_layers.npz"))
    stored = {k[2:]: tuple(z[k].shape) for k in z.files if k.startswith("p_")}
    m = _encoder(d_model=128, n_layers=2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == stored
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p_")}, strict=True)
    grads = np.load(os.path.join(GOLD, "trajectory_layers_grads.npz"))
    assert {k[2:] for k in grads.files} == {k for k, _ in m.named_parameters()}
    z3 = np.load(os.path.join(GOLD, "trajectory_layers_l3.npz"))
    m3 = _encoder(d_model=128, n_layers=3)
    extra = {k[2:]: tuple(z3[k].shape) for k in z3.files if k.startswith("p_")}
    assert set(extra) == set(m3.state_dict()) - set(m.state_dict())
    assert all(tuple(m3.state_dict()[k].shape) == s for k, s in extra.items())
    for f in ("trajectory_layers.npz", "trajectory_layers_grads.npz", "trajectory_layers_l3.npz"):
        assert os.path.getsize(os.path.join(GOLD, f)) < 2 ** 20, f


def test_zero_layers_fail_as_torchs_gru_does():
    with pytest.raises(ValueError) as ours:
        _encoder(d_model=128, n_layers=0)
    with pytest.raises(ValueError) as theirs:
        torch.nn.GRU(128, 128, num_layers=0, batch_first=True)
    assert str(ours.value) == str(theirs.value)


def test_other_hidden_sizes_still_construct():
    """d_model = 64 builds (and is refused by the kernels at the first forward: tests/test_gpu_trajectory.py), one layer or two."""
    assert _encoder(d_model=64).temporal.hidden_size == 64
    assert _encoder(d_model=64, n_layers=2).temporal.num_layers == 2


def test_probe_and_driver_take_the_depth():
    from multimodal_edema_prediction_amd import train_synthetic
    from multimodal_edema_prediction_amd.trajectory_probe import TrajectoryPathologyProbe
    m = TrajectoryPathologyProbe(n_vars=3, n_pathologies=7, n_timesteps=24, d_model=128, gru_layers=2, n_heads=4, dropout=0.1,
                                 recency_windows=(6, 12, 24))
    assert "encoder.temporal.weight_ih_l1" in m.state_dict()
    a = train_synthetic.parse_args(["trajectory_probe", "--ckpt_dir", "x", "--gru_layers", "2"])
    state = {"args": vars(a), "labels": tuple(range(7)), "model": {}}
    state["args"].update(n_vars=3)
    state["model"] = m.state_dict()
    assert train_synthetic.build_trajectory_probe_from_ckpt(state).encoder.n_layers == 2


def test_new_symbols_are_declared_and_tabled():
    from multimodal_edema_prediction_amd import abi
    header = open(os.path.join(ROOT, "include", "medp_hip.h")).read()
    for s in ("medp_gru_fwd_h16", "medp_gru_bwd_dgi16"):
        assert s in abi.SIGNATURES, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    n = len(abi.SIGNATURES["medp_gru_fwd"][1])
    assert len(abi.SIGNATURES["medp_gru_fwd_h16"][1]) == n + 4           # + hseq_bf16, dropout_p, seed, stream_id
    assert len(abi.SIGNATURES["medp_gru_bwd_dgi16"][1]) == len(abi.SIGNATURES["medp_gru_bwd"][1]) + 1
    L = abi.lib()
    assert L.medp_gru_fwd_h16(None, None, None, None, None, None, None, 0.0, 0, 0, 16, 24, 128, None) < 0
    assert b"null" in L.medp_last_error()
