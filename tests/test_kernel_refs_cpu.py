"""CPU checks behind the kernel-level GPU tests: the restatements of tests/kernel_refs.py equal the oracle functions they restate
(so the float64 references of test_gpu_loss_kernels.py / test_gpu_duett_glue_kernels.py are themselves checked without a device),
and the chunk plan of `medp_glinear_bwd` keeps the workspace of every shape that fitted before and is defined for those it refused."""
import pytest
import torch

import kernel_refs as KR
from oracle import duett_ref, losses_ref


@pytest.mark.parametrize("T,alpha,pw", [(1.0, 0.3, None), (4.0, 0.0, 2.5), (4.0, 1.0, None), (2.0, 0.7, 2.5)])
def test_kd_loss_restatement_equals_the_oracle(T, alpha, pw):
    g = torch.Generator().manual_seed(int(T * 10 + alpha * 100))
    z_s, z_t = 3 * torch.randn(257, generator=g), 3 * torch.randn(257, generator=g)         # |z| / T far inside both clamps
    y = (torch.rand(257, generator=g) < 0.4).float()
    a = z_s.clone().requires_grad_(True)
    b = z_s.clone().requires_grad_(True)
    ours, ref = KR.kd_loss(a, z_t, y, T, alpha, pw), losses_ref.student_kd_loss(b, z_t, y, T, alpha, pw)
    for k in ("total", "bce", "kd"):
        torch.testing.assert_close(ours[k], ref[k], rtol=1e-6, atol=0)
    ours["total"].backward()
    ref["total"].backward()
    torch.testing.assert_close(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    # float64, the dtype the GPU tests use: the oracle's python-float bounds and the fp32 constants agree while no element is clamped
    o64 = KR.kd_loss(z_s.double(), z_t.double(), y.double(), T, alpha, pw)
    r64 = losses_ref.vanilla_kl_kd(z_s.double(), z_t.double(), T)
    torch.testing.assert_close(o64["kd"], r64, rtol=1e-13, atol=0)


@pytest.mark.parametrize("smoothing", [0.05, 0.2])
def test_aux_residual_kl_restatement_equals_the_oracle(smoothing):
    g = torch.Generator().manual_seed(5)
    img, sc = 2 * torch.randn(37, 7, generator=g).double(), torch.randn(37, 7, generator=g).double()
    y, m = (torch.rand(37, 7, generator=g) < 0.4).double(), (torch.rand(37, 7, generator=g) < 0.7).double()
    a, b = sc.clone().requires_grad_(True), sc.clone().requires_grad_(True)
    ours, ref = KR.aux_residual_kl(img, a, y, m, smoothing), losses_ref.aux_residual_kl(img, b, y, m, smoothing)
    torch.testing.assert_close(ours, ref, rtol=1e-6, atol=0)              # the oracle forms the smoothed labels in fp32 (`.float()`)
    ours.backward()
    ref.backward()
    torch.testing.assert_close(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    z = torch.zeros_like(m)
    assert float(KR.aux_residual_kl(img, sc, y, z, smoothing)) == 0.0 == float(losses_ref.aux_residual_kl(img, sc, y, z, smoothing))


def test_ssl_terms_add_up_to_the_oracle_loss():
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g).double()
    hv, hp, he, hep, yv, ye = r(6, 16), r(6, 16), r(6, 32), r(6, 32), r(6, 16), r(6, 32)
    m, me = (torch.rand(6, 16, generator=g) < 0.5).double(), (torch.rand(6, 32, generator=g) < 0.5).double()
    ours = KR.masked_mse(hv, yv, m) + 0.2 * KR.bce_mean(hp, m) + KR.masked_mse(he, ye, me) + 0.2 * KR.bce_mean(hep, me)
    torch.testing.assert_close(ours, duett_ref.ssl_loss(hv, hp, he, hep, yv, m, ye, me, 0.2), rtol=1e-14, atol=0)
    torch.testing.assert_close(KR.masked_mse(hv, yv), KR.masked_mse(hv, yv, torch.ones_like(m)), rtol=0, atol=0)


def _tiny_duett(V, T, E, DS, g):
    cfg = duett_ref.DuettCfg(d_static_num=DS, d_time_series_num=V, n_timesteps=T, d_embedding=E, d_hidden_mlp_embedding=5, d_hidden_tab_encoder=6)
    r = lambda *s: torch.randn(*s, generator=g).double()
    sd = {"n_obs_embedding.weight": torch.linspace(-1.0, 2.0, 16).double().view(16, 1), "special_embeddings.weight": r(2, E),
          "full_rep_embedding.weight": r(cfg.tt_dim, 1)}

    def mlp(prefix, d_in, d_h, d_out, bn, last):
        sd.update({f"{prefix}0.weight": r(d_h, d_in), f"{prefix}0.bias": r(d_h), f"{prefix}{bn}.batch_norm.weight": 1 + 0.1 * r(d_h),
                   f"{prefix}{bn}.batch_norm.bias": 0.1 * r(d_h), f"{prefix}{bn}.batch_norm.running_mean": 0.1 * r(d_h),
                   f"{prefix}{bn}.batch_norm.running_var": 0.5 + torch.rand(d_h, generator=g).double(),
                   f"{prefix}{last}.weight": r(d_out, d_h), f"{prefix}{last}.bias": r(d_out)})
    for v in range(V):
        mlp(f"embedding_layers.{v}.", 2, 5, E, 3, 4)
    mlp("tab_encoder.", DS, 6, E, 3, 4)
    mlp("full_time_embedding.", 1, cfg.d_time_hidden, cfg.tt_dim, 2, 3)
    return cfg, sd


@pytest.mark.parametrize("B,T,V,E", [(1, 1, 1, 4), (3, 5, 4, 8)])
def test_embed_inputs_and_psi_assembly_restatements_equal_build_psi(B, T, V, E):
    g = torch.Generator().manual_seed(B * 100 + T)
    cfg, sd = _tiny_duett(V, T, E, 3, g)
    xs = KR.ssl_like_inputs(B, T, V, g).double()
    xs_static, xs_times = torch.randn(B, 3, generator=g).double(), torch.rand(B, T, generator=g).double()
    psi_ref, _ = duett_ref.build_psi(sd, cfg, xs_static, xs, xs_times, training=False, predict_events=True)
    xin = KR.embed_inputs(xs, sd["n_obs_embedding.weight"])
    var_out = torch.stack([duett_ref.simple_mlp_1hidden(xin[v], sd, f"embedding_layers.{v}.") for v in range(V)])
    tab_out = duett_ref.simple_mlp_1hidden(xs_static, sd, "tab_encoder.")
    assert torch.equal(KR.psi_assemble(xs, var_out, tab_out, sd["special_embeddings.weight"]), psi_ref)
    idx = KR.embed_indices(xs, 16)
    assert torch.equal(xin[..., 1], sd["n_obs_embedding.weight"][idx].squeeze(-1))
    if B * T * V > 8:
        assert int(idx.min()) == 0 and int(idx.max()) == 15


# (G, R, K, N) whose rows-per-chunk x (N + K) floats always fitted the 150-KB budget: the plan, and so every sum's order, is unchanged
FITTING = [(1, 1, 1, 1), (3, 7, 2, 64), (2, 300, 64, 24), (7, 5, 64, 1), (7, 64, 256, 64), (2, 700, 8, 128), (1, 6200, 2, 64), (2, 1100, 256, 64),
           (1, 9, 139, 255), (7, 120, 256, 64), (7, 192, 256, 64), (7, 240, 256, 64), (7, 288, 256, 64), (7, 360, 256, 64), (7, 384, 256, 64),
           (7, 7680, 256, 64), (48, 6208, 2, 64), (48, 6208, 64, 24), (1, 64, 8, 128), (1, 30000, 2, 64)]
REFUSED = [(7, 121, 256, 64), (7, 128, 256, 64), (7, 191, 256, 64), (7, 241, 256, 64), (7, 287, 256, 64), (7, 361, 256, 64), (7, 383, 256, 64),
           (7, 7681, 256, 64), (7, 20000, 256, 64), (1, 100000, 2, 64)]


def test_glinear_bwd_chunk_plan():
    from multimodal_edema_prediction_amd import abi
    L = abi.lib()
    budget_rows = lambda K, N: 150 * 1024 // 4 // (N + K)
    for G, R, K, N in FITTING:
        nc = max(1, min(64, R // 96))
        assert -(-R // nc) <= budget_rows(K, N), (G, R, K, N)                                # the list is what it says it is
        assert L.medp_glinear_bwd_workspace_bytes(G, R, K, N) == KR.glinear_dw_workspace_bytes_before(G, R, K, N), (G, R, K, N)
    for G, R, K, N in REFUSED:
        nc = max(1, min(64, R // 96))
        assert -(-R // nc) > budget_rows(K, N), (G, R, K, N)
        ws = L.medp_glinear_bwd_workspace_bytes(G, R, K, N)
        assert ws > 0 and ws % (G * (N * K + N) * 4) == 0, (G, R, K, N, ws)
        chunks = ws // (G * (N * K + N) * 4)
        assert -(-R // chunks) <= budget_rows(K, N), (G, R, K, N, chunks)                   # every chunk's dy and x rows fit LDS
        assert chunks <= -(-R // budget_rows(K, N)), (G, R, K, N, chunks)                   # and no more chunks than that takes
    assert L.medp_glinear_bwd_workspace_bytes(0, 5, 2, 2) == 0 and L.medp_glinear_bwd_workspace_bytes(1, 5, 0, 2) == 0
