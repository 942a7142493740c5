"""The fused DuETT front end (csrc/duett_embed.hip, csrc/duett.hip): `medp_duett_embed_fwd` — psi built directly in the event view with the event
embedding added and the first ScaleNorm applied, and the time embedding — and `medp_duett_swap_add_norm` (axis swap + positional
add + the next encoder's ScaleNorm in one pass), against the CPU oracle (oracle/duett_ref.py, pinned by the reference's fixtures)
and against the separate launches they replace (bit-identical ScaleNorm)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from multimodal_edema_prediction_amd import functional as Fn  # noqa: E402
from multimodal_edema_prediction_amd.abi import check, lib, ptr, stream  # noqa: E402

DEV = "cuda"


@pytest.mark.parametrize("B,T,V", [(8, 32, 16), (5, 96, 48)])
def test_embed_stage_against_oracle(B, T, V):
    from multimodal_edema_prediction_amd.cohort import CohortCfg, make_batch
    from multimodal_edema_prediction_amd.main_architecture_duett import load_duett_backbone
    from oracle import duett_ref
    DS, E = 8, 24
    torch.manual_seed(0)
    m = load_duett_backbone("synthetic", d_static_num=DS, d_time_series_num=V, n_timesteps=T, freeze=True)
    with torch.no_grad():                                   # non-trivial BatchNorm statistics and norm gains
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
        m.event_transformers[0].layers[0][0][0].g.fill_(1.3)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    batch = make_batch(CohortCfg(n_timesteps=T, n_vars=V, d_static=DS, image_size=32), 7, B, mode="student")
    x = (batch["x_ts"], batch["x_static"], list(batch["bin_ends"]))
    xin = duett_ref.feats_to_input(x, max_len=T)
    _, inter = duett_ref.encode(sd, duett_ref.DuettCfg(d_static_num=DS, d_time_series_num=V, n_timesteps=T), xin, return_intermediates=True)
    psi0, temb_ref = inter["psi0"], inter["time_emb"]                                   # [B,T+1,V+1,E], [B,T+1,(V+1)E]
    xe_ref = psi0.transpose(1, 2).flatten(2) + sd["full_event_embedding.weight"]          # model :80
    g = sd["event_transformers.0.layers.0.0.0.g"]
    h_ref = torch.nn.functional.normalize(xe_ref, dim=-1) * xe_ref.shape[-1] ** 0.5 * g

    xs_static, xs_ts, xs_times, _ = m.feats_to_input(x, B)
    w = m._prepare()[0]
    T1, V1 = T + 1, V + 1
    xe = torch.empty((B, V1, T1 * E), device=DEV)
    h = torch.empty((B, V1, T1 * E), device=DEV, dtype=torch.bfloat16)
    temb = torch.empty((B, T1, V1 * E), device=DEV)
    p0 = torch.empty((B, T1, V1, E), device=DEV)
    tab = torch.empty((B, E), device=DEV)
    check(lib().medp_duett_embed_fwd(ctypes.byref(w), ptr(xs_static), ptr(xs_ts), ptr(xs_times), B, T, ptr(xe), ptr(h), ptr(temb), ptr(p0),
                                     ptr(tab), 3, stream()), "duett_embed_fwd")
    assert float((p0.cpu() - psi0).abs().max()) < 2e-5
    assert float((xe.cpu() - xe_ref).abs().max()) < 2e-5
    assert float((temb.cpu() - temb_ref).abs().max()) < 2e-5
    assert float((h.float().cpu() - h_ref).abs().max()) < 8e-3 * float(h_ref.abs().max())            # bf16 output
    assert torch.equal(h, Fn.scalenorm(xe, m.event_transformers[0].layers[0][0][0].g))               # == the separate launch, bit for bit


def _eval_backbone(T, V, DS=8):
    """The synthetic frozen backbone in eval() with non-trivial BatchNorm running statistics: (module on the GPU, CPU state dict)."""
    from multimodal_edema_prediction_amd.main_architecture_duett import load_duett_backbone
    m = load_duett_backbone("synthetic", d_static_num=DS, d_time_series_num=V, n_timesteps=T, freeze=True)
    with torch.no_grad():
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
        m.event_transformers[0].layers[0][0][0].g.fill_(1.3)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _ssl_like_batch(B, T, V, DS=8):
    """kernel_refs.ssl_like_inputs with a static vector and bin times; asserts that the batch holds what the REP-row rule is about:
    a (b, v) whose count is -1 at t = 0 while timestep 0 itself is not masked.  Returns (xs_static, xs_ts, xs_times, such (b, v))."""
    import kernel_refs as KR
    g = torch.Generator().manual_seed(100 * T + V)
    xs_ts = KR.ssl_like_inputs(B, T, V, g)
    hit = ((xs_ts[:, 0, V:2 * V] == -1) & (xs_ts[:, 0, 2 * V] != 1).unsqueeze(1)).nonzero()
    assert len(hit) > 0, "no event masked at t = 0 under an unmasked timestep 0: the REP-row rule would go untested"
    return torch.randn(B, DS, generator=g), xs_ts, torch.rand(B, T, generator=g) * 4, hit


@pytest.mark.parametrize("B,T,V", [(3, 5, 4), (2, 70, 3), (2, 140, 3)])          # one, two and three passes of the 64-lane cell loop
def test_embed_stage_against_oracle_with_masked_events(B, T, V, request):
    """The embed kernel on an SSL-like batch (masked events, one of them at every step; masked timesteps, step 0 among them; a
    variable masked at step 0 only) against oracle/duett_ref.build_psi with predict_events.  The reference extends the event mask to
    the REP row with timestep 0's mask, so a variable whose count is -1 at t = 0 carries special[0] in the REP row, not special[1]:
    every overridden cell must be bit-equal to its special row, in the matrix-core and in the VALU form.  (The embed kernel's own copy
    of the rule wrote special[1] into every REP cell: 2 or 3 cells off per shape, |psi0 - oracle| up to 3.2.)"""
    from oracle import duett_ref
    E = 24
    torch.manual_seed(T)
    m, sd = _eval_backbone(T, V)
    xs_static, xs_ts, xs_times, hit = _ssl_like_batch(B, T, V)
    cfg = duett_ref.DuettCfg(d_static_num=xs_static.shape[1], d_time_series_num=V, n_timesteps=T)
    psi0, temb_ref = duett_ref.build_psi(sd, cfg, xs_static, xs_ts, xs_times, training=False, predict_events=True)
    special = sd["special_embeddings.weight"]
    assert not torch.equal(special[0], special[1])
    for b, v in hit.tolist():                                  # not vacuous: the oracle's REP cell there is the MASKED embedding
        assert torch.equal(psi0[b, T, v], special[0]) and not torch.equal(psi0[b, T, v], special[1])
    # the override masks, as build_psi forms them
    ev = torch.cat((xs_ts[:, :, V:2 * V] == -1, torch.zeros((B, T, 1), dtype=torch.bool)), dim=2)
    masked = torch.cat((ev, ev[:, :1, :]), dim=1) | torch.cat((xs_ts[:, :, -1] == 1, torch.zeros((B, 1), dtype=torch.bool)), dim=1).unsqueeze(2)
    rep = ~masked
    rep[:, :T] = False
    xe_ref = psi0.transpose(1, 2).flatten(2) + sd["full_event_embedding.weight"]          # model :80
    h_ref = torch.nn.functional.normalize(xe_ref, dim=-1) * xe_ref.shape[-1] ** 0.5 * sd["event_transformers.0.layers.0.0.0.g"]

    w = m._prepare()[0]
    T1, V1 = T + 1, V + 1
    dev = [t.to(DEV) for t in (xs_static, xs_ts, xs_times)]
    L = lib()
    prev = L.medp_dbg_embed_mfma(1)
    request.addfinalizer(lambda: L.medp_dbg_embed_mfma(prev))
    for form in (1, 0):
        L.medp_dbg_embed_mfma(form)
        xe = torch.full((B, V1, T1 * E), float("nan"), device=DEV)
        h = torch.zeros((B, V1, T1 * E), device=DEV, dtype=torch.bfloat16)
        temb = torch.full((B, T1, V1 * E), float("nan"), device=DEV)
        p0 = torch.full((B, T1, V1, E), float("nan"), device=DEV)
        tab = torch.empty((B, E), device=DEV)
        check(L.medp_duett_embed_fwd(ctypes.byref(w), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), B, T, ptr(xe), ptr(h), ptr(temb), ptr(p0), ptr(tab),
                                     3, stream()), "duett_embed_fwd")
        p0c = p0.cpu()
        print(f"form {form}: psi0 {float((p0c - psi0).abs().max()):.3e}  xe {float((xe.cpu() - xe_ref).abs().max()):.3e}  "
              f"masked cells off {int((p0c[masked] != special[0]).any(-1).sum())} of {int(masked.sum())}  "
              f"REP cells off {int((p0c[rep] != special[1]).any(-1).sum())} of {int(rep.sum())}")
        assert float((p0c - psi0).abs().max()) < 2e-5, form
        assert torch.equal(p0c[masked], special[0].expand(int(masked.sum()), E)), form
        assert torch.equal(p0c[rep], special[1].expand(int(rep.sum()), E)), form
        assert float((xe.cpu() - xe_ref).abs().max()) < 2e-5, form
        assert float((temb.cpu() - temb_ref).abs().max()) < 2e-5, form
        assert float((h.float().cpu() - h_ref).abs().max()) < 8e-3 * float(h_ref.abs().max()), form      # bf16 output
        assert torch.equal(h, Fn.scalenorm(xe, m.event_transformers[0].layers[0][0][0].g)), form         # == the separate launch, bit for bit


def test_inference_and_training_forms_agree_on_masked_events():
    """`_encode_inference` (one C call, the embed kernel) and `encode_training` (op-level form, psi_assemble) on one frozen eval()
    backbone and one SSL-like batch: the same tokens, within the bound the suite puts on either form against the reference's eval-mode
    encode (test_gpu_model.py, test_gpu_student.py: 3e-2).  Before the embed kernel took the shared cell rule this failed at the REP
    row: a variable whose count is -1 at t = 0 got special[1] there from the inference form and special[0] from the training form
    (measured on that commit: max 4.9e-1, all of it in the REP row; 5.8e-3 with the shared rule)."""
    from multimodal_edema_prediction_amd.duett_train import encode_training
    B, T, V = 3, 5, 4
    torch.manual_seed(5)
    m, _ = _eval_backbone(T, V)
    xs_static, xs_ts, xs_times, _ = _ssl_like_batch(B, T, V)
    xin = (xs_static.to(DEV), xs_ts.to(DEV), xs_times.to(DEV), [T] * B)
    with torch.no_grad():
        inf = m._encode_inference(xin)[0]
        trn = encode_training(m, xin)
    err = (inf - trn).abs()
    print(f"inference vs training form: max {float(err.max()):.3e} (REP row {float(err[:, T].max()):.3e}), mean {float(err.mean()):.3e}")
    assert float(err.max()) < 3e-2


@pytest.mark.parametrize("B,T,V", [(8, 32, 16), (6, 96, 48), (2, 140, 20)])
def test_embed_stage_mfma_form_is_bit_identical_to_the_valu_form(B, T, V, request):
    """The psi / time embeddings on the matrix cores in exact fp32 (`v_mfma_f32_16x16x4_f32`: a k-ordered fmaf chain) against the
    VALU kernels they replace: every output element bit for bit — psi0, the event-view rows, their bf16 ScaleNorm, the time
    embedding — on batches with masked time steps, masked events (SSL), over-length rows (T + 1 > 128: several passes of the cell
    loop) and the REP row.  So the fp32 kernel mode needs no second form (medp_dbg_embed_mfma switches at run time)."""
    from multimodal_edema_prediction_amd.main_architecture_duett import load_duett_backbone
    DS, E = 8, 24
    torch.manual_seed(3)
    m = load_duett_backbone("synthetic", d_static_num=DS, d_time_series_num=V, n_timesteps=T, freeze=True)
    with torch.no_grad():
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand_like(b))
    m = m.to(DEV)
    g = torch.Generator().manual_seed(11)
    obs = torch.rand(B, T, V, generator=g) < 0.3
    xs_ts = torch.zeros(B, T, 2 * V + 1)
    xs_ts[:, :, :V] = torch.randn(B, T, V, generator=g) * obs
    xs_ts[:, :, V:2 * V] = obs.float() * torch.randint(1, 20, (B, T, V), generator=g).float()      # counts above the table: clipped
    xs_ts[:, :, V:2 * V][torch.rand(B, T, V, generator=g) < 0.05] = -1.0                            # masked events (SSL)
    xs_ts[:, :, 2 * V] = (torch.rand(B, T, generator=g) < 0.15).float()                            # masked time steps
    xs_ts[0, :, 2 * V] = 1.0                                                                         # a sample with every step masked
    xs_ts[1, 0, V], xs_ts[1, 0, 2 * V] = -1.0, 0.0                                                   # an event masked at t = 0: its REP cell is special[0]
    xs_static, xs_times = torch.randn(B, DS, generator=g), torch.rand(B, T, generator=g) * 4
    xs_ts, xs_static, xs_times = xs_ts.to(DEV), xs_static.to(DEV), xs_times.to(DEV)
    w = m._prepare()[0]
    T1, V1 = T + 1, V + 1
    L = lib()
    prev = L.medp_dbg_embed_mfma(1)
    request.addfinalizer(lambda: L.medp_dbg_embed_mfma(prev))

    def run(on):
        L.medp_dbg_embed_mfma(on)
        xe = torch.full((B, V1, T1 * E), float("nan"), device=DEV)
        h = torch.zeros((B, V1, T1 * E), device=DEV, dtype=torch.bfloat16)
        temb = torch.full((B, T1, V1 * E), float("nan"), device=DEV)
        p0 = torch.full((B, T1, V1, E), float("nan"), device=DEV)
        tab = torch.empty((B, E), device=DEV)
        check(L.medp_duett_embed_fwd(ctypes.byref(w), ptr(xs_static), ptr(xs_ts), ptr(xs_times), B, T, ptr(xe), ptr(h), ptr(temb), ptr(p0),
                                     ptr(tab), 3, stream()), "duett_embed_fwd")
        torch.cuda.synchronize()
        return xe, h, temb, p0

    a, b_ = run(1), run(0)
    for name, x, y in zip(("xe", "h", "temb", "psi0"), a, b_):
        assert not torch.isnan(x.float()).any(), name
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ, max {float((x.float() - y.float()).abs().max()):.3e}"


@pytest.mark.parametrize("B,A1,A2", [(3, 33, 17), (4, 97, 49), (2, 49, 97), (1, 257, 97)])
@pytest.mark.parametrize("pending_norm,batched_add", [(False, False), (True, True)])
def test_swap_add_norm(B, A1, A2, pending_norm, batched_add):
    E = 24
    g0 = torch.Generator().manual_seed(B * 1000 + A1)
    x = torch.randn(B, A1, A2, E, generator=g0)
    rn = (0.5 + torch.rand(B * A1, generator=g0)) if pending_norm else None
    gp, gn = torch.tensor([1.2]), torch.tensor([0.8])
    add = torch.randn((B, A2, A1, E) if batched_add else (A2, A1, E), generator=g0)
    sc = (rn.view(B, A1, 1, 1) * ((A2 * E) ** 0.5 * gp)) if pending_norm else 1.0
    x_ref = (x * sc).transpose(1, 2) + add                                             # [B, A2, A1, E]
    xo = torch.empty((B, A2, A1 * E), device=DEV)
    ho = torch.empty((B, A2, A1 * E), device=DEV, dtype=torch.bfloat16)
    xd, rd, gpd, ad, gnd = x.to(DEV), (rn.to(DEV) if pending_norm else None), gp.to(DEV), add.to(DEV), gn.to(DEV)   # kept alive past the launch
    check(lib().medp_duett_swap_add_norm(ptr(xd), ptr(rd), ptr(gpd), ptr(ad), A2 * A1 * E if batched_add else 0, ptr(gnd), 1e-12, ptr(xo),
                                         ptr(ho), B, A1, A2, E, stream()), "swap_add_norm")
    ref = x_ref.reshape(B, A2, A1 * E)
    assert float((xo.cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-6
    assert torch.equal(ho, Fn.scalenorm(xo, gnd))                               # the fused norm == medp_scalenorm_fwd of its x


@pytest.mark.parametrize("B,N,H,dh", [(3, 17, 2, 12), (2, 33, 2, 12), (4, 49, 2, 12), (5, 97, 2, 12), (2, 257, 2, 12), (2, 100, 3, 16), (1, 16, 1, 4)])
def test_attn_dh16_mfma_forward(B, N, H, dh):
    """DuETT's attention on the matrix cores (medp_attn_dh16_fwd) against an fp64 softmax(QK^T/sqrt(dh))V on the same bf16-rounded
    operands (tolerance: bf16 probabilities and output, 8e-3 of the output range) and against the fp32 VALU kernel it replaces."""
    D = H * dh
    g0 = torch.Generator().manual_seed(N)
    qkv = torch.randn(B, N, 3 * D, generator=g0) * 1.5
    qd = qkv.to(DEV)
    o = torch.full((B, N, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    rc = lib().medp_attn_dh16_fwd(ptr(qd), 3 * D, ptr(o), D, B, N, H, dh, dh ** -0.5, stream())
    check(rc, "attn_dh16_fwd")
    r = qkv.to(torch.bfloat16).double().view(B, N, 3, H, dh)
    q, k, v = r[:, :, 0].transpose(1, 2), r[:, :, 1].transpose(1, 2), r[:, :, 2].transpose(1, 2)
    want = (torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v).transpose(1, 2).reshape(B, N, D)
    got = o.float().cpu().double()
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) < 8e-3 * max(1.0, float(want.abs().max()))
    old = Fn.attn_small_fwd(qd[..., :D], qd[..., D:2 * D], qd[..., 2 * D:], B, N, N, H, dh, dh ** -0.5, q_batch_stride=N * 3 * D,
                            kv_batch_stride=N * 3 * D, out_dtype=torch.bfloat16)
    assert float((old.float() - o.float()).abs().max()) < 3e-2 * max(1.0, float(want.abs().max()))
    assert lib().medp_attn_dh16_fwd(ptr(qd), 3 * D, ptr(o), D, B, N, H, 20, 0.2, stream()) == -2          # not built: caller falls back
