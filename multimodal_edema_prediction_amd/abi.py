"""ctypes binding of the C ABI declared in include/medp_hip.h (libmedp_hip.so, built in-tree by build.py).

The product path has NO fallback: if the library is missing or a tensor is not on the GPU the call raises.
Error mapping: rc < 0 (invalid argument) -> ValueError, rc > 0 (hipError_t) -> RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEDP_HIP_LIB") or os.path.join(_HERE, "libmedp_hip.so")   # override: the -DMEDP_V7_PHASE_TRACE profiling build

ABI_VERSION = 4      # medp_version() of the library these struct layouts belong to (csrc/api.cpp)

P, I, F, U, LL, SZ = c_void_p, c_int, c_float, c_uint, c_longlong, c_size_t


class MedpVitLayer(ctypes.Structure):
    _fields_ = [(n, P) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b",
                                 "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2")]


class MedpVitWeights(ctypes.Structure):
    _fields_ = ([(n, I) for n in ("hidden", "n_layers", "n_heads", "mlp_hidden", "patch", "pos_side", "patch_kpad")]
                + [("ln_eps", F)]
                + [(n, P) for n in ("patch_w", "patch_b", "cls", "pos", "final_ln_w", "final_ln_b")]
                + [("layers", ctypes.POINTER(MedpVitLayer))])


class MedpEncoderWeights(ctypes.Structure):
    """One x_transformers-style encoder (depth 1): see include/medp_hip.h"""
    _fields_ = [(n, P) for n in ("g_attn", "qkv_w", "out_w", "g_ff", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "g_final")]


class MedpDuettWeights(ctypes.Structure):
    _fields_ = ([(n, I) for n in ("n_vars", "n_static", "d_embedding", "n_heads", "n_layers", "d_ff", "d_hidden_embed",
                                  "d_hidden_tab", "d_hidden_time", "n_obs_rows", "final_norm")]
                + [("norm_eps", F)]
                + [(n, P) for n in ("emb_b4", "emb_l0", "emb_w4t", "n_obs_table",
                                    "tab_w0", "tab_b0", "tab_bn_scale", "tab_bn_shift", "tab_w4", "tab_b4", "special",
                                    "time_w0", "time_b0", "time_bn_scale", "time_bn_shift", "time_w3t", "time_b3",
                                    "rep_embedding", "event_embedding")]
                + [("event_enc", ctypes.POINTER(MedpEncoderWeights)), ("time_enc", ctypes.POINTER(MedpEncoderWeights))])


class MedpAdamTensor(ctypes.Structure):
    _fields_ = [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("numel", LL), ("lr", F), ("weight_decay", F)]


class MedpOperandJob(ctypes.Structure):
    _fields_ = [("src", P), ("dst_plain", P), ("dst_t", P), ("rows", I), ("cols", I), ("ld_src", I), ("ld_plain", I), ("ld_t", I),
                ("reserved_", I)]


class MedpProbeProblem(ctypes.Structure):
    """One problem of the conditional-information probe's table (include/medp_hip.h)."""
    _fields_ = [("col_off", LL), ("row_off", LL), ("n_rows", I), ("F", I), ("y_col", I), ("j0", I), ("j1", I), ("reserved_", I)]


class MedpHeadProblem(ctypes.Structure):
    """One problem of the linear-head trainer's table (include/medp_hip.h)."""
    _fields_ = ([(n, P) for n in ("X", "Y", "M", "W", "b", "mW", "vW", "mb", "vb", "t", "perm", "loss_out")] + [("ldx", LL)]
                + [(n, I) for n in ("N", "ldy", "col0", "F", "L", "label_width", "bs", "S")]
                + [(n, c_double) for n in ("lr", "weight_decay", "beta1", "beta2", "eps")]
                + [("dropout_p", F), ("seed", U), ("stream_id", U), ("reserved_", I)])


class MedpPoolHeadProblem(ctypes.Structure):
    """The attention-pooled head's problem (include/medp_hip.h)."""
    _fields_ = ([(n, P) for n in ("X", "Y", "M", "q", "W", "b", "mq", "vq", "mW", "vW", "mb", "vb", "perm", "ws", "loss_out")]
                + [(n, I) for n in ("N", "T", "d", "L", "ldy", "bs", "S", "step0")]
                + [(n, c_double) for n in ("lr", "weight_decay", "beta1", "beta2", "eps")]
                + [("dropout_p", F), ("seed", U), ("stream_id", U), ("reserved_", I)])


class MedpMlpHeadProblem(ctypes.Structure):
    """One problem of the MLP fusion head's table (include/medp_hip.h)."""
    _fields_ = ([(n, P) for n in ("X", "Y", "M", "W1", "b1", "W2", "b2", "mom", "t", "perm", "perm_host", "loss_out")] + [("ldx", LL)]
                + [(n, I) for n in ("N", "ldy", "col0", "K", "H", "L", "bs", "S", "reserved0_")]
                + [(n, c_double) for n in ("lr", "weight_decay", "beta1", "beta2", "eps")]
                + [("dropout_p", F), ("seed", U), ("stream_id", U), ("reserved_", I)])


# name -> (restype, argtypes); must list every function declared in include/medp_hip.h (tests/test_abi.py checks)
SIGNATURES = {
    "medp_last_error": (c_char_p, []),
    "medp_version": (I, []),
    "medp_arch": (c_char_p, []),
    "medp_gemm_bf16_nt": (I, [P, P, P, I, I, I, I, I, I, P, P, P, I, I, I, P]),
    "medp_gemm_nt_workspace_bytes": (SZ, [I, I, I]),
    "medp_gemm_bf16_nt_ws": (I, [P, P, P, I, I, I, I, I, I, P, P, P, I, I, I, P, SZ, P]),
    "medp_gemm_f32_nt": (I, [P, P, P, I, I, I, I, I, I, P, P, P, I, I, P]),
    "medp_gemm_f32_tn": (I, [P, P, P, I, I, I, I, I, P]),
    "medp_gemm_tn_workspace_bytes": (SZ, [I, I, I]),
    "medp_gemm_bf16_tn": (I, [P, P, P, I, I, I, I, I, P, P]),
    "medp_gemm_persistent_cap": (I, [I]),
    "medp_gemm_profile_enable": (I, [I]),
    "medp_gemm_profile_collect": (I, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_longlong), ctypes.POINTER(ctypes.c_double)]),
    "medp_attn_fwd_dh64": (I, [P, P, P, P, I, I, I, I, I, I, I, F, P]),
    "medp_attn_dh16_fwd": (I, [P, I, P, I, I, I, I, I, F, P]),
    "medp_attn_dh16_train_supported": (I, [I, I, I, I, I, I]),
    "medp_attn_dh16_train_fwd": (I, [P, I, P, I, P, I, I, I, I, I, F, F, U, U, P]),
    "medp_attn_dh16_train_bwd": (I, [P, I, P, I, P, P, P, I, I, I, I, I, I, F, F, U, U, P]),
    "medp_attn_fwd_dh64_lse": (I, [P, P, P, P, P, I, I, I, I, I, I, I, F, P]),
    "medp_attn_bwd_dh64_prep": (I, [P, I, P, I, P, I, P, I, I, I, P]),
    "medp_attn_bwd_dh64": (I, [P, P, P, I, P, I, P, P, P, P, P, I, I, I, I, F, P]),
    "medp_attn_small_fwd": (I, [P, I, LL, P, P, I, LL, P, I, I, P, I, I, I, I, I, F, F, U, U, P]),
    "medp_attn_small_bwd": (I, [P, I, P, I, LL, P, P, I, LL, P, I, P, I, P, I, LL, I, I, I, I, I, F, F, U, U, P]),
    "medp_attn_small_masked_fwd": (I, [P, I, LL, P, P, I, LL, P, I, I, P, I, I, I, I, I, F, F, U, U, P, P, LL]),
    "medp_attn_small_masked_bwd": (I, [P, I, P, I, LL, P, P, I, LL, P, I, P, I, P, I, LL, I, I, I, I, I, F, F, U, U, P, P, LL]),
    "medp_attn_fq_split_ws_bytes": (SZ, [I, I, I, I, I]),
    "medp_attn_fq_split_fwd": (I, [P, I, LL, P, P, I, LL, P, I, I, P, P, P, SZ, I, I, I, I, I, F, F, U, U, P]),
    "medp_attn_fq_split_bwd": (I, [P, I, P, I, P, P, I, LL, P, P, I, LL, P, I, P, P, I, LL, P, SZ, I, I, I, I, I, F, F, U, U, P]),
    "medp_layernorm_fwd": (I, [P, I, P, P, P, I, I, P, P, I, I, F, P]),
    "medp_colsum_workspace_bytes": (SZ, [I, I]),
    "medp_layernorm_bwd": (I, [P, I, P, I, P, P, P, P, I, I, P, P, P, I, I, P]),
    "medp_colsum_f32": (I, [P, I, P, P, I, I, P]),
    "medp_scalenorm_fwd": (I, [P, I, P, P, I, I, P, I, I, F, P]),
    "medp_scalenorm_bwd": (I, [P, I, P, I, P, P, P, I, I, P, P, I, I, P]),
    "medp_scalenorm_bwd_add": (I, [P, I, P, I, P, P, P, I, P, I, P, P, I, I, P]),
    "medp_cast_f32_bf16": (I, [P, I, P, I, I, I, P]),
    "medp_transpose_to_bf16": (I, [P, I, I, P, I, I, I, P]),
    "medp_weight_operands_multi": (I, [P, P, P, I, P]),
    "medp_gelu_bwd": (I, [P, P, P, LL, P]),
    "medp_gelu_bf16_fwd": (I, [P, P, LL, P]),
    "medp_gelu_bf16_bwd": (I, [P, P, P, LL, P]),
    "medp_im2col_patch": (I, [P, P, I, I, I, I, I, I, P]),
    "medp_vit_assemble": (I, [P, P, P, P, I, I, I, P]),
    "medp_pos_embed_bicubic": (I, [P, P, I, I, I, I, P]),
    "medp_pos_embed_bicubic_bwd": (I, [P, P, I, I, I, I, P]),
    "medp_vit_workspace_bytes": (SZ, [ctypes.POINTER(MedpVitWeights), I, I, I]),
    "medp_vit_forward": (I, [ctypes.POINTER(MedpVitWeights), P, I, I, I, P, P, P, SZ, P]),
    "medp_vit_forward_part": (I, [ctypes.POINTER(MedpVitWeights), P, I, I, I, P, P, P, SZ, I, I, P]),
    "medp_duett_embed_fwd": (I, [ctypes.POINTER(MedpDuettWeights), P, P, P, I, I, P, P, P, P, P, I, P]),
    "medp_duett_swap_add_norm": (I, [P, P, P, P, LL, P, F, P, P, I, I, I, I, P]),
    "medp_feats_to_input": (I, [P, P, LL, P, P, LL, P, I, P, P, P, P, I, I, I, I, I, F, F, U, U, P]),
    "medp_ssl_mask_batch": (I, [P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "medp_duett_workspace_bytes": (SZ, [ctypes.POINTER(MedpDuettWeights), I, I]),
    "medp_duett_encode": (I, [ctypes.POINTER(MedpDuettWeights), P, P, P, I, I, P, P, P, P, SZ, P]),
    "medp_gelu_dropout_fwd": (I, [P, P, LL, F, U, U, P]),
    "medp_gelu_dropout_bwd": (I, [P, P, P, LL, F, U, U, P]),
    "medp_gelu_dropout_fwd_bf16": (I, [P, P, LL, F, U, U, P]),
    "medp_gelu_dropout_bwd_bf16": (I, [P, P, P, P, LL, F, U, U, P]),
    "medp_dropout_add": (I, [P, P, P, LL, F, U, U, P]),
    "medp_rowdot_fwd": (I, [P, I, P, P, P, I, I, P]),
    "medp_rowdot_bwd": (I, [P, P, I, P, P, P, P, I, I, P]),
    "medp_fusion_logits_fwd": (I, [P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "medp_fusion_logits_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, P, I, I, P]),
    "medp_meanpool_fwd": (I, [P, P, I, I, I, I, P]),
    "medp_meanpool_bwd": (I, [P, P, I, I, I, I, P]),
    "medp_dual_pathology_loss": (I, [P, P, P, P, P, P, P, F, F, F, F, P, P, P, P, I, I, P]),
    "medp_student_kd_loss": (I, [P, P, P, F, F, F, P, P, I, P]),
    "medp_aux_residual_kl": (I, [P, P, P, P, F, P, P, I, P]),
    "medp_sq_mean": (I, [P, F, P, P, I, P]),
    "medp_masked_bce_global": (I, [P, P, P, P, P, I, P]),
    "medp_glinear_fwd": (I, [P, P, P, P, I, I, I, I, P]),
    "medp_glinear_bwd_workspace_bytes": (SZ, [I, I, I, I]),
    "medp_glinear_bwd": (I, [P, P, P, P, P, P, P, I, I, I, I, P]),
    "medp_gmlp_supported": (I, [I, I, I]),
    "medp_gmlp_workspace_bytes": (SZ, [I, I, I, I, I]),
    "medp_gmlp_fwd": (I, [P] * 12 + [I, I, I, I, I, F, F, I, P, P]),
    "medp_gmlp_bwd": (I, [P] * 16 + [I, I, I, I, I, F, I, P, P]),
    "medp_gbn_workspace_bytes": (SZ, [I, I, I]),
    "medp_gbn_fwd": (I, [P, P, P, P, P, P, P, P, I, I, I, F, F, I, P, P]),
    "medp_gbn_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, F, I, P, P]),
    "medp_act_fwd": (I, [P, P, LL, I, P]),
    "medp_act_bwd": (I, [P, P, P, LL, I, P]),
    "medp_embed_inputs_fwd": (I, [P, P, I, P, I, I, I, I, P]),
    "medp_embed_inputs_bwd_blocks": (I, [I, I, I]),
    "medp_embed_inputs_bwd": (I, [P, P, P, I, I, I, I, I, P]),
    "medp_psi_assemble_fwd": (I, [P, P, P, P, P, I, I, I, I, P]),
    "medp_psi_assemble_bwd_slices": (I, [I, I, I]),
    "medp_psi_assemble_bwd": (I, [P, P, P, P, P, I, I, I, I, P]),
    "medp_axis_swap": (I, [P, P, I, I, I, I, P]),
    "medp_axis_swap_add": (I, [P, P, P, P, I, I, I, I, I, P]),
    "medp_add_bcast": (I, [P, P, P, LL, I, I, P]),
    "medp_masked_mse": (I, [P, P, P, P, P, I, P]),
    "medp_bce_mean": (I, [P, P, P, P, P, I, P]),
    "medp_adamw_chunk_elems": (I, []),
    "medp_adamw_multi": (I, [P, P, P, I, F, F, F, I, P, F, P]),
    "medp_grad_sumsq_multi": (I, [P, P, P, I, P, F, P, P]),
    "medp_adamw_multi_dscale": (I, [P, P, P, I, F, F, F, I, P, P, P]),
    "medp_traj_features": (I, [P, P, I, I, I, P]),
    "medp_gru_fwd": (I, [P, P, P, P, P, P, I, I, I, P]),
    "medp_gru_fwd_f32": (I, [P, P, I, P, P, P, P, I, I, I, P]),
    "medp_gru_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, P]),
    "medp_gru_fwd_h16": (I, [P, P, P, P, P, P, P, F, U, U, I, I, I, P]),
    "medp_gru_bwd_dgi16": (I, [P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "medp_raw_traj_summary": (I, [P, P, I, I, I, I, P]),
    "medp_offset_logistic_ws_bytes": (SZ, [I, I, I]),
    "medp_offset_logistic_valgrad": (I, [P, LL, P, P, P, P, P, P, P, SZ, I, I, I, P]),
    "medp_resampled_binary_metrics": (I, [P, P, P, P, P, I, I, I, I, P]),
    "medp_counterfactual_feats": (I, [P, P, LL, P, P, LL, P, I, P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "medp_temporal_usage_summary": (I, [P, P, P, P, P, P, I, I, I, I, P]),
    "medp_youden_thresholds": (I, [P, P, P, P, P, P, I, I, I, P]),
    "medp_complementarity_cells": (I, [P, P, P, P, P, I, I, P]),
    "medp_trajectory_cells": (I, [P, I, I, I, I, I, LL, P, P, P, P, P, P, P, P]),
    "medp_column_medians": (I, [P, LL, I, I, I, I, P, P, P]),
    "medp_probe_moments": (I, [P, LL, I, P, P, P, LL, P, P, I, I, P]),
    "medp_probe_terms_ws_bytes": (SZ, [I, I, I, LL]),
    "medp_logistic_newton_terms": (I, [P, LL, I, P, I, P, P, P, LL, P, P, P, P, P, P, P, P, SZ, I, I, P]),
    "medp_probe_scores": (I, [P, LL, I, P, P, P, LL, P, P, P, P, I, I, I, P]),
    "medp_head_train_onchip": (I, [I, I, I, I]),
    "medp_head_train_epoch": (I, [P, P, I, P]),
    "medp_head_scores": (I, [P, LL, I, I, I, I, I, P, P, P, I, P, P, P]),
    "medp_pool_head_rows_onchip": (I, [I, I]),
    "medp_pool_head_ws_bytes": (SZ, [I, I, I]),
    "medp_pool_head_train_epoch": (I, [P, P, P]),
    "medp_pool_head_scores": (I, [P, I, I, I, I, P, P, P, P, I, P, P, P]),
    "medp_mlp_head_supported": (I, [I, I, I, I]),
    "medp_mlp_head_train_epoch": (I, [P, P, I, P]),
    "medp_mlp_head_scores": (I, [P, LL, I, I, I, I, I, P, P, P, P, P, I, P, P, P]),
    "medp_grad_flow_state_doubles": (SZ, [I, I]),
    "medp_grad_flow_ws_doubles": (SZ, [I, I]),
    "medp_grad_flow_seeds": (I, [P, P, P, P, P, P, P, F, P, P, P, P, P, I, I, P]),
    "medp_grad_flow_accumulate": (I, [P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "medp_grad_flow_report": (I, [P, c_double, c_double, c_double, P, I, I, P]),
    "medp_query_geometry": (I, [P, P, I, I, P]),
    "medp_rng_set_epoch_ptr": (I, [P]),
    "medp_counter_advance": (I, [P, P]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load libmedp_hip.so; raise (never fall back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"HIP extension {LIB_PATH} is missing: build it with `python -m multimodal_edema_prediction_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        built = L.medp_version()
        if built != ABI_VERSION:      # another layout of the weight structs: its kernels would walk them at the wrong stride
            raise RuntimeError(
                f"{LIB_PATH} has ABI version {built}, this package expects {ABI_VERSION}: rebuild it with "
                "`python -m multimodal_edema_prediction_amd.build --force` (`--trace` / `--ablate` for the variant libraries).")
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc == 0:
        return
    msg = lib().medp_last_error().decode("utf-8", "replace")
    if rc < 0:
        raise ValueError(f"{what}: {msg}" if what else msg)
    raise RuntimeError(f"{what}: HIP error {rc}: {msg}")


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libmedp_hip operates on GPU memory only (tensor is on %s); there is no CPU fallback" % t.device)
    return t.data_ptr()


def fp32_matrix(X: torch.Tensor, what: str):
    """fp32 [N, ...] -> (contiguous tensor, N, row stride in elements) for the kernels that take a row-major matrix."""
    if X.dtype != torch.float32:
        raise TypeError(f"{what}: the probe kernels read fp32")
    X = X.contiguous()
    return X, X.shape[0], X.numel() // max(X.shape[0], 1)


def table_bytes(host_array, count: int) -> np.ndarray:
    """The first `count` entries of a ctypes problem table as a uint8 numpy copy (what goes to the device)."""
    return np.frombuffer(host_array, dtype=np.uint8, count=ctypes.sizeof(host_array._type_) * count).copy()


def require_gpu() -> None:
    lib()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device is visible: the MI355X hot path cannot run (there is no CPU fallback)")
