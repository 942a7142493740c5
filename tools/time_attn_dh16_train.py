#!/usr/bin/env python3
"""DuETT's attention at the student step's shapes (B 64: the event-axis encoder attends over 49 tokens, the time-axis encoder over 97;
2 heads of 12), isolated launches: the training-form MFMA kernels (attention_dh16.hip) against the fp32 VALU kernels (attention_small.hip),
and the inference form of the same file."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multimodal_edema_prediction_amd import functional as Fn
from tools.bench_kernels import timeit
H, dh = 2, 12
D = H * dh
for P in (0.0, 0.1):
  for B, N in ((64, 97), (64, 49)):
      qkv = torch.randn(B, N, 3 * D, device="cuda")
      do = torch.randn(B, N, D, device="cuda")
      o, lse = Fn.attn_dh16_train_fwd(qkv, B, N, H, dh)
      dqkv = torch.empty_like(qkv)
      kw = dict(dropout_p=P, seed=1, stream_id=2)
      f = lambda: Fn.attn_dh16_train_fwd(qkv, B, N, H, dh, o=o, lse=lse, **kw)
      b = lambda: Fn.attn_dh16_train_bwd(do, qkv, lse, B, N, H, dh, dqkv=dqkv, **kw)
      q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
      fv = lambda: Fn.attn_small_fwd(q, k, v, B, N, N, H, dh, dh ** -0.5, q_batch_stride=N * 3 * D, kv_batch_stride=N * 3 * D, **kw)
      bv = lambda: Fn.attn_small_bwd(do, q, k, v, B, N, N, H, dh, dh ** -0.5, q_batch_stride=N * 3 * D, kv_batch_stride=N * 3 * D, dq_out=dqkv[..., :D],
                                     dkv_out=dqkv[..., D:], **kw)
      print(f"p={P} B={B} N={N}: MFMA fwd {timeit(f)*1e6:6.1f} us, bwd (2 launches) {timeit(b)*1e6:6.1f} us | VALU fwd {timeit(fv)*1e6:6.1f} us, bwd {timeit(bv)*1e6:6.1f} us", flush=True)
for B, N in ((64, 97), (64, 49)):
    qkv = torch.randn(B, N, 3 * D, device="cuda")
    o16 = Fn.attn_dh16_fwd(qkv, B, N, H, dh)
    print(f"inference B={B} N={N}: MFMA fwd {timeit(lambda: Fn.attn_dh16_fwd(qkv, B, N, H, dh, o=o16))*1e6:6.1f} us", flush=True)
