#!/usr/bin/env python3
"""The 224 x 256 tiles of gemm_bf16_v6.hip (GR = 112: proj / fc2, N = 768 with a residual) must reproduce the 256 x 256 tiles BIT FOR
BIT (same MFMAs, same K order per output element, same epilogue) — full, ragged last tile (one or both ping-pong groups live),
in-place residual as vit.hip runs it.  Runs itself three times (MEDP_V6_N768 = 1: default, 0: always 256 x 256, 2: also the N = 768
launches without a residual) and compares the output digests; each run also checks against an fp32 product."""
import hashlib, json, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# M = 64 x 257 (the step's proj / fc2); 14000: last 224-row tile holds exactly 112 rows; 13900: 12 rows; 15880: 200 rows (the second group partly)
SHAPES = [(16448, 768, 768), (16448, 768, 3072), (14000, 768, 768), (13900, 768, 1536), (15880, 768, 768)]


def child():
    import torch
    from multimodal_edema_prediction_amd import functional as Fn
    torch.manual_seed(0)
    dev = "cuda"
    out = {}
    def digest(t): return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
    for (m, n, k) in SHAPES:
        a = torch.randn(m, k, device=dev).bfloat16(); w = torch.randn(n, k, device=dev).bfloat16()
        bias = torch.randn(n, device=dev); scale = torch.rand(n, device=dev) + 0.5
        res = torch.randn(m, n, device=dev)
        ref0 = a.float() @ w.float().T
        refr = res + scale * (ref0 + bias)
        y0 = Fn.gemm(a, w, bias=bias, scale=scale, residual=res, out_dtype=torch.float32)
        e0 = (y0 - refr).abs().max().item() / max(1.0, refr.abs().max().item())
        x = res.clone()                                     # in place, as the encoder's residual stream
        Fn.gemm(a, w, bias=bias, scale=scale, residual=x, out=x)
        y1 = Fn.gemm(a, w, bias=bias, out_dtype=torch.bfloat16)
        ref1 = ref0 + bias
        e1 = (y1.float() - ref1).abs().max().item() / max(1.0, ref1.abs().max().item())
        same = bool(torch.equal(x, y0))
        for _ in range(10):
            same &= bool(torch.equal(Fn.gemm(a, w, bias=bias, scale=scale, residual=res, out_dtype=torch.float32), y0))
        ok = e0 <= 1e-3 and e1 <= 1e-2 and same
        key = f"{m}x{n}x{k}"
        out[key] = {"digest": [digest(y0), digest(y1)], "err": [e0, e1], "stable": same, "ok": ok}
        print(key, out[key], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
        sys.exit(0)
    res = {}
    for v in ("1", "0", "2"):
        env = dict(os.environ, MEDP_V6_N768=v)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:
            print(f"MEDP_V6_N768={v}: child failed rc={r.returncode}"); sys.exit(1)
        res[v] = json.loads(r.stdout.strip().splitlines()[-1])
    bad = 0
    for key in res["1"]:
        a, b, c = res["1"][key], res["0"][key], res["2"][key]
        same = a["digest"] == b["digest"] == c["digest"]
        good = same and a["ok"] and b["ok"] and c["ok"]
        bad += not good
        print(f"{key:18s} 224-row tiles == 256-row tiles bitwise: {same}   ok: {a['ok']} {b['ok']} {c['ok']}   err {a['err']}")
    print("FAILED" if bad else "ALL OK")
