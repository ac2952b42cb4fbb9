"""16-bit vs FP8 vs MXFP4 packed weight streams of the fused decode products
(csrc/skinny_gemm.hip), as the decode layer calls them: QKV + RoPE + cache,
dense + residual, fc1 + SwiGLU, fc2 + residual on the Llama-2-7B shapes
(--k8192: the 70B TP8 shard shapes).  Each form cycles through enough copies
of its packed weight to stream from HBM (> 600 MB per form, beyond the 256 MB
Infinity Cache); the three forms alternate trial by trial in one process and
the spread over the trials is printed beside the medians.  The TB/s figures
count the weight bytes of the form (2, 1 and 17 / 32 bytes per weight).

Usage: python scripts/mxfp4_decode_bench.py [--k8192] [--rows 1,8,16,32]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops._ext import ext  # noqa: E402
from epfl_megatron_amd.ops import decode_pack, fp8_weights, mxfp4_weights  # noqa: E402
from epfl_megatron_amd.ops.rope import rope_table  # noqa: E402

DEV, DT = "cuda", torch.bfloat16
BYTES = {"16-bit": 2.0, "fp8": 1.0, "mxfp4": 17.0 / 32.0}  # per weight, scales included


def timed(calls, trials=3):
    """Per-call microseconds of each trial (one trial = every weight copy once)."""
    out = []
    for _ in range(trials):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for c in calls:
            c()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / len(calls))
    return out


def product(C, name, M, N, K):
    """({form: calls}, weight elements) of one decode product."""
    glu = name == "fc1"
    rows = 2 * N if glu else N
    norm = name in ("qkv", "fc1") and M <= 16  # 17-32 rows: the layer norms separately
    x = torch.randn(M, K, device=DEV, dtype=DT)
    g = (torch.rand(K, device=DEV) + 0.5).to(DT) if norm else None
    res = torch.randn(M, N, device=DEV, dtype=DT)
    tail = C.skinny_glu_half_tail(N, K, norm, M) if glu else 0
    hd = 128
    r = 1 if N % (3 * hd) == 0 else 8  # MHA, or one 70B GQA group of 8 q heads
    ng = max(N // ((r + 2) * hd), 1)
    cos, sin = rope_table(hd, 64, DEV)
    pos = torch.arange(M, device=DEV).view(M, 1) + 3
    kc = torch.zeros(8, M, ng, hd, device=DEV, dtype=DT)
    vc = torch.zeros_like(kc)
    slot = torch.tensor([2], device=DEV)

    def call(w, s):
        if name == "qkv":
            return lambda: C.skinny_qkv_rope_cache(x, w, g, 1e-5, ng, r, hd, cos, sin, pos, kc, vc,
                                                   slot, 0, True, s)
        if glu:
            return lambda: C.skinny_norm_glu(x, w, g, 1e-5, 0, True, tail, s)
        return lambda: C.skinny_norm_gemm(x, w, None, 0.0, res, True, s)
    w = (torch.randn(rows, K, device=DEV) * 0.02).to(DT)
    q, scale = fp8_weights.quantize_rows(w)
    packs = {"16-bit": (decode_pack.pack(w, glu, tail), None),
             "fp8": (fp8_weights.pack_fp8(q, glu, tail), scale),
             "mxfp4": mxfp4_weights.pack_mxfp4(*mxfp4_weights.quantize_blocks(w), glu, tail)}
    del w, q
    calls = {}
    for form, (pw, ps) in packs.items():
        # the stream's content does not matter to its time: copies of one packed weight
        copies = max(2, -(-600_000_000 // int(rows * K * BYTES[form])))
        calls[form] = [call(pw.clone(), None if ps is None else ps.clone()) for _ in range(copies)]
    return calls, rows * K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k8192", action="store_true", help="Llama-2-70B TP8 shard shapes")
    ap.add_argument("--rows", default="1,8,16,32")
    a = ap.parse_args()
    C = ext()
    shapes = [("qkv", 1280, 8192), ("dense", 8192, 1024), ("fc1", 3584, 8192), ("fc2", 8192, 3584)] \
        if a.k8192 else [("qkv", 12288, 4096), ("dense", 4096, 4096), ("fc1", 11008, 4096),
                         ("fc2", 4096, 11008)]
    for name, N, K in shapes:
        for M in [int(r) for r in a.rows.split(",")]:
            with torch.no_grad():
                calls, elems = product(C, name, M, N, K)
                for cs in calls.values():  # warm-up: every copy once
                    for c in cs:
                        c()
                torch.cuda.synchronize()
                t = {form: [] for form in calls}
                for _ in range(3):  # alternate the forms
                    for form, cs in calls.items():
                        t[form] += timed(cs, 3)
            med = {form: statistics.median(v) for form, v in t.items()}
            cols = " | ".join(f"{form} {med[form]:.1f} us [{min(v):.1f}-{max(v):.1f}] "
                              f"({BYTES[form] * elems / med[form] / 1e6:.2f} TB/s)"
                              for form, v in t.items())
            print(f"{name} N={N} K={K} M={M}: {cols} -> mxfp4 {med['16-bit'] / med['mxfp4']:.2f}x "
                  f"16-bit, {med['fp8'] / med['mxfp4']:.2f}x fp8", flush=True)
            del calls
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
