"""FP8 vs 16-bit packed weight streams of the fused decode products
(csrc/skinny_gemm.hip), as the decode layer calls them: QKV + RoPE + cache,
dense + residual, fc1 + SwiGLU, fc2 + residual on the Llama-2-7B shapes
(--k8192: the 70B TP8 shard shapes).  Each form cycles through enough weight
copies to stream from HBM (> 600 MB per form, beyond the 256 MB Infinity
Cache); the two forms alternate trial by trial in one process and the spread
over the trials is printed beside the medians.

Usage: python scripts/fp8_decode_bench.py [--k8192] [--rows 1,16,32]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops._ext import ext  # noqa: E402
from epfl_megatron_amd.ops import decode_pack, fp8_weights  # noqa: E402
from epfl_megatron_amd.ops.rope import rope_table  # noqa: E402

DEV, DT = "cuda", torch.bfloat16


def timed(calls, trials=7):
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
    """(16-bit calls, FP8 calls, weight elements) of one decode product."""
    glu = name == "fc1"
    rows = 2 * N if glu else N
    norm = name in ("qkv", "fc1") and M <= 16  # 17-32 rows: the layer norms separately
    x = torch.randn(M, K, device=DEV, dtype=DT)
    g = (torch.rand(K, device=DEV) + 0.5).to(DT) if norm else None
    res = torch.randn(M, N, device=DEV, dtype=DT)
    tail = C.skinny_glu_half_tail(N, K, norm, M) if glu else 0
    copies = max(2, -(-600_000_000 // (rows * K)))
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
    c16, c8 = [], []
    for i in range(copies):
        w = (torch.randn(rows, K, device=DEV) * 0.02).to(DT)
        q, scale = fp8_weights.quantize_rows(w)
        c16.append(call(decode_pack.pack(w, glu, tail), None))
        c8.append(call(fp8_weights.pack_fp8(q, glu, tail), scale))
        del w, q
    return c16, c8, rows * K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k8192", action="store_true", help="Llama-2-70B TP8 shard shapes")
    ap.add_argument("--rows", default="1,16,32")
    a = ap.parse_args()
    C = ext()
    shapes = [("qkv", 1280, 8192), ("dense", 8192, 1024), ("fc1", 3584, 8192), ("fc2", 8192, 3584)] \
        if a.k8192 else [("qkv", 12288, 4096), ("dense", 4096, 4096), ("fc1", 11008, 4096),
                         ("fc2", 4096, 11008)]
    for name, N, K in shapes:
        for M in [int(r) for r in a.rows.split(",")]:
            with torch.no_grad():
                c16, c8, elems = product(C, name, M, N, K)
                for c in c16 + c8:  # warm-up: every copy once
                    c()
                torch.cuda.synchronize()
                t16, t8 = [], []
                for _ in range(3):  # alternate the two forms
                    t16 += timed(c16, 3)
                    t8 += timed(c8, 3)
            m16, m8 = statistics.median(t16), statistics.median(t8)
            print(f"{name} N={N} K={K} M={M}: 16-bit {m16:.1f} us [{min(t16):.1f}-{max(t16):.1f}] "
                  f"({2 * elems / m16 / 1e6:.2f} TB/s) | fp8 {m8:.1f} us [{min(t8):.1f}-{max(t8):.1f}] "
                  f"({elems / m8 / 1e6:.2f} TB/s) -> {m16 / m8:.2f}x", flush=True)
            del c16, c8
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
