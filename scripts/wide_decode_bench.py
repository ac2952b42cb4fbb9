"""Decode products at 33-64 rows: hipBLASLt on the 16-bit weight (the path
above 32 rows without csrc/wide_gemm.hip) against the wide kernel's 16-bit,
e4m3 and MXFP4 forms at the split the host picks and at the forced ones.

The four Llama-2-7B products and the LM head at M = 33, 48, 64, all
candidates of one (product, M) alternated in one process, ``--reps`` rounds of
``--iters`` launches each timed with device events; per candidate the median
and the min-max spread over the rounds, and the achieved TB/s of weight bytes.

    python scripts/wide_decode_bench.py [--reps 5] [--iters 50] > profiles/r19a_wide_decode.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, W rows, K, kind (plain / glu / qkv)
PRODUCTS = [("qkv", 12288, 4096, "qkv"), ("o_proj", 4096, 4096, "plain"),
            ("fc1_swiglu", 22016, 4096, "glu"), ("fc2", 4096, 11008, "plain"),
            ("lm_head", 32000, 4096, "plain")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rows", type=int, nargs="+", default=[33, 48, 64])
    a = ap.parse_args()
    from epfl_megatron_amd.ops._ext import ext
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8, mxfp4_weights as mx
    from epfl_megatron_amd.ops.rope import rope_table
    C, dev, dt = ext(), "cuda", torch.bfloat16
    torch.manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}; us per launch: median [min-max] over {a.reps} rounds "
          f"of {a.iters}; TB/s = weight bytes of the format / median")
    for name, n, k, kind in PRODUCTS:
        w = (torch.randn(n, k, device=dev) * 0.02).to(dt)
        glu = kind == "glu"
        packs = {"w16": (decode_pack.pack(w, glu=glu), None, 2.0)}
        q8, s8 = f8.quantize_rows(w)
        packs["fp8"] = (f8.pack_fp8(q8, glu), s8, 1.0)
        packs["mxfp4"] = (*mx.pack_mxfp4(*mx.quantize_blocks(w), glu), 0.53125)
        nblocks = n // 16
        auto = C.wide_gemm_split(nblocks)
        hd, ng = 128, 32
        cos, sin = rope_table(hd, 4096, dev)
        for m in a.rows:
            x = torch.randn(m, k, device=dev).to(dt)
            pos = torch.full((m, 1), 100, dtype=torch.long, device=dev)
            kc, vc = (torch.zeros(128, m, ng, hd, device=dev, dtype=dt) for _ in range(2))
            slot = torch.full((1,), 100, dtype=torch.long, device=dev)

            def wide(fmt, fb):
                wp, ws, _ = packs[fmt]
                if kind == "glu":
                    return lambda: C.wide_glu(x, wp, 0, ws, fb)
                if kind == "qkv":
                    return lambda: C.wide_qkv_rope_cache(x, wp, ng, 1, hd, cos, sin, pos, kc, vc,
                                                         slot, 0, ws, None, fb)
                return lambda: C.wide_gemm(x, wp, None, ws, fb)
            cands = {"hipblaslt w16 (gemm only)": (lambda: torch.nn.functional.linear(x, w), 2.0)}
            for fmt in packs:
                for fb in sorted({auto, 1, 4, 8}):
                    tag = f"wide {fmt} FB={fb},KS={8 // fb}" + (" (host)" if fb == auto else "")
                    cands[tag] = (wide(fmt, fb), packs[fmt][2])
            times = {c: [] for c in cands}
            for rep in range(a.reps + 1):  # round 0 warms up
                for c, (fn, _) in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[c].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            print(f"\n{name} N={n} K={k} M={m}")
            for c, ts in times.items():
                med = statistics.median(ts)
                print(f"  {c:34s} {med:8.1f} us [{min(ts):7.1f}-{max(ts):7.1f}]  "
                      f"{n * k * cands[c][1] / med / 1e6:5.2f} TB/s")


if __name__ == "__main__":
    main()
