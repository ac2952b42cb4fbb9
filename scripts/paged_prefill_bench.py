"""Paged against contiguous forward attention (csrc/flash_attn_fwd.hip, the
PAGED forms) at Llama-2-7B shapes: b = 1, 32 heads of 128, bf16, a block of
``sq`` queries behind a prefix of ``s0`` cached keys (sk = s0 + sq, causal,
bottom-right aligned), the form picked automatically from (b, sq, nq, hd) on
both sides.  The pool holds the same keys under a shuffled page table.

Per shape: a warm-up of each side, then --reps repetitions of --iters launches
each, alternating the two sides, timed with device events.  The margin is the
contiguous kernel's own repeat-to-repeat spread.  Outputs are compared bit for
bit at the sizes timed.

Usage: python scripts/paged_prefill_bench.py [--prefix 1024,4096] [--sq 128,1024,4096]
       [--reps 5] [--iters 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", default="1024,4096")
    ap.add_argument("--sq", default="128,1024,4096")
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv_heads", type=int, default=32)
    ap.add_argument("--head_dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import torch
    from epfl_megatron_amd.inference.paged import KV_PAGE, pages_for
    from epfl_megatron_amd.ops.attention import flash_attn_func, flash_attn_paged
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    nq, nkv, hd = a.heads, a.kv_heads, a.head_dim
    res = []
    for s0 in [int(x) for x in a.prefix.split(",")]:
        for sq in [int(x) for x in a.sq.split(",")]:
            sk = s0 + sq
            torch.manual_seed(sk)
            q = torch.randn(1, sq, nq, hd, device=dev).to(dt)
            k, v = (torch.randn(1, sk, nkv, hd, device=dev).to(dt) for _ in range(2))
            n = pages_for(sk)
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)) + 1  # page 0: null
            table = perm.to(torch.int32)[None].to(dev)
            pk, pv = (torch.zeros(1, (n + 1) * KV_PAGE, nkv, hd, device=dev, dtype=dt) for _ in range(2))
            pos = torch.arange(sk, device=dev)
            rows = table[0][pos // KV_PAGE].long() * KV_PAGE + pos % KV_PAGE
            pk[0, rows], pv[0, rows] = k[0], v[0]
            sides = {"contiguous": lambda: flash_attn_func(q, k, v, causal=True),
                     "paged": lambda: flash_attn_paged(q, pk, pv, table, sk)}
            with torch.no_grad():
                same = torch.equal(sides["paged"]().view(torch.int16),
                                   sides["contiguous"]().view(torch.int16))
                for fn in sides.values():
                    for _ in range(5):
                        fn()
                us = {name: [] for name in sides}
                for _ in range(a.reps):
                    for name, fn in sides.items():
                        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                        e0.record()
                        for _ in range(a.iters):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        us[name].append(round(1e3 * e0.elapsed_time(e1) / a.iters, 2))
            # causal FLOPs of the block: 4 hd per (query, visible key) pair
            pairs = sq * s0 + sq * (sq + 1) // 2
            best = {name: min(t) for name, t in us.items()}
            r = {"prefix": s0, "sq": sq, "sk": sk, "heads": nq, "kv_heads": nkv, "head_dim": hd,
                 "contiguous_us": us["contiguous"], "paged_us": us["paged"],
                 "contiguous_spread_pct": round(100 * (max(us["contiguous"]) / best["contiguous"] - 1), 2),
                 "paged_vs_contiguous_pct": round(100 * (best["paged"] / best["contiguous"] - 1), 2),
                 "contiguous_tflops": round(4 * hd * nq * pairs / best["contiguous"] / 1e6, 1),
                 "bitwise_equal": same}
            print(json.dumps(r), flush=True)
            res.append(r)
    return res


if __name__ == "__main__":
    main()
