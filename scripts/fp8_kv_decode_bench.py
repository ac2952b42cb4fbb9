"""Decode attention over a 16-bit and an FP8 (e4m3) KV cache, one process
(csrc/flash_decode.hip; ``--inference_fp8_kv_cache``).

MHA 32/32 hd 128 at b in {1, 32} x keys in {512, 2048, 4096} and GQA 64/8 at
b 16 x 3000 keys.  Every launch reads a cache of its own out of a pool larger
than the last-level cache, so a number is an HBM stream and no cache hit; the
launches of one measurement are captured in a hipGraph (no per-launch host
cost) and the replay is event-timed, best of 5.  The 16-bit kernel is timed
twice (before and after the FP8 one) so that its own spread is known.
Usage: python scripts/fp8_kv_decode_bench.py [--reps 40]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops import fp8_kv  # noqa: E402
from epfl_megatron_amd.ops.attention import attention_ref, flash_decode_cached  # noqa: E402

POOL_BYTES = 1 << 30  # > L2 + MALL


def timed(q, caches, kv_len, sc, reps):
    """us per launch of `reps` graph-captured launches over the rotating caches."""
    def calls():
        for i in range(reps):
            k, v = caches[i % len(caches)]
            flash_decode_cached(q, k, v, kv_len, kv_scale=sc)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), torch.no_grad():
        calls()  # warm-up: sizes the kernel's workspaces before capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=stream):
        calls()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


def run(b, keys, nq, nkv, hd, reps):
    torch.manual_seed(0)
    per16 = 2 * keys * b * nkv * hd * 2
    n = max(2, min(reps, -(-POOL_BYTES // per16)))
    q = torch.randn(b, 1, nq, hd, device="cuda", dtype=torch.bfloat16)
    kv_len = torch.tensor([keys], device="cuda", dtype=torch.int32)
    sc = fp8_kv.new_scales(nkv, "cuda")
    sc[0] *= 2.0 ** -2
    sc[1] *= 2.0 ** -1
    c16, c8 = [], []
    for _ in range(n):
        k = torch.randn(keys, b, nkv, hd, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(keys, b, nkv, hd, device="cuda", dtype=torch.bfloat16)
        c16.append((k.transpose(0, 1), v.transpose(0, 1)))
        c8.append((fp8_kv.quantize(k, sc[0]).transpose(0, 1), fp8_kv.quantize(v, sc[1]).transpose(0, 1)))
    # both forms against the fp32 reference over what they read
    with torch.no_grad():
        o16 = flash_decode_cached(q, *c16[0], kv_len)
        o8 = flash_decode_cached(q, *c8[0], kv_len, kv_scale=sc)
    r16 = attention_ref(q.float(), c16[0][0].float(), c16[0][1].float(), False, hd ** -0.5)
    r8 = attention_ref(q.float(), fp8_kv.dequantize(c8[0][0], sc[0]), fp8_kv.dequantize(c8[0][1], sc[1]),
                       False, hd ** -0.5)
    assert (o16.float() - r16).abs().max() < 3e-2 and (o8.float() - r8).abs().max() < 3e-2
    a = timed(q, c16, kv_len, None, reps)
    f = timed(q, c8, kv_len, sc, reps)
    a2 = timed(q, c16, kv_len, None, reps)
    gb16 = per16 / 1e9
    print(f"b={b:2d} keys={keys:4d} nq={nq} nkv={nkv} hd={hd}  16-bit {a:7.1f} / {a2:7.1f} us "
          f"({gb16 / min(a, a2) * 1e6:6.0f} GB/s)  fp8 {f:7.1f} us ({gb16 / 2 / f * 1e6:6.0f} GB/s)  "
          f"fp8 / 16-bit {f / min(a, a2):.2f}  cache {per16 >> 10} -> {per16 >> 11} KiB", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    for b in (1, 32):
        for keys in (512, 2048, 4096):
            run(b, keys, 32, 32, 128, a.reps)
    run(16, 3000, 64, 8, 128, a.reps)
