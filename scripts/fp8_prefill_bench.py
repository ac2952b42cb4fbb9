"""Continued prefill over a paged FP8 (e4m3) KV cache, three alternatives
alternating in one process (csrc/flash_attn_fwd.hip; ``--inference_fp8_kv_cache``
with ``kv_pages``):

  native    the FP8 paged forms of the forward kernel read the pool bytes;
  fallback  ``EMA_FA_FP8_PREFILL=0``: gather_rows + dequantize into 16-bit
            tensors + the contiguous kernel (what ran before the FP8 forms);
  16-bit    the paged forms over a 16-bit pool of the same keys.

Llama-2-7B attention (b 1, 32 / 32 heads, head_dim 128, bf16): a block of sq in
{128, 1024} queries behind a prefix of {1024, 4096} keys.  Every launch reads a
pool of its own out of a set larger than the last-level cache; the launches of
one measurement are captured in a hipGraph and the replay is event-timed, best
of 5; the three are timed in two rounds so that their spread is known.
Usage: python scripts/fp8_prefill_bench.py [--reps 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.inference.paged import KV_PAGE  # noqa: E402
from epfl_megatron_amd.ops import attention as A  # noqa: E402
from epfl_megatron_amd.ops import fp8_kv  # noqa: E402

POOL_BYTES = 1 << 30  # > L2 + MALL


def timed(fn, n_pools, reps):
    """us per call of `reps` graph-captured calls fn(i) over the rotating pools."""
    def calls():
        for i in range(reps):
            fn(i % n_pools)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), torch.no_grad():
        calls()
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


def run(s0, sq, nq, nkv, hd, reps):
    torch.manual_seed(0)
    sk = s0 + sq
    pages = -(-sk // KV_PAGE)
    rows = (pages + 1) * KV_PAGE  # page 0 stays the null page
    per16 = 2 * rows * nkv * hd * 2
    n = max(2, min(reps, -(-POOL_BYTES // per16)))
    q = torch.randn(1, sq, nq, hd, device="cuda", dtype=torch.bfloat16)
    sc = fp8_kv.new_scales(nkv, "cuda")
    sc[0] *= 2.0 ** -2
    sc[1] *= 2.0 ** -1
    # the row's pages in a scrambled order
    table = (torch.randperm(pages, generator=torch.Generator().manual_seed(1)) + 1).to(
        device="cuda", dtype=torch.int32)[None]
    p16, p8 = [], []
    for _ in range(n):
        k, v = (torch.randn(rows, 1, nkv, hd, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        k8, v8 = fp8_kv.quantize(k, sc[0]), fp8_kv.quantize(v, sc[1])
        p8.append((k8.transpose(0, 1), v8.transpose(0, 1)))
        # the 16-bit pool holds the values the bytes stand for: one result for all three
        p16.append((fp8_kv.dequantize(k8, sc[0], torch.bfloat16).transpose(0, 1),
                    fp8_kv.dequantize(v8, sc[1], torch.bfloat16).transpose(0, 1)))

    def native(i):
        A.FP8_PREFILL_NATIVE = True
        return A.flash_attn_paged(q, *p8[i], table, sk, kv_scale=sc)

    def fallback(i):
        A.FP8_PREFILL_NATIVE = False
        return A.flash_attn_paged(q, *p8[i], table, sk, kv_scale=sc)

    def paged16(i):
        return A.flash_attn_paged(q, *p16[i], table, sk)

    with torch.no_grad():
        before = dict(A.fp8_prefill_calls)
        o8, of, o16 = native(0), fallback(0), paged16(0)
        assert A.fp8_prefill_calls["native"] == before["native"] + 1
        assert A.fp8_prefill_calls["fallback"] == before["fallback"] + 1
    # power-of-two scales: the three compute the same bits
    assert torch.equal(o8, of) and torch.equal(o8, o16) and bool(o8.any())
    t = {"native": [], "fallback": [], "16-bit": []}
    for _ in range(2):
        t["native"].append(timed(native, n, reps))
        t["fallback"].append(timed(fallback, n, reps))
        t["16-bit"].append(timed(paged16, n, reps))
    A.FP8_PREFILL_NATIVE = True
    nat, fb, b16 = (min(t[x]) for x in ("native", "fallback", "16-bit"))
    print(f"prefix={s0:4d} sq={sq:4d} nq={nq} nkv={nkv} hd={hd}  "
          f"native {t['native'][0]:7.1f} / {t['native'][1]:7.1f} us  "
          f"fallback {t['fallback'][0]:7.1f} / {t['fallback'][1]:7.1f} us  "
          f"16-bit paged {t['16-bit'][0]:7.1f} / {t['16-bit'][1]:7.1f} us  "
          f"native / fallback {nat / fb:.2f}  native / 16-bit {nat / b16:.2f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for s0 in (1024, 4096):
        for sq in (128, 1024):
            run(s0, sq, 32, 32, 128, a.reps)
