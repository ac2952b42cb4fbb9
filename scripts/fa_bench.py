"""FlashAttention fwd/bwd timing (1 GPU), causal, bf16.

    python scripts/fa_bench.py [--window W] [b,s,nq,nkv,hd ...]

Default shapes: the Llama-2-7B training shape (8 x 1024, 32 heads) and the
seq-4096 one.  Per shape: median over 20 timed forward calls and over 10
forward+backward pairs (backward time = pair - forward).  EMA_FA_WAVES=4|8
forces the forward / dQ grid form.  --window W: sliding-window attention (the
TF/s figures stay those of full causal work, so they compare as times; the
line also gives the share of the causal key tiles a windowed forward visits).
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops.attention import flash_attn_func  # noqa: E402


def tile_ratio(s, window, bm=128, kt=64):
    """Key tiles a windowed forward / dQ grid visits over those of full causal:
    the kernels' own [t0, ntiles) per query block of bm rows (t0: the tile of
    the block's first row's first visible key)."""
    full = win = 0
    for m0 in range(0, s, bm):
        ntiles = (min(m0 + bm, s) + kt - 1) // kt
        full += ntiles
        win += ntiles - max(m0 - window + 1, 0) // kt
    return win / full


def run(b, s, nq, nkv, hd, window=0):
    torch.manual_seed(0)
    q = torch.randn(b, s, nq, hd, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(b, s, nkv, hd, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(b, s, nkv, hd, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(b, s, nq, hd, device="cuda", dtype=torch.bfloat16)
    fl = 4.0 * b * nq * s * s * hd / 2  # causal
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    tf = []
    with torch.no_grad():
        for it in range(23):
            e0, e1 = ev(), ev()
            e0.record()
            flash_attn_func(q, k, v, causal=True, window=window)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                tf.append(e0.elapsed_time(e1))
    tb = []
    for it in range(12):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        o = flash_attn_func(q, k, v, causal=True, window=window)
        e1.record()
        o.backward(do)
        e2.record()
        torch.cuda.synchronize()
        if it >= 2:
            tb.append(e1.elapsed_time(e2))
        q.grad = k.grad = v.grad = None
    f, bw = statistics.median(tf), statistics.median(tb)
    tag = f" W={window} (key tiles x{tile_ratio(s, window):.3f})" if window else ""
    print(f"b={b} s={s} nq={nq} nkv={nkv} hd={hd}{tag}: fwd {f * 1e3:.1f} us ({fl / f / 1e9:.0f} TF/s)  "
          f"bwd {bw * 1e3:.1f} us ({2.5 * fl / bw / 1e9:.0f} TF/s)", flush=True)


def main():
    argv, window = sys.argv[1:], 0
    if "--window" in argv:
        i = argv.index("--window")
        window = int(argv[i + 1])
        del argv[i:i + 2]
    shapes = argv or ["8,1024,32,32,128", "2,4096,32,32,128"]
    for sh in shapes:
        run(*[int(v) for v in sh.split(",")], window=window)


if __name__ == "__main__":
    main()
