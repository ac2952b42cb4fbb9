"""Multi-row decode attention (csrc/flash_decode_mq.hip: sq in 2..16 new tokens per
sequence behind a cache whose length lives on the device) against the only
alternative for the same mathematics: one causal forward call per sequence with
a host length (``flash_attn_func`` on the sequence's keys; ``flash_attn_fp8_kv``
over an e4m3 cache).  The two alternate in one process.

Shapes: Llama-2-7B attention (32 / 32 heads) and GQA 64 / 8, head_dim 128, bf16;
sq in {2, 4, 8, 16} x batch {1, 8, 32} x keys {512, 2048, 4096}, a 16-bit and an
e4m3 cache.  Every sequence holds ``keys`` keys and the cache capacity is
``keys``.  Successive launches read other sequences of a set of 64 (its size
is printed per line: the small GQA shapes fit the last-level cache, the others
do not); the launches of one measurement are captured in a hipGraph and the
replay is event-timed, best of 5, in two rounds so that the spread is seen.
Usage: python scripts/decode_mq_bench.py [--reps 8] [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops import attention as A  # noqa: E402
from epfl_megatron_amd.ops import fp8_kv  # noqa: E402

SEQS, HD = 64, 128


def timed(fn, n_rot, reps):
    """us per call of `reps` graph-captured calls fn(i) over the rotating inputs."""
    def calls():
        for i in range(reps):
            fn(i % n_rot)
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


def run(name, nq, nkv, fp8, caches, sc, sq, b, keys, reps):
    kc, vc = caches
    n_rot = SEQS // b
    q = torch.randn(b, sq, nq, HD, device="cuda", dtype=torch.bfloat16)
    kv_len = torch.full((b,), keys, dtype=torch.int32, device="cuda")
    scale = sc if fp8 else None

    def views(i):
        return kc[i * b:(i + 1) * b, :keys], vc[i * b:(i + 1) * b, :keys]

    def multi(i):
        return A.flash_decode_cached(q, *views(i), kv_len, kv_scale=scale)

    def per_sequence(i):
        k, v = views(i)
        if fp8:
            return [A.flash_attn_fp8_kv(q[j:j + 1], k[j:j + 1], v[j:j + 1], sc) for j in range(b)]
        return [A.flash_attn_func(q[j:j + 1], k[j:j + 1], v[j:j + 1], causal=True) for j in range(b)]

    with torch.no_grad():
        got, want = multi(0), torch.cat(per_sequence(0), 0)
    err = float((got.float() - want.float()).abs().max())
    assert err < 2e-2 and bool(got.any()), err
    t = {"multi": [], "fwd": []}
    for _ in range(2):
        t["multi"].append(timed(multi, n_rot, reps))
        t["fwd"].append(timed(per_sequence, n_rot, reps))
    mq, fw = min(t["multi"]), min(t["fwd"])
    set_mib = n_rot * b * keys * nkv * HD * (1 if fp8 else 2) * 2 / 2 ** 20
    print(f"{name:9s} {'e4m3' if fp8 else 'bf16'} sq={sq:2d} b={b:2d} keys={keys:4d}  "
          f"multi-row {t['multi'][0]:8.1f} / {t['multi'][1]:8.1f} us  "
          f"per-sequence forward {t['fwd'][0]:8.1f} / {t['fwd'][1]:8.1f} us  "
          f"multi / forward {mq / fw:5.2f}  set {set_mib:6.0f} MiB  max diff {err:.1e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="one shape per model and cache type")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_mq_bench.py times GPU kernels: no GPU found")
    for name, nq, nkv in (("llama2-7b", 32, 32), ("gqa-64/8", 64, 8)):
        torch.manual_seed(0)
        k16, v16 = (torch.randn(SEQS, 4096, nkv, HD, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        sc = fp8_kv.new_scales(nkv, "cuda")
        sc[0] *= 2.0 ** -2
        sc[1] *= 2.0 ** -1
        k8, v8 = fp8_kv.quantize(k16, sc[0]), fp8_kv.quantize(v16, sc[1])
        for fp8, caches in ((False, (k16, v16)), (True, (k8, v8))):
            for sq in (4,) if a.quick else (2, 4, 8, 16):
                for b in (8,) if a.quick else (1, 8, 32):
                    for keys in (2048,) if a.quick else (512, 2048, 4096):
                        run(name, nq, nkv, fp8, caches, sc, sq, b, keys, a.reps)
        del k16, v16, k8, v8
