"""The speculative decode tails alone (spec_tail_k and, for sampled requests at top-p 0.9 and
temperature 0.8, spec_sample_tail_k; csrc/decode_tail.hip) against the lockstep tails
(greedy_tail_k, sample_tail_k) at V = 32000, bf16, batch 1 and 8, S 4 and 8.

``--reps`` back-to-back launches are captured in one hipGraph and a replay is timed
with device events, five replays per round, two rounds, the kernels alternating.
Launch k reads logits rows k .. k + b * S of one random matrix, so every launch sees
other rows, no draft is confirmed and the context (128 random tokens, ngram 3) grows
by one token per launch; the state is put back before every replay.
Usage: python scripts/spec_tail_bench.py [--reps 200]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epfl_megatron_amd.ops._ext import ext  # noqa: E402

V, CTX = 32000, 128


def z(*shape, dtype=torch.long):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def greedy(b, reps, logits):
    state = [z(b), z(b, reps + 8), z(1), z(b), z(1), z(1, dtype=torch.int32), z(1, dtype=torch.int32)]

    def reset():
        state[2].zero_()  # step_idx: the history column the next launch writes

    return reset, lambda k: ext().greedy_tail(logits[k:k + b], *state)


def sample(b, reps, logits):
    state = [z(b), z(b, reps + 8), z(1), z(b), z(1), z(1, dtype=torch.int32), z(1, dtype=torch.int32),
             torch.tensor([1234, 0, 0, 0, -1, 0], device="cuda"), torch.tensor([0.8, 0.9], device="cuda")]

    def reset():
        state[2].zero_()

    return reset, lambda k: ext().sample_tail(logits[k:k + b], *state)


def spec(b, S, reps, logits, sampled=False):
    cap = CTX + reps * S + 8
    history = torch.randint(0, V, (b, cap), device="cuda")
    tokens = history[:, CTX - 1:CTX].repeat(1, S)
    pos = torch.arange(CTX - 1, CTX - 1 + S, device="cuda").repeat(b, 1)
    init = [tokens, pos, z(b) + CTX - 1, z(b, dtype=torch.int32) + CTX - 1 + S, history, z(b) + CTX,
            z(b) + cap, z(b, dtype=torch.int32) + 1, z(b), z(1), torch.tensor([-1, 3, b], device="cuda")]
    state = [t.clone() for t in init]
    scratch = [z(b, S, dtype=torch.int32), z(b + 1, dtype=torch.int32)]

    def reset():
        for t, t0 in zip(state, init):
            t.copy_(t0)

    if sampled:  # ctl grows to [stop_id, ngram, active, seed, offset0, top_k, vocab_limit]
        init[10] = torch.tensor([-1, 3, b, 1234, 0, 0, 0], device="cuda")
        state[10] = init[10].clone()
        extra = [torch.tensor([0.8, 0.9], device="cuda"), z(b) + CTX]  # fctl, gen0
        return reset, lambda k: ext().spec_sample_tail(logits[k:k + b * S], *state, *extra, *scratch)
    return reset, lambda k: ext().spec_tail(logits[k:k + b * S], *state, *scratch)


def timed(reset, launch, reps):
    """us per launch of five timed replays of ``reps`` captured launches."""
    stream = torch.cuda.Stream()
    reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k in range(reps):
            launch(k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for k in range(reps):
            launch(k)
    out = []
    for _ in range(5):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) * 1e3 / reps, 2))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spec_tail_bench.py times GPU kernels: no GPU found")
    torch.manual_seed(0)
    logits = torch.randn(a.reps + 64, V, device="cuda").bfloat16()
    for b in (1, 8):
        runs = {f"greedy b{b}": greedy(b, a.reps, logits)}
        runs.update({f"spec b{b} S{S}": spec(b, S, a.reps, logits) for S in (4, 8)})
        runs[f"sample b{b}"] = sample(b, a.reps, logits)
        runs.update({f"spec_sample b{b} S{S}": spec(b, S, a.reps, logits, True) for S in (4, 8)})
        us = {name: [] for name in runs}
        for _ in range(2):
            for name, (reset, launch) in runs.items():
                us[name] += timed(reset, launch, a.reps)
        for name, t in us.items():
            print(json.dumps({"kernel": name, "us_per_launch": t, "median": round(statistics.median(t), 2)}), flush=True)
