"""Serving benchmark: KV-cached generation throughput on 1 GPU.

Llama-2-7B architecture, random init, bf16.  For each batch size: prefill a
128-token prompt, then decode 128 tokens one step at a time (greedy argmax on
the device, no host sync inside the loop); reports prefill ms and decode
tokens/s (batch x steps / decode time).  The decode step runs the framework's
inference path: fused QKV GEMM, RoPE pass with the position offset, KV-cache
write, split-key decode attention (csrc/flash_decode.hip), SwiGLU, RMSNorm.

With --top_k / --top_p / --temperature the tokens are sampled instead: by
GraphedSamplingDecoder under --graph (the draw is inside the graph), else by
one fused launch per step (ops/sampling.py sample_fused; --eager_sample runs
inference/sampling.py's sort / softmax / multinomial chain for comparison).

--continuous: a fixed, seeded list of requests (prompt and generation lengths
drawn once from --prompt_range / --gen_range) served by ContinuousBatcher
(inference/continuous.py: ragged decode, finished rows refilled between replays
of one captured graph) at each batch size, and, where the lockstep decoders can
serve them at all (uniform prompts), the same requests in groups of B through
GraphedGreedyDecoder / GraphedSamplingDecoder, each group running to its longest
member.  Reports useful tokens/s (tokens a request asked for, prefill time
included) for both; with a prompt-length range the baseline is "not possible".

--kv_pages N (with --continuous): the batcher over a paged KV cache of N pages
of 256 keys (inference/paged.py); reports how often an admission waited for
pages and the peak pages in use.  --paged_cost: the same requests, seed and
batch through the unpaged and the paged batcher in one process, alternating.

--continuous --prefix_share: what prefix sharing buys (ContinuousBatcher(prefix_cache=True),
inference/paged.py PrefixCache).  A seeded request list with one common system
prompt of --system_prompt tokens and unique tails (--prompt_range) is served
by the paged batcher without and with the prefix cache, alternating in one
process, --reps timed repetitions each; then the same for the list without a
common prefix (prompts drawn from --no_prefix_range: the host cost of matching
when nothing matches).  Reports useful tokens/s and the mean time from a
request's admission to its first token.  The baseline is the paged batcher
without the cache.

--ragged_cost: what per-row state costs a uniform batch: RaggedGreedyDecoder
against GraphedGreedyDecoder from the same prefilled cache, --reps repetitions
each, alternating; the spread of the lockstep decoder's repetitions is the margin.

Usage: python scripts/serve_bench.py [--batches 1,8,32] [--graph]
       [--top_k K | --top_p P] [--temperature T]
       [--continuous [--requests N] [--prompt_range LO,HI] [--gen_range LO,HI]
        [--poll_every 1,4,16] [--kv_pages N] [--capacity C]] [--ragged_cost [--reps 3]]
       [--paged_cost [--reps 3] [--kv_pages N]]
       [--continuous --prefix_share [--system_prompt 1024] [--prompt_range LO,HI]
        [--no_prefix_range LO,HI] [--prefill_chunk C] [--reps 3]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--graph", action="store_true",
                    help="decode steps replayed from one captured hipGraph (inference/hip_graph.py)")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=0.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--eager_sample", action="store_true",
                    help="without --graph: sample with inference/sampling.py's eager chain")
    ap.add_argument("--fp8_weights", action="store_true",
                    help="FP8 weight-only decode (--inference_fp8_weights; ops/fp8_weights.py)")
    ap.add_argument("--mxfp4_weights", action="store_true",
                    help="MXFP4 weight-only decode (--inference_mxfp4_weights; ops/mxfp4_weights.py)")
    ap.add_argument("--fp8_kv_cache", action="store_true",
                    help="FP8 KV cache (--inference_fp8_kv_cache; ops/fp8_kv.py)")
    ap.add_argument("--continuous", action="store_true",
                    help="serve a seeded request list through ContinuousBatcher (and the lockstep "
                         "baseline where it exists)")
    ap.add_argument("--requests", type=int, default=0, help="--continuous: requests (0: 4 x batch)")
    ap.add_argument("--prompt_range", default="128,128", help="--continuous: prompt lengths LO,HI")
    ap.add_argument("--gen_range", default="16,256", help="--continuous: generation lengths LO,HI")
    ap.add_argument("--poll_every", default="4", help="--continuous: values to run, comma separated")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ragged_cost", action="store_true",
                    help="RaggedGreedyDecoder against GraphedGreedyDecoder on a uniform batch")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["lockstep", "ragged", "unpaged", "paged"], default=None,
                    help="--ragged_cost / --paged_cost: run one of the two sides (a per-kernel "
                         "profile of each)")
    ap.add_argument("--kv_pages", default="",
                    help="--continuous: pages of the paged KV cache (InferenceParams kv_pages), one "
                         "value or one per --batches entry, 0: unpaged; --paged_cost: the paged "
                         "side's pages (default: enough that nothing waits)")
    ap.add_argument("--capacity", type=int, default=0,
                    help="--continuous / --paged_cost: cache capacity per row (default: the longest "
                         "request)")
    ap.add_argument("--paged_cost", action="store_true",
                    help="the same requests through the unpaged and the paged ContinuousBatcher, "
                         "alternating, --reps repetitions each")
    ap.add_argument("--prefix_share", action="store_true",
                    help="--continuous: the paged batcher with and without prefix_cache on a "
                         "request list with a common system prompt, and on one without")
    ap.add_argument("--system_prompt", type=int, default=1024,
                    help="--prefix_share: tokens of the common prefix")
    ap.add_argument("--no_prefix_range", default="16,1920",
                    help="--prefix_share: prompt lengths LO,HI of the list without a common prefix")
    ap.add_argument("--prefill_chunk", type=int, default=0,
                    help="--prefix_share: ContinuousBatcher prefill_chunk (0: whole prompts)")
    a = ap.parse_args()
    sampling = a.top_k > 0 or a.top_p > 0.0 or a.temperature != 1.0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29561"),
                      RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch
    import finetune
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.initialize import initialize_megatron
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder, GraphedSamplingDecoder
    from epfl_megatron_amd.inference.sampling import sample
    from epfl_megatron_amd.ops.sampling import sample_fused
    skw = dict(top_k=a.top_k, top_p=a.top_p, temperature=a.temperature)

    def pick(logits):
        if not sampling:
            return logits[:, -1].argmax(-1, keepdim=True)
        if a.eager_sample:
            return sample(logits[:, -1].float(), vocab_size=32000, **skw).view(-1, 1)
        return sample_fused(logits[:, -1], vocab_size=32000, **skw).view(-1, 1)

    argv = ["--num_layers", str(a.layers), "--hidden_size", "4096", "--num_attention_heads", "32",
            "--ffn_hidden_size", "11008", "--seq_length", "4096", "--max_position_embeddings",
            "4096", "--position_embedding_type", "rotary", "--use_rms_norm", "--glu_activation",
            "swiglu", "--no_tie_embed_logits", "--model_name", "llama2", "--use_flash_attn",
            "--hidden_dropout", "0.0", "--attention_dropout", "0.0", "--bf16",
            "--tokenizer_type", "NullTokenizer", "--synthetic_vocab_size", "32000",
            "--make_vocab_size_divisible_by", "128", "--micro_batch_size", "1",
            "--global_batch_size", "1", "--train_iters", "1", "--lr", "1e-4"]
    if a.fp8_weights:
        argv.append("--inference_fp8_weights")
    if a.mxfp4_weights:
        argv.append("--inference_mxfp4_weights")
    if a.fp8_kv_cache:
        argv.append("--inference_fp8_kv_cache")
    initialize_megatron(finetune.extra_args, {"tokenizer_type": "NullTokenizer"}, args_list=argv)
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    m = model[0].eval()
    if a.paged_cost:
        return paged_cost(a, m)
    if a.continuous and a.prefix_share:
        return prefix_share(a, m)
    if a.continuous:
        return continuous(a, m, sampling, skw)
    if a.ragged_cost:
        return ragged_cost(a, m)
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        total = a.prompt + a.gen
        torch.manual_seed(0)
        prompt = torch.randint(0, 32000, (B, a.prompt), device="cuda")
        pos = torch.arange(total, device="cuda")[None].expand(B, -1)
        with torch.no_grad():
            ip = InferenceParams(B, total)
            for rep in range(2):  # rep 0 warms up allocator / kernels
                if not a.graph:
                    ip = InferenceParams(B, total)
                ip.sequence_len_offset = 0  # graph mode: same caches, prefill again
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logits = m(prompt, pos[:, :a.prompt], None, inference_params=ip)
                nxt = pick(logits)
                ip.sequence_len_offset += a.prompt
                if a.graph:  # capture (rep 0) / re-prime, outside the timed region
                    if rep == 0:
                        dec = GraphedSamplingDecoder(m, ip, B, a.gen, vocab_size=32000) \
                            if sampling else GraphedGreedyDecoder(m, ip, B, a.gen)
                    dec.start(nxt, a.prompt, **(skw if sampling else {}))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if a.graph:
                    for _ in range(a.prompt, total - 1):
                        dec.step()
                else:
                    for t in range(a.prompt, total - 1):
                        logits = m(nxt, pos[:, t:t + 1], None, inference_params=ip)
                        nxt = pick(logits)
                        ip.sequence_len_offset += 1
                torch.cuda.synchronize()
                t2 = time.perf_counter()
        steps = a.gen - 1
        mode = "greedy" if not sampling else \
            ("graph_tail" if a.graph else "eager_chain" if a.eager_sample else "fused")
        r = {"batch": B, "graph": bool(a.graph), "sampling": mode, **(skw if sampling else {}),
             "prompt": a.prompt, "gen": a.gen, "prefill_ms": round(1e3 * (t1 - t0), 2),
             "decode_ms_per_step": round(1e3 * (t2 - t1) / steps, 3),
             "decode_tokens_per_s": round(B * steps / (t2 - t1), 1)}
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def continuous(a, m, sampling, skw):
    """--continuous: useful tokens/s of ContinuousBatcher and of the lockstep
    decoders on one seeded request list per batch size."""
    import torch
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedSamplingDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder, GraphedSamplingDecoder
    from epfl_megatron_amd.ops.sampling import sample_fused
    (plo, phi), (glo, ghi) = ([int(x) for x in r.split(",")] for r in (a.prompt_range, a.gen_range))
    cap = max(phi + ghi, a.capacity)
    pages = [int(x) for x in a.kv_pages.split(",")] if a.kv_pages else [0]
    res = []
    for bi, B in enumerate([int(x) for x in a.batches.split(",")]):
        kvp = pages[min(bi, len(pages) - 1)]
        n = a.requests or 4 * B
        g = torch.Generator().manual_seed(a.seed)
        plens = torch.randint(plo, phi + 1, (n,), generator=g).tolist()
        gens = torch.randint(glo, ghi + 1, (n,), generator=g).tolist()
        prompts = [torch.randint(0, 32000, (p,), generator=g) for p in plens]
        useful = sum(gens)
        base = {"mode": "continuous", "batch": B, "requests": n, "prompt_range": [plo, phi],
                "gen_range": [glo, ghi], "useful_tokens": useful, "capacity": cap,
                "kv_pages": kvp, "sampling": dict(skw) if sampling else "greedy"}
        for poll in [int(x) for x in a.poll_every.split(",")]:
            ip = InferenceParams(B, cap, kv_pages=kvp or None)
            dec = None
            if sampling:
                dec = RaggedSamplingDecoder(m, ip, B, ghi, vocab_size=32000)
                dec.configure(**skw)
            cb = ContinuousBatcher(m, ip, B, cap, poll_every=poll, max_new_tokens=ghi, decoder=dec)
            for p in prompts[:B]:  # warm-up: the capture, the allocator, the prefill kernels
                cb.submit(p, 4)
            cb.run()
            warm, waits0 = cb.replays, cb.waits
            if kvp:
                cb.pool.peak = cb.pool.in_use
            for p, gn in zip(prompts, gens):
                cb.submit(p, gn)
            out, dt = _timed(cb.run)
            assert [len(o) for o in out[-n:]] == gens and cb.dec.captures == 1
            r = dict(base, poll_every=poll, replays=cb.replays - warm, seconds=round(dt, 3),
                     continuous_tokens_per_s=round(useful / dt, 1), kv_gib=_kv_gib(ip))
            if kvp:
                r.update(admission_waits=cb.waits - waits0, peak_pages=cb.pool.peak)
            if plo != phi:
                r["static_tokens_per_s"] = "not possible"
            res.append(r)
        if plo == phi and not kvp:  # the lockstep baseline: groups of B, each to its longest member
            ip = InferenceParams(B, cap)
            pos = torch.arange(cap, device="cuda")[None].expand(B, -1)
            dec = GraphedSamplingDecoder(m, ip, B, ghi, vocab_size=32000) if sampling else \
                GraphedGreedyDecoder(m, ip, B, ghi)

            def static(groups):
                steps = 0
                with torch.no_grad():
                    for i in range(0, groups * B, B):
                        grp = [prompts[min(j, n - 1)] for j in range(i, i + B)]  # last group: padded
                        ip.sequence_len_offset = 0
                        lg = m(torch.stack(grp).cuda(), pos[:, :plo], None, inference_params=ip)[:, -1]
                        nxt = sample_fused(lg, vocab_size=32000, **skw) if sampling else lg.argmax(-1)
                        ip.sequence_len_offset = plo
                        dec.start(nxt.view(B, 1), plo, **(skw if sampling else {}))
                        for _ in range(max(gens[i:i + B]) - 1):
                            dec.step()
                        steps += max(gens[i:i + B]) - 1
                return steps
            static(1)  # warm-up and capture
            steps, dt = _timed(lambda: static(-(-n // B)))
            for r in res[-len(a.poll_every.split(",")):]:
                r.update(static_tokens_per_s=round(useful / dt, 1), static_seconds=round(dt, 3),
                         static_replays=steps)
        for r in res[-len(a.poll_every.split(",")):]:
            print(json.dumps(r), flush=True)
    return res


def _kv_gib(ip):
    """GiB of K / V cache the layers allocated on ``ip``."""
    return round(sum(t.numel() * t.element_size() for kv in ip.key_value_memory_dict.values()
                     for t in kv) / 2 ** 30, 3)


def paged_cost(a, m):
    """--paged_cost: the same seeded request list through the unpaged and the
    paged ContinuousBatcher in one process, alternating, --reps timed
    repetitions each after a warm-up; the page count is large enough that no
    admission waits, so the difference is the indirection alone."""
    import torch
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import pages_for
    (plo, phi), (glo, ghi) = ([int(x) for x in r.split(",")] for r in (a.prompt_range, a.gen_range))
    cap = max(phi + ghi, a.capacity)
    poll = int(a.poll_every.split(",")[0])
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        n = a.requests or 4 * B
        g = torch.Generator().manual_seed(a.seed)
        plens = torch.randint(plo, phi + 1, (n,), generator=g).tolist()
        gens = torch.randint(glo, ghi + 1, (n,), generator=g).tolist()
        prompts = [torch.randint(0, 32000, (p,), generator=g) for p in plens]
        useful = sum(gens)
        kvp = int(a.kv_pages) if a.kv_pages else B * pages_for(cap) + 1
        cbs, secs, outs = {}, {}, {}
        for name in ([a.only] if a.only else ["unpaged", "paged"]):
            ip = InferenceParams(B, cap, kv_pages=kvp if name == "paged" else None)
            cb = ContinuousBatcher(m, ip, B, cap, poll_every=poll, max_new_tokens=ghi)
            for p in prompts[:B]:  # warm-up: the capture, the allocator, the prefill kernels
                cb.submit(p, 4)
            cb.run()
            cbs[name], secs[name] = cb, []
        for rep in range(a.reps):
            for name, cb in cbs.items():
                for p, gn in zip(prompts, gens):
                    cb.submit(p, gn)
                out, dt = _timed(cb.run)
                assert [len(o) for o in out[-n:]] == gens and cb.dec.captures == 1
                secs[name].append(round(dt, 4))
                outs[name] = out[-n:]
        r = {"mode": "paged_cost", "batch": B, "requests": n, "prompt_range": [plo, phi],
             "gen_range": [glo, ghi], "capacity": cap, "kv_pages": kvp, "poll_every": poll,
             "useful_tokens": useful}
        for name, cb in cbs.items():
            r[name + "_seconds"] = secs[name]
            r[name + "_tokens_per_s"] = [round(useful / t, 1) for t in secs[name]]
            r[name + "_kv_gib"] = _kv_gib(cb.ip)
        if not a.only:
            mean = {k: sum(v) / len(v) for k, v in secs.items()}
            r.update(unpaged_spread_s=round(max(secs["unpaged"]) - min(secs["unpaged"]), 4),
                     paged_minus_unpaged_s=round(mean["paged"] - mean["unpaged"], 4),
                     paged_minus_unpaged_pct=round(100 * (mean["paged"] / mean["unpaged"] - 1), 2),
                     admission_waits=cbs["paged"].waits, same_tokens=outs["paged"] == outs["unpaged"])
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def prefix_share(a, m):
    """--continuous --prefix_share: the paged ContinuousBatcher without and with
    the prefix cache, alternating, on a list with a common system prompt and
    on one without; pages enough that no admission waits."""
    import torch
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import pages_for
    (tlo, thi), (nlo, nhi), (glo, ghi) = ([int(x) for x in r.split(",")]
                                          for r in (a.prompt_range, a.no_prefix_range, a.gen_range))
    poll = int(a.poll_every.split(",")[0])
    res = []
    for B in [int(x) for x in a.batches.split(",")]:
        n = a.requests or 4 * B
        g = torch.Generator().manual_seed(a.seed)
        system = torch.randint(0, 32000, (a.system_prompt,), generator=g)
        tails = torch.randint(tlo, thi + 1, (n,), generator=g).tolist()
        gens = torch.randint(glo, ghi + 1, (n,), generator=g).tolist()
        lists = {"common_prefix": [torch.cat([system, torch.randint(0, 32000, (t,), generator=g)])
                                   for t in tails]}
        plens = torch.randint(nlo, nhi + 1, (n,), generator=g).tolist()
        lists["no_prefix"] = [torch.randint(0, 32000, (p,), generator=g) for p in plens]
        useful = sum(gens)
        for lname, prompts in lists.items():
            cap = max(max(p.numel() for p in prompts) + ghi, a.capacity)
            kvp = B * pages_for(cap) + pages_for(a.system_prompt) + 1
            cbs, secs, ttft, outs = {}, {}, {}, {}
            for name in ("baseline", "prefix_cache"):
                ip = InferenceParams(B, cap, kv_pages=kvp)
                cb = ContinuousBatcher(m, ip, B, cap, poll_every=poll, max_new_tokens=ghi,
                                       prefix_cache=name == "prefix_cache",
                                       prefill_chunk=a.prefill_chunk or None)
                cb.first_token_s = []

                def timed_prefill(row, prompt, s0=0, cb=cb, prefill=cb._prefill):
                    # admission to first token: the pages are reserved, the prompt is
                    # prefilled and the first token is read back (a host sync)
                    t0 = time.perf_counter()
                    tok = prefill(row, prompt, s0)
                    cb.first_token_s.append(time.perf_counter() - t0)
                    return tok
                cb._prefill = timed_prefill
                for p in prompts[:B]:  # warm-up: the capture, the allocator, the prefill kernels
                    cb.submit(p, 4)
                cb.run()
                cbs[name], secs[name], ttft[name] = cb, [], []
            for rep in range(a.reps):
                for name, cb in cbs.items():
                    cb.first_token_s.clear()
                    for p, gn in zip(prompts, gens):
                        cb.submit(p, gn)
                    out, dt = _timed(cb.run)
                    assert [len(o) for o in out[-n:]] == gens and cb.dec.captures == 1
                    secs[name].append(round(dt, 4))
                    ttft[name].append(round(1e3 * sum(cb.first_token_s) / n, 3))
                    outs[name] = out[-n:]
            r = {"mode": "prefix_share", "list": lname, "batch": B, "requests": n,
                 "system_prompt": a.system_prompt if lname == "common_prefix" else 0,
                 "prompt_tokens": sum(p.numel() for p in prompts), "gen_range": [glo, ghi],
                 "capacity": cap, "kv_pages": kvp, "poll_every": poll, "useful_tokens": useful,
                 "prefill_chunk": a.prefill_chunk}
            for name, cb in cbs.items():
                r[name + "_seconds"] = secs[name]
                r[name + "_tokens_per_s"] = [round(useful / t, 1) for t in secs[name]]
                r[name + "_first_token_ms"] = ttft[name]
            cb = cbs["prefix_cache"]
            mean = {k: sum(v) / len(v) for k, v in secs.items()}
            r.update(baseline_spread_s=round(max(secs["baseline"]) - min(secs["baseline"]), 4),
                     cache_minus_baseline_s=round(mean["prefix_cache"] - mean["baseline"], 4),
                     cache_minus_baseline_pct=round(100 * (mean["prefix_cache"] / mean["baseline"] - 1), 2),
                     prefix_hit_pages=cb.prefix_hit_pages, prefilled_tokens=cb.prefilled_tokens,
                     baseline_prefilled_tokens=cbs["baseline"].prefilled_tokens,
                     evictions=cb.evictions, admission_waits=cb.waits,
                     same_tokens=outs["prefix_cache"] == outs["baseline"])
            print(json.dumps(r), flush=True)
            res.append(r)
    return res


def ragged_cost(a, m):
    """--ragged_cost: decode ms/step of the ragged and the lockstep greedy
    decoder on a uniform batch, alternating repetitions."""
    import torch
    from epfl_megatron_amd.inference import RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    res = []
    steps = a.gen - 1
    for B in [int(x) for x in a.batches.split(",")]:
        total = a.prompt + a.gen
        torch.manual_seed(0)
        prompt = torch.randint(0, 32000, (B, a.prompt), device="cuda")
        pos = torch.arange(total, device="cuda")[None].expand(B, -1)
        decs, ms = {}, {"lockstep": [], "ragged": []}
        with torch.no_grad():
            for name in ([a.only] if a.only else ["lockstep", "ragged"]):
                ip = InferenceParams(B, total)
                nxt = m(prompt, pos[:, :a.prompt], None, inference_params=ip)[:, -1].argmax(-1)
                ip.sequence_len_offset = a.prompt
                dec = GraphedGreedyDecoder(m, ip, B, a.gen) if name == "lockstep" else \
                    RaggedGreedyDecoder(m, ip, B, a.gen)
                decs[name] = (dec, nxt)
            for rep in range(a.reps + 1):  # rep 0: capture and warm-up
                for name, (dec, nxt) in decs.items():
                    if name == "lockstep":
                        dec.start(nxt.view(B, 1), a.prompt)
                    else:
                        for row in range(B):
                            dec.prime(row, int(nxt[row]), a.prompt, a.gen)

                    def run():
                        for _ in range(steps):
                            dec.step()
                    _, dt = _timed(run)
                    if rep:
                        ms[name].append(round(1e3 * dt / steps, 4))
        r = {"mode": "ragged_cost", "batch": B, "prompt": a.prompt, "gen": a.gen,
             "lockstep_ms_per_step": ms["lockstep"], "ragged_ms_per_step": ms["ragged"]}
        if not a.only:
            r.update(lockstep_spread_ms=round(max(ms["lockstep"]) - min(ms["lockstep"]), 4),
                     ragged_minus_lockstep_ms=round((sum(ms["ragged"]) - sum(ms["lockstep"])) / a.reps, 4),
                     same_tokens=torch.equal(decs["lockstep"][0].history[:, :steps],
                                             decs["ragged"][0].history[:, :steps]))
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


if __name__ == "__main__":
    main()
