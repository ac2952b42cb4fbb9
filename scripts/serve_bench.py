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

Usage: python scripts/serve_bench.py [--batches 1,8,32] [--graph]
       [--top_k K | --top_p P] [--temperature T]
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


if __name__ == "__main__":
    main()
