"""Mistral support on the CPU: sliding-window attention + configurable RoPE
base through conversion, the model, KV-cached generation and the flags.

A tiny random ``transformers.MistralForCausalLM`` (sliding_window 8, rope_theta
1e6, eager attention) is converted with ``weights2megatron mistral`` and its
logits compared with this framework's, with the tolerance and method of
``test_convert.test_llama_hf_logit_parity``.
"""
import argparse
import os
import sys
import types

import pytest
import torch

from dist_utils import run_dist, init_framework

transformers = pytest.importorskip("transformers")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "weights2megatron"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, THETA = 8, 1e6


def _tiny_mistral(path):
    cfg = transformers.MistralConfig(vocab_size=96, hidden_size=64, intermediate_size=160,
                                     num_attention_heads=4, num_key_value_heads=2,
                                     num_hidden_layers=2, max_position_embeddings=64,
                                     rms_norm_eps=1e-5, sliding_window=W, rope_theta=THETA,
                                     tie_word_embeddings=False, attn_implementation="eager")
    torch.manual_seed(0)
    model = transformers.MistralForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in model.parameters():  # non-trivial norms
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model.save_pretrained(path, safe_serialization=True)
    return model


def _theta(cfg):
    d = cfg.to_dict()  # newer transformers keep the base under rope_parameters
    return d.get("rope_theta") or (d.get("rope_parameters") or {}).get("rope_theta")


def _hf_logits(model, tokens):
    with torch.no_grad():
        return model(tokens).logits.float()


def _argv(ckpt, extra=()):
    return ["--num_layers", "2", "--hidden_size", "64", "--num_attention_heads", "4",
            "--num_attention_heads_kv", "2", "--ffn_hidden_size", "160",
            "--seq_length", "32", "--max_position_embeddings", "64",
            "--position_embedding_type", "rotary", "--use_rms_norm", "--glu_activation",
            "swiglu", "--no_tie_embed_logits", "--layernorm_epsilon", "1e-5",
            "--hidden_dropout", "0.0", "--attention_dropout", "0.0",
            "--no_bias_gelu_fusion", "--no_bias_dropout_fusion",
            "--make_vocab_size_divisible_by", "1", "--synthetic_vocab_size", "96",
            "--model_name", "mistral", "--micro_batch_size", "2", "--global_batch_size", "2",
            "--load", ckpt, "--finetune", "--no_load_optim", "--no_load_rng",
            "--use_cpu_initialization", "--train_iters", "1", "--lr", "1e-4",
            "--inference_batch_times_seqlen_threshold", "4"] + list(extra)


def _model(argv):
    import run_text_generation_server as srv
    init_framework(argv, srv.add_text_generate_args)
    from epfl_megatron_amd.checkpointing import load_checkpoint
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.utils.misc import unwrap_model
    model = get_model(srv.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    load_checkpoint(model, None, None)
    return unwrap_model(model)[0].eval()


def _mega_logits(rank, world, argv, tokens):
    from epfl_megatron_amd import get_args
    m = _model(argv)
    args = get_args()
    with torch.no_grad():
        out = m(tokens, None, None).float()
    return out, args.sliding_window_size, args.rope_theta


@pytest.fixture(scope="module")
def mistral_ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("mistral")
    hf = _tiny_mistral(str(d / "hf"))
    import weights2megatron as w2m
    w2m.main("mistral", 7, str(d / "mega"), str(d / "hf"))
    tokens = torch.randint(0, 96, (2, 32), generator=torch.Generator().manual_seed(3))
    return d, hf, tokens


def test_hf_window_semantics(mistral_ckpt):
    """What the parity tests rest on: HF's eager attention applies
    sliding_window = 8 -- rows < 8 equal the same weights without a window,
    later rows differ."""
    _, hf, tokens = mistral_ckpt
    full = transformers.MistralForCausalLM(transformers.MistralConfig(
        **{**hf.config.to_dict(), "sliding_window": None})).float().eval()
    full.load_state_dict(hf.state_dict())
    a, b = _hf_logits(hf, tokens), _hf_logits(full, tokens)
    torch.testing.assert_close(a[:, :W], b[:, :W])  # rows < W: full causal
    assert not torch.allclose(a[:, W:], b[:, W:], atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("flash", [True, False])
def test_mistral_hf_logit_parity(mistral_ckpt, flash):
    """Converted weights, window and RoPE base given on the command line:
    once through the FlashAttention entry (its CPU reference path) and once
    through CoreAttention's boolean mask."""
    d, hf, tokens = mistral_ckpt
    extra = ["--sliding_window_size", str(W), "--rope_theta", str(THETA)]
    if flash:
        extra.append("--use_flash_attn")
    got, _, _ = run_dist(_mega_logits, 1, _argv(str(d / "mega"), extra), tokens)[0]
    assert got.shape == (2, 32, 96)
    torch.testing.assert_close(got, _hf_logits(hf, tokens), atol=2e-4, rtol=1e-4)


def test_mistral_without_window_misses(mistral_ckpt):
    """The same weights with --sliding_window_size unset: rows < 8 still match,
    rows >= 8 miss the parity tolerance -- the parity test sees the window."""
    d, hf, tokens = mistral_ckpt
    got, window, _ = run_dist(_mega_logits, 1, _argv(str(d / "mega"), ["--rope_theta", str(THETA)]),
                              tokens)[0]
    assert window is None
    want = _hf_logits(hf, tokens)
    torch.testing.assert_close(got[:, :W], want[:, :W], atol=2e-4, rtol=1e-4)
    assert not torch.allclose(got[:, W:], want[:, W:], atol=2e-4, rtol=1e-4)
    bad_rows = ((got - want).abs() > 2e-4 + 1e-4 * want.abs()).any(-1)
    assert not bad_rows[:, :W].any() and bad_rows[:, W:].any()


def test_use_checkpoint_args_restores_window_and_theta(mistral_ckpt):
    """--use_checkpoint_args takes both new flags from the converted checkpoint
    (neither is on the command line) and the model then matches HF."""
    d, hf, tokens = mistral_ckpt
    got, window, theta = run_dist(_mega_logits, 1,
                                  _argv(str(d / "mega"), ["--use_checkpoint_args",
                                                          "--use_flash_attn"]), tokens)[0]
    assert window == W and theta == THETA
    torch.testing.assert_close(got, _hf_logits(hf, tokens), atol=2e-4, rtol=1e-4)


def _generate(rank, world, argv, prompt, n):
    m = _model(argv)
    from epfl_megatron_amd.inference import generate_and_post_process
    out = generate_and_post_process(m, prompts=[" ".join(str(t) for t in prompt)],
                                    tokens_to_generate=n, top_k_sampling=1,
                                    use_eod_token_for_early_termination=False)
    tokens = out[3][0]
    seq = list(prompt)  # cache-free greedy decode: the full forward each step
    with torch.no_grad():
        for _ in range(n):
            logits = m(torch.tensor([seq]), None, None).float()
            seq.append(int(torch.argmax(logits[0, -1])))
    return tokens, seq


@pytest.mark.parametrize("extra", [[], ["--use_flash_attn"],
                                   ["--use_flash_attn", "--inference_hip_graph"]])
def test_mistral_kv_cached_generation(mistral_ckpt, extra):
    """Greedy KV-cached generation from a 6-token prompt to 24 tokens (three
    windows long: the cache keeps every key, attention masks all but the last
    8) equals the tokens of full no-cache forwards."""
    d, _, _ = mistral_ckpt
    prompt = [3, 14, 15, 92, 6, 53]
    argv = _argv(str(d / "mega"), ["--sliding_window_size", str(W), "--rope_theta", str(THETA),
                                   "--tokenizer_type", "NullTokenizer"] + extra)
    tokens, seq = run_dist(_generate, 1, argv, prompt, 18)[0]
    assert len(seq) == 24 and tokens[:24] == seq, (tokens, seq)


def test_megatron2hf_mistral_roundtrip(mistral_ckpt, tmp_path):
    d, hf, tokens = mistral_ckpt
    import megatron2hf
    megatron2hf.main(["--input_dir", str(d / "mega"), "--output_dir", str(tmp_path / "out"),
                      "--model", "mistral", "--no_tokenizer"])
    back = transformers.MistralForCausalLM.from_pretrained(str(tmp_path / "out")).float().eval()
    ref = hf.state_dict()
    got = back.state_dict()
    assert got.keys() == ref.keys()
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k
    assert _theta(back.config) == _theta(hf.config) == THETA
    for key in ("sliding_window", "num_key_value_heads", "num_attention_heads",
                "max_position_embeddings", "hidden_size", "intermediate_size",
                "num_hidden_layers", "vocab_size", "rms_norm_eps", "tie_word_embeddings"):
        assert getattr(back.config, key) == getattr(hf.config, key), key
    assert back.config.architectures == ["MistralForCausalLM"]


def test_converted_args_come_from_config(mistral_ckpt):
    from epfl_megatron_amd.convert.megatron_ckpt import load_full
    d, _, _ = mistral_ckpt
    args, _, _ = load_full(str(d / "mega"))
    assert (args.sliding_window_size, args.rope_theta, args.num_attention_heads_kv,
            args.max_position_embeddings, args.model_name) == (W, THETA, 2, 64, "mistral")


def _base_args(*extra):
    from epfl_megatron_amd.config.arguments import parse_args
    a = parse_args(None, ["--num_layers", "2", "--hidden_size", "64", "--num_attention_heads", "8",
                          "--seq_length", "32", "--max_position_embeddings", "32",
                          "--micro_batch_size", "1", "--attention_dropout", "0.0", *extra])
    a.rank = 0
    return a


def test_validate_args_window():
    from epfl_megatron_amd.config.arguments import validate_args
    a = _base_args("--sliding_window_size", "8", "--context_parallel_size", "2")
    a.world_size = 2
    with pytest.raises(AssertionError, match="context_parallel_size"):
        validate_args(a, {})
    a = _base_args("--sliding_window_size", "0")
    a.world_size = 1
    with pytest.raises(AssertionError, match="sliding_window_size"):
        validate_args(a, {})
    a = _base_args("--sliding_window_size", "8", "--decoder_seq_length", "16")
    a.world_size = 1
    with pytest.raises(AssertionError, match="causal"):
        validate_args(a, {})
    a = _base_args("--sliding_window_size", "8")
    a.world_size = 1
    validate_args(a, {})
    assert a.sliding_window_size == 8 and a.rope_theta == 10000.0
    a = _base_args()
    a.world_size = 1
    validate_args(a, {})
    assert a.sliding_window_size is None


def test_code_llama_checkpoint_theta(tmp_path):
    """A checkpoint whose args carry rope_theta = 1e6 (what the codellama
    conversion has always written) yields the 1e6 rotary table; one without
    the field keeps 10000."""
    from epfl_megatron_amd.checkpointing import load_args_from_checkpoint
    from epfl_megatron_amd.models.enums import PositionEmbeddingType
    from epfl_megatron_amd.models.transformer import ParallelAttention
    from epfl_megatron_amd.ops.rope import precompute_freqs

    def table(ck_args):
        d = tmp_path / f"ck{len(os.listdir(tmp_path))}"
        os.makedirs(d / "release" / "mp_rank_00")
        (d / "latest_checkpointed_iteration.txt").write_text("release")
        torch.save({"args": argparse.Namespace(**ck_args), "iteration": "release",
                    "checkpoint_version": 3.0},
                   str(d / "release" / "mp_rank_00" / "model_optim_rng.pt"))
        args = _base_args("--load", str(d))
        load_args_from_checkpoint(args)
        attn = types.SimpleNamespace(position_embedding_type=PositionEmbeddingType.rotary,
                                     hidden_size_per_attention_head=16, rope_len=32,
                                     rope_scaling=1.0, rope_theta=args.rope_theta)
        return args.rope_theta, ParallelAttention._rope(attn, "cpu")

    shape = dict(num_layers=2, hidden_size=64, num_attention_heads=8,
                 tensor_model_parallel_size=1, pipeline_model_parallel_size=1)
    theta, (cos, sin) = table(dict(shape, rope_theta=1e6))
    assert theta == 1e6
    ang = precompute_freqs(16, 32, theta=1e6)
    assert torch.equal(cos, torch.cos(ang)) and torch.equal(sin, torch.sin(ang))
    theta, (cos, _) = table(shape)
    assert theta == 10000.0
    assert torch.equal(cos, torch.cos(precompute_freqs(16, 32)))
