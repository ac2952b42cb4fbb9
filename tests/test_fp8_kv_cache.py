"""FP8 KV cache on the CPU (``--inference_fp8_kv_cache``): the torch quantiser
of ``ops/fp8_kv.py`` (the reference transcription the HIP kernels are tested
against), the model path over a uint8 cache (store, dequantise, attend), the
beam reorder, the prompt calibration and the flags."""
import pytest
import torch

from dist_utils import run_dist, init_framework, TINY_LLAMA

from epfl_megatron_amd.ops import fp8_kv

E4M3 = torch.float8_e4m3fn


def _finite_codes():
    """All 254 finite e4m3fn codes (0x7f and 0xff are the NaNs)."""
    c = torch.arange(256, dtype=torch.int16)
    return c[(c & 0x7f) != 0x7f].to(torch.uint8)


def test_quantiser_matches_the_definition():
    """bytes == (x.float() * inv).clamp(-448, 448).to(e4m3fn) on inputs with
    values beyond +-448 scale, exact ties, the subnormal range and -0."""
    scale = torch.tensor([1.0, 0.25, 8.0, 2.0 ** -7])
    vals = torch.tensor([0.0, -0.0, 1.0, -1.0, 447.0, 448.0, 449.0, 464.0, 480.0, 1e4, -1e4, 3e38,
                         # ties between neighbouring codes (1 + k/8 steps: 1.0625, 1.1875 ...)
                         1.0625, 1.1875, -1.0625, 17.0, 19.0, 208.0 + 8.0, 240.0 - 8.0,
                         # subnormals: multiples of 2^-9 below 2^-6, their ties and below the least
                         2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, -2.0 ** -10,
                         7 * 2.0 ** -9, 7.5 * 2.0 ** -9, 2.0 ** -6, 1e-8, -1e-8])
    torch.manual_seed(0)
    x = torch.cat([vals, torch.randn(128 - vals.numel()) * 100])
    x = (x[None, None, :] * scale[None, :, None]).contiguous()  # [1, nkv = 4, hd = 128]: every value at every scale
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        q = fp8_kv.quantize(xd, scale)
        inv = 1.0 / scale
        want = (xd.float() * inv[:, None]).clamp(-448, 448).to(E4M3).view(torch.uint8)
        assert q.dtype == torch.uint8 and q.shape == xd.shape
        assert torch.equal(q, want), dt
    q = fp8_kv.quantize(x, scale)
    assert not ((q & 0x7f) == 0x7f).any()  # the clamp saturates: no NaN code from an overflow
    # spot values at scale 1: saturation, -0, a tie to even, the least subnormal
    one = fp8_kv.quantize(torch.tensor([[[1e4, -1e4, -0.0, 1.0625, 1.1875, 2.0 ** -9, 2.0 ** -10]]]),
                          torch.ones(1))[0, 0].tolist()
    assert one == [0x7e, 0xfe, 0x80, 0x38, 0x3a, 0x01, 0x00]


def test_dequantise_then_quantise_is_the_identity_on_all_codes():
    """With power-of-two scales every one of the 254 finite codes survives."""
    codes = _finite_codes()
    assert codes.numel() == 254
    scale = torch.tensor([1.0, 0.5, 2.0 ** -6, 16.0, 2.0 ** 7])  # 448 x 2^7 still fits fp16
    q = codes[None, :].expand(5, -1).contiguous()  # [nkv = 5, hd = 254]
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        x = fp8_kv.dequantize(q, scale, dt)
        assert x.dtype == dt and torch.isfinite(x.float()).all()
        assert torch.equal(fp8_kv.quantize(x, scale), q), dt
    x = fp8_kv.dequantize(q, scale)
    assert torch.equal(x, q.view(E4M3).float() * scale[:, None])


def test_calibration_rule():
    """2 amax / 448 rounded up to a power of two; 1.0 where amax == 0."""
    k = torch.zeros(3, 2, 4, 8)
    v = torch.zeros(3, 2, 4, 8)
    for g, a in enumerate((448.0, 100.0, 0.0, 1e-3)):
        k[1, 0, g, 3] = -a
        v[2, 1, g, 5] = 2 * a
    sc = fp8_kv.new_scales(4, "cpu")
    fp8_kv.calibrate_(sc, k, v)
    assert sc[0].tolist() == [2.0, 0.5, 1.0, 2.0 ** -17]  # 100 / 224 = 0.446 -> 0.5
    assert sc[1].tolist() == [4.0, 1.0, 1.0, 2.0 ** -16]


FP8_TINY = TINY_LLAMA + ["--num_attention_heads_kv", "2", "--micro_batch_size", "1",
                         "--global_batch_size", "1"]


def _teacher_forced(m, tokens, plen, ip):
    """Prefill ``plen`` tokens, then one token at a time: the logits of every step."""
    n = tokens.shape[1]
    pos = torch.arange(n, device=tokens.device)[None].expand(tokens.shape[0], -1)
    with torch.no_grad():
        outs = [m(tokens[:, :plen], pos[:, :plen], None, inference_params=ip).float()]
        ip.sequence_len_offset += plen
        for t in range(plen, n):
            outs.append(m(tokens[:, t:t + 1], pos[:, t:t + 1], None, inference_params=ip).float())
            ip.sequence_len_offset += 1
    return torch.cat(outs, 1)


def _cpu_model(rank, world, argv, flag_argv):
    import finetune
    from test_parallel_equivalence import _deterministic_init
    init_framework(argv + flag_argv, finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    args = get_args()
    assert not transformer._FP8_KV or flag_argv
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    switched = (transformer._FP8_KV, transformer._FP8_KV_CALIBRATE)
    _deterministic_init(model, args)
    m = model[0].eval()
    torch.manual_seed(11)
    b, plen, n = 3, 9, 4
    vocab = args.padded_vocab_size
    tokens = torch.randint(0, min(vocab, 250), (b, plen + n))
    out = {"switched": switched}
    for name, on, cal in (("ref", False, False), ("fp8", True, False), ("cal", True, True)):
        transformer.set_fp8_kv_cache(on, calibrate=cal)
        ip = InferenceParams(b, plen + n)
        logits = _teacher_forced(m, tokens, plen, ip)
        out[name] = {"logits": logits, "kv": {l: (k.clone(), v.clone())
                                              for l, (k, v) in ip.key_value_memory_dict.items()},
                     "scales": {l: s.clone() for l, s in ip.kv_scale_dict.items()}}
        if name == "fp8":
            perm = torch.tensor([2, 0, 1])
            before = ip.key_value_memory_dict[1][0].clone()
            ip.swap_key_value_dict(perm)
            k1 = ip.key_value_memory_dict[1][0]
            out["swap"] = (k1.dtype == torch.uint8 and torch.equal(k1, before[:, perm])
                           and not torch.equal(k1, before))
            ip.set_kv_scales(1, k_scale=[0.5, 2.0], v_scale=4.0)
            out["set"] = ip.kv_scale_dict[1].tolist()
    transformer.set_fp8_kv_cache(False, calibrate=False)
    return out


@pytest.fixture(scope="module")
def cpu_runs():
    return run_dist(_cpu_model, 1, FP8_TINY, [])[0]


def test_cpu_model_cache_is_uint8_and_half_the_bytes(cpu_runs):
    # (the CPU reference model keeps fp32 caches: compare with the 16-bit size)
    for layer, (k, v) in cpu_runs["fp8"]["kv"].items():
        rk, rv = cpu_runs["ref"]["kv"][layer]
        assert k.dtype == torch.uint8 and v.dtype == torch.uint8
        assert k.shape == rk.shape and v.shape == rv.shape
        assert 2 * k.numel() * k.element_size() == rk.numel() * 2
        sc = cpu_runs["fp8"]["scales"][layer]
        assert sc.dtype == torch.float32 and sc.shape == (2, k.shape[2]) and bool((sc == 1).all())
    assert not cpu_runs["ref"]["scales"]


def test_cpu_model_layer1_cache_bytes_are_the_quantised_cache(cpu_runs):
    """Layer 1's K and V depend only on the embeddings, so the FP8 run's bytes
    equal the quantised cache of the run without the flag: prefill and decode slots."""
    ones = torch.ones(2)
    for i in (0, 1):
        ref, got = cpu_runs["ref"]["kv"][1][i], cpu_runs["fp8"]["kv"][1][i]
        assert torch.equal(got, fp8_kv.quantize(ref, ones)), "kv"[i]
        assert (got[9:] != 0).any() and (got[:9] != 0).any()
    # and the logits stay close to the unquantised run (a wrong layout would not)
    lr, lf = cpu_runs["ref"]["logits"], cpu_runs["fp8"]["logits"]
    assert torch.equal(lr[:, :9], lf[:, :9])  # the restart prefill attends over its fresh K / V
    assert not torch.equal(lr[:, 9:], lf[:, 9:])
    assert float((lr - lf).abs().max()) < 0.1 * float(lr.abs().max())


def test_cpu_model_swap_and_setter(cpu_runs):
    assert cpu_runs["swap"]
    assert cpu_runs["set"] == [[0.5, 2.0], [4.0, 4.0]]


def test_cpu_model_calibration(cpu_runs):
    """Scales are powers of two with amax / scale <= 224 over the prompt (and
    above 112: the rule rounds up, no further), cache bytes follow them."""
    for layer, sc in cpu_runs["cal"]["scales"].items():
        m, _ = torch.frexp(sc)
        assert bool((m == 0.5).all()), sc
        for i in (0, 1):
            # the prompt rows of the calibrated run's own (dequantised) cache bound amax from
            # below; layer 1's exact amax comes from the run without the flag
            if layer == 1:
                amax = cpu_runs["ref"]["kv"][1][i][:9].abs().amax(dim=(0, 1, 3))
                ratio = amax / sc[i]
                assert bool((ratio <= 224).all()) and bool((ratio > 112).all()), ratio
                got = cpu_runs["cal"]["kv"][1][i]
                assert torch.equal(got, fp8_kv.quantize(cpu_runs["ref"]["kv"][1][i], sc[i]))
    assert any(bool((sc != 1).any()) for sc in cpu_runs["cal"]["scales"].values())


def test_flags_are_parsed_and_set_the_module_switches():
    from epfl_megatron_amd.config.arguments import FLAG_TABLE
    flags = dict(FLAG_TABLE["inference"])
    assert flags["--inference_fp8_kv_cache"]["action"] == "store_true"
    assert flags["--inference_fp8_kv_calibrate"]["action"] == "store_true"
    from epfl_megatron_amd.models import transformer
    assert transformer._FP8_KV is False and transformer._FP8_KV_CALIBRATE is False


def _flag_switch(rank, world):
    import finetune
    init_framework(FP8_TINY + ["--inference_fp8_kv_cache", "--inference_fp8_kv_calibrate"],
                   finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.training import get_model
    a = get_args()
    before = transformer._FP8_KV
    get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    return (a.inference_fp8_kv_cache, a.inference_fp8_kv_calibrate, before, transformer._FP8_KV,
            transformer._FP8_KV_CALIBRATE)


def test_flags_switch_the_model():
    assert run_dist(_flag_switch, 1)[0] == (True, True, False, True, True)
