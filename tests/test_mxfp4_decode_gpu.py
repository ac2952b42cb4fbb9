"""MXFP4 weight-only decode on the GPU (``--inference_mxfp4_weights``): the W4
forms of the weight-streaming skinny GEMMs (csrc/skinny_gemm.hip) against
their 16-bit packed twins on the dequantised weights (bit equality, real block
scales) and an fp32 reference, the fused decode layer end to end, and the
captured decode graph."""
import pytest
import torch

from dist_utils import run_dist, init_framework

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACTS = ["swiglu", "geglu", "reglu", "liglu"]  # kinds 0-3 (tp.layers._GLU_KIND)


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (~(err <= tol)).sum().item()  # NaN / inf count as off
    print(f"{msg}: max err {err.max().item():.3e}, max err / tol {(err / tol).max().item():.3f}")
    assert bad == 0, f"{msg}: {bad} elems off, max err {err.max().item():.3e}"


def _operands(M, N, K, dtype, seed):
    """x, gamma, residual and the quantiser's own (codes, exps) of a Gaussian
    weight with an all-zero row and one block scaled by 2^-10 (under fp16 its
    exponent sits on the clamp)."""
    from epfl_megatron_amd.ops import mxfp4_weights as mx
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, dtype=dtype)
    g = (torch.rand(K, device=DEV) + 0.5).to(dtype)
    w = (torch.randn(N, K, device=DEV) * 0.02).to(dtype)
    w[3] = 0
    w[5, 32:64] *= 2.0 ** -10
    res = torch.randn(M, N, device=DEV, dtype=dtype)
    codes, exps = mx.quantize_blocks(w)
    assert int(exps[3].min()) == 127 and int(exps[3].max()) == 127 and int(codes[3].max()) == 0
    # the small block's exponent: about 10 below its neighbour's, or fp16's lower clamp
    assert int(exps[5, 1]) <= max(int(exps[5, 0]) - 9, 127 - 13)
    assert dtype == torch.float16 or int(codes[5, 32:64].max()) > 0
    assert exps.unique().numel() > 2  # real scales
    return x, g, res, codes, exps


def _qkv(C, x, w, g, ng, r, hd, packed, scale=None, kv_scale=None):
    """q and the written cache slots of one QKV + RoPE + cache call (device slot)."""
    from epfl_megatron_amd.ops.rope import rope_table
    M = x.shape[0]
    cos, sin = rope_table(hd, 64, DEV)
    pos = torch.arange(M, device=DEV).view(M, 1) + 3
    if kv_scale is None:
        kc = torch.zeros(4, M, ng, hd, device=DEV, dtype=x.dtype)
    else:
        kc = torch.full((4, M, ng, hd), 0xA5, device=DEV, dtype=torch.uint8)
    vc = kc.clone()
    st = torch.tensor([2], device=DEV)
    q = C.skinny_qkv_rope_cache(x, w, g, 1e-5, ng, r, hd, cos, sin, pos, kc, vc, st, 0, packed, scale,
                                *(() if kv_scale is None else (kv_scale,)))
    return q, kc, vc


def _bitwise_bundle(M, N, K, dtype, seed=0):
    """Every MXFP4 binding equals the 16-bit packed kernel on
    dequantize(codes, exps) bit for bit (same values, k order and roundings),
    with and without the RMSNorm prologue."""
    from epfl_megatron_amd.ops import decode_pack, mxfp4_weights as mx
    C = _ext()
    x, g, res, codes, exps = _operands(M, N, K, dtype, seed)
    w16 = mx.dequantize(codes, exps, dtype)
    p16 = decode_pack.pack(w16)
    p4, s4 = mx.pack_mxfp4(codes, exps)
    F = N // 2
    hd = N // 4  # one group of 2 q heads + k + v
    with torch.no_grad():
        assert torch.equal(C.skinny_gemm(x, p4, True, s4), C.skinny_gemm(x, p16, True)), "plain"
        for nw in (None, g):
            for r_ in (None, res):
                assert torch.equal(C.skinny_norm_gemm(x, p4, nw, 1e-5, r_, True, s4),
                                   C.skinny_norm_gemm(x, p16, nw, 1e-5, r_, True)), \
                    ("gemm", nw is not None, r_ is not None)
            tail = C.skinny_glu_half_tail(F, K, nw is not None, M)
            g16 = decode_pack.pack(w16, glu=True, half_tail=tail)
            g4, gs4 = mx.pack_mxfp4(codes, exps, glu=True, half_tail=tail)
            for kind in range(4):
                assert torch.equal(C.skinny_norm_glu(x, g4, nw, 1e-6, kind, True, tail, gs4),
                                   C.skinny_norm_glu(x, g16, nw, 1e-6, kind, True, tail)), \
                    ("glu", nw is not None, kind, tail)
            a = _qkv(C, x, p4, nw, 1, 2, hd, True, s4)
            b = _qkv(C, x, p16, nw, 1, 2, hd, True)
            for u, v in zip(a, b):
                assert torch.equal(u, v), ("qkv", nw is not None)
            assert a[1].abs().sum() > 0 and a[2].abs().sum() > 0  # the slot was written


# K 512 / 768: 2 / 3 k-steps (leftover pieces only); 1024: one four-step slot;
# 11008: 43 (full ring blocks + slots in the leftover loop + 3 leftover pieces);
# 4096 / 8192: the persistent kernel, both depths (8192 with 17-32 rows or the
# norm: per-block, 32 steps = whole ring blocks); N 256 / 512: 16 / 32 blocks.
@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("N,K", [(256, 512), (256, 768), (256, 1024), (64, 11008), (256, 4096),
                                 (512, 4096), (256, 8192)])
def test_mxfp4_kernels_bitwise_vs_16bit_packed(M, N, K):
    _bitwise_bundle(M, N, K, torch.bfloat16, seed=M + K)


@pytest.mark.parametrize("M,N,K", [(5, 256, 4096), (3, 256, 768), (20, 64, 11008)])
def test_mxfp4_kernels_bitwise_fp16(M, N, K):
    _bitwise_bundle(M, N, K, torch.float16, seed=7)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M", [3, 24])
@pytest.mark.parametrize("K", [4096, 8192])
def test_mxfp4_glu_half_unit_tail_bitwise(M, K, dtype):
    """F = 2816: 352 blocks = 256 + 96 on 256 CUs, so the persistent kernel
    runs the last round as 192 half units from the MXFP4 half-unit tail."""
    from epfl_megatron_amd.ops import decode_pack, mxfp4_weights as mx
    C = _ext()
    F = 2816
    x, g, _, codes, exps = _operands(M, 2 * F, K, dtype, seed=M)
    w16 = mx.dequantize(codes, exps, dtype)
    with torch.no_grad():
        for nw in (None, g):
            tail = C.skinny_glu_half_tail(F, K, nw is not None, M)
            if C.skinny_glu_half_tail(F, 4096, True, 1) > 0 and \
                    (K == 4096 or (nw is None and M <= 16)):
                assert tail > 0  # the tail is there on this device
            g16 = decode_pack.pack(w16, glu=True, half_tail=tail)
            g4, gs4 = mx.pack_mxfp4(codes, exps, glu=True, half_tail=tail)
            for kind in (0, 1):
                assert torch.equal(C.skinny_norm_glu(x, g4, nw, 1e-6, kind, True, tail, gs4),
                                   C.skinny_norm_glu(x, g16, nw, 1e-6, kind, True, tail)), \
                    (nw is not None, kind, tail)


@pytest.mark.parametrize("M", [3, 24])
@pytest.mark.parametrize("K", [512, 4096])
def test_mxfp4_kernels_vs_fp32(M, K):
    """Plain and residual against x dequantize(codes, exps)^T in fp32 (this
    decides the nibble order: the reference is the quantiser's own
    dequantisation, not a kernel); GLU and QKV against the unfused chain."""
    from epfl_megatron_amd.ops import mxfp4_weights as mx
    from epfl_megatron_amd.ops.norms import rms_norm
    from epfl_megatron_amd.ops.activations import glu
    from epfl_megatron_amd.ops.rope import rope_table, rope_qkv_inplace
    C = _ext()
    N, dtype = 512, torch.bfloat16
    x, g, res, codes, exps = _operands(M, N, K, dtype, seed=M + K)
    deq = mx.dequantize(codes, exps, dtype)
    p4, s4 = mx.pack_mxfp4(codes, exps)
    with torch.no_grad():
        ref = x.float() @ deq.float().t()
        _close(C.skinny_gemm(x, p4, True, s4), ref, 2e-2, 2e-2, "plain")
        _close(C.skinny_norm_gemm(x, p4, None, 0.0, None, True, s4), ref, 2e-2, 2e-2, "plain (ex)")
        _close(C.skinny_norm_gemm(x, p4, None, 0.0, res, True, s4), ref + res.float(), 2e-2, 2e-2,
               "residual")
        # the product of the normed rows, rounded like the unfused GEMM's output
        xn = rms_norm(x, g, 1e-5)
        prod = (xn.float() @ deq.float().t()).to(dtype)
        F = N // 2
        tail = C.skinny_glu_half_tail(F, K, True, M)
        g4, gs4 = mx.pack_mxfp4(codes, exps, glu=True, half_tail=tail)
        for kind, name in enumerate(ACTS):
            _close(C.skinny_norm_glu(x, g4, g, 1e-5, kind, True, tail, gs4), glu(prod, name),
                   2e-2, 2e-2, name)
        ng, r, hd = 1, 2, N // 4
        mixed = prod.clone().view(1, M, ng, r + 2, hd)
        cos, sin = rope_table(hd, 64, DEV)
        rope_qkv_inplace(mixed, cos, sin, torch.arange(M, device=DEV).view(M, 1) + 3)
        qo, kc, vc = _qkv(C, x, p4, g, ng, r, hd, True, s4)
        _close(qo, mixed[0, :, :, :r].reshape(M, -1), 2e-2, 2e-2, "q")
        _close(kc[2], mixed[0, :, :, r], 2e-2, 2e-2, "k slot")
        _close(vc[2], mixed[0, :, :, r + 1], 2e-2, 2e-2, "v slot")


@pytest.mark.parametrize("M,K", [(5, 4096), (20, 768)])
def test_mxfp4_qkv_with_fp8_kv_cache(M, K):
    """The FP8-KV-cache QKV epilogue on top of the W4 forms: q and the e4m3
    cache bytes equal the 16-bit packed kernel's with the same kv_scale."""
    from epfl_megatron_amd.ops import decode_pack, mxfp4_weights as mx
    C = _ext()
    ng, r, hd = 2, 2, 64
    N = ng * (r + 2) * hd
    x, g, _, codes, exps = _operands(M, N, K, torch.bfloat16, seed=M)
    nw = g if M <= 16 else None
    p16 = decode_pack.pack(mx.dequantize(codes, exps, torch.bfloat16))
    p4, s4 = mx.pack_mxfp4(codes, exps)
    kvs = torch.tensor([[2.0 ** -6, 2.0 ** -4], [2.0 ** -5, 2.0 ** -7]], device=DEV)
    with torch.no_grad():
        a = _qkv(C, x, p4, nw, ng, r, hd, True, s4, kvs)
        b = _qkv(C, x, p16, nw, ng, r, hd, True, None, kvs)
    assert a[1].dtype == torch.uint8
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bool((a[1][2] != 0xA5).any()) and bool((a[2][2] != 0xA5).any())  # the slot was written
    assert bool((a[1][[0, 1, 3]] == 0xA5).all()) and bool((a[2][[0, 1, 3]] == 0xA5).all())


def test_mxfp4_binding_checks():
    """uint8 scales select MXFP4: the weight must be the packed uint8 nibbles
    with one scale byte per 32 weights."""
    from epfl_megatron_amd.ops import mxfp4_weights as mx
    C = _ext()
    x, g, res, codes, exps = _operands(2, 64, 512, torch.bfloat16, seed=0)
    p4, s4 = mx.pack_mxfp4(codes, exps)
    w16 = mx.dequantize(codes, exps, torch.bfloat16)
    assert C.skinny_gemm(x, p4, True, s4).shape == (2, 64)
    for bad in (lambda: C.skinny_gemm(x, p4, False, s4),             # not packed
                lambda: C.skinny_gemm(x, w16, True, s4),             # 16-bit weight, uint8 scales
                lambda: C.skinny_gemm(x, p4, True, s4[:-32]),        # one scale per 32 weights
                lambda: C.skinny_gemm(x, p4, True, torch.cat((s4, s4))),
                lambda: C.skinny_gemm(x, p4, True),                  # nibbles without scales
                lambda: C.skinny_norm_gemm(x, p4, None, 0.0, None, False, s4),
                lambda: C.skinny_norm_gemm(x, w16, None, 0.0, None, True, s4),
                lambda: C.skinny_norm_gemm(x, p4, None, 0.0, None, True, s4[:-32]),
                lambda: C.skinny_norm_gemm(x, p4, None, 0.0, None, True)):
        with pytest.raises(RuntimeError):
            bad()


class _CountScaled:
    """The extension module with a count of the skinny calls that pass uint8 scales."""

    def __init__(self, C):
        self._C, self.scaled, self.plain = C, 0, 0

    def __getattr__(self, name):
        fn = getattr(self._C, name)
        if name not in ("skinny_norm_gemm", "skinny_norm_glu", "skinny_qkv_rope_cache"):
            return fn
        nargs = {"skinny_norm_gemm": 7, "skinny_norm_glu": 8, "skinny_qkv_rope_cache": 16}[name]

        def counted(*a):
            if len(a) == nargs and a[-1] is not None:
                assert a[-1].dtype == torch.uint8 and a[1].dtype == torch.uint8
                self.scaled += 1
            else:
                self.plain += 1
            return fn(*a)
        return counted


def _layer_weights(m):
    from epfl_megatron_amd.models.transformer import ParallelTransformerLayer
    return [w for layer in m.modules() if isinstance(layer, ParallelTransformerLayer)
            for w in (layer.self_attention.query_key_value.weight, layer.self_attention.dense.weight,
                      layer.mlp.dense_h_to_4h.weight, layer.mlp.dense_4h_to_h.weight)]


def _mxfp4_vs_16bit_decode(rank, world, b, big):
    """The fused decode loop (prefill 21, 8 steps) on MXFP4-representable
    weights, once through the 16-bit packs and once through the MXFP4 pairs."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA, LLAMA_H8K
    from test_parallel_equivalence import _deterministic_init
    init_framework((LLAMA_H8K if big else LLAMA_GQA) + ["--bf16"], finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.ops import decode_pack, mxfp4_weights as mx
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    args = get_args()
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, args)
    m = model[0].eval()
    ws = _layer_weights(m)
    assert len(ws) == 8
    with torch.no_grad():
        for w in ws:  # both runs see the dequantised MXFP4 values
            w.copy_(mx.dequantize(*mx.quantize_blocks(w.detach()), w.dtype))
    decode_pack.bump_weight_generation()
    counter = _CountScaled(transformer.ext())
    transformer.ext = lambda: counter
    torch.manual_seed(6)
    plen, n = 21, 8
    prompt = torch.randint(0, 512, (b, plen), device="cuda")
    pos = torch.arange(plen + n, device="cuda")[None].expand(b, -1)
    runs, counts = {}, {}
    for on in (False, True):
        transformer.set_mxfp4_weights(on)
        counter.scaled = counter.plain = 0
        with torch.no_grad():
            ip = InferenceParams(b, plen + n)
            nxt = m(prompt, pos[:, :plen], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
            ip.sequence_len_offset += plen
            logits, toks = [], []
            for t in range(plen, plen + n):
                lg = m(nxt, pos[:, t:t + 1], None, inference_params=ip).float()
                nxt = lg[:, -1].argmax(-1, keepdim=True)
                logits.append(lg)
                toks.append(nxt)
                ip.sequence_len_offset += 1
        runs[on] = (torch.cat(logits, 1), torch.cat(toks, 1),
                    [t[:plen + n].clone() for kv in ip.key_value_memory_dict.values() for t in kv])
        counts[on] = (counter.scaled, counter.plain)
    transformer.set_mxfp4_weights(False)
    l4, t4, c4 = runs[True]
    l16, t16, c16 = runs[False]
    lerr = float((l4 - l16).abs().max())
    cerr = max(float((a.float() - c.float()).abs().max()) for a, c in zip(c4, c16))
    print("mxfp4 vs 16-bit decode: logits max |diff|", lerr, "cache max |diff|", cerr, "calls", counts)
    return (counts, torch.equal(l4, l16), lerr, float(l16.abs().max()), t4.cpu().tolist(),
            t16.cpu().tolist(), len(c4), all(torch.equal(a, c) for a, c in zip(c4, c16)), cerr)


@pytest.mark.parametrize("b,big", [(3, False), (24, False), (3, True), (24, True)])
def test_gpu_mxfp4_decode_layer_equals_16bit_on_mxfp4_weights(b, big):
    """The W4 forms compute what the 16-bit forms compute on the dequantised
    weights, so logits, greedy tokens and KV caches are EQUAL; every one of the
    4 products x 2 layers x 8 steps took uint8 scales with the switch on and
    none with it off."""
    counts, same, lerr, scale, t4, t16, ncache, csame, cerr = \
        run_dist(_mxfp4_vs_16bit_decode, 1, b, big)[0]
    assert counts[True] == (4 * 2 * 8, 0) and counts[False] == (0, 4 * 2 * 8), counts
    assert ncache == 4
    assert same, (lerr, scale)
    assert t4 == t16
    assert csame, cerr


def _mxfp4_graph_decode(rank, world):
    """GraphedGreedyDecoder with the flag on against the eager MXFP4 loop."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA
    from test_parallel_equivalence import _deterministic_init
    init_framework(LLAMA_GQA + ["--bf16", "--inference_mxfp4_weights"], finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    args = get_args()
    assert args.inference_mxfp4_weights and not args.inference_fp8_weights
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    assert transformer._MXFP4_WEIGHTS and not transformer._FP8_WEIGHTS  # the flag set the module switch
    _deterministic_init(model, args)
    m = model[0].eval()
    counter = _CountScaled(transformer.ext())
    transformer.ext = lambda: counter
    torch.manual_seed(5)
    b, plen, n, cap = 2, 29, 10, 600
    prompt = torch.randint(0, 512, (b, plen), device="cuda")
    pos = torch.arange(cap, device="cuda")[None].expand(b, -1)
    with torch.no_grad():
        ip = InferenceParams(b, cap)
        nxt = m(prompt, pos[:, :plen], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
        ip.sequence_len_offset += plen
        first = nxt.clone()
        eager = []
        for t in range(plen, plen + n):
            logits_e = m(nxt, pos[:, t:t + 1], None, inference_params=ip)
            nxt = logits_e[:, -1].argmax(-1, keepdim=True)
            eager.append(nxt)
            ip.sequence_len_offset += 1
        eager = torch.cat(eager, dim=1)
        eager_calls = (counter.scaled, counter.plain)
        ip2 = InferenceParams(b, cap)
        m(prompt, pos[:, :plen], None, inference_params=ip2)
        ip2.sequence_len_offset += plen
    packs = [w._ema_decode_packed_mxfp4 for w in _layer_weights(m)]
    before = [id(t) for c in packs for v in c.values() for t in v[1]]
    counter.scaled = counter.plain = 0
    dec = GraphedGreedyDecoder(m, ip2, b, n)
    dec.start(first, plen)  # the eager warm-up forward and the capture
    capture_calls = (counter.scaled, counter.plain)
    for _ in range(n):
        dec.step()
    torch.cuda.synchronize()
    graphed = dec.history[:, :n].cpu().tolist()
    dec.start(first, plen)  # a second generation through the same graph
    for _ in range(n):
        dec.step()
    again = dec.history[:, :n].cpu().tolist()
    after = [id(t) for c in packs for v in c.values() for t in v[1]]
    lerr = float((dec.logits.float() - logits_e.float()).abs().max())
    return (graphed, again, eager.cpu().tolist(), lerr, float(logits_e.float().abs().max()),
            eager_calls, capture_calls, before == after and len(before) == 16)


def test_gpu_mxfp4_graph_greedy_decode_matches_eager_mxfp4():
    graphed, again, eager, lerr, scale, eager_calls, capture_calls, same_packs = \
        run_dist(_mxfp4_graph_decode, 1)[0]
    assert eager_calls == (4 * 2 * 10, 0), eager_calls  # the eager loop ran the MXFP4 forms
    # warm-up and capture took MXFP4 pairs only, and the ones the eager forward had built
    assert capture_calls[0] > 0 and capture_calls[1] == 0 and same_packs, capture_calls
    assert graphed == eager, (graphed, eager)
    assert again == eager
    assert lerr < 2e-2 * max(1.0, scale), (lerr, scale)
