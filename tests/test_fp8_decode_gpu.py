"""FP8 weight-only decode on the GPU (``--inference_fp8_weights``): the e4m3
forms of the weight-streaming skinny GEMMs (csrc/skinny_gemm.hip, W8) against
their 16-bit packed twins and an fp32 reference, the fused decode layer end to
end, and the captured decode graph."""
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
    assert bad == 0, f"{msg}: {bad} elems off, max err {err.max().item():.3e}"


def _operands(M, N, K, dtype, seed):
    from epfl_megatron_amd.ops import fp8_weights as f8
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, dtype=dtype)
    g = (torch.rand(K, device=DEV) + 0.5).to(dtype)
    w = (torch.randn(N, K, device=DEV) * 0.02).to(dtype)
    w[3] = 0  # an all-zero row
    res = torch.randn(M, N, device=DEV, dtype=dtype)
    q, scale = f8.quantize_rows(w)
    return x, g, res, q, scale


def _qkv(C, x, w, g, ng, r, hd, packed, scale=None):
    """q and the written cache slots of one QKV + RoPE + cache call (device slot)."""
    from epfl_megatron_amd.ops.rope import rope_table
    M = x.shape[0]
    cos, sin = rope_table(hd, 64, DEV)
    pos = torch.arange(M, device=DEV).view(M, 1) + 3
    kc = torch.zeros(4, M, ng, hd, device=DEV, dtype=x.dtype)
    vc = torch.zeros_like(kc)
    st = torch.tensor([2], device=DEV)
    q = C.skinny_qkv_rope_cache(x, w, g, 1e-5, ng, r, hd, cos, sin, pos, kc, vc, st, 0, packed, scale)
    return q, kc, vc


def _bitwise_bundle(M, N, K, dtype, seed=0):
    """scale = ones: every FP8 binding equals the 16-bit packed kernel on
    q.to(dtype) bit for bit (same values, k order and roundings), with and
    without the RMSNorm prologue."""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8
    C = _ext()
    x, g, res, q, _ = _operands(M, N, K, dtype, seed)
    ones = torch.ones(N, device=DEV)
    w16 = q.to(dtype)
    p16, p8 = decode_pack.pack(w16), f8.pack_fp8(q)
    F = N // 2
    hd = N // 4  # one group of 2 q heads + k + v
    with torch.no_grad():
        assert torch.equal(C.skinny_gemm(x, p8, True, ones), C.skinny_gemm(x, p16, True)), "plain"
        for nw in (None, g):
            for r_ in (None, res):
                assert torch.equal(C.skinny_norm_gemm(x, p8, nw, 1e-5, r_, True, ones),
                                   C.skinny_norm_gemm(x, p16, nw, 1e-5, r_, True)), \
                    ("gemm", nw is not None, r_ is not None)
            tail = C.skinny_glu_half_tail(F, K, nw is not None, M)
            g16 = decode_pack.pack(w16, glu=True, half_tail=tail)
            g8 = f8.pack_fp8(q, glu=True, half_tail=tail)
            for kind in range(4):
                assert torch.equal(C.skinny_norm_glu(x, g8, nw, 1e-6, kind, True, tail, ones),
                                   C.skinny_norm_glu(x, g16, nw, 1e-6, kind, True, tail)), \
                    ("glu", nw is not None, kind, tail)
            a = _qkv(C, x, p8, nw, 1, 2, hd, True, ones)
            b = _qkv(C, x, p16, nw, 1, 2, hd, True)
            for u, v in zip(a, b):
                assert torch.equal(u, v), ("qkv", nw is not None)
            assert a[1].abs().sum() > 0 and a[2].abs().sum() > 0  # the slot was written


# K 512: 2 k-steps (leftover loop only); 768: 3 (an odd step, the 8-B piece);
# 11008: 43 (full ring blocks + leftover + the odd step); 4096 / 8192: the
# persistent kernel (8192 with 17-32 rows or the norm: per-block, 32 steps).
@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("N,K", [(256, 512), (256, 768), (64, 11008), (256, 4096), (512, 4096),
                                 (256, 8192)])
def test_fp8_kernels_bitwise_vs_16bit_packed(M, N, K):
    _bitwise_bundle(M, N, K, torch.bfloat16, seed=M + K)


@pytest.mark.parametrize("M,N,K", [(5, 256, 4096), (3, 256, 768), (20, 64, 11008)])
def test_fp8_kernels_bitwise_fp16(M, N, K):
    _bitwise_bundle(M, N, K, torch.float16, seed=7)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,K", [(3, 4096), (24, 4096), (8, 8192)])
def test_fp8_glu_half_unit_tail_bitwise(M, K, dtype):
    """F = 2816: 352 blocks = 256 + 96 on 256 CUs, so the persistent kernel
    runs the last round as 192 half units from the FP8 half-unit tail."""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8
    C = _ext()
    F = 2816
    x, g, _, q, _ = _operands(M, 2 * F, K, dtype, seed=M)
    ones = torch.ones(2 * F, device=DEV)
    w16 = q.to(dtype)
    with torch.no_grad():
        for nw in (None, g):
            tail = C.skinny_glu_half_tail(F, K, nw is not None, M)
            if C.skinny_glu_half_tail(F, 4096, True, 1) > 0 and (K == 4096 or nw is None):
                assert tail > 0  # the tail is there on this device
            g16 = decode_pack.pack(w16, glu=True, half_tail=tail)
            g8 = f8.pack_fp8(q, glu=True, half_tail=tail)
            for kind in (0, 1):
                assert torch.equal(C.skinny_norm_glu(x, g8, nw, 1e-6, kind, True, tail, ones),
                                   C.skinny_norm_glu(x, g16, nw, 1e-6, kind, True, tail)), \
                    (nw is not None, kind, tail)


@pytest.mark.parametrize("M", [3, 24])
@pytest.mark.parametrize("K", [512, 4096])
def test_fp8_kernels_scaled_vs_fp32(M, K):
    """Real per-row scales: plain and residual against (x q^T) scale in fp32;
    GLU and QKV against the unfused chain on the dequantised product."""
    from epfl_megatron_amd.ops import fp8_weights as f8
    from epfl_megatron_amd.ops.norms import rms_norm
    from epfl_megatron_amd.ops.activations import glu
    from epfl_megatron_amd.ops.rope import rope_table, rope_qkv_inplace
    C = _ext()
    N, dtype = 512, torch.bfloat16
    x, g, res, q, scale = _operands(M, N, K, dtype, seed=M + K)
    assert scale[3] == 1 and scale.min() > 0 and (scale != 1).sum() == N - 1
    p8 = f8.pack_fp8(q)
    with torch.no_grad():
        ref = (x.float() @ q.float().t()) * scale
        _close(C.skinny_gemm(x, p8, True, scale), ref, 2e-2, 2e-2, "plain")
        _close(C.skinny_norm_gemm(x, p8, None, 0.0, None, True, scale), ref, 2e-2, 2e-2, "plain (ex)")
        _close(C.skinny_norm_gemm(x, p8, None, 0.0, res, True, scale), ref + res.float(), 2e-2, 2e-2,
               "residual")
        # the dequantised product of the normed rows, rounded like the unfused GEMM's output
        xn = rms_norm(x, g, 1e-5)
        prod = ((xn.float() @ q.float().t()) * scale).to(dtype)
        F = N // 2
        tail = C.skinny_glu_half_tail(F, K, True, M)
        g8 = f8.pack_fp8(q, glu=True, half_tail=tail)
        for kind, name in enumerate(ACTS):
            _close(C.skinny_norm_glu(x, g8, g, 1e-5, kind, True, tail, scale), glu(prod, name),
                   2e-2, 2e-2, name)
        ng, r, hd = 1, 2, N // 4
        mixed = prod.clone().view(1, M, ng, r + 2, hd)
        cos, sin = rope_table(hd, 64, DEV)
        rope_qkv_inplace(mixed, cos, sin, torch.arange(M, device=DEV).view(M, 1) + 3)
        qo, kc, vc = _qkv(C, x, p8, g, ng, r, hd, True, scale)
        _close(qo, mixed[0, :, :, :r].reshape(M, -1), 2e-2, 2e-2, "q")
        _close(kc[2], mixed[0, :, :, r], 2e-2, 2e-2, "k slot")
        _close(vc[2], mixed[0, :, :, r + 1], 2e-2, 2e-2, "v slot")


def test_fp8_binding_checks():
    """With w_scale the weight must be packed e4m3 with one fp32 scale per row."""
    from epfl_megatron_amd.ops import fp8_weights as f8
    C = _ext()
    x, g, res, q, scale = _operands(2, 64, 512, torch.bfloat16, seed=0)
    p8 = f8.pack_fp8(q)
    for bad in (lambda: C.skinny_gemm(x, p8, False, scale),            # not packed
                lambda: C.skinny_gemm(x, q.to(torch.bfloat16), True, scale),  # 16-bit weight
                lambda: C.skinny_gemm(x, p8, True, scale[:32]),        # one scale per row
                lambda: C.skinny_gemm(x, p8, True, scale.double()),    # fp32
                lambda: C.skinny_gemm(x, p8, True)):                   # e4m3 without scales
        with pytest.raises(RuntimeError):
            bad()


class _CountScaled:
    """The extension module with a count of the skinny calls that pass a w_scale."""

    def __init__(self, C):
        self._C, self.scaled, self.plain = C, 0, 0

    def __getattr__(self, name):
        fn = getattr(self._C, name)
        if name not in ("skinny_norm_gemm", "skinny_norm_glu", "skinny_qkv_rope_cache"):
            return fn
        nargs = {"skinny_norm_gemm": 7, "skinny_norm_glu": 8, "skinny_qkv_rope_cache": 16}[name]

        def counted(*a):
            if len(a) == nargs and a[-1] is not None:
                assert a[-1].dtype == torch.float32 and a[1].dtype == torch.float8_e4m3fn
                self.scaled += 1
            else:
                self.plain += 1
            return fn(*a)
        return counted


def _fp8_layer_weights(m):
    from epfl_megatron_amd.models.transformer import ParallelTransformerLayer
    return [w for layer in m.modules() if isinstance(layer, ParallelTransformerLayer)
            for w in (layer.self_attention.query_key_value.weight, layer.self_attention.dense.weight,
                      layer.mlp.dense_h_to_4h.weight, layer.mlp.dense_4h_to_h.weight)]


def _fp8_vs_16bit_decode(rank, world, b, big):
    """The fused decode loop of ``_decode_fused_vs_unfused`` (prefill 21, 8
    steps) on fp8-representable weights, once through the 16-bit packs and
    once through the FP8 packs with power-of-two scales."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA, LLAMA_H8K
    from test_parallel_equivalence import _deterministic_init
    init_framework((LLAMA_H8K if big else LLAMA_GQA) + ["--bf16"], finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    args = get_args()
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, args)
    m = model[0].eval()
    ws = _fp8_layer_weights(m)
    assert len(ws) == 8
    with torch.no_grad():
        for w in ws:  # both runs see fp8-representable weights
            q, scale = f8.quantize_rows(w.detach(), pow2=True)
            w.copy_((q.float() * scale[:, None]).to(w.dtype))
    decode_pack.bump_weight_generation()
    counter = _CountScaled(transformer.ext())
    transformer.ext = lambda: counter
    f8.POW2_SCALES = True
    torch.manual_seed(6)
    plen, n = 21, 8
    prompt = torch.randint(0, 512, (b, plen), device="cuda")
    pos = torch.arange(plen + n, device="cuda")[None].expand(b, -1)
    runs, counts = {}, {}
    for fp8 in (False, True):
        transformer.set_fp8_weights(fp8)
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
        runs[fp8] = (torch.cat(logits, 1), torch.cat(toks, 1),
                     [t[:plen + n].clone() for kv in ip.key_value_memory_dict.values() for t in kv])
        counts[fp8] = (counter.scaled, counter.plain)
    transformer.set_fp8_weights(False)
    l8, t8, c8 = runs[True]
    l16, t16, c16 = runs[False]
    lerr = float((l8 - l16).abs().max())
    cerr = max(float((a.float() - c.float()).abs().max()) for a, c in zip(c8, c16))
    print("fp8 vs 16-bit decode: logits max |diff|", lerr, "cache max |diff|", cerr, "calls", counts)
    return (counts, torch.equal(l8, l16), lerr, float(l16.abs().max()), t8.cpu().tolist(),
            t16.cpu().tolist(), len(c8), all(torch.equal(a, c) for a, c in zip(c8, c16)), cerr)


@pytest.mark.parametrize("b,big", [(3, False), (24, False), (3, True), (24, True)])
def test_gpu_fp8_decode_layer_equals_16bit_on_fp8_weights(b, big):
    """With power-of-two scales every fp32 sum of the FP8 run is the 16-bit
    run's times an exact power of two, so logits, greedy tokens and KV caches
    are EQUAL; every one of the 4 products x 2 layers x 8 steps took a w_scale."""
    counts, same, lerr, scale, t8, t16, ncache, csame, cerr = \
        run_dist(_fp8_vs_16bit_decode, 1, b, big)[0]
    assert counts[True] == (4 * 2 * 8, 0) and counts[False] == (0, 4 * 2 * 8), counts
    assert ncache == 4
    assert same, (lerr, scale)
    assert t8 == t16
    assert csame, cerr


def _fp8_graph_decode(rank, world):
    """``_graph_decode`` with the flag on: GraphedGreedyDecoder vs the eager FP8 loop."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA
    from test_parallel_equivalence import _deterministic_init
    init_framework(LLAMA_GQA + ["--bf16", "--inference_fp8_weights"], finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    args = get_args()
    assert args.inference_fp8_weights
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    assert transformer._FP8_WEIGHTS  # the flag set the module switch
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
    packs = [w._ema_decode_packed_fp8 for w in _fp8_layer_weights(m)]
    before = [id(v[1][0]) for c in packs for v in c.values()]
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
    after = [id(v[1][0]) for c in packs for v in c.values()]
    lerr = float((dec.logits.float() - logits_e.float()).abs().max())
    return (graphed, again, eager.cpu().tolist(), lerr, float(logits_e.float().abs().max()),
            eager_calls, capture_calls, before == after)


def test_gpu_fp8_graph_greedy_decode_matches_eager_fp8():
    graphed, again, eager, lerr, scale, eager_calls, capture_calls, same_packs = \
        run_dist(_fp8_graph_decode, 1)[0]
    assert eager_calls == (4 * 2 * 10, 0), eager_calls  # the eager loop ran the FP8 forms
    # warm-up and capture took FP8 pairs only, and the ones the eager forward had built
    assert capture_calls[0] > 0 and capture_calls[1] == 0 and same_packs, capture_calls
    assert graphed == eager, (graphed, eager)
    assert again == eager
    assert lerr < 2e-2 * max(1.0, scale), (lerr, scale)
