"""The Falcon decode layer's kernel forms (csrc/skinny_gemm.hip, wide_gemm.hip):
the erf-GeLU epilogue bit for bit against gelu_fwd of the plain product, the
LayerNorm prologue against fp64 with the unfused route's own error as the
yardstick, the concatenated pack, and the four-launch layer end to end."""
import math

import pytest
import torch

from dist_utils import run_dist, init_framework
from epfl_megatron_amd.ops._ext import ext as _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _wforms(w):
    """{format: (16-bit weight the operand stands for, operand, packed, scales)}"""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8, mxfp4_weights as mx
    if w.shape[1] % 256:
        return {"row": (w, w, False, None)}
    q8, s8 = f8.quantize_rows(w, pow2=True)
    codes, exps = mx.quantize_blocks(w)
    p4, s4 = mx.pack_mxfp4(codes, exps)
    return {"row": (w, w, False, None), "pack": (w, decode_pack.pack(w), True, None),
            "fp8": ((q8.float() * s8[:, None]).to(w.dtype), f8.pack_fp8(q8), True, s8),
            "mxfp4": (mx.dequantize(codes, exps, w.dtype), p4, True, s4)}


@DTYPES
@pytest.mark.parametrize("M,N,K", [(M, N, K) for M in (1, 5, 16, 24) for N, K in
                                   ((48, 256), (32, 384), (0, 4096), (32, 8192))] +
                         [(33, 48, 512), (64, 48, 512)])
def test_act_epilogue_bitwise(dtype, M, N, K):
    """EPI_ACT == gelu_fwd of the plain product of the same layout (e4m3 / MXFP4:
    of the packed form on the dequantised weights), written into a wider buffer
    (ldy > N) whose other columns stay; 33 / 64 rows: the wide kernel, one shape."""
    from epfl_megatron_amd.ops import decode_pack
    C = _ext()
    wide = M > 32
    # N = 0: 16 (CUs + 3) features, a persistent workgroup's second block
    N = N or 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 3)
    torch.manual_seed(M + K)
    x = torch.randn(M, K, device=DEV, dtype=dtype)
    w = (torch.randn(N, K, device=DEV) * 0.05).to(dtype)
    for fmt, (w16, wop, packed, sc) in _wforms(w).items():
        buf = torch.full((M, N + 48), 7.0, device=DEV, dtype=dtype)
        out = buf[:, 16:16 + N]
        if wide and packed:
            ref = C.gelu_fwd(C.wide_gemm(x, decode_pack.pack(w16)), None, 1)
            C.wide_gemm(x, wop, None, sc, 0, out, True)
        elif not wide:
            ref = C.gelu_fwd(C.skinny_gemm(x, decode_pack.pack(w16) if packed else w16, packed), None, 1)
            C.skinny_norm_gemm(x, wop, None, 0.0, None, packed, sc, gelu=True, out=out)
        else:
            continue
        assert torch.equal(out, ref), fmt
        assert bool((buf[:, :16] == 7).all()) and bool((buf[:, 16 + N:] == 7).all()), fmt


def _ln_errors(x, w, fmt, g, bt, eps=1e-5, hd=64):
    """max |error| against fp64 (LN(x) W^T on the stored inputs, the normalised
    operand rounded once) of (in-kernel LayerNorm, layernorm op + un-normed form)
    for the plain, GeLU and QKV (q, written k / v cache row) outputs."""
    from epfl_megatron_amd.ops.rope import rope_table
    C = _ext()
    w16, wop, packed, sc = _wforms(w)[fmt]
    M, N = x.shape[0], w.shape[0]
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps)
    y = ((xd - mu) * rstd * g.double() + bt.double()).to(x.dtype).double() @ w16.double().t()
    ng, r = N // (4 * hd), 2
    cos, sin = rope_table(hd, 64, DEV)
    pos = torch.arange(M, device=DEV).view(M, 1) + 3
    c, s = cos[pos[:, 0]].double()[:, None, None], sin[pos[:, 0]].double()[:, None, None]
    h = y.view(M, ng, r + 2, hd // 2, 2).clone()
    a, b = h[:, :, :r + 1, :, 0].clone(), h[:, :, :r + 1, :, 1].clone()
    h[:, :, :r + 1, :, 0], h[:, :, :r + 1, :, 1] = a * c - b * s, a * s + b * c
    h = h.view(M, ng, r + 2, hd)
    refs = (y, 0.5 * y * (1 + torch.erf(y / math.sqrt(2))), h[:, :, :r].reshape(M, -1),
            h[:, :, r], h[:, :, r + 1])
    errs = []
    for nw, nb, xin in ((g, bt, x), (None, None, C.layernorm_fwd(x, g, bt, eps, None)[0])):
        kc = torch.zeros(4, M, ng, hd, device=DEV, dtype=x.dtype)
        vc = kc.clone()
        q = C.skinny_qkv_rope_cache(xin, wop, nw, eps, ng, r, hd, cos, sin, pos, kc, vc,
                                    torch.tensor([2], device=DEV), 0, packed, sc, norm_b=nb)
        outs = (C.skinny_norm_gemm(xin, wop, nw, eps, None, packed, sc, norm_b=nb),
                C.skinny_norm_gemm(xin, wop, nw, eps, None, packed, sc, norm_b=nb, gelu=True),
                q, kc[2], vc[2])
        errs.append([float((o.double() - ref).abs().max()) for o, ref in zip(outs, refs)])
    print("LayerNorm prologue (fused, unfused) max |err|:", list(zip(*errs)))
    return errs


# every kernel path row-major; packed / e4m3 / MXFP4 in the persistent (4096) and the per-block
# (8192) kernel; rows from {2048, 2064}: the mean is ~256 sigma, an fp32 E[x^2] - mu^2 has lost it
LN_CASES = [(M, K, "row", False) for M in (1, 5, 16) for K in (256, 384, 4096, 8192)] + \
    [(5, K, f, False) for K in (4096, 8192) for f in ("pack", "fp8", "mxfp4")] + \
    [(5, 4096, "row", True)]


@DTYPES
@pytest.mark.parametrize("M,K,fmt,centred", LN_CASES)
def test_layernorm_prologue_vs_fp64(dtype, M, K, fmt, centred):
    """Allowance: twice the unfused route's largest error on the same inputs."""
    torch.manual_seed(M + K)
    x = (torch.randn(M, K, device=DEV) * 2 + 0.5).to(dtype)
    if centred:
        x = (2048 + 16 * torch.randint(0, 2, (M, K), device=DEV)).to(dtype)
    w = (torch.randn(512, K, device=DEV) * 0.05).to(dtype)
    g = (torch.rand(K, device=DEV) + 0.5).to(dtype)
    bt = (torch.randn(K, device=DEV) * 0.2).to(dtype)
    fused, unfused = _ln_errors(x, w, fmt, g, bt)
    for f, u in zip(fused, unfused):
        assert f <= 2 * u, (fused, unfused)


def test_cat_pack_follows_both_parameters():
    """The cached pack of [wo | w2] is rebuilt when either parameter changes."""
    from epfl_megatron_amd.ops import decode_pack as dp, fp8_weights as f8, mxfp4_weights as mx
    wo, w2 = (torch.nn.Parameter(torch.randn(32, k).bfloat16()) for k in (256, 512))
    for cached, content in (
            (dp.packed, lambda p, c: torch.equal(dp.unpack(p), c)),
            (f8.packed_fp8, lambda p, c: torch.equal(f8.unpack_fp8(p[0]).view(torch.uint8),
                                                     f8.quantize_rows(c)[0].view(torch.uint8))),
            (mx.packed_mxfp4, lambda p, c: torch.equal(mx.unpack_mxfp4(*p)[0],
                                                       mx.quantize_blocks(c)[0]))):
        for changed in (None, wo, w2):
            with torch.no_grad():
                changed is None or changed.mul_(-0.5)
            p = cached(wo, cat=w2)
            assert content(p, torch.cat((wo, w2), 1).detach()), (cached.__name__, changed is wo)
            assert cached(wo, cat=w2) is p and cached(wo) is not p


def _falcon_decode(rank, world, extra, b):
    """Prefill + 8 decode steps on the tiny Falcon (b = 40: through the wide
    kernel): the fused parallel path and the EMA_DECODE_FUSED=0 path against an
    fp32 CPU run, lockstep and with per-row slots over a paged pool; the graphed
    greedy tokens; MXFP4 against 16-bit on the dequantised weights."""
    import copy
    import finetune
    from test_gpu_e2e import FALCON_MQA
    from test_paged_kv_gpu import _prefill
    from test_parallel_equivalence import _deterministic_init
    init_framework(FALCON_MQA + ["--bf16", "--no_tie_embed_logits"] + extra, finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType, transformer
    from epfl_megatron_amd.ops import decode_pack, mxfp4_weights as mx
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference import RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, get_args())
    m = model[0].eval()
    transformer._WIDE_GEMM = "1"  # (33-64 rows with 16-bit weights too)
    torch.manual_seed(6)
    # token v is followed by perm[v] (test_spec_decode.py), the embedding large beside
    # the layers' outputs: a wide top-1 / top-2 gap
    emb, perm = torch.randn(512, 256), torch.randperm(512)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("word_embeddings.weight"):
                p.copy_(8 * emb)
            elif name.endswith("lm_head"):
                p[perm] = emb.to(p)
    plen, n = 21, 8
    prompt = torch.randint(0, 512, (b, plen + 9), device="cuda")
    pos = torch.arange(plen + n, device="cuda")[None].expand(b, -1)
    steps = [torch.randint(0, 512, (b, 1), device="cuda") for _ in range(n)]
    cpu = copy.deepcopy(m).float().cpu()
    for mod in cpu.modules():  # fp32 KV cache too
        if hasattr(mod, "params_dtype"):
            mod.params_dtype = torch.float32
    calls = transformer.decode_parallel_calls

    def run(net, dev):  # lockstep, teacher-forced with `steps`
        with torch.no_grad():
            ip = InferenceParams(b, plen + n)
            net(prompt[:, :plen].to(dev), pos[:, :plen].to(dev), None, inference_params=ip)
            ip.sequence_len_offset += plen
            out = []
            for t in range(plen, plen + n):
                out.append(net(steps[t - plen].to(dev), pos[:, t:t + 1].to(dev), None,
                               inference_params=ip).float().cpu())
                ip.sequence_len_offset += 1
        return torch.cat(out, 1)

    def both(fn):  # fn with the switch on (and the fused layers it ran) and off
        before = calls["fused"]
        on = fn()
        ran = calls["fused"] - before
        transformer._DECODE_FUSED = False
        off = fn()
        transformer._DECODE_FUSED = True
        return on, off, ran
    fused, plain, ran = both(lambda: run(m, "cuda"))
    ref = run(cpu, "cpu")
    top = ref.topk(2, -1).values
    res = {"calls": ran, "err": (float((fused - ref).abs().max()), float((plain - ref).abs().max())),
           "gap": float((top[..., 0] - top[..., 1]).min())}

    # per-row slots over a paged pool: rows of different lengths, pages in reverse order
    lens = [plen + 3 * (row % 4) for row in range(b)]

    def ragged():
        ip = InferenceParams(b, 256, kv_pages=b + 1)
        dec = RaggedGreedyDecoder(m, ip, b, n)
        for row in range(b):
            dec.write_table(row, [b - row], lens[row] + n)
        first = [_prefill(m, ip, row, prompt[row, :lens[row]]) for row in range(b)]
        for row in range(b):
            dec.prime(row, first[row], lens[row], n)
        out = []
        for _ in range(n):
            dec.step()
            out.append(dec.logits[:, -1].float().cpu())
        return torch.stack(out, 1), [first[row:row + 1] + dec.history[row].tolist() for row in range(b)]
    (rf, tf), (rp, tp_), res["ragged_calls"] = both(ragged)
    rref, tref = [], []
    with torch.no_grad():
        for row in range(b):  # the fp32 greedy loop without a cache
            seq, lg = prompt[row, :lens[row]].tolist(), []
            for _ in range(n + 1):
                lg.append(cpu(torch.tensor([seq]), None, None)[0, -1])
                seq.append(int(lg[-1].argmax()))
            rref.append(torch.stack(lg[1:]))
            tref.append(seq[lens[row]:])
    rref = torch.stack(rref)
    res["ragged_err"] = (float((rf - rref).abs().max()), float((rp - rref).abs().max()))
    res["ragged_tokens"] = tf == tref and tp_ == tref

    def graphed():  # the captured greedy step
        with torch.no_grad():
            ip = InferenceParams(b, plen + n)
            first = m(prompt[:, :plen], pos[:, :plen], None, inference_params=ip)[:, -1] \
                .argmax(-1, keepdim=True)
            ip.sequence_len_offset += plen
            dec = GraphedGreedyDecoder(m, ip, b, n)
            dec.start(first, plen)
            for _ in range(n):
                dec.step()
        return dec.history[:, :n].tolist()
    on, off, _ = both(graphed)
    res["graph_tokens"] = on == off
    # on MXFP4-representable weights the W4 layer is the 16-bit layer bit for bit
    ws = [w for name, w in m.named_parameters() if "layers" in name and w.dim() == 2]
    with torch.no_grad():
        for w in ws:
            w.copy_(mx.dequantize(*mx.quantize_blocks(w.detach()), w.dtype))
    decode_pack.bump_weight_generation()
    l16 = run(m, "cuda")
    transformer.set_mxfp4_weights(True)
    l4 = run(m, "cuda")
    transformer.set_mxfp4_weights(False)
    res["mxfp4"] = len(ws) == 8 and all(hasattr(w, "_ema_decode_packed_mxfp4") for w in ws[:3]) \
        and torch.equal(l4, l16)
    return res


@pytest.mark.parametrize("extra,b", [([], 2), (["--parallel_layernorm"], 2),
                                     (["--parallel_layernorm"], 40)], ids=["ln1", "ln2", "ln2-wide"])
def test_gpu_falcon_decode_layer(extra, b):
    r = run_dist(_falcon_decode, 1, extra, b)[0]
    print("falcon decode (fused, unfused) |logit err|:", r["err"], "paged", r["ragged_err"], r["gap"])
    assert r["calls"] == 2 * 8  # both layers, every step
    assert r["ragged_calls"] == 2 * 2  # both layers, the warm-up and the capture
    for f, u in (r["err"], r["ragged_err"]):
        assert f <= 2 * u, r
    assert r["gap"] > 20 * r["err"][1] and r["graph_tokens"] and r["ragged_tokens"], r
    assert r["mxfp4"]
