"""The multi-row device step through the fused decode layer (``ip.device_multi =
"fused"``): the multi-row geometry of the QKV epilogue (``SkinnyArgs::seqs``,
csrc/skinny_epi.h) bit for bit against fp64 in both GEMM families, the cache
cell, the model step against the fp32 CPU model, the decoder with ``fused=True``."""
import contextlib
import functools

import pytest
import torch

import gemm_exact_inputs as G
from dist_utils import run_dist
from test_decode_mq_gpu import NEW, PROMPT
from test_spec_sample import TABLE

pytestmark = pytest.mark.gpu
DEV, NG, L, SENTINEL = "cuda", 2, 24, 7
PAGES = TABLE + ((0, 8), (9, 7))  # five sequences: neither adjacent nor in order


def _weights(w, form, dt):
    """(weight operand, packed flag, scale operand, the values it stands for)."""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8, mxfp4_weights as mx
    if form == "e4m3":
        q8, s8 = f8.quantize_rows(w, pow2=True)
        return f8.pack_fp8(q8, False), True, s8, (q8.float() * s8[:, None]).to(dt)
    if form == "mxfp4":
        codes, exps = mx.quantize_blocks(w)
        wp, ws = mx.pack_mxfp4(codes, exps, False)
        return wp, True, ws, mx.dequantize(codes, exps, dt)
    return (decode_pack.pack(w), True, None, w) if form == "packed" else (w, False, None, w)


def _epilogue_case(b, sq, layout, fp8, hd, r, dt, K, forms, norm=False):
    from epfl_megatron_amd.inference.paged import KV_PAGE
    from epfl_megatron_amd.ops import fp8_kv
    from epfl_megatron_amd.ops._ext import ext
    C, M, N, paged = ext(), sq * b, NG * (r + 2) * hd, layout == "paged"
    x, w, _ = G.skinny_case(M, N, K, dt, DEV)
    gamma = torch.ones(K, dtype=dt, device=DEV) if norm else None
    if norm:  # rows of +-1 with gamma 1 and eps 0: the RMSNorm prologue returns x
        x = torch.where(x == 0, torch.ones_like(x), x.sign())
    if paged:  # first positions mid-page, on a page's last row (the rows cross its edge), 0, ...
        first = (7, KV_PAGE - 1, 0, KV_PAGE - 3, 3)[:b]
        phys = lambda m, p: PAGES[m][p // KV_PAGE] * KV_PAGE + p % KV_PAGE
        slots = [phys(m, p) for m, p in enumerate(first)]
        # where[(t, m)] = (cache row, column) of the rows that are stored
        where = {(t, m): (phys(m, p + t), 0) for m, p in enumerate(first) for t in range(sq)}
    else:  # sequence 1 starts two rows before the cache's end: its later rows are dropped
        first = (9,) * b if layout == "one_slot" else (7, L - 2, 0, 11, 5)[:b]
        slots = list(first[:1] if layout == "one_slot" else first)
        where = {(t, m): (p + t, m) for m, p in enumerate(first) for t in range(sq) if p + t < L}
    # rotary tables of quarter turns: cos / sin in {0, +-1}, the rotation is exact
    quad = (torch.arange(2 * KV_PAGE)[:, None] + torch.arange(hd // 2)[None]) % 4
    cos, sin = torch.tensor([1., 0., -1., 0.])[quad], torch.tensor([0., 1., 0., -1.])[quad]
    pos = torch.tensor(first)[:, None] + torch.arange(sq)[None]  # [b, sq]
    scales = torch.tensor([[0.125, 2.0], [4.0, 0.25]]) if fp8 else None  # K past +-448 in group 0
    shape = (len(PAGES) * 2 * KV_PAGE, 1, NG, hd) if paged else (L, b, NG, hd)
    for form in forms:
        wop, packed, ws, wval = _weights(w, form, dt)
        # fp64 reference: x W^T rounded once, quarter-turn rotation, placement
        acc = G.expect16(G.ref_nt(x, wval), dt).cpu().double().view(sq, b, NG, r + 2, hd)
        c, s = (t[pos].transpose(0, 1)[:, :, None, None].double() for t in (cos, sin))
        rot = acc.clone()
        x0, x1 = acc[..., :r + 1, 0::2], acc[..., :r + 1, 1::2]
        rot[..., :r + 1, 0::2], rot[..., :r + 1, 1::2] = x0 * c - x1 * s, x0 * s + x1 * c
        want_q = rot[..., :r, :].reshape(M, -1).to(dt)
        new = [rot[..., r + i, :].to(dt) for i in (0, 1)]  # k, v [sq, b, NG, hd]
        if fp8:
            new = [fp8_kv.quantize(t, scales[i]) for i, t in enumerate(new)]
        want = [torch.full(shape, SENTINEL, dtype=new[0].dtype) for _ in (0, 1)]
        for (t, m), (row, col) in where.items():
            for cache, rows in zip(want, new):
                cache[row, col] = rows[t, m]
        caches = [torch.full(shape, SENTINEL, dtype=new[0].dtype, device=DEV) for _ in (0, 1)]
        tail = (None if scales is None else scales.to(DEV), b,
                torch.tensor([p + sq for p in first], dtype=torch.int32, device=DEV) if paged else None,
                torch.tensor(PAGES[:b], dtype=torch.int32, device=DEV) if paged else None)
        args = (NG, r, hd, cos.to(DEV), sin.to(DEV), pos.to(DEV),
                *(t.expand(-1, b, -1, -1) if paged else t for t in caches), torch.tensor(slots, device=DEV), 0)
        if M > 32:
            q = C.wide_qkv_rope_cache(x, wop, *args, ws, tail[0], 0, *tail[1:])
        else:
            q = C.skinny_qkv_rope_cache(x, wop, gamma, 0.0, *args, packed, ws, *tail)
        assert G.exact_ok(q.cpu(), want_q), (form, G.first_mismatch(q.cpu(), want_q))
        for got, exp in zip(caches, want):  # the written cells, and the sentinel everywhere else
            assert torch.equal(got.cpu(), exp), (form, G.first_mismatch(got.cpu(), exp))


ALL, QUANT = ("plain", "packed", "e4m3", "mxfp4"), ("e4m3", "mxfp4")
# 12, 24 and 40 rows at K = 256: the per-block kernel with one and two row blocks and the wide one,
# sequences across the 16-row seams; then the persistent (K = 4096), normed and quantised forms
CASES = [(b, sq, lay, f8, *h, 256, ("packed",) if b * sq > 32 else ALL[:2], False)
         for b, sq in ((3, 4), (3, 8), (5, 8)) for lay in ("columns", "one_slot", "paged")
         for f8 in (False, True) for h in ((64, 4, G.BF16), (128, 1, G.FP16))] + \
    [(b, sq, lay, f8, 128, 1, G.BF16, K, forms, norm) for lay, f8 in (("columns", True), ("paged", False))
     for b, sq, K, forms, norm in ((3, 4, 4096, ALL, False), (3, 8, 4096, ALL, False), (3, 4, 4096, ALL[:2], True),
                                   (3, 4, 256, ALL[1:2], True), (3, 8, 256, QUANT, False), (5, 8, 256, QUANT, False))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1] for v in c[:8]) + "-n" * c[9])
def test_epilogue_places_every_row_exactly(case):
    _epilogue_case(*case)


@pytest.mark.parametrize("value,ok", [("fused", True), (True, False)])
def test_cell_takes_the_fused_layer_only_under_its_value(value, ok):
    from epfl_megatron_amd.inference import kv_cache
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    ip, dev = InferenceParams(2, 64), torch.device("cuda", 0)
    ip.device_multi, ip.sequence_len_offset = value, 8
    ip.device_offset = torch.tensor([8], device=dev)
    ip.device_kv_len = torch.tensor([12], dtype=torch.int32, device=dev)
    with contextlib.nullcontext() if ok else pytest.raises(NotImplementedError):
        assert kv_cache.LayerKV(ip, 1, 2, 64, G.BF16, dev, 4, 2, fused=True).kind == kv_cache.DEVICE_MULTI


# (extra model flags, kv_pages, FP8 KV cache)
MODEL_CASES = {"hd64": ([], None, False), "paged": ([], 4, False), "fp8kv": ([], None, True),
               "hd128": (["--num_attention_heads", "2", "--num_attention_heads_kv", "1"], None, False)}


def _model_step(rank, world, case, gpu):
    """Prompt + 4 rows at batch 2.  CPU: the fp32 model's logits.  GPU: an unfused and
    a fused multi-row step, the (rows, batch) of every call of the fused decode layer."""
    from test_fp8_kv_cache_gpu import _model_and_tokens
    from test_gpu_e2e import LLAMA_GQA
    from epfl_megatron_amd.inference import kv_cache
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import KV_PAGE
    from epfl_megatron_amd.models.transformer import ParallelTransformerLayer as Layer
    flags, pages, fp8 = MODEL_CASES[case]
    m, _ = _model_and_tokens(LLAMA_GQA + ["--hidden_size", "256"] + flags, 2, gpu)
    tokens = torch.randint(0, 512, (2, PROMPT + NEW), generator=torch.Generator().manual_seed(8))
    pos = torch.arange(PROMPT + NEW)[None].expand(2, -1)
    if not gpu:
        with torch.no_grad():
            return m(tokens, pos, None)[:, PROMPT:].float()
    tokens, pos = tokens.cuda(), pos.cuda()
    kv_cache.set_fp8_kv_cache(fp8)
    calls, inner, res = [], Layer._forward_decode_fused, {}
    Layer._forward_decode_fused = lambda self, h, *a: (calls.append(tuple(h.shape[:2])), inner(self, h, *a))[1]
    for value in (True, "fused"):
        ip, first = InferenceParams(2, 64, kv_pages=pages, table_device=DEV), [PROMPT, PROMPT]
        with torch.no_grad():
            if pages:  # one row at a time: the paged prefill's cell
                ip.page_table[:2] = torch.tensor([[3], [1]], dtype=torch.int32)
                first = [3 * KV_PAGE + PROMPT, KV_PAGE + PROMPT]
            for rows in (slice(0, 1), slice(1, 2)) if pages else (slice(0, 2),):
                ip.batch_size_offset = rows.start
                m(tokens[rows, :PROMPT], pos[rows, :PROMPT], None, inference_params=ip)
            ip.batch_size_offset, ip.sequence_len_offset, ip.device_multi = 0, PROMPT, value
            ip.device_offset = torch.tensor(first, device=DEV)
            ip.device_kv_len = torch.tensor([PROMPT + NEW] * 2, dtype=torch.int32, device=DEV)
            res[value] = m(tokens[:, PROMPT:], pos[:, PROMPT:].contiguous(), None,
                           inference_params=ip).float().cpu()
    kv_cache.set_fp8_kv_cache(False)
    return res[True], res["fused"], calls


@functools.lru_cache(maxsize=None)
def _cpu_ref(case):
    return run_dist(_model_step, 1, case, False, env={"HIP_VISIBLE_DEVICES": ""})[0]


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_fused_model_step_against_the_cpu_model(case):
    """Error against the fp32 CPU model <= 2 x the unfused multi-row step's."""
    unfused, fused, calls = run_dist(_model_step, 1, case, True)[0]
    ref = _cpu_ref("hd128" if case == "hd128" else "hd64")
    base, err = float((unfused - ref).abs().max()), float((fused - ref).abs().max())
    print(f"{case}: logits against the fp32 CPU model: fused step {err:.3e}, unfused step {base:.3e}")
    assert calls and all(c == (NEW, 2) for c in calls)  # every layer, only under "fused"
    assert err <= 2 * base, (err, base)


def _decoders(rank, world, mxfp4):
    """Lockstep and fused speculative tokens on test_spec_decode.py's large-gap
    model; MXFP4: on weights pre-rounded to the format (one model for both)."""
    import test_spec_decode as T
    from epfl_megatron_amd.inference import SpeculativeGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    from epfl_megatron_amd.models import transformer
    from epfl_megatron_amd.ops import mxfp4_weights as mx
    m, prompts = T._model(G.BF16)
    prompts, B = prompts.cuda(), prompts.shape[0]
    with torch.no_grad():
        for name, p in m.named_parameters() if mxfp4 else ():
            if p.dim() == 2 and ".layers." in name:
                p.copy_(mx.dequantize(*mx.quantize_blocks(p), p.dtype))
        transformer.set_mxfp4_weights(mxfp4)
        ip = InferenceParams(B, T.CAP)
        spec = SpeculativeGreedyDecoder(m, ip, B, T.NEW, rows=4, ngram=3, fused=True)
        spec.start(prompts, T._prefill(m, ip, prompts))
        while spec.active_rows():
            spec.step()
        ip = InferenceParams(B, T.CAP)
        lock = GraphedGreedyDecoder(m, ip, B, T.NEW)
        lock.start(T._prefill(m, ip, prompts), T.L)
        for _ in range(T.NEW):
            lock.step()
    transformer.set_mxfp4_weights(False)
    return spec.generated()[0].tolist(), lock.history[:, :T.NEW].tolist(), spec.mean_accepted()


@pytest.mark.parametrize("mxfp4", [False, True], ids=["bf16", "mxfp4"])
def test_fused_decoder_commits_the_greedy_tokens(mxfp4):
    toks, greedy, accepted = run_dist(_decoders, 1, mxfp4)[0]
    print(f"mean accepted {accepted:.3f}")
    assert toks == greedy and accepted > 0
