"""The 33-64-row weight-streaming GEMM (csrc/wide_gemm.hip): exact integer
products, the e4m3 / MXFP4 forms bitwise against the 16-bit form, every
epilogue against fp64, and the decode layer at batch 40."""
import pytest
import torch

from dist_utils import run_dist
from test_kernels_gpu import _close, _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (33, 48, 49, 64)
# (W rows, K, fb): the host's split everywhere; KS = 1 / 4 / 8 forced where the
# sub-streams have seams (S = 3) or are long with a ragged last workgroup (5 blocks)
CASES = [(256, 512, 0), (512, 4096, 0)] + [(n, k, fb) for n, k in ((256, 768), (80, 11008))
                                           for fb in (0, 8, 2, 1)]
QKV = {80: (1, 3, 16), 256: (2, 2, 32), 512: (2, 2, 64)}  # W rows -> (ng, r, hd)
ACTS = (torch.nn.functional.silu, lambda g: torch.nn.functional.gelu(g), torch.relu, lambda g: g)


def _ops(M, N, K, dt, ints=False):
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + K)
    if ints:
        x = torch.randint(-4, 5, (M, K), device=DEV, generator=g).to(dt)
        w = (torch.randint(-4, 5, (N, K), device=DEV, generator=g).float() / 256).to(dt)
        res = torch.randint(-8, 9, (M, N), device=DEV, generator=g).to(dt)
    else:
        x = torch.randn(M, K, device=DEV, generator=g).to(dt)
        w = (torch.randn(N, K, device=DEV, generator=g) * 0.03).to(dt)
        res = torch.randn(M, N, device=DEV, generator=g).to(dt)
    return x, w, res


def _qkv(C, x, wp, N, dt, fb, ws=None, fp8=False):
    """q and the two caches (fill byte 0x55) with per-row slots 3 + (5 m) % 7."""
    ng, r, hd = QKV[N]
    from epfl_megatron_amd.ops.rope import rope_table
    M = x.shape[0]
    cos, sin = rope_table(hd, 128, DEV)
    pos = (torch.arange(M, device=DEV) * 3 % 128).view(M, 1)
    slot = 3 + torch.arange(M, device=DEV) * 5 % 7
    kc, vc = (torch.full((12, M, ng, hd), 0x55, dtype=torch.uint8, device=DEV) if fp8 else
              torch.full((12, M, ng, hd * 2), 0x55, dtype=torch.uint8, device=DEV).view(dt)
              for _ in range(2))
    kvs = (torch.rand(2, ng, device=DEV) + 0.5) if fp8 else None
    q = C.wide_qkv_rope_cache(x, wp, ng, r, hd, cos, sin, pos, kc, vc, slot, 0, ws, kvs, fb)
    return q, kc, vc, (cos, sin, pos, slot, kvs)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,fb", CASES)
def test_exact_integers(M, N, K, fb):
    """|sum| < 2^24 quanta: the fp32 sum is exact in any order, so every output
    equals the fp64 result rounded as the epilogue rounds; nothing else is written."""
    from epfl_megatron_amd.ops import decode_pack
    C, dt = _ext(), torch.bfloat16
    assert C.wide_gemm_supported(M, N, K) and not C.skinny_gemm_supported(M, N, K)
    x, w, res = _ops(M, N, K, dt, ints=True)
    acc = (x.double() @ w.double().t()).to(dt)
    out = torch.full((M + 3, N + 8), float("nan"), device=DEV, dtype=dt)
    y = C.wide_gemm(x, decode_pack.pack(w), None, None, fb, out)
    assert torch.equal(y, acc) and out[M:].isnan().all() and out[:, N:].isnan().all()
    y = C.wide_gemm(x, decode_pack.pack(w), res, None, fb)
    assert torch.equal(y, (acc.double() + res.double()).to(dt))
    F = N // 2
    for kind in (2, 3):
        out.fill_(float("nan"))
        y = C.wide_glu(x, decode_pack.pack(w, glu=True), kind, None, fb, out)
        assert torch.equal(y, (acc[:, :F].double() * ACTS[kind](acc[:, F:].double())).to(dt))
        assert out[M:].isnan().all() and out[:, F:].isnan().all()


@pytest.mark.parametrize("dt,M,N,K,fb", [(torch.bfloat16, m, *c) for m in MS for c in CASES] +
                         [(torch.float16, 49, 256, 768, 2), (torch.float16, 33, 80, 11008, 0)])
def test_formats_bitwise(dt, M, N, K, fb):
    """e4m3 (power-of-two row scales) and MXFP4 weights against the 16-bit form
    on the dequantised weights: the same k order, so the same bits."""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8, mxfp4_weights as mx
    C = _ext()
    x, w, res = _ops(M, N, K, dt)
    q8, s8 = f8.quantize_rows(w, pow2=True)
    codes, exps = mx.quantize_blocks(w)
    forms = [((q8.float() * s8[:, None]).to(dt), lambda g: (f8.pack_fp8(q8, g), s8)),
             (mx.dequantize(codes, exps, dt), lambda g: mx.pack_mxfp4(codes, exps, g))]
    for wd, packq in forms:
        wp, ws = packq(False)
        for r_ in (None, res):
            assert torch.equal(C.wide_gemm(x, wp, r_, ws, fb),
                               C.wide_gemm(x, decode_pack.pack(wd), r_, None, fb))
        a = _qkv(C, x, wp, N, dt, fb, ws)[:3]
        b = _qkv(C, x, decode_pack.pack(wd), N, dt, fb)[:3]
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        wp, ws = packq(True)
        for kind in range(4):
            assert torch.equal(C.wide_glu(x, wp, kind, ws, fb),
                               C.wide_glu(x, decode_pack.pack(wd, glu=True), kind, None, fb)), kind


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,fb", CASES)
def test_against_fp64(M, N, K, fb):
    from epfl_megatron_amd.ops import decode_pack
    C, dt = _ext(), torch.bfloat16
    x, w, res = _ops(M, N, K, dt)
    acc = x.double() @ w.double().t()
    wp = decode_pack.pack(w)
    _close(C.wide_gemm(x, wp, None, None, fb), acc, 2e-2, 2e-2, "plain")
    _close(C.wide_gemm(x, wp, res, None, fb), acc + res.double(), 2e-2, 2e-2, "residual")
    F = N // 2
    for kind in range(4):
        y = C.wide_glu(x, decode_pack.pack(w, glu=True), kind, None, fb)
        _close(y, acc[:, :F] * ACTS[kind](acc[:, F:]), 2e-2, 2e-2, f"glu {kind}")
    ng, r, hd = QKV[N]
    for fp8 in (False, True):
        q, kc, vc, (cos, sin, pos, slot, kvs) = _qkv(C, x, wp, N, dt, fb, fp8=fp8)
        t = acc.view(M, ng, r + 2, hd // 2, 2)
        c, s = (v[pos[:, 0]].double().view(M, 1, 1, hd // 2) for v in (cos, sin))
        rot = torch.stack((t[..., 0] * c - t[..., 1] * s, t[..., 0] * s + t[..., 1] * c), -1)
        rot = rot.view(M, ng, r + 2, hd)
        _close(q, rot[:, :, :r].reshape(M, -1), 2e-2, 2e-2, "q")
        rows = torch.arange(M, device=DEV)
        for cache, want, sc in ((kc, rot[:, :, r], 0), (vc, acc.view(M, ng, r + 2, hd)[:, :, r + 1], 1)):
            got = cache.view(torch.float8_e4m3fn).double() * kvs[sc].view(1, 1, ng, 1) if fp8 else cache
            # e4m3 keeps 3 mantissa bits: half an ulp is 2^-4 relative
            _close(got[slot, rows], want, 2e-2, 2e-2 + (2 ** -4 if fp8 else 0), "cache")
            mask = torch.ones(cache.shape[:2], dtype=torch.bool, device=DEV)
            mask[slot, rows] = False
            assert (cache.view(torch.uint8)[mask] == 0x55).all()


def _layer_b40(rank, world):
    """Fused (wide kernel) vs unfused decode at b = 40 on the small GQA model;
    MXFP4 weights against the fused path on the dequantised weights; one
    RaggedGreedyDecoder replay against the eager loop."""
    from test_continuous_gpu import CAP, _model, _prefill
    from epfl_megatron_amd.inference import RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.models import transformer
    from epfl_megatron_amd.ops import mxfp4_weights as mx
    m = _model()
    transformer._WIDE_GEMM = "1"  # also with 16-bit weights
    calls = [0]
    orig = transformer.ParallelTransformerLayer._forward_decode_fused

    def counted(self, *a, **k):
        calls[0] += 1
        return orig(self, *a, **k)
    transformer.ParallelTransformerLayer._forward_decode_fused = counted
    torch.manual_seed(6)
    b, plen, n = 40, 21, 4
    prompt = torch.randint(0, 512, (b, plen), device=DEV)
    pos = torch.arange(plen + n, device=DEV)[None].expand(b, -1)

    def decode(ip, nxt, feed=None):
        """n eager steps from a prefilled cache: (logits, greedy tokens); the
        input of step i + 1 is ``feed[:, i]`` when given, else the greedy token,
        so that two paths are compared on the same inputs at every step."""
        logits, toks = [], []
        for i, t in enumerate(range(plen, plen + n)):
            lg = m(nxt, pos[:, t:t + 1], None, inference_params=ip).float()
            toks.append(lg[:, -1].argmax(-1, keepdim=True))
            nxt = toks[-1] if feed is None else feed[:, i:i + 1]
            logits.append(lg)
            ip.sequence_len_offset += 1
        return torch.cat(logits, 1), torch.cat(toks, 1)

    def run(fused, mxfp4=False, feed=None):
        transformer._DECODE_FUSED, transformer._MXFP4_WEIGHTS = fused, mxfp4
        with torch.no_grad():
            ip = InferenceParams(b, plen + n)
            nxt = m(prompt, pos[:, :plen], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
            ip.sequence_len_offset += plen
            logits, toks = decode(ip, nxt, feed)
        transformer._DECODE_FUSED, transformer._MXFP4_WEIGHTS = True, False
        return logits, toks, [t[:plen + n].float() for t in ip.key_value_memory_dict[1]]
    lf, tf, cf = run(True)
    ncalls = calls[0]
    lu, tu, cu = run(False, feed=tf)
    # a fused token is a greedy token of the unfused logits: equal to their
    # argmax, or, where their two largest entries are exactly equal, one of the two
    greedy = lu.gather(-1, tf[..., None])[..., 0] == lu.amax(-1)
    out = {"calls": ncalls, "err": float((lf - lu).abs().max()), "scale": float(lu.abs().max()),
           "same": int(greedy.sum()), "argmax_same": int((tf == tu).sum()),
           "cache": max(float((a - c).abs().max()) for a, c in zip(cf, cu))}
    # graphed ragged decode against the eager loop, both over caches prefilled row by row
    ips = [InferenceParams(b, CAP) for _ in range(2)]
    first = [[int(_prefill(m, ip, row, prompt[row]).argmax()) for row in range(b)] for ip in ips][0]
    dec = RaggedGreedyDecoder(m, ips[0], b, n)
    for row in range(b):
        dec.prime(row, first[row], plen, n)
    for _ in range(n):
        dec.step()
    ips[1].sequence_len_offset = plen
    with torch.no_grad():
        le, te = decode(ips[1], torch.tensor(first, device=DEV).view(b, 1))
    out["ragged"] = int((dec.history[:, :n] == te).sum())
    # MXFP4 weights vs the fused path on their dequantised values (set first:
    # the prefill reads the 16-bit weights either way)
    with torch.no_grad():
        for layer in (l for l in m.modules() if isinstance(l, transformer.ParallelTransformerLayer)):
            for w in (layer.self_attention.query_key_value.weight, layer.self_attention.dense.weight,
                      layer.mlp.dense_h_to_4h.weight, layer.mlp.dense_4h_to_h.weight):
                w.copy_(mx.dequantize(*mx.quantize_blocks(w), w.dtype))
    lq, tq, _ = run(True, mxfp4=True)
    ld, td, _ = run(True)
    out["mx"] = (torch.equal(tq, td), torch.equal(lq, ld))
    transformer.ParallelTransformerLayer._forward_decode_fused = orig
    return out


def test_layer_batch40():
    """Measured on the MI355X: logit difference 0.03125 at scale 4.875, cache
    difference 7.6e-6, 160 of 160 fused tokens greedy under the unfused logits
    (159 equal to torch.argmax's pick; in the other one the unfused logits' two
    largest entries are exactly equal), 160 of 160 ragged tokens."""
    o = run_dist(_layer_b40, 1)[0]
    print(sorted(o.items()))
    assert o["calls"] == 2 * 4, o  # every decode step of both layers took the fused path
    assert o["err"] < 2e-2 * max(1.0, o["scale"]), o
    assert o["same"] == 40 * 4, o  # greedy tokens equal (up to exact ties of the reference)
    assert o["cache"] < 5e-2, o
    assert o["ragged"] == 40 * 4 and o["mx"] == (True, True), o
