"""ops/fp8_weights.py on the CPU: the per-row e4m3 quantiser, the packed FP8
layout of the weight-streaming decode kernels and the cache of the packed
pairs (FP8 weight-only decode, ``--inference_fp8_weights``)."""
import pytest
import torch

from epfl_megatron_amd.ops import decode_pack as dp
from epfl_megatron_amd.ops import fp8_weights as f8


def _rand_q(n, k, seed=0):
    """Random e4m3 bytes without the two NaN encodings (0x7f / 0xff)."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (n, k), generator=g, dtype=torch.uint8)
    b[(b & 0x7f) == 0x7f] = 0x3c
    return b.view(torch.float8_e4m3fn)


def _bytes(t):
    return t.view(torch.uint8)


@pytest.mark.parametrize("n,k,glu,tail", [(32, 512, False, 0), (32, 512, True, 0),
                                          (48, 4096, True, 1), (32, 768, False, 0),
                                          (32, 768, True, 0)],
                         ids=["plain", "glu", "glu_half_tail", "odd_steps", "glu_odd_steps"])
def test_fp8_pack_round_trip(n, k, glu, tail):
    q = _rand_q(n, k)
    p = f8.pack_fp8(q, glu, tail)
    assert p.shape == q.shape and p.dtype == torch.float8_e4m3fn
    assert torch.equal(_bytes(f8.unpack_fp8(p, glu, tail)), _bytes(q))
    assert not torch.equal(_bytes(p), _bytes(q))


def test_fp8_pack_layout():
    """Per (block, wave) S x 512 bytes: two-step units of 1 KiB with lane
    q * 16 + r at byte 16 L (k-step 2 p in the low 8 bytes, 2 p + 1 in the
    high ones), an odd last k-step as 8-B pieces; the GLU half-unit tail as
    512-B two-step units ``[q, pr, h, e]``.  The k index of a lane's bytes is
    the 16-bit pack's (``test_decode_pack_layout``)."""
    S = 3
    for glu in (False, True):
        q = _rand_q(64, 256 * S, seed=1)
        qb = _bytes(q)
        p = _bytes(f8.pack_fp8(q, glu)).reshape(-1, 8, S * 512)  # [block, wave, stream]
        for (b, wv, s, qq, r, e) in [(0, 0, 0, 0, 0, 0), (1, 3, 1, 2, 9, 5), (3, 7, 2, 3, 15, 7),
                                     (2, 5, 2, 0, 4, 1)]:
            row = (8 * b + r if r < 8 else 32 + 8 * b + r - 8) if glu else 16 * b + r
            lane = 16 * qq + r
            if s == S - 1:  # the odd last step: 8-B pieces behind the S // 2 full units
                off = (S // 2) * 1024 + 8 * lane + e
            else:
                off = (s // 2) * 1024 + 16 * lane + 8 * (s % 2) + e
            assert p[b, wv, off] == qb[row, wv * 32 * S + 32 * s + 8 * qq + e]
    # one chosen element of the plain form, spelled out
    q = _rand_q(32, 768, seed=2)
    p = _bytes(f8.pack_fp8(q)).reshape(-1)
    # W[17, 300]: block 1, r 1; 300 = wave 3 * 96 + 12 -> wave 3, step 0, q 1, e 4
    assert p[(1 * 8 + 3) * 3 * 512 + 16 * (16 * 1 + 1) + 4] == _bytes(q)[17, 300]
    # GLU half-unit tail: [unit, wave, p, q, pr, h, e], pr = 4 up then 4 gate rows
    S, F = 4, 56
    q = _rand_q(2 * F, 256 * S, seed=3)
    qb = _bytes(q)
    pk = f8.pack_fp8(q, True, half_tail=3)
    assert torch.equal(_bytes(f8.unpack_fp8(pk, True, half_tail=3)), qb)
    full = F // 8 - 3
    v = _bytes(pk).reshape(-1)[full * 16 * 256 * S:].view(3, 2, 8, S // 2, 4, 8, 2, 8)
    for (bt, hf, wv, pp, qq, pr, h, e) in [(0, 0, 0, 0, 0, 0, 0, 0), (2, 1, 7, 1, 3, 7, 1, 5),
                                           (1, 0, 3, 1, 2, 5, 0, 1)]:
        f = 8 * (full + bt) + 4 * hf + (pr & 3)
        assert v[bt, hf, wv, pp, qq, pr, h, e] == \
            qb[f if pr < 4 else F + f, wv * 32 * S + 32 * (2 * pp + h) + 8 * qq + e]
    # the full blocks in front of the tail are the plain GLU layout
    assert torch.equal(_bytes(pk).reshape(-1)[:full * 16 * 256 * S],
                       _bytes(f8.pack_fp8(torch.cat((q[:8 * full], q[F:F + 8 * full])), True)).reshape(-1))
    assert not f8.packable(torch.zeros(16, 384))
    assert f8.packed_fp8(torch.zeros(16, 384).bfloat16()) is None


def _weights(dtype):
    torch.manual_seed(4)
    w = (0.02 * torch.randn(48, 512)).to(dtype)
    w[5] = 0  # an all-zero row
    w[9, 100] = 3.0  # one outlier
    return w


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fp8_quantize_rows_error_bound(dtype):
    """|q scale - w| <= max(|w| 2^-4, scale 2^-10): half an ulp of three
    mantissa bits, or half the 2^-9 subnormal spacing."""
    w = _weights(dtype)
    q, scale = f8.quantize_rows(w)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert q.shape == w.shape and scale.shape == (w.shape[0],)
    wf = w.float()
    assert torch.equal(scale, torch.where(wf.abs().amax(1) == 0, torch.ones(48),
                                          wf.abs().amax(1) / 448))
    assert scale[5] == 1 and not q.float().isnan().any()
    err = (q.float() * scale[:, None] - wf).abs()
    bound = torch.maximum(wf.abs() * 2.0 ** -4, scale[:, None] * 2.0 ** -10) * (1 + 1e-6)
    print("max err / bound", float((err / bound.clamp_min(1e-30)).max()))
    assert (err <= bound).all()
    assert q.float().abs().amax(1)[9] == 448  # the row maximum lands on the format's


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fp8_pow2_scales_idempotent(dtype):
    """Power-of-two scales: q scale is exact in the weight dtype, and
    quantising that again dequantises to the same values bitwise (the scale
    may halve while q doubles)."""
    w = _weights(dtype)
    q, scale = f8.quantize_rows(w, pow2=True)
    amax = w.float().abs().amax(1)
    m, _ = torch.frexp(scale)
    assert (m == 0.5).all()  # powers of two
    nz = amax > 0
    assert (scale[nz] >= amax[nz] / 448).all() and (scale[nz] < 2 * amax[nz] / 448).all()
    assert scale[5] == 1
    deq = q.float() * scale[:, None]
    w1 = deq.to(dtype)
    assert torch.equal(w1.float(), deq)  # exact
    q2, scale2 = f8.quantize_rows(w1, pow2=True)
    assert torch.equal(q2.float() * scale2[:, None], deq)
    assert (scale2 <= scale).all()


def test_fp8_packed_cache_rules():
    """packed_fp8 follows decode_pack.packed's key (storage, _version, weight
    generation, form) and leaves the 16-bit packs alone."""
    flat = (0.02 * torch.randn(64 * 512)).bfloat16()
    w = torch.nn.Parameter(torch.empty(0, dtype=torch.bfloat16), requires_grad=False)
    w.data = flat.view(64, 512)
    p16 = dp.packed(w, glu=True, half_tail=0)
    a = f8.packed_fp8(w, glu=True, half_tail=0)
    b = f8.packed_fp8(w)
    assert f8.packed_fp8(w, glu=True, half_tail=0) is a and f8.packed_fp8(w) is b
    assert a[0] is f8.packed_fp8(w, glu=True)[0] and a[1] is f8.packed_fp8(w, glu=True)[1]
    q, scale = f8.quantize_rows(w.detach())
    assert torch.equal(_bytes(a[0]), _bytes(f8.pack_fp8(q, True))) and torch.equal(a[1], scale)
    assert torch.equal(_bytes(b[0]), _bytes(f8.pack_fp8(q)))
    assert a[0].dtype == torch.float8_e4m3fn and a[1].dtype == torch.float32
    assert dp.packed(w, glu=True, half_tail=0) is p16  # the 16-bit form was not evicted
    with torch.no_grad():
        flat.add_(1.0)  # rewritten through the flat buffer: _version does not move
    dp.bump_weight_generation()
    a2 = f8.packed_fp8(w, glu=True, half_tail=0)
    q2, scale2 = f8.quantize_rows(w.detach())
    assert a2 is not a and torch.equal(_bytes(a2[0]), _bytes(f8.pack_fp8(q2, True)))
    assert torch.equal(a2[1], scale2)
    with torch.no_grad():
        w.mul_(0.5)  # an in-place write moves _version
    a3 = f8.packed_fp8(w, glu=True, half_tail=0)
    assert a3 is not a2 and torch.equal(a3[1], f8.quantize_rows(w.detach())[1])
    assert f8.packed_fp8(w, glu=True, half_tail=0) is a3


def test_fp8_flag_sets_the_module_switch():
    """--inference_fp8_weights is parsed next to --inference_hip_graph and is off by default."""
    from epfl_megatron_amd.config.arguments import FLAG_TABLE
    flags = dict(FLAG_TABLE["inference"])
    assert flags["--inference_fp8_weights"]["action"] == "store_true"
    from epfl_megatron_amd.models import transformer
    assert transformer._FP8_WEIGHTS is False
