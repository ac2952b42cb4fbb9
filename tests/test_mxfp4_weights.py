"""ops/mxfp4_weights.py on the CPU: the OCP MXFP4 block quantiser (e2m1
elements, one e8m0 scale per 32 k), the packed layout of the weight-streaming
decode kernels' W4 forms, the cache of the packed pairs and the flag (MXFP4
weight-only decode, ``--inference_mxfp4_weights``)."""
import pytest
import torch

from epfl_megatron_amd.ops import decode_pack as dp
from epfl_megatron_amd.ops import mxfp4_weights as mx

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
# value / 2^e -> code: the grid itself, then every midpoint (ties to the even code)
TABLE = [(v, c) for c, v in enumerate(GRID)] + \
    [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6)]


def _block(vals, e, dtype):
    """One row of 32: ``vals`` 2^e, padded with zeros, with a 4 2^e element
    that pins the block exponent to e."""
    row = torch.zeros(32)
    row[:len(vals)] = torch.tensor(vals)
    row[31] = 4.0
    return torch.ldexp(row, torch.tensor(e)).to(dtype)[None]


@DTYPES
@pytest.mark.parametrize("e", [0, -6, 3])
def test_mxfp4_quantiser_table(dtype, e):
    """Every grid value and every tie, each sign, lands on the stated code."""
    vals = [v for v, _ in TABLE]
    for sign in (1.0, -1.0):
        w = _block([sign * v for v in vals], e, dtype)
        assert torch.equal(w.float()[0, :len(vals)], sign * torch.tensor(vals) * 2.0 ** e)  # exact inputs
        codes, exps = mx.quantize_blocks(w)
        assert codes.dtype == torch.uint8 and exps.dtype == torch.uint8
        assert codes.shape == (1, 32) and exps.shape == (1, 1)
        assert int(exps[0, 0]) == e + 127
        want = [c + (8 if sign < 0 and c else 0) for _, c in TABLE]  # a zero of either sign is code 0
        assert codes[0, :len(vals)].tolist() == want
        assert int(codes[0, 31]) == 6
        d = mx.dequantize(codes, exps, dtype)
        assert torch.equal(d.float()[0, :len(vals)],
                           sign * torch.tensor([GRID[c] for _, c in TABLE]) * 2.0 ** e)


@DTYPES
def test_mxfp4_zero_block_saturation_and_negative_zero(dtype):
    z = torch.zeros(1, 32, dtype=dtype)
    z[0, 3] = -0.0
    codes, exps = mx.quantize_blocks(z)
    assert codes.abs().sum() == 0 and int(exps[0, 0]) == 127
    # amax in (6, 8) 2^e: floor(log2 amax) = e + 2 still, the value saturates to 6
    for e in (0, -4):
        w = torch.zeros(1, 32)
        w[0, 0], w[0, 1], w[0, 2] = 7.0, -7.5, 6.5
        w = torch.ldexp(w, torch.tensor(e)).to(dtype)
        codes, exps = mx.quantize_blocks(w)
        assert int(exps[0, 0]) == e + 127
        assert codes[0, :3].tolist() == [7, 15, 7]
        assert mx.dequantize(codes, exps, dtype)[0, :3].float().tolist() == \
            [6.0 * 2.0 ** e, -6.0 * 2.0 ** e, 6.0 * 2.0 ** e]


def test_mxfp4_exponent_clamps():
    """Every dequantised value is a normal number of the model dtype: e in
    [-125, 125] for bf16 and [-13, 13] for fp16."""
    tiny16 = torch.finfo(torch.float16).tiny  # 2^-14
    # fp16, low end: amax 2^-14 -> floor(log2) - 2 = -16, clamped to -13
    w = torch.zeros(2, 32, dtype=torch.float16)
    w[0, 0] = tiny16
    w[0, 1] = tiny16 / 4  # a subnormal: 2^-16 / 2^-13 = 0.125 -> 0
    w[1, 0] = 2.0 ** -24  # the smallest subnormal alone: the block flushes to zero
    codes, exps = mx.quantize_blocks(w)
    assert exps[:, 0].tolist() == [127 - 13, 127 - 13]
    assert codes[0, :2].tolist() == [1, 0] and codes[1].sum() == 0
    d = mx.dequantize(codes, exps, torch.float16)
    assert float(d[0, 0]) == tiny16 and d[1].abs().sum() == 0
    # fp16, high end: 65504 -> e = 13, saturates to 6 2^13 = 49152
    w = torch.zeros(1, 32, dtype=torch.float16)
    w[0, 0] = 65504.0
    codes, exps = mx.quantize_blocks(w)
    assert int(exps[0, 0]) == 127 + 13 and int(codes[0, 0]) == 7
    assert float(mx.dequantize(codes, exps, torch.float16)[0, 0]) == 49152.0
    # a bf16 tensor quantised for an fp16 model clamps where bf16 itself would not
    w = torch.zeros(2, 32, dtype=torch.bfloat16)
    w[0, 0] = 2.0 ** 20
    w[1, 0] = 2.0 ** -20
    codes, exps = mx.quantize_blocks(w, torch.float16)
    assert exps[:, 0].tolist() == [127 + 13, 127 - 13]
    assert int(codes[0, 0]) == 7 and codes[1].sum() == 0
    assert mx.quantize_blocks(w)[1][:, 0].tolist() == [127 + 18, 127 - 22]
    # bf16: the smallest normal (2^-126) -> -128, clamped to -125; the largest -> 125
    w = torch.zeros(2, 32, dtype=torch.bfloat16)
    w[0, 0] = 2.0 ** -126
    w[0, 1] = 2.0 ** -125
    w[1, 0] = torch.finfo(torch.bfloat16).max
    codes, exps = mx.quantize_blocks(w)
    assert exps[:, 0].tolist() == [127 - 125, 127 + 125]
    assert codes[0, :2].tolist() == [1, 2] and int(codes[1, 0]) == 7
    d = mx.dequantize(codes, exps, torch.bfloat16).float()
    assert float(d[0, 0]) == 2.0 ** -126 and float(d[1, 0]) == 6.0 * 2.0 ** 125
    assert int(exps.min()) >= 2  # never the zero encoding the kernel's conversion cannot take


def _weights(dtype, n=48, k=512):
    torch.manual_seed(4)
    w = (0.02 * torch.randn(n, k)).to(dtype)
    w[5] = 0  # an all-zero row
    w[7, 64:96] *= 1e-6  # one tiny block
    w[9, 100] = 3.0  # one outlier
    return w


@DTYPES
def test_mxfp4_dequantize_exact_and_value_idempotent(dtype):
    w = _weights(dtype)
    codes, exps = mx.quantize_blocks(w)
    assert int(codes.max()) <= 15
    # the exact value in fp32, and its rounding to the model dtype loses nothing
    grid = torch.tensor(GRID + [-v for v in GRID])
    exact = grid[codes.long()] * torch.ldexp(torch.ones(1), exps.int() - 127).repeat_interleave(32, 1)
    d = mx.dequantize(codes, exps, dtype)
    assert d.dtype == dtype and torch.equal(d.float(), exact)
    d2 = mx.dequantize(*mx.quantize_blocks(d), dtype)
    assert torch.equal(d2, d)  # values, not exponent bytes
    # the block amax lands in [4, 6] 2^e: the block error is at most amax / 4
    # (the saturation of (6, 8) 2^e), an element's at most half a grid step
    blk = w.float().reshape(48, -1, 32)
    err = (d.float() - w.float()).reshape(48, -1, 32).abs()
    step = torch.ldexp(torch.ones(1), exps.int() - 127)[:, :, None]
    a = blk.abs() / step
    half = torch.where(a <= 2, 0.25, torch.where(a <= 4, 0.5, torch.where(a <= 6, 1.0, 2.0)))
    assert (err <= half * step).all()
    rel = float((d.float() - w.float()).norm() / w.float().norm())
    print("relative RMS weight error", rel)
    gauss = (0.02 * torch.randn(256, 1024, generator=torch.Generator().manual_seed(0))).to(dtype)
    dg = mx.dequantize(*mx.quantize_blocks(gauss), dtype)
    rel = float((dg.float() - gauss.float()).norm() / gauss.float().norm())
    print("relative RMS weight error, N(0, 0.02^2)", rel)
    assert 0.05 < rel < 0.15  # the format's error (about 0.11)


def _rand(n, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8),
            torch.randint(2, 253, (n, k // 32), generator=g, dtype=torch.uint8))


@pytest.mark.parametrize("s", [2, 3, 4, 16, 32, 43])
@pytest.mark.parametrize("glu,tail", [(False, 0), (True, 0), (True, 1)],
                         ids=["plain", "glu", "glu_half_tail"])
def test_mxfp4_pack_round_trip(s, glu, tail):
    if tail and s % 4:
        with pytest.raises(AssertionError):
            mx.pack_mxfp4(*_rand(48, 256 * s), glu, tail)
        return
    codes, exps = _rand(48, 256 * s, seed=s)
    wq, ws = mx.pack_mxfp4(codes, exps, glu, tail)
    assert wq.dtype == torch.uint8 and ws.dtype == torch.uint8
    assert wq.shape == (48, 128 * s) and ws.shape == (48 * 8 * s,)
    assert wq.is_contiguous() and ws.is_contiguous()
    c2, e2 = mx.unpack_mxfp4(wq, ws, glu, tail)
    assert torch.equal(c2, codes) and torch.equal(e2, exps)
    assert not torch.equal(ws.reshape(48, -1), exps)


def test_mxfp4_pack_layout():
    """One lane's piece of one slot and its scale dword, read out of the packed
    bytes where the module docstring puts them: per (block, wave) S x 256
    weight bytes and S x 16 scale bytes; four-step slots of 1 KiB (lane
    16 q + r at byte 16 L, k-step 4 p + h in dword h, nibble pairs low first)
    with the row's scale dword at 64 p + 4 r; leftover steps as 4-B pieces
    with one scale byte; GLU half units at half the size."""
    S = 7  # one slot + 3 leftover steps
    for glu in (False, True):
        codes, exps = _rand(64, 256 * S, seed=1)
        wq, ws = mx.pack_mxfp4(codes, exps, glu)
        wq = wq.reshape(-1, 8, S * 256)  # [block, wave, stream]
        ws = ws.reshape(-1, 8, S * 16)
        for (b, wv, s, qq, r, j) in [(0, 0, 0, 0, 0, 0), (1, 3, 1, 2, 9, 3), (3, 7, 3, 3, 15, 2),
                                     (2, 5, 4, 0, 4, 1), (1, 2, 5, 1, 8, 0), (3, 6, 6, 3, 7, 3)]:
            row = (8 * b + r if r < 8 else 32 + 8 * b + r - 8) if glu else 16 * b + r
            lane = 16 * qq + r
            k = wv * 32 * S + 32 * s + 8 * qq + 2 * j
            if s < 4:  # the slot: byte 16 L + 4 h + j, scale 4 r + h
                byte, sc = wq[b, wv, 16 * lane + 4 * s + j], ws[b, wv, 4 * r + s]
            else:      # leftover step: behind the slot, byte 4 L + j, scale byte r
                byte, sc = wq[b, wv, 1024 + 256 * (s - 4) + 4 * lane + j], ws[b, wv, 64 + 16 * (s - 4) + r]
            assert int(byte) == int(codes[row, k]) | int(codes[row, k + 1]) << 4
            assert int(sc) == int(exps[row, wv * S + s])
    # one chosen element of the plain form, spelled out (S = 8)
    codes, exps = _rand(32, 2048, seed=2)
    wq, ws = mx.pack_mxfp4(codes, exps)
    # W[17, 1300..1301]: block 1, r 1; 1300 = wave 5 * 256 + 20 -> step 0, q 2, j 2; slot 0
    assert int(wq.reshape(-1)[(1 * 8 + 5) * 8 * 256 + 16 * (16 * 2 + 1) + 2]) == \
        int(codes[17, 1300]) | int(codes[17, 1301]) << 4
    # W[17, 1500]: 1500 = wave 5 * 256 + 220 -> step 6 = slot 1, h 2: the scale of block 1500 // 32
    assert int(ws[(1 * 8 + 5) * 8 * 16 + 64 * 1 + 4 * 1 + 2]) == int(exps[17, 1500 // 32])
    # GLU half-unit tail: [unit, half, wave, p, q, pr, h, j], pr = 4 up then 4 gate rows
    S, F = 8, 56
    codes, exps = _rand(2 * F, 256 * S, seed=3)
    wq, ws = mx.pack_mxfp4(codes, exps, True, half_tail=3)
    full = F // 8 - 3
    v = wq.reshape(-1)[full * 8 * 256 * S:].view(3, 2, 8, S // 4, 4, 8, 4, 4)
    sv = ws[full * 16 * 8 * S:].view(3, 2, 8, S // 4, 8, 4)
    for (bt, hf, wv, pp, qq, pr, h, j) in [(0, 0, 0, 0, 0, 0, 0, 0), (2, 1, 7, 1, 3, 7, 3, 3),
                                           (1, 0, 3, 1, 2, 5, 2, 1)]:
        f = 8 * (full + bt) + 4 * hf + (pr & 3)
        row = f if pr < 4 else F + f
        k = wv * 32 * S + 32 * (4 * pp + h) + 8 * qq + 2 * j
        assert int(v[bt, hf, wv, pp, qq, pr, h, j]) == int(codes[row, k]) | int(codes[row, k + 1]) << 4
        assert int(sv[bt, hf, wv, pp, pr, h]) == int(exps[row, wv * S + 4 * pp + h])
    # the full blocks in front of the tail are the plain GLU layout
    head = mx.pack_mxfp4(torch.cat((codes[:8 * full], codes[F:F + 8 * full])),
                         torch.cat((exps[:8 * full], exps[F:F + 8 * full])), True)
    assert torch.equal(wq.reshape(-1)[:full * 8 * 256 * S], head[0].reshape(-1))
    assert torch.equal(ws[:full * 16 * 8 * S], head[1])


def test_mxfp4_packed_cache_rules():
    """packed_mxfp4 follows decode_pack.packed's key (storage, _version, weight
    generation, form), leaves the 16-bit packs alone and returns None for
    shapes that do not pack."""
    flat = (0.02 * torch.randn(64 * 512)).bfloat16()
    w = torch.nn.Parameter(torch.empty(0, dtype=torch.bfloat16), requires_grad=False)
    w.data = flat.view(64, 512)
    p16 = dp.packed(w, glu=True, half_tail=0)
    a = mx.packed_mxfp4(w, glu=True, half_tail=0)
    b = mx.packed_mxfp4(w)
    assert mx.packed_mxfp4(w, glu=True, half_tail=0) is a and mx.packed_mxfp4(w) is b
    assert a[0] is mx.packed_mxfp4(w, glu=True)[0] and a[1] is mx.packed_mxfp4(w, glu=True)[1]
    codes, exps = mx.quantize_blocks(w.detach())
    for got, want in ((a, mx.pack_mxfp4(codes, exps, True)), (b, mx.pack_mxfp4(codes, exps))):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert a[0].dtype == torch.uint8 and a[1].dtype == torch.uint8
    assert a[0].shape == (64, 256) and a[1].shape == (64 * 512 // 32,)
    assert dp.packed(w, glu=True, half_tail=0) is p16  # the 16-bit form was not evicted
    assert isinstance(w._ema_decode_packed_mxfp4, dict)
    with torch.no_grad():
        flat.add_(1.0)  # rewritten through the flat buffer: _version does not move
    dp.bump_weight_generation()
    a2 = mx.packed_mxfp4(w, glu=True, half_tail=0)
    want = mx.pack_mxfp4(*mx.quantize_blocks(w.detach()), True)
    assert a2 is not a and torch.equal(a2[0], want[0]) and torch.equal(a2[1], want[1])
    with torch.no_grad():
        w.mul_(0.5)  # an in-place write moves _version
    a3 = mx.packed_mxfp4(w, glu=True, half_tail=0)
    assert a3 is not a2 and torch.equal(a3[1], mx.pack_mxfp4(*mx.quantize_blocks(w.detach()), True)[1])
    assert mx.packed_mxfp4(w, glu=True, half_tail=0) is a3
    assert not mx.packable(torch.zeros(16, 384, dtype=torch.uint8))
    assert mx.packed_mxfp4(torch.zeros(16, 384).bfloat16()) is None   # K % 256
    assert mx.packed_mxfp4(torch.zeros(24, 512).bfloat16()) is None   # N % 16
    assert mx.packed_mxfp4(torch.zeros(16, 512)) is None              # fp32
    enabled = dp.ENABLED
    try:
        dp.ENABLED = False
        assert mx.packed_mxfp4(w) is None
    finally:
        dp.ENABLED = enabled


def test_mxfp4_flag_parses_and_excludes_fp8_weights(capsys):
    """--inference_mxfp4_weights is parsed next to --inference_fp8_weights, is
    off by default, and the two weight formats exclude each other."""
    from epfl_megatron_amd.config.arguments import FLAG_TABLE, parse_args
    names = [f for f, _ in FLAG_TABLE["inference"]]
    flags = dict(FLAG_TABLE["inference"])
    assert flags["--inference_mxfp4_weights"]["action"] == "store_true"
    assert names.index("--inference_mxfp4_weights") == names.index("--inference_fp8_weights") + 1
    from epfl_megatron_amd.models import transformer
    assert transformer._MXFP4_WEIGHTS is False and transformer._FP8_WEIGHTS is False
    assert parse_args(args_list=[]).inference_mxfp4_weights is False
    assert parse_args(args_list=["--inference_mxfp4_weights"]).inference_mxfp4_weights is True
    assert parse_args(args_list=["--inference_fp8_weights"]).inference_mxfp4_weights is False
    with pytest.raises(SystemExit) as e:
        parse_args(args_list=["--inference_fp8_weights", "--inference_mxfp4_weights"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--inference_fp8_weights" in err and "--inference_mxfp4_weights" in err
    try:
        transformer.set_mxfp4_weights(True)
        assert transformer._MXFP4_WEIGHTS is True
    finally:
        transformer.set_mxfp4_weights(False)
