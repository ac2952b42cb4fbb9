"""MXFP4 weight-only decode: 4-bit block-scaled weights for the skinny GEMMs.

A decode step is the weight stream from HBM (``ops/decode_pack.py``); with
``--inference_mxfp4_weights`` the four per-layer products stream 4.25 bits per
weight instead of 16 (FP8: 8).  The format is OCP MXFP4: ``e2m1`` elements
(grid 0, 0.5, 1, 1.5, 2, 3, 4, 6 and a sign bit) with one ``e8m0``
power-of-two scale per block of 32 consecutive k of one W row: exactly the
skinny kernel's k-step, so every (W row, k-step) has one scale.  gfx950
converts two nibbles to two scaled bf16 / fp16 values in one instruction
(``v_cvt_scalef32_pk_{bf16,f16}_fp4``); the kernel (``csrc/skinny_gemm.hip``,
W4 forms) expands each piece in front of the same MFMAs, and since a power of
two times an e2m1 value is exact in bf16 / fp16 nothing changes after the
reduction: the W4 forms compute what the 16-bit packed forms compute on
:func:`dequantize`'s weights, bit for bit.  Activations, the KV cache, the LM
head, the embeddings and the prefill are untouched, and the 16-bit parameters
stay: this buys bandwidth, not memory.  All storage is ``torch.uint8``.

Quantiser (:func:`quantize_blocks`), per block of 32: ``amax = max |w|``,
``e = floor(log2 amax) - 2`` (2 = e2m1's emax, the OCP MX rule; ``amax == 0``:
``e = 0``), clamped so that every dequantised value is a normal number of the
model dtype ([-125, 125] for bf16, [-13, 13] for fp16), stored as ``e + 127``.
``|w| / 2^e`` is rounded to the nearest grid value, ties to the even code,
saturating at 6; bit 3 of the code is the sign and every zero is code 0.  On
N(0, 0.02^2) weights the relative RMS weight error is about 0.11.

Packed layout (K % 256 == 0, N % 16 == 0, S = K / 256 k-steps of 32 per wave,
8 waves; the block / wave / k-step / lane structure and ``row(b, r)`` of
``decode_pack``: plain / QKV ``16 b + r``; GLU 8 up rows then the 8 matching
gate rows).  A byte holds element 2 i in its low nibble and element 2 i + 1
in its high nibble.  The ring's loads stay 16 B per lane: one lane's piece
holds its 8 nibbles (4 B) of FOUR consecutive k-steps.  Per (block b, wave)
the weight stream ``wq`` is S x 256 bytes: ``S // 4`` four-step slots of 1 KiB,
``slot[p][q, r, h, j] = C[row(b, r), wave * 32 S + 32 (4 p + h) + 8 q + 2 j]
| C[.., .. + 2 j + 1] << 4`` (lane L = 16 q + r at byte 16 L, k-step 4 p + h in
its dword h), then the ``S % 4`` leftover k-steps (Llama-2-7B fc2: K = 11008,
S = 43 = 10 slots + 3) as single-step 256-B units ``[q, r, j]`` (lane L at
byte 4 L).  So k-step s of a (block, wave) starts at byte 256 s.  The scale
stream ``ws`` has the same order at 16 bytes per k-step: per (block, wave)
``S // 4`` units of 64 B ``[r, h]`` (a lane fetches the 4 scale bytes of its
row for one slot as the aligned dword at ``64 p + 4 r``, byte h = k-step
4 p + h), then per leftover k-step 16 bytes ``[r]``.  Nothing is padded:
``wq`` is ``[N, K / 2]`` and ``ws`` ``[N K / 32]``.  The last ``half_tail``
GLU blocks follow in both streams as half units (the persistent kernel's last
round, K = 4096 / 8192, S a multiple of 4): per (half unit, wave) ``S // 4``
slots of 512 B ``[q, pr, h, j]`` with ``pr`` = the 4 up then the 4 gate rows
(the piece of MFMA rows r and r + 4 at byte ``16 (8 q + pr)``) and 32 scale
bytes ``[pr, h]`` per slot.  The k index a lane feeds to the MFMA and the
ascending k-step order are those of the 16-bit pack.

The cached ``(wq, ws)`` pairs live next to the parameter
(``_ema_decode_packed_mxfp4``) under ``decode_pack.packed``'s key and
invalidation rules (storage pointer, ``_version``, weight generation, form);
they do not touch the 16-bit or FP8 packs.
"""
import torch

from . import decode_pack

BLOCK = 32  # values per e8m0 scale
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# block exponents that keep 0.5 * 2^e .. 6 * 2^e normal in the model dtype
EXP_RANGE = {torch.bfloat16: (-125, 125), torch.float16: (-13, 13)}


def quantize_blocks(w, dtype=None):
    """MXFP4 quantisation of ``w`` [N, K] (bf16 / fp16, K % 32 == 0, CPU or
    GPU) for a model of ``dtype`` (default: ``w``'s): ``(codes, exps)`` with
    ``codes`` uint8 [N, K] in 0..15 and ``exps`` uint8 [N, K / 32] (e + 127)."""
    dtype = w.dtype if dtype is None else dtype
    assert w.dim() == 2 and w.dtype in EXP_RANGE and dtype in EXP_RANGE, (w.shape, w.dtype, dtype)
    n, k = w.shape
    assert k % BLOCK == 0, f"mxfp4: K = {k} is not a multiple of {BLOCK}"
    wf = w.float().reshape(n, k // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=2)
    # amax = m 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    _, ex = torch.frexp(amax)
    lo, hi = EXP_RANGE[dtype]
    e = torch.where(amax == 0, torch.zeros_like(ex), ex - 3).clamp(lo, hi)
    a = torch.ldexp(wf.abs(), -e[:, :, None])
    # nearest grid value, the midpoints going to the even code
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code + (((wf < 0) & (code > 0)).to(torch.uint8) << 3)
    return code.reshape(n, k), (e + 127).to(torch.uint8)


def dequantize(codes, exps, dtype):
    """The exact ``[N, K]`` tensor of ``dtype`` that ``(codes, exps)`` stand for."""
    n, k = codes.shape
    grid = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float32, device=codes.device)
    v = grid[codes.long()].reshape(n, k // BLOCK, BLOCK)
    return torch.ldexp(v, exps.to(torch.int32)[:, :, None] - 127).reshape(n, k).to(dtype)


def packable(codes):
    """codes [N, K] the packed MXFP4 skinny forms can read."""
    return codes.dim() == 2 and codes.shape[1] % 256 == 0 and codes.shape[0] % 16 == 0


def _blocks(b, n, k, glu):
    """[N, k] bytes -> [N / 16, 16 MFMA rows, k] (decode_pack's ``row(b, r)``)."""
    if glu:
        f = n // 2
        return torch.stack((b[:f].reshape(f // 8, 8, k), b[f:].reshape(f // 8, 8, k)), 1) \
            .reshape(f // 8, 16, k)
    return b.reshape(n // 16, 16, k)


def _unblocks(blocks, n, k, glu):
    if glu:
        f = n // 2
        return torch.cat((blocks[:, :8].reshape(f, k), blocks[:, 8:].reshape(f, k)), 0).contiguous()
    return blocks.reshape(n, k).contiguous()


def pack_mxfp4(codes, exps, glu=False, half_tail=0):
    """``(wq, ws)``: the packed nibbles ([N, K / 2] uint8) and the e8m0 scales
    in stream order ([N K / 32] uint8) of ``codes`` [N, K], ``exps`` [N, K / 32]."""
    assert codes.dtype == torch.uint8 and exps.dtype == torch.uint8 and packable(codes), \
        f"mxfp4 pack: unsupported weight {tuple(codes.shape)} {codes.dtype}"
    n, k = codes.shape
    assert tuple(exps.shape) == (n, k // BLOCK), (codes.shape, exps.shape)
    assert glu or not half_tail
    s = k // 256
    sp, left = s // 4, s % 4
    assert not half_tail or left == 0, "half units come in four-step pieces"
    by = codes[:, 0::2] | (codes[:, 1::2] << 4)  # [N, K / 2]
    blocks = _blocks(by, n, k // 2, glu)
    eb = _blocks(exps, n, k // BLOCK, glu)
    full = blocks.shape[0] - half_tail
    x = blocks[:full].reshape(full, 16, 8, s, 4, 4)  # [b, r, wave, s, q, j]
    # slots [b, r, wave, p, h, q, j] -> [b, wave, p, q, r, h, j]: lane q * 16 + r, 16 B
    parts = [x[:, :, :, :4 * sp].reshape(full, 16, 8, sp, 4, 4, 4)
             .permute(0, 2, 3, 5, 1, 4, 6).reshape(full, 8, sp * 1024)]
    for i in range(4 * sp, s):  # leftover k-steps: [b, r, wave, q, j] -> [b, wave, q, r, j]
        parts.append(x[:, :, :, i].permute(0, 2, 3, 1, 4).reshape(full, 8, 256))
    wq = [torch.cat(parts, 2).reshape(-1)]
    y = eb[:full].reshape(full, 16, 8, s)  # [b, r, wave, s]
    # [b, r, wave, p, h] -> [b, wave, p, r, h]
    parts = [y[:, :, :, :4 * sp].reshape(full, 16, 8, sp, 4).permute(0, 2, 3, 1, 4)
             .reshape(full, 8, sp * 64)]
    for i in range(4 * sp, s):  # [b, r, wave] -> [b, wave, r]
        parts.append(y[:, :, :, i].permute(0, 2, 1))
    ws = [torch.cat(parts, 2).reshape(-1)]
    if half_tail:
        t = blocks[full:].reshape(half_tail, 2, 2, 4, k // 2)  # [b, up|gate, half, row, bytes]
        t = t.permute(0, 2, 1, 3, 4).reshape(half_tail, 2, 8, 8, sp, 4, 4, 4)  # [b, half, pr, wave, p, h, q, j]
        wq.append(t.permute(0, 1, 3, 4, 6, 2, 5, 7).reshape(-1))  # [b, half, wave, p, q, pr, h, j]
        t = eb[full:].reshape(half_tail, 2, 2, 4, 8 * s)
        t = t.permute(0, 2, 1, 3, 4).reshape(half_tail, 2, 8, 8, sp, 4)  # [b, half, pr, wave, p, h]
        ws.append(t.permute(0, 1, 3, 4, 2, 5).reshape(-1))  # [b, half, wave, p, pr, h]
    return torch.cat(wq).reshape(n, k // 2).contiguous(), torch.cat(ws).contiguous()


def unpack_mxfp4(wq, ws, glu=False, half_tail=0):
    """Inverse of ``pack_mxfp4`` (tests): ``(codes, exps)``."""
    n, k = wq.shape[0], 2 * wq.shape[1]
    s = k // 256
    sp = s // 4
    nb = n // 16
    full = nb - half_tail
    dev = wq.device
    flat = wq.reshape(-1)
    per = flat[:full * 8 * k].reshape(full, 8, s * 256)
    x = torch.empty(full, 16, 8, s, 4, 4, dtype=torch.uint8, device=dev)
    # [b, wave, p, q, r, h, j] -> [b, r, wave, p, h, q, j]
    x[:, :, :, :4 * sp] = per[:, :, :sp * 1024].reshape(full, 8, sp, 4, 16, 4, 4) \
        .permute(0, 4, 1, 2, 5, 3, 6).reshape(full, 16, 8, 4 * sp, 4, 4)
    for i in range(4 * sp, s):
        x[:, :, :, i] = per[:, :, 256 * i:256 * (i + 1)].reshape(full, 8, 4, 16, 4).permute(0, 3, 1, 2, 4)
    blocks = [x.reshape(full, 16, k // 2)]
    sflat = ws.reshape(-1)
    sper = sflat[:full * 16 * k // BLOCK].reshape(full, 8, s * 16)
    y = torch.empty(full, 16, 8, s, dtype=torch.uint8, device=dev)
    # [b, wave, p, r, h] -> [b, r, wave, p, h]
    y[:, :, :, :4 * sp] = sper[:, :, :sp * 64].reshape(full, 8, sp, 16, 4) \
        .permute(0, 3, 1, 2, 4).reshape(full, 16, 8, 4 * sp)
    for i in range(4 * sp, s):
        y[:, :, :, i] = sper[:, :, 16 * i:16 * (i + 1)].permute(0, 2, 1)
    eb = [y.reshape(full, 16, k // BLOCK)]
    if half_tail:
        t = flat[full * 8 * k:].reshape(half_tail, 2, 8, sp, 4, 8, 4, 4)  # [b, half, wave, p, q, pr, h, j]
        t = t.permute(0, 1, 5, 2, 3, 6, 4, 7)  # [b, half, pr, wave, p, h, q, j]
        t = t.reshape(half_tail, 2, 2, 4, k // 2).permute(0, 2, 1, 3, 4)  # [b, up|gate, half, row, bytes]
        blocks.append(t.reshape(half_tail, 16, k // 2))
        t = sflat[full * 16 * k // BLOCK:].reshape(half_tail, 2, 8, sp, 8, 4)  # [b, half, wave, p, pr, h]
        t = t.permute(0, 1, 4, 2, 3, 5)  # [b, half, pr, wave, p, h]
        t = t.reshape(half_tail, 2, 2, 4, k // BLOCK).permute(0, 2, 1, 3, 4)
        eb.append(t.reshape(half_tail, 16, k // BLOCK))
    by = _unblocks(torch.cat(blocks), n, k // 2, glu)
    codes = torch.stack((by & 15, by >> 4), 2).reshape(n, k)
    return codes, _unblocks(torch.cat(eb), n, k // BLOCK, glu)


def packed_mxfp4(w, glu=False, half_tail=0):
    """Cached ``(packed nibbles, e8m0 scale stream)`` of parameter ``w``, or
    None where the 16-bit weights must be streamed (packing disabled /
    unsupported shape)."""
    if not decode_pack.ENABLED or not decode_pack.packable(w):
        return None
    form = (bool(glu), int(half_tail))
    key = (w.data_ptr(), w._version, decode_pack.weight_generation(), w.dtype, tuple(w.shape))
    cache = getattr(w, "_ema_decode_packed_mxfp4", None)
    if not isinstance(cache, dict):
        cache = {}
        w._ema_decode_packed_mxfp4 = cache
    hit = cache.get(form)
    if hit is not None and hit[0] == key:
        return hit[1]
    for f in [f for f, v in cache.items() if v[0] != key]:
        del cache[f]  # stale forms of an older generation
    with torch.no_grad():
        pair = pack_mxfp4(*quantize_blocks(w.detach()), glu, half_tail)
    cache[form] = (key, pair)
    return pair
