"""FP8 weight-only decode: e4m3 weights for the weight-streaming skinny GEMMs.

A decode step is the weight stream from HBM (``ops/decode_pack.py``); with
``--inference_fp8_weights`` the four per-layer products stream one byte per
weight instead of two.  Only the stored weights change: each W row is scaled
to the OCP ``e4m3fn`` range, the kernel (``csrc/skinny_gemm.hip``, W8 forms)
expands the bytes to bf16 / fp16 (exact) in front of the same MFMAs, and the
fp32 sums are multiplied by the row scale before the epilogue's first
rounding.  Activations, the KV cache, the LM head, the embeddings and the
prefill (hipBLASLt on the 16-bit weights) are untouched, and the 16-bit
parameters stay: this buys bandwidth, not memory.

Quantiser (:func:`quantize_rows`): ``scale[n] = amax(|W[n]|) / 448`` (fp32;
an all-zero row gets 1), ``q = (W / scale).clamp(-448, 448)`` rounded to
``float8_e4m3fn``.  ``pow2=True`` rounds the scale up to a power of two, so
that ``q * scale`` is exact in bf16 / fp16 and the scaled sums are exact
multiples of the unscaled ones (tests; :data:`POW2_SCALES`).

Packed FP8 layout (K % 256 == 0, S = K / 256 k-steps of 32 per wave, 8
waves; the same block / wave / k-step / lane structure as ``decode_pack``).
The ring's loads stay 16 B per lane: one lane's piece holds its 8 e4m3 values
of TWO consecutive k-steps.  Per (block b, wave) the stream is S x 512 bytes:
``S // 2`` two-step units of 1 KiB,
``unit[p][q, r, h, e] = Q[row(b, r), wave * 32 S + 32 (2 p + h) + 8 q + e]``
(lane L = 16 q + r at byte 16 L, k-step 2 p in its low 8 bytes, 2 p + 1 in
the high ones), and, when S is odd (Llama-2-7B fc2: K = 11008, S = 43), the
last k-step as one 512-B unit of 8-B pieces ``[q, r, e]`` (lane L at byte
8 L).  Nothing is padded: the packed tensor keeps the ``[N, K]`` shape and the
kernel never reads X past K.  ``row(b, r)`` is ``decode_pack``'s (plain / QKV:
``16 b + r``; GLU: 8 up rows then the 8 matching gate rows).  The last
``half_tail`` GLU blocks follow as half units (the persistent kernel's last
round, K = 4096 / 8192, S even): per (half unit, wave) ``S // 2`` two-step
units of 512 B, ``[q, pr, h, e]`` with ``pr`` = the 4 up then the 4 gate rows
(the piece of MFMA rows r and r + 4 at byte ``16 (8 q + pr)``).  The k index
a lane feeds to the MFMA and the ascending k-step order are those of the
16-bit pack.  The scales stay in original W row order (``[N]``; GLU ``[2F]``,
up rows then gate rows).

The cached ``(packed, scale)`` pairs live next to the parameter
(``_ema_decode_packed_fp8``) under ``decode_pack.packed``'s key and
invalidation rules (storage pointer, ``_version``, weight generation, form);
they do not touch the 16-bit packs.
"""
import os

import torch

from . import decode_pack

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
# power-of-two row scales in packed_fp8 (exactness tests; EMA_FP8_POW2_SCALES=1)
POW2_SCALES = os.environ.get("EMA_FP8_POW2_SCALES", "0") == "1"


def quantize_rows(w, pow2=False):
    """Per-row e4m3 quantisation of ``w`` [N, K] (bf16 / fp16, CPU or GPU):
    ``(q, scale)`` with ``q`` float8_e4m3fn [N, K] and ``scale`` fp32 [N]."""
    assert w.dim() == 2 and w.dtype in (torch.bfloat16, torch.float16), (w.shape, w.dtype)
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = amax / FP8_MAX
    if pow2:
        # 2^ceil(log2(scale)) without a transcendental: scale = m 2^e, m in [0.5, 1)
        m, e = torch.frexp(scale)
        scale = torch.ldexp(torch.ones_like(scale), torch.where(m == 0.5, e - 1, e))
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, scale


def packable(q):
    """Q [N, K] the packed FP8 skinny forms can read."""
    return q.dim() == 2 and q.shape[1] % 256 == 0 and q.shape[0] % 16 == 0


def _blocks(b, n, k, glu):
    """[N, K] bytes -> [N / 16, 16 MFMA rows, K] (decode_pack's ``row(b, r)``)."""
    if glu:
        f = n // 2
        return torch.stack((b[:f].reshape(f // 8, 8, k), b[f:].reshape(f // 8, 8, k)), 1) \
            .reshape(f // 8, 16, k)
    return b.reshape(n // 16, 16, k)


def pack_fp8(q, glu=False, half_tail=0):
    """The packed copy of ``q`` ([N, K] float8_e4m3fn -> [N, K], same device)."""
    assert q.dtype == FP8 and packable(q), f"fp8 pack: unsupported weight {tuple(q.shape)} {q.dtype}"
    assert glu or not half_tail
    n, k = q.shape
    s = k // 256
    sp = s // 2
    assert not half_tail or s % 2 == 0, "half units come in two-step pieces"
    blocks = _blocks(q.view(torch.uint8), n, k, glu)
    nb = blocks.shape[0]
    full = nb - half_tail
    x = blocks[:full].reshape(full, 16, 8, s, 4, 8)  # [b, r, wave, s, q, e]
    # pairs [b, r, wave, p, h, q, e] -> [b, wave, p, q, r, h, e]: lane q * 16 + r, 16 B
    parts = [x[:, :, :, :2 * sp].reshape(full, 16, 8, sp, 2, 4, 8)
             .permute(0, 2, 3, 5, 1, 4, 6).reshape(full, 8, sp * 1024)]
    if s % 2:  # the odd last k-step: [b, r, wave, q, e] -> [b, wave, q, r, e], 8 B per lane
        parts.append(x[:, :, :, s - 1].permute(0, 2, 3, 1, 4).reshape(full, 8, 512))
    out = [torch.cat(parts, 2).reshape(-1)]
    if half_tail:
        t = blocks[full:].reshape(half_tail, 2, 2, 4, k)  # [b, up|gate, half, row, k]
        t = t.permute(0, 2, 1, 3, 4).reshape(half_tail, 2, 8, 8, sp, 2, 4, 8)  # [b, half, pr, wave, p, h, q, e]
        out.append(t.permute(0, 1, 3, 4, 6, 2, 5, 7).reshape(-1))  # [b, half, wave, p, q, pr, h, e]
    return torch.cat(out).reshape(n, k).view(FP8)


def unpack_fp8(p, glu=False, half_tail=0):
    """Inverse of ``pack_fp8`` (tests)."""
    n, k = p.shape
    s = k // 256
    sp = s // 2
    nb = n // 16
    full = nb - half_tail
    flat = p.view(torch.uint8).reshape(-1)
    per = flat[:full * 16 * k].reshape(full, 8, s * 512)
    x = torch.empty(full, 16, 8, s, 4, 8, dtype=torch.uint8, device=p.device)
    # [b, wave, p, q, r, h, e] -> [b, r, wave, p, h, q, e]
    x[:, :, :, :2 * sp] = per[:, :, :sp * 1024].reshape(full, 8, sp, 4, 16, 2, 8) \
        .permute(0, 4, 1, 2, 5, 3, 6).reshape(full, 16, 8, 2 * sp, 4, 8)
    if s % 2:
        x[:, :, :, s - 1] = per[:, :, sp * 1024:].reshape(full, 8, 4, 16, 8).permute(0, 3, 1, 2, 4)
    blocks = [x.reshape(full, 16, k)]
    if half_tail:
        t = flat[full * 16 * k:].reshape(half_tail, 2, 8, sp, 4, 8, 2, 8)
        t = t.permute(0, 1, 5, 2, 3, 6, 4, 7)  # [b, half, pr, wave, p, h, q, e]
        t = t.reshape(half_tail, 2, 2, 4, k).permute(0, 2, 1, 3, 4)  # [b, up|gate, half, row, k]
        blocks.append(t.reshape(half_tail, 16, k))
    blocks = torch.cat(blocks)
    if glu:
        f = n // 2
        out = torch.cat((blocks[:, :8].reshape(f, k), blocks[:, 8:].reshape(f, k)), 0)
    else:
        out = blocks.reshape(n, k)
    return out.contiguous().view(FP8)


def packed_fp8(w, glu=False, half_tail=0):
    """Cached ``(packed e4m3 weight, fp32 row scales)`` of parameter ``w``, or
    None where the 16-bit weights must be streamed (packing disabled /
    unsupported shape)."""
    if not decode_pack.ENABLED or not decode_pack.packable(w):
        return None
    pow2 = bool(POW2_SCALES)
    form = (bool(glu), int(half_tail), pow2)
    key = (w.data_ptr(), w._version, decode_pack.weight_generation(), w.dtype, tuple(w.shape))
    cache = getattr(w, "_ema_decode_packed_fp8", None)
    if not isinstance(cache, dict):
        cache = {}
        w._ema_decode_packed_fp8 = cache
    hit = cache.get(form)
    if hit is not None and hit[0] == key:
        return hit[1]
    for f in [f for f, v in cache.items() if v[0] != key]:
        del cache[f]  # stale forms of an older generation
    with torch.no_grad():
        q, scale = quantize_rows(w.detach(), pow2)
        pair = (pack_fp8(q, glu, half_tail), scale.contiguous())
    cache[form] = (key, pair)
    return pair
