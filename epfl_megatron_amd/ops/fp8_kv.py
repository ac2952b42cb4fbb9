"""FP8 KV cache for decode: e4m3 keys and values (``--inference_fp8_kv_cache``).

The KV cache is the one stream of a decode step that grows with batch and
context.  Under the flag K and V are stored as OCP ``e4m3fn`` bytes (``uint8``
tensors in the 16-bit cache's layout ``[max_seq, max_batch, nkv, hd]``) with an
fp32 scale per KV head (``[2, nkv]``: row 0 the K scales, row 1 the V scales),
which halves both the bytes ``csrc/flash_decode.hip`` streams per step and the
memory the cache occupies.

Stored value: ``byte = e4m3_rne(clamp(x * (1 / scale), -448, 448))`` where ``x``
is the value the 16-bit cache would have held (K after RoPE, rounded to the
model dtype).  The clamp comes first: the convert alone turns an overflow into
NaN.  The kernels multiply by the reciprocal, which is exact for power-of-two
scales.  The decode kernel expands the bytes to fp32 (exact), folds the K scale
into the score scale and the V scale into the final normalisation.

This module holds the torch quantiser / dequantiser (the reference
transcription that the kernels are tested against bit for bit), the
calibration rule and the wrappers of the HIP store kernel.
"""
import torch

from ._ext import ext, use_native

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def new_scales(nkv, device):
    """Scales of one layer's cache: fp32 ``[2, nkv]``, all 1.0."""
    return torch.ones(2, nkv, dtype=torch.float32, device=device)


def quantize(x, scale):
    """``x [..., nkv, hd]`` (any float dtype) and ``scale [nkv]`` fp32 -> the
    e4m3fn bytes as ``uint8`` of ``x``'s shape."""
    inv = (1.0 / scale.float()).to(x.device)
    return (x.float() * inv[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8).view(torch.uint8)


def dequantize(q, scale, dtype=torch.float32):
    """The values ``q [..., nkv, hd]`` (uint8 e4m3fn bytes) stands for, in
    ``dtype`` (exact in fp32; exact in bf16 / fp16 for power-of-two scales
    within the format's range)."""
    return (q.view(FP8).float() * scale.float().to(q.device)[:, None]).to(dtype)


def calibrate_(scales, k, v):
    """Set ``scales [2, nkv]`` in place from the prompt's ``k / v [sq, b, nkv,
    hd]``: ``2 amax / 448`` rounded up to a power of two (a factor of two of
    headroom for later tokens, which saturate beyond it), 1.0 where ``amax ==
    0``.  Device-side torch ops only: no host sync."""
    for row, t in ((0, k), (1, v)):
        amax = t.detach().float().abs().amax(dim=(0, 1, 3))
        # 2^ceil(log2(s)) without a transcendental: s = m 2^e, m in [0.5, 1)
        m, e = torch.frexp(2.0 * amax / FP8_MAX)
        s = torch.ldexp(torch.ones_like(amax), torch.where(m == 0.5, e - 1, e))
        scales[row].copy_(torch.where(amax == 0, torch.ones_like(s), s))


def store_native_ok(k):
    """The HIP store kernel takes these rows (GPU, bf16 / fp16, head dim a
    multiple of 8, 16-byte aligned strided rows)."""
    return (use_native(k) and k.dtype in (torch.bfloat16, torch.float16) and k.dim() == 4
            and k.shape[-1] % 8 == 0 and k.stride(-1) == 1
            and all(s % 8 == 0 for s in k.stride()[:3]) and k.data_ptr() % 16 == 0)


def store(k, v, kcache, vcache, scales, slot=0, slot_t=None):
    """Quantise ``k / v [sq, b, nkv, hd]`` into rows ``slot .. slot + sq - 1`` of
    the caches ``[L, >= b, nkv, hd]`` (uint8 views at the batch offset);
    ``slot_t``: the slot as an int64 device scalar (hipGraph decode), or with
    ``sq == 1`` and ``b > 1`` elements one slot per sequence (ragged decode).
    One HIP launch on the GPU, the torch quantiser elsewhere."""
    sq, b = k.shape[:2]
    if store_native_ok(k) and store_native_ok(v):
        ext().kv_store_fp8(k, v, kcache, vcache, scales, slot_t, int(slot))
        return
    qk, qv = quantize(k, scales[0]), quantize(v, scales[1])
    if slot_t is not None and sq == 1 and b > 1 and slot_t.numel() == b:
        rows = torch.arange(b, device=qk.device)
        kcache[slot_t, rows] = qk[0]
        vcache[slot_t, rows] = qv[0]
    elif slot_t is not None:
        kcache[:, :b].index_copy_(0, slot_t, qk)
        vcache[:, :b].index_copy_(0, slot_t, qv)
    else:
        kcache[slot:slot + sq, :b] = qk
        vcache[slot:slot + sq, :b] = qv
