"""Fused attention.

``flash_attn_qkvpacked`` is the training hot path: it takes the fused QKV
projection output in the reference's GQA layout ``[s, b, ng, r+2, hd]``
(r = nq/nkv query heads per KV group, then k, then v;
reference ``megatron/model/transformer.py:445-455``) and runs the
hand-written gfx950 FlashAttention-2 kernel
(``csrc/flash_attn_fwd.hip`` / ``flash_attn_bwd.hip``) reading Q/K/V through
strides.  GQA/MQA is native: query head ``j`` reads KV group ``j // r``; K/V
are never expanded to ``nq`` heads (the reference broadcast them, D2).
RoPE is fused: a k-only pass rotates the key heads, the forward kernel
rotates Q in registers (and writes it back for the backward), and the
backward kernels apply R^T to dQ/dK in their epilogues while writing them
straight into a ``[s, b, ng, r+2, hd]`` gradient buffer for the QKV GEMM
backward.

``flash_attn_func`` is the general entry (separate q/k/v, ``sq <= sk`` with
bottom-right-aligned causal mask) used by KV-cached inference; single-token
decode steps go to the split-key decode kernel (``csrc/flash_decode.hip``).

CPU tensors use an exact fp32 math reference (GPU test oracle and the gloo
plumbing path).
"""
import math
import os

import torch

from ._ext import ext, use_native
from .rope import rope_qkv_inplace, apply_rope_ref


# --------------------------------------------------------------------------
# Reference math (CPU path + test oracle)
# --------------------------------------------------------------------------
def attention_ref(q, k, v, causal=True, softmax_scale=None, return_lse=False, doc_bounds=None,
                  window=0):
    """q ``[b, sq, nq, d]``, k/v ``[b, sk, nkv, d]`` -> ``[b, sq, nq, d]`` (fp32 math).

    ``doc_bounds``: optional int32 ``[2, b, s]`` (document start, end) of
    packed sequences: query i sees key j only if ``doc_start[i] <= j``.
    ``window`` (W >= 1, causal only; 0: none): query i sees key j only if
    ``i + (sk - sq) - W < j``."""
    _check_window(window, causal)
    b, sq, nq, d = q.shape
    sk, nkv = k.shape[1], k.shape[2]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    rep = nq // nkv
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(sq, device=q.device)[:, None]
        j = torch.arange(sk, device=q.device)[None, :]
        s = s.masked_fill(j > i + (sk - sq), float("-inf"))
        if window:
            s = s.masked_fill(j <= i + (sk - sq) - window, float("-inf"))
    if doc_bounds is not None:
        j = torch.arange(sk, device=q.device)[None, None, :]
        before = j < doc_bounds[0].to(q.device).long()[:, :, None]  # [b, sq, sk]
        s = s.masked_fill(before[:, None], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, vf).permute(0, 2, 1, 3).to(q.dtype)
    if return_lse:
        return o, lse
    return o


def _check_window(window, causal):
    if window < 0 or (window and not causal):
        raise ValueError("a sliding window must be >= 1 (0: none) and needs causal attention")


def _split_qkv5(qkv5):
    s, b, ng, r2, hd = qkv5.shape
    r = r2 - 2
    q = qkv5[:, :, :, :r, :].reshape(s, b, ng * r, hd)
    k = qkv5[:, :, :, r, :]
    v = qkv5[:, :, :, r + 1, :]
    return q, k, v


# --------------------------------------------------------------------------
# Native path
# --------------------------------------------------------------------------
# One kernel signature serves every layout: each operand is a (tensor view,
# strides) pair.  Query head j lives at (j // r) * q_sg + (j % r) * q_sh and
# reads KV group j // r at g * k_sg; all strides are in elements.
def _qkv5_views(qkv5):
    s, b, ng, r2, hd = qkv5.shape
    r = r2 - 2
    ss, sb, sg, sh, sd = qkv5.stride()
    if sd != 1:
        raise AssertionError("head_dim must be contiguous")
    q = qkv5[:, :, :, 0, :]
    k = qkv5[:, :, :, r, :]
    v = qkv5[:, :, :, r + 1, :]
    qs = (sb, ss, sg, sh)
    ks = (sb, ss, sg)
    return q, k, v, qs, ks


def _bsnd_strides(t, r):
    """[b, s, n, d] tensor -> (sb, ss, sg, sh) with group stride r*sh."""
    sb, ss, sh, sd = t.stride()
    if sd != 1:
        raise AssertionError("head_dim must be contiguous")
    return (sb, ss, r * sh, sh)


class _FlashQKVPackedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, ng, r, hd, causal, scale, cos, sin, position_ids, docs, window=0):
        s, b = qkv.shape[0], qkv.shape[1]
        qkv5 = qkv.view(s, b, ng, r + 2, hd)
        if position_ids is not None and position_ids.dtype != torch.int64:
            position_ids = position_ids.long()
        if cos is not None:  # keys only: Q is rotated inside the attention kernel
            rope_qkv_inplace(qkv5, cos, sin, position_ids, k_only=True)
        q, k, v, qs, ks = _qkv5_views(qkv5)
        nq = ng * r
        out = torch.empty(s, b, nq, hd, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(b, nq, s, dtype=torch.float32, device=qkv.device)
        os_ = (out.stride(1), out.stride(0), out.stride(2))
        ext().flash_attn_fwd(q, k, v, out, lse, b, s, s, nq, ng, hd,
                             list(qs), list(ks), list(ks), list(os_), bool(causal), float(scale),
                             cos, sin, position_ids, docs, window=int(window))
        ctx.save_for_backward(qkv, out, lse, cos, sin, position_ids, docs)
        ctx.meta = (ng, r, hd, causal, scale)
        ctx.window = int(window)
        return out.view(s, b, nq * hd)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cos, sin, position_ids, docs = ctx.saved_tensors
        ng, r, hd, causal, scale = ctx.meta
        s, b = qkv.shape[0], qkv.shape[1]
        nq = ng * r
        qkv5 = qkv.view(s, b, ng, r + 2, hd)
        dout = dout.reshape(s, b, nq, hd)
        if not dout.is_contiguous():
            dout = dout.contiguous()
        dqkv5 = torch.empty_like(qkv5)
        q, k, v, qs, ks = _qkv5_views(qkv5)
        dq, dk, dv, _, _ = _qkv5_views(dqkv5)
        os_ = (out.stride(1), out.stride(0), out.stride(2))
        ext().flash_attn_bwd(dout, q, k, v, out, lse, dq, dk, dv, b, s, s, nq, ng, hd,
                             list(qs), list(ks), list(ks), list(os_), bool(causal), float(scale),
                             cos, sin, position_ids, docs, window=ctx.window)
        return dqkv5.view(s, b, -1), None, None, None, None, None, None, None, None, None, None


def _flash_decode(q, k, v, scale, kv_len=None, window=0, kv_scale=None, page_table=None, sk=None):
    """sq == 1 against a KV cache (generation): split-key decode kernel
    (``csrc/flash_decode.hip``); no autograd.  ``kv_len``: optional device
    int32 tensor with the number of valid keys (k / v then span the whole
    cache; the launch does not depend on the step, for hipGraph capture).
    ``window``: only the last ``window`` valid keys count (0: all).
    ``kv_scale``: fp32 ``[2, nkv]`` when k / v are an FP8 cache (uint8 e4m3fn
    bytes, ``ops/fp8_kv.py``).  ``page_table``: k / v are the pool of a paged
    cache ``[1, n_pages * KV_PAGE, nkv, d]`` and ``sk`` the logical capacity."""
    b, _, nq, d = q.shape
    nkv = k.shape[2]
    if page_table is None:
        sk = k.shape[1]
    r = nq // nkv
    out = torch.empty(b, 1, nq, d, dtype=q.dtype, device=q.device)
    ext().flash_decode(q, k, v, out, b, sk, nq, nkv, d, list(_bsnd_strides(q, r)),
                       list(_bsnd_strides(k, 1)[:3]), list(_bsnd_strides(v, 1)[:3]),
                       [out.stride(0), out.stride(1), out.stride(2)], float(scale), kv_len,
                       window=int(window), kv_scale=kv_scale, page_table=page_table)
    return out


def flash_decode_cached(q, k, v, kv_len, softmax_scale=None, window=0, kv_scale=None,
                        page_table=None, capacity=None):
    """One query row per sequence against a whole KV cache ``k / v [b, smax,
    nkv, d]`` of which the first ``kv_len`` (device int32) keys are valid
    (with ``window``: the last ``window`` of those).  ``kv_len`` None: all
    ``smax`` keys are valid.  ``kv_scale``: fp32 ``[2, nkv]`` when k / v are an
    FP8 cache (uint8 e4m3fn bytes, ``ops/fp8_kv.py``).  A ``kv_len`` of ``b >
    1`` elements holds one length per sequence (ragged decode): row ``i`` sees
    the keys ``[max(0, n_i - window), n_i)``, none (zeros) at ``n_i == 0``.

    ``page_table`` (int32 ``[>= b, pages_per_row]``): a paged cache
    (``inference/paged.py``).  k / v are then the pool ``[1, n_pages * KV_PAGE,
    nkv, d]``, key ``j`` of row ``i`` is pool row ``page_table[i, j // KV_PAGE] *
    KV_PAGE + j % KV_PAGE``, ``kv_len`` is required and ``capacity`` (default
    ``pages_per_row * KV_PAGE``) is the logical cache length that sizes the
    launch as ``smax`` does without a table."""
    _check_window(window, True)
    if page_table is not None:
        from ..inference.paged import KV_PAGE, gather_rows
        if kv_len is None:
            raise ValueError("a page_table needs kv_len (the keys each row's pages hold)")
        if capacity is None:
            capacity = page_table.shape[1] * KV_PAGE
        if capacity > page_table.shape[1] * KV_PAGE:
            raise ValueError("capacity exceeds the page_table's pages per row")
        if not use_native(q):
            # gather each row's pages into the contiguous cache and take the reference
            lens = kv_len.reshape(-1).tolist()
            lens = lens * q.shape[0] if len(lens) == 1 else lens
            rows = []
            for i in range(q.shape[0]):
                n = min(lens[i], capacity)
                if n <= 0:
                    rows.append(torch.zeros_like(q[i:i + 1]))
                    continue
                ki, vi = (gather_rows(t[0], page_table[i], n)[None] for t in (k, v))
                rows.append(flash_decode_cached(q[i:i + 1], ki, vi, None, softmax_scale, window,
                                                kv_scale))
            return torch.cat(rows, 0)
        scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
        return _flash_decode(q, k, v, scale, kv_len, window, kv_scale, page_table, int(capacity))
    if not use_native(q):
        if kv_len is not None and q.shape[0] > 1 and kv_len.numel() == q.shape[0]:
            rows = []
            for i, n in enumerate(kv_len.reshape(-1).tolist()):
                if min(n, k.shape[1]) <= 0:
                    rows.append(torch.zeros_like(q[i:i + 1]))
                else:
                    rows.append(flash_decode_cached(q[i:i + 1], k[i:i + 1], v[i:i + 1],
                                                    kv_len.reshape(-1)[i:i + 1], softmax_scale,
                                                    window, kv_scale))
            return torch.cat(rows, 0)
        n = int(kv_len.reshape(-1)[0]) if kv_len is not None else k.shape[1]
        lo = max(n - window, 0) if window else 0
        k, v = k[:, lo:n], v[:, lo:n]
        if kv_scale is not None:
            from . import fp8_kv
            k = fp8_kv.dequantize(k, kv_scale[0], q.dtype)
            v = fp8_kv.dequantize(v, kv_scale[1], q.dtype)
        return attention_ref(q, k, v, False,
                             softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1]))
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
    return _flash_decode(q, k, v, scale, kv_len, window, kv_scale)


# Native FP8 prefill (uint8 e4m3 K / V read in place by the FP8 forms of the
# forward kernel).  EMA_FA_FP8_PREFILL=0 / FP8_PREFILL_NATIVE = False: the
# fallback that gathers and dequantises into 16-bit tensors first (A/B knob).
FP8_PREFILL_NATIVE = os.environ.get("EMA_FA_FP8_PREFILL", "1") != "0"
# calls that took the native FP8 forms / the dequantising fallback (tests)
fp8_prefill_calls = {"native": 0, "fallback": 0}


def _fp8_prefill_native(q, k8, v8, kv_scale):
    """uint8 K / V of these queries go to the FP8 forms of the forward kernel."""
    d = q.shape[-1]
    ok = (FP8_PREFILL_NATIVE and use_native(q) and d in (64, 128)
          and q.dtype in (torch.bfloat16, torch.float16)
          and k8.is_cuda and v8.is_cuda and kv_scale.is_cuda)
    fp8_prefill_calls["native" if ok else "fallback"] += 1
    return ok


def _flash_fwd_fp8(q, k8, v8, kv_scale, sk, scale, window, page_table, waves, kv2):
    b, sq, nq, d = q.shape
    nkv = k8.shape[2]
    r = nq // nkv
    out = torch.empty(b, sq, nq, d, dtype=q.dtype, device=q.device)
    lse = torch.empty(b, nq, sq, dtype=torch.float32, device=q.device)
    ext().flash_attn_fwd(q, k8, v8, out, lse, b, sq, sk, nq, nkv, d,
                         list(_bsnd_strides(q, r)), list(_bsnd_strides(k8, 1)[:3]),
                         list(_bsnd_strides(v8, 1)[:3]),
                         [out.stride(0), out.stride(1), out.stride(2)], True, float(scale),
                         None, None, None, None, window=int(window), page_table=page_table,
                         waves=int(waves), kv2=int(kv2), kv_scale=kv_scale)
    return out


def flash_attn_fp8_kv(q, k8, v8, kv_scale, softmax_scale=None, window=0, waves=0, kv2=-1):
    """A block of queries over the keys of an FP8 cache (the continued prefill
    of ``--inference_fp8_kv_cache``).  ``q [b, sq, nq, d]`` holds the last
    ``sq`` of ``sk`` positions (causal, bottom-right aligned); ``k8 / v8 [b, sk,
    nkv, d]`` are uint8 views of e4m3fn bytes (any strides with ``d``
    contiguous and 16-byte aligned rows: the cache ``[max_seq, max_batch, nkv,
    d]`` sliced and transposed) and ``kv_scale`` is fp32 ``[2, nkv]``
    (``ops/fp8_kv.py``).  No autograd.

    On the GPU (bf16 / fp16 queries, head_dim 64 / 128) the FP8 forms of the
    forward kernel read the bytes in place; everything else dequantises into
    ``q``'s dtype and runs the contiguous attention.  ``waves`` / ``kv2`` force
    a kernel form (tests)."""
    _check_window(window, True)
    if k8.dtype != torch.uint8 or v8.dtype != torch.uint8:
        raise ValueError("flash_attn_fp8_kv: k8 / v8 must be uint8 (e4m3fn bytes)")
    if kv_scale is None:
        raise ValueError("flash_attn_fp8_kv: an FP8 (uint8) cache needs its kv_scale tensor")
    b, sq, nq, d = q.shape
    sk = k8.shape[1]
    if not 0 < sq <= sk:
        raise ValueError(f"flash_attn_fp8_kv: q holds the last sq of sk positions (sq {sq}, sk {sk})")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    if _fp8_prefill_native(q, k8, v8, kv_scale):
        return _flash_fwd_fp8(q, k8, v8, kv_scale, sk, scale, window, None, waves, kv2)
    from . import fp8_kv
    k = fp8_kv.dequantize(k8, kv_scale[0], q.dtype)
    v = fp8_kv.dequantize(v8, kv_scale[1], q.dtype)
    with torch.no_grad():
        return flash_attn_func(q, k, v, causal=True, softmax_scale=scale, window=window)


def flash_attn_paged(q, k_pool, v_pool, page_table, sk, softmax_scale=None, window=0,
                     kv_scale=None, waves=0, kv2=-1):
    """A block of queries over keys that live in pages (the continued prefill
    of a paged KV cache, ``inference/paged.py``).  ``q [b, sq, nq, d]`` holds
    the last ``sq`` of ``sk`` logical positions (causal, bottom-right aligned),
    the pools are ``[1, n_pages * KV_PAGE, nkv, d]`` and key ``j`` of row ``i``
    is pool row ``page_table[i, j // KV_PAGE] * KV_PAGE + j % KV_PAGE``
    (``page_table`` int32 ``[>= b, pages_per_row]``).  No autograd.

    Native pools go to the paged forms of the forward kernel
    (``csrc/flash_attn_fwd.hip``), which read the pages in place: 16-bit pools
    of ``q``'s dtype, and FP8 pools (uint8 e4m3fn bytes with ``kv_scale`` fp32
    ``[2, nkv]``), which the FP8 forms expand on the way to LDS.  Everything
    else (CPU, fp32, other head dims, ``EMA_FA_FP8_PREFILL=0``) gathers each
    row's first ``sk`` keys, dequantises FP8 bytes, and runs the contiguous
    attention on them.  ``waves`` / ``kv2`` force a
    kernel form (tests), as the ``flash_attn_fwd`` binding takes them."""
    from ..inference.paged import KV_PAGE, gather_rows
    _check_window(window, True)
    b, sq, nq, d = q.shape
    sk = int(sk)
    if not 0 < sq <= sk:
        raise ValueError(f"flash_attn_paged: q holds the last sq of sk positions (sq {sq}, sk {sk})")
    if sk > page_table.shape[1] * KV_PAGE:
        raise ValueError("flash_attn_paged: sk exceeds the page_table's pages per row")
    fp8 = k_pool.dtype == torch.uint8
    if fp8 != (kv_scale is not None):
        raise ValueError("an FP8 (uint8) pool needs its kv_scale tensor" if fp8
                         else "kv_scale given for a 16-bit pool")
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    if not fp8 and use_native(q) and d in (64, 128) and k_pool.dtype == q.dtype:
        nkv = k_pool.shape[2]
        r = nq // nkv
        out = torch.empty(b, sq, nq, d, dtype=q.dtype, device=q.device)
        lse = torch.empty(b, nq, sq, dtype=torch.float32, device=q.device)
        ext().flash_attn_fwd(q, k_pool, v_pool, out, lse, b, sq, sk, nq, nkv, d,
                             list(_bsnd_strides(q, r)), list(_bsnd_strides(k_pool, 1)[:3]),
                             list(_bsnd_strides(v_pool, 1)[:3]),
                             [out.stride(0), out.stride(1), out.stride(2)], True, float(scale),
                             None, None, None, None, window=int(window), page_table=page_table,
                             waves=int(waves), kv2=int(kv2))
        return out
    if fp8 and _fp8_prefill_native(q, k_pool, v_pool, kv_scale):
        return _flash_fwd_fp8(q, k_pool, v_pool, kv_scale, sk, scale, window, page_table, waves, kv2)
    k = torch.stack([gather_rows(k_pool[0], page_table[i], sk) for i in range(b)])
    v = torch.stack([gather_rows(v_pool[0], page_table[i], sk) for i in range(b)])
    if fp8:
        from . import fp8_kv
        k = fp8_kv.dequantize(k, kv_scale[0], q.dtype)
        v = fp8_kv.dequantize(v, kv_scale[1], q.dtype)
    with torch.no_grad():
        return flash_attn_func(q, k, v, causal=True, softmax_scale=scale, window=window)


class _FlashFn(torch.autograd.Function):
    """Separate q ``[b, sq, nq, d]``, k/v ``[b, sk, nkv, d]``."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, window=0):
        b, sq, nq, d = q.shape
        sk, nkv = k.shape[1], k.shape[2]
        r = nq // nkv
        out = torch.empty(b, sq, nq, d, dtype=q.dtype, device=q.device)
        lse = torch.empty(b, nq, sq, dtype=torch.float32, device=q.device)
        qs = _bsnd_strides(q, r)
        ks = _bsnd_strides(k, 1)[:3]
        vs = _bsnd_strides(v, 1)[:3]
        os_ = (out.stride(0), out.stride(1), out.stride(2))
        ext().flash_attn_fwd(q, k, v, out, lse, b, sq, sk, nq, nkv, d,
                             list(qs), list(ks), list(vs), list(os_), bool(causal), float(scale),
                             None, None, None, None, window=int(window))
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal, ctx.scale, ctx.window = causal, scale, int(window)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        b, sq, nq, d = q.shape
        sk, nkv = k.shape[1], k.shape[2]
        r = nq // nkv
        dout = dout.contiguous()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        qs = _bsnd_strides(q, r)
        ks = _bsnd_strides(k, 1)[:3]
        os_ = (out.stride(0), out.stride(1), out.stride(2))
        ext().flash_attn_bwd(dout, q, k, v, out, lse, dq, dk, dv, b, sq, sk, nq, nkv, d,
                             list(qs), list(ks), list(ks), list(os_), bool(ctx.causal),
                             float(ctx.scale), None, None, None, None, window=ctx.window)
        return dq, dk, dv, None, None, None


def flash_attn_qkvpacked(qkv, num_groups, q_per_group, head_dim, causal=True,
                         softmax_scale=None, rope=None, position_ids=None, doc_bounds=None,
                         window=0):
    """qkv ``[s, b, ng*(r+2)*hd]`` -> context ``[s, b, ng*r*hd]``.

    ``rope`` = (cos, sin) tables or None.  ``doc_bounds``: int32 ``[2, b, s]``
    document (start, end) per position for packed sequences
    (``--reset_attention_mask``; :func:`utils.misc.doc_bounds`), or None.
    ``window``: sliding-window size (query i sees keys ``i - window + 1 .. i``;
    0: none)."""
    _check_window(window, causal)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(head_dim)
    cos, sin = rope if rope is not None else (None, None)
    if doc_bounds is not None:
        if not causal:
            raise ValueError("document masking is defined for causal attention only")
        doc_bounds = doc_bounds.to(device=qkv.device, dtype=torch.int32).contiguous()
    if use_native(qkv):
        return _FlashQKVPackedFn.apply(qkv, num_groups, q_per_group, head_dim, causal, scale,
                                       cos, sin, position_ids, doc_bounds, window)
    s, b = qkv.shape[0], qkv.shape[1]
    qkv5 = qkv.view(s, b, num_groups, q_per_group + 2, head_dim)
    q, k, v = _split_qkv5(qkv5)
    if cos is not None:
        q = apply_rope_ref(q, cos, sin, position_ids)
        k = apply_rope_ref(k, cos, sin, position_ids)
    o = attention_ref(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), causal, scale,
                      doc_bounds=doc_bounds, window=window)
    return o.transpose(0, 1).reshape(s, b, -1)


def flash_attn_func(q, k, v, causal=True, softmax_scale=None, window=0):
    """Separate tensors ``[b, s, n, d]`` (inference / generic callers).
    ``window``: sliding-window size relative to the bottom-right-aligned
    diagonal (0: none)."""
    _check_window(window, causal)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if use_native(q):
        b, sq, nq = q.shape[:3]
        r = nq // k.shape[2]
        if sq == 1 and (r >= 2 or nq * b < 256 or k.shape[1] <= 512) and not (
                torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)):
            # split-key decode: GQA/MQA reads each K/V byte once; small grids
            # spread over the chunks; short caches (profiles/r2f_decode_bench.txt)
            # the last position sees every cached key (of its window)
            return _flash_decode(q, k, v, scale, window=window)
        return _FlashFn.apply(q, k, v, causal, scale, window)
    return attention_ref(q, k, v, causal, scale, window=window)
