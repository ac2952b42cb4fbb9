"""One attention layer's KV cache during one model call: where it lives, where
the new rows go and which attention kernel reads it.

``ip.key_value_memory_dict[layer] = (K, V)`` on the ``InferenceParams`` is a
column per row ``[max_seq, max_batch, nkv, hd]``, or with ``ip.kv_pages`` a pool
``[kv_pages * KV_PAGE, 1, nkv, hd]`` that ``ip.page_table`` addresses
(``inference/paged.py``); in the model dtype, or under the FP8 switch e4m3 bytes
(``uint8``) with the scales ``ip.kv_scale_dict[layer]`` (``ops/fp8_kv.py``).

The cells that exist, by ``step_kind`` (``LayerKV._check`` refuses the rest):

- device-slot decode (``hip_graph.py``, ``continuous.py``): the new row goes to
  ``ip.device_offset`` (one slot, or one per row) and ``flash_decode_cached``
  reads ``ip.device_kv_len`` keys of the whole cache.  Paged: one slot per row
  only (pool rows), read through the table.
- device-slot multi-row step (opt-in: ``ip.device_multi``, with ``sq`` in 2..16
  and ``ip.device_offset`` set): the ``sq`` new rows go to ``ip.device_offset +
  t`` (the slot of each sequence's first new row, one value or one per row;
  paged: physical, and the later rows through the table) and
  ``flash_decode_cached`` reads ``ip.device_kv_len`` keys, the count after the
  ``sq`` rows.  No host value is read.  Not with FP8 calibration.  On the GPU
  (bf16 / fp16, head dim 64 / 128) RoPE and the write are one launch,
  ``write_multi_native`` (``csrc/kv_write_multi.hip``); elsewhere the layer's
  RoPE pass and ``_write_multi`` in torch.  Callers: the speculative decoders
  (``inference/speculative.py``), whose verify step is this cell.
- the same step through the fused decode layer (opt-in: ``ip.device_multi ==
  "fused"``; any other truthy value keeps the unfused layer, and ``fused=True``
  is refused under it): the layer's QKV epilogue stores the ``sq * b`` rows by
  the same rules (``SkinnyArgs::seqs``, ``csrc/skinny_epi.h``) and
  ``decode_multi`` reads them.
- eager decode step: host slot ``s0``.  Not paged.
- restart prefill: host slot 0; attends over the fresh K / V (16-bit columns:
  over the cached rows).  Paged: one row, scattered by its table.
- continued prefill: host slot ``s0``; FP8 columns through ``flash_attn_fp8_kv``.
  Paged: one row under ``ip.continue_prefill``, through ``flash_attn_paged``.

The FP8 kernels of the unfused layer need the GPU, head dim 64 or 128 and
``--use_flash_attn``; else the keys in hand are gathered / dequantised for
``flash_attn_func`` or the layer's core attention.  The fused decode layer
(``models/transformer.py``) stores the new row in its QKV epilogue: it takes
``kc``, ``vc``, ``slot_t``, ``slot``, ``scales`` and calls ``decode``
(``decode_multi`` in the multi-row cell).
"""
import os

import torch

from ..ops import fp8_kv
from ..ops._ext import ext, use_native
from ..ops.attention import (flash_attn_fp8_kv, flash_attn_func, flash_attn_paged,
                             flash_decode_cached)
from .paged import KV_PAGE, gather_rows, physical_slots

# FP8 KV cache (--inference_fp8_kv_cache, opt-in): caches allocated under the
# switch hold e4m3 bytes with a scale per KV head (ops/fp8_kv.py); the decode
# steps read them in csrc/flash_decode.hip's FP8 forms.  With calibration
# (--inference_fp8_kv_calibrate) the prefill that restarts a cache sets the
# scales from the prompt; else they stay 1.0.
FP8_KV = os.environ.get("EMA_FP8_KV", "0") == "1"
FP8_KV_CALIBRATE = os.environ.get("EMA_FP8_KV_CALIBRATE", "0") == "1"
# The multi-row device step's RoPE + cache write in one HIP launch
# (LayerKV.write_multi_native); off: the separate RoPE pass and _write_multi in
# torch, bit for bit the same cache (scripts/serve_bench.py --torch_front times both)
WRITE_MULTI_NATIVE = os.environ.get("EMA_KV_WRITE_MULTI", "1") == "1"


def set_fp8_kv_cache(on, calibrate=None):
    """Switch the FP8 KV cache for every cache allocated from now on (and,
    with ``calibrate``, the prompt calibration of its scales)."""
    global FP8_KV, FP8_KV_CALIBRATE
    FP8_KV = bool(on)
    if calibrate is not None:
        FP8_KV_CALIBRATE = bool(calibrate)


DEVICE_DECODE = "device-slot decode"
EAGER_DECODE = "eager decode"
RESTART_PREFILL = "restart prefill"
CONTINUED_PREFILL = "continued prefill"
DEVICE_MULTI = "device-slot multi-row step"


def step_kind(ip, sq):
    """Which of the steps a call with ``sq`` new tokens per row is (the
    multi-row device step only under ``ip.device_multi``: the graphed decoders
    keep ``device_offset`` set while their prefills run)."""
    if sq == 1:
        return EAGER_DECODE if ip.device_offset is None else DEVICE_DECODE
    if ip.device_offset is not None and getattr(ip, "device_multi", False):
        return DEVICE_MULTI
    return RESTART_PREFILL if ip.sequence_len_offset == 0 else CONTINUED_PREFILL


class LayerKV:
    """The cache of layer ``layer_number`` for one call of ``b`` rows with ``sq``
    new tokens each, allocated on ``ip`` on first use.  Built per call and not
    kept: ``ip.page_table`` and the offsets are read as they are now.
    ``kc / vc``: the cache as the store kernels take it, ``[L, b, nkv, hd]``:
    the columns of the call's rows, or the pool as a stride-0 batch view, so
    that row ``m`` lands at the pool row ``ip.device_offset[m]`` (kept physical
    by the ragged decoders).  ``slot_t`` / ``slot``: the device slot tensor or
    the host slot of the new rows.  ``scales``: the FP8 scales or None."""

    def __init__(self, ip, layer_number, nkv, hd, params_dtype, device, sq, b, fused=False):
        self.ip = ip
        self.s0, self.b0 = s0, b0 = ip.sequence_len_offset, ip.batch_size_offset
        self.paged = paged = ip.page_table is not None
        mem = ip.key_value_memory_dict.get(layer_number)
        if mem is None:
            shape = (ip.kv_pages * KV_PAGE, 1, nkv, hd) if paged else \
                (ip.max_sequence_len, ip.max_batch_size, nkv, hd)
            # e4m3 bytes are zeroed: an unwritten row must not read as NaN
            new, dtype = (torch.zeros, torch.uint8) if FP8_KV else (torch.empty, params_dtype)
            mem = ip.key_value_memory_dict[layer_number] = (
                new(shape, dtype=dtype, device=device), new(shape, dtype=dtype, device=device))
        self.kmem, self.vmem = kmem, vmem = mem
        self.fp8 = kmem.dtype == torch.uint8
        self.scales = None
        if self.fp8:  # fp32 [2, nkv], 1.0 until set
            if layer_number not in ip.kv_scale_dict:
                ip.kv_scale_dict[layer_number] = fp8_kv.new_scales(nkv, device)
            self.scales = ip.kv_scale_dict[layer_number]
        on_gpu = device.type == "cuda"
        self.native = on_gpu and hd in (64, 128)
        self.kind = kind = step_kind(ip, sq)
        self._check(sq, b, fused, on_gpu)
        if paged:
            self.table = ip.page_table[b0:b0 + b]
            self.kc, self.vc = kmem.expand(-1, b, -1, -1), vmem.expand(-1, b, -1, -1)
        elif b0 == 0 and b == ip.max_batch_size:  # every column: the same view, unsliced
            self.kc, self.vc = kmem, vmem
        else:
            self.kc, self.vc = kmem[:, b0:b0 + b], vmem[:, b0:b0 + b]
        if kind in (DEVICE_DECODE, DEVICE_MULTI):
            self.slot_t, self.slot = ip.device_offset, 0
        else:
            self.slot_t, self.slot = None, s0

    def _check(self, sq, b, fused, on_gpu):
        """Every cell the cache does not serve is refused here."""
        ip, kind = self.ip, self.kind
        if kind == DEVICE_DECODE and on_gpu and not self.native:
            raise NotImplementedError("hipGraph decode needs the native decode attention "
                                      "kernel (GPU, bf16/fp16, head_dim 64 or 128)")
        if kind == DEVICE_MULTI:
            if fused and ip.device_multi != "fused":
                raise NotImplementedError("the fused decode layer takes a multi-row device step "
                                          "only under device_multi = \"fused\": any other value "
                                          "runs the unfused layer")
            if self.fp8 and FP8_KV_CALIBRATE:
                raise NotImplementedError("a multi-row device step does not calibrate the FP8 KV "
                                          "scales (--inference_fp8_kv_calibrate)")
            if sq > 16:
                raise NotImplementedError("a multi-row device step takes 2..16 rows per sequence")
            if ip.device_offset.numel() not in (1, b):
                raise NotImplementedError("a multi-row device step needs one device cache slot, "
                                          "or one per row")
            if self.paged and ip.device_offset.numel() != b:
                raise NotImplementedError("paged KV cache: a multi-row device step needs one "
                                          "device cache slot per row")
            return
        if not self.paged:
            return
        why = None
        if sq == 1:
            if kind == DEVICE_DECODE and ip.device_offset.numel() == b:
                return
            if kind == DEVICE_DECODE or fused:
                raise NotImplementedError(
                    "paged KV cache: a decode step needs one device cache slot per row (the "
                    "ragged decoders of inference/continuous.py); the eager loop and the "
                    "lockstep decoders of inference/hip_graph.py are not paged; use "
                    "kv_pages=None")
            why = "a decode step without device slots (the eager KV-cached loop)"
        elif kind == CONTINUED_PREFILL and not ip.continue_prefill:
            why = "a prefill that continues a cached sequence (sequence_len_offset > 0)"
        elif b > 1:
            why = "a prefill of more than one row"
        elif self.fp8 and FP8_KV_CALIBRATE:
            why = "prompt calibration of the FP8 KV scales (--inference_fp8_kv_calibrate)"
        if why is not None:
            raise NotImplementedError(f"paged KV cache: {why} is not supported (only the "
                                      "whole-prompt prefill of one row and the ragged decode "
                                      "step are); use kv_pages=None")

    def write(self, k, v):
        """Store the new rows ``k / v [sq, b, nkv, hd]`` (K already rotated)."""
        s0, sc, kc, vc, kmem, vmem = self.s0, self.scales, self.kc, self.vc, self.kmem, self.vmem
        sq, b = k.shape[:2]
        slots = self.slot_t
        if self.kind == DEVICE_MULTI:
            return self._write_multi(k, v)
        if self.paged:
            # the FP8 pool's HIP store kernel, else fp8_kv.quantize and torch indexing
            store8 = self.fp8 and fp8_kv.store_native_ok(k) and fp8_kv.store_native_ok(v)
            if slots is not None and store8:
                fp8_kv.store(k, v, kc, vc, sc, slot_t=slots)
            elif slots is not None:  # (a stride-0 view takes no indexed write)
                kmem[slots, 0] = fp8_kv.quantize(k[0], sc[0]) if self.fp8 else k[0]
                vmem[slots, 0] = fp8_kv.quantize(v[0], sc[1]) if self.fp8 else v[0]
            else:
                # the prompt's rows go to the pool rows its table names: device-side
                # indices (computed by the first layer of a prefill and shared by the
                # others: the table's version counter moves with every write to it)
                ip = self.ip
                key = (self.b0, s0, sq, id(ip.page_table), ip.page_table._version)
                if ip._prefill_slots[0] != key:
                    pos = torch.arange(s0, s0 + sq, device=k.device)
                    ip._prefill_slots = (key, physical_slots(self.table[0], pos))
                idx = ip._prefill_slots[1]
                if not store8:
                    kmem.index_copy_(0, idx, fp8_kv.quantize(k, sc[0]) if self.fp8 else k)
                    vmem.index_copy_(0, idx, fp8_kv.quantize(v, sc[1]) if self.fp8 else v)
                    return
                p0 = 0
                while p0 < sq:  # a page's rows are consecutive in the pool: cut at page edges
                    p1 = min(sq, ((s0 + p0) // KV_PAGE + 1) * KV_PAGE - s0)
                    fp8_kv.store(k[p0:p1], v[p0:p1], kmem, vmem, sc, slot_t=idx[p0:p0 + 1])
                    p0 = p1
        elif self.fp8:
            if slots is None and s0 == 0 and self.b0 == 0 and FP8_KV_CALIBRATE:
                fp8_kv.calibrate_(sc, k, v)
            fp8_kv.store(k, v, kc, vc, sc, slot=self.slot, slot_t=slots)
        elif slots is None:
            kc[s0:s0 + sq] = k
            vc[s0:s0 + sq] = v
        elif b > 1 and slots.numel() == b:
            # one slot per sequence (ragged decode, inference/continuous.py)
            rows = torch.arange(b, device=k.device)
            kc[slots, rows] = k[0]
            vc[slots, rows] = v[0]
        else:
            kc.index_copy_(0, slots, k)
            vc.index_copy_(0, slots, v)

    def write_multi_native(self, qkv5, rope, position_ids):
        """The front of a multi-row device step in one HIP launch
        (``csrc/kv_write_multi.hip``): RoPE of the q and k heads of the packed
        projection ``qkv5 [sq, b, g, r + 2, hd]`` in place (``rope``: the
        ``(cos, sin)`` tables or None) and the cache write of its k / v rows,
        as ``write`` does it after the separate RoPE pass, bit for bit.  False
        when the kernel does not take the call (``WRITE_MULTI_NATIVE`` off,
        CPU, fp32, another head dim, strides that lose the 16-byte alignment,
        RoPE without ``[b, sq]`` position ids or with tables of another width,
        a key count that is not int32): the caller then rotates and calls
        ``write``."""
        sq, b, hd = qkv5.shape[0], qkv5.shape[1], qkv5.shape[-1]
        ok = (WRITE_MULTI_NATIVE and self.kind == DEVICE_MULTI and self.native and use_native(qkv5)
              and qkv5.dtype in (torch.bfloat16, torch.float16) and qkv5.stride(-1) == 1
              and all(s % 8 == 0 for s in qkv5.stride()[:4]) and qkv5.data_ptr() % 16 == 0
              and self.kmem.dtype in (qkv5.dtype, torch.uint8)
              and not (torch.is_grad_enabled() and qkv5.requires_grad))
        if ok and rope is not None:
            ok = (position_ids is not None and tuple(position_ids.shape) == (b, sq)
                  and not position_ids.dtype.is_floating_point
                  and all(t.dtype == torch.float32 and t.is_contiguous()
                          and tuple(t.shape[1:]) == (hd // 2,) for t in rope))
        if ok and self.paged:
            ok = self.ip.device_kv_len.dtype == torch.int32 and self.table.dtype == torch.int32
        if not ok:
            return False
        cos, sin = rope if rope is not None else (None, None)
        pos = None if rope is None else position_ids.long().contiguous()
        ext().kv_write_multi(qkv5, cos, sin, pos, self.kc, self.vc,
                             self.slot_t.reshape(-1).long().contiguous(),
                             self.ip.device_kv_len.reshape(-1).contiguous() if self.paged else None,
                             self.scales, self.table.contiguous() if self.paged else None)
        return True

    def _write_multi(self, k, v):
        """The ``sq`` rows of a multi-row device step: row ``t`` of sequence ``m``
        to slot ``device_offset[m] + t``, all indices on the device."""
        sc, kmem, vmem = self.scales, self.kmem, self.vmem
        sq, b = k.shape[:2]
        first = self.slot_t.reshape(-1).long()
        steps = torch.arange(sq, device=k.device)
        if self.fp8:
            k, v = fp8_kv.quantize(k, sc[0]), fp8_kv.quantize(v, sc[1])
        if self.paged:
            # the first slot is physical; the rows after it may cross into the
            # sequence's next page: their logical positions through the table
            pos = (self.ip.device_kv_len.reshape(-1).long().expand(b) - sq)[None, :] + steps[:, None]
            pi = (pos // KV_PAGE).clamp(0, self.table.shape[1] - 1)
            page = self.table.long().gather(1, pi.t()).t()
            idx = page * KV_PAGE + pos % KV_PAGE
            idx = torch.cat([first[None, :], idx[1:]], 0).reshape(-1)
            kmem.index_copy_(0, idx, k.reshape(sq * b, 1, *k.shape[2:]))
            vmem.index_copy_(0, idx, v.reshape(sq * b, 1, *v.shape[2:]))
            return
        rows = first[None, :] + steps[:, None]  # [sq, b] (one slot for the batch broadcasts)
        cols = torch.arange(self.b0, self.b0 + b, device=k.device)[None, :]
        kmem[rows, cols] = k
        vmem[rows, cols] = v

    def decode(self, q, window):
        """Attention of one query row per sequence, ``q [b, 1, np, hd]`` -> ``[b,
        1, np, hd]``, over the cache with the new row in it: the device-slot
        steps and the eager steps of the fused decode layer.  ``window(sk)``:
        the sliding window to pass for ``sk`` keys."""
        ip, sc = self.ip, self.scales
        if self.kind == DEVICE_DECODE:
            # cache slot and key count live in device tensors, so no launch depends
            # on the step (on the CPU the static-buffer step runs eagerly)
            if self.paged:
                return flash_decode_cached(q, self.kmem.transpose(0, 1), self.vmem.transpose(0, 1),
                                           ip.device_kv_len, window=window(ip.max_sequence_len),
                                           kv_scale=sc, page_table=self.table,
                                           capacity=ip.max_sequence_len)
            return flash_decode_cached(q, self.kc.transpose(0, 1), self.vc.transpose(0, 1),
                                       ip.device_kv_len, window=window(self.kc.shape[0]),
                                       kv_scale=sc)
        n = self.s0 + 1
        keys, vals = self.kc[:n].transpose(0, 1), self.vc[:n].transpose(0, 1)
        if self.fp8:
            # every step reads the bytes in the FP8 decode kernel (the MHA route
            # to the FlashAttention forward takes 16-bit K / V)
            return flash_decode_cached(q, keys, vals, None, window=window(n), kv_scale=sc)
        return flash_attn_func(q, keys, vals, causal=True, window=window(n))

    def decode_multi(self, q, window, rows_first=True):
        """Attention of the multi-row device step, ``q [b, sq, np, hd]`` (any
        strides with ``hd`` contiguous: the fused layer passes its ``[sq * b,
        np * hd]`` projection as a view) over the cache with the ``sq`` new
        rows of every sequence in it.  ``rows_first``: the result ``[b, sq, np,
        hd]`` lies in memory in ``[sq, b]`` row order, as the fused layer's next
        product reads it."""
        ip = self.ip
        if self.paged:
            return flash_decode_cached(q, self.kmem.transpose(0, 1), self.vmem.transpose(0, 1),
                                       ip.device_kv_len, window=window(ip.max_sequence_len),
                                       kv_scale=self.scales, page_table=self.table,
                                       capacity=ip.max_sequence_len, rows_first=rows_first)
        return flash_decode_cached(q, self.kc.transpose(0, 1), self.vc.transpose(0, 1),
                                   ip.device_kv_len, window=window(self.kc.shape[0]),
                                   kv_scale=self.scales, rows_first=rows_first)

    def attend(self, q, k, v, window, flash, core):
        """The unfused layer's attention after ``write(k, v)``: ``q [sq, b, np,
        hd]`` -> ``[sq, b, np * hd]``.  ``flash``: the layer's ``use_flash_attn``;
        ``core(q, keys, vals)``: its fallback over ``[sk, b, nkv, hd]`` keys."""
        sc, s0 = self.scales, self.s0
        sq, b = q.shape[:2]
        n = s0 + sq
        qt = q.transpose(0, 1)
        fp8_native = self.fp8 and self.native and flash
        if self.kind == DEVICE_MULTI:
            o = self.decode_multi(qt, window, rows_first=False)
        elif self.kind == DEVICE_DECODE or (sq == 1 and fp8_native):
            o = self.decode(qt, window)
        elif self.paged and s0 > 0 and flash:  # continued: the first s0 keys are in the pages only
            o = flash_attn_paged(qt, self.kmem.transpose(0, 1), self.vmem.transpose(0, 1),
                                 self.table, n, window=window(n), kv_scale=sc)
        elif s0 > 0 and fp8_native and not self.paged:
            # the FP8 forms of the forward kernel read the stored bytes (the new
            # rows' own included) in place
            o = flash_attn_fp8_kv(qt, self.kc[:n].transpose(0, 1), self.vc[:n].transpose(0, 1),
                                  sc, window=window(n))
        else:
            if self.paged and s0 > 0:
                keys, vals = (gather_rows(m, self.table[0], n) for m in (self.kmem, self.vmem))
            elif s0 == 0 and (self.paged or self.fp8):
                keys, vals = k, v
            else:
                keys, vals = self.kc[:n], self.vc[:n]
            if keys.dtype == torch.uint8:
                keys = fp8_kv.dequantize(keys, sc[0], q.dtype)
                vals = fp8_kv.dequantize(vals, sc[1], q.dtype)
            if not flash:
                return core(q, keys, vals)
            o = flash_attn_func(qt, keys.transpose(0, 1), vals.transpose(0, 1), causal=True,
                                window=window(n))
        return o.transpose(0, 1).reshape(sq, b, -1)
