"""Incremental (KV-cached) forward for generation (reference
``megatron/text_generation/forward_step.py``).

``InferenceParams`` owns the per-layer KV caches (allocated lazily by each
attention layer as ``[max_seq, max_batch, nkv_per_tp, hd]`` — GQA keys stay at
``nkv`` heads, already rotated) and the running sequence / batch offsets.
``ForwardStep`` runs one model call per generation step across pipeline
stages; when ``batch x new_tokens`` exceeds
``--inference_batch_times_seqlen_threshold`` the batch is split into
micro-batches that stream through the pipeline (prefill of long prompts).
"""
from collections.abc import Iterable

import torch

from .. import global_vars
from ..parallel import state
from .communication import device, recv_from_prev_pipeline_rank_, send_to_next_pipeline_rank


class InferenceParams:

    def __init__(self, max_batch_size, max_sequence_len, kv_pages=None, table_device=None):
        """``kv_pages = N``: a paged cache (``inference/paged.py``), per layer one
        pool of ``N`` pages of ``KV_PAGE`` keys for K and one for V, and
        ``page_table`` (int32 ``[max_batch_size, pages_per_row]``, zero-filled:
        every entry at the null page 0) on ``table_device`` (default: the
        inference device).  None: a full-capacity cache column per row."""
        self.kv_pages = self.page_table = None
        if kv_pages is not None:
            from .paged import pages_for
            if kv_pages < 2:
                raise ValueError("kv_pages must be >= 2: page 0 is the null page")
            self.kv_pages = int(kv_pages)
            self.pages_per_row = pages_for(max_sequence_len)
            self.page_table = torch.zeros(max_batch_size, self.pages_per_row, dtype=torch.int32,
                                          device=table_device if table_device is not None
                                          else device())
        self.max_sequence_len = max_sequence_len
        self.max_batch_size = max_batch_size
        self.sequence_len_offset = 0
        self.batch_size_offset = 0
        # paged cache only (host flag): a b = 1 prefill at sequence_len_offset
        # > 0 continues row batch_size_offset over the keys its table already
        # names (a shared prefix, an earlier chunk); clear, it raises
        self.continue_prefill = False
        self.key_value_memory_dict = {}
        # hipGraph decode (inference/hip_graph.py): the cache slot of the new
        # token (int64 [1]) and the valid key count (int32 [1]) on the device;
        # [batch] elements each: one per row (inference/continuous.py)
        self.device_offset = None
        self.device_kv_len = None
        # FP8 KV cache (--inference_fp8_kv_cache): per layer an fp32 device
        # tensor [2, nkv_per_tp] (row 0: K scales, row 1: V scales), 1.0 until
        # set; the kernels read it from device memory on every launch
        self.kv_scale_dict = {}

    def set_kv_scales(self, layer, k_scale=None, v_scale=None):
        """Set the per-head e4m3 scales of ``layer``'s cache in place (values
        broadcastable to ``[nkv_per_tp]``; None keeps a row).  What the cache
        already holds was quantised with the old scales, so set them before the
        prefill."""
        sc = self.kv_scale_dict[layer]
        for row, val in ((0, k_scale), (1, v_scale)):
            if val is not None:
                sc[row].copy_(torch.as_tensor(val, dtype=torch.float32).to(sc.device).expand_as(sc[row]))

    def swap_key_value_dict(self, batch_idx):
        """Reorder the cached batch rows (beam search keeps the best beams)."""
        if self.page_table is not None:
            raise NotImplementedError("swap_key_value_dict (beam search) reorders cache columns, "
                                      "which a paged KV cache does not have; use kv_pages=None")
        if not self.key_value_memory_dict:
            raise ValueError("should not swap when dict in empty")
        for layer, (k, v) in self.key_value_memory_dict.items():
            if len(batch_idx) != k.shape[1]:
                raise AssertionError("batch size mismatch while reordering the KV cache")
            # in place: a captured hipGraph (inference/hip_graph.py) holds
            # these cache addresses
            k.copy_(k[:, batch_idx])
            v.copy_(v[:, batch_idx])


class ForwardStep:

    def __init__(self, model, max_batch_size, max_sequence_len):
        if isinstance(model, Iterable):
            raise AssertionError("interleaving schedule is not supported for inference")
        model.eval()
        self.model = model
        self.inference_params = InferenceParams(max_batch_size, max_sequence_len)
        args = global_vars.get_args()
        self.pipelined = args.pipeline_model_parallel_size > 1
        self.threshold = args.inference_batch_times_seqlen_threshold
        self.graphed = None
        if getattr(args, "inference_hip_graph", False):
            # a hipGraph per pipeline stage on the GPU; on the CPU the same
            # static-buffer step runs eagerly
            from .hip_graph import GraphedDecodeForward
            self.graphed = GraphedDecodeForward(model, self.inference_params, max_batch_size)

    def __call__(self, tokens, position_ids, attention_mask):
        if self.graphed is not None and tokens.size(1) == 1 and \
                tokens.size(0) == self.inference_params.max_batch_size:
            out = self.graphed(tokens, position_ids)
            self.inference_params.sequence_len_offset += 1
            return out
        if self.pipelined and tokens.size(0) * tokens.size(1) >= self.threshold:
            mbs = max(1, self.threshold // tokens.size(1))
            return _with_pipelining_forward_step(self.model, tokens, position_ids,
                                                 attention_mask, self.inference_params, mbs)
        return _no_pipelining_forward_step(self.model, tokens, position_ids, attention_mask,
                                           self.inference_params)


def _recv_dtype(args):
    return torch.float if args.fp32_residual_connection else args.params_dtype


def _allocate_recv_buffer(batch_size, sequence_length):
    if state.is_pipeline_first_stage():
        return None
    args = global_vars.get_args()
    return torch.empty((sequence_length, batch_size, args.hidden_size), dtype=_recv_dtype(args),
                       device=device())


def _forward_step_helper(model, tokens, position_ids, attention_mask, inference_params,
                         recv_buffer=None):
    if recv_buffer is None:
        recv_buffer = _allocate_recv_buffer(tokens.size(0), tokens.size(1))
    recv_from_prev_pipeline_rank_(recv_buffer)
    model.set_input_tensor(recv_buffer)
    out = model(tokens, position_ids, attention_mask, inference_params=inference_params)
    send_to_next_pipeline_rank(out)
    return out


def _no_pipelining_forward_step(model, tokens, position_ids, attention_mask, inference_params,
                                recv_buffer=None):
    out = _forward_step_helper(model, tokens, position_ids, attention_mask, inference_params,
                               recv_buffer)
    inference_params.sequence_len_offset += tokens.size(1)
    return out if state.is_pipeline_last_stage() else None


def _with_pipelining_forward_step(model, tokens, position_ids, attention_mask, inference_params,
                                  micro_batch_size):
    b, s = tokens.shape
    logits = None
    if state.is_pipeline_last_stage():
        args = global_vars.get_args()
        logits = torch.empty((b, s, args.padded_vocab_size), dtype=torch.float32,
                             device=device())
    recv = _allocate_recv_buffer(micro_batch_size, s)
    for start in range(0, b, micro_batch_size):
        end = min(start + micro_batch_size, b)
        out = _forward_step_helper(model, tokens[start:end], position_ids[start:end],
                                   attention_mask, inference_params,
                                   recv if end - start == micro_batch_size else None)
        inference_params.batch_size_offset += end - start
        if logits is not None:
            logits[start:end] = out
    inference_params.sequence_len_offset += s
    inference_params.batch_size_offset = 0
    return logits
