"""Speculative decode on one captured hipGraph, greedy or sampled: n-gram
(prompt-lookup) drafts, verified by the multi-row device step.

A decode step at small batch is a weight stream that costs the same for one
row per sequence or for eight.  ``SpeculativeGreedyDecoder`` feeds ``S`` rows per
sequence: the last committed token and ``D = S - 1`` drafted continuations.  The
forward is the "device-slot multi-row step" cell of ``inference/kv_cache.py``
(the unfused layer, RoPE and the cache write in one launch,
``csrc/kv_write_multi.hip``, then ``flash_decode_cached`` with ``sq = S``:
``csrc/flash_decode_mq.hip``), and the tail (``spec_tail_k``,
``csrc/decode_tail.hip``) takes the argmax of all ``S`` logits rows, accepts the
drafts that the model itself would have produced, commits them and the one
token after them, and drafts the next step: the longest suffix of the context
(up to ``ngram`` tokens) is looked up earlier in the context and what followed
it there is proposed.  The committed tokens are exactly the greedy sequence:
row ``t`` sees the same keys the one-row decode would see at its position, and
a row behind a rejected draft is discarded; its cache rows are overwritten by
the next step, whose ``S`` rows start at the new position, and the key count
never covers a row before it is rewritten.

No draft model, no second graph, no host work per step: every quantity the
step depends on is a device tensor (``spec_tail_k``'s comment lists them).

``fused=True`` (opt-in) runs the verify step through the fused decode layer
instead (``ip.device_multi = "fused"``: the ``batch * rows`` rows take the
weight-streaming GEMMs of ``csrc/skinny_gemm.hip`` / ``csrc/wide_gemm.hip``,
whose QKV epilogue rotates and stores every row by the multi-row cell's rules,
and the e4m3 / MXFP4 weight packs of ``--inference_fp8_weights`` /
``--inference_mxfp4_weights``).  It needs ``batch * rows`` <= 32 (64 where
the wide kernel is on); steps above that, and layers the fused decode layer
does not take, run the unfused layer as without it.

Not built: a draft model, tree drafts, the continuous batcher and paged
caches, the text-generation API / server flag, sampling settings per row, the
fused verify step as the default.

``SpeculativeSamplingDecoder`` is the same loop for sampled requests: its tail
(``spec_sample_tail_k``) draws every row with ``sample_tail_k``'s draw and
accepts a draft iff it is the token drawn before it (class docstring).
"""
import torch

from ..ops.sampling import _next_seed_offset, sample_ref
from ..parallel import state
from . import kv_cache
from .hip_graph import _check_unpaged, broadcast_seed_offset

MAX_NGRAM = 4


def spec_tail_ref(logits, tokens, pos, slot, kv_len, history, hist_len, limit, active, accepted,
                  tick, ctl, am=None):
    """``spec_tail_k`` in plain torch, in place on the state tensors: ``logits
    [b * S, V]``, ``tokens / pos [b, S]``, the others per sequence; ``ctl =
    [stop_id, ngram, sequences still active (written)]``.  ``am [b, S]``: the
    token of every row where it is not the argmax (``spec_sample_tail_ref``)."""
    b, S = tokens.shape
    am = (logits.argmax(-1).view(b, S) if am is None else am).tolist()
    stop_id, G = int(ctl[0]), min(max(int(ctl[1]), 0), MAX_NGRAM)
    still = 0
    for r in range(b):
        if not int(active[r]):
            continue
        a, tok, hl, lim = am[r], tokens[r].tolist(), int(hist_len[r]), int(limit[r])
        n = 0
        while n < S - 1 and tok[n + 1] == a[n]:
            n += 1
        commit = a[:min(n + 1, max(lim - hl, 1))]
        stopped = stop_id >= 0 and stop_id in commit
        if stopped:
            commit = commit[:commit.index(stop_id) + 1]
        c = len(commit)
        history[r, hl:hl + c] = torch.tensor(commit, dtype=history.dtype)
        hist_len[r] = nl = hl + c
        accepted[r] += c - 1
        if stopped or nl >= lim:
            active[r] = 0
            continue
        still += 1
        h = history[r, :nl].tolist()
        end = -1  # one past the winning match
        for g in range(G, 0, -1):
            starts = [j for j in range(nl - g) if h[j:j + g] == h[nl - g:]]
            if starts:
                end = starts[-1] + g
                break
        draft = [h[end + k] if end >= 0 and end + k < nl else h[-1] for k in range(S - 1)]
        tokens[r] = torch.tensor([h[-1]] + draft, dtype=tokens.dtype)
        pos[r] = torch.arange(nl - 1, nl - 1 + S, dtype=pos.dtype)
        slot[r] = nl - 1
        kv_len[r] = nl - 1 + S
    tick += 1
    ctl[2] = still


def spec_sample_tail_ref(logits, tokens, pos, slot, kv_len, history, hist_len, limit, active,
                         accepted, tick, ctl, fctl, gen0):
    """``spec_sample_tail_k`` in fp64 / torch (CPU), in place as ``spec_tail_ref``:
    row ``t`` of sequence ``r`` draws with ``sample_ref`` at the noise index of
    the token it would commit, Philox row ``r`` and step ``hist_len[r] + t -
    gen0[r]``, and the greedy tail's bookkeeping runs on the drawn tokens.
    ``ctl = [stop_id, ngram, still active (written), seed, offset0, top_k,
    vocab_limit]``, ``fctl = [temperature, top_p]``."""
    b, S = tokens.shape
    seed, offset0, top_k, vocab = (int(x) for x in ctl[3:7])
    x, drawn = logits.detach().float().cpu(), torch.zeros(b, S, dtype=torch.long)
    for r in range(b):
        for t in range(S if int(active[r]) else 0):
            # sample_ref numbers its rows from 0: row r of r + 1 copies is Philox row r
            drawn[r, t] = sample_ref(x[r * S + t].expand(r + 1, -1), seed, offset0,
                                     int(hist_len[r]) + t - int(gen0[r]), top_k, float(fctl[1]),
                                     float(fctl[0]), vocab or None)[r]
    spec_tail_ref(logits, tokens, pos, slot, kv_len, history, hist_len, limit, active, accepted,
                  tick, ctl, am=drawn)


class SpeculativeGreedyDecoder:
    """Greedy decode of ``batch`` sequences, up to ``rows`` tokens per replay.

    Usage::

        dec = SpeculativeGreedyDecoder(model, ip, batch, max_new_tokens, rows=8, ngram=3)
        dec.start(prompt_tokens, next_tokens)   # the prefilled prompt, the first new token
        while dec.active_rows():                # (reads the device)
            dec.step()                          # one replay: 1..rows tokens per active row
        tokens, lengths = dec.generated()       # [batch, max_new_tokens], [batch]
        dec.mean_accepted()                     # accepted drafts per sequence and step

    The prompt ``[batch, L]`` was prefilled eagerly into ``ip`` (with
    ``ip.device_multi`` unset: ``start`` sets it, and a later prefill into the
    same ``ip`` must clear it again); ``next_tokens`` is the greedy choice from
    its logits.  Every row generates ``max_new_tokens`` tokens after
    ``next_tokens`` unless it commits ``stop_id`` first.  ``graph=False`` runs
    the same step eagerly (on the CPU with ``spec_tail_ref``).  ``fused=True``:
    the verify step through the fused decode layer (module docstring; off by
    default).  Measured (``profiles/r23a_spec_fused.txt``, Llama-2-7B shapes) a
    replay takes 2.98 against 3.50 ms at 4 rows and 4.96 against 5.05 ms at 32
    in bf16, 1.83 against 3.49 and 3.85 against 5.05 ms under MXFP4; it loses
    in one cell, ``batch * rows`` = 64 under MXFP4 (6.77 against 5.59 ms: the
    wide kernel), which a default should exclude."""

    def __init__(self, model, inference_params, batch, max_new_tokens, rows=4, ngram=3, graph=True,
                 fused=False):
        if state.model_parallel_is_initialized() and \
                state.get_pipeline_model_parallel_world_size() > 1:
            raise NotImplementedError("the speculative decode loop needs the whole model (PP = 1)")
        _check_unpaged(inference_params, type(self).__name__)
        if kv_cache.FP8_KV and kv_cache.FP8_KV_CALIBRATE:
            raise NotImplementedError("a multi-row device step does not calibrate the FP8 KV "
                                      "scales (--inference_fp8_kv_calibrate)")
        if not 2 <= rows <= 16:
            raise ValueError("rows (the committed token and its drafts) must be in 2..16")
        if not 0 <= ngram <= MAX_NGRAM:
            raise ValueError(f"ngram must be in 0..{MAX_NGRAM}")
        if graph and not torch.cuda.is_available():
            raise RuntimeError("hipGraph decode needs a GPU")
        self.model, self.ip, self.batch = model, inference_params, batch
        self.max_new, self.rows, self.ngram, self.graph_mode = max_new_tokens, rows, ngram, graph
        self.fused = fused
        self.dev = torch.device("cuda", torch.cuda.current_device()) if graph else \
            next(model.parameters()).device
        self.graph = None
        self.logits = None
        self.history = None

    def _allocate(self, L):
        b, S, dev = self.batch, self.rows, self.dev

        def z(shape, dtype=torch.long):
            return torch.zeros(shape, dtype=dtype, device=dev)
        self.prompt_len = L
        self.tokens, self.pos = z((b, S)), z((b, S))
        self.slot, self.kv_len = z(b), z(b, torch.int32)
        self.history = z((b, L + 1 + self.max_new))
        self.hist_len, self.limit, self.accepted = z(b), z(b), z(b)
        self.active = z(b, torch.int32)
        self.tick, self.ctl = z(1), z(3)
        self.am, self.counters = z((b, S), torch.int32), z(b + 1, torch.int32)

    def _state(self):
        return (self.tokens, self.pos, self.slot, self.kv_len, self.history, self.hist_len,
                self.limit, self.active, self.accepted, self.tick, self.ctl)

    def _fused_tail(self, flat):
        from ..ops._ext import use_native
        return (use_native(flat) and flat.stride(1) == 1
                and flat.dtype in (torch.bfloat16, torch.float16, torch.float32)
                and flat.data_ptr() % 16 == 0 and (flat.stride(0) * flat.element_size()) % 16 == 0)

    def _forward(self):
        return self.model(self.tokens, self.pos, None, inference_params=self.ip)

    def _body(self):
        logits = self._forward()
        flat = logits.reshape(self.batch * self.rows, -1)
        if self._fused_tail(flat):
            self._tail(flat, True)
        elif self.graph_mode:
            raise RuntimeError("the speculative tail needs bf16 / fp16 / fp32 logits on the GPU "
                               "with 16-byte aligned rows")
        else:
            self._tail(flat, False)
        return logits

    def _tail(self, flat, native):
        if native:
            from ..ops._ext import ext
            ext().spec_tail(flat, *self._state(), self.am, self.counters)
        else:
            spec_tail_ref(flat, *self._state())

    def start(self, prompt_tokens, next_tokens, stop_id=-1):
        """Seed the context with the prefilled ``prompt_tokens [batch, L]`` and
        the first new token of every row (``next_tokens``, ``batch`` elements),
        draft nothing yet (every draft of the first step is ``next_tokens``) and
        capture the graph on the first call."""
        b, S, ip = self.batch, self.rows, self.ip
        prompt = torch.as_tensor(prompt_tokens).view(b, -1)
        L = prompt.shape[1]
        if L + self.max_new + S - 1 > ip.max_sequence_len:
            raise ValueError("KV cache too short for max_new_tokens and the drafts' rows")
        if self.history is None:
            self._allocate(L)
        elif L != self.prompt_len:
            raise ValueError(f"the decoder was started with prompts of {self.prompt_len} tokens")
        with torch.no_grad():
            first = torch.as_tensor(next_tokens).to(self.dev).view(b, 1)
            self.history.zero_()
            self.history[:, :L] = prompt.to(self.dev)
            self.history[:, L:L + 1] = first
            self.tokens.copy_(first.expand(b, S))
            self.pos.copy_(torch.arange(L, L + S, device=self.dev).expand(b, S))
            self.slot.fill_(L)
            self.kv_len.fill_(L + S)
            self.hist_len.fill_(L + 1)
            self.limit.fill_(L + 1 + self.max_new)
            self.accepted.zero_()
            self.tick.zero_()
            self.active.fill_(1)
            self.ctl[:3].copy_(torch.tensor([stop_id, self.ngram, b]))
            ip.device_offset, ip.device_kv_len = self.slot, self.kv_len
            ip.device_multi = "fused" if self.fused else True
            if self.graph_mode and self.graph is None:
                self._capture()

    def _capture(self):
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            # warm-up at the current state: writes the S cache slots per row
            # that the first replay writes again (idempotent), initialises lazy state
            self._forward()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._body()

    def step(self):
        """One replay: every active row commits 1..rows tokens."""
        with torch.no_grad():
            if self.graph_mode:
                self.graph.replay()
            else:
                self.logits = self._body()
        return self.tokens

    def active_rows(self):
        """The rows still generating (reads the device)."""
        return self.active.nonzero().flatten().tolist()

    def generated(self):
        """(tokens ``[batch, max_new_tokens]``, lengths ``[batch]``): what each
        row committed after ``next_tokens`` (device tensors; zeros past a
        row's length)."""
        L = self.prompt_len
        return self.history[:, L + 1:], self.hist_len - (L + 1)

    def mean_accepted(self):
        """Accepted drafts per sequence and step so far (reads the device)."""
        return float(self.accepted.sum()) / max(int(self.tick) * self.batch, 1)


class SpeculativeSamplingDecoder(SpeculativeGreedyDecoder):
    """``SpeculativeGreedyDecoder`` for sampled requests: temperature and top-k or
    top-p, the draw inside the captured graph (``spec_sample_tail_k``).

    Usage::

        dec = SpeculativeSamplingDecoder(model, ip, batch, max_new_tokens, rows=8, ngram=3,
                                         vocab_size=None)
        dec.start(prompt_tokens, next_tokens, top_k=0, top_p=0.9, temperature=0.8, stop_id=-1)
        while dec.active_rows():
            dec.step()
        tokens, lengths = dec.generated()

    Every row of a step draws the token that follows it, with the noise of that
    token's place in its sequence: Philox row = the sequence, offset =
    ``offset0 + n`` for generated token ``n``, the pair ``GraphedSamplingDecoder``
    uses.  A draft is accepted iff it is the token drawn before it, which for a
    deterministic draft is exact speculative sampling, so the committed tokens
    are distributed as the one-token-at-a-time sampler's, and for the same logits
    they ARE its tokens.  The settings live in device tensors (``ctl``,
    ``fctl``): a later ``start()`` with others replays the same graph.
    ``start()`` takes ``(seed, offset0)`` from the CUDA generator (TP rank 0's)
    and advances it past the generation, or from ``seed_offset``.  ``graph=False``
    runs eagerly (on the CPU with ``spec_sample_tail_ref``); ``fused`` as in
    ``SpeculativeGreedyDecoder``."""

    def __init__(self, model, inference_params, batch, max_new_tokens, rows=4, ngram=3, graph=True,
                 vocab_size=None, fused=False):
        super().__init__(model, inference_params, batch, max_new_tokens, rows, ngram, graph, fused)
        self.vocab_size = vocab_size
        self.seed = self.offset0 = None

    def _allocate(self, L):
        super()._allocate(L)
        self.ctl = torch.zeros(7, dtype=torch.long, device=self.dev)
        self.fctl = torch.ones(2, dtype=torch.float32, device=self.dev)
        self.gen0 = torch.full((self.batch,), L + 1, dtype=torch.long, device=self.dev)

    def _tail(self, flat, native):
        if native:
            from ..ops._ext import ext
            ext().spec_sample_tail(flat, *self._state(), self.fctl, self.gen0, self.am,
                                   self.counters)
        else:
            spec_sample_tail_ref(flat, *self._state(), self.fctl, self.gen0)

    def start(self, prompt_tokens, next_tokens, top_k=0, top_p=0.0, temperature=1.0, stop_id=-1,
              seed_offset=None):
        """As ``SpeculativeGreedyDecoder.start`` plus the sampling settings of
        this generation (one setting per batch, as the text-generation API has)."""
        if top_k < 0 or (top_k > 0 and top_p != 0.0):
            raise AssertionError("cannot set both top-k and top-p samplings")
        if not 0.0 <= top_p <= 1.0:
            raise AssertionError("top-p should be in (0, 1]")
        if not temperature > 0.0:
            raise AssertionError("temperature should be positive")
        if seed_offset is not None:
            seed, offset0 = seed_offset
        elif self.dev.type == "cuda":
            gen = torch.cuda.default_generators[self.dev.index]
            seed, offset0 = gen.initial_seed(), gen.get_offset()
            # one Philox offset per generated token; the generator moves in multiples of 4
            gen.set_offset(offset0 + (self.max_new + 4) // 4 * 4)
        else:
            seed, offset0 = _next_seed_offset(self.dev)
        if self.dev.type == "cuda":
            seed, offset0 = broadcast_seed_offset(seed, offset0, self.dev)
        self.seed, self.offset0 = seed, offset0
        super().start(prompt_tokens, next_tokens, stop_id=stop_id)
        self.ctl[3:].copy_(torch.tensor([seed, offset0, top_k, self.vocab_size or 0]))
        self.fctl.copy_(torch.tensor([temperature, top_p], dtype=torch.float32))
