"""Ragged decode and continuous (in-flight) batching on one captured hipGraph.

The decoders of ``hip_graph.py`` move a batch in lockstep: one cache slot, one
key count and one step index for all rows.  Here every row is its own
sequence.  The per-row state lives in device tensors of ``batch`` elements:

  ``slot`` int64 (= ``InferenceParams.device_offset``), ``kv_len`` int32
  (= ``device_kv_len``), ``pos`` int64, ``hist_idx`` int64, ``limit`` int64,
  ``active`` int32; shared: ``tick`` int64 ``[1]``, the replay count.

The kernels pick the per-row forms from the element count: the QKV epilogue
writes row ``m``'s K / V at ``slot[m]`` (``csrc/skinny_gemm.hip``), the decode
attention bounds sequence ``b`` by ``kv_len[b]`` (``csrc/flash_decode.hip``,
grid still sized for the capacity), and the ragged tail (``ragged_tail_k``,
``csrc/decode_tail.hip``) selects a token for every active row, advances that
row alone and parks it when it emits ``stop_id`` or reaches its limit.  A
parked row stays in the batch: it keeps rewriting a cache slot it owns and
its outputs are ignored; a row that was never primed sits at ``kv_len = 0``
(the attention gives exact zeros there).  ``prime()`` rewrites one row's state
with small copies between replays, so a new request enters a finished row
without recapture: ``ContinuousBatcher`` does that, prefilling the prompt
eagerly into the row's cache column (``batch_size_offset = row``).

Every kernel of the step computes a row from that row's inputs alone, so a
row's tokens and logits are bitwise those of a lockstep decode of the same
batch size and capacity with the scalars set to that row's values.

Without a GPU (``capture=False``) the same static-buffer step runs eagerly
with a torch transcription of the tail (``ragged_tail_reference``); the CPU
tests drive the decoders and the scheduler through it.  PP must be 1; under
TP the sampling decoder broadcasts TP rank 0's Philox ``(seed, offset)``.

Paged cache (``InferenceParams(..., kv_pages=N)``, ``inference/paged.py``): the
rows share one pool of pages per layer and ``ip.page_table`` names each row's
pages.  ``slot`` then holds pool rows: ``prime(..., pages=)`` writes the row's
table and its first slot, the tail computes the next slot from the table, and
``release(row)`` sends a finished row to the null page (``slot = 0``, ``kv_len =
0``, a zero table row) so that the K / V write it still performs on every replay
cannot land in a page that has gone to another row.  ``ContinuousBatcher``
reserves all of a request's pages at admission from a ``PagePool`` and makes the
request wait, in order, while the pool is short.

Chunked prefill (``ContinuousBatcher(prefill_chunk=c)``): a prompt is prefilled
in pieces that end at the multiples of ``c``, back to back, each a ``b = 1``
call at ``sequence_len_offset`` = the piece's first position; on a paged cache
``ip.continue_prefill`` is set around the calls and a piece attends over the
earlier ones through the page table.  Decode replays do not run between the
pieces of one prompt.

Prefix sharing (``prefix_cache=True``, paged only; ``PrefixCache`` in
``inference/paged.py``): at admission the prompt's leading full pages are looked
up in the cache; the row's table starts with the pages found, only the others
are allocated, and the prefill starts behind them.  After the prefill the row's
own full prompt pages are registered for later requests.  Shared pages are
never written: only full prompt pages are shared, the prefill writes at
positions past the shared pages and the decoder at positions ``>= len(prompt)``.
A finished row is released first (its later K / V writes go to the null page);
then its private pages return to the pool and its cached pages lose a reader,
staying cached until an admission that finds the pool short evicts them.

The reference has no in-flight batching (``megatron/text_generation/
generation.py`` runs a fixed batch to its longest member); this is an
MI355X-side addition.
"""
from collections import deque

import torch

from ..parallel import state
from .hip_graph import broadcast_seed_offset
from .paged import KV_PAGE, PagePool, PrefixCache, pages_for, physical_slots

_TOO_SHORT = "KV cache too short for max_new_tokens"


def ragged_tail_reference(tok, tokens, history, hist_idx, pos, slot, kv_len, active, limit, tick,
                          ctl, page_table=None, n_pages=0):
    """Thread 0's bookkeeping of ``ragged_tail_k`` in torch, for the selected
    tokens ``tok [b]`` (any value in parked rows): in place on the state
    tensors; ``ctl[4]`` is the stop id, ``ctl[5]`` receives the number of rows
    still active.  ``page_table`` (int32 ``[b, pages_per_row]``, a pool of
    ``n_pages`` pages): an advancing row's slot becomes the pool row of its new
    position, the table entry clamped to the pool as the kernel clamps it."""
    tok = tok.view(-1).to(tokens.dtype)
    act = active != 0
    rows = act.nonzero().flatten()
    stop_id = ctl[4]
    tokens.copy_(torch.where(act, tok, tokens))
    history[rows, hist_idx[rows]] = tok[rows]
    hist_idx.add_(act.to(hist_idx.dtype))
    done = ((stop_id >= 0) & (tok == stop_id)) | (hist_idx >= limit)
    go = act & ~done
    active.copy_(go.to(active.dtype))
    pos.add_(go.to(pos.dtype))
    if page_table is None:
        slot.add_(go.to(slot.dtype))
    else:
        pi = (pos // KV_PAGE).clamp(0, page_table.shape[1] - 1)
        page = page_table.gather(1, pi.view(-1, 1)).view(-1).clamp(0, n_pages - 1)
        slot.copy_(torch.where(go, page.to(slot.dtype) * KV_PAGE + pos % KV_PAGE, slot))
    kv_len.add_(go.to(kv_len.dtype))
    tick.add_(1)
    ctl[5] = go.sum()


class RaggedGreedyDecoder:
    """Greedy decode of ``batch`` independent sequences, one captured graph.

    Usage::

        dec = RaggedGreedyDecoder(model, ip, batch, max_new_tokens)
        dec.prime(row, first_token, position, max_new)   # per row, after its prefill
        while dec.active_rows():                          # (reads the device)
            dec.step()                                    # one replay: a token per active row
        dec.history[row, :dec.hist_idx[row]]              # the row's tokens

    ``max_new_tokens`` sizes the history; ``prime`` takes each row's own
    limit.  ``set_stop_id`` sets the token (one per decoder) that parks a row
    that emits it."""

    sample = False

    def __init__(self, model, inference_params, batch, max_new_tokens, capture=None):
        if state.model_parallel_is_initialized() and \
                state.get_pipeline_model_parallel_world_size() > 1:
            raise NotImplementedError("the ragged decode loop needs the whole model (PP = 1)")
        from ..models import transformer
        if transformer._FP8_KV and transformer._FP8_KV_CALIBRATE:
            raise NotImplementedError(
                "ragged decode refills rows one at a time: prompt calibration of the FP8 KV "
                "scales (--inference_fp8_kv_calibrate) would rescale the other rows' cached "
                "bytes; set the scales with InferenceParams.set_kv_scales")
        self.model = model
        self.ip = inference_params
        self.batch = batch
        self.max_new = max_new_tokens
        self.capture = torch.cuda.is_available() if capture is None else capture
        dev = torch.device("cuda", torch.cuda.current_device()) if self.capture else \
            torch.device("cpu")

        def z(n, dtype=torch.long):
            return torch.zeros(n, dtype=dtype, device=dev)
        self.tokens, self.pos = z((batch, 1)), z((batch, 1))
        self.history = z((batch, max_new_tokens))
        self.hist_idx, self.limit, self.tick = z(batch), z(batch), z(1)
        self.slot, self.kv_len = z(batch), z(batch, torch.int32)
        self.active = z(batch, torch.int32)
        self.tail_counter = z(1, torch.int32)
        # paged cache: the table lives next to the state it indexes
        self.paged = getattr(inference_params, "page_table", None) is not None
        if self.paged:
            if batch > self.ip.page_table.shape[0]:
                raise ValueError("batch exceeds the rows of the page table")
            self.ip.page_table = self.ip.page_table.to(dev)
        self._row_pages = {}  # row -> the pages write_table gave it (host copy)
        # [seed, offset0, top_k, vocab_limit, stop_id, rows still active]
        self.ctl = z(6)
        self.stop_id = -1
        self.ctl[4] = -1
        self.fctl = torch.ones(2, dtype=torch.float32, device=dev)
        self._attach()
        self.graph = None
        self.logits = None
        self.captures = 0

    def _attach(self):
        self.ip.device_offset, self.ip.device_kv_len = self.slot, self.kv_len

    # -- the step ---------------------------------------------------------
    def _forward(self):
        return self.model(self.tokens, self.pos, None, inference_params=self.ip)

    def _state(self):
        return (self.tokens.view(-1), self.history, self.hist_idx, self.pos.view(-1), self.slot,
                self.kv_len, self.active, self.limit, self.tick)

    def _body(self):
        logits = self._forward()
        last = logits[:, -1]
        if self.capture:
            from ..ops._ext import ext, use_native
            if not (use_native(last) and last.stride(1) == 1 and last.data_ptr() % 16 == 0
                    and (last.stride(0) * last.element_size()) % 16 == 0):
                raise RuntimeError("the ragged tail needs bf16 / fp16 / fp32 logits on the GPU "
                                   "with 16-byte aligned rows")
            ext().ragged_tail(last, *self._state(), self.tail_counter, self.ctl, self.fctl,
                              self.sample, *self._table())
        else:
            ragged_tail_reference(self._select(last), *self._state(), self.ctl, *self._table())
        return logits

    def _select(self, last):
        return last.argmax(-1)

    def _table(self):
        """(page table of the batch's rows, pages of the pool), or () unpaged."""
        return (self.ip.page_table[:self.batch], self.ip.kv_pages) if self.paged else ()

    def _capture(self):
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            # warm-up at the current state: every row writes the cache slot
            # the first replay writes again (idempotent), initialises lazy state
            self._forward()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._body()
        self.captures += 1

    def step(self):
        """One replay: a token for every active row.  Returns the static
        next-token buffer ``[batch, 1]``."""
        with torch.no_grad():
            self._attach()
            self._reserve()
            if not self.capture:
                self.logits = self._body()
            else:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
        return self.tokens

    def _reserve(self):
        pass

    # -- row management ---------------------------------------------------
    def set_stop_id(self, stop_id):
        """The stop token of every row (-1: none).  The decoder is its one
        owner: ``ContinuousBatcher`` reads it from here."""
        self.stop_id = int(stop_id)
        with torch.no_grad():
            self.ctl[4] = self.stop_id

    def prime(self, row, first_token, position, max_new, pages=None):
        """Start a sequence in ``row``: ``first_token`` is fed at absolute
        ``position`` (= the number of tokens the row's cache column holds) and
        up to ``max_new`` tokens are generated.  Small copies on the current
        stream; the captured graph is untouched.  Paged cache: ``pages`` lists
        the row's pages (enough for ``position + max_new`` keys; None keeps the
        table row as it stands, e.g. as written before the prefill); the table
        row is written, unused entries 0, and the slot is the pool row of
        ``position``."""
        if not 0 <= row < self.batch:
            raise ValueError(f"row {row} outside the batch of {self.batch}")
        if max_new < 1 or max_new > self.max_new:
            raise ValueError(f"max_new must be in [1, {self.max_new}]")
        if position + max_new > self.ip.max_sequence_len:
            raise ValueError(_TOO_SHORT)
        if pages is not None and not self.paged:
            raise ValueError("pages given, but the inference params hold no paged cache")
        with torch.no_grad():
            slot = position
            if self.paged:
                if pages is not None:
                    self.write_table(row, pages, position + max_new)
                held = self._row_pages.get(row)  # the host's copy of a row this decoder wrote
                if held is not None and position // KV_PAGE < len(held):
                    slot = held[position // KV_PAGE] * KV_PAGE + position % KV_PAGE
                else:
                    slot = physical_slots(self.ip.page_table[row],
                                          torch.tensor(position, device=self.slot.device))
            self.tokens[row] = int(first_token)
            self.pos[row] = position
            self.slot[row] = slot
            self.kv_len[row] = position + 1
            self.hist_idx[row] = 0
            self.limit[row] = max_new
            self.active[row] = 1

    def write_table(self, row, pages, n_keys):
        """Row ``row`` of the page table = ``pages`` (which must hold ``n_keys``
        keys and exclude the null page), the rest 0."""
        table = self.ip.page_table
        pages = [int(p) for p in pages]
        if len(pages) > table.shape[1] or len(pages) < pages_for(n_keys):
            raise ValueError(f"{len(pages)} pages for {n_keys} keys (pages per row: "
                             f"{table.shape[1]})")
        if any(not 0 < p < self.ip.kv_pages for p in pages):
            raise ValueError(f"pages must lie in [1, {self.ip.kv_pages})")
        with torch.no_grad():
            table[row] = torch.tensor(pages + [0] * (table.shape[1] - len(pages)),
                                      dtype=table.dtype).to(table.device)
        self._row_pages[row] = pages

    def release(self, row):
        """Send ``row`` to the null page: inactive, no keys, slot 0 and (paged) a
        zero table row, on the current stream.  After it the row's former pages
        may go to another row: the idle row's K / V writes land in page 0."""
        with torch.no_grad():
            self.active[row] = 0
            self.kv_len[row] = 0
            self.slot[row] = 0
            if self.paged:
                self.ip.page_table[row].zero_()
                self._row_pages.pop(row, None)

    def park(self, row):
        """Take ``row`` out of the generation: it keeps its cache slot and
        writes no token."""
        with torch.no_grad():
            self.active[row] = 0

    def active_rows(self):
        """The rows still generating (the one call that reads the device)."""
        return self.active.nonzero().flatten().tolist()


class RaggedSamplingDecoder(RaggedGreedyDecoder):
    """``RaggedGreedyDecoder`` with the sampling tail: temperature and top-k
    or top-p (``ops/sampling.py``), one setting per decoder (``configure``).
    The replay with tick ``t`` draws its noise at Philox offset ``offset0 +
    t``, whatever a row's history index is: a refilled row does not replay
    its predecessor's noise.

    Offsets are reserved from the CUDA generator (TP rank 0's under tensor
    parallelism) in blocks of ``RESERVE`` replays, and the generator is
    advanced past a block at the moment the block is taken: the first one by
    the first ``configure`` / ``prime``, each further one by the ``step`` that
    would leave the current block, from wherever the generator then stands
    (``offset0`` is re-based so that ``offset0 + tick`` continues in the new
    block).  Whatever else draws from the generator between replays, the
    first-token draws of ``ContinuousBatcher`` included (``draw_seed_offset``),
    therefore never shares an offset with a replay."""

    sample = True
    RESERVE = 1024

    def __init__(self, model, inference_params, batch, max_new_tokens, vocab_size=None,
                 capture=None):
        super().__init__(model, inference_params, batch, max_new_tokens, capture)
        self.vocab_size = vocab_size
        self.seed = self.offset0 = None
        self.ticks = 0          # replays so far (= the device tick)
        self.block_end = 0      # one past the last offset of the reserved block
        self.blocks = []        # (first offset, one past the last) of every block taken
        self.first_draws = []   # offsets handed out by draw_seed_offset
        self._cpu_offset = 0    # stands in for the generator's offset without a GPU
        self.settings = dict(top_k=0, top_p=0.0, temperature=1.0)

    # -- the generator ------------------------------------------------------
    def _take(self, n):
        """``n`` offsets (rounded up to the generator's granularity of 4) from
        the generator's current position, which moves past them now: (seed,
        first offset) as every TP rank must use them."""
        dev = self.tokens.device
        n = (n + 3) // 4 * 4
        if dev.type == "cuda":
            gen = torch.cuda.default_generators[dev.index]
            seed, off = gen.initial_seed(), gen.get_offset()
            gen.set_offset(off + n)
        else:
            seed, off = torch.initial_seed() & (2 ** 63 - 1), self._cpu_offset
            self._cpu_offset += n
        return broadcast_seed_offset(seed, off, dev)

    def _new_block(self):
        self.seed, off = self._take(self.RESERVE)
        self.offset0 = off - self.ticks  # offset0 + tick continues at `off`
        self.block_end = off + (self.RESERVE + 3) // 4 * 4
        self.blocks.append((off, self.block_end))
        with torch.no_grad():
            self.ctl[:2] = torch.tensor([self.seed, self.offset0], dtype=torch.long)

    def draw_seed_offset(self):
        """(seed, offset) for one draw outside the replays (the first token of
        a request, from its prefill logits): taken from the generator, which
        stands past every reserved block, and the same on every TP rank."""
        seed, off = self._take(4)
        self.first_draws.append(off)
        return seed, off

    def configure(self, top_k=0, top_p=0.0, temperature=1.0, stop_id=-1):
        """The sampling settings and the stop token of every row from now on;
        the first call reserves the first block of Philox offsets."""
        if top_k < 0 or (top_k > 0 and top_p != 0.0):
            raise AssertionError("cannot set both top-k and top-p samplings")
        if not 0.0 <= top_p <= 1.0:
            raise AssertionError("top-p should be in (0, 1]")
        if not temperature > 0.0:
            raise AssertionError("temperature should be positive")
        if self.seed is None:
            self._new_block()
        self.settings = dict(top_k=top_k, top_p=top_p, temperature=temperature)
        with torch.no_grad():
            self.ctl[2:4] = torch.tensor([top_k, self.vocab_size or 0], dtype=torch.long)
            self.fctl.copy_(torch.tensor([temperature, top_p], dtype=torch.float32))
        self.set_stop_id(stop_id)

    def _reserve(self):
        if self.seed is None:
            self.configure()
        if self.offset0 + self.ticks >= self.block_end:
            self._new_block()
        self.ticks += 1

    def prime(self, row, first_token, position, max_new, pages=None):
        if self.seed is None:
            self.configure()
        super().prime(row, first_token, position, max_new, pages)

    def _select(self, last):
        from ..ops.sampling import sample_ref
        s = self.settings
        if s["top_k"] == 1:
            tok = last.argmax(-1)
        else:
            tok = torch.as_tensor(sample_ref(last.float().cpu(), self.seed,
                                             self.offset0 + int(self.tick), **s))
        if self.vocab_size:
            tok = tok.clamp(max=self.vocab_size - 1)
        return tok.to(last.device)


class ContinuousBatcher:
    """In-flight batching over one ragged decoder: requests queue up, every
    free row of the batch takes the next one, and a row that finishes is
    refilled between replays: no recapture, ever.

    Usage::

        cb = ContinuousBatcher(model, ip, batch, capacity)
        ids = [cb.submit(prompt_tokens, max_new_tokens) for ...]
        results = cb.run()          # token lists, in submission order

    A request yields at most ``max_new_tokens`` tokens: the first is picked
    from the prefill logits, the rest by the decoder, and generation ends
    early with ``stop_id``.  The whole sequence must fit the row's cache
    column (``len(prompt) + max_new_tokens <= capacity``).  A refill prefills
    the prompt eagerly with ``b = 1`` into the row (decode stalls for that
    one prefill); prompts need at least two tokens (a one-token prefill would
    take the decode branch of the attention layers).

    ``poll_every``: the host reads ``active`` every that many replays.  A
    smaller value refills a finished row sooner, a larger one syncs less.
    The default, 4, comes from the sweep of ``profiles/r15c_continuous.txt``
    (Llama-2-7B shapes, generation lengths 16-256): 3.39k / 3.40k / 3.28k /
    2.86k useful tokens/s at 1 / 4 / 16 / 64 at batch 32 and 1.71k / 1.70k /
    1.62k / 1.40k at batch 8.  1 and 4 are within 1 % of each other, so 4
    takes a quarter of the host syncs for nothing; from 16 on the finished
    rows that sit idle until the next read cost 3-18 %.

    ``decoder``: a ``RaggedSamplingDecoder`` (configured) to sample instead of
    the greedy decoder built by default.  The stop token belongs to the
    decoder: ``stop_id`` here is handed to the decoder this class builds, and
    with ``decoder=`` it must be left out or agree with the decoder's.

    ``prefill_chunk``: an integer ``>= 2`` prefills a prompt in pieces that
    end at the multiples of it (a piece of one token is merged into its
    neighbour); None: one call per prompt.  ``prefix_cache=True`` (paged cache
    only) shares the full prompt pages of earlier requests; ``prefix_log``
    records ``(request id, pages matched)`` per admission, ``prefix_hit_pages``
    their sum, ``prefilled_tokens`` the tokens the prefills ran and
    ``evictions`` the cached pages freed for an admission."""

    def __init__(self, model, ip, batch, capacity, poll_every=4, max_new_tokens=None, stop_id=None,
                 decoder=None, capture=None, prefill_chunk=None, prefix_cache=False):
        if capacity > ip.max_sequence_len or batch > ip.max_batch_size:
            raise ValueError("batch / capacity exceed the inference params' cache")
        if poll_every < 1:
            raise ValueError("poll_every must be >= 1")
        if prefill_chunk is not None and int(prefill_chunk) < 2:
            raise ValueError("prefill_chunk must be >= 2 (None: the whole prompt in one call)")
        if prefix_cache and getattr(ip, "page_table", None) is None:
            raise ValueError("prefix_cache needs a paged KV cache (InferenceParams(kv_pages=...))")
        self.model, self.ip, self.batch, self.capacity = model, ip, batch, capacity
        self.poll_every = poll_every
        if decoder is None:
            decoder = RaggedGreedyDecoder(model, ip, batch, max_new_tokens or capacity,
                                          capture=capture)
            decoder.set_stop_id(-1 if stop_id is None else stop_id)
        elif stop_id is not None and stop_id != decoder.stop_id:
            raise ValueError(f"stop_id {stop_id} disagrees with the decoder's {decoder.stop_id}")
        self.dec = decoder
        self.queue = deque()
        self.requests = []      # (prompt, max_new) by request id
        self.results = {}
        self.rows = [None] * batch  # request id, first token per busy row
        self.primed = []        # (row, position, max_new) of every prime, for inspection
        self.replays = 0
        self.paged = getattr(ip, "page_table", None) is not None
        self.pool = PagePool(ip.kv_pages) if self.paged else None
        self.row_pages = [None] * batch  # pages held by each busy row
        self.page_log = []      # (request id, row, pages) of every admission
        self._idle_since = list(range(batch))  # idle rows are offered the queue oldest first
        self._idle_tick = batch
        self.waits = 0          # admissions that found the pool short
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self.cache = PrefixCache(self.pool) if prefix_cache else None
        self.row_cached = [None] * batch  # cache entries each busy row holds a reference to
        self.prefix_log = []    # (request id, pages matched) of every admission
        self.prefix_hit_pages = 0
        self.prefilled_tokens = 0
        self.evictions = 0

    def submit(self, prompt_tokens, max_new_tokens):
        """Queue a request; returns its id (= its index in ``run()``'s result)."""
        prompt = torch.as_tensor(prompt_tokens, dtype=torch.long).view(-1)
        if prompt.numel() < 2:
            raise ValueError("a prompt needs at least two tokens (a one-token prefill would take "
                             "the decode step's branch)")
        if prompt.numel() + max_new_tokens > self.capacity:
            raise ValueError(_TOO_SHORT)
        if max_new_tokens < 1 or max_new_tokens - 1 > self.dec.max_new:
            raise ValueError(f"max_new_tokens must be in [1, {self.dec.max_new + 1}]")
        if self.paged:
            need = pages_for(prompt.numel() + max_new_tokens)
            if need > self.pool.n_pages - 1 or need > self.ip.page_table.shape[1]:
                raise ValueError(f"the request needs {need} KV pages: more than the pool's "
                                 f"{self.pool.n_pages - 1} usable pages or the "
                                 f"{self.ip.page_table.shape[1]} pages of a row")
        self.requests.append((prompt, int(max_new_tokens)))
        self.queue.append(len(self.requests) - 1)
        return len(self.requests) - 1

    def _pieces(self, s0, n):
        """The prefill of positions ``[s0, n)`` as (first, one past the last)
        pieces: cut at the multiples of ``prefill_chunk``, a piece of one token
        (which would take the decode step's branch) merged into a neighbour."""
        if self.prefill_chunk is None:
            return [(s0, n)]
        c = self.prefill_chunk
        cuts = [s0]
        while cuts[-1] < n:
            cuts.append(min(n, (cuts[-1] // c + 1) * c))
        i = 1
        while i < len(cuts) and len(cuts) > 2:
            if cuts[i] - cuts[i - 1] == 1:
                del cuts[i if i < len(cuts) - 1 else i - 1]
            else:
                i += 1
        return list(zip(cuts[:-1], cuts[1:]))

    def _prefill(self, row, prompt, s0=0):
        """Eager ``b = 1`` prefill of ``prompt`` from position ``s0`` (the keys
        before it are in the row's shared pages) into cache column ``row``, in
        the pieces of ``_pieces``; the device slot tensors are hidden so that
        no layer takes the graph branch, and the host offsets are restored for
        the decode step (whose graph branch reads neither)."""
        ip, dev = self.ip, self.dec.tokens.device
        saved = (ip.device_offset, ip.device_kv_len, ip.sequence_len_offset, ip.batch_size_offset,
                 ip.continue_prefill)
        ip.device_offset = ip.device_kv_len = None
        ip.batch_size_offset = row
        try:
            n = prompt.numel()
            tokens = prompt.to(dev)[None]
            for a, b in self._pieces(s0, n):
                ip.sequence_len_offset = a
                ip.continue_prefill = self.paged and a > 0
                pos = torch.arange(a, b, device=dev)[None]
                with torch.no_grad():
                    logits = self.model(tokens[:, a:b], pos, None, inference_params=ip)
            self.prefilled_tokens += n - s0
            return self._first(logits[:, -1])
        finally:
            (ip.device_offset, ip.device_kv_len, ip.sequence_len_offset, ip.batch_size_offset,
             ip.continue_prefill) = saved

    def _first(self, last):
        if self.dec.sample and self.dec.settings["top_k"] != 1:
            from ..ops.sampling import sample_fused
            return int(sample_fused(last, vocab_size=self.dec.vocab_size,
                                    seed_offset=self.dec.draw_seed_offset(), **self.dec.settings))
        return int(last.argmax(-1))

    def _admit(self, row):
        """Fill ``row`` from the queue until a request needs the decoder.
        Paged: the head request's pages are reserved first; if the pool is
        short the request stays at the head and the row stays idle."""
        while self.queue:
            rid = self.queue[0]
            prompt, max_new = self.requests[rid]
            pages, chain = None, []
            if self.paged:
                need = pages_for(prompt.numel() + max_new)
                if self.cache is not None:
                    # the shared pages are held before anything is evicted for the rest
                    chain = self.cache.match(prompt)
                    self.cache.acquire(chain)
                    need -= len(chain)
                    if need > self.pool.available:
                        self.evictions += len(self.cache.evict(need - self.pool.available))
                pages = self.pool.alloc(need)
                if pages is None:
                    if self.cache is not None:
                        self.cache.release(chain)  # it waits without a reference
                    self.waits += 1
                    break
                table = [e.page for e in chain] + pages
                self.page_log.append((rid, row, list(table)))
                # the table row before the eager prefill, which scatters by it
                self.dec.write_table(row, table, prompt.numel() + max_new)
            self.queue.popleft()
            first = self._prefill(row, prompt, len(chain) * KV_PAGE)
            if self.cache is not None:
                self.prefix_log.append((rid, len(chain)))
                self.prefix_hit_pages += len(chain)
                # the row's own full prompt pages now belong to the cache
                chain = chain + self.cache.insert(prompt, table, len(chain))
                cached = {e.page for e in chain}
                pages = [p for p in pages if p not in cached]
            if max_new == 1 or (self.dec.stop_id >= 0 and first == self.dec.stop_id):
                self.results[rid] = [first]  # done on its first token
                if self.paged:
                    self._give_back(row, pages, chain)
                continue
            self.dec.prime(row, first, prompt.numel(), max_new - 1)
            self.primed.append((row, prompt.numel(), max_new - 1))
            self.rows[row] = (rid, first)
            self.row_pages[row] = pages
            self.row_cached[row] = chain
            return
        self.rows[row] = None

    def _give_back(self, row, pages, cached=()):
        """The order that keeps a parked row from corrupting its successor:
        ``release`` is enqueued first (the row's later K / V writes go to the
        null page), then the row's private pages return to the free list and
        its cached pages lose a reader."""
        self.dec.release(row)
        self.pool.free(pages)
        if cached:
            self.cache.release(cached)

    def _collect(self, row, hist_idx):
        rid, first = self.rows[row]
        self.results[rid] = [first] + self.dec.history[row, :hist_idx[row]].tolist()
        if self.paged:
            self._give_back(row, self.row_pages[row], self.row_cached[row] or ())
            self.row_pages[row] = self.row_cached[row] = None
            self._idle_since[row], self._idle_tick = self._idle_tick, self._idle_tick + 1
        self.rows[row] = None

    def run(self):
        """Serve every queued request; token lists in submission order."""
        dec = self.dec
        for row in range(self.batch):
            if self.rows[row] is None:
                self._admit(row)
        while any(r is not None for r in self.rows):
            for _ in range(self.poll_every):
                dec.step()
            self.replays += self.poll_every
            active = dec.active.tolist()
            if all(active[row] for row in range(self.batch) if self.rows[row] is not None):
                continue
            hist_idx = dec.hist_idx.tolist()
            done = [row for row in range(self.batch)
                    if self.rows[row] is not None and not active[row]]
            if not self.paged:
                for row in done:
                    self._collect(row, hist_idx)
                    self._admit(row)
                continue
            # paged: free every finished row's pages first, then offer the queue
            # to every idle row (a request that waited for pages may now fit)
            for row in done:
                self._collect(row, hist_idx)
            idle = [row for row in range(self.batch) if self.rows[row] is None]
            for row in sorted(idle, key=self._idle_since.__getitem__):
                self._admit(row)
        return [self.results[i] for i in range(len(self.requests))]
