"""Ragged decode on the GPU: per-row key counts in the decode attention,
per-row cache slots in the QKV epilogue and the FP8 store, the ragged tails,
and the decoders / batcher of ``inference/continuous.py`` on one captured graph.

Almost every check is exact: a ragged launch does, for row i, the arithmetic
of a uniform launch of the same batch, capacity and keys per wave with the
scalar set to row i's value, so outputs are compared bit for bit."""
import types

import pytest
import torch

import attention_edge_inputs as E
from dist_utils import run_dist, init_framework

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = 600


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


# ---------------------------------------------------------------- 1. decode attention, per-row lengths

DEC_B = 4
WINDOWS = (0, 33, 257)


def _length_vectors(x, w):
    """Vectors of DEC_B lengths over every (kv_len, w) case of the edge
    inputs: for w = 0 that is every chunk edge of DECODE_LENS."""
    ns = [n for n, ww in x.cases if ww == w]
    vecs = [(0, 1, 600, 257), (255, 256, 257, 605), (31, 32, 33, 512)] if w == 0 else []
    assert all(n in ns for v in vecs for n in v)
    for i in range(0, len(ns), DEC_B):
        v = ns[i:i + DEC_B]
        vecs.append(tuple(v + ns[:DEC_B - len(v)]))
    assert all(len(set(min(n, CAP) for n in v)) > 1 for v in vecs)
    return vecs


def _seqs4(x, mem):
    """``[DEC_B, cap, nkv, hd]``: sequences 0, 1, 0, 1 of the edge inputs (a row
    is told from the one two below by its length)."""
    return mem[:x.cap, [1, 2, 1, 2]].transpose(0, 1)


def _expect(x, vecs, w):
    """The edge inputs' expectations gathered per row: row i of vector j is
    case (n_ji, w) of sequence i % 2."""
    ci = torch.tensor([[x.cases.index((n, w)) for n in v] for v in vecs], device=DEV)
    seq = (torch.arange(DEC_B, device=DEV) % E.DECODE_B)[None].expand_as(ci)
    for v, row in zip(vecs, ci.tolist()):  # per-row visibility: the mask rule itself
        for n, c in zip(v, row):
            assert torch.equal(x.vis[c].cpu(), E.decode_visibility(min(n, x.cap), w, x.rows))
    y = types.SimpleNamespace(needle_e=x.needle_e[ci, seq], needle_ref=x.needle_ref[ci, seq],
                              t_visible=x.t_visible[ci, seq])
    return ci, seq, x.census_e[ci, seq], y


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("r", [1, 2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_decode_per_row_lengths(dtype, hd, r, fp8):
    """b = 4 over a 600-key cache, keys per wave forced to 8 / 16 / 64, windows
    0 / 33 / 257: output row i of the per-row launch equals, bitwise, row i of
    the scalar launch with kv_len = n_i, and the per-row launch itself passes
    the census and needle checks of the mask-edge inputs."""
    from test_attention_edges_gpu import _decode, _store
    x = E.decode_inputs(dtype, hd, r, fp8, CAP, DEV)
    sc = torch.stack([x.k_scale, x.v_scale]).float().contiguous() if fp8 else None
    kk, vc, vn = (_seqs4(x, _store(x, t)) for t in (x.k, x.v_census, x.v_needle))
    qc = x.q_census[[0, 1, 0, 1]]
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for w in WINDOWS:
            vecs = _length_vectors(x, w)
            ci, seq, census_e, y = _expect(x, vecs, w)
            for kpw in (8, 16, 64):
                oc, on = [], []
                for j, v in enumerate(vecs):
                    lens = torch.tensor(v, dtype=torch.int32, device=DEV)
                    qn = x.q_needle[ci[j], seq[j]].unsqueeze(1)
                    oc.append(_decode(qc, kk, vc, sc, lens, w, kpw))
                    on.append(_decode(qn, kk, vn, sc, lens, w, kpw))
                    for i, n in enumerate(v):
                        if n in v[:i]:
                            continue
                        one.fill_(n)
                        what = f"w={w} kpw={kpw} lens={v} row {i}"
                        sc_c = _decode(qc, kk, vc, sc, one, w, kpw)
                        sc_n = _decode(qn, kk, vn, sc, one, w, kpw)
                        rows = [i2 for i2, n2 in enumerate(v) if n2 == n]
                        assert torch.equal(oc[-1][rows].view(torch.int16),
                                           sc_c[rows].view(torch.int16)), what + " census"
                        assert torch.equal(on[-1][rows].view(torch.int16),
                                           sc_n[rows].view(torch.int16)), what + " needle"
                oc, on = torch.stack(oc), torch.stack(on)
                ok = E.census_ok(oc, census_e)
                assert ok.all(), f"w={w} kpw={kpw}: census off for {[v for v, g in zip(vecs, ok.tolist()) if not g]}"
                ok = E.needle_ok(on, y)
                assert ok.all(), f"w={w} kpw={kpw}: needle off for {[v for v, g in zip(vecs, ok.tolist()) if not g]}"
                zero = torch.tensor([[n == 0 for n in v] for v in vecs], device=DEV)
                assert not oc[zero].any() and not on[zero].any()  # kv_len 0: exact zeros


def test_decode_per_row_checks_see_the_row():
    """The negative run: with the lengths rotated by one row the per-row launch
    fails the census check for every vector and the needle check for most (a
    kernel that read another row's length fails on the data)."""
    from test_attention_edges_gpu import _decode, _store
    x = E.decode_inputs(torch.bfloat16, 128, 4, False, CAP, DEV)
    kk, vc, vn = (_seqs4(x, _store(x, t)) for t in (x.k, x.v_census, x.v_needle))
    qc = x.q_census[[0, 1, 0, 1]]
    for w in WINDOWS:
        vecs = _length_vectors(x, w)
        ci, seq, census_e, y = _expect(x, vecs, w)
        oc, on = [], []
        with torch.no_grad():
            for j, v in enumerate(vecs):
                lens = torch.tensor(v, dtype=torch.int32, device=DEV).roll(1)
                oc.append(_decode(qc, kk, vc, None, lens, w, 16))
                on.append(_decode(x.q_needle[ci[j], seq[j]].unsqueeze(1), kk, vn, None, lens, w, 16))
        assert not E.census_ok(torch.stack(oc), census_e).any(), w
        assert E.needle_ok(torch.stack(on), y).sum() <= len(vecs) // 2, w


# ---------------------------------------------------------------- 2. QKV epilogue and FP8 store, per-row slots

SENT16, SENT8 = -1.5, 0xA5


def _qkv_weights(form, N, K, dt, seed):
    """(weight argument, packed flag, scale argument) of one weight format."""
    from epfl_megatron_amd.ops import decode_pack, fp8_weights as f8, mxfp4_weights as mx
    torch.manual_seed(seed)
    w = (torch.randn(N, K, device=DEV) * 0.05).to(dt)
    if form == "rowmajor":
        return w, False, None
    if form == "packed":
        return decode_pack.pack(w), True, None
    if form == "fp8w":
        q8, wsc = f8.quantize_rows(w)
        return f8.pack_fp8(q8), True, wsc
    p4, s4 = mx.pack_mxfp4(*mx.quantize_blocks(w))
    return p4, True, s4


@pytest.mark.parametrize("form", ["rowmajor", "packed", "fp8w", "mxfp4"])
@pytest.mark.parametrize("K,ng", [(512, 2), (4096, 1)], ids=["per-block", "persistent"])
@pytest.mark.parametrize("M", [3, 16, 24])
def test_qkv_epilogue_per_row_slots(M, K, ng, form):
    """``skinny_qkv_rope_cache`` with one distinct slot per row against caches
    pre-filled with a sentinel: the whole cache equals, bitwise, the one
    assembled from M scalar-slot calls (row m from the call with slot =
    slot[m]), q is bitwise the scalar call's, every sentinel outside the M
    written rows is intact.  bf16 and fp16, each normed and un-normed (M = 24:
    un-normed, as the decode layer runs 17-32 rows), 16-bit and FP8 caches."""
    from epfl_megatron_amd.ops.rope import rope_table
    C = _ext()
    r, hd, L, B, b0 = 2, 128, CAP, M + 2, 1
    N = ng * (r + 2) * hd
    slots = [0, 599, 7] + [(37 * m + 11) % 590 + 8 for m in range(3, M)]
    assert len(set(slots)) == M and max(slots) < L
    cos, sin = rope_table(hd, 64, DEV)
    pos = (torch.arange(M, device=DEV).view(M, 1) * 3 + 2) % 64
    sc = torch.ldexp(torch.ones(2, ng), torch.arange(2 * ng).view(2, ng) - 6.0).to(DEV)
    for dt, normed in [(dt, nm) for dt in (torch.bfloat16, torch.float16)
                       for nm in ((True, False) if M <= 16 else (False,))]:
        w, packed, wsc = _qkv_weights(form, N, K, dt, 10 * M + K)
        torch.manual_seed(M)
        x = torch.randn(M, K, device=DEV, dtype=dt)
        g = (torch.rand(K, device=DEV) + 0.5).to(dt) if normed else None
        st = torch.tensor(slots, device=DEV)
        for kv8 in (False, True):
            def fresh():
                if kv8:
                    return torch.full((L, B, ng, hd), SENT8, device=DEV, dtype=torch.uint8)
                return torch.full((L, B, ng, hd), SENT16, device=DEV, dtype=dt)
            tail = (packed, wsc) + ((sc,) if kv8 else ())
            args = (x, w, g, 1e-5, ng, r, hd, cos, sin, pos)
            what = f"{form} {dt} normed={normed} kv8={kv8}"
            with torch.no_grad():
                kr, vr = fresh(), fresh()
                q = C.skinny_qkv_rope_cache(*args, kr[:, b0:b0 + M], vr[:, b0:b0 + M], st, 0, *tail)
                ke, ve = fresh(), fresh()
                for m, s in enumerate(slots):
                    ks, vs = fresh(), fresh()
                    one = torch.tensor([s], device=DEV)
                    qs = C.skinny_qkv_rope_cache(*args, ks[:, b0:b0 + M], vs[:, b0:b0 + M], one, 0, *tail)
                    assert torch.equal(q.view(torch.int16), qs.view(torch.int16)), what + " q"
                    ke[s, b0 + m], ve[s, b0 + m] = ks[s, b0 + m], vs[s, b0 + m]
            bits = torch.uint8 if kv8 else torch.int16
            assert torch.equal(kr.view(bits), ke.view(bits)), what + " k cache"
            assert torch.equal(vr.view(bits), ve.view(bits)), what + " v cache"
            keep = torch.ones(L, B, dtype=torch.bool, device=DEV)
            keep[st, torch.arange(M, device=DEV) + b0] = False
            sent = SENT8 if kv8 else SENT16
            assert bool((kr[keep] == sent).all()) and bool((vr[keep] == sent).all()), what
            assert bool((kr[~keep] != sent).any()) and bool((vr[~keep] != sent).any()), what


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("b", [3, 24])
def test_kv_store_fp8_per_row_slots(b, dt):
    """``kv_store_fp8`` (sq = 1) with one slot per sequence: the caches equal
    the ones assembled from scalar-slot stores, sentinels elsewhere intact."""
    from epfl_megatron_amd.ops import fp8_kv
    nkv, r, hd, L, B, b0 = 2, 2, 128, CAP, b + 2, 1
    torch.manual_seed(b)
    mixed = (torch.randn(1, b, nkv, r + 2, hd, device=DEV) * 30).to(dt)
    k, v = mixed[:, :, :, r], mixed[:, :, :, r + 1]
    sc = torch.ldexp(torch.ones(2, nkv), torch.arange(2 * nkv).view(2, nkv) - 3.0).to(DEV)
    slots = [0, 599, 7] + [(37 * m + 11) % 590 + 8 for m in range(3, b)]
    st = torch.tensor(slots, device=DEV)
    k8, v8 = (torch.full((L, B, nkv, hd), SENT8, device=DEV, dtype=torch.uint8) for _ in range(2))
    fp8_kv.store(k, v, k8[:, b0:b0 + b], v8[:, b0:b0 + b], sc, slot_t=st)
    ke, ve = torch.full_like(k8, SENT8), torch.full_like(v8, SENT8)
    for m, s in enumerate(slots):
        ks, vs = torch.full_like(k8, SENT8), torch.full_like(v8, SENT8)
        fp8_kv.store(k, v, ks[:, b0:b0 + b], vs[:, b0:b0 + b], sc, slot_t=torch.tensor([s], device=DEV))
        ke[s, b0 + m], ve[s, b0 + m] = ks[s, b0 + m], vs[s, b0 + m]
    assert torch.equal(k8, ke) and torch.equal(v8, ve)
    assert torch.equal(k8[st, torch.arange(b, device=DEV) + b0], fp8_kv.quantize(k[0], sc[0]))
    keep = torch.ones(L, B, dtype=torch.bool, device=DEV)
    keep[st, torch.arange(b, device=DEV) + b0] = False
    assert bool((k8[keep] == SENT8).all()) and bool((v8[keep] == SENT8).all())


# ---------------------------------------------------------------- 3. ragged tails

SEED, OFFSET = 1234, 40


class _RaggedState:
    """The ragged tail's state at b = 5: rows 0 and 4 run on, row 1 stops on
    stop_id (planted in step 2), row 2 on its limit (2), row 3 is parked."""

    def __init__(self, dev, top_k=0, top_p=0.0, temperature=1.0, stop_id=-1):
        L = torch.long
        self.tokens = torch.full((5,), -7, dtype=L, device=dev)
        self.history = torch.full((5, 6), -7, dtype=L, device=dev)
        self.hist_idx = torch.tensor([0, 1, 0, 2, 0], dtype=L, device=dev)
        self.pos = torch.tensor([5, 9, 30, 77, 598], dtype=L, device=dev)
        self.slot = self.pos.clone()
        self.kv_len = (self.pos + 1).int()
        self.active = torch.tensor([1, 1, 1, 0, 1], dtype=torch.int32, device=dev)
        self.limit = torch.tensor([6, 6, 2, 6, 6], dtype=L, device=dev)
        self.tick = torch.tensor([3], dtype=L, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ctl = torch.tensor([SEED, OFFSET, top_k, 0, stop_id, -1], dtype=L, device=dev)
        self.fctl = torch.tensor([temperature, top_p], dtype=torch.float32, device=dev)

    def fields(self):
        return (self.tokens, self.history, self.hist_idx, self.pos, self.slot, self.kv_len,
                self.active, self.limit, self.tick)

    def launch(self, logits, sample):
        _ext().ragged_tail(logits, *self.fields(), self.counter, self.ctl, self.fctl, sample)

    def emulate(self, tok):
        """The tail's bookkeeping for the selected tokens ``tok``, row by row."""
        stop = int(self.ctl[4])
        for row in range(5):
            if not int(self.active[row]):
                continue
            t, hi = int(tok[row]), int(self.hist_idx[row])
            self.tokens[row] = t
            self.history[row, hi] = t
            self.hist_idx[row] = hi + 1
            if (stop >= 0 and t == stop) or hi + 1 == int(self.limit[row]):
                self.active[row] = 0
            else:
                self.pos[row] += 1
                self.slot[row] += 1
                self.kv_len[row] += 1
        self.tick += 1
        self.ctl[5] = int(self.active.sum())

    def same(self, other):
        return all(torch.equal(a.cpu(), b.cpu()) for a, b in
                   zip(self.fields() + (self.ctl, self.counter),
                       other.fields() + (other.ctl, other.counter)))


def _tail_logits(step, dtype, stop_row=None, stop_id=None):
    torch.manual_seed(100 + step)
    x = (torch.randn(5, 512, device=DEV) * 3).to(dtype)
    x[:, 100 + step] = x.max()  # a tied maximum per row at most: the first index wins
    if stop_row is not None:
        x[stop_row, stop_id] = 60.0
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "top_k_1"])
def test_ragged_tail_greedy(sample, dtype):
    """Four launches at b = 5, V = 512 against the torch emulation: a row stops
    on stop_id, one on its limit, a parked row keeps its sentinels; ctl[5], the
    tick and the zeroed counter after every launch; tokens = torch.argmax."""
    stop = 300
    st = _RaggedState(DEV, top_k=1 if sample else 0, stop_id=stop)
    em = _RaggedState("cpu", top_k=1 if sample else 0, stop_id=stop)
    left = []
    for step in range(4):
        logits = _tail_logits(step, dtype, 1 if step == 1 else None, stop)
        was = st.active.clone().bool()
        st.launch(logits, sample)
        em.emulate(logits.float().argmax(1).cpu())
        assert st.same(em), step
        assert torch.equal(st.tokens[was], logits.float().argmax(1)[was])
        assert int(st.counter) == 0 and int(st.tick) == 4 + step
        left.append(int(st.ctl[5]))
    assert left == [4, 2, 2, 2]  # step 2: row 1 emits stop_id, row 2 reaches its limit
    assert st.active.tolist() == [1, 0, 0, 0, 1] and st.hist_idx.tolist() == [4, 3, 2, 2, 4]
    assert st.history[3].tolist() == [-7] * 6 and int(st.tokens[3]) == -7
    assert st.slot.tolist() == [9, 10, 31, 77, 602]  # finished rows stay where they were


@pytest.mark.parametrize("kw", [dict(top_p=0.9, temperature=0.8), dict(top_k=40, temperature=1.3)])
def test_ragged_tail_sampling_offset_is_the_tick(kw):
    """With a temperature every active row's token is ``ops/sampling.py``'s
    reference draw at Philox offset offset0 + tick (not the row's history
    index), and the bookkeeping follows the emulation."""
    from epfl_megatron_amd.ops.sampling import sample_ref
    st, em = _RaggedState(DEV, **kw), _RaggedState("cpu", **kw)
    checked = ambiguous = 0
    for step in range(4):
        logits = _tail_logits(step, torch.bfloat16)
        tick, was = int(st.tick), st.active.tolist()
        st.launch(logits, True)
        _, sets = sample_ref(logits, SEED, OFFSET + tick, return_sets=True, **kw)
        for row in range(5):
            if was[row]:
                assert int(st.tokens[row]) in sets[row], (step, row, int(st.tokens[row]), sets[row])
                checked += 1
                ambiguous += len(sets[row]) > 1
        em.emulate(st.tokens.cpu())
        assert st.same(em), step
    assert st.tokens.unique().numel() > 2
    # an offset check only while the reference sets are singletons (the bound of
    # test_sampling_gpu.py: at most 1 % of the rows ambiguous)
    assert checked >= 12 and ambiguous <= 0.01 * checked, (ambiguous, checked)


# ---------------------------------------------------------------- 4-7. the decoders and the batcher

def _model(extra=()):
    """The tiny GQA Llama of test_gpu_e2e.py in bf16, its rotary table long
    enough for the 600-slot cache (the 300-token prompt decodes past 256)."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA
    from test_parallel_equivalence import _deterministic_init
    init_framework(LLAMA_GQA + ["--bf16", "--max_position_embeddings", "640"] + list(extra),
                   finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, get_args())
    return model[0].eval()


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in (5, 29, 300, 64)]


def _prefill(m, ip, row, prompt):
    """Eager b = 1 prefill into cache column ``row``; the logits of the last position."""
    saved = ip.device_offset, ip.device_kv_len
    ip.device_offset = ip.device_kv_len = None
    ip.sequence_len_offset, ip.batch_size_offset = 0, row
    with torch.no_grad():
        out = m(prompt[None], torch.arange(prompt.numel(), device=DEV)[None], None, inference_params=ip)
    ip.batch_size_offset = 0
    ip.device_offset, ip.device_kv_len = saved
    return out[0, -1].clone()


def _lockstep(m, prompt, b, marks):
    """``prompt`` prefilled (b = 1) into all ``b`` rows of a fresh cache and
    decoded by GraphedGreedyDecoder: (first token, history, {step: logits})."""
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    ip = InferenceParams(b, CAP)
    first = [int(_prefill(m, ip, row, prompt).argmax()) for row in range(b)]
    dec = GraphedGreedyDecoder(m, ip, b, max(marks))
    dec.start(torch.tensor(first, device=DEV).view(b, 1), prompt.numel())
    logits = {}
    for s in range(1, max(marks) + 1):
        dec.step()
        if s in marks:
            logits[s] = dec.logits[:, -1].clone()
    return first, dec.history[:, :max(marks)].clone(), logits


def _bits(t):
    return t.contiguous().view(torch.int16)


def _uniform(rank, world, extra):
    """Test 4: every row primed at the same position against GraphedGreedyDecoder."""
    from epfl_megatron_amd.inference import RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m = _model(extra)
    b, n, plen = 3, 10, 29
    torch.manual_seed(5)
    prompt = torch.randint(0, 512, (b, plen), device=DEV)
    pos = torch.arange(plen, device=DEV)[None].expand(b, -1)
    hist, logits = [], []
    for ragged in (False, True):
        ip = InferenceParams(b, CAP)
        with torch.no_grad():
            first = m(prompt, pos, None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
        ip.sequence_len_offset = plen
        if ragged:
            dec = RaggedGreedyDecoder(m, ip, b, n)
            for row in range(b):
                dec.prime(row, int(first[row]), plen, n)
        else:
            from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
            dec = GraphedGreedyDecoder(m, ip, b, n)
            dec.start(first, plen)
        for _ in range(n):
            dec.step()
        hist.append(dec.history[:, :n].cpu())
        logits.append(_bits(dec.logits[:, -1]).cpu())
    from epfl_megatron_amd.models import transformer
    return (hist, logits, dec.active_rows(), dec.captures, ip.key_value_memory_dict[1][0].dtype,
            transformer._DECODE_FUSED)


@pytest.mark.parametrize("extra,fused", [((), "1"), (("--inference_fp8_kv_cache",), "1"),
                                         (("--inference_fp8_kv_cache",), "0"), ((), "0")],
                         ids=["kv16-fused", "kv8-fused", "kv8-unfused", "kv16-unfused"])
def test_ragged_decoder_uniform_lengths_match_lockstep(extra, fused):
    hist, logits, active, captures, cache_dt, was_fused = run_dist(
        _uniform, 1, list(extra), env={"EMA_DECODE_FUSED": fused})[0]
    assert was_fused == (fused == "1")  # the switch reached the worker's model code
    assert cache_dt == (torch.uint8 if extra else torch.bfloat16)
    assert torch.equal(hist[0], hist[1]), (hist[0], hist[1])
    assert torch.equal(logits[0], logits[1])
    assert active == [] and captures == 1


def _ragged(rank, world):
    """Tests 5 and 6: ragged prompts, then the refill of row 1 by the batcher."""
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m = _model()
    P, b = _prompts(), 3
    out = {}
    # references: prompt i in all three rows of a fresh cache, lockstep decode
    refs = [_lockstep(m, P[i], b, (10, 12)) for i in range(3)]
    ref3 = _lockstep(m, P[3], b, (6,))
    # ragged run, no refill, 12 tokens; logits after the steps 1, 10 and 12
    ip = InferenceParams(b, CAP)
    first = [int(_prefill(m, ip, row, P[row]).argmax()) for row in range(b)]
    dec = RaggedGreedyDecoder(m, ip, b, 12)
    for row in range(b):
        dec.prime(row, first[row], P[row].numel(), 12)
    lg = {}
    for s in range(1, 13):
        dec.step()
        if s in (1, 10, 12):
            lg[s] = dec.logits[:, -1].clone()
    hist = dec.history.clone()
    out["first_ok"] = [first[i] == refs[i][0][i] for i in range(b)]
    out["tok10"] = [torch.equal(hist[i, :10], refs[i][1][i, :10]) for i in range(b)]
    out["log10"] = [torch.equal(_bits(lg[10][i]), _bits(refs[i][2][10][i])) for i in range(b)]
    out["tok12"] = [torch.equal(hist[i], refs[i][1][i]) for i in range(b)]
    out["log12"] = [torch.equal(_bits(lg[12][i]), _bits(refs[i][2][12][i])) for i in range(b)]
    out["state"] = (dec.active_rows(), dec.hist_idx.tolist(), dec.captures)
    # loose end-to-end check: row 2's first step against the eager KV-cached forward
    ipe = InferenceParams(1, CAP)
    _prefill(m, ipe, 0, P[2])
    ipe.sequence_len_offset = P[2].numel()
    with torch.no_grad():
        le = m(torch.tensor([[first[2]]], device=DEV), torch.tensor([[P[2].numel()]], device=DEV),
               None, inference_params=ipe)[0, -1].float()
    out["eager"] = (float((lg[1][2].float() - le).abs().max()), float(le.abs().max()))
    # the batcher: row 1 finishes after 4 steps and takes the 64-token prompt
    ipb = InferenceParams(b, CAP)
    cb = ContinuousBatcher(m, ipb, b, CAP, poll_every=1, max_new_tokens=12)
    for prompt, mn in ((P[0], 13), (P[1], 5), (P[2], 13), (P[3], 7)):
        cb.submit(prompt.cpu(), mn)
    res = cb.run()
    final = cb.dec.logits[:, -1]
    out["cb_rows"] = [res[i] == [refs[i][0][i]] + refs[i][1][i, :n].tolist()
                      for i, n in ((0, 12), (1, 4), (2, 12))]
    out["cb_final"] = [torch.equal(_bits(final[i]), _bits(lg[12][i])) for i in (0, 2)]
    out["cb_refill"] = res[3] == [ref3[0][1]] + ref3[1][1, :6].tolist()
    out["cb_state"] = (cb.dec.captures, cb.dec.hist_idx.tolist(), cb.dec.active.tolist(),
                       cb.replays, cb.primed)
    errs = []
    for args in ((P[0][:1].cpu(), 4), (P[1].cpu(), CAP - 29 + 1)):
        try:
            cb.submit(*args)
            errs.append(None)
        except ValueError as e:
            errs.append(str(e))
    try:
        cb.dec.prime(0, 1, 29, 12)
        cb.dec.prime(0, 1, CAP - 11, 12)
        errs.append(None)
    except ValueError as e:
        errs.append(str(e))
    out["errs"] = errs
    return out


@pytest.fixture(scope="module")
def ragged_run():
    return run_dist(_ragged, 1)[0]


def test_ragged_lengths_match_per_prompt_lockstep(ragged_run):
    """b = 3, prompts of 5 / 29 / 300 tokens, n = 10: row i's tokens and last
    logits are bitwise those of prompt i decoded in lockstep in all three rows."""
    r = ragged_run
    assert all(r["first_ok"]) and all(r["tok10"]) and all(r["log10"]), r
    lerr, scale = r["eager"]
    assert lerr < 2e-2 * max(1.0, scale), (lerr, scale)


def test_refill_leaves_the_other_rows_bitwise_alone(ragged_run):
    """Row 1 (limit 4) is refilled with a 64-token prompt while rows 0 and 2 run
    on to 12 tokens: one captured graph, rows 0 and 2 bitwise the run without a
    refill, row 1's second generation bitwise its own reference."""
    r = ragged_run
    assert all(r["tok12"]) and all(r["log12"]), r
    assert r["state"] == ([], [12, 12, 12], 1)
    assert all(r["cb_rows"]) and all(r["cb_final"]) and r["cb_refill"], r
    captures, hist_idx, active, replays, primed = r["cb_state"]
    assert captures == 1 and hist_idx == [12, 6, 12] and active == [0, 0, 0] and replays == 12
    assert primed == [(0, 5, 12), (1, 29, 4), (2, 300, 12), (1, 64, 6)]
    one_token, too_long, prime = r["errs"]
    assert one_token is not None and "two tokens" in one_token
    assert too_long == prime == "KV cache too short for max_new_tokens"


def _sampling(rank, world):
    """Test 7: the sampling decoder."""
    from epfl_megatron_amd.inference import RaggedGreedyDecoder, RaggedSamplingDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.ops.sampling import sample_ref
    m = _model()
    P, b, n = _prompts(), 3, 8

    def fresh(cls, **kw):
        ip = InferenceParams(b, CAP)
        first = [int(_prefill(m, ip, row, P[row]).argmax()) for row in range(b)]
        return cls(m, ip, b, n, **kw), first

    out = {}
    greedy, first = fresh(RaggedGreedyDecoder)
    top1, _ = fresh(RaggedSamplingDecoder, vocab_size=512)
    top1.configure(top_k=1)
    for dec in (greedy, top1):
        for row in range(b):
            dec.prime(row, first[row], P[row].numel(), n)
        for _ in range(n):
            dec.step()
    out["top1"] = torch.equal(greedy.history, top1.history)
    kw = dict(top_p=0.9, temperature=0.8)
    runs, bad, checked = [], [], [0, 0]
    for rep in range(2):
        torch.manual_seed(77)
        dec, _ = fresh(RaggedSamplingDecoder, vocab_size=512)
        dec.configure(**kw)
        dec.prime(0, first[0], P[0].numel(), n)
        dec.prime(1, first[1], P[1].numel(), 3)
        dec.prime(2, first[2], P[2].numel(), n)
        for t in range(n):
            if t == 5:  # row 1 parked itself after 3 replays: refill it at tick 5
                _prefill(m, dec.ip, 1, P[3])
                dec.prime(1, first[1], P[3].numel(), 3)
            was = dec.active.tolist()
            dec.step()
            if rep == 0:
                assert int(dec.tick) == t + 1
                _, sets = sample_ref(dec.logits[:, -1], dec.seed, dec.offset0 + t, vocab_size=512,
                                     return_sets=True, **kw)
                for row in range(b):
                    if was[row] and int(dec.tokens[row, 0]) not in sets[row]:
                        bad.append((t, row, int(dec.tokens[row, 0]), sets[row]))
                    checked[0] += bool(was[row])
                    checked[1] += bool(was[row]) and len(sets[row]) > 1
        runs.append((dec.history.cpu().tolist(), dec.hist_idx.tolist()))
    out["bad"], out["runs"], out["offset_moved"] = bad, runs, None
    out["checked"] = checked
    # the batcher with sampled first tokens, refills and blocks of 8 offsets: the
    # generator is shared by the replays and the first-token draws
    from epfl_megatron_amd.inference import ContinuousBatcher
    torch.manual_seed(99)
    ipb = InferenceParams(b, CAP)
    decb = RaggedSamplingDecoder(m, ipb, b, n, vocab_size=512)
    decb.RESERVE = 8
    decb.configure(**kw)
    cb = ContinuousBatcher(m, ipb, b, CAP, poll_every=1, decoder=decb)
    used, badb, chk = [], [], [0, 0]
    replay = decb.step

    def step():
        was = decb.active.tolist()
        replay()
        off = decb.offset0 + decb.ticks - 1
        used.append(off)
        _, sets = sample_ref(decb.logits[:, -1], decb.seed, off, vocab_size=512, return_sets=True, **kw)
        for row in range(b):
            if was[row]:
                chk[0] += 1
                chk[1] += len(sets[row]) > 1
                if int(decb.tokens[row, 0]) not in sets[row]:
                    badb.append((off, row, int(decb.tokens[row, 0]), sets[row]))
    decb.step = step
    gens = (9, 4, 9, 5, 6, 3)
    for i, mn in enumerate(gens):
        cb.submit(P[i % 4].cpu(), mn)
    res = cb.run()
    out["cb"] = dict(used=used, first=list(decb.first_draws), blocks=list(decb.blocks), bad=badb,
                     chk=chk, lens=[len(r) for r in res], gens=list(gens), tick=int(decb.tick),
                     captures=decb.captures)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    out["offset_moved"] = gen.get_offset() >= dec.offset0 + n
    return out


def test_ragged_sampling_decoder():
    r = run_dist(_sampling, 1)[0]
    assert r["top1"]                      # top_k = 1 is the greedy decoder, bitwise
    assert r["runs"][0] == r["runs"][1]   # same generator state, same tokens
    assert r["runs"][0][1] == [8, 3, 8]   # the refilled row generated 3 more
    assert not r["bad"], r["bad"]         # every draw at offset0 + tick, the refilled row's too
    assert r["offset_moved"]
    assert r["checked"][0] >= 20 and r["checked"][1] <= 0.01 * r["checked"][0], r["checked"]
    _check_offsets(r["cb"])
    c = r["cb"]
    assert c["lens"] == c["gens"] and c["captures"] == 1 and not c["bad"], c
    assert c["chk"][0] >= 20 and c["chk"][1] <= 0.01 * c["chk"][0], c["chk"]


def _check_offsets(c):
    """The Philox offsets of a run: every replay inside a reserved block, no
    offset twice, none shared with a first-token draw (4 offsets each, the
    generator's granularity), more than one block taken."""
    used, first, blocks = c["used"], c["first"], c["blocks"]
    assert c["tick"] == len(used) and len(set(used)) == len(used)
    assert len(first) == len(c["gens"]) and len(blocks) >= 2
    assert all(any(lo <= u < hi for lo, hi in blocks) for u in used)
    taken = [(lo, hi) for lo, hi in blocks] + [(f, f + 4) for f in first]
    taken.sort()
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:])), taken  # disjoint ranges
