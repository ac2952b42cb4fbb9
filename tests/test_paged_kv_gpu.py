"""Paged KV cache on the GPU: the page table in the decode attention and the
ragged tail, the QKV epilogue and the FP8 store over a stride-0 pool, and the
paged ``ContinuousBatcher`` on one captured graph.

Paging changes only where a chunk's rows are fetched from: with the same
logical capacity (hence the same keys per wave, split count and combine order)
the paged kernel must equal, bit for bit, the per-row kernel on the gathered
contiguous cache.  No tolerance appears in the kernel tests."""
import types

import pytest
import torch

import attention_edge_inputs as E
from dist_utils import run_dist, init_framework
from test_paged_kv import CAP, REQUESTS, request_prompts

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAGE = 256
NKV = 2


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def test_one_page_size():
    from epfl_megatron_amd.inference.paged import KV_PAGE
    assert _ext().KV_PAGE == KV_PAGE == PAGE


# ---------------------------------------------------------------- helpers

def _call(q, k, v, sc, kv_len, window, kpw, table=None, sk=None, **over):
    """``flash_decode`` with the keys per wave forced: k / v ``[b, sk, nkv, hd]``
    column caches, or with ``table`` the pool ``[1, rows, nkv, hd]``."""
    from epfl_megatron_amd.ops.attention import _bsnd_strides
    b, _, nq, d = q.shape
    nkv = k.shape[2]
    out = torch.zeros(b, 1, nq, d, dtype=q.dtype, device=q.device)
    args = dict(q=q, k=k, v=v, out=out, b=b, sk=k.shape[1] if sk is None else sk, nq=nq, nkv=nkv,
                hd=d, qs=list(_bsnd_strides(q, nq // nkv)), ks=list(_bsnd_strides(k, 1)[:3]),
                vs=list(_bsnd_strides(v, 1)[:3]), os=[out.stride(0), out.stride(1), out.stride(2)],
                scale=d ** -0.5, kv_len=kv_len, kpw=kpw, window=window, kv_scale=sc)
    if table is not None:
        args["page_table"] = table
    args.update(over)
    _ext().flash_decode(**args)
    return out[:, 0]


def _dead(t):
    """The value no visible key may hold: NaN, or the e4m3 NaN byte."""
    return 0x7f if t.dtype == torch.uint8 else float("nan")


def _paginate(cache, table, lens, n_pages):
    """``cache [b, cap, nkv, hd]`` -> (the pool ``[n_pages * 256, 1, nkv, hd]``
    with row i's first ``lens[i]`` keys at the rows ``table`` names and the dead
    value everywhere else, the cache with the dead value past each length)."""
    b, cap = cache.shape[:2]
    pool = torch.full((n_pages * PAGE, 1) + cache.shape[2:], _dead(cache), dtype=cache.dtype,
                      device=cache.device)
    gathered = cache.clone()
    j = torch.arange(cap, device=cache.device)
    for i, n in enumerate(lens):
        gathered[i, n:] = _dead(cache)
        rows = table[i].to(cache.device)[j[:n] // PAGE].long() * PAGE + j[:n] % PAGE
        pool[rows, 0] = cache[i, :n]
    return pool, gathered


def _bits(t):
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------- 1. decode attention through the table

TABLE = ((5, 2, 7), (3, 8, 0), (6, 0, 0), (0, 0, 0))
LENS = ((513, 257, 255, 0), (512, 256, 256, 0))
WINDOWS = (0, 100, 300)


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("r", [1, 2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_paged_decode_is_bitwise_the_gathered_cache(dtype, hd, r, fp8):
    """b = 4, three pages per row (sk = 768) in a pool of 9, tables neither
    sorted nor contiguous, lengths that end one past, on and one before a page
    edge and an empty row; every pool row that no (table, kv_len) makes visible
    holds NaN.  Keys per wave 8 / 16 / 64, windows 0 / 100 (edge inside a page)
    / 300 (across one): bitwise the unpaged call on the gathered cache."""
    torch.manual_seed(hd + r)
    b, sk, nq = 4, 3 * PAGE, NKV * r
    q = torch.randn(b, 1, nq, hd, device=DEV).to(dtype)
    k, v = (torch.randn(b, sk, NKV, hd, device=DEV) for _ in range(2))
    sc = None
    if fp8:
        sc = torch.tensor([[2.0 ** -3, 2.0 ** -2], [2.0 ** -2, 2.0 ** -4]], device=DEV)
        k, v = ((t * 8).to(torch.float8_e4m3fn).view(torch.uint8) for t in (k, v))
        assert not bool(((k & 0x7f) == 0x7f).any() | ((v & 0x7f) == 0x7f).any())
    else:
        k, v = k.to(dtype), v.to(dtype)
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for lens in LENS:
            (pk, gk), (pv, gv) = (_paginate(t, table, lens, 9) for t in (k, v))
            kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
            for w in WINDOWS:
                for kpw in (8, 16, 64):
                    want = _call(q, gk, gv, sc, kv_len, w, kpw)
                    got = _call(q, pk.transpose(0, 1), pv.transpose(0, 1), sc, kv_len, w, kpw,
                                table=table, sk=sk)
                    what = f"lens={lens} w={w} kpw={kpw}"
                    assert not bool(want.isnan().any()), what
                    assert torch.equal(_bits(got), _bits(want)), what
                    assert not bool(got[3].any()) and bool(got[:3].any()), what


# ---------------------------------------------------------------- 2. the test sees the table

def _edge_pool(x, t, table, lens, n_pages=9):
    """The edge inputs' physical cache ``[cap + 8, b + 1, nkv, hd]`` as a pool."""
    from test_attention_edges_gpu import _store
    return _paginate(_store(x, t)[:x.cap, 1:].transpose(0, 1).contiguous(), table, lens, n_pages)[0]


def test_swapped_table_entries_move_the_needle():
    """Needle inputs (all weight on one key) at n = 600, window 256 over the
    tables [5, 2, 7] and [3, 8, 1]: every visible target gives its V row bit
    for bit; with the first two entries of row 0's table swapped the window's
    keys 344 .. 511 come from the other page (a needle finds its key wherever
    it lies among the visible ones, so the swap must change which are visible):
    row 0 changes and fails the check, row 1 does not move."""
    W = 256
    x = E.decode_inputs(torch.bfloat16, 128, 4, False, 600, DEV)
    ci = x.cases.index((600, W))
    assert {344, 511} <= set(x.targets[ci, 0].tolist())
    table = torch.tensor([[5, 2, 7], [3, 8, 1]], dtype=torch.int32, device=DEV)
    lens = (600, 600)
    pk, pv = (_edge_pool(x, t, table, lens).transpose(0, 1) for t in (x.k, x.v_needle))
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    qn = x.q_needle[ci].unsqueeze(1)
    y = types.SimpleNamespace(needle_e=x.needle_e[ci][None], needle_ref=x.needle_ref[ci][None],
                              t_visible=x.t_visible[ci][None])
    assert bool(x.t_visible[ci, 0].any())
    for kpw in (8, 16, 64):
        o = _call(qn, pk, pv, None, kv_len, W, kpw, table=table, sk=x.cap)
        assert bool(E.needle_ok(o[None], y).all()), kpw
        swapped = table.clone()
        swapped[0, 0], swapped[0, 1] = table[0, 1], table[0, 0]
        o2 = _call(qn, pk, pv, None, kv_len, W, kpw, table=swapped, sk=x.cap)
        assert not torch.equal(_bits(o2[0]), _bits(o[0])), kpw
        assert torch.equal(_bits(o2[1]), _bits(o[1])), kpw
        assert not bool(E.needle_ok(o2[None], y).all()), kpw


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
def test_census_over_a_table_counts_kv_len_keys(fp8):
    """Q = 0: the output is (visible keys per column) / (visible keys), so a
    row of ``kv_len`` keys must count exactly those, page by page."""
    x = E.decode_inputs(torch.float16, 64, 2, fp8, 600, DEV)
    sc = torch.stack([x.k_scale, x.v_scale]).float().contiguous() if fp8 else None
    table = torch.tensor([[5, 2, 7], [3, 8, 1]], dtype=torch.int32, device=DEV)
    for lens in ((513, 257), (255, 600), (256, 512)):
        ci = [x.cases.index((n, 0)) for n in lens]
        want = torch.stack([x.census_e[c, i] for i, c in enumerate(ci)])
        pk, pv = (_edge_pool(x, t, table, lens).transpose(0, 1) for t in (x.k, x.v_census))
        kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
        for kpw in (8, 16, 64):
            o = _call(x.q_census, pk, pv, sc, kv_len, 0, kpw, table=table, sk=x.cap)
            assert bool(E.census_ok(o[None], want[None]).all()), (lens, kpw)


# ---------------------------------------------------------------- 3. the tail

class _TailState:
    """b = 3: row 0 (pages 4, 1) at position 254, row 1 (page 2) at position 10,
    row 2 idle on the null page."""

    def __init__(self, dev, top_k, stop_id):
        L = torch.long
        self.table = torch.tensor([[4, 1], [2, 0], [0, 0]], dtype=torch.int32, device=dev)
        self.tokens = torch.full((3,), -7, dtype=L, device=dev)
        self.history = torch.full((3, 6), -7, dtype=L, device=dev)
        self.hist_idx = torch.zeros(3, dtype=L, device=dev)
        self.pos = torch.tensor([254, 10, 0], dtype=L, device=dev)
        self.slot = torch.tensor([4 * PAGE + 254, 2 * PAGE + 10, 0], dtype=L, device=dev)
        self.kv_len = torch.tensor([255, 11, 0], dtype=torch.int32, device=dev)
        self.active = torch.tensor([1, 1, 0], dtype=torch.int32, device=dev)
        self.limit = torch.full((3,), 6, dtype=L, device=dev)
        self.tick = torch.zeros(1, dtype=L, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ctl = torch.tensor([1234, 40, top_k, 0, stop_id, -1], dtype=L, device=dev)
        self.fctl = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)

    def fields(self):
        return (self.tokens, self.history, self.hist_idx, self.pos, self.slot, self.kv_len,
                self.active, self.limit, self.tick)


@pytest.mark.parametrize("stop_step", [None, 1], ids=["runs-on", "parks-at-the-crossing"])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "top_k_1"])
def test_ragged_tail_follows_the_table(sample, stop_step):
    """Four replays against ``ragged_tail_reference`` with the table: row 0's
    slots are 4 * 256 + 255, 1 * 256 + 0, 1 * 256 + 1, ...; with the stop id
    planted in the second replay row 0 parks on the last row of page 4."""
    from epfl_megatron_amd.inference.continuous import ragged_tail_reference
    stop = 300
    st, ref = (_TailState(d, 1 if sample else 0, stop) for d in (DEV, "cpu"))
    slots = []
    for step in range(4):
        torch.manual_seed(50 + step)
        logits = (torch.randn(3, 512, device=DEV) * 3).to(torch.bfloat16)
        logits[:, 300] = -50.0
        if step == stop_step:
            logits[0, stop] = 60.0
        _ext().ragged_tail(logits, *st.fields(), st.counter, st.ctl, st.fctl, sample,
                           page_table=st.table, n_pages=5)
        ragged_tail_reference(logits.float().argmax(1).cpu(), *ref.fields(), ref.ctl, ref.table, 5)
        for name, a, e in zip(("tokens", "history", "hist_idx", "pos", "slot", "kv_len", "active",
                               "limit", "tick"), st.fields(), ref.fields()):
            assert torch.equal(a.cpu(), e), (step, name, a.tolist(), e.tolist())
        assert int(st.ctl[5]) == int(ref.ctl[5]) and int(st.counter) == 0
        slots.append(int(st.slot[0]))
    if stop_step is None:
        assert slots == [4 * PAGE + 255, PAGE, PAGE + 1, PAGE + 2]
        assert st.slot.tolist() == [PAGE + 2, 2 * PAGE + 14, 0]
    else:
        assert slots == [4 * PAGE + 255] * 4 and st.active.tolist() == [0, 1, 0]
        assert st.kv_len.tolist() == [256, 15, 0]


# ---------------------------------------------------------------- 4. writers over a stride-0 pool

SENT16, SENT8 = -1.5, 0xA5
POOL_PAGES = 4


def _phys_slots(M):
    """Distinct pool rows over four pages: page edges first, then a stride
    coprime with the pool size."""
    slots = [255, 256, 1023] + [(211 * m + 7) % (POOL_PAGES * PAGE) for m in range(3, M)]
    assert len(set(slots)) == M and len({s // PAGE for s in slots}) >= min(M, 3)
    return slots


def _untouched(pool, st, sent):
    keep = torch.ones(pool.shape[0], dtype=torch.bool, device=DEV)
    keep[st] = False
    return bool((pool[keep] == sent).all()) and bool((pool[~keep] != sent).any())


@pytest.mark.parametrize("form", ["rowmajor", "packed", "fp8w", "mxfp4"])
@pytest.mark.parametrize("K,ng", [(512, 2), (4096, 1)], ids=["per-block", "persistent"])
@pytest.mark.parametrize("M", [3, 16, 24])
def test_qkv_epilogue_writes_the_pool(M, K, ng, form):
    """``skinny_qkv_rope_cache`` with the pool expanded over the batch (batch
    stride 0) and physical per-row slots: row m's K / V at pool row slot[m] are
    bitwise what the per-column call writes at (slot[m], m), q is bitwise the
    same, every other pool byte keeps its sentinel."""
    from epfl_megatron_amd.ops.rope import rope_table
    from test_continuous_gpu import _qkv_weights
    C = _ext()
    r, hd, L = 2, 128, POOL_PAGES * PAGE
    N = ng * (r + 2) * hd
    slots = _phys_slots(M)
    st = torch.tensor(slots, device=DEV)
    rows = torch.arange(M, device=DEV)
    cos, sin = rope_table(hd, 64, DEV)
    pos = (torch.arange(M, device=DEV).view(M, 1) * 3 + 2) % 64
    sc = torch.ldexp(torch.ones(2, ng), torch.arange(2 * ng).view(2, ng) - 6.0).to(DEV)
    for dt, normed in [(dt, nm) for dt in (torch.bfloat16, torch.float16)
                       for nm in ((True, False) if M <= 16 else (False,))]:
        w, packed, wsc = _qkv_weights(form, N, K, dt, 10 * M + K)
        torch.manual_seed(M)
        x = torch.randn(M, K, device=DEV, dtype=dt)
        g = (torch.rand(K, device=DEV) + 0.5).to(dt) if normed else None
        for kv8 in (False, True):
            def fresh(B):
                if kv8:
                    return torch.full((L, B, ng, hd), SENT8, device=DEV, dtype=torch.uint8)
                return torch.full((L, B, ng, hd), SENT16, device=DEV, dtype=dt)
            tail = (packed, wsc) + ((sc,) if kv8 else ())
            args = (x, w, g, 1e-5, ng, r, hd, cos, sin, pos)
            what = f"{form} {dt} normed={normed} kv8={kv8}"
            with torch.no_grad():
                kr, vr = fresh(M), fresh(M)
                q = C.skinny_qkv_rope_cache(*args, kr, vr, st, 0, *tail)
                kp, vp = fresh(1), fresh(1)
                qp = C.skinny_qkv_rope_cache(*args, kp.expand(-1, M, -1, -1),
                                             vp.expand(-1, M, -1, -1), st, 0, *tail)
            assert torch.equal(_bits(qp), _bits(q)), what + " q"
            assert torch.equal(_bits(kp[st, 0]), _bits(kr[st, rows])), what + " k"
            assert torch.equal(_bits(vp[st, 0]), _bits(vr[st, rows])), what + " v"
            sent = SENT8 if kv8 else SENT16
            assert _untouched(kp[:, 0], st, sent) and _untouched(vp[:, 0], st, sent), what


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("b", [3, 24])
def test_kv_store_fp8_writes_the_pool(b, dt):
    from epfl_megatron_amd.ops import fp8_kv
    nkv, r, hd, L = 2, 2, 128, POOL_PAGES * PAGE
    torch.manual_seed(b)
    mixed = (torch.randn(1, b, nkv, r + 2, hd, device=DEV) * 30).to(dt)
    k, v = mixed[:, :, :, r], mixed[:, :, :, r + 1]
    sc = torch.ldexp(torch.ones(2, nkv), torch.arange(2 * nkv).view(2, nkv) - 3.0).to(DEV)
    st = torch.tensor(_phys_slots(b), device=DEV)
    rows = torch.arange(b, device=DEV)
    k8, v8 = (torch.full((L, b, nkv, hd), SENT8, device=DEV, dtype=torch.uint8) for _ in range(2))
    fp8_kv.store(k, v, k8, v8, sc, slot_t=st)
    kp, vp = (torch.full((L, 1, nkv, hd), SENT8, device=DEV, dtype=torch.uint8) for _ in range(2))
    fp8_kv.store(k, v, kp.expand(-1, b, -1, -1), vp.expand(-1, b, -1, -1), sc, slot_t=st)
    assert torch.equal(kp[st, 0], k8[st, rows]) and torch.equal(vp[st, 0], v8[st, rows])
    assert torch.equal(kp[st, 0], fp8_kv.quantize(k[0], sc[0]))
    assert _untouched(kp[:, 0], st, SENT8) and _untouched(vp[:, 0], st, SENT8)


# ---------------------------------------------------------------- 5 / 6. the decoders and the batcher

def _model(extra=()):
    """The tiny GQA Llama of test_continuous_gpu.py, its rotary table long
    enough for the 768-slot cache."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA
    from test_parallel_equivalence import _deterministic_init
    init_framework(LLAMA_GQA + ["--bf16", "--max_position_embeddings", "800"] + list(extra),
                   finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, get_args())
    return model[0].eval()


def _prefill(m, ip, row, prompt):
    saved = ip.device_offset, ip.device_kv_len
    ip.device_offset = ip.device_kv_len = None
    ip.sequence_len_offset, ip.batch_size_offset = 0, row
    with torch.no_grad():
        out = m(prompt[None], torch.arange(prompt.numel(), device=DEV)[None], None,
                inference_params=ip)
    ip.batch_size_offset = 0
    ip.device_offset, ip.device_kv_len = saved
    return int(out[0, -1].argmax())


def _end_to_end(rank, world, extra):
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m = _model(extra)
    prompts = request_prompts(512)
    out = {}

    def serve(kv_pages):
        ip = InferenceParams(4, CAP, kv_pages=kv_pages)
        cb = ContinuousBatcher(m, ip, 4, CAP, poll_every=1, max_new_tokens=32)
        for p, (_, mn) in zip(prompts, REQUESTS):
            cb.submit(p, mn)
        return cb.run(), cb
    out["unpaged"], _ = serve(None)
    out["paged"], cb = serve(8)
    out["cb"] = (cb.waits, cb.page_log, cb.pool.peak, cb.pool.in_use, cb.dec.captures)
    out["cache"] = (cb.ip.key_value_memory_dict[1][0].dtype,
                    tuple(cb.ip.key_value_memory_dict[1][0].shape))
    # rows primed identically: the step logits of the paged and the unpaged decoder
    pages = ([5, 2], [3], [7, 1], [6, 4])
    n = 8
    runs = []
    for paged in (False, True):
        ip = InferenceParams(4, CAP, kv_pages=8 if paged else None)
        dec = RaggedGreedyDecoder(m, ip, 4, n)
        first = []
        for row in range(4):
            if paged:
                dec.write_table(row, pages[row], REQUESTS[row][0] + n)
            first.append(_prefill(m, ip, row, prompts[row].to(DEV)))
        for row in range(4):
            dec.prime(row, first[row], REQUESTS[row][0], n)
        logits = []
        for _ in range(n):
            dec.step()
            logits.append(dec.logits[:, -1].clone())
        runs.append((first, dec.history.cpu(), torch.stack(logits).cpu(), dec.slot.tolist(),
                     dec.captures))
    out["first"] = runs[0][0] == runs[1][0]
    out["hist"] = torch.equal(runs[0][1], runs[1][1])
    out["logits"] = [torch.equal(_bits(runs[0][2][s]), _bits(runs[1][2][s])) for s in range(n)]
    out["slots"] = runs[1][3]
    out["captures"] = (runs[0][4], runs[1][4])
    return out


@pytest.mark.parametrize("extra", [(), ("--inference_fp8_kv_cache",)], ids=["kv16", "kv8"])
def test_paged_batcher_matches_unpaged_on_one_graph(extra):
    """Batch 4, capacity 768, six requests of which several cross a page while
    generating, 8 pages (7 usable) where the unpaged cache holds 12 pages'
    worth: some admission waits, a page is reused, every request's tokens are
    the unpaged batcher's, and identically primed rows give bitwise the same
    step logits, all on one captured graph per decoder."""
    r = run_dist(_end_to_end, 1, list(extra), env={"EMA_DECODE_FUSED": "1"})[0]
    assert [len(t) for t in r["unpaged"]] == [mn for _, mn in REQUESTS]
    assert r["paged"] == r["unpaged"]
    waits, page_log, peak, in_use, captures = r["cb"]
    handed = [p for _, _, pages in page_log for p in pages]
    assert waits >= 1 and len(set(handed)) < len(handed) and 0 not in handed
    assert peak == 7 and in_use == 0 and captures == 1
    assert r["cache"] == (torch.uint8 if extra else torch.bfloat16, (8 * PAGE, 1, 2, 128))
    assert r["first"] and r["hist"] and all(r["logits"]), r
    # rows 0 (250 + 7) and 3 (254 + 7) crossed into their second pages
    assert r["slots"][0] // PAGE == 2 and r["slots"][3] // PAGE == 4 and r["captures"] == (1, 1)


def _released(rank, world):
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m = _model()
    prompts = request_prompts(512)
    a, b = (prompts[0], 12), (prompts[2], 14)   # 250 + 12 and 300 + 14 keys: two pages each
    out = {}
    cb = ContinuousBatcher(m, InferenceParams(2, CAP, kv_pages=3), 2, CAP, poll_every=1,
                           max_new_tokens=32)
    seen, prime = [], cb.dec.prime

    def spy(row, *args, **kw):
        seen.append((row, cb.dec.slot.tolist(), cb.dec.kv_len.tolist(),
                     cb.ip.page_table.tolist(), cb.replays))
        prime(row, *args, **kw)
    cb.dec.prime = spy
    cb.submit(*a)
    cb.submit(*b)
    out["tokens"] = cb.run()
    out["seen"], out["log"], out["replays"] = seen, cb.page_log, cb.replays
    out["waits"], out["captures"] = cb.waits, cb.dec.captures
    solo = ContinuousBatcher(m, InferenceParams(2, CAP), 2, CAP, poll_every=1, max_new_tokens=32)
    solo.submit(*b)
    out["solo"] = solo.run()[0]
    return out


def test_released_row_idles_on_the_null_page():
    """Batch 2, two usable pages.  A (two pages) runs in row 0; B can only enter
    once A's pages are free and goes to row 1, into A's former pages, while row
    0 sits idle for all of B's replays.  Had row 0 kept A's last slot (key 260
    of page 2) it would overwrite B's key 260 on every replay."""
    r = run_dist(_released, 1)[0]
    (rid_a, row_a, pages_a), (rid_b, row_b, pages_b) = r["log"]
    assert (rid_a, row_a, rid_b, row_b) == (0, 0, 1, 1) and pages_a == pages_b == [1, 2]
    assert r["waits"] >= 1 and r["captures"] == 1
    (_, _, _, _, _), (row, slot, kv_len, table, replays_at_b) = r["seen"]
    assert row == 1 and slot[0] == 0 and kv_len[0] == 0 and table[0] == [0, 0, 0]
    assert r["replays"] - replays_at_b >= 8
    assert len(r["tokens"][1]) == 14 and r["tokens"][1] == r["solo"]


# ---------------------------------------------------------------- 7. binding checks

def test_binding_checks_name_the_argument():
    dt, hd, r = torch.bfloat16, 64, 2
    q = torch.zeros(4, 1, NKV * r, hd, device=DEV, dtype=dt)
    pool = torch.zeros(9 * PAGE, 1, NKV, hd, device=DEV, dtype=dt)
    pk = pv = pool.transpose(0, 1)
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    kv_len = torch.tensor(LENS[0], dtype=torch.int32, device=DEV)
    ok = dict(table=table, sk=3 * PAGE)
    _call(q, pk, pv, None, kv_len, 0, 16, **ok)
    with pytest.raises(RuntimeError, match="page_table must be an int32"):
        _call(q, pk, pv, None, kv_len, 0, 16, table=table.long(), sk=3 * PAGE)
    with pytest.raises(RuntimeError, match="page_table must be on q's device"):
        _call(q, pk, pv, None, kv_len, 0, 16, table=table.cpu(), sk=3 * PAGE)
    with pytest.raises(RuntimeError, match="page_table must be 2-D contiguous"):
        _call(q, pk, pv, None, kv_len, 0, 16, table=table[:2], sk=3 * PAGE)
    with pytest.raises(RuntimeError, match="sk exceeds the page_table"):
        _call(q, pk, pv, None, kv_len, 0, 16, table=table, sk=3 * PAGE + 1)
    short = pool[:9 * PAGE - 1].transpose(0, 1)
    with pytest.raises(RuntimeError, match="pool must hold n_pages"):
        _call(q, short, short, None, kv_len, 0, 16, **ok)
    with pytest.raises(RuntimeError, match="page_table needs kv_len"):
        _call(q, pk, pv, None, None, 0, 16, **ok)
