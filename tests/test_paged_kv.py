"""Paged KV cache on the CPU (gloo, fp32 tiny model, ``capture=False``): the
page allocator, the torch transcription of the paged ragged tail, the gathered
reference of the paged decode attention, the paged ``ContinuousBatcher``
against the unpaged one through the eager path, its admission order under a
short pool, the order of ``release`` and ``free``, and the cases a paged cache
refuses.  The kernels and the captured graph are covered by
``test_paged_kv_gpu.py``."""
import pytest
import torch

from dist_utils import run_dist
from test_inference import _argv, _setup

CAP = 768
# the request list of the end-to-end tests (prompt length, new tokens): the
# requests take 2 / 1 / 2 / 2 / 1 / 3 pages, so four rows fill the 7 usable
# pages of an 8-page pool, request 4 reuses the page of request 1 and request
# 5 has to wait for three pages; 250 / 254 / 500 cross a page while generating
REQUESTS = ((250, 16), (40, 12), (300, 20), (254, 14), (12, 12), (500, 18))


def request_prompts(vocab, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n, _ in REQUESTS]


# ---------------------------------------------------------------- the allocator

def test_page_pool():
    from epfl_megatron_amd.inference.paged import KV_PAGE, PagePool, pages_for
    assert KV_PAGE == 256
    assert [pages_for(n) for n in (1, 256, 257, 512, 513)] == [1, 1, 2, 2, 3]
    pool = PagePool(5)
    assert pool.available == 4
    a = pool.alloc(3)
    assert a == [1, 2, 3] and pool.in_use == 3   # page 0 is never handed out
    assert pool.alloc(2) is None and pool.available == 1  # short: nothing taken
    b = pool.alloc(1)
    assert b == [4] and pool.alloc(1) is None and pool.alloc(0) == []
    pool.free(a[:2])
    assert pool.available == 2 and pool.peak == 4
    with pytest.raises(ValueError, match="double free"):
        pool.free([1])
    with pytest.raises(ValueError, match="null page"):
        pool.free([0])
    with pytest.raises(ValueError):
        pool.free([3, 3])
    assert pool.in_use == 2                       # a refused free returns nothing
    with pytest.raises(ValueError):
        pool.free([7])
    assert sorted(pool.alloc(2)) == [1, 2]         # freed pages are handed out again
    with pytest.raises(ValueError):
        PagePool(1)


# ---------------------------------------------------------------- the tail's transcription

def test_ragged_tail_reference_with_table_at_the_page_crossing():
    """Rows 0 (pages 4, 1; position 254) and 1 (pages 2, -; position 10) and an
    idle row 2: the slot follows the table over the page edge, a row that parks
    at the crossing keeps the last slot of its first page."""
    from epfl_megatron_amd.inference.continuous import ragged_tail_reference
    L = torch.long
    table = torch.tensor([[4, 1], [2, 0], [0, 0]], dtype=torch.int32)
    for stop_at in (None, 1):
        tokens, history = torch.zeros(3, dtype=L), torch.full((3, 6), -7, dtype=L)
        hist_idx = torch.zeros(3, dtype=L)
        pos = torch.tensor([254, 10, 0], dtype=L)
        slot = torch.tensor([4 * 256 + 254, 2 * 256 + 10, 0], dtype=L)
        kv_len = torch.tensor([255, 11, 0], dtype=torch.int32)
        active = torch.tensor([1, 1, 0], dtype=torch.int32)
        limit, tick = torch.full((3,), 6, dtype=L), torch.zeros(1, dtype=L)
        ctl = torch.tensor([0, 0, 0, 0, 99, -1], dtype=L)
        st = (tokens, history, hist_idx, pos, slot, kv_len, active, limit, tick, ctl)
        slots = []
        for step in range(4):
            tok = torch.tensor([99 if step == stop_at else 5, 6, 7])
            ragged_tail_reference(tok, *st, table, 5)
            slots.append(slot.tolist())
        if stop_at is None:
            assert [s[0] for s in slots] == [4 * 256 + 255, 256, 257, 258]
            assert pos.tolist() == [258, 14, 0] and kv_len.tolist() == [259, 15, 0]
        else:  # parked on the step that would have crossed: the slot stays in page 4
            assert [s[0] for s in slots] == [4 * 256 + 255] * 4 and active.tolist() == [0, 1, 0]
            assert pos.tolist() == [255, 14, 0] and kv_len.tolist() == [256, 15, 0]
        assert [s[1] for s in slots] == [2 * 256 + 11 + i for i in range(4)]
        assert [s[2] for s in slots] == [0] * 4
    # an entry outside the pool is clamped as the kernel clamps it
    bad = torch.tensor([[4, 9], [2, 0], [0, 0]], dtype=torch.int32)
    pos, slot = torch.tensor([255, 0, 0], dtype=L), torch.zeros(3, dtype=L)
    ragged_tail_reference(torch.tensor([5, 6, 7]), torch.zeros(3, dtype=L),
                          torch.zeros(3, 2, dtype=L), torch.zeros(3, dtype=L), pos, slot,
                          torch.zeros(3, dtype=torch.int32),
                          torch.tensor([1, 0, 0], dtype=torch.int32), torch.full((3,), 6, dtype=L),
                          torch.zeros(1, dtype=L), torch.tensor([0, 0, 0, 0, -1, -1], dtype=L), bad, 5)
    assert slot.tolist() == [4 * 256, 0, 0]


# ---------------------------------------------------------------- the gathered attention reference

@pytest.mark.parametrize("window", [0, 100, 300])
def test_flash_decode_cached_paged_reference(window):
    """Off the GPU the paged call gathers each row's pages: equal to the
    per-row call on the gathered contiguous cache, NaN pages never read."""
    from epfl_megatron_amd.inference.paged import KV_PAGE
    from epfl_megatron_amd.ops.attention import flash_decode_cached
    torch.manual_seed(0)
    b, nq, nkv, hd, n_pages = 4, 4, 2, 16, 9
    table = torch.tensor([[5, 2, 7], [3, 8, 0], [6, 0, 0], [0, 0, 0]], dtype=torch.int32)
    lens = [513, 257, 255, 0]
    cap = 3 * KV_PAGE
    q = torch.randn(b, 1, nq, hd)
    k, v = torch.randn(b, cap, nkv, hd), torch.randn(b, cap, nkv, hd)
    pk = torch.full((n_pages * KV_PAGE, 1, nkv, hd), float("nan"))
    pv = pk.clone()
    for i, n in enumerate(lens):
        k[i, n:], v[i, n:] = float("nan"), float("nan")
        for j in range(n):
            row = int(table[i, j // KV_PAGE]) * KV_PAGE + j % KV_PAGE
            pk[row, 0], pv[row, 0] = k[i, j], v[i, j]
    kv_len = torch.tensor(lens, dtype=torch.int32)
    want = flash_decode_cached(q, k, v, kv_len, window=window)
    got = flash_decode_cached(q, pk.transpose(0, 1), pv.transpose(0, 1), kv_len, window=window,
                              page_table=table, capacity=cap)
    assert torch.equal(got, want) and not got[3].any() and not got.isnan().any()
    with pytest.raises(ValueError, match="kv_len"):
        flash_decode_cached(q, pk.transpose(0, 1), pv.transpose(0, 1), None, page_table=table)
    with pytest.raises(ValueError, match="capacity"):
        flash_decode_cached(q, pk.transpose(0, 1), pv.transpose(0, 1), kv_len, page_table=table,
                            capacity=cap + 1)


# ---------------------------------------------------------------- the batcher through the eager path

def _serve(model, prompts, kv_pages, batch, fp8=False, requests=REQUESTS, record=None):
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.models import transformer
    transformer.set_fp8_kv_cache(fp8)
    try:
        ip = InferenceParams(batch, CAP, kv_pages=kv_pages)
        cb = ContinuousBatcher(model, ip, batch, CAP, poll_every=1, max_new_tokens=32,
                               capture=False)
        if record is not None:
            release, free = cb.dec.release, cb.pool.free

            def rel(row):
                record.append(("release", row, list(cb.row_pages[row] or [])))
                release(row)

            def fr(pages):
                record.append(("free", list(pages)))
                free(pages)
            cb.dec.release, cb.pool.free = rel, fr
        for p, (_, mn) in zip(prompts, requests):
            cb.submit(p, mn)
        return cb.run(), cb
    finally:
        transformer.set_fp8_kv_cache(False)


def _cpu_run(rank, world):
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedDecodeForward
    from epfl_megatron_amd.models import transformer
    model = _setup(_argv(["--max_position_embeddings", "800"]))
    prompts = request_prompts(250)
    out = {}
    record = []
    out["unpaged"], _ = _serve(model, prompts, None, 4)
    out["paged"], cb = _serve(model, prompts, 8, 4, record=record)
    out["record"] = record
    out["page_log"], out["waits"], out["peak"] = cb.page_log, cb.waits, cb.pool.peak
    out["after"] = (cb.pool.in_use, cb.ip.page_table.tolist(), cb.dec.slot.tolist(),
                    cb.dec.kv_len.tolist(), cb.dec.captures)
    out["pool_shape"] = tuple(cb.ip.key_value_memory_dict[1][0].shape)
    out["unpaged8"], _ = _serve(model, prompts, None, 4, fp8=True)
    out["paged8"], cb8 = _serve(model, prompts, 8, 4, fp8=True)
    out["pool8_dtype"] = cb8.ip.key_value_memory_dict[1][0].dtype
    # a short pool: 3 usable pages, two rows, requests of 2 / 2 / 1 / 3 pages (request
    # 2 outlives request 1, so request 3 finds the pool short as well)
    short = ((250, 16), (300, 12), (12, 20), (500, 18))
    sp = [prompts[0], prompts[2], prompts[4], prompts[5]]
    out["short_unpaged"], _ = _serve(model, sp, None, 2, requests=short)
    out["short_paged"], cbs = _serve(model, sp, 4, 2, requests=short)
    out["short_log"], out["short_waits"] = cbs.page_log, cbs.waits
    # submit rejections
    errs = {}
    cb = ContinuousBatcher(model, InferenceParams(2, CAP, kv_pages=3), 2, CAP, capture=False)
    for name, args in (("fits", ([1] * 500, 12)), ("pool", ([1] * 500, 13))):
        try:
            cb.submit(*args)
            errs[name] = None
        except ValueError as e:
            errs[name] = str(e)
    cb = ContinuousBatcher(model, InferenceParams(2, CAP, kv_pages=8), 2, 300, capture=False)
    cb.ip.page_table = cb.ip.page_table[:, :1].contiguous()  # a table of one page per row
    try:
        cb.submit([1] * 250, 12)
        errs["row"] = None
    except ValueError as e:
        errs["row"] = str(e)
    out["errs"] = errs

    # the cases a paged cache refuses
    def refused(fn):
        try:
            fn()
            return None
        except NotImplementedError as e:
            return str(e)
    ni = {}
    tok = torch.tensor([[3, 4, 5]])

    def call(ip, t):
        with torch.no_grad():
            return model(t, torch.arange(t.shape[1])[None].expand(t.shape[0], -1), None,
                         inference_params=ip)
    ip = InferenceParams(2, CAP, kv_pages=4)
    ip.page_table[0, 0] = 1
    call(ip, tok)  # the supported prefill
    ip.sequence_len_offset = 3
    ni["continue"] = refused(lambda: call(ip, tok))
    ni["eager_step"] = refused(lambda: call(ip, tok[:, :1]))
    ip.sequence_len_offset = 0
    ni["batch"] = refused(lambda: call(ip, tok.expand(2, -1)))
    ni["swap"] = refused(lambda: ip.swap_key_value_dict([1, 0]))
    ni["lockstep"] = refused(lambda: GraphedDecodeForward(model, ip, 2, capture=False))
    transformer.set_fp8_kv_cache(True, calibrate=True)
    try:
        ipc = InferenceParams(2, CAP, kv_pages=4)
        ipc.page_table[0, 0] = 1
        ni["calibrate"] = refused(lambda: call(ipc, tok))
    finally:
        transformer.set_fp8_kv_cache(False, calibrate=False)
    out["refused"] = ni
    # prime / release on the eager decoder
    ipd = InferenceParams(3, CAP, kv_pages=6)
    dec = RaggedGreedyDecoder(model, ipd, 3, 8, capture=False)
    dec.prime(0, 7, 254, 8, pages=[4, 1])
    dec.prime(1, 7, 10, 8, pages=[2])
    st = [dec.slot.tolist(), dec.kv_len.tolist(), ipd.page_table.tolist()]
    dec.release(0)
    st += [dec.slot.tolist(), dec.kv_len.tolist(), dec.active.tolist(), ipd.page_table.tolist()]
    bad = []
    for pages in ([0, 1], [6], [1]):  # the null page, outside the pool, too few for 262 keys
        try:
            dec.prime(0, 7, 254, 8, pages=pages)
            bad.append(None)
        except ValueError as e:
            bad.append(str(e))
    out["prime"] = st, bad
    return out


@pytest.fixture(scope="module")
def cpu_run():
    return run_dist(_cpu_run, 1)[0]


def test_paged_batcher_matches_unpaged(cpu_run):
    """The item-5 request list, batch 4, capacity 768: 8 pages (7 usable) against
    the 12 columns' worth of the unpaged cache; 16-bit and FP8 caches."""
    r = cpu_run
    assert [len(t) for t in r["unpaged"]] == [mn for _, mn in REQUESTS]
    assert r["paged"] == r["unpaged"]
    assert r["paged8"] == r["unpaged8"] and r["pool8_dtype"] == torch.uint8
    assert r["pool_shape"][:2] == (8 * 256, 1)
    in_use, table, slot, kv_len, captures = r["after"]
    assert in_use == 0 and not any(any(t) for t in table) and slot == [0] * 4 and kv_len == [0] * 4
    assert captures == 0


def test_the_request_list_waits_and_reuses_pages(cpu_run):
    """The property the GPU end-to-end test relies on, checked on this path:
    an admission waits for pages and a page is handed out twice."""
    r = cpu_run
    assert r["waits"] >= 1 and r["peak"] == 7
    handed = [p for _, _, pages in r["page_log"] for p in pages]
    assert len(handed) == 11 and len(set(handed)) < len(handed) and 0 not in handed
    assert [len(pages) for _, _, pages in r["page_log"]] == [2, 1, 2, 2, 1, 3]


def test_admissions_are_fifo_under_a_short_pool(cpu_run):
    """3 usable pages, 2 rows: request 1 (2 pages) waits for request 0's pages
    although request 2 (1 page) would fit: nothing overtakes the head."""
    r = cpu_run
    assert r["short_paged"] == r["short_unpaged"]
    assert [rid for rid, _, _ in r["short_log"]] == [0, 1, 2, 3]
    assert r["short_waits"] >= 2
    assert [rid for rid, _, _ in r["page_log"]] == list(range(len(REQUESTS)))


def test_release_comes_before_free(cpu_run):
    """Every return of pages is preceded, immediately, by the release of the
    row that held exactly those pages."""
    rec = cpu_run["record"]
    frees = [i for i, c in enumerate(rec) if c[0] == "free"]
    assert len(frees) == len(REQUESTS) and len(rec) == 2 * len(frees)
    for i in frees:
        assert i > 0 and rec[i - 1][0] == "release" and rec[i - 1][2] == rec[i][1], rec[i - 1:i + 1]


def test_submit_rejects_what_can_never_be_admitted(cpu_run):
    e = cpu_run["errs"]
    assert e["fits"] is None                      # 512 keys: the pool's two usable pages
    assert e["pool"] is not None and "KV pages" in e["pool"]
    assert e["row"] is not None and "KV pages" in e["row"]


def test_unsupported_cases_raise(cpu_run):
    ni = cpu_run["refused"]
    for case, word in (("continue", "sequence_len_offset"), ("eager_step", "decode step"),
                       ("batch", "more than one row"), ("swap", "swap_key_value_dict"),
                       ("lockstep", "lockstep"), ("calibrate", "inference_fp8_kv_calibrate")):
        assert ni[case] is not None, case
        assert word in ni[case] and "kv_pages=None" in ni[case], (case, ni[case])


def test_prime_and_release(cpu_run):
    (slot, kv_len, table, slot2, kv_len2, active2, table2), bad = cpu_run["prime"]
    assert slot == [4 * 256 + 254, 2 * 256 + 10, 0] and kv_len == [255, 11, 0]
    assert table == [[4, 1, 0], [2, 0, 0], [0, 0, 0]]
    assert slot2 == [0, 2 * 256 + 10, 0] and kv_len2 == [0, 11, 0] and active2 == [0, 1, 0]
    assert table2 == [[0, 0, 0], [2, 0, 0], [0, 0, 0]]
    assert all(b is not None for b in bad), bad
