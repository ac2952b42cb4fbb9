"""Prefix sharing for the paged KV cache on the CPU (gloo, fp32 tiny model,
``capture=False``): the ``PrefixCache`` index, the continued paged prefill of
the model against the unpaged one, and the ``ContinuousBatcher`` with
``prefix_cache`` / ``prefill_chunk`` against the unpaged chunked batcher.  The
paged forms of the attention kernel and the captured graph are covered by
``test_paged_prefill_gpu.py``."""
import pytest
import torch

from dist_utils import run_dist
from test_inference import _argv, _setup

CAP = 768
PREFIX = 512
# (prompt, new tokens) of the end-to-end tests, P a common prefix of 512 tokens:
# P + 20 own tokens registers two pages, P + 30 others hits both, P[:256] + 100
# others hits one, P itself (n = 512) may share only one, a stranger of 40
# tokens, P[:257] shares nothing (and ends on a merged one-token piece), and
# the second request once more
NEW = (12, 16, 20, 14, 12, 18, 10)
WANT_LOG = [(0, 0), (1, 2), (2, 1), (3, 1), (4, 0), (5, 0), (6, 2)]
# what the prefills have to run: the prompts without their shared pages
WANT_PREFILLED = 532 + 30 + 100 + 256 + 40 + 257 + 30
# the short pool of the eviction run: 7 pages, 6 usable (8 pages serve this
# list without an eviction).  Requests 0 - 2 take 3 + 1 + 1 pages, request 3
# waits for the page request 0 frees; when request 5 needs two pages one is
# free, and the second page of P, which requests 0 and 1 no longer read and
# request 3 keeps a private copy of, is evicted for it
SHORT_POOL = 7


def share_prompts(vocab, seed=5):
    g = torch.Generator().manual_seed(seed)

    def rnd(n):
        return torch.randint(0, vocab, (n,), generator=g)
    p = rnd(PREFIX)
    second = torch.cat([p, rnd(30)])
    return [torch.cat([p, rnd(20)]), second, torch.cat([p[:256], rnd(100)]), p.clone(), rnd(40),
            p[:257].clone(), second.clone()]


# ---------------------------------------------------------------- the index

def _ids(*pages, tail=0):
    """A prompt of full pages filled with the given values and ``tail`` more tokens."""
    return torch.cat([torch.full((256,), v) for v in pages] + [torch.full((tail,), 99)])


def test_prefix_cache_index():
    from epfl_megatron_amd.inference.paged import PagePool, PrefixCache
    pool = PagePool(9)
    cache = PrefixCache(pool)
    a = _ids(1, 2, 3, tail=5)
    assert cache.match(a) == []
    pa = pool.alloc(4)
    added = cache.insert(a, pa, 0)
    assert [e.page for e in added] == pa[:3] and all(e.refs == 1 for e in added)
    assert cache.pages() == pa[:3] and len(cache) == 3
    # the chain diverges in the second page
    b = _ids(1, 7, 3, tail=5)
    assert [e.page for e in cache.match(b)] == pa[:1]
    assert [e.page for e in cache.match(a)] == pa[:3]
    assert cache.match(_ids(2, 2, 3, tail=5)) == []
    # the cap: at least two tokens are left to prefill
    full = _ids(1, 2, 3)
    for n, want in ((257, 0), (258, 1), (512, 1), (513, 1), (514, 2)):
        assert len(cache.match(full[:n])) == want == (n - 2) // 256, n
    # insert skips an existing entry: the row keeps its page private
    chain = cache.match(b)
    cache.acquire(chain)
    assert chain[0].refs == 2
    pb = [chain[0].page] + pool.alloc(3)
    added_b = cache.insert(b, pb, 1)
    assert [e.page for e in added_b] == pb[1:3]      # pages (1, 7) and (1, 7, 3): new entries
    pc = pool.alloc(1)                                # the last free page: a second copy of (1)
    assert cache.insert(_ids(1, tail=9), pc, 0) == [] and len(cache) == 5
    with pytest.raises(ValueError, match="not the cached page"):
        cache.insert(b, [pc[0]] + pb[1:], 1)
    pool.free(pc)
    # evict never takes a referenced page
    assert cache.evict(4) == [] and len(cache) == 5 and pool.available == 1
    cache.release(added)                               # row a goes: (1) is still read by row b
    with pytest.raises(ValueError, match="released more often"):
        cache.release(added[1:])
    # leaves before parents, least recently used first: (1, 2, 3), then (1, 2)
    assert cache.evict(1) == [pa[2]] and cache.evict(1) == [pa[1]]
    assert cache.evict(1) == [] and pool.available == 3    # (1) has a reader and children
    cache.release(chain + added_b)
    assert all(e.refs == 0 for e in chain + added_b)
    assert cache.evict(1) == [pb[2]]                       # the leaf (1, 7, 3) first
    # after clear() the pool has everything back but row a's private page
    assert sorted(cache.clear()) == sorted([pa[0], pb[1]]) and len(cache) == 0
    pool.free([pa[3], pb[3]])
    assert pool.in_use == 0 and pool.available == 8


def test_the_batcher_refuses_a_prefix_cache_without_pages():
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    ip = InferenceParams(2, CAP, table_device="cpu")
    with pytest.raises(ValueError, match="paged"):
        ContinuousBatcher(None, ip, 2, CAP, capture=False, prefix_cache=True)
    with pytest.raises(ValueError, match="prefill_chunk"):
        ContinuousBatcher(None, ip, 2, CAP, capture=False, prefill_chunk=1)


# ---------------------------------------------------------------- the model and the batcher

def _two_calls(model, ip, prompt, split, paged):
    def call(a, b):
        ip.sequence_len_offset = a
        ip.continue_prefill = paged and a > 0
        with torch.no_grad():
            return model(prompt[None, a:b], torch.arange(a, b)[None], None, inference_params=ip)
    call(0, split)
    logits = call(split, prompt.numel())
    ip.continue_prefill = False
    return logits[0, -1]


def _continued_prefill(model, fp8):
    """300 tokens as [0, s) + [s, 300), paged (pages 2, 1) against unpaged."""
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import gather_rows
    from epfl_megatron_amd.models import transformer
    transformer.set_fp8_kv_cache(fp8)
    res = {}
    try:
        prompt = torch.randint(0, 250, (300,), generator=torch.Generator().manual_seed(3))
        for split in (256, 255, 2):
            ipu = InferenceParams(1, CAP)
            want = _two_calls(model, ipu, prompt, split, False)
            ipp = InferenceParams(2, CAP, kv_pages=4)
            ipp.page_table[0, :2] = torch.tensor([2, 1], dtype=torch.int32)
            got = _two_calls(model, ipp, prompt, split, True)
            rows = True
            for layer, (ku, vu) in ipu.key_value_memory_dict.items():
                kp, vp = ipp.key_value_memory_dict[layer]
                rows = rows and kp.dtype == ku.dtype and \
                    torch.equal(gather_rows(kp, ipp.page_table[0], 300)[:, 0], ku[:300, 0]) and \
                    torch.equal(gather_rows(vp, ipp.page_table[0], 300)[:, 0], vu[:300, 0])
            res[split] = (torch.equal(got, want), bool(got.isfinite().all()), rows,
                          len(ipu.key_value_memory_dict), ku.dtype)
    finally:
        transformer.set_fp8_kv_cache(False)
    return res


def _serve(model, prompts, kv_pages, fp8=False, record=None, **kw):
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.models import transformer
    transformer.set_fp8_kv_cache(fp8)
    try:
        ip = InferenceParams(4, CAP, kv_pages=kv_pages)
        cb = ContinuousBatcher(model, ip, 4, CAP, poll_every=1, max_new_tokens=32, capture=False,
                               **kw)
        if record is not None:
            release, free, deref = cb.dec.release, cb.pool.free, cb.cache.release

            def rel(row):
                record.append(("release", row, list(cb.row_pages[row] or []),
                               [e.page for e in cb.row_cached[row] or []]))
                release(row)

            def fr(pages):
                record.append(("free", list(pages)))
                free(pages)

            def de(chain):
                record.append(("deref", [e.page for e in chain]))
                deref(chain)
            cb.dec.release, cb.pool.free, cb.cache.release = rel, fr, de
        for p, mn in zip(prompts, NEW):
            cb.submit(p, mn)
        return cb.run(), cb
    finally:
        transformer.set_fp8_kv_cache(False)


def _cpu_run(rank, world):
    model = _setup(_argv(["--max_position_embeddings", "800"]))
    prompts = share_prompts(250)
    out = {"continued": _continued_prefill(model, False), "continued8": _continued_prefill(model, True)}
    for tag, fp8 in (("", False), ("8", True)):
        out["oracle" + tag], _ = _serve(model, prompts, None, fp8, prefill_chunk=256)
        record = []
        out["shared" + tag], cb = _serve(model, prompts, 16, fp8, record=record, prefill_chunk=256,
                                         prefix_cache=True)
        held = cb.cache.pages()
        out["stats" + tag] = (cb.prefix_log, cb.prefilled_tokens, cb.prefix_hit_pages, cb.evictions,
                              cb.pool.in_use, held, cb.ip.page_table.tolist())
        out["record" + tag] = list(record)
        cb.cache.clear()
        out["cleared" + tag] = (cb.pool.in_use, len(cb.cache))
        out["short" + tag], cbs = _serve(model, prompts, SHORT_POOL, fp8, prefill_chunk=256,
                                         prefix_cache=True)
        out["short_stats" + tag] = (cbs.evictions, cbs.waits, cbs.prefix_log, cbs.pool.in_use,
                                    len(cbs.cache))
    out["oracle_prefilled"] = _serve(model, prompts, None, prefill_chunk=256)[1].prefilled_tokens
    out["plain"], _ = _serve(model, prompts, None)
    out["chunk100"], _ = _serve(model, prompts, None, prefill_chunk=100)
    out["chunk100_paged"], cb = _serve(model, prompts, 16, prefill_chunk=100)
    out["chunk100_pool"] = cb.pool.in_use
    out["pieces"] = [cb._pieces(*a) for a in ((0, 257), (0, 301), (256, 512), (200, 201 + 100))]
    cb.prefill_chunk = 257
    out["pieces257"] = cb._pieces(256, 600)
    return out


@pytest.fixture(scope="module")
def cpu_run():
    return run_dist(_cpu_run, 1)[0]


@pytest.mark.parametrize("tag", ["continued", "continued8"])
def test_continued_paged_prefill_equals_the_unpaged_one(cpu_run, tag):
    """Both sides run the same fp32 ops on the same values: the logits of the
    last position are equal, and the pool rows the table names are the
    unpaged column (16-bit and FP8 cache; split points on a page edge, one
    before it, and after two tokens)."""
    for split, (same, finite, rows, layers, dtype) in cpu_run[tag].items():
        assert same and finite and rows and layers >= 1, (split, same, finite, rows)
        assert dtype == (torch.uint8 if tag.endswith("8") else torch.float32)


@pytest.mark.parametrize("tag", ["", "8"])
def test_prefix_sharing_batcher_equals_the_unpaged_chunked_one(cpu_run, tag):
    """Served the same requests, the sharing batcher runs for every request a
    suffix of the oracle's prefill pieces with identical shapes: equal tokens,
    no tolerance."""
    r = cpu_run
    assert [len(t) for t in r["oracle" + tag]] == list(NEW)
    assert r["shared" + tag] == r["oracle" + tag]
    log, prefilled, hits, evictions, in_use, held, table = r["stats" + tag]
    assert log == WANT_LOG
    assert prefilled == WANT_PREFILLED and r["oracle_prefilled"] == WANT_PREFILLED + 6 * 256
    assert hits == 6 and hits >= 5 and evictions == 0
    # what is still out is what the cache holds: the two pages of P
    assert in_use == len(held) == 2 and not any(any(t) for t in table)
    assert r["cleared" + tag] == (0, 0)


@pytest.mark.parametrize("tag", ["", "8"])
def test_a_short_pool_evicts_and_serves_the_same_tokens(cpu_run, tag):
    """SHORT_POOL pages: an admission has to evict cached pages nobody reads."""
    r = cpu_run
    evictions, waits, log, in_use, cached = r["short_stats" + tag]
    assert evictions >= 1
    assert r["short" + tag] == r["oracle" + tag]
    assert [rid for rid, _ in log] == list(range(7)) and in_use == cached


def test_chunked_prefill_gives_the_unchunked_tokens(cpu_run):
    """``prefill_chunk=100``, unpaged and paged, against the unchunked unpaged
    batcher on the fp32 model: the same tokens (checked where this test was
    written: no near-tie among the first tokens of this request list)."""
    r = cpu_run
    assert r["oracle"] == r["plain"]
    assert r["chunk100"] == r["plain"]
    assert r["chunk100_paged"] == r["plain"] and r["chunk100_pool"] == 0
    assert r["pieces"] == [[(0, 100), (100, 200), (200, 257)],
                           [(0, 100), (100, 200), (200, 301)],
                           [(256, 300), (300, 400), (400, 500), (500, 512)],
                           [(200, 301)]]
    assert r["pieces257"] == [(256, 514), (514, 600)]


@pytest.mark.parametrize("tag", ["", "8"])
def test_release_comes_before_pages_are_freed_or_dereferenced(cpu_run, tag):
    """Every finished row: ``release(row)``, then its private pages are freed,
    then its cached pages are dereferenced, and nothing in between."""
    rec = cpu_run["record" + tag]
    rels = [i for i, c in enumerate(rec) if c[0] == "release"]
    assert len(rels) == 7
    seen_deref = 0
    for n, i in enumerate(rels):
        _, row, private, cached = rec[i]
        assert private, rec[i]                         # every row decodes into a page of its own
        assert rec[i + 1] == ("free", private), rec[i:i + 2]
        follow = rec[i + 2:rels[n + 1] if n + 1 < len(rels) else len(rec)]
        assert follow == ([("deref", cached)] if cached else []), rec[i:i + 3]
        seen_deref += bool(cached)
    assert seen_deref == 5 and len(rec) == 2 * 7 + 5  # the stranger and P[:257] hold no cached page
