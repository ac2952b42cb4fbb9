"""Paged prefill on the GPU: the page-table forms of the forward attention
kernel, the continued paged prefill of the model, and the prefix-sharing
``ContinuousBatcher`` on one captured graph.

Paging changes only where a key tile's rows are fetched from: the same forced
form (4-wave, 8-wave, split-key) must give, bit for bit, the output and the
log-sum-exp of the contiguous kernel on the gathered keys.  No tolerance
appears in the kernel tests."""
import pytest
import torch

import attention_edge_inputs as E
from dist_utils import run_dist
from test_paged_kv_gpu import _bits, _model, _paginate
from test_prefix_cache import CAP, NEW, WANT_LOG, WANT_PREFILLED, share_prompts

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAGE = 256
NKV = 2
N_PAGES = 9
TABLE = ((5, 2, 7), (3, 8, 1))
# (keys before the block, queries): one page + 2, + more than a 4-wave block,
# a block that starts one before a page edge, sq == s0 off the page grid, the
# whole-prompt prefill through the table, two full pages + one
SHAPES = ((256, 2), (256, 130), (511, 3), (300, 300), (0, 513), (512, 256))
WINDOWS = (0, 100, 300)


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def _forms(hd):
    """(waves, kv2) of every form the head dim has."""
    return ((4, -1), (8, -1)) + (((0, 1),) if hd == 128 else ())


def _fwd(q, k, v, sk, window=0, waves=0, kv2=-1, table=None, **over):
    """The ``flash_attn_fwd`` binding on ``q [b, sq, nq, hd]`` (the last sq of sk
    positions, causal): k / v ``[b, sk, nkv, hd]``, or with ``table`` the pools
    ``[1, rows, nkv, hd]``.  Returns (out, lse)."""
    from epfl_megatron_amd.ops.attention import _bsnd_strides
    b, sq, nq, d = q.shape
    nkv = k.shape[2]
    out = torch.zeros(b, sq, nq, d, dtype=q.dtype, device=q.device)
    lse = torch.zeros(b, nq, sq, dtype=torch.float32, device=q.device)
    args = dict(q=q, k=k, v=v, out=out, lse=lse, b=b, sq=sq, sk=sk, nq=nq, nkv=nkv, hd=d,
                qs=list(_bsnd_strides(q, nq // nkv)), ks=list(_bsnd_strides(k, 1)[:3]),
                vs=list(_bsnd_strides(v, 1)[:3]), os=[out.stride(0), out.stride(1), out.stride(2)],
                causal=True, scale=d ** -0.5, rope_cos=None, rope_sin=None, rope_pos=None,
                docs=None, window=window, waves=waves, kv2=kv2)
    if table is not None:
        args["page_table"] = table
    args.update(over)
    _ext().flash_attn_fwd(**args)
    return out, lse


def _pools(k, v, table, sk):
    """Pools ``[1, N_PAGES * 256, nkv, hd]`` holding each row's ``sk`` keys at
    the rows ``table`` names, NaN everywhere else."""
    return tuple(_paginate(t, table, (sk,) * t.shape[0], N_PAGES)[0].transpose(0, 1) for t in (k, v))


# ---------------------------------------------------------------- 1. the bitwise twin

@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_paged_forward_is_bitwise_the_gathered_keys(dtype, hd, r):
    """b = 2, tables [5, 2, 7] and [3, 8, 1] in a pool of 9 pages whose other
    rows hold NaN; every shape, window and forced form: output and lse are bit
    for bit those of the same form on the gathered contiguous K / V."""
    torch.manual_seed(hd + r)
    b, nq = 2, NKV * r
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for s0, sq in SHAPES:
        sk = s0 + sq
        q = torch.randn(b, sq, nq, hd, device=DEV).to(dtype)
        k, v = (torch.randn(b, sk, NKV, hd, device=DEV).to(dtype) for _ in range(2))
        pk, pv = _pools(k, v, table, sk)
        assert bool(pk.isnan().any()) or sk == 3 * PAGE
        for w in WINDOWS:
            for waves, kv2 in _forms(hd):
                what = f"s0={s0} sq={sq} w={w} waves={waves} kv2={kv2}"
                want, want_lse = _fwd(q, k, v, sk, w, waves, kv2)
                got, got_lse = _fwd(q, pk, pv, sk, w, waves, kv2, table=table)
                assert not bool(want.isnan().any() | got.isnan().any()), what
                assert not bool(got_lse.isnan().any()), what
                assert torch.equal(_bits(got), _bits(want)), what
                assert torch.equal(_bits(got_lse), _bits(want_lse)), what
                assert bool(got.any()), what


def test_automatic_form_does_not_depend_on_the_table():
    """``waves = 0, kv2 = -1``: the op picks the form from (b, sq, nq, hd) with
    and without a table (``flash_attn_paged`` against ``flash_attn_func`` on
    the gathered keys, the pair the model's two prefill paths run)."""
    from epfl_megatron_amd.ops.attention import flash_attn_func, flash_attn_paged
    torch.manual_seed(3)
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for hd, nq, (s0, sq) in ((128, 8, (256, 130)), (64, 4, (300, 300)), (128, 2, (511, 3))):
        sk = s0 + sq
        q = torch.randn(2, sq, nq, hd, device=DEV).to(torch.bfloat16)
        k, v = (torch.randn(2, sk, NKV, hd, device=DEV).to(torch.bfloat16) for _ in range(2))
        pk, pv = _pools(k, v, table, sk)
        for w in (0, 100):
            with torch.no_grad():
                want = flash_attn_func(q, k, v, causal=True, window=w)
            got = flash_attn_paged(q, pk, pv, table, sk, window=w)
            assert torch.equal(_bits(got), _bits(want)), (hd, nq, s0, sq, w)


# ---------------------------------------------------------------- 2. the test sees the table

@pytest.mark.parametrize("hd", [64, 128])
def test_census_through_a_table_counts_the_visible_keys(hd):
    """Q = 0: the output is (visible keys per column) / (visible keys) and the
    lse is ln(visible keys): row i of the block sees exactly ``s0 + i + 1`` keys
    (or the window), fetched page by page through the table."""
    dtype, nq = torch.float16, 4
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for s0, sq in SHAPES:
        sk = s0 + sq
        q, k, v = (t.to(DEV) for t in E.prefill_census_inputs(2, sq, sk, nq, NKV, hd, dtype))
        pk, pv = _pools(k, v, table, sk)
        for w in WINDOWS:
            vis, _ = E.prefill_visibility(2, sq, sk, True, w if w < sk else 0, None)
            e, count = E.prefill_expected(v, vis, nq)
            i = torch.arange(sq, device=DEV)
            assert torch.equal(count[0], torch.clamp(s0 + i + 1, max=w) if w else s0 + i + 1)
            for waves, kv2 in _forms(hd):
                o, lse = _fwd(q, pk, pv, sk, w, waves, kv2, table=table)
                what = (s0, sq, w, waves, kv2)
                assert bool(E.census_ok(o, e).all()), what
                ok, err = E.lse_ok(lse, count)
                assert ok, (what, err)


def test_swapped_table_entries_change_that_row_only():
    """s0 = 512, sq = 256, window 300 (the rows see keys 213 .. 767, so the
    first two pages are not interchangeable): with the first two entries of row
    0's table swapped, row 0's census output changes and fails the check, row
    1's does not move."""
    dtype, nq, hd, s0, sq, w = torch.bfloat16, 4, 128, 512, 256, 300
    sk = s0 + sq
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    swapped = table.clone()
    swapped[0, 0], swapped[0, 1] = table[0, 1], table[0, 0]
    q, k, v = (t.to(DEV) for t in E.prefill_census_inputs(2, sq, sk, nq, NKV, hd, dtype))
    pk, pv = _pools(k, v, table, sk)
    e, _ = E.prefill_expected(v, E.prefill_visibility(2, sq, sk, True, w, None)[0], nq)
    for waves, kv2 in _forms(hd):
        o, _ = _fwd(q, pk, pv, sk, w, waves, kv2, table=table)
        o2, _ = _fwd(q, pk, pv, sk, w, waves, kv2, table=swapped)
        assert E.census_ok(o, e).tolist() == [True, True], (waves, kv2)
        assert E.census_ok(o2, e).tolist() == [False, True], (waves, kv2)
        assert not torch.equal(_bits(o2[0]), _bits(o[0])), (waves, kv2)
        assert torch.equal(_bits(o2[1]), _bits(o[1])), (waves, kv2)


# ---------------------------------------------------------------- 3. binding checks

def test_binding_checks_name_the_argument():
    dt, hd, nq, sq, sk = torch.bfloat16, 64, 4, 130, 386
    q = torch.zeros(2, sq, nq, hd, device=DEV, dtype=dt)
    pool = torch.zeros(N_PAGES * PAGE, 1, NKV, hd, device=DEV, dtype=dt)
    pk = pv = pool.transpose(0, 1)
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    _fwd(q, pk, pv, sk, table=table)
    _fwd(q, pk, pv, 3 * PAGE, table=table)
    with pytest.raises(RuntimeError, match="page_table must be an int32"):
        _fwd(q, pk, pv, sk, table=table.long())
    with pytest.raises(RuntimeError, match="page_table must be on q's device"):
        _fwd(q, pk, pv, sk, table=table.cpu())
    with pytest.raises(RuntimeError, match="page_table must be 2-D contiguous"):
        _fwd(q, pk, pv, sk, table=table[:1])
    with pytest.raises(RuntimeError, match="page_table must be 2-D contiguous"):
        _fwd(q, pk, pv, sk, table=table[:, :2])
    with pytest.raises(RuntimeError, match="sk exceeds the page_table"):
        _fwd(q, pk, pv, 3 * PAGE + 1, table=table)
    short = pool[:N_PAGES * PAGE - 1].transpose(0, 1)
    with pytest.raises(RuntimeError, match="pool must hold n_pages"):
        _fwd(q, short, short, sk, table=table)
    with pytest.raises(RuntimeError, match="page_table needs causal"):
        _fwd(q, pk, pv, sk, table=table, causal=False)
    cos = torch.ones(1024, hd // 2, device=DEV)
    with pytest.raises(RuntimeError, match="rope_cos cannot be combined with a page_table"):
        _fwd(q, pk, pv, sk, table=table, rope_cos=cos, rope_sin=cos)
    docs = torch.zeros(2, 2, sq, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="docs cannot be combined with a page_table"):
        _fwd(q, pk, pv, sk, table=table, docs=docs)
    # the forcing arguments, with and without a table
    k = torch.zeros(2, sk, NKV, hd, device=DEV, dtype=dt)
    for kw in (dict(table=table, k=pk, v=pv), dict(k=k, v=k)):
        with pytest.raises(RuntimeError, match="waves must be 0"):
            _fwd(q, kw["k"], kw["v"], sk, waves=2, table=kw.get("table"))
        with pytest.raises(RuntimeError, match="kv2 must be -1"):
            _fwd(q, kw["k"], kw["v"], sk, kv2=2, table=kw.get("table"))
        with pytest.raises(RuntimeError, match="kv2 = 1 .* needs head_dim 128"):
            _fwd(q, kw["k"], kw["v"], sk, kv2=1, table=kw.get("table"))


# ---------------------------------------------------------------- 4 / 5. the model and the batcher

def _two_calls(m, ip, prompt, split, paged):
    def call(a, b):
        ip.sequence_len_offset = a
        ip.continue_prefill = paged and a > 0
        with torch.no_grad():
            return m(prompt[None, a:b], torch.arange(a, b, device=DEV)[None], None,
                     inference_params=ip)
    call(0, split)
    logits = call(split, prompt.numel())
    ip.continue_prefill = False
    return logits[0, -1].clone()


def _gpu_run(rank, world, extra):
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import gather_rows
    m = _model(extra)
    out = {}
    # the continued prefill: 300 tokens as [0, s) + [s, 300), pages (2, 1)
    prompt = torch.randint(0, 512, (300,), generator=torch.Generator().manual_seed(3)).to(DEV)
    for split in (256, 255):
        ipu = InferenceParams(1, CAP)
        want = _two_calls(m, ipu, prompt, split, False)
        ipp = InferenceParams(2, CAP, kv_pages=4, table_device=DEV)
        ipp.page_table[0, :2] = torch.tensor([2, 1], dtype=torch.int32)
        got = _two_calls(m, ipp, prompt, split, True)
        rows = True
        for layer, (ku, vu) in ipu.key_value_memory_dict.items():
            kp, vp = ipp.key_value_memory_dict[layer]
            for pool, col in ((kp, ku), (vp, vu)):
                rows = rows and torch.equal(_bits(gather_rows(pool, ipp.page_table[0], 300)[:, 0]),
                                            _bits(col[:300, 0]))
        out[split] = (torch.equal(_bits(got), _bits(want)), bool(got.float().isfinite().all()),
                      rows, kp.dtype)
    # the batcher
    prompts = share_prompts(512)

    def serve(kv_pages, spy=False, **kw):
        ip = InferenceParams(4, CAP, kv_pages=kv_pages)
        cb = ContinuousBatcher(m, ip, 4, CAP, poll_every=1, max_new_tokens=32, **kw)
        snap = []
        if spy:
            prefill = cb._prefill

            def first_prefill(row, prompt, s0=0):
                tok = prefill(row, prompt, s0)
                if not snap:  # request 0: the two pages of P are its table's first two
                    pages = cb.page_log[0][2][:2]
                    rows = torch.cat([torch.arange(p * PAGE, (p + 1) * PAGE) for p in pages]).to(DEV)
                    snap.append((pages, rows, [(k[rows].clone(), v[rows].clone())
                                               for k, v in ip.key_value_memory_dict.values()]))
                return tok
            cb._prefill = first_prefill
        for p, mn in zip(prompts, NEW):
            cb.submit(p, mn)
        return cb.run(), cb, snap
    out["oracle"], _, _ = serve(None, prefill_chunk=256)
    out["shared"], cb, snap = serve(16, spy=True, prefill_chunk=256, prefix_cache=True)
    pages, rows, before = snap[0]
    after = [(k[rows], v[rows]) for k, v in cb.ip.key_value_memory_dict.values()]
    out["pages_unchanged"] = all(torch.equal(_bits(a), _bits(b)) and bool(_bits(a).any())
                                 for pa, pb in zip(before, after) for a, b in zip(pa, pb))
    out["stats"] = (cb.prefix_log, cb.prefilled_tokens, cb.prefix_hit_pages, cb.evictions,
                    cb.dec.captures, cb.pool.in_use, cb.cache.pages(), pages, len(before))
    return out


@pytest.mark.parametrize("extra", [(), ("--inference_fp8_kv_cache",)], ids=["kv16", "kv8"])
def test_continued_prefill_and_prefix_sharing_on_one_graph(extra):
    """The tiny GQA Llama, bf16.  Model: the logits of the continued paged
    prefill are bitwise those of the unpaged continued prefill (GEMMs of the
    same shapes, the attention its bitwise twin) and the pool rows are the
    unpaged column.  Batcher: the request list of the CPU test; the tokens are
    the unpaged ``prefill_chunk=256`` batcher's, on one captured graph, with
    the CPU run's prefix log, and the two pages of P hold after ``run()`` the
    bits they held after the first request's prefill."""
    r = run_dist(_gpu_run, 1, list(extra), env={"EMA_DECODE_FUSED": "1"})[0]
    for split in (256, 255):
        same, finite, rows, dtype = r[split]
        assert same and finite and rows, (split, same, finite, rows)
        assert dtype == (torch.uint8 if extra else torch.bfloat16)
    assert [len(t) for t in r["oracle"]] == list(NEW)
    assert r["shared"] == r["oracle"]
    log, prefilled, hits, evictions, captures, in_use, held, pages, layers = r["stats"]
    assert captures == 1 and log == WANT_LOG and prefilled == WANT_PREFILLED and hits == 6
    assert evictions == 0 and in_use == 2 and held == sorted(pages) and layers >= 1
    assert r["pages_unchanged"]
