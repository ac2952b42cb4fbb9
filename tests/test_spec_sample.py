"""Speculative decode for sampled requests and the HIP front of the multi-row step:
``spec_sample_tail_k`` against ``spec_sample_tail_ref`` (bitwise), against ``spec_tail_k``
at ``top_k == 1`` and against ``sample_ref`` at the lockstep decoder's noise index;
``SpeculativeSamplingDecoder`` on the tiny model of ``test_spec_decode.py``; and
``kv_write_multi_k`` against the ``rope`` op followed by ``LayerKV._write_multi``."""
import functools

import pytest
import torch

from dist_utils import run_dist
from test_spec_decode import BF16, CAP, F32, FP16, NEW, _model, _prefill, _run

Lg, I32 = torch.long, torch.int32
SEED, OFF0 = 1234, 8
FILTERS = {"none": (0, 0.0), "top_k5": (5, 0.0), "top_p0.9": (0, 0.9), "top_k1": (1, 0.0)}


def _state(S, V, dtype, top_k=0, top_p=0.0, temp=1.0, vocab=None, stops=True):
    """(logits [3 * S, V padded to 16 bytes], the state list of ``spec_sample_tail_ref``).
    Sequence 0 has every draft planted (its logit at 40: whatever the filter, it is drawn) and a
    limit that cuts the commit; 1 is inactive; 2 commits the stop token, after one accepted draft at S = 2, else at
    once behind a rejected draft (``stops`` unset: no stop token is set, it commits the same
    tokens and goes on: new position, slot, key count and drafts).  Every other row is a free draw."""
    b, g = 3, torch.Generator().manual_seed(S * V)
    x = 3 * torch.randn(b * S, (V + 7) // 8 * 8, generator=g)
    tokens, stop = torch.randint(0, V - 3, (b, S), generator=g), V - 2
    room, k = (1, 1) if S == 2 else (3, 0)
    for t in range(S - 1):
        x[t, tokens[0, t + 1]] = 40.0
    for t in range(k):
        x[2 * S + t, tokens[2, t + 1]] = 40.0
    x[2 * S + k, stop] = 40.0
    hl = torch.tensor([9, 5, 7])
    history = torch.randint(0, V - 3, (b, 64), generator=g)
    history[torch.arange(b), hl - 1] = tokens[:, 0]
    pos = (hl - 1)[:, None] + torch.arange(S)[None]
    ctl = torch.tensor([stop if stops else -1, 3, -7, SEED, OFF0, top_k, V - 1 if vocab is None else vocab])
    st = [tokens, pos, hl - 1, (hl - 1 + S).to(I32), history, hl.clone(), hl + torch.tensor([room, 90, 90]),
          torch.tensor([1, 0, 1], dtype=I32), torch.zeros(b, dtype=Lg), torch.zeros(1, dtype=Lg), ctl,
          torch.tensor([temp, top_p]), torch.tensor([4, 2, 3])]
    return x.to(dtype), st


def _scratch(b, S):
    return torch.zeros(b, S, dtype=I32).cuda(), torch.zeros(b + 1, dtype=I32).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("V", [1003, 32000])
@pytest.mark.parametrize("S", [2, 4, 16])
@pytest.mark.parametrize("dtype", [BF16, FP16, F32], ids=["bf16", "fp16", "fp32"])
def test_tail_against_transcription(dtype, S, V, filt, temp):
    from epfl_megatron_amd.inference.speculative import spec_sample_tail_ref
    from epfl_megatron_amd.ops._ext import ext
    stops = temp == 1.0  # at the other temperature sequence 2 goes on instead
    lg, ref = _state(S, V, dtype, *FILTERS[filt], temp, stops=stops)
    dev = [t.cuda() for t in ref]
    spec_sample_tail_ref(lg[:, :V], *ref)
    accepted = ref[8]
    assert int(accepted.max()) >= min(2, S - 1) and int(accepted[[0, 2]].min()) == 0, accepted
    # cut at the limit, untouched, stopped (or going on with the drafts of the next step)
    assert ref[7].tolist() == [0, 0, int(not stops)] and int(ref[5][1]) == 5
    assert stops or ref[1][2].tolist() == list(range(int(ref[5][2]) - 1, int(ref[5][2]) - 1 + S))
    scratch = _scratch(3, S)
    ext().spec_sample_tail(lg.cuda()[:, :V], *dev, *scratch)
    for i, (want, got) in enumerate(zip(ref[:11], dev)):  # tokens .. accepted, tick, ctl
        assert torch.equal(got.cpu(), want), (i, got.cpu(), want)
    assert not bool(scratch[1].any())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 4, 16])
def test_top_k_1_is_the_greedy_tail(S):
    from epfl_megatron_amd.ops._ext import ext
    lg, st = _state(S, 1003, BF16, top_k=1, vocab=0)
    greedy, sampled = [t.cuda() for t in st[:11]], [t.cuda() for t in st]
    greedy[10] = greedy[10][:3].clone()
    ext().spec_tail(lg.cuda()[:, :1003], *greedy, *_scratch(3, S))
    ext().spec_sample_tail(lg.cuda()[:, :1003], *sampled, *_scratch(3, S))
    for i, (want, got) in enumerate(zip(greedy, sampled)):
        assert torch.equal(got[:3] if i == 10 else got, want), (i, got, want)


@pytest.mark.gpu
def test_noise_index_is_the_lockstep_decoders():
    """One logits row for every row of every step: generated token n of sequence r is
    ``sample_ref`` of that row at Philox row r, step n, whatever S and ngram are."""
    from epfl_megatron_amd.ops._ext import ext
    from epfl_megatron_amd.ops.sampling import sample_ref
    b, V, P, n_new = 2, 1003, 4, 12
    row = 2.5 * torch.randn(1, 1008, generator=torch.Generator().manual_seed(3))
    want = torch.stack([sample_ref(row[:, :V].expand(b, -1), SEED, OFF0, n, temperature=0.7)
                        for n in range(n_new)], 1)
    assert len(set(want.flatten().tolist())) < b * n_new  # tokens repeat: the drafter finds some
    for S in (2, 8):
        for ngram in (0, 3):
            z = functools.partial(torch.zeros, dtype=Lg, device="cuda")
            history, hl = z(b, P + 1 + n_new), z(b) + P + 1
            st = [z(b, S), P + torch.arange(S).cuda().repeat(b, 1), z(b) + P, (z(b) + P + S).to(I32),
                  history, hl, z(b) + P + 1 + n_new, torch.ones(b, dtype=I32).cuda(), z(b), z(1),
                  torch.tensor([-1, ngram, b, SEED, OFF0, 0, 0]).cuda(),
                  torch.tensor([0.7, 0.0]).cuda(), z(b) + P + 1]
            scratch, lg, steps = _scratch(b, S), row.cuda().repeat(b * S, 1)[:, :V], 0
            while bool(st[7].any()):
                ext().spec_sample_tail(lg, *st, *scratch)
                steps += 1
                assert steps <= n_new
            assert torch.equal(history[:, P + 1:].cpu(), want), (S, ngram)
            assert S == 2 or steps < n_new  # some draft was accepted (the runs of one token)


def _sampled_run(rank, world, dtype, tokens=None):
    """GPU: step ``SpeculativeSamplingDecoder`` by hand: (tokens, the logits row behind each, seed,
    offset0, accepted).  CPU (``tokens`` given): the fp32 one-token-at-a-time logits for them."""
    m, prompts = _model(dtype)
    if tokens is not None:
        out = []
        with torch.no_grad():
            for row, new in zip(prompts.tolist(), tokens):
                seq, lg = list(row), []
                for t in new:
                    seq.append(t)
                    lg.append(m(torch.tensor([seq]), None, None).float()[0, -1])
                out.append(torch.stack(lg[:-1]))
        return torch.stack(out)
    from epfl_megatron_amd.inference import SpeculativeSamplingDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    prompts, B = prompts.cuda(), prompts.shape[0]
    ip = InferenceParams(B, CAP)
    with torch.no_grad():
        first = _prefill(m, ip, prompts)
        dec = SpeculativeSamplingDecoder(m, ip, B, NEW, rows=4, ngram=3, graph=True)
        dec.start(prompts, first, top_p=0.95, temperature=25.0)
        logits, done = torch.zeros(B, NEW, 512), [0] * B
        while dec.active_rows():
            dec.step()
            now = dec.generated()[1].tolist()
            for r, (i, j) in enumerate(zip(done, now)):
                logits[r, i:j] = dec.logits[r, :j - i].float().cpu()
            done = now
    return (dec.generated()[0].cpu(), logits, first.tolist(), dec.seed, dec.offset0,
            dec.mean_accepted(), dec.logits.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_decoder_commits_the_draw_of_the_row_it_holds(dtype):
    from epfl_megatron_amd.ops.sampling import sample_ref
    toks, logits, first, seed, off0, accepted, ldt = run_dist(_sampled_run, 1, dtype)[0]
    for n in range(NEW):  # the rows as the kernel read them, at the lockstep decoder's index
        want = sample_ref(logits[:, n].to(ldt), seed, off0, n, top_p=0.95, temperature=25.0)
        assert toks[:, n].tolist() == want.tolist(), n
    fp32 = run_dist(_sampled_run, 1, F32, [[f] + t for f, t in zip(first, toks.tolist())],
                    env={"HIP_VISIBLE_DEVICES": ""})[0]
    err16 = float((_run(dtype)[8, 3, 0][3] - _run(F32)["logits"]).abs().max())
    err = float((logits - fp32).abs().max())
    print(f"logit error {err:.3e}, GraphedGreedyDecoder's {err16:.3e}, accepted {accepted:.3f}")
    assert err <= 4 * err16  # test_spec_decode.py's bound for the multi-row step


# ---------------------------------------------------------------- kv_write_multi_k
G, B, PAGES = 2, 3, 7
TABLE = ((4, 2), (6, 1), (3, 5))  # as test_kv_multirow.py: neither adjacent nor in order


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("sq", [2, 4, 16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("layout", ["columns", "paged", "one_slot"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "e4m3"])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_write_kernel_is_rope_then_write_multi(dtype, fp8, layout, hd, sq, r):
    from epfl_megatron_amd.inference import kv_cache
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.paged import KV_PAGE
    from epfl_megatron_amd.ops.rope import rope_qkv_inplace, rope_table
    paged, dev = layout == "paged", torch.device("cuda", 0)
    # first new position: mid-page, a page's last slot (the rows cross its edge), 0
    first = (9, 9, 9) if layout == "one_slot" else (7, KV_PAGE - 1, 0)
    cos, sin = rope_table(hd, 2 * KV_PAGE, dev)
    pos = torch.tensor(first, device=dev)[:, None] + torch.arange(sq, device=dev)[None]
    x = torch.randn(sq, B, G, r + 2, hd, generator=torch.Generator().manual_seed(sq * hd + r))
    x[0, 0, 0, r:, :4] = torch.tensor([1e4, -1e4, 500.0, -0.0])  # past the e4m3 clamp on both sides
    got, want = x.to(dtype).cuda(), x.to(dtype).cuda()
    kv_cache.set_fp8_kv_cache(fp8)
    try:
        mems = []
        for native in (True, False):
            ip = InferenceParams(B, 2 * KV_PAGE, kv_pages=PAGES if paged else None)
            ip.device_multi = True
            if paged:
                ip.page_table[:B] = torch.tensor(TABLE, dtype=I32)
            slots = [TABLE[m][p // KV_PAGE] * KV_PAGE + p % KV_PAGE if paged else p
                     for m, p in enumerate(first)]
            ip.device_offset = torch.tensor(slots[:1] if layout == "one_slot" else slots, device=dev)
            ip.device_kv_len = torch.tensor([p + sq for p in first], dtype=I32, device=dev)
            kv = kv_cache.LayerKV(ip, 1, G, hd, dtype, dev, sq, B)
            kv.kmem.fill_(7)
            kv.vmem.fill_(7)
            if fp8:
                kv.scales.copy_(torch.tensor([[0.5, 2.0], [4.0, 1.0]]))
            if native:
                assert kv.write_multi_native(got, (cos, sin), pos)
            else:
                rope_qkv_inplace(want, cos, sin, pos)
                kv._write_multi(want[:, :, :, r], want[:, :, :, r + 1])
            mems.append((kv.kmem, kv.vmem))
    finally:
        kv_cache.set_fp8_kv_cache(False)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    target = torch.zeros(mems[0][0].shape[:2], dtype=torch.bool)
    for m, p in enumerate(first):
        for t in range(sq):
            q = p + t
            target[(TABLE[m][q // KV_PAGE] * KV_PAGE + q % KV_PAGE, 0) if paged else (q, m)] = True
    for a, b_ in zip(*mems):  # (K, V) of the kernel, of the torch path
        a, b_, bits = a.cpu(), b_.cpu(), torch.uint8 if fp8 else torch.int16
        assert torch.equal(a.view(bits), b_.view(bits))
        assert bool((b_[~target] == 7).all()) and float((b_[target] != 7).float().mean()) > 0.5
