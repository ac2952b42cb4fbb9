"""Ragged decode and continuous batching on the CPU (gloo, fp32 tiny model):
the reference paths, the eager (``capture=False``) ragged decoder against
per-sequence cache-free greedy generation, and the scheduler of
``ContinuousBatcher``.  The GPU kernels and the captured graph are covered by
``test_continuous_gpu.py``."""
import pytest
import torch

from dist_utils import run_dist
from test_inference import _argv, _setup

CAP = 32  # TINY_LLAMA's rotary table


# ---------------------------------------------------------------- reference paths

@pytest.mark.parametrize("window", [0, 3, 9])
def test_flash_decode_cached_per_row_lengths(window):
    """Row i of a per-row ``kv_len`` sees the keys [max(0, n_i - window), n_i)."""
    from epfl_megatron_amd.ops.attention import attention_ref, flash_decode_cached
    torch.manual_seed(0)
    b, cap, nq, nkv, hd = 4, 20, 4, 2, 16
    q = torch.randn(b, 1, nq, hd)
    k, v = torch.randn(b, cap, nkv, hd), torch.randn(b, cap, nkv, hd)
    lens = [0, 1, 20, 11]
    o = flash_decode_cached(q, k, v, torch.tensor(lens, dtype=torch.int32), window=window)
    assert o.shape == (b, 1, nq, hd)
    for i, n in enumerate(lens):
        if n == 0:
            assert not o[i].any()
            continue
        lo = max(n - window, 0) if window else 0
        want = attention_ref(q[i:i + 1], k[i:i + 1, lo:n], v[i:i + 1, lo:n], False, hd ** -0.5)
        torch.testing.assert_close(o[i:i + 1], want, atol=0, rtol=0)
    # one element: the whole batch, as before
    o1 = flash_decode_cached(q, k, v, torch.tensor([11], dtype=torch.int32), window=window)
    torch.testing.assert_close(o1[3], o[3], atol=0, rtol=0)


def test_ragged_tail_reference_by_hand():
    """Three steps of the torch transcription of the ragged tail against
    values written out by hand: row 0 stops on stop_id in step 2, row 1 on its
    limit in step 2, row 2 is parked throughout, row 3 runs on."""
    from epfl_megatron_amd.inference.continuous import ragged_tail_reference
    L = torch.long
    tokens = torch.full((4,), -7, dtype=L)
    history = torch.full((4, 5), -7, dtype=L)
    hist_idx = torch.tensor([0, 0, 3, 1], dtype=L)
    pos = torch.tensor([5, 9, 30, 2], dtype=L)
    slot = pos.clone()
    kv_len = (pos + 1).int()
    active = torch.tensor([1, 1, 0, 1], dtype=torch.int32)
    limit = torch.tensor([5, 2, 5, 5], dtype=L)
    tick = torch.zeros(1, dtype=L)
    ctl = torch.tensor([0, 0, 0, 0, 99, -1], dtype=L)
    st = (tokens, history, hist_idx, pos, slot, kv_len, active, limit, tick, ctl)
    ragged_tail_reference(torch.tensor([11, 21, 31, 41]), *st)
    assert tokens.tolist() == [11, 21, -7, 41] and active.tolist() == [1, 1, 0, 1]
    assert pos.tolist() == [6, 10, 30, 3] and kv_len.tolist() == [7, 11, 31, 4]
    assert int(ctl[5]) == 3 and int(tick) == 1
    ragged_tail_reference(torch.tensor([99, 22, 32, 42]), *st)
    assert tokens.tolist() == [99, 22, -7, 42] and active.tolist() == [0, 0, 0, 1]
    # finished rows keep their slot (never the one past their last token)
    assert pos.tolist() == [6, 10, 30, 4] and slot.tolist() == [6, 10, 30, 4]
    assert kv_len.tolist() == [7, 11, 31, 5] and hist_idx.tolist() == [2, 2, 3, 3]
    assert int(ctl[5]) == 1 and int(tick) == 2
    ragged_tail_reference(torch.tensor([13, 23, 33, 43]), *st)
    assert tokens.tolist() == [99, 22, -7, 43] and hist_idx.tolist() == [2, 2, 3, 4]
    assert history.tolist() == [[11, 99, -7, -7, -7], [21, 22, -7, -7, -7], [-7] * 5,
                                [-7, 41, 42, 43, -7]]
    assert int(ctl[5]) == 1 and int(tick) == 3


# ---------------------------------------------------------------- the eager decoder and the batcher

PROMPTS = ([3, 14, 15], [5, 35, 8, 9, 7, 9, 3], [2, 7, 1, 8, 2, 8, 1, 8, 2, 8, 4, 5],
           [9, 9], [4, 4, 4, 4, 4], [6, 5, 3, 5, 8, 9], [1, 2])
MAX_NEW = (6, 4, 7, 3, 1, 5, 6)


def _prefill_row(model, ip, row, prompt):
    """Eager b = 1 prefill of ``prompt`` into cache column ``row``."""
    ip.sequence_len_offset, ip.batch_size_offset = 0, row
    t = torch.tensor([prompt])
    with torch.no_grad():
        logits = model(t, torch.arange(len(prompt))[None], None, inference_params=ip)
    ip.batch_size_offset = 0
    return logits[0, -1]


def _cpu_run(rank, world):
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.models import transformer
    model = _setup(_argv())
    out = {}
    n = 6
    # cache-free greedy generation per sequence: tokens and the logits that picked them
    refs = []
    for p, mn in zip(PROMPTS, MAX_NEW):
        seq = list(p)
        with torch.no_grad():
            for i in range(max(mn, n)):
                logits = model(torch.tensor([seq]), None, None).float()[0, -1]
                seq.append(int(logits.argmax()))
                if i == n - 1:  # the logits that pick token n
                    lp_n = torch.log_softmax(logits, -1)
        refs.append((seq[len(p):], lp_n))
    out["refs"] = [r[0] for r in refs]
    # RaggedGreedyDecoder(capture=False) on three ragged prompts
    b = 3
    ip = InferenceParams(b, CAP)
    dec = RaggedGreedyDecoder(model, ip, b, n, capture=False)
    ip.device_offset = ip.device_kv_len = None
    firsts = []
    for row in range(b):
        firsts.append(int(_prefill_row(model, ip, row, PROMPTS[row]).argmax()))
    for row in range(b):
        dec.prime(row, firsts[row], len(PROMPTS[row]), n - 1)
    steps = 0
    while dec.active_rows():
        dec.step()
        steps += 1
    out["dec_tokens"] = [[firsts[r]] + dec.history[r, :n - 1].tolist() for r in range(b)]
    out["dec_steps"], out["dec_hist_idx"] = steps, dec.hist_idx.tolist()
    # the last step fed token n - 1 of every row: its logits pick token n
    lp = torch.log_softmax(dec.logits[:, -1].float(), -1)
    out["dec_lp_err"] = [float((lp[r] - refs[r][1]).abs().max()) for r in range(b)]
    out["dec_state"] = (dec.pos.view(-1).tolist(), dec.slot.tolist(), dec.kv_len.tolist())

    # the batcher: 7 requests over 2 rows
    def serve(poll, stop_id=-1, batch=2):
        ipb = InferenceParams(batch, CAP)
        cb = ContinuousBatcher(model, ipb, batch, CAP, poll_every=poll, stop_id=stop_id,
                               capture=False)
        ids = [cb.submit(p, mn) for p, mn in zip(PROMPTS, MAX_NEW)]
        res = cb.run()
        return ids, res, cb
    ids, res1, cb1 = serve(1)
    _, res5, cb5 = serve(5)
    out["ids"], out["res1"], out["res5"] = ids, res1, res5
    out["primed"] = cb1.primed + cb5.primed
    out["replays"] = (cb1.replays, cb5.replays)
    out["captures"] = cb1.dec.captures
    out["ip_after"] = (cb1.ip.sequence_len_offset, cb1.ip.batch_size_offset,
                       cb1.ip.device_offset is cb1.dec.slot)
    # a request that stops on its first generated (decoder) token: stop on request 0's
    # second token; and on the first token picked from the prefill
    stop = refs[0][0][1]
    _, res_stop, _ = serve(1, stop_id=stop)
    out["stop"], out["res_stop"] = stop, res_stop
    # sampled first tokens and refills with blocks of 8 Philox offsets: the replays'
    # offsets (offset0 + tick) against the ones handed to the first-token draws
    from epfl_megatron_amd.inference import RaggedSamplingDecoder
    ips = InferenceParams(2, CAP)
    decs = RaggedSamplingDecoder(model, ips, 2, 8, vocab_size=250, capture=False)
    decs.RESERVE = 8
    decs.configure(top_p=0.9, temperature=0.8, stop_id=-1)
    cbs = ContinuousBatcher(model, ips, 2, CAP, poll_every=1, decoder=decs)
    used, replay = [], decs.step

    def step():
        replay()
        used.append(decs.offset0 + decs.ticks - 1)
    decs.step = step
    for p, mn in zip(PROMPTS, MAX_NEW):
        cbs.submit(p, mn)
    res_s = cbs.run()
    out["sampled"] = dict(used=used, first=list(decs.first_draws), blocks=list(decs.blocks),
                          lens=[len(r) for r in res_s], tick=int(decs.tick))
    # errors
    errs = {}
    cb = ContinuousBatcher(model, InferenceParams(2, CAP), 2, CAP, capture=False)
    for name, args in (("one_token", ([5], 4)), ("fits", ([1] * 20, CAP - 20)),
                       ("too_long", ([1] * 20, CAP - 20 + 1))):
        try:
            cb.submit(*args)
            errs[name] = None
        except ValueError as e:
            errs[name] = str(e)
    decs.set_stop_id(7)
    try:  # one owner of the stop token: the decoder
        ContinuousBatcher(model, ips, 2, CAP, decoder=decs, stop_id=9)
        errs["stop_owner"] = None
    except ValueError as e:
        errs["stop_owner"] = str(e)
    errs["stop_kept"] = (ContinuousBatcher(model, ips, 2, CAP, decoder=decs).dec.stop_id,
                         int(decs.ctl[4]))
    transformer.set_fp8_kv_cache(True, calibrate=True)
    try:
        RaggedGreedyDecoder(model, InferenceParams(2, CAP), 2, 4, capture=False)
        errs["calibrate"] = None
    except NotImplementedError as e:
        errs["calibrate"] = str(e)
    finally:
        transformer.set_fp8_kv_cache(False, calibrate=False)
    out["errs"] = errs
    return out


@pytest.fixture(scope="module")
def cpu_run():
    return run_dist(_cpu_run, 1)[0]


def test_eager_ragged_decoder_matches_per_sequence_generation(cpu_run):
    r, n = cpu_run, 6
    for row in range(3):
        assert r["dec_tokens"][row] == r["refs"][row][:n], row
        # the tolerance of test_inference.py for KV-cached against the full forward
        assert r["dec_lp_err"][row] <= 2e-4, r["dec_lp_err"]
    assert r["dec_steps"] == n - 1 and r["dec_hist_idx"] == [n - 1] * 3
    # a finished row stays on the slot of its last fed token
    plens = [len(p) for p in PROMPTS[:3]]
    pos, slot, kv_len = r["dec_state"]
    assert pos == slot == [p + n - 2 for p in plens] and kv_len == [p + n - 1 for p in plens]


def test_batcher_serves_more_requests_than_rows_in_order(cpu_run):
    r = cpu_run
    assert r["ids"] == list(range(len(PROMPTS)))
    for i, mn in enumerate(MAX_NEW):
        assert r["res1"][i] == r["refs"][i][:mn], i
    assert r["res5"] == r["res1"]  # poll_every changes when a row is refilled, not what it says
    assert r["captures"] == 0  # the eager step
    assert r["ip_after"] == (0, 0, True)


def test_batcher_never_primes_past_capacity(cpu_run):
    assert cpu_run["primed"]
    for row, position, max_new in cpu_run["primed"]:
        assert 0 <= row < 2 and position + max_new <= CAP - 1


def test_batcher_stop_token(cpu_run):
    r = cpu_run
    stop = r["stop"]
    for i, mn in enumerate(MAX_NEW):
        want = r["refs"][i][:mn]
        if stop in want:
            want = want[:want.index(stop) + 1]
        assert r["res_stop"][i] == want, i
    # request 0 stops on the first token the decoder generates (or on the one
    # from the prefill, should the model repeat itself)
    assert len(r["res_stop"][0]) <= 2 and r["res_stop"][0][-1] == stop


def test_batcher_errors(cpu_run):
    e = cpu_run["errs"]
    assert e["one_token"] is not None and "two tokens" in e["one_token"]
    # the bound GraphedGreedyDecoder.start enforces, with its text: the whole
    # sequence must fit the cache; exactly filling it is the last legal request
    assert e["fits"] is None
    assert e["too_long"] == "KV cache too short for max_new_tokens"
    assert e["calibrate"] is not None and "set_kv_scales" in e["calibrate"]
    assert e["stop_owner"] is not None and "disagrees" in e["stop_owner"]
    assert e["stop_kept"] == (7, 7)


def test_sampling_offsets_are_never_shared(cpu_run):
    """Sampled first tokens (one generator draw per admission) and refills over
    blocks of 8 reserved offsets: every replay draws inside a reserved block,
    no offset is used twice, and none is shared with a first-token draw."""
    c = cpu_run["sampled"]
    used, first, blocks = c["used"], c["first"], c["blocks"]
    assert c["lens"] == list(MAX_NEW)
    assert c["tick"] == len(used) and len(set(used)) == len(used)
    assert len(first) == len(PROMPTS) and len(blocks) >= 2
    assert all(any(lo <= u < hi for lo, hi in blocks) for u in used)
    taken = sorted([tuple(b) for b in blocks] + [(f, f + 4) for f in first])
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:])), taken
