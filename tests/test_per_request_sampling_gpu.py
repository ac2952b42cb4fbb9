"""The per-row form of the ragged tail (``ragged_tail_k``, ``csrc/decode_tail.hip``)
on the GPU, then the batcher with mixed requests.  Rows of the kernel-level
launch: 0 greedy on all-equal logits (a V-way tie: token 0, log p = -log V), 1
top-k, 2 top-p, 3 temperature only, 4 greedy with a stop id that it hits, its
maximum 60 above the rest (log p = 0, the sum is rescaled), 5 inactive, 6
greedy, its maximum in the last column, which vocab_limit = V - 1 clamps."""
import functools
import math
import types

import pytest
import torch

from dist_utils import run_dist
from epfl_megatron_amd.ops._ext import ext as _ext

pytestmark = pytest.mark.gpu

DEV, L, B, H = "cuda", torch.long, 7, 6
# per row: top_k, top_p, temperature, seed, offset0, hist_idx, pos, stop id (row
# 0 emits row 4's stop id too and runs on)
TOP_K, TOP_P, TEMP, SEED, OFF0, HIST_IDX, POS, STOPS = zip(
    (1, 0.0, 1.0, 11, 0, 0, 5, 1), (40, 0.0, 1.0, 22, 100, 2, 9, -1), (0, 0.9, 0.8, 33, 7, 1, 30, -1),
    (0, 0.0, 1.3, 44, 4096, 3, 77, -1), (1, 0.0, 1.0, 55, 3, 0, 598, 0), (0, 0.0, 1.0, 66, 9, 1, 12, -1),
    (1, 0.0, 1.0, 77, 1, 4, 40, -1))
ACT, PERM = [0, 1, 2, 3, 4, 6], (3, 5, 1, 6, 0, 4, 2)
CASES = [(dt, V) for dt in (torch.bfloat16, torch.float16) for V in (1003, 32000, 65024)]


def _padded(x):  # on the device with 16-byte aligned rows
    buf = torch.zeros(x.shape[0], -(-x.shape[1] // 8) * 8, dtype=x.dtype, device=DEV)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


@functools.lru_cache(None)
def _logits(dtype, V):
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(V)) * 3).to(dtype)
    x[0] = 1.5
    x[4, 0] = float(x[4].float().max()) + 60
    x[6, V - 1] = float(x[6].float().max()) + 2
    return x


def _launch(x, order=range(B), tick=3, rows=True, sample=True, logp=True, limit=(H,) * B):
    def t(v, dtype=L):
        return torch.tensor([v[i] for i in order], dtype=dtype, device=DEV)
    s = types.SimpleNamespace(
        tokens=torch.full((B,), -7, dtype=L, device=DEV),
        history=torch.full((B, H), -7, dtype=L, device=DEV), hist_idx=t(HIST_IDX), pos=t(POS),
        slot=t(POS), kv_len=t(POS, torch.int32) + 1, active=t([r in ACT for r in range(B)], torch.int32),
        limit=t(limit), tick=torch.tensor([tick], device=DEV),
        counter=torch.zeros(1, dtype=torch.int32, device=DEV),
        # seed, offset0 and top_k are garbage where the row tables replace them
        ctl=torch.tensor([999, 999, 7 if rows else 0, x.shape[1] - 1, -1, -1], device=DEV),
        fctl=torch.tensor([0.3, 0.0], device=DEV),
        logprob=torch.full((B,), 9.0, device=DEV), hist_logprob=torch.full((B, H), 9.0, device=DEV))
    kw = dict(logprob=s.logprob, hist_logprob=s.hist_logprob) if logp else {}
    if rows:
        kw.update(row_ctl=torch.stack([t(SEED), t(OFF0), t(TOP_K), t(STOPS)], 1).contiguous(),
                  row_fctl=torch.stack([t(TEMP, torch.float32), t(TOP_P, torch.float32)], 1).contiguous())
    _ext().ragged_tail(_padded(x[list(order)]), s.tokens, s.history, s.hist_idx, s.pos, s.slot,
                       s.kv_len, s.active, s.limit, s.tick, s.counter, s.ctl, s.fctl, sample, **kw)
    return s


def _lp_errors(x, tok, got):
    # per row: |got - fp64 log_softmax of x at tok|, and the yardstick: torch's fp32 one on the CPU
    x, idx = x.cpu(), tok.cpu().view(-1, 1)
    ref = torch.log_softmax(x.double(), -1).gather(1, idx).view(-1)
    yard = (torch.log_softmax(x.float(), -1).gather(1, idx).view(-1) - ref).abs()
    return (got.cpu() - ref).abs(), yard


@pytest.mark.parametrize("dtype,V", CASES)
def test_per_row_tail_draws_log_probabilities_and_state(dtype, V):
    x = _logits(dtype, V)
    s = _launch(x)
    for r in (1, 2, 3):
        want = torch.empty(1, dtype=L, device=DEV)
        _ext().sample_rows(_padded(x[r:r + 1]), want, SEED[r], OFF0[r] + HIST_IDX[r], TOP_K[r],
                           TOP_P[r], TEMP[r], V - 1)
        assert int(s.tokens[r]) == int(want), r
    assert x[[0, 4, 6]].float().argmax(1).tolist() == [0, 0, V - 1]
    assert s.tokens[[0, 4, 6]].tolist() == [0, 0, V - 2]  # first of the tie; clamped
    moved = _launch(x, PERM, tick=11)
    assert moved.tokens.tolist() == [int(s.tokens[i]) for i in PERM]
    assert torch.equal(moved.logprob, s.logprob[list(PERM)])
    err, yard = _lp_errors(x[ACT], s.tokens[ACT], s.logprob[ACT])
    allow = 4 * float(yard.max()) + 1e-6
    print(f"log-probability error {float(err.max()):.3e}, fp32 on the CPU {float(yard.max()):.3e}")
    assert float(err.max()) <= allow
    assert abs(float(s.logprob[0]) + math.log(V)) <= allow and abs(float(s.logprob[4])) <= allow
    assert s.hist_logprob[ACT, [HIST_IDX[r] for r in ACT]].tolist() == s.logprob[ACT].tolist()
    assert int((s.hist_logprob != 9.0).sum()) == len(ACT) and float(s.logprob[5]) == 9.0
    # the existing greedy launch on logits that select the same tokens (row 4 parks on its limit)
    onehot = torch.zeros(B, V, dtype=dtype)
    onehot[torch.arange(B), s.tokens.cpu().clamp(min=0)] = 1.0
    e = _launch(onehot, rows=False, sample=False, logp=False, limit=(H,) * 4 + (1, H, H))
    for name in ("tokens", "history", "hist_idx", "pos", "slot", "kv_len", "active", "tick", "counter"):
        assert torch.equal(getattr(s, name), getattr(e, name)), name
    assert int(s.ctl[5]) == int(e.ctl[5]) == 5 and s.active.tolist() == [1, 1, 1, 1, 0, 0, 1]


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_single_setting_tails_report_log_probabilities_too(sample):
    # the shared-setting forms: the tokens of the launch without the outputs, bitwise
    x = _logits(torch.bfloat16, 32000)
    plain, s = (_launch(x, rows=False, sample=sample, logp=lp) for lp in (False, True))
    assert torch.equal(s.tokens, plain.tokens) and torch.equal(s.history, plain.history)
    err, yard = _lp_errors(x[ACT], s.tokens[ACT], s.logprob[ACT])
    assert float(err.max()) <= 4 * float(yard.max()) + 1e-6


SETTINGS = (dict(top_k=1), dict(top_k=50), dict(top_p=0.9, temperature=0.8), dict(temperature=1.2))
MAX_NEW = (6, 9, 5, 7, 8, 4, 9, 6)


def _batcher(rank, world):
    from test_continuous_gpu import CAP, _model, _prompts
    from epfl_megatron_amd.inference import ContinuousBatcher, RaggedSamplingDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m, P = _model(), _prompts()

    def batcher(b):
        ip = InferenceParams(b, CAP)
        dec = RaggedSamplingDecoder(m, ip, b, 12, vocab_size=512, per_row=True, return_log_probs=True)
        dec.configure()
        return ContinuousBatcher(m, ip, b, CAP, poll_every=1, decoder=dec)
    cb, solo = batcher(4), batcher(1)
    dec, replay, worst = cb.dec, cb.dec.step, [0.0, 0.0]

    def step():  # every replay: hist_logprob against log_softmax of the step's own logits
        rows = dec.active.nonzero().flatten()
        hi = dec.hist_idx[rows]
        replay()
        if not rows.numel():
            return
        errs = _lp_errors(dec.logits[rows, -1], dec.tokens[rows], dec.hist_logprob[rows, hi])
        worst[:] = [max(w, float(e.max())) for w, e in zip(worst, errs)]
    dec.step = step
    for i in range(8):
        for b in (cb, solo):
            b.submit(P[i % 4].cpu(), MAX_NEW[i], seed=1000 + i, **SETTINGS[(i + i // 4) % 4])
        solo.run()
    return cb.run(), cb.log_probs, solo.run(), solo.log_probs, worst, dec.captures


def test_mixed_requests_in_one_batch_are_the_requests_alone():
    # tokens and log p of each request alone at batch one (bitwise the batch-4 logits at this
    # model size, docs/guide/kernels.md); every replay's log p against that replay's own logits
    res, lps, alone, alone_lps, (err, yard), captures = run_dist(_batcher, 1)[0]
    assert [len(t) for t in res] == [len(lps[i]) for i in range(8)] == list(MAX_NEW) and captures == 1
    assert res == alone and lps == alone_lps and len({tuple(t) for t in res}) == 8
    assert err <= 4 * yard + 1e-6, (err, yard)
