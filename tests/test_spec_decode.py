"""Speculative greedy decode (``inference/speculative.py``): ``spec_tail_k`` against
``spec_tail_ref`` on hand-built states; ``SpeculativeGreedyDecoder`` against an fp32
one-token-at-a-time greedy loop on the CPU (eager) and the GPU (graph replay, and
against ``GraphedGreedyDecoder``).  The model's output rows are its embedding rows
under a permutation with cycles of 7, so the context repeats (the drafter finds
something) and greedy is robust to 16-bit rounding: the fp32 top-1 / top-2 gap
(``MIN_GAP``) must be 8x the 16-bit logit error of ``GraphedGreedyDecoder``.  It also
makes the next token a function of the last one alone, so the tokens cannot show a
stale cache row, a wrong ``kv_len``, slot or position; the logits do (another context
moves them by up to 33).  So the logits row behind every committed token is held to
the fp32 loop's: within 4x the error ``GraphedGreedyDecoder`` shows in the same run
(greedy survives an error e while 2 e < gap, and gap >= 8 errors: 4x is the room the
multi-row kernels' other rounding has), and on the CPU within 2^-10 of the largest
logit (fp32 eps is 2^-23 and both sides add the same products in another order)."""
import functools

import pytest
import torch

from dist_utils import init_framework, run_dist
from test_gpu_e2e import LLAMA_GQA

SEED, L, NEW, CAP = 11, 12, 40, 80
MIN_GAP = 90.0  # measured on the CPU: 109.4 (_cpu_run)
BF16, FP16, F32 = torch.bfloat16, torch.float16, torch.float32


def _scenarios(S):
    """name -> (context, argmax of row t, accepted drafts, limit - hist_len, and, traced by
    hand, ``tokens[r]`` after the first call with ngram 3: a ``*_cut`` row parks and keeps its)."""
    D, up = S - 1, lambda a: list(range(a, a + 16))
    g1 = {2: [40, 100], 5: [42, 102, 43, 103, 44],
          16: [47, 107, 30, 40, 41, 42, 43, 44, 45, 46] + [47] * 6}[S]
    return {"g3_clip": ([5, 6, 7, 8, 9, 1, 2, 5, 6], [7] + up(400), 0, 99, [7, 8, 9, 1, 2, 5, 6] + [7] * 9),
            "g1_partial": (sum(([40 + i, 100 + i] for i in range(8)), []) + [30], up(40), D // 2, 99, g1),
            "none_full": ([50, 51, 52], list(range(1001, 985, -1)), D, 99, [1002 - S] * 16),
            "near_end": ([70, 71, 70], [71] + up(420), 0, 99, [71, 70] + [71] * 14),
            "later_wins": ([80, 81, 82, 90, 80, 81, 82, 91, 80, 81], [82] + up(440), 0, 99,
                           [82, 91, 80, 81] + [82] * 12),
            "limit_cut": ([50, 51, 52], up(60), D, (S + 1) // 2, [52] + up(60)),
            "stop_cut": ([55, 56], up(200), D, 99, [56] + up(200))}


# (the three active rows, ngram, stop_id as an index into stop_cut's argmaxes)
CASES = {"hits": (("g3_clip", "g1_partial", "none_full"), 3, None),
         "edges": (("near_end", "later_wins", "limit_cut"), 3, None),
         "ngram0_stop": (("g3_clip", "stop_cut", "later_wins"), 0, True)}


def _logits(am, V, dtype):
    """Rows whose maximum stands at ``am[i]`` and again at ``V - 1``: the first must win."""
    x = torch.randn(len(am), (V + 7) // 8 * 8, generator=torch.Generator().manual_seed(V))
    x[torch.arange(len(am)), am] = 30.0
    x[:, V - 1] = 30.0
    return x.to(dtype)  # [n, ld]: the caller takes [:, :V], rows 16-byte aligned


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("V", [1003, 32000])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("S", [2, 5, 16])
def test_tail_kernel_against_reference(S, dtype, V, case):
    from epfl_megatron_amd.inference.speculative import spec_tail_ref
    from epfl_megatron_amd.ops._ext import ext
    (names, ngram, stop), sc, Lg, I32 = CASES[case], _scenarios(S), torch.long, torch.int32
    b, rows = 4, (0, 1, 3)  # row 2 is inactive: its sentinels must survive
    tokens, pos = torch.full((b, S), -7, dtype=Lg), torch.full((b, S), -7, dtype=Lg)
    slot, kv_len = torch.full((b,), -7, dtype=Lg), torch.full((b,), -7, dtype=I32)
    history, hist_len = torch.full((b, 64), -7, dtype=Lg), torch.full((b,), -7, dtype=Lg)
    limit, accepted = torch.full((b,), -7, dtype=Lg), torch.full((b,), -7, dtype=Lg)
    active, tick = torch.tensor([1, 1, 0, 1], dtype=I32), torch.zeros(1, dtype=Lg)
    ctl = torch.tensor([sc["stop_cut"][1][(S - 1) // 2] if stop else -1, ngram, -7])
    am = torch.zeros(b, S, dtype=Lg)
    for r, name in zip(rows, names):
        ctx, a, n, room, _ = sc[name]
        p = len(ctx) - 1
        tokens[r] = torch.tensor([ctx[-1]] + a[:n] + [a[t] + 1 for t in range(n, S - 1)])
        pos[r], slot[r], kv_len[r] = torch.arange(p, p + S), p, p + S
        history[r, :len(ctx)], hist_len[r] = torch.tensor(ctx), len(ctx)
        limit[r], accepted[r], am[r] = len(ctx) + room, 0, torch.tensor(a[:S])
    ref = [tokens, pos, slot, kv_len, history, hist_len, limit, active, accepted, tick, ctl]
    dev = [t.cuda() for t in ref]
    scratch = (torch.zeros(b, S, dtype=I32).cuda(), torch.zeros(b + 1, dtype=I32).cuda())
    for call in range(2):  # the second on the first's output: every counter re-armed
        if call:  # the first draft of every row is right, the others wrong
            am = torch.cat([tokens[:, 1:2], 300 + torch.arange(b * (S - 1)).view(b, S - 1)], 1)
        lg = _logits(am.view(-1), V, dtype)
        spec_tail_ref(lg[:, :V], *ref)
        ext().spec_tail(lg.cuda()[:, :V], *dev, *scratch)
        for i, (want, got) in enumerate(zip(ref, dev)):
            assert torch.equal(got.cpu(), want), (call, i, got.cpu(), want)
        assert int(tick) == call + 1 and not bool(scratch[1].any())
        for r, name in zip(rows, names if not call else ()):  # the outcome each name states
            exp, parked = sc[name][4], name.endswith("_cut")
            assert tokens[r].tolist() == (exp[:S] if ngram or parked else exp[:1] * S), name
            assert int(active[r]) == (not parked), name
    assert tokens[2].tolist() == [-7] * S and int(hist_len[2]) == -7


def _model(dtype):
    import finetune
    from test_parallel_equivalence import _deterministic_init
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    flag = {BF16: ["--bf16"], FP16: ["--fp16"], F32: []}[dtype]
    init_framework(LLAMA_GQA + ["--hidden_size", "256"] + flag, finetune.extra_args)
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, get_args())
    g = torch.Generator().manual_seed(SEED)
    emb = torch.randn(512, 256, generator=g)
    ids, i = torch.randperm(512, generator=g), torch.arange(512)
    perm = torch.empty(512, dtype=torch.long)
    perm[ids] = ids[(i // 7 * 7 + (i % 7 + 1) % 7).clamp(max=511)]  # cycles of 7 tokens
    head = torch.empty_like(emb)
    head[perm] = emb  # the row of perm[v] is v's embedding: v is followed by perm[v]
    with torch.no_grad():
        for name, p in model[0].named_parameters():
            if name.endswith("word_embeddings.weight"):
                p.copy_(emb)
            elif name.endswith("lm_head"):
                p.copy_(head)
    prompts = torch.randint(0, 512, (3, 4), generator=g).repeat(1, L // 4)  # period 4
    return model[0].eval(), prompts


def _prefill(m, ip, prompts):
    ip.sequence_len_offset, ip.device_multi = 0, False
    pos = torch.arange(prompts.shape[1], device=prompts.device)[None].expand_as(prompts)
    first = m(prompts, pos, None, inference_params=ip)[:, -1].argmax(-1)
    ip.sequence_len_offset = prompts.shape[1]
    return first


def _spec(m, prompts, S, ngram, graph, new=NEW, stop_id=-1):
    from epfl_megatron_amd.inference import SpeculativeGreedyDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    ip = InferenceParams(prompts.shape[0], CAP)
    with torch.no_grad():
        first = _prefill(m, ip, prompts)
        dec = SpeculativeGreedyDecoder(m, ip, prompts.shape[0], new, rows=S, ngram=ngram, graph=graph)
        dec.start(prompts, first, stop_id=stop_id)
        seen = [[0] * len(prompts)]  # the lengths every row passed through
        logits = torch.zeros(len(prompts), new, 512)  # the logits row behind every committed token
        while dec.active_rows():
            dec.step()
            seen.append(dec.generated()[1].tolist())
            for r, (i, j) in enumerate(zip(*seen[-2:])):  # row r committed tokens i..j-1 from rows 0..
                logits[r, i:j] = dec.logits[r, :j - i].float().cpu()
    return ([t[:n].tolist() for t, n in zip(*dec.generated())], dec.mean_accepted(), seen, logits)


def _cpu_run(rank, world):
    """The fp32 greedy loop and the eager decoder on the same prompts."""
    m, prompts = _model(F32)
    ref, logits = [], []
    with torch.no_grad():
        for row in prompts.tolist():
            seq, lg = list(row), []
            for _ in range(NEW + 1):
                lg.append(m(torch.tensor([seq]), None, None).float()[0, -1])
                seq.append(int(lg[-1].argmax()))
            ref.append(seq[L + 1:])
            logits.append(torch.stack(lg[1:]))
    top = torch.stack(logits).topk(2, -1).values
    out = {"ref": ref, "logits": torch.stack(logits), "gap": float((top[..., 0] - top[..., 1]).min())}
    out["spec"], out["accepted"], out["seen"], out["spec_logits"] = _spec(m, prompts, 5, 3, False)
    stop = ref[0][9]
    out["stop"] = (stop, _spec(m, prompts, 5, 3, False, stop_id=stop)[0])
    out["short"] = _spec(m, prompts, 5, 3, False, new=23)[0]
    return out


def test_decoder_on_the_cpu_is_the_greedy_loop():
    out = _run(F32)
    print(f"fp32 top-1/top-2 gap {out['gap']:.3f}, mean accepted {out['accepted']:.3f}")
    assert out["gap"] >= MIN_GAP
    assert out["spec"] == out["ref"] and out["accepted"] > 0
    err = float((out["spec_logits"] - out["logits"]).abs().max())
    print(f"fp32 logit difference {err:.3e} at a largest logit of {float(out['logits'].abs().max()):.1f}")
    assert err <= 2.0 ** -10 * float(out["logits"].abs().max())
    stop, got = out["stop"]
    assert got == [r[:r.index(stop) + 1] if stop in r else r for r in out["ref"]]
    assert len(got[0]) < NEW  # the stop token fell inside the window
    assert out["short"] == [r[:23] for r in out["ref"]]
    assert any(23 not in [n[r] for n in out["seen"]] for r in range(3))  # cut an accepted run


def _gpu_run(rank, world, dtype):
    """Per (S, batch, fp8): tokens of ngram 3 / ngram 0 / GraphedGreedyDecoder, its logits."""
    from epfl_megatron_amd.inference import kv_cache
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder
    m, prompts = _model(dtype)
    prompts, out = prompts.cuda(), {}
    for S, B, fp8 in [(S, B, 0) for S in (2, 8) for B in (1, 3)] + [(8, 3, 1)]:
        kv_cache.set_fp8_kv_cache(bool(fp8))
        pr, ip = prompts[:B], InferenceParams(B, CAP)
        res = {n: _spec(m, pr, S, n, True) for n in (3, 0)}
        with torch.no_grad():
            dec = GraphedGreedyDecoder(m, ip, B, NEW)
            dec.start(_prefill(m, ip, pr), L)
            lg = []
            for _ in range(NEW):
                dec.step()
                lg.append(dec.logits[:, -1].float().cpu())
        out[S, B, fp8] = (res[3][0], res[0][0], dec.history[:, :NEW].tolist(), torch.stack(lg, 1),
                          res[3][1], torch.stack([res[3][3], res[0][3]]))
    kv_cache.set_fp8_kv_cache(False)
    return out


@functools.lru_cache(maxsize=None)
def _run(dtype):
    if dtype is F32:
        return run_dist(_cpu_run, 1, env={"HIP_VISIBLE_DEVICES": ""})[0]
    return run_dist(_gpu_run, 1, dtype)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("S,B,fp8", [(2, 1, 0), (2, 3, 0), (8, 1, 0), (8, 3, 0), (8, 3, 1)])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_decoder_on_the_gpu(dtype, S, B, fp8):
    cpu = _run(F32)
    spec3, spec0, greedy, logits, accepted, spec_logits = _run(dtype)[S, B, fp8]
    err = float((logits - cpu["logits"][:B]).abs().max())
    spec_err = float((spec_logits - cpu["logits"][:B]).abs().max())  # ngram 3 and ngram 0
    print(f"16-bit logit error {err:.3e} (speculative {spec_err:.3e}), fp32 gap {cpu['gap']:.3f}, "
          f"mean accepted {accepted:.3f}")
    assert spec3 == spec0  # a difference is a bookkeeping or cache-slot bug
    assert spec3 == greedy == cpu["ref"][:B]
    assert fp8 or 8 * err <= cpu["gap"]
    assert spec_err <= 4 * err  # the tokens cannot see the context (docstring); the logits do
