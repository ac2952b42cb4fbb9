"""The sampling decode tail on the GPU (csrc/decode_tail.hip ``sample_tail_k``)
against its fp64 reference (ops/sampling.py ``sample_ref``), the graphed
sampling decoder and ``--inference_fused_sampling`` through the API.

The kernel works in fp32, the reference in fp64, so a draw whose two best
keys are closer than the fp32 error, or whose top-p boundary moves within it,
may legitimately differ: ``sample_ref(return_sets=True)`` returns the tokens a
correct kernel may pick (margins derived in ops/sampling.py), and every case
asserts that at most 1 % of its rows have more than one."""
import pytest
import torch

from dist_utils import run_dist, init_framework

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, OFFSET = 0x1234ABCD5678, 40

SHAPES = [(1, 32000, torch.bfloat16), (5, 1003, torch.bfloat16), (3, 32000, torch.float32),
          (16, 4096, torch.float16), (2, 128256, torch.bfloat16)]
MODES = {"nofilter": dict(), "k50_t07": dict(top_k=50, temperature=0.7), "k2": dict(top_k=2),
         "p09_t13": dict(top_p=0.9, temperature=1.3), "p005": dict(top_p=0.05),
         "k8_tied": dict(top_k=8)}


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def _logits(b, V, dtype, seed):
    """randn * 3 rows as a strided view with 16-byte aligned rows."""
    g = torch.Generator().manual_seed(seed)
    full = (torch.randn(b, (V + 5 + 7) // 8 * 8, generator=g) * 3).to(dtype).to(DEV)
    return full[:, :V]


class _Tail:
    """The tail's state tensors, as GraphedSamplingDecoder holds them."""

    def __init__(self, b, top_k=0, top_p=0.0, temperature=1.0, vocab_limit=0, stop_id=-1,
                 tokens=None):
        self.b = b
        self.tokens = torch.zeros(b, dtype=torch.long, device=DEV) if tokens is None \
            else tokens.to(DEV)
        self.history = torch.full((b, 8), -1, dtype=torch.long, device=DEV)
        self.step = torch.tensor([2], dtype=torch.long, device=DEV)
        self.pos = torch.arange(b, dtype=torch.long, device=DEV) + 10
        self.slot = torch.tensor([40], dtype=torch.long, device=DEV)
        self.kvl = torch.tensor([41], dtype=torch.int32, device=DEV)
        self.counter = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ctl = torch.tensor([SEED, OFFSET, top_k, vocab_limit, stop_id, -5], device=DEV)
        self.fctl = torch.tensor([temperature, top_p], dtype=torch.float32, device=DEV)

    def run(self, logits):
        _ext().sample_tail(logits, self.tokens, self.history, self.step, self.pos, self.slot,
                           self.kvl, self.counter, self.ctl, self.fctl)
        return self.tokens.clone()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("b,V,dtype", SHAPES)
def test_sample_tail_matches_reference(b, V, dtype, mode):
    """Two consecutive tail calls: the token of each row (noise indexed by the
    device step), the history column, the position / step / slot / key-count
    increments and the re-armed counter."""
    from epfl_megatron_amd.ops.sampling import sample_ref
    kw = MODES[mode]
    logits = _logits(b, V, dtype, b * V + len(mode))
    if mode == "k8_tied":  # the 8th value twice: nine tokens stay
        order = logits.float().argsort(1, descending=True)
        logits.scatter_(1, order[:, 8:9], logits.gather(1, order[:, 7:8]))
    st = _Tail(b, **kw)
    ambiguous = 0
    for it in range(2):
        got = st.run(logits).cpu()
        want, kept, sets = sample_ref(logits, SEED, OFFSET, step=2 + it, return_kept=True,
                                      return_sets=True, **kw)
        if mode == "k8_tied":  # (>: bf16 rows can hold further ties of their own)
            assert (kept.sum(1) >= 9).all()
        for r in range(b):
            assert int(got[r]) in sets[r], (r, it, int(got[r]), sets[r], int(want[r]))
        ambiguous += sum(len(s) > 1 for s in sets)
        assert torch.equal(st.history[:, 2 + it].cpu(), got)
    assert ambiguous <= 0.01 * 2 * b, ambiguous
    assert torch.all(st.history[:, :2] == -1) and torch.all(st.history[:, 4:] == -1)
    assert st.step.item() == 4 and st.slot.item() == 42 and st.kvl.item() == 43
    assert st.counter.item() == 0 and st.ctl[5].item() == 0
    assert torch.equal(st.pos, torch.arange(b, device=DEV) + 12)


def _crowded_logits():
    """fp32 rows whose values all fall into one or two 12-bit key bins."""
    g = torch.Generator().manual_seed(99)
    return (1.0 + 0.12 * torch.rand(4, 8192, generator=g)).to(DEV)


@pytest.mark.parametrize("kw", [dict(top_k=50), dict(top_p=0.9),
                                dict(top_p=0.5, temperature=0.7)])
def test_sample_tail_crowded_threshold_bin(kw):
    """Thousands of elements share the threshold's 12-bit key bin, more than
    the kernel's LDS candidate list holds (2048): the lower digits of the
    threshold and the last draws then run on the row again."""
    from epfl_megatron_amd.ops.sampling import sample_ref
    logits = _crowded_logits()
    st = _Tail(4, **kw)
    ambiguous = 0
    for it in range(2):
        got = st.run(logits).cpu()
        _, kept, sets = sample_ref(logits, SEED, OFFSET, step=2 + it, return_kept=True,
                                   return_sets=True, **kw)
        assert (kept.sum(1) > 2048).all() or "top_k" in kw
        for r in range(4):
            assert int(got[r]) in sets[r], (r, it, int(got[r]), sets[r])
        ambiguous += sum(len(s) > 1 for s in sets)
    assert ambiguous == 0
    assert st.step.item() == 4 and st.counter.item() == 0


@pytest.mark.parametrize("b,V,dtype", SHAPES[:4])
def test_sample_tail_top_k_1_is_greedy_tail(b, V, dtype):
    logits = _logits(b, V, dtype, 3 * b + V)
    logits[:, V // 3] = logits.max(1).values  # a tied maximum: the first index wins
    greedy = _Tail(b)
    _ext().greedy_tail(logits, greedy.tokens, greedy.history, greedy.step, greedy.pos,
                       greedy.slot, greedy.kvl, greedy.counter)
    st = _Tail(b, top_k=1)
    assert torch.equal(st.run(logits), greedy.tokens)
    assert torch.equal(st.tokens, logits.float().argmax(1))
    assert torch.equal(st.history, greedy.history) and torch.equal(st.pos, greedy.pos)
    limit = int(greedy.tokens.min()) + 1  # the clamp to the unpadded vocabulary
    st = _Tail(b, top_k=1, vocab_limit=limit)
    assert torch.equal(st.run(logits), greedy.tokens.clamp(max=limit - 1))


@pytest.mark.parametrize("kw", [dict(top_p=0.9, temperature=0.8), dict(top_k=50), dict()])
def test_sample_tail_is_deterministic(kw):
    logits = _logits(8, 32000, torch.bfloat16, 17)
    runs = [_Tail(8, **kw).run(logits) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert runs[0].unique().numel() > 1


def test_sample_tail_stop_token():
    b, V, stop = 6, 1003, 7
    logits = _logits(b, V, torch.bfloat16, 23)
    fed = torch.tensor([3, stop, 3, 3, stop, 3])
    free = _Tail(b, top_p=0.9, tokens=fed)
    base = free.run(logits)
    st = _Tail(b, top_p=0.9, stop_id=stop, tokens=fed)
    got = st.run(logits)
    assert got[1].item() == stop and got[4].item() == stop
    others = [0, 2, 3, 5]
    assert torch.equal(got[others], base[others])
    assert st.ctl[5].item() == int((got == stop).sum()) >= 2
    assert free.ctl[5].item() == 0
    assert torch.equal(st.history[:, 2], got) and torch.equal(st.pos, free.pos)
    assert st.step.item() == 3 and st.counter.item() == 0


def test_sample_fused_matches_reference():
    from epfl_megatron_amd.ops.sampling import sample_fused, sample_ref
    x = _logits(3, 1003, torch.bfloat16, 5).contiguous()  # 2006-byte rows: the padded copy
    for kw in (dict(top_k=8, temperature=0.7), dict(top_p=0.5), dict(top_k=1)):
        got = sample_fused(x, vocab_size=1000, seed_offset=(SEED, OFFSET), **kw).cpu()
        _, sets = sample_ref(x, SEED, OFFSET, vocab_size=1000, return_sets=True, **kw)
        assert all(int(t) in s for t, s in zip(got, sets)), (got, sets)
    y = _logits(64, 4096, torch.float32, 6)
    torch.manual_seed(3)
    a, b = sample_fused(y, top_p=0.9), sample_fused(y, top_p=0.9)
    torch.manual_seed(3)
    assert torch.equal(a, sample_fused(y, top_p=0.9))  # the generator's (seed, offset)
    assert not torch.equal(a, b)                      # ... which every call advances


def _graph_sample(rank, world):
    """GraphedSamplingDecoder on the tiny GQA Llama: after every replay the
    token in the history and the one fed back must be the reference's draw
    from the logits of that very replay (the in-graph wiring, without
    comparing two numerically different forwards)."""
    import finetune
    from test_gpu_e2e import LLAMA_GQA
    from test_parallel_equivalence import _deterministic_init
    init_framework(LLAMA_GQA + ["--bf16"], finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedSamplingDecoder
    from epfl_megatron_amd.ops.sampling import sample_ref
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, get_args())
    m = model[0].eval()
    torch.manual_seed(5)
    b, plen, n, cap = 2, 29, 10, 600
    prompt = torch.randint(0, 512, (b, plen), device="cuda")
    pos = torch.arange(cap, device="cuda")[None].expand(b, -1)
    with torch.no_grad():
        ip = InferenceParams(b, cap)
        nxt = m(prompt, pos[:, :plen], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
        ip.sequence_len_offset += plen
        first = nxt.clone()
        eager = []
        for t in range(plen, plen + n):
            nxt = m(nxt, pos[:, t:t + 1], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
            eager.append(nxt)
            ip.sequence_len_offset += 1
        eager = torch.cat(eager, dim=1)
        ip2 = InferenceParams(b, cap)
        m(prompt, pos[:, :plen], None, inference_params=ip2)
        ip2.sequence_len_offset += plen
    dec = GraphedSamplingDecoder(m, ip2, b, n, vocab_size=512)
    kw = dict(top_p=0.9, temperature=1.3)

    def generate(check, **kw):
        dec.start(first, plen, **kw)
        bad = []
        for s in range(n):
            dec.step()
            if check:
                _, sets = sample_ref(dec.logits[:, -1], dec.seed, dec.offset0, step=s,
                                     vocab_size=512, return_sets=True, **kw)
                for r in range(b):
                    tok = int(dec.history[r, s])
                    if tok not in sets[r] or int(dec.tokens[r, 0]) != tok:
                        bad.append((s, r, tok, int(dec.tokens[r, 0]), sets[r]))
        return dec.history[:, :n].cpu().tolist(), bad

    torch.manual_seed(77)
    run1, bad = generate(True, **kw)
    graph = dec.graph
    greedy, _ = generate(False, top_k=1)
    torch.manual_seed(77)
    run2, _ = generate(False, **kw)
    run3, _ = generate(False, **kw)  # the generator moved on: a fresh draw
    return (bad, run1, run2, run3, greedy, eager.cpu().tolist(), dec.graph is graph,
            dec.n_stopped)


def test_gpu_graphed_sampling_decoder():
    bad, run1, run2, run3, greedy, eager, same_graph, n_stopped = run_dist(_graph_sample, 1)[0]
    assert not bad, bad
    assert same_graph and n_stopped == 0
    assert greedy == eager
    assert run2 == run1
    assert run3 != run1


def _gen_api(rank, world):
    """One process: started with ``--inference_fused_sampling``; the run
    "without the flag" is the same model with the parsed flag switched off."""
    from test_gpu_e2e import LLAMA_GQA
    from test_inference import _setup, PROMPTS
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.inference import generate_and_post_process
    argv = LLAMA_GQA + ["--bf16", "--micro_batch_size", "1", "--global_batch_size", "1",
                        "--distributed_backend", "nccl", "--inference_fused_sampling"]
    try:
        model = _setup(argv)
    except SystemExit as e:
        # an unknown flag makes argparse exit: run_dist only hears of exceptions,
        # and would wait for this rank's result for ever
        raise RuntimeError(f"argument parsing exited with {e.code}")
    assert get_args().inference_fused_sampling is True
    kw = dict(model=model, prompts=PROMPTS, tokens_to_generate=8,
              use_eod_token_for_early_termination=False)
    fused = generate_and_post_process(top_k_sampling=1, **kw)[3]
    sampled = [generate_and_post_process(top_p_sampling=0.9, random_seed=5, **kw)[3]
               for _ in range(2)]
    get_args().inference_fused_sampling = False
    plain = generate_and_post_process(top_k_sampling=1, **kw)[3]
    return fused, plain, sampled


def test_gpu_generation_api_fused_sampling():
    fused, plain, (a, b) = run_dist(_gen_api, 1)[0]
    assert fused == plain
    assert a == b
    assert all(0 <= t < 512 for seq in a for t in seq)
