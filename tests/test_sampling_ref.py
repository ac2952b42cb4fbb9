"""Fused sampling (ops/sampling.py) without a GPU: the fp64 reference of the
``sample_tail_k`` kernel against ``inference/sampling.py``'s filters and
against the distribution it must draw from, the TP seed broadcast of
``GraphedSamplingDecoder`` and ``--inference_fused_sampling`` through the
text-generation API on gloo (where ``sample_fused`` runs the reference)."""
import numpy as np
import pytest
import torch

from dist_utils import run_dist, init_framework

SEED, OFFSET = 0x1234ABCD5678, 40


def _distinct_rows(b, V, gen):
    """fp32 rows of V distinct values in [-6, 6) in random order."""
    rows = [torch.randperm(V, generator=gen).float() * (12.0 / V) - 6.0 for _ in range(b)]
    return torch.stack(rows)


@pytest.mark.parametrize("top_k", [2, 8, 50])
def test_ref_top_k_kept_set(top_k):
    from epfl_megatron_amd.inference.sampling import modify_logits_for_top_k_filtering
    from epfl_megatron_amd.ops.sampling import sample_ref
    x = _distinct_rows(4, 1003, torch.Generator().manual_seed(top_k))
    _, kept = sample_ref(x, SEED, OFFSET, top_k=top_k, return_kept=True)
    want = x.double()
    modify_logits_for_top_k_filtering(want, top_k)
    assert np.array_equal(kept, torch.isfinite(want).numpy())
    assert (kept.sum(1) == top_k).all()
    # the k-th value three times: all three stay (the ``logits < kth`` rule)
    order = x[0].argsort(descending=True)
    x[0, order[top_k]] = x[0, order[top_k - 1]]
    x[0, order[top_k + 1]] = x[0, order[top_k - 1]]
    _, kept = sample_ref(x, SEED, OFFSET, top_k=top_k, return_kept=True)
    want = x.double()
    modify_logits_for_top_k_filtering(want, top_k)
    assert np.array_equal(kept, torch.isfinite(want).numpy())
    assert kept[0].sum() == top_k + 2 and kept[0, order[top_k - 1:top_k + 2]].all()


@pytest.mark.parametrize("top_p", [0.05, 0.5, 0.9, 1.0])
def test_ref_top_p_kept_set(top_p):
    from epfl_megatron_amd.inference.sampling import modify_logits_for_top_p_filtering
    from epfl_megatron_amd.ops.sampling import sample_ref
    x = _distinct_rows(4, 1003, torch.Generator().manual_seed(7))
    _, kept = sample_ref(x, SEED, OFFSET, top_p=top_p, return_kept=True)
    want = x.double()  # fp64, so the filter's own cumsum rounding stays far from p
    modify_logits_for_top_p_filtering(want, float(np.float32(top_p)))
    assert np.array_equal(kept, torch.isfinite(want).numpy())
    assert kept.all() if top_p == 1.0 else not kept.all()


def test_ref_greedy_and_clamp():
    from epfl_megatron_amd.ops.sampling import sample_ref, sample_fused
    x = torch.randn(6, 300, generator=torch.Generator().manual_seed(1))
    x[:, 120] = x.max(1).values  # a tied maximum: the first index wins
    assert torch.equal(sample_ref(x, SEED, OFFSET, top_k=1), x.argmax(1))
    assert torch.equal(sample_ref(x, SEED, OFFSET, top_k=1, vocab_size=5),
                       x.argmax(1).clamp(max=4))
    assert int(sample_ref(x, SEED, OFFSET, top_p=0.9, vocab_size=3).max()) <= 2
    assert torch.equal(sample_fused(x, top_k=1), x.argmax(1))
    # a -inf logit is never drawn while a finite one exists
    y = torch.full((64, 8), float("-inf"))
    y[:, 5] = -3.0
    assert sample_ref(y, SEED, OFFSET).tolist() == [5] * 64
    with pytest.raises(AssertionError):
        sample_fused(x, top_k=2, top_p=0.5)
    with pytest.raises(AssertionError):
        sample_fused(x, top_k=301)
    with pytest.raises(AssertionError):
        sample_fused(x, top_p=1.5)


def test_ref_uniforms():
    from epfl_megatron_amd.ops.sampling import philox_uniform, sample_ref
    u = philox_uniform(3, 1003, SEED, OFFSET, step=2)
    assert u.shape == (3, 1003) and (u > 0).all() and (u < 1).all()
    assert np.array_equal(u, philox_uniform(3, 1003, SEED, OFFSET, step=2))
    assert np.array_equal(u, philox_uniform(3, 1003, SEED, OFFSET + 2, step=0))
    assert not np.array_equal(u, philox_uniform(3, 1003, SEED, OFFSET, step=3))
    assert not np.array_equal(u[0], u[1])
    # the extreme words stay inside (0, 1) (fp64 holds (n + 0.5) * 2^-24 exactly)
    for w, want in ((0, 2.0 ** -25), (0xFFFFFFFF, 1 - 2.0 ** -25)):
        assert ((w >> 8) + 0.5) * 2.0 ** -24 == want
    x = torch.randn(32, 257, generator=torch.Generator().manual_seed(2))
    a = sample_ref(x, SEED, OFFSET, step=1)
    assert torch.equal(a, sample_ref(x, SEED, OFFSET, step=1))
    assert not torch.equal(a, sample_ref(x, SEED, OFFSET, step=2))


@pytest.mark.parametrize("V,kw", [(1003, dict(top_k=8, temperature=0.8)), (64, dict(top_p=0.9))])
def test_ref_chi_square(V, kw):
    """8192 draws (rows of one repeated logit row, fixed seed) against the
    softmax over the kept set; threshold: the 1 - 1e-6 chi-square quantile."""
    from scipy.stats import chi2
    from epfl_megatron_amd.ops.sampling import sample_ref
    n = 8192
    row = torch.randn(V, generator=torch.Generator().manual_seed(V)) * 2.0
    tok, kept = sample_ref(row[None].expand(n, V), SEED, OFFSET, return_kept=True, **kw)
    keep = kept[0]
    assert (kept == keep).all()
    if "top_k" in kw:
        assert keep.sum() == 8
    y = row.double().numpy() / np.float64(np.float32(kw.get("temperature", 1.0)))
    prob = np.where(keep, np.exp(y - y.max()), 0.0)
    prob /= prob.sum()
    obs = np.bincount(tok.numpy(), minlength=V)
    assert obs[~keep].sum() == 0
    stat = float((((obs - n * prob) ** 2)[keep] / (n * prob[keep])).sum())
    dof = int(keep.sum()) - 1
    limit = float(chi2.ppf(1 - 1e-6, dof))
    if dof == 7:
        assert limit == pytest.approx(40.5, abs=0.1)
    print(f"chi2 {stat:.2f} dof {dof} limit {limit:.1f}")
    assert stat < limit, (stat, dof, limit)


def _bcast(rank, world):
    import finetune
    from dist_utils import TINY_LLAMA
    init_framework(TINY_LLAMA + ["--tensor_model_parallel_size", "2", "--micro_batch_size", "1",
                                 "--global_batch_size", "1"], finetune.extra_args)
    from epfl_megatron_amd.inference.hip_graph import broadcast_seed_offset
    return broadcast_seed_offset(1000 + rank, 8 * (rank + 1), torch.device("cpu"))


def test_tp_seed_broadcast():
    assert [tuple(r) for r in run_dist(_bcast, 2)] == [(1000, 8), (1000, 8)]


def _gen(rank, world, extra, kw):
    from test_inference import _setup, _argv, PROMPTS
    try:
        model = _setup(_argv(extra))
    except SystemExit as e:
        # an unknown flag makes argparse exit: run_dist only hears of exceptions,
        # and would wait for this rank's result for ever
        raise RuntimeError(f"argument parsing exited with {e.code}: {extra}")
    from epfl_megatron_amd.inference import generate_and_post_process
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        outs.append(generate_and_post_process(model, prompts=PROMPTS, tokens_to_generate=6,
                                              use_eod_token_for_early_termination=False,
                                              **kw)[3])
    return outs


def test_api_fused_sampling_flag():
    flag = ["--inference_fused_sampling"]
    fused = run_dist(_gen, 1, flag, dict(top_k_sampling=1))[0]
    plain = run_dist(_gen, 1, [], dict(top_k_sampling=1))[0]
    assert fused[0] == plain[0]
    a, b = run_dist(_gen, 1, flag, dict(top_p_sampling=0.9, temperature=1.5))[0]
    assert a == b
    assert all(0 <= t < 250 for seq in a for t in seq)
    assert a != plain[0]  # (sampled at T = 1.5: not the greedy continuation)
