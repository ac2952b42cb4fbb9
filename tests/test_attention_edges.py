"""CPU self-test of the exact mask-edge checks (``attention_edge_inputs.py``),
for exactly the cases ``test_attention_edges_gpu.py`` runs on the kernels:

(a) plain-torch fp32 emulations of the decode algorithm (per-chunk max / sum /
    partial O, exp2, in-order combine) and of a tiled online-softmax forward
    pass every check, so the references alone stay inside the limits;
(b) every mutation of the visibility rule is rejected by those same checks,
    and each single-key mutant of a census case lies at least 3 ulps of the
    output type from the correctly rounded expectation (a condition on the
    cases, not a measurement: a case that violates it is changed, not the limit).

The emulations treat heads and sequences independently, so the head count
only moves the needle targets: r = 1 (four (batch, head) pairs: the four
single-key targets) and r = 12 (every target in every case) are run for
decode; the prefill masks do not depend on the heads at all, so the prefill
cases run with two KV groups (the 2^-g scaling) and, without document bounds,
one sequence.
"""
import functools

import pytest
import torch

import attention_edge_inputs as E

DTYPES = [torch.bfloat16, torch.float16]
MIN_SEPARATION_ULPS = 3.0
CPU_R = (1, 12)


@functools.lru_cache(maxsize=None)
def _mutant_vis(cap, mutant):
    rows = cap + E.DECODE_PAD_ROWS
    return torch.stack([E.decode_visibility(min(n, cap), w, rows, mutant) for n, w in E.decode_cases(cap)])


def test_decode_cases_cover_the_edges():
    """The case list holds what the checks are about: every length of the
    issue, kv_len past the capacity, and for each keys-per-wave a window edge
    one before, on and one after a chunk edge."""
    cases = E.decode_cases(600)
    assert {n for n, w in cases if w == 0} == set(E.DECODE_LENS[600]) and (605, 0) in cases
    assert {w for _, w in cases} == {0, *E.DECODE_WINDOWS[600]}
    klo = {max(min(n, 600) - w, 0) for n, w in cases if w}
    for chunk in (32, 64, 256):
        assert {chunk - 1, chunk, chunk + 1} <= klo, chunk
    assert len(cases) == len(set(cases))
    assert [E.DECODE_CONFIGS.count(c) for c in E.DECODE_CONFIGS] == [1] * 4
    assert [-(-cap // (4 * kpw)) for cap, kpw in E.DECODE_CONFIGS] == [19, 10, 3, 1]


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_emulation_passes_and_mutants_fail(dtype, hd, fp8):
    applied = {m: 0 for m in E.DECODE_MUTANTS + ("neighbours_swapped",)}
    needle_hits = dict(applied)
    for r in CPU_R:
        for cap in sorted({c for c, _ in E.DECODE_CONFIGS}):
            x = E.decode_inputs(dtype, hd, r, fp8, cap)
            # a condition on the inputs, not on the kernel
            assert x.min_target_weight >= 1 - 2.0 ** -20, x.min_target_weight
            for kpw in [k for c, k in E.DECODE_CONFIGS if c == cap]:
                what = f"r={r} cap={cap} kpw={kpw}"
                oc = E.decode_emulate(x, x.q_census, x.v_census, x.vis, kpw)
                on = E.decode_emulate(x, x.q_needle, x.v_needle, x.vis, kpw)
                assert E.census_ok(oc, x.census_e).all(), what
                assert E.needle_ok(on, x).all(), what
                zero = x.n_eff == 0
                assert not oc[zero].any() and not on[zero].any()  # exact zeros, not NaN
                for mut in E.DECODE_MUTANTS:
                    mvis = _mutant_vis(cap, mut)
                    moved = mvis ^ x.vis
                    applies = moved.any(1)
                    applied[mut] += int(applies.sum())
                    ok = E.census_ok(E.decode_emulate(x, x.q_census, x.v_census, mvis, kpw), x.census_e)
                    assert not (ok & applies).any(), f"{what} {mut}: census accepts a mutant"
                    if mut in E.DECODE_SINGLE_KEY_MUTANTS:
                        sep = E.census_separation(x.census_e, E.decode_census_expected(x, mvis), dtype)
                        assert (sep[applies] >= MIN_SEPARATION_ULPS).all(), (what, mut, sep[applies].min())
                    # the needle sees a mutant when one of the case's targets is a key it moved
                    hit = torch.gather(moved, 1, x.targets.view(len(moved), -1)).any(1)
                    needle_hits[mut] += int(hit.sum())
                    ok = E.needle_ok(E.decode_emulate(x, x.q_needle, x.v_needle, mvis, kpw), x)
                    assert not (ok & hit).any(), f"{what} {mut}: needle accepts a mutant"
                ok = E.needle_ok(E.decode_emulate(x, x.q_needle, x.v_needle, x.vis, kpw, v_swap=True), x)
                hit = x.t_visible.flatten(1).any(1)
                applied["neighbours_swapped"] += int(hit.sum())
                needle_hits["neighbours_swapped"] += int(hit.sum())
                assert not (ok & hit).any(), f"{what}: needle accepts swapped neighbours"
    assert all(v > 0 for v in applied.values()) and all(v > 0 for v in needle_hits.values()), \
        (applied, needle_hits)


def _prefill_case(dtype, hd, nq, nkv, b, case, applied, big=False):
    sq, sk, causal, window, docs = case
    vis, _ = E.prefill_visibility(b, sq, sk, causal, window, docs)
    q, k, v = E.prefill_census_inputs(b, sq, sk, nq, nkv, hd, dtype)
    e64, cnt = E.prefill_expected(v, vis, nq)
    o, lse = E.prefill_emulate(q, k, v, vis, hd ** -0.5)
    what = f"{case} nq={nq} nkv={nkv}"
    assert E.census_ok(o, e64).all(), what
    ok, err = E.lse_ok(lse, cnt)
    assert ok, (what, err)
    for mut in (("diag+1", "tile_dropped") if big else E.PREFILL_MUTANTS):
        mvis, _ = E.prefill_visibility(b, sq, sk, causal, window, docs, mut)
        if torch.equal(mvis, vis):
            continue
        applied[mut] += 1
        mo, mlse = E.prefill_emulate(q, k, v, mvis, hd ** -0.5)
        assert not E.census_ok(mo, e64).all(), f"{what} {mut}: O accepts a mutant"
        assert not E.lse_ok(mlse, cnt)[0], f"{what} {mut}: lse accepts a mutant"
        if mut != "tile_dropped":
            sep = E.census_separation(e64, E.prefill_expected(v, mvis, nq)[0], dtype)
            assert sep.max() >= MIN_SEPARATION_ULPS, (what, mut, sep.max())


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prefill_emulation_passes_and_mutants_fail(dtype, hd):
    applied = {m: 0 for m in E.PREFILL_MUTANTS}
    for case in E.prefill_cases():
        _prefill_case(dtype, hd, 2, 2, E.PREFILL_B if case[4] else 1, case, applied)
    assert all(v > 0 for v in applied.values()), applied


@pytest.mark.parametrize("s,hd", sorted({(c[1], c[4]) for c in E.PREFILL_BIG}))
def test_prefill_emulation_large_grids(s, hd):
    """The grids that pick the 8-wave, the split-key and the paired forward: the
    masks do not depend on the heads, so one head of one sequence is emulated."""
    applied = {m: 0 for m in E.PREFILL_MUTANTS}
    for case in E.prefill_big_cases(s):
        _prefill_case(torch.bfloat16, hd, 1, 1, 1, case, applied, big=True)
    assert applied["diag+1"] > 0 and applied["tile_dropped"] > 0


@pytest.mark.parametrize("hd", [64, 128])
def test_dv_emulation_passes_and_mutants_fail(hd):
    dtype, nq, nkv = torch.bfloat16, 4, 2  # two heads per group: their dO adds up
    applied = {m: 0 for m in E.PREFILL_MUTANTS}
    for case in E.dv_cases():
        sq, sk, causal, window, docs = case
        b = E.PREFILL_B if docs else 1
        vis, _ = E.prefill_visibility(b, sq, sk, causal, window, docs)
        q, k, v = E.prefill_census_inputs(b, sq, sk, nq, nkv, hd, dtype)
        dout = E.dv_census_dout(b, sq, nq, hd, dtype)
        ref = E.dv_expected(dout, vis, nkv)
        assert ref.max() > 0
        _, _, dv = E.prefill_emulate(q, k, v, vis, hd ** -0.5, dout=dout)
        assert E.dv_ok(dv, ref), case
        for mut in E.PREFILL_MUTANTS:
            mvis, _ = E.prefill_visibility(b, sq, sk, causal, window, docs, mut)
            if torch.equal(mvis, vis):
                continue
            applied[mut] += 1
            _, _, mdv = E.prefill_emulate(q, k, v, mvis, hd ** -0.5, dout=dout)
            assert not E.dv_ok(mdv, ref), f"{case} {mut}: dV accepts a mutant"
    assert all(v > 0 for v in applied.values()), applied


def test_census_values_layout():
    v = E.census_values(600, 128, 2)
    assert v.shape == (600, 2, 128) and torch.equal(v[:, 1], v[:, 0] / 2)
    assert torch.equal(v[:, 0, :64].sum(1), torch.ones(600)) and torch.equal(v[:, 0, 64:].sum(1), torch.ones(600))
    assert v[0, 0, 0] == 1 and v[9, 0, 0] == 1 and v[10, 0, 1] == 1 and v[65, 0, 65] == 1
    for dt in (torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        assert torch.equal(v.to(dt).float(), v)
    # length 1 (where a block census alone fails): one key, both halves set
    e1, e2 = E.census_expected(v, 0, 1), E.census_expected(v, 0, 2)
    assert e1[0, 0] == 1 and e1[0, 64] == 1 and e2[0, 0] == 1 and e2[0, 64] == 0.5 and e2[0, 65] == 0.5
