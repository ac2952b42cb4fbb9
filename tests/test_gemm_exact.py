"""CPU self-test of the bitwise integer-operand GEMM checks
(``gemm_exact_inputs.py``), for exactly the cases ``test_gemm_exact_gpu.py``
runs on the kernels:

(a) every case meets its exactness bounds (worst-case |sum| < 2^24 quanta,
    fp16 outputs in range), and the expected split plans are what the
    transcribed ``nt_ksplit`` / ``best_split`` give (and what the extension's
    host functions give, when it imports: they fix the CU count at 256);
(b) a plain-torch fp32 emulation of the decompositions (K in steps of 32 / 64
    and in split ranges, tokens in 32-row subtiles and split ranges, both row
    map formulas) equals the fp64 reference bitwise on every case, so the
    method holds whatever the order of accumulation;
(c) every mutant of the emulation is flagged by the check the GPU file uses;
(d) the rounding mutants are only visible where the integer does not fit the
    output's significand: the long-K bf16 cases have >= 10 % of elements
    inexact in bf16 and >= 5 % exact ties (conditions on the cases);
(e) an fp32 emulation of ``act_math.h`` stays inside the SwiGLU / GeGLU
    tolerance with no element excluded.
"""
import pytest
import torch

import gemm_exact_inputs as G

DT = pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)


def _ext_or_none():
    try:
        from epfl_megatron_amd.ops._ext import ext
        return ext()
    except Exception:  # not built here: the transcription alone is checked
        return None


# ---------------------------------------------------------------- (a) bounds and plans

def test_every_case_meets_its_exactness_bounds():
    for dtype in G.DTYPES:
        ks = [K for _, _, K, _ in G.NT_PLAIN] + [K for _, _, K, _ in G.NT_SPLITK]
        ks += [K for *_, K in G.NT_ROW_MAPS] + [G.NT_STRIDED["K"]]
        for K in ks:
            assert G.check_bound(G.bound(K, *G.nt_range(dtype, K)), 0, dtype)
        for M, F, K, wmax, shift in G.GLU_SHAPES + (tuple(G.GLU_CMAP[k] for k in ("R", "F", "K", "wmax", "shift")),):
            assert G.check_bound(G.bound(K, *G.GLU_ACT, -wmax, wmax), shift, dtype)
        for N, K in G.SKINNY_NK:
            assert G.check_bound(G.bound(K, G.SK_LO, G.SK_HI, extra=G.SK_RES), 0, dtype)
    ms = [M for M, _, _ in G.WGRAD_SHAPES] + [s[0] for s, _ in G.WGRAD_PLANS]
    ms += [w * c * R for w, c, R, _, _ in G.WGRAD_TOKMAPS] + [16384]
    for M in ms:
        assert G.check_bound(G.bound(M, G.WG_LO, G.WG_HI, extra=G.WG_G0))
    # the issue's figure for the census operands: |sum| <= 1610 at K = 8192 in [-3, 3]
    a, b = G.nt_case(*G.NT_CENSUS, G.BF16)
    assert G.ref_nt(a, b).abs().max() <= 1610


def test_expected_plans_match_the_transcribed_rules():
    C = _ext_or_none()
    for M, N, K, sp in G.NT_SPLITK:
        assert G.nt_ksplit(M, N, K) == sp, (M, N, K)
        if C is not None:
            assert C.gemm_nt_ksplit(M, N, K) == sp, (M, N, K)
    for tp, c, R, N, K in G.NT_ROW_MAPS:  # the K = 1024 map case really splits
        assert G.nt_ksplit(tp * R, N, K) == (2 if K == 1024 else 1)
    for (M, N, K), plan in G.WGRAD_PLANS:
        assert G.wgrad_plan(M, N, K) == plan, (M, N, K)
        if C is not None:
            assert list(C.wgrad_plan(M, N, K)) == plan, (M, N, K)
    for M, N, K in G.WGRAD_SHAPES:
        assert G.wgrad_plan(M, N, K)[3] == 1
    w, c, R, N, K = G.WGRAD_TOKMAPS[1]
    assert G.wgrad_plan(w * c * R, N, K)[3] > 1  # the split path with a map
    if C is not None:  # the plans the suite already pins, through the transcription
        for shape in ((16384, 22016, 4096), (16384, 4352, 4096), (16384, 1536, 512), (1024, 768, 512),
                      (16384, 2752, 4096), (16384, 4096, 512)):
            assert list(C.wgrad_plan(*shape)) == G.wgrad_plan(*shape), shape


def test_row_and_token_map_formulas():
    """Both formulas of kernels.h against the views the layers use."""
    from epfl_megatron_amd.parallel.tensor.layers import _apply_token_map, _rows_view
    tp, c, R = 4, 2, 200
    full = torch.arange(tp * c * R * 3).view(tp * c * R, 3)
    for j in range(c):
        got = full[G.row_map_index(tp * R, (R, c * R, j * R))]
        assert torch.equal(got, _rows_view(full, (R, c * R, j * R), tp * R).reshape(tp * R, 3))
    for world, c, R, _, _ in G.WGRAD_TOKMAPS:
        M = world * c * R
        x = torch.arange(M * 2).view(M, 2)
        for xm in G.wgrad_tokmaps(world, c, R):
            idx = G.tok_map_index(M, xm)
            assert torch.equal(x[idx], _apply_token_map(x, tuple(xm), M))
            assert sorted(idx.tolist()) == list(range(M))  # a permutation


# ---------------------------------------------------------------- (b), (c): NT

def _flagged(out, expected):
    return not G.exact_ok(out, expected)


@DT
@pytest.mark.parametrize("M,N,K", [c[:3] for c in G.NT_PLAIN], ids=lambda v: str(v))
def test_nt_emulation_is_bitwise_and_mutants_are_flagged(M, N, K, dtype):
    a, b = G.nt_case(M, N, K, dtype)
    e = G.expect16(G.ref_nt(a, b), dtype)
    assert G.exact_ok(G.emulate_nt(a, b), e)
    assert _flagged(G.emulate_nt(a, b, mutant="kstep_dropped"), e)
    if (M, N, K) == G.NT_CENSUS and dtype == G.BF16:  # fp16 holds these integers exactly
        assert _flagged(G.emulate_nt(a, b, mutant="truncate"), e)


@DT
@pytest.mark.parametrize("M,N,K,sp", G.NT_SPLITK)
def test_nt_split_emulation_is_bitwise_and_mutants_are_flagged(M, N, K, sp, dtype):
    a, b = G.nt_case(M, N, K, dtype)
    e = G.expect16(G.ref_nt(a, b), dtype)
    assert G.exact_ok(G.emulate_nt(a, b, sp), e)
    assert _flagged(G.emulate_nt(a, b, sp, mutant="kstep_dropped"), e)
    if sp > 1:
        assert _flagged(G.emulate_nt(a, b, sp, mutant="split_twice"), e)
        assert _flagged(G.emulate_nt(a, b, sp, mutant="split_omitted"), e)
    if K >= 4096 and dtype == G.BF16:
        assert _flagged(G.emulate_nt(a, b, sp, mutant="truncate"), e)


@DT
@pytest.mark.parametrize("tp,c,R,N,K", G.NT_ROW_MAPS)
def test_nt_row_map_emulation_is_bitwise_and_mutants_are_flagged(tp, c, R, N, K, dtype):
    full, b = G.nt_case(tp * c * R, N, K, dtype)
    sp = G.nt_ksplit(tp * R, N, K)
    for j in range(c):
        amap = (R, c * R, j * R)
        e = G.expect16(G.ref_nt(full.view(tp, c, R, K)[:, j].reshape(tp * R, K), b), dtype)
        assert G.exact_ok(G.emulate_nt(full, b, sp, amap, tp * R), e)
        assert _flagged(G.emulate_nt(full, b, sp, amap, tp * R, mutant="neighbour_group"), e)
        # a wrong row in one group only: group 1 of the output read from the neighbour
        mixed = G.emulate_nt(full, b, sp, amap, tp * R)
        mixed[R:R + 1] = G.emulate_nt(full, b, sp, amap, tp * R, mutant="neighbour_group")[R:R + 1]
        assert _flagged(mixed, e)


# ---------------------------------------------------------------- (d) the census conditions

def test_long_k_cases_exercise_rounding_and_ties():
    inexact, ties = G.census_shares(G.BF16)
    assert inexact >= 0.10 and ties >= 0.05, (inexact, ties)
    M, F, K, wmax, shift = G.GLU_INEXACT
    x, w1 = G.glu_case(M, F, K, wmax, shift, G.BF16)
    inexact, _ = G.inexact_share(G.ref_nt(x, w1), G.BF16)
    assert inexact >= 0.10, inexact


# ---------------------------------------------------------------- (b), (c), (e): GLU

@DT
@pytest.mark.parametrize("M,F,K,wmax,shift", G.GLU_SHAPES)
def test_glu_inputs_reach_the_curved_part(M, F, K, wmax, shift, dtype):
    x, w1 = G.glu_case(M, F, K, wmax, shift, dtype)
    pre = G.ref_nt(x, w1)
    assert 0.5 <= float(pre.std()) <= 2.0
    assert float((pre[:, F:].abs() < 4).double().mean()) >= 0.5


@DT
@pytest.mark.parametrize("kind", list(G.KINDS))
@pytest.mark.parametrize("M,F,K,wmax,shift", G.GLU_SHAPES)
def test_glu_emulation_passes_and_mutants_are_flagged(M, F, K, wmax, shift, kind, dtype):
    x, w1 = G.glu_case(M, F, K, wmax, shift, dtype)
    pre_e = G.expect16(G.ref_nt(x, w1), dtype)
    e, s, x2 = G.glu_expected(pre_e, kind)
    pre, y = G.emulate_glu(x, w1, kind)
    assert G.exact_ok(pre, pre_e)
    ok, margin = G.glu_ok(y, e, s, x2, kind)
    assert ok, margin
    assert margin <= G.GLU_FACTOR
    pre_m, y_m = G.emulate_glu(x, w1, kind, "kstep_dropped")
    assert _flagged(pre_m, pre_e)
    if kind != "liglu":  # x1 x2 is symmetric: nothing to swap
        _, y_m = G.emulate_glu(x, w1, kind, "x1_x2_swapped")
        assert not G.glu_ok(y_m, e, s, x2, kind)[0]
    if (M, F, K, wmax, shift) == G.GLU_INEXACT and dtype == G.BF16:
        pre_m, _ = G.emulate_glu(x, w1, kind, "truncate")
        assert _flagged(pre_m, pre_e)
        _, y_m = G.emulate_glu(x, w1, kind, "y_from_unrounded")
        assert not G.glu_ok(y_m, e, s, x2, kind)[0]


@DT
@pytest.mark.parametrize("kind", list(G.KINDS))
@pytest.mark.parametrize("M,F,K,wmax,shift", G.GLU_SHAPES)
def test_dglu_emulation_passes(M, F, K, wmax, shift, kind, dtype):
    dy, w2t, pre = G.dglu_case(M, F, K, wmax, shift, dtype)
    g = G.expect16(G.ref_nt(dy, w2t), dtype)
    e, s, x2 = G.dglu_expected(g, pre, kind)
    d = G.emulate_dglu(dy, w2t, pre, kind)
    ok, margin = G.glu_ok(d, e, s, x2, kind)
    assert ok, margin
    assert margin <= G.GLU_FACTOR
    # the halves swapped (the gate half written where the up half belongs)
    swapped = torch.cat([d[:, F:], d[:, :F]], dim=1)
    assert not G.glu_ok(swapped, e, s, x2, kind)[0]


# ---------------------------------------------------------------- (b), (c): wgrad

def _wgrad_check(M, N, K, dtype, nsplit, x_map=None, xrows=None):
    dy, x, g0 = G.wgrad_case(M, N, K, dtype, xrows=xrows)
    xp = x[G.tok_map_index(M, x_map)]
    nan = torch.full((N, K), float("nan"))
    e_acc, e_st = G.ref_wgrad(dy, xp, g0).float(), G.ref_wgrad(dy, xp).float()
    assert G.exact_ok(G.emulate_wgrad(dy, x, g0, True, nsplit, x_map), e_acc)
    assert G.exact_ok(G.emulate_wgrad(dy, x, nan, False, nsplit, x_map), e_st)
    return dy, x, g0, nan, e_acc, e_st


@DT
@pytest.mark.parametrize("M,N,K", G.WGRAD_SHAPES + tuple(s for s, _ in G.WGRAD_PLANS[:-1]))
def test_wgrad_emulation_is_bitwise_and_mutants_are_flagged(M, N, K, dtype):
    nsplit = G.wgrad_plan(M, N, K)[3]
    dy, x, g0, nan, e_acc, e_st = _wgrad_check(M, N, K, dtype, nsplit)
    muts = ["subtile_dropped", "acc_as_store"] + (["split_twice", "split_omitted"] if nsplit > 1 else [])
    for m in muts:
        assert _flagged(G.emulate_wgrad(dy, x, g0, True, nsplit, mutant=m), e_acc), m
    assert _flagged(G.emulate_wgrad(dy, x, nan, False, nsplit, mutant="store_as_acc"), e_st)
    # a store that leaves the old content (integers, not NaN) in place is flagged too
    assert _flagged(G.emulate_wgrad(dy, x, g0, False, nsplit, mutant="store_as_acc"), e_st)


def test_wgrad_emulation_whole_round_and_split_tail():
    """The largest case (17 x 16 tiles: a whole-tile round and a split tail), bf16."""
    (M, N, K), plan = G.WGRAD_PLANS[-1]
    _wgrad_check(M, N, K, G.BF16, plan[3])


@DT
@pytest.mark.parametrize("world,c,R,N,K", G.WGRAD_TOKMAPS)
def test_wgrad_token_map_emulation_is_bitwise(world, c, R, N, K, dtype):
    M = world * c * R
    for xm in G.wgrad_tokmaps(world, c, R):
        _wgrad_check(M, N, K, dtype, G.wgrad_plan(M, N, K)[3], xm)


# ---------------------------------------------------------------- skinny, wiring

@DT
@pytest.mark.parametrize("N,K", G.SKINNY_NK)
def test_skinny_residual_expectation_rounds_twice(N, K, dtype):
    """The residual epilogue is Y = T(T(acc) + R) (csrc/skinny_gemm.hip): the
    two roundings must differ from one somewhere, or the case cannot tell them
    apart (bf16 at K = 4096: |acc| goes past 256)."""
    x, w, res = G.skinny_case(16, N, K, dtype)
    ref = G.ref_nt(x, w)
    twice = G.expect16(G.expect16(ref, dtype).double() + res.double(), dtype)
    once = G.expect16(ref + res.double(), dtype)
    if dtype == G.BF16 and K == 4096:
        assert not torch.equal(twice, once)


@DT
@pytest.mark.parametrize("kind", G.EXACT_KINDS)
def test_wiring_chain_is_exact(kind, dtype):
    """Every GEMM of the MLP and linear wiring cases is exact in fp32 on the
    data it really gets (the rounded outputs of the GEMM before it)."""
    w = G.wire_mlp_expected(kind, dtype)
    assert w["checked"] == 6 * G.WIRE_MICROBATCHES
    lin = G.wire_linear_expected(dtype)
    assert lin["checked"] == 3 * G.WIRE_MICROBATCHES


# ---------------------------------------------------------------- (c) the mutant table in one place

def test_every_listed_mutant_is_flagged():
    """One line per mutant the method must catch, each on the smallest case
    that can show it, each through the check the GPU file uses."""
    bf = G.BF16
    a, b = G.nt_case(300, 264, 192, bf)
    e = G.expect16(G.ref_nt(a, b), bf)
    flagged = {"one K-step dropped in one strip of one tile": _flagged(G.emulate_nt(a, b, mutant="kstep_dropped"), e)}
    a, b = G.nt_case(512, 256, 1536, bf)
    e = G.expect16(G.ref_nt(a, b), bf)
    flagged["one K split counted twice"] = _flagged(G.emulate_nt(a, b, 3, mutant="split_twice"), e)
    flagged["one K split omitted"] = _flagged(G.emulate_nt(a, b, 3, mutant="split_omitted"), e)
    tp, c, R, N, K = G.NT_ROW_MAPS[2]
    full, b = G.nt_case(tp * c * R, N, K, bf)
    e = G.expect16(G.ref_nt(full.view(tp, c, R, K)[:, 0].reshape(tp * R, K), b), bf)
    flagged["row-map group read from its neighbour"] = _flagged(
        G.emulate_nt(full, b, 1, (R, c * R, 0), tp * R, mutant="neighbour_group"), e)
    a, b = G.nt_case(*G.NT_CENSUS, bf)
    flagged["truncation on the 16-bit store"] = _flagged(G.emulate_nt(a, b, mutant="truncate"),
                                                         G.expect16(G.ref_nt(a, b), bf))
    x, w1 = G.glu_case(*G.GLU_INEXACT, bf)
    e, s, x2 = G.glu_expected(G.expect16(G.ref_nt(x, w1), bf), "reglu")
    flagged["y from the unrounded accumulator"] = not G.glu_ok(
        G.emulate_glu(x, w1, "reglu", "y_from_unrounded")[1], e, s, x2, "reglu")[0]
    flagged["x1 / x2 swapped in the GLU epilogue"] = not G.glu_ok(
        G.emulate_glu(x, w1, "reglu", "x1_x2_swapped")[1], e, s, x2, "reglu")[0]
    dy, x, g0 = G.wgrad_case(4096, 256, 256, bf)
    nan = torch.full_like(g0, float("nan"))
    e_acc, e_st = G.ref_wgrad(dy, x, g0).float(), G.ref_wgrad(dy, x).float()
    flagged["one 32-token subtile dropped"] = _flagged(G.emulate_wgrad(dy, x, g0, True, 2, mutant="subtile_dropped"), e_acc)
    flagged["one token split counted twice"] = _flagged(G.emulate_wgrad(dy, x, g0, True, 2, mutant="split_twice"), e_acc)
    flagged["one token split omitted"] = _flagged(G.emulate_wgrad(dy, x, g0, True, 2, mutant="split_omitted"), e_acc)
    flagged["accumulate done as store"] = _flagged(G.emulate_wgrad(dy, x, g0, True, 2, mutant="acc_as_store"), e_acc)
    flagged["store done as accumulate"] = _flagged(G.emulate_wgrad(dy, x, nan, False, 2, mutant="store_as_acc"), e_st)
    assert all(flagged.values()), [k for k, v in flagged.items() if not v]
