"""Exact mask-edge tests of the decode and FlashAttention kernels.

Uniform attention (Q = 0) turns the output into a census of the visible keys:
O = (visible keys per column) / (visible keys) with one rounding, lse =
ln(visible keys), both known from the mask rule alone, checked to 1 ulp with
no absolute tolerance.  Needle inputs put the whole softmax weight on one key
at a mask edge: a visible target gives its V row bit for bit, an invisible one
must not leak.  Inputs, cases, expectations and checks come from
``attention_edge_inputs.py``; ``test_attention_edges.py`` shows on the CPU that
a plain emulation passes them and every off-by-one mask mutant fails them.
"""
import pytest
import torch

import attention_edge_inputs as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def _decode(q, k, v, sc, kv_len=None, window=0, kpw=0):
    """ops.attention._flash_decode with the keys per wave forced."""
    from epfl_megatron_amd.ops.attention import _bsnd_strides
    b, _, nq, d = q.shape
    sk, nkv = k.shape[1], k.shape[2]
    out = torch.empty(b, 1, nq, d, dtype=q.dtype, device=q.device)
    _ext().flash_decode(q, k, v, out, b, sk, nq, nkv, d, list(_bsnd_strides(q, nq // nkv)),
                        list(_bsnd_strides(k, 1)[:3]), list(_bsnd_strides(v, 1)[:3]),
                        [out.stride(0), out.stride(1), out.stride(2)], d ** -0.5, kv_len,
                        kpw=kpw, window=window, kv_scale=sc)
    return out[:, 0]


def _failing(ok, cases):
    return [c for c, good in zip(cases, ok.tolist()) if not good][:8]


def _store(x, t):
    """The physical cache ``[cap + 8, b + 1, nkv, hd]`` in the cache type."""
    return t.to(torch.float8_e4m3fn).view(torch.uint8) if x.fp8 else t.to(x.dtype)


def _seqs(x, mem):
    """The strided inference view ``[b, cap, nkv, hd]`` (batch slot 0 is padding)."""
    return mem[:x.cap, 1:].transpose(0, 1)


def _poisoned(x, mem, n, klo):
    """Rows >= the length and the padding batch slot hold NaN (16-bit) or
    +-448 bytes (FP8: the production cache is zero-filled, NaN bytes are out
    of contract); rows below the window hold +-large finite values."""
    p = mem.clone()
    sign = torch.arange(x.hd, device=DEV) % 2 == 0
    if x.fp8:
        big = dead = torch.where(sign, 0x7e, 0xfe).to(torch.uint8)
    else:
        big = torch.where(sign, 3.0e4, -3.0e4).to(x.dtype)
        dead = torch.full((x.hd,), float("nan"), device=DEV, dtype=x.dtype)
    p[n:] = dead
    p[:, 0] = dead
    p[:klo] = big
    return p


def _check_decode(x, kpw, oc, on, what):
    ok = E.census_ok(oc, x.census_e)
    assert ok.all(), f"{what}: census off in cases (kv_len, window) {_failing(ok, x.cases)}"
    ok = E.needle_ok(on, x)
    assert ok.all(), f"{what}: needle off in cases (kv_len, window) {_failing(ok, x.cases)}"


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("r", E.DECODE_R)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_mask_edges(dtype, hd, r, fp8):
    """One (type, head_dim, heads per KV group, cache type) of the decode
    matrix: keys per wave forced to 8 / 16 / 64 over a 600-key cache (19, 10
    and 3 chunks) and 64 over a 200-key one (the one-chunk form), a device
    kv_len through every chunk edge (0: exact zeros; past the capacity: the
    capacity), windows whose edge lands before, on and after a chunk edge.
    Census and needle checks, inertness of the rows outside [klo, kv_len) and
    of the padding batch slot, and re-arming of the arrival counters (two
    launches bitwise equal; kv_len changes in place between launches)."""
    for cap in sorted({c for c, _ in E.DECODE_CONFIGS}):
        x = E.decode_inputs(dtype, hd, r, fp8, cap, DEV)
        assert x.min_target_weight >= 1 - 2.0 ** -20, x.min_target_weight  # on the inputs
        sc = torch.stack([x.k_scale, x.v_scale]).float().contiguous() if fp8 else None
        kmem, vcen, vndl = _store(x, x.k), _store(x, x.v_census), _store(x, x.v_needle)
        qc, qn = x.q_census, x.q_needle
        kpws = [k for c, k in E.DECODE_CONFIGS if c == cap]
        kv_len = torch.zeros(1, dtype=torch.int32, device=DEV)
        outs = {k: {name: [] for name in ("census", "needle", "census_p", "needle_p", "again")} for k in kpws}
        with torch.no_grad():
            for ci, (n, w) in enumerate(x.cases):
                n_eff, klo = int(min(n, cap)), int(max(min(n, cap) - w, 0) if w else 0)
                kp, vcp, vnp = (_poisoned(x, m, n_eff, klo) for m in (kmem, vcen, vndl))
                q1 = qn[ci].unsqueeze(1)
                kv_len.fill_(n)  # in place: the launches read it on the device
                for kpw in kpws:
                    o = outs[kpw]
                    o["census"].append(_decode(qc, _seqs(x, kmem), _seqs(x, vcen), sc, kv_len, w, kpw))
                    o["needle"].append(_decode(q1, _seqs(x, kmem), _seqs(x, vndl), sc, kv_len, w, kpw))
                    o["census_p"].append(_decode(qc, _seqs(x, kp), _seqs(x, vcp), sc, kv_len, w, kpw))
                    o["needle_p"].append(_decode(q1, _seqs(x, kp), _seqs(x, vnp), sc, kv_len, w, kpw))
                    o["again"].append(_decode(q1, _seqs(x, kmem), _seqs(x, vndl), sc, kv_len, w, kpw))
        for kpw in kpws:
            what = f"cap={cap} kpw={kpw}"
            o = {name: torch.stack(t) for name, t in outs[kpw].items()}
            _check_decode(x, kpw, o["census"], o["needle"], what)
            zero = x.n_eff == 0
            assert zero.any() and not o["census"][zero].any() and not o["needle"][zero].any(), what
            # .view(int16): bitwise, and NaN compares equal to itself
            bits = {name: t.view(torch.int16) for name, t in o.items()}
            assert torch.equal(bits["census_p"], bits["census"]), what + ": census reads rows outside [klo, kv_len)"
            assert torch.equal(bits["needle_p"], bits["needle"]), what + ": needle reads rows outside [klo, kv_len)"
            assert torch.equal(bits["again"], bits["needle"]), what + ": two launches differ"
            full, past = x.cases.index((cap, 0)), x.cases.index((cap + 5, 0))
            assert torch.equal(bits["census"][past], bits["census"][full])
            assert torch.equal(bits["needle"][past], bits["needle"][full])


def test_decode_checks_see_one_key():
    """The checks resolve one key of the kernel's own output: launched with a
    kv_len one short of the case's, every case fails both checks."""
    cap, kpw = 600, 16
    x = E.decode_inputs(torch.bfloat16, 128, 4, False, cap, DEV)
    kk, vc, vn = (_seqs(x, _store(x, t)) for t in (x.k, x.v_census, x.v_needle))
    kv_len = torch.zeros(1, dtype=torch.int32, device=DEV)
    oc, on = [], []
    with torch.no_grad():
        for ci, (n, w) in enumerate(x.cases):
            kv_len.fill_(max(min(n, cap) - 1, 0))
            oc.append(_decode(x.q_census, kk, vc, None, kv_len, w, kpw))
            on.append(_decode(x.q_needle[ci].unsqueeze(1), kk, vn, None, kv_len, w, kpw))
    short = x.n_eff >= 1
    assert short.sum() >= len(x.cases) - 8
    assert not E.census_ok(torch.stack(oc), x.census_e)[short].any()
    assert not E.needle_ok(torch.stack(on), x)[short].any()


@pytest.mark.parametrize("r", E.DECODE_R)
def test_decode_auto_dispatch(r):
    """The public entries on the automatic keys-per-wave path pass the same
    checks: flash_attn_func over the sliced cache (host length, 16-bit) and
    flash_decode_cached over the whole cache with a device kv_len (FP8)."""
    from epfl_megatron_amd.ops.attention import flash_attn_func, flash_decode_cached
    cap = 600
    for dtype, hd, fp8 in ((torch.bfloat16, 128, False), (torch.float16, 64, True)):
        x = E.decode_inputs(dtype, hd, r, fp8, cap, DEV)
        sc = torch.stack([x.k_scale, x.v_scale]).float().contiguous() if fp8 else None
        kk, vc, vn = (_seqs(x, _store(x, t)) for t in (x.k, x.v_census, x.v_needle))
        kv_len = torch.zeros(1, dtype=torch.int32, device=DEV)
        oc, on = [], []
        with torch.no_grad():
            for ci, (n, w) in enumerate(x.cases):
                q1 = x.q_needle[ci].unsqueeze(1)
                if fp8 or not 1 <= n <= cap:  # a host length cannot be 0 or exceed the cache
                    kv_len.fill_(n)
                    oc.append(flash_decode_cached(x.q_census, kk, vc, kv_len, window=w, kv_scale=sc)[:, 0])
                    on.append(flash_decode_cached(q1, kk, vn, kv_len, window=w, kv_scale=sc)[:, 0])
                else:
                    oc.append(flash_attn_func(x.q_census, kk[:, :n], vc[:, :n], causal=True, window=w)[:, 0])
                    on.append(flash_attn_func(q1, kk[:, :n], vn[:, :n], causal=True, window=w)[:, 0])
        _check_decode(x, 0, torch.stack(oc), torch.stack(on), f"auto r={r} {dtype} hd={hd} fp8={fp8}")


# ---------------------------------------------------------------- prefill

def _fwd(q, k, v, causal, window):
    """ext().flash_attn_fwd as ops.attention._FlashFn.forward calls it -> O, lse."""
    from epfl_megatron_amd.ops.attention import _bsnd_strides
    b, sq, nq, d = q.shape
    sk, nkv = k.shape[1], k.shape[2]
    out = torch.empty(b, sq, nq, d, dtype=q.dtype, device=q.device)
    lse = torch.empty(b, nq, sq, dtype=torch.float32, device=q.device)
    _ext().flash_attn_fwd(q, k, v, out, lse, b, sq, sk, nq, nkv, d, list(_bsnd_strides(q, nq // nkv)),
                          list(_bsnd_strides(k, 1)[:3]), list(_bsnd_strides(v, 1)[:3]),
                          [out.stride(0), out.stride(1), out.stride(2)], bool(causal), d ** -0.5,
                          None, None, None, None, window=int(window))
    return out, lse


def _pack(q, k, v):
    """``[b, s, n, hd]`` q / k / v -> the fused projection layout ``[s, b, ng (r + 2) hd]``."""
    b, s, nq, hd = q.shape
    ng = k.shape[2]
    qkv5 = torch.cat([q.view(b, s, ng, nq // ng, hd), k[:, :, :, None], v[:, :, :, None]], dim=3)
    return qkv5.transpose(0, 1).reshape(s, b, -1).contiguous()


def _fwd_packed(qkv, ng, r, hd, docs, window):
    """ext().flash_attn_fwd as _FlashQKVPackedFn.forward calls it -> O ``[b, s, nq, hd]``, lse."""
    from epfl_megatron_amd.ops.attention import _qkv5_views
    s, b = qkv.shape[:2]
    q, k, v, qs, ks = _qkv5_views(qkv.view(s, b, ng, r + 2, hd))
    nq = ng * r
    out = torch.empty(s, b, nq, hd, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(b, nq, s, dtype=torch.float32, device=qkv.device)
    _ext().flash_attn_fwd(q, k, v, out, lse, b, s, s, nq, ng, hd, list(qs), list(ks), list(ks),
                          [out.stride(1), out.stride(0), out.stride(2)], True, hd ** -0.5,
                          None, None, None, docs, window=int(window))
    return out.transpose(0, 1), lse


def _forward_case(dtype, hd, nq, nkv, b, case):
    from epfl_megatron_amd.ops.attention import flash_attn_qkvpacked
    sq, sk, causal, window, docs = case
    vis, bounds = E.prefill_visibility(b, sq, sk, causal, window, docs)
    q, k, v = (t.to(DEV) for t in E.prefill_census_inputs(b, sq, sk, nq, nkv, hd, dtype))
    e64, cnt = E.prefill_expected(v, vis, nq)
    with torch.no_grad():
        if docs is None:
            o, lse = _fwd(q, k, v, causal, window)
        else:
            qkv, bounds = _pack(q, k, v), bounds.to(DEV)
            o, lse = _fwd_packed(qkv, nkv, nq // nkv, hd, bounds, window)
            ow = flash_attn_qkvpacked(qkv, nkv, nq // nkv, hd, causal=True, doc_bounds=bounds, window=window)
            assert torch.equal(ow.view(sq, b, nq, hd).transpose(0, 1), o), case
    what = f"{case} nq={nq} nkv={nkv} hd={hd} {dtype}"
    ok = E.census_ok(o.transpose(0, 1).reshape(sq, -1), e64.transpose(0, 1).reshape(sq, -1))
    rows = (~ok).nonzero().flatten().tolist()[:8]
    assert ok.all(), f"{what}: O off in query rows {rows}, visible-key counts {cnt[:, rows].tolist()}"
    ok, err = E.lse_ok(lse, cnt)
    assert ok, (f"{what}: lse off, max |lse - ln n| {err:.3e} (bound {E.LSE_ATOL:.3e}), counts from lse "
                f"{torch.round(torch.exp(lse.double()))[0, 0, -4:].tolist()} expected {cnt[0, -4:].tolist()}")


@pytest.mark.parametrize("nq,nkv", E.PREFILL_HEADS)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prefill_forward_census(dtype, hd, nq, nkv):
    """O within 1 ulp, round(exp(lse)) the visible-key count exactly and |lse -
    ln n| within the measured bound: causal and not, windows on both sides of
    the 64-key tile edges, sq < sk, document starts at tile edges alone and
    with a window (through the packed-QKV entry)."""
    for case in E.prefill_cases():
        _forward_case(dtype, hd, nq, nkv, E.PREFILL_B, case)


@pytest.mark.parametrize("s,window", [(65, 2), (257, 64), (600, 129)])
def test_prefill_checks_see_one_key(s, window):
    """The checks resolve one key of the kernels' own output: run with a
    window one key too wide, O, lse and dV all fail them."""
    from epfl_megatron_amd.ops.attention import flash_attn_func
    b, nq, nkv, hd, dtype = E.PREFILL_B, 8, 2, 128, torch.bfloat16
    vis, _ = E.prefill_visibility(b, s, s, True, window, None)
    q, k, v = (t.to(DEV).requires_grad_() for t in E.prefill_census_inputs(b, s, s, nq, nkv, hd, dtype))
    e64, cnt = E.prefill_expected(v.detach(), vis, nq)
    dout = E.dv_census_dout(b, s, nq, hd, dtype).to(DEV)
    with torch.no_grad():
        o, lse = _fwd(q, k, v, True, window + 1)
    assert not E.census_ok(o, e64).all() and not E.lse_ok(lse, cnt)[0]
    flash_attn_func(q, k, v, causal=True, window=window + 1).backward(dout)
    assert not E.dv_ok(v.grad, E.dv_expected(dout, vis, nkv))


@pytest.mark.parametrize("switch", ["fa_set_kv2", "fa_set_pairing"])
@pytest.mark.parametrize("nq,nkv", E.PREFILL_HEADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prefill_forward_census_switched_off(dtype, nq, nkv, switch):
    """The same checks with the split-key forward off (head_dim-128 grids of at
    most one block per CU then run the plain 4-wave forward) and with the
    causal pairing off."""
    C = _ext()
    getattr(C, switch)(False)
    try:
        for case in E.prefill_cases():
            _forward_case(dtype, 128, nq, nkv, E.PREFILL_B, case)
    finally:
        getattr(C, switch)(True)


@pytest.mark.parametrize("switch", [None, "fa_set_kv2", "fa_set_pairing"])
@pytest.mark.parametrize("b,s,nq,nkv,hd,what", E.PREFILL_BIG, ids=[c[-1] for c in E.PREFILL_BIG])
def test_prefill_forward_census_large_grids(b, s, nq, nkv, hd, what, switch):
    """The smallest grid that picks the 8-wave forward, the split-key forward
    shape and a grid of exactly two 4-wave blocks per CU (causal pairing),
    each also with the switches off."""
    C = _ext()
    if switch:
        getattr(C, switch)(False)
    try:
        for case in E.prefill_big_cases(s):
            _forward_case(torch.bfloat16, hd, nq, nkv, b, case)
    finally:
        if switch:
            getattr(C, switch)(True)


@pytest.mark.parametrize("nq,nkv", E.PREFILL_HEADS)
@pytest.mark.parametrize("hd", [64, 128])
def test_dv_census(hd, nq, nkv):
    """dV of uniform attention against fp64, relative-only 2^-7 (derived in
    attention_edge_inputs.DV_RTOL) and exactly 0 where the reference is 0:
    window, document bounds and sq < sk."""
    from epfl_megatron_amd.ops.attention import flash_attn_func, flash_attn_qkvpacked
    dtype, b = torch.bfloat16, E.PREFILL_B
    for case in E.dv_cases():
        sq, sk, causal, window, docs = case
        vis, bounds = E.prefill_visibility(b, sq, sk, causal, window, docs)
        q, k, v = (t.to(DEV) for t in E.prefill_census_inputs(b, sq, sk, nq, nkv, hd, dtype))
        dout = E.dv_census_dout(b, sq, nq, hd, dtype).to(DEV)
        ref = E.dv_expected(dout, vis, nkv)
        if docs is None:
            q, k, v = (t.requires_grad_() for t in (q, k, v))
            flash_attn_func(q, k, v, causal=causal, window=window).backward(dout)
            dv = v.grad
        else:
            r = nq // nkv
            qkv = _pack(q, k, v).requires_grad_()
            o = flash_attn_qkvpacked(qkv, nkv, r, hd, causal=True, doc_bounds=bounds.to(DEV), window=window)
            o.backward(dout.transpose(0, 1).reshape(sq, b, -1))
            dv = qkv.grad.view(sq, b, nkv, r + 2, hd)[:, :, :, r + 1].transpose(0, 1)
        d = dv.double()
        rel = ((d - ref).abs() / ref.clamp(min=1e-300))[ref > 0].max().item()
        assert E.dv_ok(dv, ref), (f"{case} nq={nq} nkv={nkv} hd={hd}: max relative error {rel:.3e} (bound "
                                  f"{E.DV_RTOL:.3e}), non-zeros where the reference is 0: "
                                  f"{int((d[ref == 0] != 0).sum())}")
