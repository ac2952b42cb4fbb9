"""Native FP8 KV-cache prefill on the GPU: the e4m3 K / V forms of the forward
attention kernel (paged and contiguous), the ops that route to them and the
model's continued prefill over an FP8 cache.

The FP8 forms expand the stored bytes exactly and run the 16-bit form's
arithmetic on the unscaled values; the K scale folds into the score scale and
the V scale into the final normalisation.  With power-of-two scales both folds
commute with every rounding, so the same forced form of the 16-bit contiguous
kernel on the gathered, dequantised K / V must give the same bits: no tolerance
appears in tests 1-4 and 6-8.  Test 5 (general scales) takes its bound from the
16-bit kernel's own error, measured at run time.

Measured on an MI355X (test 5, head_dim 128, bf16, s0 = sq = 300, scales K
0.37 / 1.9, V 0.011 / 3.3; largest absolute error against fp64 attention over
the exactly dequantised K / V): FP8 form 1.41e-3, 16-bit kernel 2.51e-3."""
import math

import pytest
import torch

import attention_edge_inputs as E
from dist_utils import run_dist
from test_paged_kv_gpu import _bits, _model, _paginate
from test_paged_prefill_gpu import (N_PAGES, NKV, PAGE, SHAPES, TABLE, WINDOWS, _forms, _fwd,
                                    _two_calls)
from test_prefix_cache import CAP, NEW, share_prompts

pytestmark = pytest.mark.gpu

DEV = "cuda"
# per-head power-of-two scales, distinct per head and between K and V
SCALES = ((2.0 ** -3, 2.0 ** 1), (2.0 ** 2, 2.0 ** -1))


def _fp8():
    from epfl_megatron_amd.ops import fp8_kv
    return fp8_kv


def _scales(rows=SCALES):
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _quantized(b, sk, hd, sc):
    """e4m3 bytes ``[b, sk, NKV, hd]`` of N(0, 1) K and V under ``sc``; no NaN byte."""
    k8, v8 = (_fp8().quantize(torch.randn(b, sk, NKV, hd, device=DEV), sc[i]) for i in range(2))
    assert not bool(((k8 & 0x7f) == 0x7f).any() | ((v8 & 0x7f) == 0x7f).any())
    return k8, v8


def _dequantized(k8, v8, sc, dtype, exact=True):
    """K / V in ``dtype``; ``exact``: asserted equal to the fp64 product."""
    out = []
    for i, t in enumerate((k8, v8)):
        d = _fp8().dequantize(t, sc[i], dtype)
        if exact:
            want = t.view(torch.float8_e4m3fn).double() * sc[i].double()[:, None]
            assert torch.equal(d.double(), want)
        out.append(d)
    return out


def _pools8(k8, v8, table, sk):
    """uint8 pools ``[1, N_PAGES * 256, nkv, hd]``: each row's ``sk`` keys at the
    rows ``table`` names, the e4m3 NaN byte 0x7F everywhere else."""
    pools = tuple(_paginate(t, table, (sk,) * t.shape[0], N_PAGES)[0].transpose(0, 1)
                  for t in (k8, v8))
    assert sk == 3 * PAGE or bool((pools[0] == 0x7f).any())
    return pools


def _same(got, want, what):
    (o, lse), (wo, wlse) = got, want
    assert not bool(o.isnan().any() | wo.isnan().any() | lse.isnan().any()), what
    assert torch.equal(_bits(o), _bits(wo)), what
    assert torch.equal(_bits(lse), _bits(wlse)), what
    assert bool(o.any()), what


# ---------------------------------------------------------------- 1 / 2. the bitwise twins

@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fp8_paged_forward_is_bitwise_the_dequantised_keys(dtype, hd, r):
    """b = 2, tables [5, 2, 7] and [3, 8, 1] in a pool of 9 pages whose other
    bytes are 0x7F; every shape, window and forced form: output and lse of the
    FP8 paged form are bit for bit those of the same form of the 16-bit
    contiguous kernel on the gathered, dequantised K / V."""
    torch.manual_seed(hd + r)
    b, nq = 2, NKV * r
    sc = _scales()
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for s0, sq in SHAPES:
        sk = s0 + sq
        q = torch.randn(b, sq, nq, hd, device=DEV).to(dtype)
        k8, v8 = _quantized(b, sk, hd, sc)
        k, v = _dequantized(k8, v8, sc, dtype)
        pk, pv = _pools8(k8, v8, table, sk)
        for w in WINDOWS:
            for waves, kv2 in _forms(hd):
                want = _fwd(q, k, v, sk, w, waves, kv2)
                got = _fwd(q, pk, pv, sk, w, waves, kv2, table=table, kv_scale=sc)
                _same(got, want, f"s0={s0} sq={sq} w={w} waves={waves} kv2={kv2}")


@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fp8_contiguous_forward_is_bitwise_the_dequantised_keys(dtype, hd, r):
    """The unpaged cache ``[max_seq, max_batch = 3, nkv, hd]`` sliced as the
    model slices it (batch rows 1 .. 2, the first sk keys, transposed), 0x7F
    everywhere else: ``flash_attn_fp8_kv`` and the binding on those byte
    strides against the 16-bit kernel on the dequantised keys."""
    from epfl_megatron_amd.ops.attention import flash_attn_fp8_kv
    torch.manual_seed(hd + r + 1)
    b, nq, max_seq = 2, NKV * r, 3 * PAGE + 5
    sc = _scales()
    for s0, sq in SHAPES:
        sk = s0 + sq
        q = torch.randn(b, sq, nq, hd, device=DEV).to(dtype)
        k8, v8 = _quantized(b, sk, hd, sc)
        k, v = _dequantized(k8, v8, sc, dtype)
        caches = []
        for t in (k8, v8):
            c = torch.full((max_seq, 3, NKV, hd), 0x7f, dtype=torch.uint8, device=DEV)
            c[:sk, 1:3] = t.transpose(0, 1)
            caches.append(c[:, 1:3][:sk].transpose(0, 1))
        ck, cv = caches
        assert not ck.is_contiguous() and ck.shape == k8.shape
        for w in WINDOWS:
            for waves, kv2 in _forms(hd):
                what = f"s0={s0} sq={sq} w={w} waves={waves} kv2={kv2}"
                want = _fwd(q, k, v, sk, w, waves, kv2)
                _same(_fwd(q, ck, cv, sk, w, waves, kv2, kv_scale=sc), want, what)
                o = flash_attn_fp8_kv(q, ck, cv, sc, window=w, waves=waves, kv2=kv2)
                assert torch.equal(_bits(o), _bits(want[0])), what


# ---------------------------------------------------------------- 3. the automatic form

def test_fp8_automatic_form_is_the_16_bit_one():
    """``flash_attn_paged`` on uint8 pools picks the form from (b, sq, nq, hd)
    as ``flash_attn_func`` does on the dequantised gathered keys, and runs the
    native forms (the call counter moves)."""
    from epfl_megatron_amd.ops import attention as A
    torch.manual_seed(3)
    sc = _scales()
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for hd, nq, (s0, sq) in ((128, 8, (256, 130)), (64, 4, (300, 300)), (128, 2, (511, 3))):
        sk = s0 + sq
        q = torch.randn(2, sq, nq, hd, device=DEV).to(torch.bfloat16)
        k8, v8 = _quantized(2, sk, hd, sc)
        k, v = _dequantized(k8, v8, sc, torch.bfloat16)
        pk, pv = _pools8(k8, v8, table, sk)
        for w in (0, 100):
            with torch.no_grad():
                want = A.flash_attn_func(q, k, v, causal=True, window=w)
            before = dict(A.fp8_prefill_calls)
            got = A.flash_attn_paged(q, pk, pv, table, sk, window=w, kv_scale=sc)
            assert A.fp8_prefill_calls["native"] == before["native"] + 1
            assert A.fp8_prefill_calls["fallback"] == before["fallback"]
            assert torch.equal(_bits(got), _bits(want)), (hd, nq, s0, sq, w)


# ---------------------------------------------------------------- 4. the fold is per head

@pytest.mark.parametrize("hd", [64, 128])
def test_k_scale_is_read_per_kv_head(hd):
    """The two heads' K scales swapped in ``kv_scale`` only: the output of
    both heads' queries changes and is the reference built with the swapped
    scales (a kernel that reads ``k_scale[0]`` for every group fails here)."""
    torch.manual_seed(11)
    dtype, r, (s0, sq) = torch.bfloat16, 2, (256, 130)
    sk, nq = s0 + sq, NKV * r
    sc = _scales()
    swapped = _scales((SCALES[0][::-1], SCALES[1]))
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    q = torch.randn(2, sq, nq, hd, device=DEV).to(dtype)
    k8, v8 = _quantized(2, sk, hd, sc)
    pk, pv = _pools8(k8, v8, table, sk)
    k, v = _dequantized(k8, v8, swapped, dtype)
    for waves, kv2 in _forms(hd):
        base, _ = _fwd(q, pk, pv, sk, 0, waves, kv2, table=table, kv_scale=sc)
        got = _fwd(q, pk, pv, sk, 0, waves, kv2, table=table, kv_scale=swapped)
        _same(got, _fwd(q, k, v, sk, 0, waves, kv2), (waves, kv2))
        for g in range(NKV):
            heads = slice(g * r, (g + 1) * r)
            assert not torch.equal(_bits(got[0][:, :, heads]), _bits(base[:, :, heads])), (waves, kv2, g)


# ---------------------------------------------------------------- 5. general scales

def _attention64(q, k, v, scale):
    """fp64 causal (bottom-right aligned) attention, ``[b, s, n, d]``."""
    b, sq, nq, d = q.shape
    sk, r = k.shape[1], nq // k.shape[2]
    qf = q.double().permute(0, 2, 1, 3)
    kf, vf = (t.permute(0, 2, 1, 3).repeat_interleave(r, dim=1) for t in (k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    i = torch.arange(sq, device=q.device)[:, None]
    j = torch.arange(sk, device=q.device)[None, :]
    s = s.masked_fill(j > i + (sk - sq), -math.inf)
    return torch.matmul(torch.softmax(s, dim=-1), vf).permute(0, 2, 1, 3)


def test_general_scales_within_twice_the_16_bit_kernels_error():
    """Scales that are no powers of two (K 0.37 / 1.9, V 0.011 / 3.3),
    head_dim 128, bf16, s0 = sq = 300, through the table.  Reference: fp64
    attention over the exactly dequantised (fp64) K / V.  Bound: twice the
    largest error of the 16-bit contiguous kernel against that reference on the
    same inputs with the dequantised values rounded to bf16, measured here (one
    extra rounding that the V-scale placement can add, and the 16-bit kernel
    seeing rounded inputs).

    Measured on an MI355X: 16-bit kernel 2.509e-3, FP8 form 1.408e-3."""
    torch.manual_seed(5)
    dtype, hd, r, (s0, sq) = torch.bfloat16, 128, 4, (300, 300)
    sk, nq = s0 + sq, NKV * r
    sc = _scales(((0.37, 1.9), (0.011, 3.3)))
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    q = torch.randn(2, sq, nq, hd, device=DEV).to(dtype)
    k8, v8 = _quantized(2, sk, hd, sc)
    k64, v64 = (t.view(torch.float8_e4m3fn).double() * sc[i].double()[:, None]
                for i, t in enumerate((k8, v8)))
    ref = _attention64(q, k64, v64, hd ** -0.5)
    k16, v16 = _dequantized(k8, v8, sc, dtype, exact=False)
    base, _ = _fwd(q, k16, v16, sk)
    pk, pv = _pools8(k8, v8, table, sk)
    got, _ = _fwd(q, pk, pv, sk, table=table, kv_scale=sc)
    err16 = float((base.double() - ref).abs().max())
    err8 = float((got.double() - ref).abs().max())
    print(f"general scales: 16-bit kernel max abs error {err16:.6e}, FP8 form {err8:.6e}")
    assert not bool(got.isnan().any()) and err16 > 0
    assert err8 <= 2 * err16, (err8, err16)


# ---------------------------------------------------------------- 6. census

@pytest.mark.parametrize("hd", [64, 128])
def test_fp8_census_through_a_table_counts_the_visible_keys(hd):
    """Q = 0, the census V (e4m3-representable, asserted) stored with scale 1:
    output and lse count exactly the visible keys of every row, for every
    shape, window and form, fetched as bytes through the table."""
    dtype, nq = torch.float16, 4
    one = _scales(((1.0, 1.0), (1.0, 1.0)))
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    for s0, sq in SHAPES:
        sk = s0 + sq
        q, k, v = (t.to(DEV) for t in E.prefill_census_inputs(2, sq, sk, nq, NKV, hd, dtype))
        assert torch.equal(v.float().to(torch.float8_e4m3fn).float(), v.float())
        k8, v8 = _fp8().quantize(k, one[0]), _fp8().quantize(v, one[1])
        assert torch.equal(_fp8().dequantize(v8, one[1], dtype), v)
        pk, pv = _pools8(k8, v8, table, sk)
        for w in WINDOWS:
            vis, _ = E.prefill_visibility(2, sq, sk, True, w if w < sk else 0, None)
            e, count = E.prefill_expected(v, vis, nq)
            for waves, kv2 in _forms(hd):
                o, lse = _fwd(q, pk, pv, sk, w, waves, kv2, table=table, kv_scale=one)
                what = (s0, sq, w, waves, kv2)
                assert bool(E.census_ok(o, e).all()), what
                ok, err = E.lse_ok(lse, count)
                assert ok, (what, err)


# ---------------------------------------------------------------- 7. binding checks

def test_fp8_binding_checks_name_the_argument():
    dt, hd, nq, sq, sk = torch.bfloat16, 64, 4, 130, 386
    q = torch.zeros(2, sq, nq, hd, device=DEV, dtype=dt)
    k8 = torch.zeros(2, sk, NKV, hd, device=DEV, dtype=torch.uint8)
    k16 = torch.zeros(2, sk, NKV, hd, device=DEV, dtype=dt)
    pool = torch.zeros(N_PAGES * PAGE, 1, NKV, hd, device=DEV, dtype=torch.uint8).transpose(0, 1)
    table = torch.tensor(TABLE, dtype=torch.int32, device=DEV)
    sc = _scales()
    _fwd(q, k8, k8, sk, kv_scale=sc)
    _fwd(q, pool, pool, sk, table=table, kv_scale=sc)
    with pytest.raises(RuntimeError, match="need their kv_scale"):
        _fwd(q, k8, k8, sk)
    with pytest.raises(RuntimeError, match="need their kv_scale"):
        _fwd(q, pool, pool, sk, table=table)
    with pytest.raises(RuntimeError, match="kv_scale given for 16-bit k / v"):
        _fwd(q, k16, k16, sk, kv_scale=sc)
    with pytest.raises(RuntimeError, match="FP8 k needs FP8 .* v"):
        _fwd(q, k8, k16, sk, kv_scale=sc)
    with pytest.raises(RuntimeError, match="kv_scale need causal"):
        _fwd(q, k8, k8, sk, kv_scale=sc, causal=False)
    cos = torch.ones(1024, hd // 2, device=DEV)
    with pytest.raises(RuntimeError, match="rope_cos cannot be combined with FP8"):
        _fwd(q, k8, k8, sk, kv_scale=sc, rope_cos=cos, rope_sin=cos)
    docs = torch.zeros(2, 2, sq, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="docs cannot be combined with FP8"):
        _fwd(q, k8, k8, sk, kv_scale=sc, docs=docs)
    for bad in (sc[:, :1].contiguous(), sc.t().contiguous()[:1], sc.double(), sc.cpu(), sc.reshape(-1)):
        with pytest.raises(RuntimeError, match="kv_scale must be a contiguous device fp32"):
            _fwd(q, k8, k8, sk, kv_scale=bad)
    # byte strides: rows of a uint8 view must stay 16-byte aligned
    odd = torch.zeros(2, sk, NKV, hd + 8, device=DEV, dtype=torch.uint8)[..., :hd]
    with pytest.raises(RuntimeError, match="k strides must keep 16-byte alignment"):
        _fwd(q, odd, odd, sk, kv_scale=sc)


# ---------------------------------------------------------------- 8. the model and the batcher

def _model_run(rank, world, extra):
    from epfl_megatron_amd.inference import ContinuousBatcher
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.ops import attention as A
    m = _model(extra)
    out = {}
    prompt = torch.randint(0, 512, (300,), generator=torch.Generator().manual_seed(3)).to(DEV)

    def prefill(paged, native):
        A.FP8_PREFILL_NATIVE = native
        before = dict(A.fp8_prefill_calls)
        if paged:
            ip = InferenceParams(2, CAP, kv_pages=4, table_device=DEV)
            ip.page_table[0, :2] = torch.tensor([2, 1], dtype=torch.int32)
        else:
            ip = InferenceParams(1, CAP)
        logits = _two_calls(m, ip, prompt, 130, paged)
        calls = {k: A.fp8_prefill_calls[k] - before[k] for k in before}
        mem = [(k.clone(), v.clone()) for k, v in ip.key_value_memory_dict.values()]
        return logits, calls, mem

    for paged in (False, True):
        on, calls_on, mem_on = prefill(paged, True)
        off, calls_off, mem_off = prefill(paged, False)
        out[paged] = dict(
            same=torch.equal(_bits(on), _bits(off)), finite=bool(on.float().isfinite().all()),
            calls_on=calls_on, calls_off=calls_off, layers=len(mem_on),
            dtype=mem_on[0][0].dtype,
            mem=all(torch.equal(a, b) for pa, pb in zip(mem_on, mem_off) for a, b in zip(pa, pb)))

    prompts = share_prompts(512)

    def serve(native):
        A.FP8_PREFILL_NATIVE = native
        before = dict(A.fp8_prefill_calls)
        ip = InferenceParams(4, CAP, kv_pages=16)
        cb = ContinuousBatcher(m, ip, 4, CAP, poll_every=1, max_new_tokens=32, prefill_chunk=256,
                               prefix_cache=True)
        for p, mn in zip(prompts, NEW):
            cb.submit(p, mn)
        toks = cb.run()
        return toks, {k: A.fp8_prefill_calls[k] - before[k] for k in before}, cb.prefix_hit_pages
    out["on"], out["off"] = serve(True), serve(False)
    A.FP8_PREFILL_NATIVE = True
    return out


def test_model_prefill_is_bitwise_the_fallback_and_runs_the_native_forms():
    """The tiny GQA Llama, bf16, FP8 KV cache with the default scales (1.0),
    unpaged and paged: 300 tokens prefilled as 130 + 170.  The second call's
    logits and the cache bytes afterwards are bitwise the same with the native
    FP8 forms and with the dequantising fallback (module switch, in process),
    the native forms ran once per layer when on and never when off; the
    prefix-sharing batcher over an FP8 pool gives identical tokens either way."""
    r = run_dist(_model_run, 1, ["--inference_fp8_kv_cache"], env={"EMA_DECODE_FUSED": "1"})[0]
    for paged in (False, True):
        c = r[paged]
        assert c["dtype"] == torch.uint8 and c["layers"] >= 1
        assert c["same"] and c["finite"] and c["mem"], (paged, c)
        assert c["calls_on"] == {"native": c["layers"], "fallback": 0}, (paged, c)
        assert c["calls_off"] == {"native": 0, "fallback": c["layers"]}, (paged, c)
    (toks_on, calls_on, hits_on), (toks_off, calls_off, hits_off) = r["on"], r["off"]
    assert [len(t) for t in toks_on] == list(NEW)
    assert toks_on == toks_off
    assert hits_on == hits_off and hits_on > 0
    assert calls_on["native"] > 0 and calls_on["fallback"] == 0
    assert calls_off["native"] == 0 and calls_off["fallback"] == calls_on["native"]
