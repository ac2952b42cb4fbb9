"""FP8 KV-cache prefill, the parts that need no GPU: on CPU tensors
``flash_attn_paged`` and ``flash_attn_fp8_kv`` take the dequantising fallback
and agree with an fp32 reference, the Python layer validates its arguments, and
``fp8_kv.dequantize`` is exact for the power-of-two scales that the GPU tests'
bitwise comparisons rest on."""
import pytest
import torch

from epfl_megatron_amd.inference.paged import KV_PAGE
from epfl_megatron_amd.ops import attention as A
from epfl_megatron_amd.ops import fp8_kv

NKV = 2
# the scales of tests/test_fp8_prefill_gpu.py
SCALES = ((2.0 ** -3, 2.0 ** 1), (2.0 ** 2, 2.0 ** -1))
TABLE = ((5, 2, 7), (3, 8, 1))
N_PAGES = 9


def _case(b, sq, sk, nq, hd, seed=0):
    g = torch.Generator().manual_seed(seed)
    sc = torch.tensor(SCALES)
    q = torch.randn(b, sq, nq, hd, generator=g)
    k8, v8 = (fp8_kv.quantize(torch.randn(b, sk, NKV, hd, generator=g), sc[i]) for i in range(2))
    return q, k8, v8, sc


def _pools(k8, v8, table, sk):
    pools = []
    j = torch.arange(sk)
    for t in (k8, v8):
        pool = torch.full((N_PAGES * KV_PAGE, 1) + tuple(t.shape[2:]), 0x7f, dtype=torch.uint8)
        for i in range(t.shape[0]):
            pool[table[i][j // KV_PAGE].long() * KV_PAGE + j % KV_PAGE, 0] = t[i]
        pools.append(pool.transpose(0, 1))
    return pools


@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("s0,sq", [(256, 2), (300, 300), (0, 513)])
def test_cpu_tensors_take_the_fallback_and_match_the_reference(s0, sq, window):
    sk, hd, nq = s0 + sq, 32, 4
    q, k8, v8, sc = _case(2, sq, sk, nq, hd, seed=sk)
    k, v = fp8_kv.dequantize(k8, sc[0]), fp8_kv.dequantize(v8, sc[1])
    want = A.attention_ref(q, k, v, True, window=window)
    before = dict(A.fp8_prefill_calls)
    got = A.flash_attn_fp8_kv(q, k8, v8, sc, window=window)
    table = torch.tensor(TABLE, dtype=torch.int32)
    pk, pv = _pools(k8, v8, table, sk)
    got_paged = A.flash_attn_paged(q, pk, pv, table, sk, window=window, kv_scale=sc)
    assert A.fp8_prefill_calls["native"] == before["native"]
    assert A.fp8_prefill_calls["fallback"] == before["fallback"] + 2
    for o in (got, got_paged):
        assert o.dtype == q.dtype and o.shape == q.shape and not bool(o.isnan().any())
        # fp32 math on both sides, sums in another order
        assert torch.allclose(o, want, atol=1e-5, rtol=1e-5)
    # the model's view of the unpaged cache: [max_seq, max_batch, nkv, hd], rows 1 .. 2
    cache = [torch.full((sk + 3, 3, NKV, hd), 0x7f, dtype=torch.uint8) for _ in range(2)]
    for c, t in zip(cache, (k8, v8)):
        c[:sk, 1:3] = t.transpose(0, 1)
    ck, cv = (c[:, 1:3][:sk].transpose(0, 1) for c in cache)
    assert torch.equal(A.flash_attn_fp8_kv(q, ck, cv, sc, window=window), got)


def test_python_layer_validates_its_arguments():
    q, k8, v8, sc = _case(2, 4, 260, 4, 32)
    table = torch.tensor(TABLE, dtype=torch.int32)
    pk, pv = _pools(k8, v8, table, 260)
    # sq <= sk
    with pytest.raises(ValueError, match="last sq of sk"):
        A.flash_attn_fp8_kv(torch.zeros(2, 261, 4, 32), k8, v8, sc)
    with pytest.raises(ValueError, match="last sq of sk"):
        A.flash_attn_paged(q, pk, pv, table, 3, kv_scale=sc)
    # table coverage
    with pytest.raises(ValueError, match="sk exceeds the page_table"):
        A.flash_attn_paged(q, pk, pv, table, 3 * KV_PAGE + 1, kv_scale=sc)
    # the uint8 / kv_scale pairing
    with pytest.raises(ValueError, match="needs its kv_scale"):
        A.flash_attn_paged(q, pk, pv, table, 260)
    with pytest.raises(ValueError, match="kv_scale given for a 16-bit pool"):
        A.flash_attn_paged(q, pk.float(), pv.float(), table, 260, kv_scale=sc)
    with pytest.raises(ValueError, match="needs its kv_scale"):
        A.flash_attn_fp8_kv(q, k8, v8, None)
    with pytest.raises(ValueError, match="must be uint8"):
        A.flash_attn_fp8_kv(q, k8.float(), v8.float(), sc)
    with pytest.raises(ValueError, match="sliding window"):
        A.flash_attn_fp8_kv(q, k8, v8, sc, window=-1)


def test_the_switch_forces_the_fallback(monkeypatch):
    """``FP8_PREFILL_NATIVE = False`` (EMA_FA_FP8_PREFILL=0) is read at every
    call; on CPU tensors both settings take the fallback."""
    q, k8, v8, sc = _case(1, 3, 20, 2, 16)
    assert isinstance(A.FP8_PREFILL_NATIVE, bool)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(A, "FP8_PREFILL_NATIVE", on)
        before = A.fp8_prefill_calls["fallback"]
        outs.append(A.flash_attn_fp8_kv(q, k8, v8, sc))
        assert A.fp8_prefill_calls["fallback"] == before + 1
    assert torch.equal(*outs)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_dequantize_is_exact_for_the_power_of_two_scales(dtype):
    """Every e4m3 byte (NaN excepted) under every scale the GPU tests use: the
    dequantised value in bf16 / fp16 is the fp64 product, and quantising it
    gives the byte back."""
    byte = torch.arange(256, dtype=torch.uint8)
    byte = byte[(byte & 0x7f) != 0x7f]
    for s in sorted({s for row in SCALES for s in row} | {1.0}):
        sc = torch.tensor([s])
        x = byte.view(-1, 1, 1)
        d = fp8_kv.dequantize(x, sc, dtype)
        want = x.view(torch.float8_e4m3fn).double() * s
        assert torch.equal(d.double(), want), s
        back = fp8_kv.quantize(d, sc)
        # (-0 and +0 keep their own bytes)
        assert torch.equal(back, x), s
