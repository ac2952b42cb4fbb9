"""Multi-row decode attention (``csrc/flash_decode_mq.hip``) through
``flash_decode_cached`` with 2..16 query rows per sequence, against fp64
attention with the op's mask.  Tolerance: measured, never fixed: at most twice
the error of the forward kernel (``flash_attn_func``, causal, per sequence over
the same keys) against the same reference.  Paged against contiguous, FP8 under
power-of-two scales against the dequantised cache, repeated calls and graph
replays are bitwise.  Measured on an MI355X (multi-row / forward kernel): bf16
8.9e-3 / 6.5e-3, fp16 1.07e-3 / 1.07e-3, FP8 general scales 7.8e-3 / 1.0e-2 and
1.04e-3 / 1.22e-3; model logits 4.2e-2 / 4.9e-2 against the fp32 CPU model."""
import functools
import math

import pytest
import torch

from dist_utils import run_dist
from test_paged_kv_gpu import _paginate

pytestmark = pytest.mark.gpu

DEV, CAP, PAGE = "cuda", 1024, 256
BF16, FP16 = torch.bfloat16, torch.float16
# one shape per MFMA form: (hd, dtype, nq, nkv, sq), 12 and 32 packed rows
FORMS = [pytest.param(128, BF16, 4, 4, 3, id="rows16"), pytest.param(64, FP16, 8, 2, 8, id="rows32")]


def _ops():
    from epfl_megatron_amd.ops import attention, fp8_kv
    return attention, fp8_kv


def _lens(sq):
    return [0, sq - 1, sq, 31, 32, 33, 255, 256, 257, 700]


def _inputs(hd, dtype, nq, nkv, sq, b, cap=CAP, seed=0):
    torch.manual_seed(1000 * hd + 10 * nq + sq + seed)
    q = torch.randn(b, sq, nq, hd, device=DEV).to(dtype)
    k, v = (torch.randn(b, cap, nkv, hd, device=DEV).to(dtype) for _ in range(2))
    return q, k, v


def _call(q, k, v, kv_len, poison=True, **kw):
    """The op, after a NaN-filled block of the output's size went back to the allocator."""
    if poison:
        del_me = torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device)
        del del_me
    out = _ops()[0].flash_decode_cached(q, k, v, kv_len, **kw)
    assert out.shape == q.shape and out.dtype == q.dtype
    return out


def _ref64(q, k, v, lens, window=0):
    """fp64 reference ``[b, sq, nq, hd]``; rows with ``e <= 0`` are zero."""
    b, sq, nq, hd = q.shape
    rep = nq // k.shape[2]
    out = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    for i, n in enumerate(lens):
        if n <= 0:
            continue
        kk = k[i, :n].double().repeat_interleave(rep, 1)  # [n, nq, hd]
        vv = v[i, :n].double().repeat_interleave(rep, 1)
        s = torch.einsum("tnd,jnd->ntj", q[i].double(), kk) / math.sqrt(hd)
        e = n - (sq - 1 - torch.arange(sq, device=q.device))[:, None]
        j = torch.arange(n, device=q.device)[None, :]
        dead = (j >= e) | (j < (e - window if window else 0 * e))
        p = torch.softmax(s.masked_fill(dead[None], float("-inf")), -1)
        p = torch.where(dead.all(-1)[None, :, None], torch.zeros_like(p), p)
        out[i] = torch.einsum("ntj,jnd->tnd", p, vv)
    return out


def _baseline_err(q, k, v, lens, ref, window=0):
    """Largest error of the forward kernel, per sequence that holds all ``sq`` rows."""
    fa = _ops()[0].flash_attn_func
    sq, err = q.shape[1], 0.0
    for i, n in enumerate(lens):
        if n >= sq:
            o = fa(q[i:i + 1], k[i:i + 1, :n], v[i:i + 1, :n], causal=True, window=window)
            err = max(err, float((o.double() - ref[i:i + 1]).abs().max()))
    return err


def _check(out, q, k, v, lens, window=0, kref=None, vref=None, what=""):
    """``out`` within twice the forward kernel's own error; dead rows exact zeros."""
    sq = q.shape[1]
    ref = _ref64(q, k if kref is None else kref, v if vref is None else vref, lens, window)
    base = _baseline_err(q, k, v, lens, ref, window)
    assert not bool(out.isnan().any()), what
    err = float((out.double() - ref).abs().max())
    print(f"{what} window={window}: multi-row {err:.3e}, forward kernel {base:.3e}")
    for i, n in enumerate(lens):
        dead = max(0, min(sq, sq - n))  # tokens t < sq - n have e <= 0
        assert torch.equal(out[i, :dead], torch.zeros_like(out[i, :dead])), (what, i)
        assert n < sq or bool(out[i].any())
    assert err <= 2 * base, (what, window, err, base)
    return err, base


@pytest.mark.parametrize("sq", [2, 3, 5, 8, 16])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
def test_ragged_lengths_against_fp64(dtype, hd, nq, nkv, sq):
    lens = _lens(sq)
    q, k, v = _inputs(hd, dtype, nq, nkv, sq, len(lens))
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _check(_call(q, k, v, kv_len), q, k, v, lens, what=f"hd{hd} {nq}/{nkv} sq{sq}")


@pytest.mark.parametrize("mode", ["one", "none"])
def test_one_length_for_the_batch_and_no_length(mode):
    """``kv_len=None``: every key of a cache of 300 rows (no multiple of a chunk)."""
    n = 700 if mode == "one" else 300
    q, k, v = _inputs(128, BF16, 8, 2, 4, 3, cap=CAP if mode == "one" else n)
    kv_len = torch.tensor([n], dtype=torch.int32, device=DEV) if mode == "one" else None
    _check(_call(q, k, v, kv_len), q, k, v, [n] * 3, what=mode)


@pytest.mark.parametrize("window", [1, 7, 64, 300])
@pytest.mark.parametrize("hd,dtype,nq,nkv,sq", FORMS)
def test_windows(hd, dtype, nq, nkv, sq, window):
    lens = _lens(sq)
    q, k, v = _inputs(hd, dtype, nq, nkv, sq, len(lens))
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _check(_call(q, k, v, kv_len, window=window), q, k, v, lens, window, what="window")


P_LENS = [0, 5, 255, 256, 257, 700]
SCALES2 = ((2.0 ** -3, 2.0 ** 1), (2.0 ** 2, 2.0 ** -1))  # K / V rows, distinct per KV head


def _table(lens, n_pages):
    """A shuffled table ``[b, 4]``; entries no key needs hold stale values outside the pool."""
    g = torch.Generator().manual_seed(4)
    free = torch.randperm(n_pages, generator=g).tolist()
    rows = []
    for n in lens:
        own = (n + PAGE - 1) // PAGE
        rows.append([free.pop() for _ in range(own)] + [10 ** 6, -3, 10 ** 6, -3][:4 - own])
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _scales(rows, nkv):
    return torch.tensor([(r * nkv)[:nkv] for r in rows], dtype=torch.float32, device=DEV)


def _quantize(k, v, sc):
    fp8 = _ops()[1]
    k8, v8 = fp8.quantize(k.float(), sc[0]), fp8.quantize(v.float(), sc[1])
    assert not bool(((k8 & 0x7f) == 0x7f).any() | ((v8 & 0x7f) == 0x7f).any())
    return k8, v8


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("hd,dtype,nq,nkv,sq", FORMS)
def test_paged_is_bitwise_the_gathered_cache(hd, dtype, nq, nkv, sq, fp8):
    lens, n_pages, sc = P_LENS, 9, None
    q, k, v = _inputs(hd, dtype, nq, nkv, sq, len(lens))
    if fp8:
        sc = _scales(SCALES2, nkv)
        k, v = _quantize(k, v, sc)
    table = _table(lens, n_pages)
    (pk, k), (pv, v) = (_paginate(t, table, lens, n_pages) for t in (k, v))  # dead values past n_i
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for window in (0, 64):
        want = _call(q, k, v, kv_len, window=window, kv_scale=sc)
        got = _call(q, pk.transpose(0, 1), pv.transpose(0, 1), kv_len, window=window, kv_scale=sc,
                    page_table=table, capacity=CAP)
        assert not bool(want.isnan().any()) and bool(want.any())
        assert torch.equal(got, want), window


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "general"])
@pytest.mark.parametrize("hd,dtype,nq,nkv,sq", FORMS)
def test_fp8_cache(hd, dtype, nq, nkv, sq, pow2):
    """Power-of-two scales: bitwise the 16-bit form on the dequantised cache.
    General scales: the measured tolerance, reference on the exact bytes."""
    lens = _lens(sq)
    q, k, v = _inputs(hd, dtype, nq, nkv, sq, len(lens))
    sc = _scales(SCALES2 if pow2 else ((0.37, 1.9), (0.011, 3.3)), nkv)
    k8, v8 = _quantize(k, v, sc)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got = _call(q, k8, v8, kv_len, kv_scale=sc)
    fp8 = _ops()[1]
    kd, vd = fp8.dequantize(k8, sc[0], dtype), fp8.dequantize(v8, sc[1], dtype)
    if pow2:
        want = _call(q, kd, vd, kv_len)
        assert bool(want.any()) and torch.equal(got, want)
        return
    exact = [t.view(torch.float8_e4m3fn).double() * s.double()[:, None] for t, s in ((k8, sc[0]), (v8, sc[1]))]
    _check(got, q, kd, vd, lens, kref=exact[0], vref=exact[1], what="fp8 general scales")


@pytest.mark.parametrize("hd,dtype,nq,nkv,sq", FORMS)
def test_rearm_and_graph_replay(hd, dtype, nq, nkv, sq):
    lens = _lens(sq)
    q, k, v = _inputs(hd, dtype, nq, nkv, sq, len(lens))
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    first = _call(q, k, v, kv_len)
    assert torch.equal(_call(q, k, v, kv_len), first)  # the counters were re-armed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _call(q, k, v, kv_len, poison=False)
    for rep in range(3):  # new lengths and cache contents, in place
        kv_len.copy_(torch.tensor(lens[rep + 1:] + lens[:rep + 1], dtype=torch.int32))
        k.copy_(torch.randn_like(k))
        v.copy_(torch.randn_like(v))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, _call(q, k, v, kv_len)), rep
    assert not torch.equal(out, first)


def test_row_count_validation():
    attention = _ops()[0]
    q, k, v = _inputs(64, BF16, 4, 2, 17, 2)
    kv_len = torch.tensor([40, 50], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="flash_attn_func"):
        attention.flash_decode_cached(q, k, v, kv_len)
    one = attention.flash_decode_cached(q[:, :1], k, v, kv_len)  # sq == 1: the path it always took
    want = attention._flash_decode(q[:, :1], k, v, 1.0 / math.sqrt(64), kv_len)
    assert one.shape == (2, 1, 4, 64) and torch.equal(one, want)


PROMPT, NEW = 40, 4


def _model_step(rank, world, gpu):
    """Prompt of 40 tokens, then 4 more as a continued prefill and (GPU) as one
    multi-row device step: the 4 tokens' logits and layer 1's cache rows."""
    from test_fp8_kv_cache_gpu import _model_and_tokens
    from test_gpu_e2e import LLAMA_GQA
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    m, _ = _model_and_tokens(LLAMA_GQA + ["--hidden_size", "256"], 2, gpu)  # hd 64, GQA 4/2
    dev = "cuda" if gpu else "cpu"
    tokens = torch.randint(0, 512, (2, PROMPT + NEW), generator=torch.Generator().manual_seed(8)).to(dev)
    pos = torch.arange(PROMPT + NEW, device=dev)[None].expand(2, -1)
    res = {}
    for name in ("continued", "multi") if gpu else ("continued",):
        ip = InferenceParams(2, 64)
        with torch.no_grad():
            m(tokens[:, :PROMPT], pos[:, :PROMPT], None, inference_params=ip)
            ip.sequence_len_offset = PROMPT
            if name == "multi":
                ip.device_multi = True
                ip.device_offset = torch.tensor([PROMPT], device=dev)
                ip.device_kv_len = torch.tensor([PROMPT + NEW], dtype=torch.int32, device=dev)
            logits = m(tokens[:, PROMPT:], pos[:, PROMPT:], None, inference_params=ip)
        kc, vc = ip.key_value_memory_dict[1]
        res[name] = (logits.float().cpu(), kc[PROMPT:PROMPT + NEW].cpu(), vc[PROMPT:PROMPT + NEW].cpu())
    return res


@functools.lru_cache(maxsize=None)
def _model_runs(gpu):
    return run_dist(_model_step, 1, gpu, env=None if gpu else {"HIP_VISIBLE_DEVICES": ""})[0]


def test_model_multirow_step_against_the_cpu_model():
    ref = _model_runs(False)["continued"][0]
    runs = _model_runs(True)
    (lc, kc, vc), (lm, km, vm) = runs["continued"], runs["multi"]
    base, err = float((lc - ref).abs().max()), float((lm - ref).abs().max())
    print(f"logits against the fp32 CPU model: multi-row step {err:.3e}, continued prefill {base:.3e}")
    assert torch.equal(km, kc) and torch.equal(vm, vc) and bool(km.any())
    assert err <= 2 * base, (err, base)
