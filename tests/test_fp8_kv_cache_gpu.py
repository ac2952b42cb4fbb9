"""FP8 KV cache on the GPU (``--inference_fp8_kv_cache``): the quantising cache
store and the QKV epilogue's e4m3 write against the torch quantiser bit for
bit, the FP8 forms of the decode attention kernel against an fp32 reference
over the exactly dequantised cache, the binding checks, and the model: cache
bytes, fused against unfused, graph against eager, FP8-KV against 16-bit."""
import functools

import pytest
import torch

from dist_utils import run_dist, init_framework

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (~(err <= tol)).sum().item()  # NaN / inf count as off
    assert bad == 0, f"{msg}: {bad} elems off, max err {err.max().item():.3e}"


def _scales(nkv, lo):
    """Power-of-two scales that differ per head: 2^lo .. 2^(lo + 4), K and V apart."""
    e = torch.arange(nkv, device=DEV)
    return torch.stack((torch.ldexp(torch.ones(nkv, device=DEV), lo + e % 5),
                        torch.ldexp(torch.ones(nkv, device=DEV), lo + 1 + (e + 2) % 4)))


# ---------------------------------------------------------------- store kernel and EPI_QKV write

SENT = 0xA5


@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("ng,r,hd,K", [(2, 2, 128, 512), (8, 8, 128, 4096), (4, 1, 64, 512)])
def test_qkv_epilogue_and_store_write_the_quantised_rows(ng, r, hd, K, M):
    """The rows the FP8 forms write equal, bitwise, the reference quantiser
    applied to the rows the 16-bit form writes from the same inputs; q is the
    16-bit form's q; every other byte of a sentinel-filled cache is unchanged.
    K = 4096 takes the persistent kernels, M > 16 the two-row-block forms.
    Variants: row-major / packed / FP8 weights, bf16 / fp16, host / device slot.
    Head scales 2^-9 .. 2^-4: the small ones saturate (the clamp)."""
    from epfl_megatron_amd.ops import decode_pack, fp8_kv, fp8_weights as f8
    from epfl_megatron_amd.ops.rope import rope_table
    C = _ext()
    L, B, b0, slot = 9, M + 2, 1, 5
    N = ng * (r + 2) * hd
    cos, sin = rope_table(hd, 64, DEV)
    pos = (torch.arange(M, device=DEV).view(M, 1) * 3 + 2) % 64
    sc = _scales(ng, -9)
    keep = torch.ones(L, B, dtype=torch.bool, device=DEV)
    keep[slot, b0:b0 + M] = False
    variants = [("rowmajor", torch.bfloat16, False), ("packed", torch.float16, True),
                ("packed", torch.bfloat16, False), ("fp8w", torch.bfloat16, True)]
    for i, (form, dt, dev_slot) in enumerate(variants):
        torch.manual_seed(100 * M + ng + i)
        x = torch.randn(M, K, device=DEV, dtype=dt)
        g = (torch.rand(K, device=DEV) + 0.5).to(dt) if M <= 16 else None
        w = (torch.randn(N, K, device=DEV) * 0.05).to(dt)
        wsc = None
        if form == "packed":
            w = decode_pack.pack(w)
        elif form == "fp8w":
            q8, wsc = f8.quantize_rows(w)
            w = f8.pack_fp8(q8)
        st = torch.tensor([slot], device=DEV) if dev_slot else None
        args = (x, w, g, 1e-5, ng, r, hd, cos, sin, pos)
        tail = (st, 0 if dev_slot else slot, form != "rowmajor", wsc)
        k16 = torch.zeros(L, B, ng, hd, device=DEV, dtype=dt)
        v16 = torch.zeros_like(k16)
        k8 = torch.full((L, B, ng, hd), SENT, device=DEV, dtype=torch.uint8)
        v8 = torch.full_like(k8, SENT)
        with torch.no_grad():
            q16 = C.skinny_qkv_rope_cache(*args, k16[:, b0:b0 + M], v16[:, b0:b0 + M], *tail)
            qf8 = C.skinny_qkv_rope_cache(*args, k8[:, b0:b0 + M], v8[:, b0:b0 + M], *tail, sc)
        what = f"{form} {dt} dev_slot={dev_slot}"
        assert torch.equal(qf8, q16), what
        rows_k, rows_v = k16[slot, b0:b0 + M], v16[slot, b0:b0 + M]
        assert rows_k.abs().max() > 0 and rows_v.abs().max() > 0
        want_k, want_v = fp8_kv.quantize(rows_k, sc[0]), fp8_kv.quantize(rows_v, sc[1])
        assert torch.equal(k8[slot, b0:b0 + M], want_k), what + " k"
        assert torch.equal(v8[slot, b0:b0 + M], want_v), what + " v"
        assert bool((k8[keep] == SENT).all()) and bool((v8[keep] == SENT).all()), what
        assert ((want_k & 0x7f) == 0x7e).any()  # some values saturated
        # the store kernel on the 16-bit rows (strided views of the 16-bit cache)
        k8s, v8s = torch.full_like(k8, SENT), torch.full_like(v8, SENT)
        fp8_kv.store(k16[slot:slot + 1, b0:b0 + M], v16[slot:slot + 1, b0:b0 + M],
                     k8s[:, b0:b0 + M], v8s[:, b0:b0 + M], sc, slot=slot, slot_t=st)
        assert torch.equal(k8s, k8) and torch.equal(v8s, v8), what + " store"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sq,b,nkv,r,hd", [(1, 3, 2, 2, 128), (21, 3, 2, 2, 128), (67, 5, 4, 1, 64),
                                           (300, 2, 8, 8, 128)])
def test_store_kernel_prefill_rows(sq, b, nkv, r, hd, dt):
    """k / v as the strided slices of a fused QKV projection [sq, b, ng, r + 2,
    hd] (edge values planted) into rows slot .. slot + sq - 1: more than one
    workgroup, a count that is no multiple of 256 threads, host and device slot."""
    from epfl_megatron_amd.ops import fp8_kv
    torch.manual_seed(sq + b)
    mixed = (torch.randn(sq, b, nkv, r + 2, hd, device=DEV) * 30).to(dt)
    edge = torch.tensor([0.0, -0.0, 1e4, -1e4, 448.0, 1.0625, 1.1875, 2.0 ** -9, 2.0 ** -10,
                         3 * 2.0 ** -10, -2.0 ** -11, 464.0], device=DEV).to(dt)
    mixed[0, 0, 0, r, :12] = edge
    mixed[sq - 1, b - 1, nkv - 1, r + 1, hd - 12:] = edge
    k, v = mixed[:, :, :, r], mixed[:, :, :, r + 1]
    sc = _scales(nkv, -3)
    L, B, b0, slot = sq + 7, b + 2, 1, 4
    keep = torch.ones(L, B, dtype=torch.bool, device=DEV)
    keep[slot:slot + sq, b0:b0 + b] = False
    for st in (None, torch.tensor([slot], device=DEV)):
        k8 = torch.full((L, B, nkv, hd), SENT, device=DEV, dtype=torch.uint8)
        v8 = torch.full_like(k8, SENT)
        assert fp8_kv.store_native_ok(k)
        fp8_kv.store(k, v, k8[:, b0:b0 + b], v8[:, b0:b0 + b], sc, slot=0 if st is not None else slot,
                     slot_t=st)
        assert torch.equal(k8[slot:slot + sq, b0:b0 + b], fp8_kv.quantize(k, sc[0]))
        assert torch.equal(v8[slot:slot + sq, b0:b0 + b], fp8_kv.quantize(v, sc[1]))
        assert bool((k8[keep] == SENT).all()) and bool((v8[keep] == SENT).all())


def test_calibration_on_the_device():
    """calibrate_ on GPU tensors: the CPU rule's scales (powers of two, amax /
    scale in (112, 224], 1.0 for an all-zero head), written in place into the
    tensor the kernels read, and the store that follows does not saturate."""
    from epfl_megatron_amd.ops import fp8_kv
    torch.manual_seed(3)
    sq, b, nkv, hd = 21, 3, 4, 128
    mag = torch.tensor([1e-3, 1.0, 0.0, 300.0], device=DEV)
    k = (torch.randn(sq, b, nkv, hd, device=DEV) * mag[None, None, :, None]).to(torch.bfloat16)
    v = (torch.randn(sq, b, nkv, hd, device=DEV) * mag.flip(0)[None, None, :, None]).to(torch.bfloat16)
    sc = fp8_kv.new_scales(nkv, DEV)
    ptr = sc.data_ptr()
    fp8_kv.calibrate_(sc, k, v)
    ref = fp8_kv.new_scales(nkv, "cpu")
    fp8_kv.calibrate_(ref, k.cpu(), v.cpu())
    assert sc.data_ptr() == ptr and torch.equal(sc.cpu(), ref)
    assert sc[0, 2] == 1 and sc[1, 1] == 1
    for row, t in ((0, k), (1, v)):
        amax = t.float().abs().amax(dim=(0, 1, 3))
        ratio = (amax / sc[row])[amax > 0]
        assert bool((ratio <= 224).all()) and bool((ratio > 112).all()), ratio
    k8 = torch.zeros(sq, b, nkv, hd, device=DEV, dtype=torch.uint8)
    v8 = torch.zeros_like(k8)
    fp8_kv.store(k, v, k8, v8, sc)
    assert not ((k8 & 0x7f) >= 0x78).any() and not ((v8 & 0x7f) >= 0x78).any()  # all below 256


# ---------------------------------------------------------------- decode kernel

def _fp8_cache(shape, seed):
    """Random e4m3 bytes without the NaN codes (0x7f, 0xff)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    c = torch.randint(0, 254, shape, device=DEV, generator=gen)
    return (c + (c >= 127).long()).to(torch.uint8)  # skips 0x7f; 254 -> never reaches 0xff


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
    return out


@pytest.mark.parametrize("b,sk,nq,nkv,hd", [(2, 1, 8, 8, 128), (2, 77, 8, 2, 128),
                                            (1, 300, 71, 1, 64), (3, 1000, 64, 8, 128),
                                            (1, 4096, 32, 32, 128), (2, 513, 12, 4, 64)])
def test_flash_decode_fp8(b, sk, nq, nkv, hd):
    """The FP8 forms against attention_ref in fp32 over the exactly dequantised
    cache (so quantisation error is no part of the tolerance: 2e-2 / 2e-2 as
    for the 16-bit kernel): host length and device kv_len, keys per wave auto
    and forced to 8 / 16 / 64, windows; two launches are bitwise equal."""
    from epfl_megatron_amd.ops import fp8_kv
    from epfl_megatron_amd.ops.attention import attention_ref, flash_decode_cached
    torch.manual_seed(sk + nq)
    kmem = _fp8_cache((sk + 70, b + 1, nkv, hd), sk)
    vmem = _fp8_cache((sk + 70, b + 1, nkv, hd), sk + 1)
    assert not ((kmem & 0x7f) == 0x7f).any() and (kmem == 0xfe).any() and (kmem == 0x7e).any()
    # log-uniform bytes: rms about 100 x scale -> keys and values of order one
    sc = _scales(nkv, -8)
    kv_len = torch.tensor([sk], device=DEV, dtype=torch.int32)
    whole_k, whole_v = kmem[:, 1:b + 1].transpose(0, 1), vmem[:, 1:b + 1].transpose(0, 1)
    keys, vals = whole_k[:, :sk], whole_v[:, :sk]
    kf, vf = fp8_kv.dequantize(keys, sc[0]), fp8_kv.dequantize(vals, sc[1])
    for dt in (torch.bfloat16, torch.float16):
        q = (torch.randn(1, b, nq, hd, device=DEV, dtype=dt) * 2).transpose(0, 1)
        for W in (0, 1, 100, 5000):
            ref = attention_ref(q.float(), kf, vf, causal=True, window=W)
            assert torch.isfinite(ref).all() and ref.abs().max() > 0.1
            for kpw in (0, 8, 16, 64):
                what = f"{dt} W={W} kpw={kpw}"
                with torch.no_grad():
                    o = _decode(q, keys, vals, sc, None, W, kpw)
                    oc = _decode(q, whole_k, whole_v, sc, kv_len, W, kpw)
                    o2 = _decode(q, keys, vals, sc, None, W, kpw)
                    oc2 = _decode(q, whole_k, whole_v, sc, kv_len, W, kpw)
                _close(o, ref, 2e-2, 2e-2, what + " host length")
                _close(oc, ref, 2e-2, 2e-2, what + " device length")
                assert torch.equal(o, o2) and torch.equal(oc, oc2), what
        with torch.no_grad():  # the public wrappers
            ow = flash_decode_cached(q, whole_k, whole_v, kv_len, window=100, kv_scale=sc)
        assert torch.equal(ow, _decode(q, whole_k, whole_v, sc, kv_len, 100))


def test_flash_decode_fp8_reads_the_scales_on_the_device():
    """The scales are read from device memory at every launch: doubling the V
    scales in place doubles the output, K scales move the softmax."""
    b, sk, nq, nkv, hd = 2, 300, 8, 2, 128
    kmem, vmem = _fp8_cache((b, sk, nkv, hd), 1), _fp8_cache((b, sk, nkv, hd), 2)
    torch.manual_seed(0)
    q = torch.randn(b, 1, nq, hd, device=DEV, dtype=torch.bfloat16)
    sc = _scales(nkv, -8)
    o1 = _decode(q, kmem, vmem, sc)
    sc[1] *= 2
    o2 = _decode(q, kmem, vmem, sc)
    assert torch.equal(o2.float(), 2 * o1.float())
    sc[0] *= 4
    assert not torch.equal(_decode(q, kmem, vmem, sc), o2)


def test_fp8_kv_binding_checks():
    """A missing, non-fp32 or wrong-size scale tensor and mixed K / V dtypes raise."""
    from epfl_megatron_amd.ops.rope import rope_table
    C = _ext()
    b, sk, nq, nkv, hd = 2, 64, 8, 2, 128
    k8, v8 = _fp8_cache((b, sk, nkv, hd), 1), _fp8_cache((b, sk, nkv, hd), 2)
    k16 = torch.randn(b, sk, nkv, hd, device=DEV, dtype=torch.bfloat16)
    q = torch.randn(b, 1, nq, hd, device=DEV, dtype=torch.bfloat16)
    sc = _scales(nkv, -8)
    _decode(q, k8, v8, sc)
    for bad in (lambda: _decode(q, k8, v8, None),             # FP8 cache without scales
                lambda: _decode(q, k8, v8, sc.double()),      # not fp32
                lambda: _decode(q, k8, v8, sc[:, :1].contiguous()),  # wrong size
                lambda: _decode(q, k8, v8, sc[0]),            # K scales only
                lambda: _decode(q, k8, v8, sc.cpu()),         # host tensor
                lambda: _decode(q, k8, k16, sc),              # mixed K / V dtypes
                lambda: _decode(q, k16, v8, sc),
                lambda: _decode(q, k16, k16, sc)):            # scales with a 16-bit cache
        with pytest.raises(RuntimeError):
            bad()
    # the QKV projection and the store
    ng, r, M, K = nkv, nq // nkv, 3, 512
    cos, sin = rope_table(hd, 64, DEV)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(ng * (r + 2) * hd, K, device=DEV, dtype=torch.bfloat16) * 0.05
    pos = torch.arange(M, device=DEV).view(M, 1)
    c8 = [torch.zeros(8, M, ng, hd, device=DEV, dtype=torch.uint8) for _ in range(2)]
    c16 = [torch.zeros(8, M, ng, hd, device=DEV, dtype=torch.bfloat16) for _ in range(2)]

    def qkv(kc, vc, *scale):
        return C.skinny_qkv_rope_cache(x, w, None, 0.0, ng, r, hd, cos, sin, pos, kc, vc, None, 2,
                                       False, None, *scale)
    qkv(c8[0], c8[1], sc)
    for bad in (lambda: qkv(c8[0], c8[1]), lambda: qkv(c8[0], c8[1], sc.double()),
                lambda: qkv(c8[0], c8[1], sc[:, :1].contiguous()), lambda: qkv(c8[0], c16[1], sc),
                lambda: qkv(c16[0], c16[1], sc),
                lambda: C.kv_store_fp8(c16[0][:1], c16[1][:1], c8[0], c8[1], sc[:, :1].contiguous()),
                lambda: C.kv_store_fp8(c16[0][:1], c16[1][:1], c8[0], c16[1], sc),
                lambda: C.kv_store_fp8(c16[0], c16[1], c8[0], c8[1], sc, None, 1),  # rows past the end
                lambda: C.kv_store_fp8(c16[0][:1].float(), c16[1][:1].float(), c8[0], c8[1], sc)):
        with pytest.raises(RuntimeError):
            bad()


# ---------------------------------------------------------------- model level

PLEN, NSTEP = 21, 8

# max |logits(FP8 KV) - logits(16-bit KV)| of the same tiny model on the CPU
# fp32 path (attention_ref + the torch quantiser, scales 1.0), same weights and
# tokens, teacher-forced, prefill 21 + 8 steps: measured by _fp8_vs_16 below
# with gpu=False (logits of |max| 5.6 / 5.7 / 19.0 / 21.2).  Keys: (h 8192 model, batch).
# The figures are large because the scales are 1.0 and this initialisation's K
# and V lie mostly below 2^-6, where e4m3 is subnormal (absolute error 2^-10).
CPU_FP8_VS_16 = {(False, 3): 0.3829, (False, 24): 0.4710, (True, 3): 4.840, (True, 24): 7.036}


def _model_and_tokens(argv, b, gpu):
    import finetune
    from test_parallel_equivalence import _deterministic_init
    init_framework(argv + (["--bf16"] if gpu else []), finetune.extra_args)
    from epfl_megatron_amd import get_args
    from epfl_megatron_amd.models import ModelType
    from epfl_megatron_amd.training import get_model
    args = get_args()
    model = get_model(finetune.model_provider, ModelType.encoder_or_decoder, wrap_with_ddp=False)
    _deterministic_init(model, args)
    gen = torch.Generator()
    gen.manual_seed(6)
    tokens = torch.randint(0, 512, (b, PLEN + NSTEP), generator=gen)  # the same on CPU and GPU
    return model[0].eval(), tokens.cuda() if gpu else tokens


def _fp8_vs_16(rank, world, big, b, gpu=True):
    """Teacher-forced prefill + decode of one model: the 16-bit cache (fused
    decode layer), the FP8 cache through the fused layer and through the
    unfused layer.  Returns the figures the model-level tests assert on."""
    from test_gpu_e2e import LLAMA_GQA, LLAMA_H8K
    from test_fp8_kv_cache import _teacher_forced
    m, tokens = _model_and_tokens(LLAMA_H8K if big else LLAMA_GQA, b, gpu)
    from epfl_megatron_amd.models import transformer
    from epfl_megatron_amd.ops import fp8_kv
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    calls = [0]
    orig = transformer.ParallelTransformerLayer._forward_decode_fused

    def counted(self, *a, **k):
        calls[0] += 1
        return orig(self, *a, **k)
    transformer.ParallelTransformerLayer._forward_decode_fused = counted
    runs = {}
    for name, fp8, fused in (("ref", False, True), ("ref_unfused", False, False),
                             ("fused", True, True), ("unfused", True, False)):
        transformer.set_fp8_kv_cache(fp8)
        transformer._DECODE_FUSED = fused
        calls[0] = 0
        ip = InferenceParams(b, PLEN + NSTEP)
        logits = _teacher_forced(m, tokens, PLEN, ip)
        runs[name] = (logits, ip, calls[0])
    transformer.set_fp8_kv_cache(False)
    transformer._DECODE_FUSED = True
    lr, ipr, _ = runs["ref"]
    lf, ipf, ncalls = runs["fused"]
    lu, ipu, ucalls = runs["unfused"]
    k16, v16 = ipr.key_value_memory_dict[1]
    ones = torch.ones(k16.shape[2], device=lr.device)
    res = {"fused_calls": ncalls, "unfused_calls": ucalls, "scale": float(lr.abs().max()),
           "fp8_vs_16": float((lf - lr).abs().max()),
           "fused_vs_unfused": float((lf - lu).abs().max()),
           "prefill_equal": bool(torch.equal(lf[:, :PLEN], lr[:, :PLEN])),
           "bytes_16": k16.numel() * k16.element_size(),
           "bytes_8": ipf.key_value_memory_dict[1][0].numel()}
    for name, ip, ref in (("fused", ipf, ipr), ("unfused", ipu, runs["ref_unfused"][1])):
        k8, v8 = ip.key_value_memory_dict[1]
        kr, vr = ref.key_value_memory_dict[1]  # the 16-bit run through the same layer code
        res[name + "_dtype"] = str(k8.dtype)
        res[name + "_layer1"] = bool(torch.equal(k8, fp8_kv.quantize(kr, ones))
                                     and torch.equal(v8, fp8_kv.quantize(vr, ones)))
        res[name + "_decode_rows_written"] = bool((k8[PLEN:] != 0).any() and (v8[PLEN:] != 0).any())
    return res


@functools.lru_cache(maxsize=None)
def _runs(big, b):
    return run_dist(_fp8_vs_16, 1, big, b)[0]


MODEL_CASES = [(False, 3), (False, 24), (True, 3), (True, 24)]


@pytest.mark.parametrize("big,b", MODEL_CASES)
def test_gpu_model_layer1_cache_bytes(big, b):
    """Layer 1's K and V depend only on the embeddings: with the flag on the
    cache bytes equal the quantised layer-1 cache of the 16-bit run, bitwise
    (prefill rows through the store kernel; decode rows through the QKV
    epilogue in the fused layer and through the store kernel in the unfused one)."""
    r = _runs(big, b)
    assert r["fused_dtype"] == "torch.uint8" and 2 * r["bytes_8"] == r["bytes_16"]
    assert r["fused_decode_rows_written"] and r["unfused_decode_rows_written"]
    assert r["fused_layer1"], "fused layer"
    assert r["unfused_layer1"], "unfused layer"


@pytest.mark.parametrize("big,b", MODEL_CASES)
def test_gpu_model_fused_matches_unfused(big, b):
    """Two independent routes over the same cached bytes (the new kernels in
    the fused layer; the store kernel + FP8 decode kernel behind the unfused
    projections), the bound of test_gpu_fused_decode_matches_unfused; the fused
    path is counted on every step."""
    r = _runs(big, b)
    assert r["fused_calls"] == 2 * NSTEP and r["unfused_calls"] == 0, r
    assert r["fused_vs_unfused"] < 2e-2 * max(1.0, r["scale"]), r


@pytest.mark.parametrize("big,b", MODEL_CASES)
def test_gpu_model_fp8_kv_against_16bit_logits(big, b):
    """max |logits(FP8 KV) - logits(16-bit KV)| over prefill 21 + 8 teacher-forced
    steps, bf16 on the GPU, within 3 x the same difference of the same model
    on the CPU fp32 path (CPU_FP8_VS_16; the margin covers bf16 arithmetic on
    top of the quantisation noise).  A wrong scale or layout gives errors of
    the order of the logits themselves.

    (model, b): CPU fp32 figure / GPU bf16 figure / bound (|logits|max)
    LLAMA_GQA b 3:  0.3829 / 0.3970 /  1.149  (5.6)
    LLAMA_GQA b 24: 0.4710 / 0.5098 /  1.413  (5.7)
    LLAMA_H8K b 3:  4.840  / 4.741  / 14.52   (19.0)
    LLAMA_H8K b 24: 7.036  / 5.606  / 21.11   (21.2)
    (profiles/r13a_fp8_kv_cache.txt)
    """
    r = _runs(big, b)
    print(f"fp8 kv vs 16-bit: big={big} b={b} gpu {r['fp8_vs_16']:.4f} cpu "
          f"{CPU_FP8_VS_16[(big, b)]:.4f} bound {3 * CPU_FP8_VS_16[(big, b)]:.4f} "
          f"|logits|max {r['scale']:.2f} fused-vs-unfused {r['fused_vs_unfused']:.4f}")
    assert r["prefill_equal"]  # the restart prefill attends over its fresh 16-bit K / V
    assert 0 < r["fp8_vs_16"] <= 3 * CPU_FP8_VS_16[(big, b)], r


def _graph_decode_fp8(rank, world):
    """GraphedGreedyDecoder under the flag vs the eager FP8-KV greedy loop,
    twice through one captured graph; then one sampling-decoder run."""
    from test_gpu_e2e import LLAMA_GQA
    m, _ = _model_and_tokens(LLAMA_GQA + ["--inference_fp8_kv_cache"], 2, True)
    from epfl_megatron_amd.models import transformer
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    from epfl_megatron_amd.inference.hip_graph import GraphedGreedyDecoder, GraphedSamplingDecoder
    assert transformer._FP8_KV  # the flag set the module switch
    torch.manual_seed(5)
    b, plen, n, cap = 2, 29, 10, 600  # cache longer than one 256-key chunk
    prompt = torch.randint(0, 512, (b, plen), device="cuda")
    pos = torch.arange(cap, device="cuda")[None].expand(b, -1)
    with torch.no_grad():
        ip = InferenceParams(b, cap)
        nxt = m(prompt, pos[:, :plen], None, inference_params=ip)[:, -1].argmax(-1, keepdim=True)
        ip.sequence_len_offset += plen
        first = nxt.clone()
        eager = []
        for t in range(plen, plen + n):
            logits_e = m(nxt, pos[:, t:t + 1], None, inference_params=ip)
            nxt = logits_e[:, -1].argmax(-1, keepdim=True)
            eager.append(nxt)
            ip.sequence_len_offset += 1
        eager = torch.cat(eager, dim=1)
        ip2 = InferenceParams(b, cap)
        m(prompt, pos[:, :plen], None, inference_params=ip2)
        ip2.sequence_len_offset += plen
    assert ip2.key_value_memory_dict[1][0].dtype == torch.uint8
    dec = GraphedGreedyDecoder(m, ip2, b, n)
    out = []
    for _ in range(2):  # the second generation re-primes the same graph
        dec.start(first, plen)
        for _ in range(n):
            dec.step()
        torch.cuda.synchronize()
        out.append(dec.history[:, :n].cpu().tolist())
    lerr = float((dec.logits.float() - logits_e.float()).abs().max())
    with torch.no_grad():
        ip3 = InferenceParams(b, cap)
        m(prompt, pos[:, :plen], None, inference_params=ip3)
        ip3.sequence_len_offset += plen
    sdec = GraphedSamplingDecoder(m, ip3, b, n, vocab_size=512)
    sdec.start(first, plen, top_p=0.9, temperature=1.3)
    for _ in range(n):
        sdec.step()
    torch.cuda.synchronize()
    sampled = sdec.history[:, :n].cpu().tolist()
    return out[0], out[1], eager.cpu().tolist(), lerr, float(logits_e.float().abs().max()), sampled


def test_gpu_graph_decode_matches_eager_under_the_flag():
    graphed, again, eager, lerr, scale, sampled = run_dist(_graph_decode_fp8, 1)[0]
    assert graphed == eager, (graphed, eager)
    assert again == eager
    assert lerr < 2e-2 * max(1.0, scale), (lerr, scale)
    assert all(0 <= t < 512 for row in sampled for t in row) and len(sampled[0]) == 10
