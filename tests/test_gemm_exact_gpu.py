"""Bitwise integer-operand tests of the NT GEMM (csrc/gemm_nt.hip: plain
store, split-K, row maps, strided operands, GLU / dGLU epilogues), the wgrad
GEMM (csrc/gemm_wgrad.hip: both kernels, split plans, token maps), the skinny
decode GEMM (csrc/skinny_gemm.hip) and the layer wiring around them.

Every operand is a small integer times one power of two, so every partial
sum is exact in fp32 whatever the order of accumulation and the expected
output is an fp64 matmul rounded once (``gemm_exact_inputs.py``; the method,
its mutants and the tolerance of the two curved activations are validated on
the CPU in ``test_gemm_exact.py``).  Outputs are pre-filled with NaN where
the kernel must write and with 7 where it must not; nothing is compared
through a norm or an absolute floor.

The first test is the premise: hipBLASLt on the same operands is bitwise
equal to the fp64 reference, i.e. MFMA fp32 accumulation of exactly
representable integers is exact on this hardware.  With it, any mismatch
below is a bug of the kernel under test.
"""
import contextlib

import pytest
import torch

import gemm_exact_inputs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = pytest.mark.parametrize("dtype", G.DTYPES, ids=G.DTYPE_IDS)
NAN = float("nan")


def _ext():
    from epfl_megatron_amd.ops._ext import ext
    return ext()


@contextlib.contextmanager
def _nt_variant(v):
    C = _ext()
    C.gemm_nt_set_variant(v)
    try:
        yield C
    finally:
        C.gemm_nt_set_variant(0)


@contextlib.contextmanager
def _wgrad_variant(v):
    C = _ext()
    C.wgrad_set_variant(v)
    try:
        yield C
    finally:
        C.wgrad_set_variant(4)  # the default


def _filled(shape, value, dtype):
    return torch.full(tuple(shape), value, device=DEV, dtype=dtype)


def _exact(out, expected, what):
    assert G.exact_ok(out, expected), f"{what}: {G.first_mismatch(out, expected)}"


def _e16(a, b, dtype):
    return G.expect16(G.ref_nt(a, b), dtype)


# ---------------------------------------------------------------- the premise

def test_premise_hipblaslt_is_bitwise_on_integer_operands():
    """hipBLASLt, one integer case per training layout, against fp64: the
    forward (NT) on the long-K census operands with a bf16 output, the dgrad
    (NN) with a bf16 output, the wgrad (TN) accumulating into fp32 from g0."""
    C = _ext()
    a, b = G.nt_case(*G.NT_CENSUS, G.BF16, DEV)
    y = _filled((a.shape[0], b.shape[0]), NAN, G.BF16)
    C.lt_gemm(a, False, b, True, y, 1.0, 0.0, -1)
    _exact(y, _e16(a, b, G.BF16), "forward layout, K = 8192")
    M, N, K = 512, 1024, 768
    dy, w = G.nt_case(M, K, N, G.BF16, DEV, seed=1)[0], G.nt_case(N, K, K, G.BF16, DEV, seed=2)[0]
    dx = _filled((M, K), NAN, G.BF16)  # dX [M, K] = dY [M, N] W [N, K]
    C.lt_gemm(dy, False, w, False, dx, 1.0, 0.0, -1)
    _exact(dx, G.expect16(dy.double() @ w.double(), G.BF16), "dgrad layout")
    dyw, x, g0 = G.wgrad_case(4096, 256, 512, G.BF16, DEV)
    g = g0.clone()
    C.lt_gemm(dyw, True, x, False, g, 1.0, 1.0, -1)
    _exact(g, G.ref_wgrad(dyw, x, g0).float(), "wgrad layout, M = 4096, accumulate")


# ---------------------------------------------------------------- gemm_nt: plain store

@DT
@pytest.mark.parametrize("M,N,K,variants", G.NT_PLAIN, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_nt_plain_is_bitwise(M, N, K, variants, dtype):
    a, b = G.nt_case(M, N, K, dtype, DEV)
    e = _e16(a, b, dtype)
    for v in variants:
        with _nt_variant(v) as C:
            c = _filled((M, N), NAN, dtype)
            C.gemm_nt(a, b, c)
        _exact(c, e, f"variant {v}")


@DT
@pytest.mark.parametrize("M,N,K,splits", G.NT_SPLITK)
def test_gemm_nt_split_k_is_bitwise(M, N, K, splits, dtype):
    C = _ext()
    assert C.gemm_nt_ksplit(M, N, K) == splits
    a, b = G.nt_case(M, N, K, dtype, DEV)
    c = _filled((M, N), NAN, dtype)
    C.gemm_nt(a, b, c)
    _exact(c, _e16(a, b, dtype), f"{splits} splits")
    c2 = _filled((M, N), NAN, dtype)
    C.gemm_nt(a, b, c2)
    assert torch.equal(c, c2)


# ---------------------------------------------------------------- gemm_nt: row maps, strides

@DT
@pytest.mark.parametrize("tp,c,R,N,K", G.NT_ROW_MAPS)
def test_gemm_nt_row_maps_are_bitwise(tp, c, R, N, K, dtype):
    """a_map and c_map, every j: the mapped rows are exact, and every row of
    the destination outside the map still holds the sentinel 7."""
    C = _ext()
    full, b = G.nt_case(tp * c * R, N, K, dtype, DEV)
    g = G.nt_case(tp * R, N, K, dtype, DEV, seed=7)[0]
    eg = _e16(g, b, dtype)
    for j in range(c):
        rmap = [R, c * R, j * R]
        idx = G.row_map_index(tp * R, rmap, DEV)
        out = _filled((tp * R, N), NAN, dtype)
        C.gemm_nt(full, b, out, a_map=rmap, m=tp * R)
        _exact(out, _e16(full[idx], b, dtype), f"a_map j={j}")
        dst = _filled((tp * c * R, N), G.SENTINEL, dtype)
        dst[idx] = NAN
        want = _filled((tp * c * R, N), G.SENTINEL, dtype)
        want[idx] = eg
        C.gemm_nt(g, b, dst, c_map=rmap)
        _exact(dst, want, f"c_map j={j}")


@DT
def test_gemm_nt_strided_operands_are_bitwise(dtype):
    """A a column slice of a wider matrix (lda > K), C a column slice of a
    wider sentinel-filled matrix: the slice is exact, the columns on both
    sides of it are intact."""
    s = G.NT_STRIDED
    M, N, K = s["M"], s["N"], s["K"]
    wide_a = G.nt_case(M, N, s["lda"], dtype, DEV, seed=3)[0]
    b = G.nt_case(M, N, K, dtype, DEV)[1]
    a = wide_a[:, s["a0"]:s["a0"] + K]
    assert a.stride(0) == s["lda"] > K
    wide_c = _filled((M, s["ldc"]), G.SENTINEL, dtype)
    out = wide_c[:, s["c0"]:s["c0"] + N]
    out.fill_(NAN)
    want = _filled((M, s["ldc"]), G.SENTINEL, dtype)
    want[:, s["c0"]:s["c0"] + N] = _e16(a, b, dtype)
    _ext().gemm_nt(a, b, out)
    _exact(wide_c, want, "strided")


# ---------------------------------------------------------------- gemm_nt_glu / gemm_nt_dglu

def _glu_check(o, e, s, x2, kind, what):
    """Bitwise (ReGLU / LiGLU) or inside the per-element tolerance with no
    element excluded (SwiGLU / GeGLU); prints the measured margin first."""
    ok, margin = G.glu_ok(o, e, s, x2, kind)
    print(f"[glu margin] {what}: {margin:.3e} (limit {G.GLU_FACTOR:.3e})")
    assert ok, f"{what}: activation margin {margin:.3e} > {G.GLU_FACTOR:.3e}, or a wrong element"


@DT
@pytest.mark.parametrize("kind", list(G.KINDS))
@pytest.mark.parametrize("M,F,K,wmax,shift", G.GLU_SHAPES)
def test_gemm_nt_glu_forward(M, F, K, wmax, shift, kind, dtype):
    """pre is bitwise the rounded product; y is x1 act(x2) of the *rounded*
    pre: bitwise for ReGLU / LiGLU, within ulp + 2^-20 |x1| max(1, |x2|) of the
    fp64 formula for SwiGLU / GeGLU.  Variants 5 and 6 (a case a variant does
    not take falls to the next kernel: only results are asserted).

    Measured on an MI355X: the largest need of the second term over every
    case of this file (forward and backward, both dtypes, both variants) is
    1.33e-08 per unit of s max(1, |x2|), in the GeGLU backward: 1.4 % of 2^-20."""
    x, w1 = G.glu_case(M, F, K, wmax, shift, dtype, DEV)
    pre_e = _e16(x, w1, dtype)
    e, s, x2 = G.glu_expected(pre_e, kind)
    for v in G.GLU_VARIANTS:
        with _nt_variant(v) as C:
            pre, y = _filled((M, 2 * F), NAN, dtype), _filled((M, F), NAN, dtype)
            C.gemm_nt_glu(x, w1, G.KINDS[kind], pre, y)
        _exact(pre, pre_e, f"pre, variant {v}")
        _glu_check(y, e, s, x2, kind, f"y {kind} {(M, F, K)} {dtype} variant {v}")


@DT
@pytest.mark.parametrize("kind", list(G.KINDS))
def test_gemm_nt_glu_forward_through_c_map(kind, dtype):
    """pre and y scattered through a c_map: exact / in tolerance on the mapped
    rows, the sentinel 7 everywhere else."""
    m = G.GLU_CMAP
    tp, c, R, F, K = m["tp"], m["c"], m["R"], m["F"], m["K"]
    x, w1 = G.glu_case(tp * R, F, K, m["wmax"], m["shift"], dtype, DEV)
    pre_e = _e16(x, w1, dtype)
    e, s, x2 = G.glu_expected(pre_e, kind)
    for j in range(c):
        rmap = [R, c * R, j * R]
        idx = G.row_map_index(tp * R, rmap, DEV)
        pre, y = _filled((tp * c * R, 2 * F), G.SENTINEL, dtype), _filled((tp * c * R, F), G.SENTINEL, dtype)
        pre[idx], y[idx] = NAN, NAN
        _ext().gemm_nt_glu(x, w1, G.KINDS[kind], pre, y, rmap)
        want = _filled((tp * c * R, 2 * F), G.SENTINEL, dtype)
        want[idx] = pre_e
        _exact(pre, want, f"pre j={j}")
        _glu_check(y[idx], e, s, x2, kind, f"y {kind} c_map j={j} {dtype}")
        keep = torch.ones(tp * c * R, dtype=torch.bool, device=DEV)
        keep[idx] = False
        assert bool((y[keep] == G.SENTINEL).all())


@DT
@pytest.mark.parametrize("kind", list(G.KINDS))
@pytest.mark.parametrize("M,F,K,wmax,shift", G.GLU_SHAPES)
def test_gemm_nt_dglu_backward(M, F, K, wmax, shift, kind, dtype):
    """d(pre) = [g act(x2), g x1 act'(x2)] with g = dAct rounded to T first:
    both halves bitwise for ReGLU / LiGLU, within ulp + 2^-20 s max(1, |x2|)
    (s = |g|, |g x1|) of the fp64 formula for SwiGLU / GeGLU."""
    dy, w2t, pre = G.dglu_case(M, F, K, wmax, shift, dtype, DEV)
    g = _e16(dy, w2t, dtype)
    e, s, x2 = G.dglu_expected(g, pre, kind)
    for v in G.GLU_VARIANTS:
        with _nt_variant(v) as C:
            d = _filled((M, 2 * F), NAN, dtype)
            C.gemm_nt_dglu(dy, w2t, pre, G.KINDS[kind], d)
        _glu_check(d, e, s, x2, kind, f"dpre {kind} {(M, F, K)} {dtype} variant {v}")


# ---------------------------------------------------------------- wgrad_gemm

def _wgrad_both(C, dy, x, g0, e_acc, e_st, what, xm=()):
    g = g0.clone()
    C.wgrad_gemm(dy, x, g, True, list(xm))
    _exact(g, e_acc, f"{what}, accumulate")
    g = _filled(g0.shape, NAN, torch.float32)
    C.wgrad_gemm(dy, x, g, False, list(xm))
    _exact(g, e_st, f"{what}, store")


def _wgrad_case(M, N, K, xm=None):
    """Operands (bf16; exact in fp16 too) and both fp32 expectations."""
    from epfl_megatron_amd.parallel.tensor.layers import _apply_token_map
    dy, x, g0 = G.wgrad_case(M, N, K, G.BF16, DEV)
    xp = x if xm is None else _apply_token_map(x, tuple(xm), M)
    return dy, x, g0, G.ref_wgrad(dy, xp, g0).float(), G.ref_wgrad(dy, xp).float()


@pytest.mark.parametrize("M,N,K", G.WGRAD_SHAPES)
def test_wgrad_gemm_is_bitwise(M, N, K):
    dy, x, g0, e_acc, e_st = _wgrad_case(M, N, K)
    for dtype in G.DTYPES:
        for v in G.WGRAD_VARIANTS:
            with _wgrad_variant(v) as C:
                _wgrad_both(C, dy.to(dtype), x.to(dtype), g0, e_acc, e_st, f"{dtype} variant {v}")


@pytest.mark.parametrize("shape,plan", G.WGRAD_PLANS, ids=lambda v: str(v).replace(" ", ""))
def test_wgrad_gemm_split_plans_are_bitwise(shape, plan):
    M, N, K = shape
    assert list(_ext().wgrad_plan(M, N, K)) == plan
    dy, x, g0, e_acc, e_st = _wgrad_case(M, N, K)
    for dtype in G.DTYPES:
        for v in G.WGRAD_VARIANTS:
            with _wgrad_variant(v) as C:
                _wgrad_both(C, dy.to(dtype), x.to(dtype), g0, e_acc, e_st, f"{dtype} variant {v}")


@pytest.mark.parametrize("world,c,R,N,K", G.WGRAD_TOKMAPS)
def test_wgrad_gemm_token_maps_are_bitwise(world, c, R, N, K):
    M = world * c * R
    for xm in G.wgrad_tokmaps(world, c, R):
        dy, x, g0, e_acc, e_st = _wgrad_case(M, N, K, xm)
        for dtype in G.DTYPES:
            for v in G.WGRAD_VARIANTS:
                with _wgrad_variant(v) as C:
                    _wgrad_both(C, dy.to(dtype), x.to(dtype), g0, e_acc, e_st,
                                f"map {xm} {dtype} variant {v}", xm)


# ---------------------------------------------------------------- layer wiring

def _param(t, shape):
    p = torch.nn.Parameter(t.clone())
    p.main_grad = _filled(shape, NAN, torch.float32)
    p._mg_fresh = True  # the first micro-batch stores, the later ones accumulate
    return p


@DT
@pytest.mark.parametrize("nt", [False, True], ids=["hipblaslt", "gemm_nt"])
def test_linear_layer_wiring_is_bitwise(nt, dtype, monkeypatch):
    """The linear autograd function: y, dX (through transpose16 and, with the
    NT kernel switched on, gemm_nt) and main_grad after one fresh store and two
    accumulating micro-batches from a NaN fill."""
    from epfl_megatron_amd.parallel.tensor import layers
    monkeypatch.setattr(layers, "_NT_GEMM", nt)
    layers.new_weight_transpose_generation()  # dX through the per-step W^T
    exp = G.wire_linear_expected(dtype, DEV)
    w = _param(exp["w"], exp["w"].shape)
    for i, mb in enumerate(exp["mbs"]):
        x = mb["x"].clone().requires_grad_()
        y = layers.linear_with_grad_accumulation_and_async_allreduce(x, w, None, True, False, False)
        _exact(y.detach(), mb["y"], f"y, micro-batch {i}")
        y.backward(mb["dy"])
        _exact(x.grad, mb["dx"], f"dX, micro-batch {i}")
    assert w.grad is None
    _exact(w.main_grad, exp["main_grad"], "main_grad")


@DT
@pytest.mark.parametrize("nt", [False, True], ids=["hipblaslt", "gemm_nt"])
@pytest.mark.parametrize("kind", G.EXACT_KINDS)
def test_glu_mlp_wiring_is_bitwise(kind, nt, dtype, monkeypatch):
    """glu_mlp with ReGLU / LiGLU (every stage an exact sum or product rounded
    once): out, dX and both main_grads, three micro-batches from a NaN fill."""
    from epfl_megatron_amd.parallel.tensor import layers
    monkeypatch.setattr(layers, "_NT_GEMM", nt)
    layers.new_weight_transpose_generation()
    exp = G.wire_mlp_expected(kind, dtype, DEV)
    w1, w2 = _param(exp["w1"], exp["w1"].shape), _param(exp["w2"], exp["w2"].shape)
    for i, mb in enumerate(exp["mbs"]):
        x = mb["x"].clone().requires_grad_()
        out = layers.glu_mlp(x, w1, w2, kind, sequence_parallel=False, tp_async_allreduce=False,
                             gradient_accumulation_fusion=True)
        _exact(out.detach(), mb["out"], f"out, micro-batch {i}")
        out.backward(mb["dout"])
        _exact(x.grad, mb["dx"], f"dX, micro-batch {i}")
    _exact(w1.main_grad, exp["main_grad1"], "fc1 main_grad")
    _exact(w2.main_grad, exp["main_grad2"], "fc2 main_grad")


# ---------------------------------------------------------------- skinny_gemm

@DT
@pytest.mark.parametrize("M", G.SKINNY_M)
@pytest.mark.parametrize("N,K", G.SKINNY_NK)
def test_skinny_gemm_is_bitwise(N, K, M, dtype):
    """Plain, packed-weight (K % 256 == 0) and residual forms.  The residual
    epilogue is Y = T(T(acc) + R) (the unfused path's two roundings, stated in
    the kernel's header): the expectation rounds twice."""
    from epfl_megatron_amd.ops import decode_pack
    C = _ext()
    x, w, res = G.skinny_case(M, N, K, dtype, DEV)
    e = _e16(x, w, dtype)
    e_res = G.expect16(e.double() + res.double(), dtype)
    with torch.no_grad():
        _exact(C.skinny_gemm(x, w), e, "plain")
        _exact(C.skinny_norm_gemm(x, w, None, 0.0, res), e_res, "residual")
        if K % 256 == 0:
            wp = decode_pack.pack(w)
            _exact(C.skinny_gemm(x, wp, True), e, "packed")
            _exact(C.skinny_norm_gemm(x, wp, None, 0.0, res, True), e_res, "packed, residual")


# ---------------------------------------------------------------- refusals (host checks only)

def test_out_of_contract_arguments_are_refused_on_the_host():
    """Every call here fails a TORCH_CHECK before any launch."""
    C = _ext()
    a, b = G.nt_case(256, 256, 64, G.BF16, DEV)
    bad = [
        lambda: C.gemm_nt(a[:, :48].contiguous(), b[:, :48].contiguous()),       # K % 32
        lambda: C.gemm_nt(a, b[:252]),                                           # N % 8
        lambda: C.gemm_nt(a, b.to(G.FP16)),                                      # dtypes differ
        lambda: C.gemm_nt(a, b, a_map=[128, 256, 128], m=256),                   # rows 128..383 of 256
        lambda: C.gemm_nt(a, b, _filled((256, 256), G.SENTINEL, G.BF16), c_map=[128, 256, 64]),
        lambda: C.gemm_nt(a, b, _filled((256, 256), G.SENTINEL, G.FP16)),        # output dtype
        lambda: C.gemm_nt_glu(a, b, 0, _filled((256, 256), G.SENTINEL, G.BF16)),  # one output of two
        lambda: C.gemm_nt_dglu(a, b, _filled((256, 256), 1.0, G.BF16), 0),       # pre is not [M, 2F]
        lambda: C.wgrad_gemm(a[:48].contiguous(), b[:48].contiguous(),
                             _filled((64, 64), G.SENTINEL, torch.float32), False),  # M % 32
        lambda: C.wgrad_gemm(a, b, _filled((64, 64), G.SENTINEL, G.BF16), False),  # g not fp32
        lambda: C.wgrad_gemm(a, b, _filled((64, 64), G.SENTINEL, torch.float32), False, [48, 2, 128, 48]),
        lambda: C.wgrad_gemm(a, b, _filled((64, 64), G.SENTINEL, torch.float32), False, [64, 2, 256, 64]),
        lambda: C.skinny_gemm(_filled((33, 128), 1.0, G.BF16), _filled((64, 128), 1.0, G.BF16)),  # M > 32
        lambda: C.skinny_gemm(_filled((4, 128), 1.0, G.BF16), _filled((64, 128), 1.0, G.BF16), True),  # packed, K % 256
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} was accepted")
