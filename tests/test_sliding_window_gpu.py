"""Sliding-window attention in the gfx950 FlashAttention and decode kernels
against the fp32 reference ``attention_ref(..., window=W)``.

Key k is visible to query q iff ``q + (sk - sq) - W < k <= q + (sk - sq)``.
The window is a per-row lower key bound folded into the document-mask path of
the forward / dQ kernels (tile skipping from the block's first row), an upper
query bound per key block in the dK/dV kernel and a lower key bound in the
split-key decode kernel.
"""
import pytest
import torch

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


def _qkv(b, sq, sk, nq, nkv, hd, seed, grad=True):
    torch.manual_seed(seed)
    q = torch.randn(b, sq, nq, hd, device=DEV, dtype=torch.bfloat16, requires_grad=grad)
    k = torch.randn(b, sk, nkv, hd, device=DEV, dtype=torch.bfloat16, requires_grad=grad)
    v = torch.randn(b, sk, nkv, hd, device=DEV, dtype=torch.bfloat16, requires_grad=grad)
    return q, k, v


def _fwd_bwd(q, k, v, g, window):
    from epfl_megatron_amd.ops.attention import flash_attn_func
    for t in (q, k, v):
        t.grad = None
    o = flash_attn_func(q, k, v, causal=True, window=window)
    o.backward(g)
    return [o.detach().clone()] + [t.grad.clone() for t in (q, k, v)]


def _against_ref(q, k, v, window, seed=5, what="window"):
    """fwd + bwd of flash_attn_func against the fp32 reference on the GPU."""
    from epfl_megatron_amd.ops.attention import attention_ref
    torch.manual_seed(seed)
    g = torch.randn(q.shape, device=DEV, dtype=torch.bfloat16)
    got = _fwd_bwd(q, k, v, g, window)
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    orf = attention_ref(qr, kr, vr, causal=True, window=window)
    orf.backward(g.float())
    _close(got[0], orf, 2e-2, 2e-2, f"{what} fwd")
    for a, r, name in zip(got[1:], (qr, kr, vr), ("dq", "dk", "dv")):
        _close(a, r.grad, 5e-2, 5e-2, f"{what} {name}")
    return got, g


def test_reference_window_rows():
    """The oracle itself: with W = 8 row 20 attends keys 13..20 only and rows
    < W equal full causal."""
    from epfl_megatron_amd.ops.attention import attention_ref
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 32, 2, 16, device=DEV) for _ in range(3))
    full = attention_ref(q, k, v, causal=True)
    win = attention_ref(q, k, v, causal=True, window=8)
    assert torch.equal(win[:, :8], full[:, :8])
    assert not torch.allclose(win[:, 20], full[:, 20])
    k2, v2 = k.clone(), v.clone()
    k2[:, :13], v2[:, :13] = 7.0, -3.0  # row 20 must not see keys < 13
    k2[:, 21:], v2[:, 21:] = 5.0, 9.0
    assert torch.equal(attention_ref(q, k2, v2, causal=True, window=8)[:, 20], win[:, 20])


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (4, 1)])
@pytest.mark.parametrize("W", [1, 37, 64, 200, 599, 600, 5000])
def test_flash_attention_window(W, nq, nkv, hd):
    """Windows inside one 64-key tile, off the tile grid, of exactly one tile,
    spanning 128-row blocks, and >= s (bitwise the window-less result)."""
    b, s = 2, 600
    q, k, v = _qkv(b, s, s, nq, nkv, hd, seed=W + nq + hd)
    got, g = _against_ref(q, k, v, W)
    if W >= s:
        for a, bb, name in zip(got, _fwd_bwd(q, k, v, g, 0), ("o", "dq", "dk", "dv")):
            assert torch.equal(a, bb), name


def test_flash_attention_window_8wave():
    """A grid large enough for the 8-wave forward and dQ (3-slot K/V ring
    started at the block's first visible tile)."""
    b, s, nq, W = 4, 1024, 32, 300
    assert (s + 255) // 256 * nq * b >= 512  # flash_attn_waves() picks 8
    _against_ref(*_qkv(b, s, s, nq, nq, 128, seed=31), W, what="8-wave window")


@pytest.mark.parametrize("kv2", [True, False])
def test_flash_attention_window_split_key(kv2):
    """The split-key forward / dQ grid (one 4-wave block per CU): the halves of
    [t0, ntiles) and their LDS merge under a window, and the 4-wave kernels on
    the same shape."""
    C = _ext()
    C.fa_set_kv2(kv2)
    try:
        _against_ref(*_qkv(1, 4096, 4096, 8, 1, 128, seed=32), 1000, what=f"kv2={kv2} window")
    finally:
        C.fa_set_kv2(True)


def test_flash_attention_window_pairing():
    """The paired causal grid (two 4-wave blocks per CU) with a window: pairing
    on and off bitwise equal."""
    C = _ext()
    b, s, nq, W = 1, 4096, 16, 700
    q, k, v = _qkv(b, s, s, nq, nq, 128, seed=33)
    g = torch.randn(b, s, nq, 128, device=DEV, dtype=torch.bfloat16)
    outs = []
    for on in (True, False):
        C.fa_set_pairing(on)
        try:
            outs.append(_fwd_bwd(q, k, v, g, W))
        finally:
            C.fa_set_pairing(True)
    for a, bb, name in zip(outs[0], outs[1], ("o", "dq", "dk", "dv")):
        assert torch.equal(a, bb), name


def _packed_tokens(b, s, seed, eod=0):
    """Token rows of packed documents: EODs at random places, one near the
    start, a 1-token document straddling a 64-key tile edge."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 100, (b, s), generator=g)
    for i in range(b):
        n = int(torch.randint(1, 6, (1,), generator=g))
        t[i, torch.randint(0, s, (n,), generator=g)] = eod
        if i == 0:
            t[i, 2] = eod
            t[i, 63:65] = eod
    return t


@pytest.mark.parametrize("with_docs", [False, True])
@pytest.mark.parametrize("s,b,ng,r,hd", [(600, 2, 2, 3, 128), (333, 3, 1, 8, 64)])
def test_flash_attention_window_qkvpacked(s, b, ng, r, hd, with_docs):
    """The training entry: fused RoPE, a window of 100 and (with_docs) packed
    documents -- the row's bound is max(document start, row - W + 1) -- fwd and
    bwd against the fp32 CPU reference."""
    from epfl_megatron_amd.ops.attention import flash_attn_qkvpacked
    from epfl_megatron_amd.ops.rope import rope_table
    from epfl_megatron_amd.utils.misc import get_ltor_masks_and_position_ids
    W = 100
    docs = pos = None
    if with_docs:
        tokens = _packed_tokens(b, s, seed=s + b).to(DEV)
        docs, _, pos = get_ltor_masks_and_position_ids(tokens, 0, True, True, False,
                                                        flash_doc_bounds=True)
        assert docs.dtype == torch.int32 and docs.shape == (2, b, s)
    cos, sin = rope_table(hd, 8192, DEV)
    torch.manual_seed(s)
    x = torch.randn(s, b, ng * (r + 2) * hd, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    o = flash_attn_qkvpacked(x.clone(), ng, r, hd, causal=True, rope=(cos, sin), position_ids=pos,
                             doc_bounds=docs, window=W)
    xr = x.detach().float().cpu().requires_grad_()
    orf = flash_attn_qkvpacked(xr, ng, r, hd, causal=True, rope=(cos.cpu(), sin.cpu()),
                               position_ids=None if pos is None else pos.cpu(),
                               doc_bounds=None if docs is None else docs.cpu(), window=W)
    _close(o.cpu(), orf, 3e-2, 3e-2, "windowed qkvpacked fwd")
    g = torch.randn_like(o)
    o.backward(g)
    orf.backward(g.float().cpu())
    _close(x.grad.cpu(), xr.grad, 6e-2, 6e-2, "windowed qkvpacked bwd")


@pytest.mark.parametrize("W", [50, 100, 400])
def test_flash_attention_window_prefill_offset(W):
    """KV-cache prefill: 70 new queries over 333 keys, the window measured from
    the bottom-right aligned diagonal."""
    from epfl_megatron_amd.ops.attention import attention_ref, flash_attn_func
    q, k, v = _qkv(2, 70, 333, 8, 2, 128, seed=W, grad=False)
    o = flash_attn_func(q, k, v, causal=True, window=W)
    _close(o, attention_ref(q.float(), k.float(), v.float(), causal=True, window=W), 2e-2, 2e-2,
           "windowed prefill")


def test_flash_attention_window_bwd_kv_longer():
    """Backward with sk > sq, ragged tiles and a window."""
    torch.manual_seed(11)
    q = torch.randn(1, 100, 4, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(1, 230, 2, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(1, 230, 2, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    _against_ref(q, k, v, 100, what="window (sk > sq)")


@pytest.mark.parametrize("W", [1, 100, 256, 5000])
@pytest.mark.parametrize("b,sk,nq,nkv,hd", [(2, 77, 8, 2, 128), (3, 1000, 64, 8, 128),
                                              (1, 300, 71, 1, 64)])
def test_flash_decode_window(b, sk, nq, nkv, hd, W):
    """Single-token decode over the last W cached keys: the key count from the
    host (the cache sliced to sk keys) and from the device (kv_len, whole cache)."""
    from epfl_megatron_amd.ops.attention import (attention_ref, flash_attn_func,
                                                 flash_decode_cached)
    torch.manual_seed(sk + nq + W)
    kmem = torch.randn(sk + 70, b + 1, nkv, hd, device=DEV, dtype=torch.bfloat16)
    vmem = torch.randn(sk + 70, b + 1, nkv, hd, device=DEV, dtype=torch.bfloat16)
    q = (torch.randn(1, b, nq, hd, device=DEV, dtype=torch.bfloat16) * 2).transpose(0, 1)
    keys, vals = kmem[:sk, 1:b + 1].transpose(0, 1), vmem[:sk, 1:b + 1].transpose(0, 1)
    ref = attention_ref(q.float(), keys.float(), vals.float(), causal=True, window=W)
    with torch.no_grad():
        o = flash_attn_func(q, keys, vals, causal=True, window=W)
        kv_len = torch.tensor([sk], device=DEV, dtype=torch.int32)
        oc = flash_decode_cached(q, kmem[:, 1:b + 1].transpose(0, 1),
                                 vmem[:, 1:b + 1].transpose(0, 1), kv_len, window=W)
    _close(o, ref, 2e-2, 2e-2, "windowed decode (host length)")
    _close(oc, ref, 2e-2, 2e-2, "windowed decode (device length)")


def test_flash_attention_window_skips_and_masks():
    """Keys below every window of rows >= 512 (s = 1024, W = 100: keys < 413)
    replaced by other finite values: those rows' outputs and dQ, and dK / dV of
    keys >= 512, stay bitwise the same -- tiles below the window are skipped or
    masked to exact zeros.  Finite values: 0 x NaN would poison a loaded tile."""
    b, s, nq, nkv, hd, W = 1, 1024, 4, 2, 128, 100
    q, k, v = _qkv(b, s, s, nq, nkv, hd, seed=41)
    torch.manual_seed(42)
    g = torch.randn(b, s, nq, hd, device=DEV, dtype=torch.bfloat16)
    base = _fwd_bwd(q, k, v, g, W)
    cut = 512 - (W - 1)
    k2, v2 = k.detach().clone(), v.detach().clone()
    k2[:, :cut] = (torch.randn_like(k2[:, :cut].float()) * 50).to(k2.dtype)
    v2[:, :cut] = (torch.randn_like(v2[:, :cut].float()) * 50).to(v2.dtype)
    k2.requires_grad_()
    v2.requires_grad_()
    other = _fwd_bwd(q, k2, v2, g, W)
    assert torch.equal(base[0][:, 512:], other[0][:, 512:]), "o"
    assert torch.equal(base[1][:, 512:], other[1][:, 512:]), "dq"
    assert torch.equal(base[2][:, 512:], other[2][:, 512:]), "dk"
    assert torch.equal(base[3][:, 512:], other[3][:, 512:]), "dv"
    assert not torch.equal(base[0][:, :cut], other[0][:, :cut])  # the replacement is seen elsewhere


def test_flash_attention_window_deterministic():
    q, k, v = _qkv(2, 600, 600, 8, 2, 128, seed=51)
    g = torch.randn(2, 600, 8, 128, device=DEV, dtype=torch.bfloat16)
    a, bb = _fwd_bwd(q, k, v, g, 200), _fwd_bwd(q, k, v, g, 200)
    for x, y, name in zip(a, bb, ("o", "dq", "dk", "dv")):
        assert torch.equal(x, y), name


def test_window_needs_causal():
    from epfl_megatron_amd.ops.attention import flash_attn_func
    q, k, v = _qkv(1, 64, 64, 2, 2, 64, seed=1, grad=False)
    with pytest.raises(ValueError):
        flash_attn_func(q, k, v, causal=False, window=8)
    lse = torch.empty(1, 2, 64, device=DEV)
    with pytest.raises(RuntimeError):
        _ext().flash_attn_fwd(q, k, v, torch.empty_like(q), lse, 1, 64, 64, 2, 2, 64,
                              [q.stride(0), q.stride(1), q.stride(2), q.stride(2)],
                              [k.stride(0), k.stride(1), k.stride(2)],
                              [k.stride(0), k.stride(1), k.stride(2)],
                              [q.stride(0), q.stride(1), q.stride(2)], False, 0.125,
                              None, None, None, None, window=8)
