"""Inputs, expected values, checks and plain-torch emulations for the exact
mask-edge tests of the decode and FlashAttention kernels
(``test_attention_edges.py`` on the CPU, ``test_attention_edges_gpu.py`` on
the GPU; both take their cases from here, so they cannot drift apart).

Two families of inputs make a single wrongly admitted or dropped key visible:

* census: Q = 0, so every score is 0 and every unnormalised probability is
  exactly 1, whatever P is rounded to.  The output is (visible keys per
  column) / (visible keys) with one final rounding, the log-sum-exp is
  ln(visible keys), and both follow from the mask rule alone.  Every quantity
  is non-negative, so the checks need no absolute tolerance.
* needle: every (batch, head) aims its query at one target key whose softmax
  weight is >= 1 - 2^-20; for a visible target the output is that key's V row
  exactly, for an invisible one it is an O(1) soft mixture of the others.

Nothing here is kernel code: pure torch, on whatever device the caller asks.
"""
import functools
import math

import torch

LOG2E = 1.4426950408889634

# ---------------------------------------------------------------- units in the last place

MANT = {torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}  # smallest normal exponent


def ulp(e, dtype):
    """Spacing of ``dtype`` at the (fp64) values ``e`` > 0 that are exact in ``dtype``."""
    _, ex = torch.frexp(e.double())  # e = m 2^ex, m in [0.5, 1)
    ex = torch.clamp(ex - 1, min=MIN_EXP[dtype])
    return torch.ldexp(torch.ones_like(e, dtype=torch.float64), ex - MANT[dtype])


def _per_case(bad):
    return ~bad.reshape(bad.shape[0], -1).any(dim=1)


def census_ok(o, e64, tol_ulp=1.0):
    """Per leading index: every element of ``o`` within ``tol_ulp`` ulp(E) of E =
    ``e64`` rounded to o's dtype, and exactly 0 where E is 0.  NaN fails.
    (Accumulators are exact integers, there is one division, and o / L may be
    lowered to a reciprocal multiply: 1 ulp.)"""
    E = e64.to(o.dtype).double()
    O = o.double()
    zero = E == 0
    err = (O - E).abs() / ulp(torch.where(zero, torch.ones_like(E), E), o.dtype)
    bad = torch.where(zero, O != 0, ~(err <= tol_ulp))
    return _per_case(bad)


def census_separation(e64, emut64, dtype):
    """Per leading index: the largest distance, in ulps of ``dtype`` at the
    correctly rounded expectation, between a mutant's exact expectation and
    the correctly rounded one (inf where one is zero and the other is not)."""
    E = e64.to(dtype).double()
    zero = E == 0
    sep = (emut64 - E).abs() / ulp(torch.where(zero, torch.ones_like(E), E), dtype)
    sep = torch.where(zero, torch.where(emut64 != 0, math.inf, 0.0), sep)
    return sep.reshape(sep.shape[0], -1).amax(dim=1)


def close_ok(o, ref64, atol=2e-2, rtol=2e-2):
    """Element mask of the suite's ``_close`` (NaN / inf count as off)."""
    return (o.double() - ref64).abs() <= atol + rtol * ref64.abs()


# ---------------------------------------------------------------- census values

def census_values(cap, hd, nkv, rows=None):
    """V ``[rows or cap, nkv, hd]`` fp32 of 0 / 2^-g.  Column d < hd / 2 is set
    where ``j // ceil(cap / (hd / 2)) == d`` (a contiguous block census: a
    dropped chunk empties columns); column hd / 2 + d where ``j % (hd / 2) ==
    d`` (separates neighbours and short lengths).  KV group g is scaled by
    2^-g so that a wrong group index shows.  Exact in bf16, fp16 and e4m3."""
    h = hd // 2
    blk = -(-cap // h)
    j = torch.arange(rows if rows is not None else cap)[:, None]
    d = torch.arange(h)[None, :]
    base = torch.cat([j // blk == d, j % h == d], dim=1).float()
    g = torch.ldexp(torch.ones(nkv), -torch.arange(nkv))
    return base[:, None, :] * g[None, :, None]


def census_expected(v, lo=None, hi=None, vis=None):
    """fp64 expected output of uniform attention.  ``v [..., sk, nkv, hd]``;
    the visible keys are ``[lo, hi)`` or the rows of a boolean ``vis [..., sq,
    sk]`` -> ``[..., sq, nkv, hd]`` (no sq axis with lo / hi).  A row without
    visible keys gives 0."""
    v = v.double()
    if vis is None:
        j = torch.arange(v.shape[-3], device=v.device)
        return census_expected(v, vis=((j >= lo) & (j < hi))[None]).squeeze(-3)
    w = vis.double()
    cnt = w.sum(-1)
    num = torch.einsum("...ij,...jgd->...igd", w, v)
    return num / cnt.clamp(min=1)[..., None, None]


def needle_values(rows, hd, salt=0):
    """``[rows, hd]`` fp32 of +-(1 + m / 8), m in 0..7: sign and m from a fixed
    hash of (row, column), so neighbouring rows differ in most columns."""
    j = torch.arange(rows, dtype=torch.int64)[:, None]
    d = torch.arange(hd, dtype=torch.int64)[None, :]
    x = (j * 2654435761 + d * 40503 + salt * 7919 + 12345) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 2246822519) & 0xFFFFFFFF
    x = x ^ (x >> 13)
    sign = 1.0 - 2.0 * ((x >> 3) & 1).float()
    return sign * (1.0 + (x & 7).float() / 8.0)


# ---------------------------------------------------------------- the mask rule and its mutants

def visibility(sq, sk, causal, window=0, doc_start=None, mutant=None):
    """Boolean ``[sq, sk]`` (``[b, sq, sk]`` with ``doc_start [b, sq]``): key j
    is visible to query i iff ``j <= i + coff`` (causal, coff = sk - sq),
    ``j > i + coff - window`` (window > 0) and ``j >= doc_start[i]``.
    ``mutant`` bends one of the three rules by one key, or drops a 64-key tile
    for the last 128 rows."""
    i = torch.arange(sq)[:, None]
    j = torch.arange(sk)[None, :]
    coff = sk - sq
    vis = torch.ones(sq, sk, dtype=torch.bool)
    if causal:
        vis = vis & (j <= i + coff + (1 if mutant == "diag+1" else 0))
    if window:
        lo = i + coff - window + {"window_lo+1": 1, "window_lo-1": -1}.get(mutant, 0)
        vis = vis & (j > lo)
    if doc_start is not None:
        ds = doc_start.long()[..., None] - (1 if mutant == "doc-1" else 0)
        vis = vis & (j >= ds)
    if mutant == "tile_dropped":
        last = vis[..., -1, :].reshape(-1, sk)[0].nonzero().flatten()
        t0 = int(last[len(last) // 2]) // 64 * 64  # the tile of the last row's middle visible key
        vis = vis & ~((i >= sq - 128) & (j >= t0) & (j < t0 + 64))
    return vis


PREFILL_MUTANTS = ("diag+1", "window_lo+1", "window_lo-1", "doc-1", "tile_dropped")


def decode_visibility(n, window, rows, mutant=None):
    """Boolean ``[rows]`` over the physical cache rows: decode sees the last
    ``window`` (0: all) of the first ``n`` keys.  Mutants: the newest key
    dropped, key ``n`` admitted, the window's lower bound off by one, one
    whole chunk of 32 / 64 / 256 keys dropped (the one holding the middle
    visible key)."""
    j = torch.arange(rows)
    dlo = {"window_lo+1": 1, "window_lo-1": -1}.get(mutant, 0)
    lo = max(n - window + dlo, 0) if window else 0
    hi = n + {"newest_dropped": -1, "kv_len_admitted": 1}.get(mutant, 0)
    vis = (j >= lo) & (j < hi)
    if mutant is not None and mutant.startswith("chunk_dropped_") and hi > lo:
        size = int(mutant.rsplit("_", 1)[1])
        c0 = ((lo + hi - 1) // 2) // size * size
        vis = vis & ~((j >= c0) & (j < c0 + size))
    return vis


DECODE_SINGLE_KEY_MUTANTS = ("newest_dropped", "kv_len_admitted", "window_lo+1", "window_lo-1")
DECODE_MUTANTS = DECODE_SINGLE_KEY_MUTANTS + ("chunk_dropped_32", "chunk_dropped_64",
                                              "chunk_dropped_256")

# ---------------------------------------------------------------- decode cases

DECODE_B, DECODE_NKV, DECODE_PAD_ROWS = 2, 2, 8
DECODE_R = (1, 2, 3, 4, 7, 8, 12)  # all four heads-per-workgroup forms; 3, 7, 12: partial last slice
# (capacity, keys per wave): 19 / 10 / 3 chunks (one, two and three batches of
# the 8-wide combine loop, ragged ends), and the one-chunk form that writes O directly
DECODE_CONFIGS = ((600, 8), (600, 16), (600, 64), (200, 64))
DECODE_LENS = {600: (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 599, 600, 605),
               200: (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 199, 200, 205)}
DECODE_WINDOWS = {600: (1, 2, 33, 256, 257, 599, 600, 5000), 200: (1, 2, 33, 199, 200, 5000)}
CHUNK_EDGES = (32, 64, 256, 512)  # 256 and 512 are chunk edges at every keys-per-wave


@functools.lru_cache(maxsize=None)
def decode_cases(cap):
    """(device kv_len, window) pairs: every length without a window; every
    window with the lengths that put its lower edge klo = n - W one before,
    on and one after a chunk edge of each keys-per-wave, plus lengths inside
    the window, the full cache and a kv_len past the capacity."""
    cases = [(n, 0) for n in DECODE_LENS[cap]]
    for w in DECODE_WINDOWS[cap]:
        ns = {1, min(w, cap), min(w + 1, cap), cap, cap + 5}
        ns |= {w + e + d for e in CHUNK_EDGES for d in (-1, 0, 1) if w + e + d <= cap}
        cases += [(n, w) for n in sorted(ns)]
    return tuple(cases)


def decode_targets(n, window, npairs):
    """Needle targets of one case, round-robin over the (batch, head) pairs:
    the newest key, the first key past the length, both sides of the window
    edge, both sides of the last chunk edge, key 0, n - 2 and n + 1.  (The
    first four are the keys the single-key mutants move, so they come first:
    MHA at batch 2 has only four pairs.)"""
    klo = max(n - window, 0) if window else 0
    size = next((s for s in (256, 64, 32) if (n - 1) // s >= 1), 0)
    edge = (n - 1) // size * size if size else 0
    cand = [n - 1, n, klo, klo - 1, edge - 1, edge, 0, n - 2, n + 1]
    cand = [t if t >= 0 else 0 for t in cand]
    return [cand[p % len(cand)] for p in range(npairs)]


class DecodeInputs:
    """One (dtype, hd, r, cache type, capacity) of the decode matrix: the
    physical caches ``[cap + 8, b + 1, nkv, hd]`` (batch slot 0 is padding) as
    fp32 stored values, scales, queries, and the fp64 expectations of every case."""


@functools.lru_cache(maxsize=4)
def decode_inputs(dtype, hd, r, fp8, cap, device="cpu"):
    from epfl_megatron_amd.ops import fp8_kv
    b, nkv = DECODE_B, DECODE_NKV
    nq, rows = r * nkv, cap + DECODE_PAD_ROWS
    gen = torch.Generator().manual_seed(1000 * hd + 10 * r + cap + int(fp8))
    x = DecodeInputs()
    x.dtype, x.hd, x.r, x.fp8, x.cap, x.nq, x.rows = dtype, hd, r, fp8, cap, nq, rows
    x.cases = decode_cases(cap)
    C = len(x.cases)
    x.n_eff = torch.tensor([min(n, cap) for n, _ in x.cases])
    x.klo = torch.tensor([max(min(n, cap) - w, 0) if w else 0 for n, w in x.cases])
    x.vis = torch.stack([decode_visibility(min(n, cap), w, rows) for n, w in x.cases]).to(device)
    # scales: powers of two that differ per head (1.0 for the 16-bit cache)
    x.k_scale = torch.tensor([2.0 ** -6, 2.0 ** -5]) if fp8 else torch.ones(nkv)
    x.v_scale = torch.tensor([2.0 ** -2, 2.0 ** -3]) if fp8 else torch.ones(nkv)
    # K: N(0, 1) rounded to the cache type (stored value = byte / 16-bit value)
    # (rows with |k|^2 < hd redrawn, first of 8 draws that has it: a short target
    # row does not reach the weight 1 - 2^-20 that the needle check rests on)
    draws = torch.randn(8, rows, b + 1, nkv, hd, generator=gen)
    n2 = draws.square().sum(-1)
    pick = torch.where((n2 >= hd).any(0), (n2 >= hd).int().argmax(0), n2.argmax(0))
    kreal = torch.gather(draws, 0, pick[None, ..., None].expand(1, rows, b + 1, nkv, hd))[0]
    if fp8:
        x.k = fp8_kv.dequantize(fp8_kv.quantize(kreal, x.k_scale), torch.ones(nkv))
    else:
        x.k = kreal.to(dtype).float()
    # census V: batch slot s scaled by 2^-(nkv s), so a wrong batch index shows
    cv = census_values(cap, hd, nkv, rows) / x.v_scale[None, :, None]
    slot = torch.ldexp(torch.ones(b + 1), -nkv * torch.arange(b + 1).roll(1))  # slot 0: the smallest
    x.v_census = cv[:, None] * slot[None, :, None, None]
    x.v_needle = torch.stack([torch.stack([needle_values(rows, hd, salt=10 * s + g) for g in range(nkv)], 1)
                              for s in range(b + 1)], 1)
    for t in (x.v_census, x.v_needle):  # exact in every cache type
        assert torch.equal(t.to(torch.float8_e4m3fn).float(), t) and torch.equal(t.to(dtype).float(), t)
    # needle queries: q = round(c k_t), c = 4 at head_dim 128 and 6 at 64
    x.targets = torch.tensor([decode_targets(int(n), w, b * nq)
                              for n, (_, w) in zip(x.n_eff, x.cases)]).view(C, b, nq)
    grp = (torch.arange(nq) // r)[None, None, :].expand(C, b, nq)
    bat = torch.arange(b)[None, :, None].expand(C, b, nq)
    kt = x.k[x.targets, bat + 1, grp] * x.k_scale[grp][..., None]
    x.q_needle = ((4.0 if hd == 128 else 6.0) * kt).to(dtype)
    x.q_census = torch.zeros(b, 1, nq, hd, dtype=dtype)
    x.scale = hd ** -0.5
    for name in ("k", "v_census", "v_needle", "k_scale", "v_scale", "targets", "q_needle", "q_census",
                 "n_eff", "klo"):
        setattr(x, name, getattr(x, name).to(device))
    # expectations (fp64)
    x.census_e = decode_census_expected(x, x.vis)
    x.t_visible = torch.gather(x.vis[:, None, :].expand(C, b * nq, rows), 2,
                               x.targets.view(C, b * nq, 1)).view(C, b, nq)
    p, x.needle_ref = decode_reference(x, x.vis)
    wt = torch.gather(p, 3, x.targets[..., None]).squeeze(-1)
    x.min_target_weight = float(wt[x.t_visible].min()) if bool(x.t_visible.any()) else 1.0
    grp, bat = grp.to(device), bat.to(device)
    x.needle_e = (x.v_needle[x.targets, bat + 1, grp] * x.v_scale[grp][..., None]).double()
    return x


def _views(x, t):
    """Physical ``[rows, b + 1, nkv, hd]`` -> the sequences' ``[b, rows, nkv, hd]``."""
    return t[:, 1:].transpose(0, 1)


def decode_census_expected(x, vis):
    """``[C, b, nq, hd]`` fp64 for the visibility rows ``vis [C, rows]``."""
    v = _views(x, x.v_census).double() * x.v_scale.double()[None, None, :, None]
    e = torch.einsum("cj,bjgd->cbgd", vis.double(), v) / vis.sum(-1).clamp(min=1)[:, None, None, None]
    return e.repeat_interleave(x.r, dim=2)


def decode_reference(x, vis):
    """fp64 attention of the needle queries over the visible keys: the
    probabilities ``[C, b, nq, rows]`` and the output ``[C, b, nq, hd]`` (0
    where no key is visible)."""
    C, b, nkv = vis.shape[0], DECODE_B, DECODE_NKV
    k = _views(x, x.k).double() * x.k_scale.double()[None, None, :, None]
    v = _views(x, x.v_needle).double() * x.v_scale.double()[None, None, :, None]
    q = x.q_needle.double().reshape(C, b, nkv, x.r, x.hd)
    s = torch.einsum("cbgrd,bjgd->cbgrj", q, k) * x.scale
    s = s.masked_fill(~vis[:, None, None, None, :], -math.inf)
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)  # no visible key: all -inf
    o = torch.einsum("cbgrj,bjgd->cbgrd", p, v)
    return p.reshape(C, b, x.nq, -1), o.reshape(C, b, x.nq, x.hd)


def needle_ok(o, x):
    """Per case: visible targets give V[t] v_scale bit for bit, invisible ones
    the fp64 reference within the suite's 2e-2 / 2e-2 (the output is O(1)
    there, a leak is an O(1) error)."""
    exact = o.double() == x.needle_e
    soft = close_ok(o, x.needle_ref)
    bad = ~torch.where(x.t_visible[..., None], exact, soft)
    return _per_case(bad)


def decode_emulate(x, q, v, vis, kpw, v_swap=False):
    """The decode algorithm in plain fp32 torch: chunks of 4 kpw keys, per
    chunk the maximum, the sum of exp2 and the unnormalised partial output,
    then the in-order combine and one rounding to the output type.  ``q [C,
    b, nq, hd]`` (or ``[b, 1, nq, hd]`` for all cases), ``v`` the physical V
    cache, ``vis [C, rows]`` the keys each case admits (a mutant passes its
    own).  ``v_swap``: P.V reads the V row of each key's neighbour (j ^ 1)."""
    C, b, nkv, hd, r = vis.shape[0], DECODE_B, DECODE_NKV, x.hd, x.r
    ch = 4 * kpw
    ns = -(-x.cap // ch)
    pad = ns * ch - x.rows
    kk, vv = _views(x, x.k).float(), _views(x, v).float()
    if v_swap:
        vv = vv[:, torch.arange(x.rows, device=vv.device) ^ 1]
    if pad > 0:
        kk = torch.nn.functional.pad(kk, (0, 0, 0, 0, 0, pad))
        vv = torch.nn.functional.pad(vv, (0, 0, 0, 0, 0, pad))
        vis = torch.nn.functional.pad(vis, (0, pad))
    kk, vv, vis = kk[:, :ns * ch], vv[:, :ns * ch], vis[:, :ns * ch]
    if q.dim() == 4 and q.shape[1] == 1 and q.shape[0] == b:
        q = q.transpose(0, 1).expand(C, b, x.nq, hd)
    q5 = q.float().reshape(C, b, nkv, r, hd)
    sl2 = (torch.tensor(x.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
           * x.k_scale.float())  # the K scale folded into the score scale
    s = torch.einsum("cbgrd,bjgd->cbgrj", q5, kk) * sl2[None, None, :, None, None]
    s = s.masked_fill(~vis[:, None, None, None, :], -math.inf).reshape(C, b, nkv, r, ns, ch)
    m = s.amax(-1)
    p = torch.where(torch.isinf(m)[..., None], torch.zeros_like(s), torch.exp2(s - m[..., None]))
    l = p.sum(-1)
    o = torch.einsum("cbgrsj,bsjgd->cbgrsd", p, vv.reshape(b, ns, ch, nkv, hd))
    M = m.amax(-1, keepdim=True)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
    L = torch.zeros_like(l[..., 0])
    O = torch.zeros_like(o[..., 0, :])
    for sp in range(ns):  # splits in order
        L = L + l[..., sp] * w[..., sp]
        O = O + o[..., sp, :] * w[..., sp, None]
    out = torch.where(L[..., None] > 0, O / L[..., None] * x.v_scale.float()[None, None, :, None, None],
                      torch.zeros_like(O))
    return out.to(x.dtype).reshape(C, b, x.nq, hd)


# ---------------------------------------------------------------- prefill cases

PREFILL_B = 2
PREFILL_S = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)
PREFILL_HEADS = ((4, 4), (8, 2))
PREFILL_SQ_LT_SK = ((5, 70), (130, 257))
DOC_STARTS = ((0, 63, 64, 128, 257), (0, 65, 129, 256))  # batch 0, batch 1
DOC_S = (129, 257, 600)
DV_S = (65, 129, 257, 600)
DV_SQ_LT_SK = ((100, 230),)
# larger grids, forward only: (b, s, nq, nkv, hd, what)
# (the smallest grid that picks the 8-wave forward; one 4-wave block per CU: the
# split-key forward; exactly two 4-wave blocks per CU: the causal pairing)
PREFILL_BIG = ((2, 1024, 64, 8, 128, "8-wave"), (1, 4096, 8, 1, 128, "split-key"),
               (1, 4096, 16, 2, 128, "pairing"))


def _windows(sk):
    return sorted({w for w in (1, 2, 63, 64, 65, 128, 129, sk - 1, sk) if 1 <= w <= sk})


@functools.lru_cache(maxsize=None)
def prefill_cases():
    """(sq, sk, causal, window, docs) of the forward census; docs: the
    per-batch document starts or None."""
    cases = []
    for s in PREFILL_S:
        cases += [(s, s, False, 0, None), (s, s, True, 0, None)]
        cases += [(s, s, True, w, None) for w in _windows(s)]
    for sq, sk in PREFILL_SQ_LT_SK:
        cases += [(sq, sk, False, 0, None), (sq, sk, True, 0, None)]
        cases += [(sq, sk, True, w, None) for w in _windows(sk)]
    for s in DOC_S:
        cases += [(s, s, True, w, DOC_STARTS) for w in (0, 1, 64, 65, 129)]
    return tuple(cases)


def prefill_big_cases(s):
    """The cases of the larger grids (PREFILL_BIG)."""
    return ((s, s, False, 0, None), (s, s, True, 0, None), (s, s, True, 129, None))


@functools.lru_cache(maxsize=None)
def dv_cases():
    cases = []
    for s in DV_S:
        cases += [(s, s, False, 0, None), (s, s, True, 0, None), (s, s, True, 64, None),
                  (s, s, True, 0, DOC_STARTS), (s, s, True, 65, DOC_STARTS)]
    for sq, sk in DV_SQ_LT_SK:
        cases += [(sq, sk, False, 0, None), (sq, sk, True, 0, None), (sq, sk, True, 129, None)]
    return tuple(cases)


def doc_bounds_from_starts(starts, b, s):
    """int32 ``[2, b, s]`` (document start, one past its end) per position."""
    out = torch.zeros(2, b, s, dtype=torch.int32)
    for bi in range(b):
        st = sorted(t for t in starts[bi % len(starts)] if t < s)
        edges = torch.tensor(st + [s])
        idx = torch.bucketize(torch.arange(s), edges, right=True) - 1
        out[0, bi], out[1, bi] = edges[idx].int(), edges[idx + 1].int()
    return out


def prefill_visibility(b, sq, sk, causal, window, docs, mutant=None):
    """``[b, sq, sk]`` for one prefill case (and the doc bounds or None)."""
    bounds = doc_bounds_from_starts(docs, b, sq) if docs is not None else None
    vis = visibility(sq, sk, causal, window, None if bounds is None else bounds[0], mutant)
    return (vis if vis.dim() == 3 else vis[None].expand(b, sq, sk)), bounds


def prefill_census_inputs(b, sq, sk, nq, nkv, hd, dtype, seed=0):
    """Q = 0, K ~ N(0, 1), V the census (batch 1 reversed along the keys so
    that a wrong batch index shows): ``[b, s, n, hd]`` in ``dtype``."""
    gen = torch.Generator().manual_seed(seed + sq + 7 * sk)
    q = torch.zeros(b, sq, nq, hd, dtype=dtype)
    k = torch.randn(b, sk, nkv, hd, generator=gen).to(dtype)
    cv = census_values(sk, hd, nkv)
    v = torch.stack([cv if bi % 2 == 0 else cv.flip(0) for bi in range(b)]).to(dtype)
    return q, k, v


def dv_census_dout(b, sq, nq, hd, dtype):
    """dO[i, d] = 1 where ``i // ceil(sq / hd) == d``, scaled 2^-h per head."""
    blk = -(-sq // hd)
    base = (torch.arange(sq)[:, None] // blk == torch.arange(hd)[None, :]).float()
    hs = torch.ldexp(torch.ones(nq), -torch.arange(nq))
    return (base[None, :, None, :] * hs[None, None, :, None]).expand(b, sq, nq, hd).to(dtype).contiguous()


def prefill_expected(v, vis, nq):
    """fp64 O ``[b, sq, nq, hd]``, the visible-key count ``[b, sq]``."""
    e = census_expected(v, vis=vis.to(v.device))
    return e.repeat_interleave(nq // v.shape[2], dim=2), vis.sum(-1).to(v.device)


def dv_expected(dout, vis, nkv):
    """fp64 dV ``[b, sk, nkv, hd]`` of uniform attention: P = vis / count."""
    w = vis.double().to(dout.device)
    p = w / w.sum(-1, keepdim=True).clamp(min=1)
    b, sq, nq, hd = dout.shape
    dg = dout.double().view(b, sq, nkv, nq // nkv, hd).sum(3)  # the heads of a group see the same P
    return torch.einsum("bij,bigd->bjgd", p, dg)


# |log_fp32(n) - log_fp64(n)| over the integers n = 1 .. 4096 (every visible-key
# count used here), torch.log on the CPU: measured 4.7672e-07 (2.382e-07 up to
# n = 1024); times 4 for the hardware log / exp2 approximations
# (the kernels' largest |lse - ln n| over every case here: 1.07e-06 on an MI355X)
LSE_ATOL = 4 * 4.7672e-07
# dV: every term is non-negative, P is rounded once to 16 bits (<= 2^-9), the
# output once (<= 2^-9); the sum doubled for the fp32 accumulation order
# (the bf16 kernels' largest relative error over every case here: 6.2e-03)
DV_RTOL = 2.0 ** -7


def lse_ok(lse, count):
    """``lse [b, nq, sq]`` fp32 against ``count [b, sq]``: round(exp(lse)) is
    the count exactly, and |lse - ln count| <= LSE_ATOL.  Returns (ok, max error)."""
    cnt = count.double()[:, None, :]
    err = (lse.double() - torch.log(cnt)).abs()
    exact = torch.round(torch.exp(lse.double())) == cnt
    return bool(exact.all()) and bool((err <= LSE_ATOL).all()), float(err.max())


def dv_ok(dv, ref64):
    """Relative-only 2^-7, exactly 0 where the reference is 0."""
    d = dv.double()
    bad = torch.where(ref64 == 0, d != 0, ~((d - ref64).abs() <= DV_RTOL * ref64))
    return not bool(bad.any())


def prefill_emulate(q, k, v, vis, scale, tile=64, dout=None):
    """A tiled online-softmax forward in plain fp32 torch: key tiles of
    ``tile``, running maximum and sum, exp2, P rounded to the 16-bit type for
    P.V, one final normalisation.  Returns O in q's dtype and the fp32 lse ``[b,
    nq, sq]``; with ``dout`` also dV = P^T dO with P recomputed from the lse
    and rounded to 16 bits."""
    b, sq, nq, hd = q.shape
    sk, nkv = k.shape[1], k.shape[2]
    r = nq // nkv
    dt = q.dtype
    qf = q.float().view(b, sq, nkv, r, hd)
    kf, vf = k.float(), v.float()
    m = torch.full((b, nkv, r, sq), -math.inf)
    l = torch.zeros(b, nkv, r, sq)
    o = torch.zeros(b, nkv, r, sq, hd)
    sl2 = scale * LOG2E
    for t0 in range(0, sk, tile):
        s = torch.einsum("bigrd,bjgd->bgrij", qf, kf[:, t0:t0 + tile]) * sl2
        s = s.masked_fill(~vis[:, None, None, :, t0:t0 + tile], -math.inf)
        mn = torch.maximum(m, s.amax(-1))
        safe = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        p = torch.exp2(s - safe[..., None])
        alpha = torch.exp2(m - safe)
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + torch.einsum("bgrij,bjgd->bgrid", p.to(dt).float(), vf[:, t0:t0 + tile])
        m = mn
    out = (o / l[..., None]).permute(0, 3, 1, 2, 4).reshape(b, sq, nq, hd).to(dt)
    lse2 = m + torch.log2(l)
    lse = (lse2 * math.log(2.0)).view(b, nq, sq)
    if dout is None:
        return out, lse
    s = torch.einsum("bigrd,bjgd->bgrij", qf, kf) * sl2
    p = torch.exp2(s - lse2[..., None]).masked_fill(~vis[:, None, None], 0.0).to(dt).float()
    dv = torch.einsum("bgrij,bigrd->bjgd", p, dout.float().view(b, sq, nkv, r, hd))
    return out, lse, dv.to(dt)
