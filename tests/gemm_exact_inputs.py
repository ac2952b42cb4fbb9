"""Inputs, expected values, checks and plain-torch emulations for the bitwise
integer-operand tests of the NT, wgrad and skinny GEMMs (``test_gemm_exact.py``
on the CPU, ``test_gemm_exact_gpu.py`` on the GPU; both take their cases from
here, so they cannot drift apart).

The method: every operand element is a small integer times one power of two
(2^-shift, the operand's quantum).  Every product and every partial sum of a
GEMM is then an integer number of quanta, and as long as the worst-case |sum|
stays below 2^24 quanta it is exact in fp32 whatever the order of accumulation:
however K is cut into steps and splits, however the tokens are cut into
subtiles, whichever kernel variant runs.  The fp32 result is *the* integer, a
16-bit output is that integer rounded once to nearest even, and both follow
from an fp64 matmul (exact too: the integers are far below 2^53).  So a GEMM
output is compared with ``torch.equal``: one wrong element fails.

Nothing here is kernel code: pure torch, on whatever device the caller asks.
"""
import functools
import math

import torch

from attention_edge_inputs import MIN_EXP, ulp

BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = (BF16, FP16)
DTYPE_IDS = ("bf16", "fp16")
TWO24 = 2 ** 24
FP16_MAX = 65504
TILE = 256      # output tile edge of every 256 x 256 kernel
SUBTILE = 32    # token subtile of the wgrad kernels, row strip of a dropped K-step
SENTINEL = 7.0  # "must not be touched"; NaN is "must be written"

# ---------------------------------------------------------------- generators, bounds, references


def int_operand(shape, lo, hi, dtype, shift=0, seed=0, device="cpu"):
    """Random integers in ``[lo, hi]`` times ``2^-shift`` in ``dtype`` (drawn on
    the CPU from ``seed``, so every device and dtype sees the same values)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen).double() * 2.0 ** -shift
    t = v.to(dtype)
    assert torch.equal(t.double(), v), "operand values must be exact in the operand dtype"
    return t.to(device)


def bound(k, lo, hi, lo2=None, hi2=None, extra=0):
    """Worst-case |sum|, in quanta, of ``k`` products of one integer of ``[lo,
    hi]`` and one of ``[lo2, hi2]`` (default: the same range) plus ``extra``."""
    lo2, hi2 = (lo, hi) if lo2 is None else (lo2, hi2)
    return k * max(abs(lo), abs(hi)) * max(abs(lo2), abs(hi2)) + extra


def check_bound(b, shift=0, out_dtype=None):
    """The exactness conditions of one case: < 2^24 quanta (fp32 holds every
    partial sum exactly), and no fp16 output beyond the format's largest value."""
    assert b < TWO24, f"worst-case |sum| {b} quanta is not exact in fp32"
    if out_dtype == FP16:
        assert b <= FP16_MAX * 2 ** shift, f"worst-case |sum| {b} x 2^-{shift} overflows fp16"
    return True


def abs_bound(a, b):
    """Data-driven form of ``bound`` for operands that are not drawn from a
    range (the layer wiring feeds one GEMM's rounded output to the next): the
    largest sum of |a_ik| |b_jk| over k of ``a [M, K] b [N, K]^T``, fp64."""
    return float((a.double().abs() @ b.double().abs().t()).max())


def check_abs_bound(a, b, out_dtype=None):
    """fp32 exactness of ``a b^T`` from the data: integer operands, the sum of
    |terms| below 2^24; fp16 outputs in range."""
    assert bool((a.double() == a.double().round()).all()) and bool((b.double() == b.double().round()).all())
    s = abs_bound(a, b)
    assert s < TWO24, f"sum of |terms| {s} is not exact in fp32"
    if out_dtype == FP16:
        assert s <= FP16_MAX, f"sum of |terms| {s} overflows fp16"
    return True


def ref_nt(a, b):
    """fp64 ``a [M, K] b [N, K]^T`` (exact for these operands)."""
    return a.double() @ b.double().t()


def ref_wgrad(dy, x, g0=None):
    """fp64 ``g0 + dy [M, N]^T x [M, K]`` (``g0`` None: the plain product)."""
    r = dy.double().t() @ x.double()
    return r if g0 is None else r + g0.double()


def expect16(ref64, dtype):
    """The one rounding (to nearest even) of an exact fp64 result to ``dtype``.
    (Every reference here is exact in fp32 as well, so the conversion has no
    double rounding whichever way torch goes.)"""
    return ref64.to(dtype)


def exact_ok(out, expected):
    """The bitwise check of both files: same dtype, same shape, every element
    equal (a NaN sentinel left behind fails: NaN != NaN)."""
    return out.dtype == expected.dtype and out.shape == expected.shape and torch.equal(out, expected)


def first_mismatch(out, expected):
    """'(row, col): got, expected' of the first differing element, and the count."""
    bad = ~(out.double() == expected.double())
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no mismatch"
    i = tuple(int(v) for v in idx[0])
    return f"{int(bad.sum())} elements differ, first at {i}: got {float(out[i])}, expected {float(expected[i])}"


def truncate16(x32, dtype):
    """fp32 -> ``dtype`` by truncation (round towards zero): the wrong rounding
    mode the census cases must flag.  Normal-range values only."""
    bits = x32.contiguous().view(torch.int32)
    drop = 16 if dtype == BF16 else 13
    return (bits & ~((1 << drop) - 1)).view(torch.float32).to(dtype)


def inexact_share(ref64, dtype):
    """Share of elements not representable in ``dtype`` and share of exact
    ties (halfway between two neighbours) of an exact fp64 result."""
    r = expect16(ref64, dtype).double()
    inexact = r != ref64
    t = truncate16(ref64.float(), dtype).double()
    # a tie: the distance to the truncated neighbour is half the spacing there
    spacing = ulp(torch.where(t == 0, torch.ones_like(t), t.abs()), dtype)
    tie = inexact & ((ref64 - t).abs() * 2 == spacing)
    n = ref64.numel()
    return float(inexact.sum()) / n, float(tie.sum()) / n


# ---------------------------------------------------------------- row / token maps (csrc/kernels.h)


def row_map_index(m, rmap, device="cpu"):
    """RowMap: logical row q lives at (q / rows) * stride + offset + q % rows."""
    q = torch.arange(m, device=device)
    if not rmap:
        return q
    rows, stride, offset = rmap
    return (q // rows) * stride + offset + q % rows


def tok_map_index(m, xmap, device="cpu"):
    """TokMap: token q of dY is X row ((q / rows) % n1) * s1 + ((q / rows) / n1)
    * s2 + q % rows."""
    q = torch.arange(m, device=device)
    if not xmap:
        return q
    rows, n1, s1, s2 = xmap
    g = q // rows
    return (g % n1) * s1 + (g // n1) * s2 + q % rows


# ---------------------------------------------------------------- the host plans, transcribed


def _cdiv(a, b):
    return -(-a // b)


def nt_ksplit(M, N, K, ncu=256):
    """``nt_ksplit`` of csrc/gemm_nt.hip: the K split of a few-tile plain product."""
    tiles = _cdiv(M, TILE) * _cdiv(N, TILE)
    if tiles * 2 > ncu or K % 64 != 0:
        return 1
    steps = K // 64
    best = 1
    for sp in range(2, 9):
        if tiles * sp <= ncu and steps % sp == 0 and steps // sp >= 8:
            best = sp
    return best


def best_split(t, M, ncu=256):
    """``best_split`` of csrc/gemm_wgrad.hip (same expressions, same order)."""
    if t <= 0:
        return 1
    tile_us = 2.0 * TILE * TILE * float(M) / (1.3e15 / ncu) * 1e6
    whole = ((t + ncu - 1) // ncu) * (tile_us + 5.0)
    best, best_c = 1, whole * 0.95
    for sp in range(2, 17):
        if M // sp < 2048 or t * sp > 4 * ncu:
            break
        if M % 64 == 0 and M % (64 * sp) != 0:
            continue
        rounds = (t * sp + ncu - 1) // ncu
        c = rounds * (tile_us / sp + 5.0) + float(t) * sp * TILE * TILE * 4.0 * 2.0 / 5e12 * 1e6 + 3.0
        if c < best_c:
            best_c, best = c, sp
    return best


def wgrad_plan(M, N, K, ncu=256):
    """``wgrad_plan``: [main_tiles, tail_lin0, tail_tiles, nsplit]."""
    tiles = _cdiv(N, TILE) * _cdiv(K, TILE)
    tail = tiles if tiles < ncu else tiles % ncu
    sp = best_split(tail, M, ncu)
    if sp > 1:
        return [tiles - tail, tiles - tail, tail, sp]
    return [tiles, tiles, 0, 1]


# ---------------------------------------------------------------- case tables

NT_LO, NT_HI = -3, 3


def nt_range(dtype, K):
    """Operands in [-3, 3]; fp16 at K >= 4096 in [-2, 2] (outputs within fp16)."""
    return (-2, 2) if (dtype == FP16 and K >= 4096) else (NT_LO, NT_HI)


# (M, N, K, variants); variant 0: the default
NT_PLAIN = (
    (256, 256, 32, (0,)),           # K % 64 != 0: the 8-wave kernel
    (256, 256, 64, (0,)),           # one K-step: the one-shot kernel
    (256, 256, 128, (0, 5, 6, 8)),  # the persistent kernel's minimum
    (300, 264, 192, (0, 5, 6, 8)),  # ragged M and N, odd step count
    (520, 520, 96, (0,)),           # ragged, 8-wave
    (4352, 4096, 128, (6, 8)),      # 272 tiles: more than one per workgroup, partial last round
    (256, 256, 8192, (0,)),         # long K: the rounding and tie census
)
NT_CENSUS = (256, 256, 8192)
# (M, N, K, the split the plan picks)
NT_SPLITK = ((256, 256, 1024, 2), (256, 256, 4096, 8), (300, 264, 1024, 2), (512, 256, 1536, 3),
             (256, 256, 960, 1))  # 15 steps: too few to split
# (tp, c, R, N, K): groups of whole tiles (persistent), the same with a K split, ragged groups (one-shot)
NT_ROW_MAPS = ((2, 2, 256, 256, 128), (2, 2, 256, 256, 1024), (4, 2, 200, 264, 96))
# A = wide[:, col0:col0 + K] of [M, lda]; C = wide[:, c0:c0 + N] of [M, ldc]
NT_STRIDED = dict(M=512, N=384, K=512, lda=640, a0=64, ldc=400, c0=8)

KINDS = {"swiglu": 0, "geglu": 1, "reglu": 2, "liglu": 3}
EXACT_KINDS = ("reglu", "liglu")
GLU_VARIANTS = (5, 6)
GLU_ACT = (-2, 2)  # activations (A) of the GLU products
# (M, F, K, weight |max|, shift): pre ~ N(0, sigma), sigma = sqrt(K 2 var_w) 2^-shift = 1.41, 0.87, 0.91
# (the long-K case draws its weights from [-4, 4]: [-3, 3] 2^-8 leaves 7.9 % of pre inexact in
# bf16, under the 10 % its rounding mutants need; [-4, 4] gives 14 %)
GLU_SHAPES = ((256, 128, 64, 3, 4), (300, 200, 96, 3, 5), (512, 264, 4096, 4, 8))
GLU_INEXACT = (512, 264, 4096, 4, 8)  # the case whose pre is not exact in 16 bits
GLU_CMAP = dict(tp=2, c=2, R=256, F=128, K=128, wmax=3, shift=4)
DGLU_PRE = (-96, 96, 4)  # the saved pre of dGLU: multiples of 2^-4 in [-6, 6]
GLU_FACTOR = 2.0 ** -20  # the fp32 activation term of the tolerance (see glu_tol)

WG_LO, WG_HI = -4, 4
WG_G0 = 2 ** 20  # g0 in [-2^20, 2^20]: 16 M + 2^20 < 2^24 up to M = 16384 and beyond
WGRAD_VARIANTS = (4, 8)
WGRAD_SHAPES = ((32, 256, 256), (96, 512, 256),  # M < 128 or M % 64 != 0: the 8-wave kernel
                (128, 256, 256),                 # the 4-wave minimum
                (2048, 264, 520))                # ragged
WGRAD_PLANS = (((4096, 256, 256), [0, 0, 1, 2]), ((6144, 256, 256), [0, 0, 1, 3]),
               ((8192, 256, 512), [0, 0, 2, 4]),
               ((4096, 264, 520), [0, 0, 6, 2]),     # ragged tiles, split
               ((4128, 256, 256), [0, 0, 1, 2]),     # M % 64 != 0: the split on the 8-wave kernel
               ((4096, 4352, 4096), [256, 256, 16, 2]))  # whole-tile round + split tail in one call
# (world, c, R, N, K); the second has M = 4096: the split path with a map
WGRAD_TOKMAPS = ((4, 4, 64, 512, 768), (2, 2, 1024, 256, 256))


def wgrad_tokmaps(world, c, R):
    """Both orders ``test_wgrad_gemm_token_map`` uses."""
    return ([R, c, world * R, R], [R, world, c * R, R])


SK_LO, SK_HI = -3, 3
SK_RES = 64  # integer residual in [-64, 64]
SKINNY_M = (1, 5, 16)
SKINNY_NK = ((512, 384), (4096, 4096))  # K % 256 != 0: row-major only; K = 4096: packed too

# layer wiring: (M, out, in) of the linear (32 wgrad tiles: the hand-written
# wgrad takes it); (M, H, F) of the GLU MLP (64 and 32 wgrad tiles)
WIRE_LINEAR = (256, 1024, 2048)
WIRE_MLP = (256, 1024, 2048)
WIRE_MICROBATCHES = 3  # one fresh store, two accumulating


def nt_case(M, N, K, dtype, device="cpu", seed=0):
    lo, hi = nt_range(dtype, K)
    check_bound(bound(K, lo, hi), 0, dtype)
    a = int_operand((M, K), lo, hi, dtype, 0, 1000 + seed + M + 3 * K, device)
    b = int_operand((N, K), lo, hi, dtype, 0, 2000 + seed + N + 5 * K, device)
    return a, b


def glu_case(M, F, K, wmax, shift, dtype, device="cpu"):
    """Forward operands: x [M, K] integers in [-2, 2], w1 [2F, K] in [-wmax,
    wmax] 2^-shift."""
    check_bound(bound(K, *GLU_ACT, -wmax, wmax), shift, dtype)
    x = int_operand((M, K), *GLU_ACT, dtype, 0, 3000 + M + K, device)
    w1 = int_operand((2 * F, K), -wmax, wmax, dtype, shift, 4000 + F + K, device)
    return x, w1


def dglu_case(M, F, K, wmax, shift, dtype, device="cpu"):
    """Backward operands: dy [M, K], w2t [F, K] as the forward's, and the saved
    pre [M, 2F] of multiples of 2^-4 in [-6, 6]."""
    check_bound(bound(K, *GLU_ACT, -wmax, wmax), shift, dtype)
    dy = int_operand((M, K), *GLU_ACT, dtype, 0, 5000 + M + K, device)
    w2t = int_operand((F, K), -wmax, wmax, dtype, shift, 6000 + F + K, device)
    pre = int_operand((M, 2 * F), DGLU_PRE[0], DGLU_PRE[1], dtype, DGLU_PRE[2], 7000 + M + F, device)
    return dy, w2t, pre


def wgrad_case(M, N, K, dtype, device="cpu", xrows=None):
    check_bound(bound(M, WG_LO, WG_HI, extra=WG_G0))
    dy = int_operand((M, N), WG_LO, WG_HI, dtype, 0, 8000 + M + N, device)
    x = int_operand((xrows or M, K), WG_LO, WG_HI, dtype, 0, 9000 + M + K, device)
    g0 = int_operand((N, K), -WG_G0, WG_G0, torch.float32, 0, 10000 + N + K, device)
    return dy, x, g0


def skinny_case(M, N, K, dtype, device="cpu"):
    check_bound(bound(K, SK_LO, SK_HI, extra=SK_RES), 0, dtype)
    x = int_operand((M, K), SK_LO, SK_HI, dtype, 0, 11000 + M + K, device)
    w = int_operand((N, K), SK_LO, SK_HI, dtype, 0, 12000 + N + K, device)
    res = int_operand((M, N), -SK_RES, SK_RES, dtype, 0, 13000 + M + N, device)
    return x, w, res


# ---------------------------------------------------------------- GLU: fp64 expectations, tolerance


def act64(kind, x):
    if kind == "swiglu":
        return x * torch.sigmoid(x)
    if kind == "geglu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == "reglu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x


def dact64(kind, x):
    if kind == "swiglu":
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if kind == "geglu":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if kind == "reglu":
        return (x > 0).to(x.dtype)
    return torch.ones_like(x)


def glu_expected(pre16, kind):
    """From the *rounded* pre [M, 2F]: (E, s, x2) of y = x1 act(x2), fp64."""
    F = pre16.shape[1] // 2
    x1, x2 = pre16[:, :F].double(), pre16[:, F:].double()
    return x1 * act64(kind, x2), x1.abs(), x2


def dglu_expected(g16, pre16, kind):
    """From g = dAct rounded to T and the saved pre: (E, s, x2) of d(pre) =
    [g act(x2), g x1 act'(x2)], the halves concatenated, fp64."""
    F = pre16.shape[1] // 2
    x1, x2, g = pre16[:, :F].double(), pre16[:, F:].double(), g16.double()
    e = torch.cat([g * act64(kind, x2), g * x1 * dact64(kind, x2)], dim=1)
    s = torch.cat([g.abs(), (g * x1).abs()], dim=1)
    return e, s, torch.cat([x2, x2], dim=1)


def _ulp_rounded(e64, dtype):
    """ulp_T at round_T(E); at 0 the spacing of the smallest magnitudes of T."""
    er = e64.to(dtype).double().abs()
    return ulp(er.clamp(min=2.0 ** MIN_EXP[dtype]), dtype)


def glu_tol(e64, s, x2, dtype, factor=GLU_FACTOR):
    """ulp_T(round_T(E)) + factor s max(1, |x2|): one wrong final rounding,
    plus 16 fp32 ulps (factor 2^-20) of absolute error of the fp32 activation
    or derivative, of magnitude <= ~1.2 max(1, |x|), where 1 + erf or 1 + x (1 -
    sigma) cancels."""
    return _ulp_rounded(e64, dtype) + factor * s * x2.abs().clamp(min=1.0)


def glu_ok(o, e64, s, x2, kind, factor=GLU_FACTOR):
    """ReGLU / LiGLU: bitwise.  SwiGLU / GeGLU: every element within glu_tol of
    E (NaN fails, nothing excluded).  Returns (ok, margin): the largest (|o - E|
    - ulp) / (s max(1, |x2|)), i.e. the smallest ``factor`` that would pass."""
    if kind in EXACT_KINDS:
        return exact_ok(o, expect16(e64, o.dtype)), 0.0
    err = (o.double() - e64).abs()
    ok = bool((err <= glu_tol(e64, s, x2, o.dtype, factor)).all())
    den = s * x2.abs().clamp(min=1.0)
    over = (err - _ulp_rounded(e64, o.dtype)).clamp(min=0)
    margin = torch.where(den > 0, over / den.clamp(min=1e-300), torch.where(over > 0, math.inf, 0.0))
    return ok, float(margin.nan_to_num(nan=math.inf).max())


# fp32 torch emulation of csrc/act_math.h
_LOG2E32 = torch.tensor(-1.4426950408889634, dtype=torch.float32)
_INV_SQRT2 = torch.tensor(0.70710678118654752, dtype=torch.float32)
_INV_SQRT2PI = torch.tensor(0.39894228040143268, dtype=torch.float32)


def _sigmoid32(x):
    return 1.0 / (1.0 + torch.exp2(x * _LOG2E32))


def act32(kind, x):
    if kind == "swiglu":
        return x * _sigmoid32(x)
    if kind == "geglu":
        return 0.5 * x * (1.0 + torch.erf(x * _INV_SQRT2))
    return act64(kind, x)


def act_dact32(kind, x):
    """``act_dact``: SwiGLU shares one sigmoid and forms d = fma(a, 1 - sg, sg)."""
    if kind == "swiglu":
        sg = _sigmoid32(x)
        a = x * sg
        d = (a.double() * (1.0 - sg).double() + sg.double()).float()  # the fused multiply-add
        return a, d
    if kind == "geglu":
        d = 0.5 * (1.0 + torch.erf(x * _INV_SQRT2)) + x * _INV_SQRT2PI * torch.exp(-0.5 * x * x)
        return act32(kind, x), d
    return act64(kind, x), dact64(kind, x)


# ---------------------------------------------------------------- emulations of the decompositions

def _mid_tile(M, N):
    """Rows of one 32-row strip and columns of one 256-wide tile (the last
    tile, the strip in the middle of its valid rows)."""
    tm, tn = (M - 1) // TILE, (N - 1) // TILE
    rows = min(TILE, M - tm * TILE)
    r0 = tm * TILE + (rows // 2) // SUBTILE * SUBTILE
    return slice(r0, min(r0 + SUBTILE, M)), slice(tn * TILE, min(tn * TILE + TILE, N))


def nt_acc32(a, b, ksplit=1, a_map=None, m=None, mutant=None):
    """The fp32 accumulator of C = A B^T as the kernels form it: K in steps of
    64 (32 where K % 64 != 0) accumulated in fp32 within each of ``ksplit``
    contiguous ranges, the ranges' partials then summed in fp32 in order; A's
    rows through ``a_map``.  ``mutant``: one K-step dropped in one 32-row strip
    of one tile, one split counted twice or omitted, the row-map groups read
    from the neighbouring group."""
    m = a.shape[0] if m is None else m
    if a_map and mutant == "neighbour_group":
        rows, stride, offset = a_map
        a_map = (rows, stride, (offset + rows) % stride)
    af = a[row_map_index(m, a_map)].float()
    bf = b.float()
    K = af.shape[1]
    step = 64 if K % 64 == 0 else 32
    steps = K // step
    assert steps % ksplit == 0
    per = steps // ksplit
    rs, cs = _mid_tile(m, bf.shape[0])
    parts = []
    for sp in range(ksplit):
        acc = torch.zeros(m, bf.shape[0])
        for t in range(sp * per, (sp + 1) * per):
            k = slice(t * step, (t + 1) * step)
            acc += af[:, k] @ bf[:, k].t()
            if mutant == "kstep_dropped" and t == steps // 2:
                acc[rs, cs] -= af[rs, k] @ bf[cs, k].t()  # exact: as if never added
        parts.append(acc)
    if mutant == "split_twice":
        parts.append(parts[ksplit // 2])
    if mutant == "split_omitted":
        del parts[ksplit // 2]
    out = parts[0] if parts else torch.zeros(m, bf.shape[0])
    for p in parts[1:]:
        out = out + p
    return out


def emulate_nt(a, b, ksplit=1, a_map=None, m=None, mutant=None):
    acc = nt_acc32(a, b, ksplit, a_map, m, mutant)
    return truncate16(acc, a.dtype) if mutant == "truncate" else acc.to(a.dtype)


def emulate_glu(x, w1, kind, mutant=None):
    """fc1 + GLU as the epilogues state it: the accumulator rounded to T once
    (pre), y = x1 act(x2) in fp32 on the rounded values, rounded once."""
    acc = nt_acc32(x, w1, mutant=mutant if mutant == "kstep_dropped" else None)
    pre = truncate16(acc, x.dtype) if mutant == "truncate" else acc.to(x.dtype)
    F = pre.shape[1] // 2
    src = acc if mutant == "y_from_unrounded" else pre.float()
    x1, x2 = src[:, :F], src[:, F:]
    if mutant == "x1_x2_swapped":
        x1, x2 = x2, x1
    return pre, (x1 * act32(kind, x2)).to(x.dtype)


def emulate_dglu(dy, w2t, pre, kind):
    """fc2 dgrad + GLU backward: dAct rounded to T first, then both halves in fp32."""
    g = nt_acc32(dy, w2t).to(dy.dtype).float()
    F = pre.shape[1] // 2
    x1, x2 = pre[:, :F].float(), pre[:, F:].float()
    av, dv = act_dact32(kind, x2)
    return torch.cat([(g * av).to(dy.dtype), (g * x1 * dv).to(dy.dtype)], dim=1)


def emulate_wgrad(dy, x, g, accumulate, nsplit=1, x_map=None, mutant=None):
    """G (+)= dY^T X as the kernels form it: the tokens in ``nsplit`` contiguous
    ranges (rounded up to whole 32-token subtiles), each accumulated in fp32 one
    32-token subtile at a time, the ranges' partials summed in fp32 in order on
    top of G (accumulate) or of zero (store); X's rows through ``x_map``.
    ``g`` is the buffer's content before the call (a NaN fill for a store)."""
    M = dy.shape[0]
    dyf, xf = dy.float(), x[tok_map_index(M, x_map)].float()
    msplit = _cdiv(_cdiv(M, nsplit), SUBTILE) * SUBTILE
    N, K = dyf.shape[1], xf.shape[1]
    ns, ks = _mid_tile(N, K)
    ns = slice(ns.start // TILE * TILE, min(ns.start // TILE * TILE + TILE, N))  # the whole tile
    parts = []
    for sp in range(nsplit):
        acc = torch.zeros(N, K)
        t_hi = min((sp + 1) * msplit, M)
        for t0 in range(sp * msplit, t_hi, SUBTILE):
            t = slice(t0, min(t0 + SUBTILE, t_hi))
            acc += dyf[t].t() @ xf[t]
            if mutant == "subtile_dropped" and t0 == (M // 2) // SUBTILE * SUBTILE:
                acc[ns, ks] -= dyf[t, ns].t() @ xf[t, ks]
        parts.append(acc)
    if mutant == "split_twice":
        parts.append(parts[nsplit // 2])
    if mutant == "split_omitted":
        del parts[nsplit // 2]
    if mutant == "acc_as_store":
        accumulate = False
    if mutant == "store_as_acc":
        accumulate = True
    out = g.float().clone() if accumulate else torch.zeros(N, K)
    for p in parts:
        out = out + p
    return out


@functools.lru_cache(maxsize=None)
def census_shares(dtype):
    """(inexact share, tie share) of the long-K census case in ``dtype``."""
    a, b = nt_case(*NT_CENSUS, dtype)
    return inexact_share(ref_nt(a, b), dtype)


# ---------------------------------------------------------------- layer wiring: the chained expectations


def _checked_nt(a, b, dtype):
    """expect16(a b^T) after the data-driven exactness check of that product."""
    check_abs_bound(a, b)
    r = ref_nt(a, b)
    assert float(r.abs().max()) <= (FP16_MAX if dtype == FP16 else 3e38)
    return expect16(r, dtype)


def sparse_operand(shape, dtype, seed, keep=4, device="cpu"):
    """Integers in [-1, 1], all but one in ``keep`` zeroed: the chained GEMMs
    of the MLP stay far below 2^24 (and fp16's range) with such weights."""
    v = int_operand(shape, -1, 1, dtype, 0, seed, device)
    return v * (int_operand(shape, 0, keep - 1, dtype, 0, seed + 1, device) == 0).to(dtype)


class _MainGrad:
    """fp64 sum of the micro-batches' dY^T X with the running sum of |terms|."""

    def __init__(self):
        self.sum, self.abs = None, None

    def add(self, dy, x):
        r, a = ref_wgrad(dy, x), ref_wgrad(dy.abs(), x.abs())
        self.sum = r if self.sum is None else self.sum + r
        self.abs = a if self.abs is None else self.abs + a
        assert float(self.abs.max()) < TWO24
        return 1


@functools.lru_cache(maxsize=4)
def wire_linear_expected(dtype, device="cpu"):
    """The linear layer's case: weight [out, in] in [-1, 1], per micro-batch x
    and dy in [-2, 2]; expected y, dX (each one rounding of an exact sum) and
    the fp32 main_grad after all micro-batches."""
    M, N, K = WIRE_LINEAR
    w = int_operand((N, K), -1, 1, dtype, 0, 20000, device)
    mg, mbs, checked = _MainGrad(), [], 0
    for i in range(WIRE_MICROBATCHES):
        x = int_operand((M, K), -2, 2, dtype, 0, 20001 + 2 * i, device)
        dy = int_operand((M, N), -2, 2, dtype, 0, 20002 + 2 * i, device)
        y = _checked_nt(x, w, dtype)
        dx = _checked_nt(dy, w.t(), dtype)
        checked += 2 + mg.add(dy, x)
        mbs.append(dict(x=x, dy=dy, y=y, dx=dx))
    return dict(w=w, mbs=mbs, main_grad=mg.sum.float(), checked=checked)


@functools.lru_cache(maxsize=4)
def wire_mlp_expected(kind, dtype, device="cpu"):
    """The GLU MLP's case (ReGLU / LiGLU: every stage is exact products and
    sums rounded once): sparse weights in [-1, 1], per micro-batch x and dOut
    in [-1, 1]; expected out, dX and both main_grads."""
    assert kind in EXACT_KINDS
    M, H, F = WIRE_MLP
    w1 = sparse_operand((2 * F, H), dtype, 21000, device=device)
    w2 = sparse_operand((H, F), dtype, 21010, device=device)
    mg1, mg2, mbs, checked = _MainGrad(), _MainGrad(), [], 0
    for i in range(WIRE_MICROBATCHES):
        x = int_operand((M, H), -1, 1, dtype, 0, 21020 + 2 * i, device)
        dout = int_operand((M, H), -1, 1, dtype, 0, 21021 + 2 * i, device)
        pre = _checked_nt(x, w1, dtype)
        e, _, _ = glu_expected(pre, kind)
        y = expect16(e, dtype)
        out = _checked_nt(y, w2, dtype)
        g = _checked_nt(dout, w2.t(), dtype)
        de, _, _ = dglu_expected(g, pre, kind)
        assert float(e.abs().max()) < TWO24 and float(de.abs().max()) < TWO24  # exact fp32 products
        dpre = expect16(de, dtype)
        dx = _checked_nt(dpre, w1.t(), dtype)
        checked += 4 + mg2.add(dout, y) + mg1.add(dpre, x)
        mbs.append(dict(x=x, dout=dout, out=out, dx=dx))
    return dict(w1=w1, w2=w2, mbs=mbs, main_grad1=mg1.sum.float(), main_grad2=mg2.sum.float(),
                checked=checked)
