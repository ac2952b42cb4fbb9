"""Fused next-token sampling: temperature, top-k or top-p and the draw in one
HIP launch (``csrc/decode_tail.hip``, ``sample_tail_k``).

Semantics (fixed so that ``sample_ref`` reproduces the kernel token for token):

1. ``y_i = x_i / temperature`` in fp32.
2. Filter.  Top-k (``k >= 2``): keep ``i`` iff fewer than ``k`` elements are
   strictly greater than ``y_i`` (``inference/sampling.py``'s ``logits < kth``
   rule, ties included).  Top-p: keep ``i`` iff ``M(y_i) <= p`` with ``M(y)``
   the softmax mass of the elements strictly greater than ``y``: for distinct
   values exactly ``modify_logits_for_top_p_filtering`` (the crossing token
   stays).  The one deliberate difference: elements tied with the crossing one
   are all kept, where ``torch.sort`` keeps an arbitrary one of them.
3. Gumbel-max draw: ``argmax`` over the kept ``i`` of ``y_i + g_i``, ``g_i =
   -log(-log(u_i))``, ties to the smaller index.  ``u_i = ((w >> 8) + 0.5) *
   2**-24`` (never 0 or 1) with ``w`` word ``i & 3`` of ``philox(ctr = (row <<
   32) | (i >> 2), offset = offset0 + step, seed)`` (the Philox-4x32-10 of the
   dropout kernel).  The distribution is the softmax over the kept set; the
   random stream is NOT ``torch.multinomial``'s.
4. ``top_k == 1`` is the plain argmax (first maximum, no noise).
5. The token is clamped to ``vocab_size - 1``.

``sample_fused`` is the public entry (one launch on the GPU, ``sample_ref`` on
CPU tensors); ``sample_ref`` is the fp64 NumPy transcription: the CPU path and
the oracle of the GPU tests.
"""
import numpy as np
import torch

from ._ext import ext, use_native
from .dropout import _next_philox, _philox

# margins of ``sample_ref(..., return_sets=True)``: fp32 epsilon is 6e-8, the
# keys are <= ~60 in magnitude and go through a handful of operations, the
# softmax mass through a log2(V)-deep sum: ~1e-5 of key error, ~1e-6 of
# relative mass error.  The margins are ten times those.
KEY_MARGIN = 1e-4
P_MARGIN = 1e-5


def philox_words(b, V, seed, offset):
    """The kernel's noise words: uint32 ``[b, V]``."""
    nblk = (V + 3) // 4
    ctr = (np.arange(b, dtype=np.uint64)[:, None] << np.uint64(32)) | \
        np.arange(nblk, dtype=np.uint64)[None, :]
    return np.stack(_philox(ctr, offset, seed), axis=2).reshape(b, nblk * 4)[:, :V]


def philox_uniform(b, V, seed, offset, step=0):
    """``u`` of the semantics above, fp64 ``[b, V]`` (exact), strictly in (0, 1)."""
    w = philox_words(b, V, seed, offset + step)
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def _check_args(logits, top_k, top_p, temperature, vocab_size):
    if logits.ndim != 2:
        raise AssertionError("expected the logits to be of [b, v] shape")
    if not logits.dtype.is_floating_point:
        raise AssertionError("input logits should be floats")
    if top_k == 1 and top_p != 0.0:
        raise AssertionError("cannot set both greedy and top-p samplings")
    if top_k > 1:
        if top_p != 0.0:
            raise AssertionError("cannot set both top-k and top-p samplings")
        if top_k > logits.size(1) or (vocab_size and top_k >= vocab_size):
            raise AssertionError("top-k is larger than the vocabulary")
    if top_p < 0.0 or top_p > 1.0:
        raise AssertionError("top-p should be in (0, 1]")
    if not temperature > 0.0:
        raise AssertionError("temperature should be positive")


def _kept_top_p(y, p):
    """bool [b, V]: M(y_i) <= p, M = softmax mass strictly above (fp64)."""
    kept = np.empty(y.shape, dtype=bool)
    for r in range(y.shape[0]):
        vals, inv = np.unique(y[r], return_inverse=True)  # ascending
        with np.errstate(invalid="ignore"):
            e = np.where(np.isneginf(y[r]), 0.0, np.exp(y[r] - y[r].max()))
        mass = np.bincount(inv.reshape(-1), weights=e, minlength=len(vals))
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])
        kept[r] = (above <= p * mass.sum())[inv.reshape(-1)]
    return kept


def _winner(y, g, kept):
    return np.where(kept, y + g, -np.inf).argmax(1)


def sample_ref(logits, seed, offset, step=0, top_k=0, top_p=0.0, temperature=1.0,
               vocab_size=None, return_sets=False, return_kept=False):
    """fp64 reference of ``sample_tail_k``: int64 ``[b]`` (CPU).

    ``return_kept``: also the bool ``[b, V]`` kept mask.  ``return_sets``: also,
    per row, the set of tokens a correct fp32 kernel may return: the fp64
    winner, the runner-up when the two best keys are closer than
    ``KEY_MARGIN``, and the winners under ``top_p * (1 +- P_MARGIN)``."""
    _check_args(logits, top_k, top_p, temperature, vocab_size)
    x = logits.detach().float().cpu().numpy()
    b, V = x.shape

    def clamp(t):
        return np.minimum(t, vocab_size - 1) if vocab_size else t

    if top_k == 1:
        tok = clamp(x.argmax(1).astype(np.int64))
        kept = x == x.max(1, keepdims=True)
        sets = [{int(t)} for t in tok]
    else:
        y = (x / np.float32(temperature) + np.float32(0.0)).astype(np.float64)  # -0 -> +0
        u = philox_uniform(b, V, seed, offset, step)
        g = -np.log(-np.log(u))
        p = float(np.float32(top_p))
        if top_k > 1:
            kth = np.partition(y, V - top_k, axis=1)[:, V - top_k:V - top_k + 1]
            kepts = [y >= kth]
        elif top_p > 0.0:
            kepts = [_kept_top_p(y, q) for q in (p, p * (1 - P_MARGIN), p * (1 + P_MARGIN))]
        else:
            kepts = [np.ones_like(y, dtype=bool)]
        kept = kepts[0]
        tok = clamp(_winner(y, g, kept).astype(np.int64))
        sets = []
        if return_sets:
            for r in range(b):
                s = set()
                for kq in kepts:
                    key = np.where(kq[r], y[r] + g[r], -np.inf)
                    first = int(key.argmax())
                    s.add(first)
                    best = key[first]
                    key[first] = -np.inf
                    second = int(key.argmax())
                    if np.isfinite(best) and best - key[second] < KEY_MARGIN:
                        s.add(second)
                sets.append({int(clamp(np.int64(t))) for t in s})
    out = (torch.from_numpy(np.asarray(tok, dtype=np.int64)),)
    if return_kept:
        out += (kept,)
    if return_sets:
        out += (sets,)
    return out[0] if len(out) == 1 else out


def _next_seed_offset(device):
    """(seed, offset) for one draw: the CUDA generator's Philox state for GPU
    tensors (as the fused dropout), the CPU generator for CPU tensors; both
    advance, so the next call draws fresh noise under the same manual seed."""
    if device.type == "cuda":
        return _next_philox(device)
    return torch.initial_seed() & (2 ** 63 - 1), 4 * int(torch.randint(0, 2 ** 40, (1,)))


def _aligned_rows(logits):
    """The kernel reads rows with 16-byte loads: last dim contiguous, row base
    and stride 16-byte aligned (a copy into a padded buffer otherwise)."""
    es = logits.element_size()
    if logits.stride(1) == 1 and logits.data_ptr() % 16 == 0 and (logits.stride(0) * es) % 16 == 0:
        return logits
    b, V = logits.shape
    n = 16 // es
    buf = torch.empty(b, (V + n - 1) // n * n, dtype=logits.dtype, device=logits.device)
    buf[:, :V].copy_(logits)
    return buf[:, :V]


def sample_fused(logits, top_k=0, top_p=0.0, temperature=1.0, vocab_size=None, seed_offset=None):
    """``logits`` bf16 / fp16 / fp32 ``[b, v]`` -> int64 ``[b]``: the drop-in for
    ``inference.sampling.sample`` (same argument checks) with the semantics of
    this module.  ``seed_offset``: explicit ``(seed, offset)`` instead of the
    generator's."""
    _check_args(logits, top_k, top_p, temperature, vocab_size)
    seed, offset = seed_offset if seed_offset is not None else _next_seed_offset(logits.device)
    if not use_native(logits):
        return sample_ref(logits, seed, offset, 0, top_k, top_p, temperature, vocab_size)
    if logits.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        logits = logits.float()
    rows = _aligned_rows(logits)
    tokens = torch.empty(rows.size(0), dtype=torch.long, device=rows.device)
    ext().sample_rows(rows, tokens, seed, offset, top_k, top_p, temperature,
                      vocab_size if vocab_size else 0)
    return tokens
