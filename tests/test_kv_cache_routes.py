"""``inference/kv_cache.py`` on its own (CPU, no model): ``LayerKV.write`` against
an oracle built by plain indexing (and ``fp8_kv.quantize`` for the e4m3 cache)
in every cell of (16-bit | e4m3) x (column per row | paged pool) x (host slot |
one device slot | one device slot per row | prefill scatter) that exists, and
the step kind or the refusal of every (layout, step) pair."""
import pytest
import torch

from epfl_megatron_amd.inference import kv_cache
from epfl_megatron_amd.inference.forward_step import InferenceParams
from epfl_megatron_amd.inference.kv_cache import (CONTINUED_PREFILL, DEVICE_DECODE, EAGER_DECODE,
                                                  RESTART_PREFILL, LayerKV)
from epfl_megatron_amd.inference.paged import KV_PAGE
from epfl_megatron_amd.ops import fp8_kv

NKV, HD, B, CAP, PAGES = 2, 8, 3, 2 * KV_PAGE, 6
CPU = torch.device("cpu")
TABLE_ROW = (4, 2)  # the row's two pages: not adjacent in the pool, out of order


@pytest.fixture
def fp8_switch():
    def switch(on, calibrate=False):
        kv_cache.set_fp8_kv_cache(on, calibrate=calibrate)
    yield switch
    kv_cache.set_fp8_kv_cache(False, calibrate=False)


def _params(paged, s0=0, b0=0, slots=None, cont=False):
    ip = InferenceParams(B + 1, CAP, kv_pages=PAGES if paged else None, table_device=CPU)
    ip.sequence_len_offset, ip.batch_size_offset, ip.continue_prefill = s0, b0, cont
    if paged:
        ip.page_table[b0] = torch.tensor(TABLE_ROW, dtype=torch.int32)
    if slots is not None:
        ip.device_offset = torch.tensor(slots, dtype=torch.long)
        ip.device_kv_len = torch.zeros(len(slots), dtype=torch.int32)
    return ip


def _layer(ip, sq, b, fused=False, device=CPU, hd=HD):
    return LayerKV(ip, 1, NKV, hd, torch.float32, device, sq, b, fused)


def _written(ip, sq, b):
    """(K, V) after ``write`` of random rows and the oracle's (K, V): the cache
    as it was (a sentinel in every element) with ``stored(x)[t, m]`` put at the
    cache index ``where(t, m)`` by the caller."""
    kv = _layer(ip, sq, b)
    g = torch.Generator().manual_seed(5)
    k, v = (torch.randn(sq, b, NKV, HD, generator=g) * 3 for _ in range(2))
    if kv.fp8:
        kv.scales.copy_(torch.tensor([[0.5, 2.0], [4.0, 1.0]]))
        stored = [fp8_kv.quantize(k, kv.scales[0]), fp8_kv.quantize(v, kv.scales[1])]
    else:
        stored = [k, v]
    for mem in ip.key_value_memory_dict[1]:
        mem.fill_(7)
    oracle = [mem.clone() for mem in ip.key_value_memory_dict[1]]
    kv.write(k, v)
    return kv, ip.key_value_memory_dict[1], oracle, stored


def _check(ip, sq, b, where):
    kv, mem, oracle, stored = _written(ip, sq, b)
    for o, x in zip(oracle, stored):
        for t in range(sq):
            for m in range(b):
                o[where(t, m)] = x[t, m]
    assert mem[0].dtype == (torch.uint8 if kv.fp8 else torch.float32)
    assert torch.equal(mem[0], oracle[0]) and torch.equal(mem[1], oracle[1])
    assert not torch.equal(mem[0], torch.full_like(mem[0], 7))
    return kv


def _pool_row(pos):
    return TABLE_ROW[pos // KV_PAGE] * KV_PAGE + pos % KV_PAGE


# ------------------------------------------------------------------ write

@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
@pytest.mark.parametrize("s0,sq,b0,b,cont", (
    (0, 4, 0, B, False), (0, 4, 1, B, False), (5, 1, 0, B, False), (3, 4, 1, B, False),
    (3, 4, 0, B, True), (5, 1, 0, B + 1, False)),
    ids=("restart", "restart-b0", "eager-step", "continued", "continued-flag", "whole-batch-step"))
def test_write_host_slot_columns(fp8_switch, fp8, s0, sq, b0, b, cont):
    fp8_switch(fp8)
    ip = _params(False, s0=s0, b0=b0, cont=cont)
    kv = _check(ip, sq, b, lambda t, m: (s0 + t, b0 + m))
    assert ip.key_value_memory_dict[1][0].shape == (CAP, B + 1, NKV, HD)
    assert (kv.slot_t, kv.slot) == (None, s0)


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
def test_write_one_device_slot_columns(fp8_switch, fp8):
    fp8_switch(fp8)
    ip = _params(False, s0=2, b0=1, slots=[9])  # the device slot counts, not the host offset
    kv = _check(ip, 1, B, lambda t, m: (9, 1 + m))
    assert kv.slot_t is ip.device_offset and kv.slot == 0


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
@pytest.mark.parametrize("slots", ([11, 3, 300], [11, 3, 300, 0]), ids=("rows", "whole-batch"))
def test_write_per_row_slots_columns(fp8_switch, fp8, slots):
    fp8_switch(fp8)  # the slots: distinct, out of order
    kv = _check(_params(False, slots=slots), 1, len(slots), lambda t, m: (slots[m], m))
    assert kv.kc.shape == (CAP, len(slots), NKV, HD)


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
def test_write_per_row_slots_paged(fp8_switch, fp8):
    fp8_switch(fp8)
    slots = [4 * KV_PAGE + 7, 2 * KV_PAGE + KV_PAGE - 1, KV_PAGE]  # pool rows
    ip = _params(True, slots=slots)
    _check(ip, 1, B, lambda t, m: (slots[m], 0))
    assert ip.key_value_memory_dict[1][0].shape == (PAGES * KV_PAGE, 1, NKV, HD)


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
@pytest.mark.parametrize("s0,cont", ((0, False), (0, True), (KV_PAGE - 2, True)),
                         ids=("restart", "restart-flag", "continued-over-page-edge"))
def test_write_prefill_scatter_paged(fp8_switch, fp8, s0, cont):
    fp8_switch(fp8)
    ip = _params(True, s0=s0, cont=cont)
    _check(ip, 4, 1, lambda t, m: (_pool_row(s0 + t), 0))
    if s0:
        assert _pool_row(s0 + 1) + 1 != _pool_row(s0 + 2)  # the rows cross to the other page
    # the memo serves the prefill's other layers and no other call
    key, idx = ip._prefill_slots
    assert idx.tolist() == [_pool_row(s0 + t) for t in range(4)]
    LayerKV(ip, 2, NKV, HD, torch.float32, CPU, 4, 1).write(torch.zeros(4, 1, NKV, HD),
                                                           torch.zeros(4, 1, NKV, HD))
    assert ip._prefill_slots[1] is idx
    ip.page_table[0, 0] = 5
    _layer(ip, 4, 1).write(torch.zeros(4, 1, NKV, HD), torch.zeros(4, 1, NKV, HD))
    assert ip._prefill_slots[1] is not idx


def test_calibration_on_the_restart_prefill_only(fp8_switch):
    fp8_switch(True, calibrate=True)
    ip = _params(False)
    kv = _layer(ip, 4, B)
    g = torch.Generator().manual_seed(6)
    k, v = (torch.randn(4, B, NKV, HD, generator=g) * 40 for _ in range(2))
    want = fp8_kv.new_scales(NKV, CPU)
    fp8_kv.calibrate_(want, k, v)
    assert not torch.equal(want, torch.ones_like(want))
    kv.write(k, v)
    assert torch.equal(ip.kv_scale_dict[1], want)
    assert torch.equal(ip.key_value_memory_dict[1][0][:4, :B], fp8_kv.quantize(k, want[0]))
    assert torch.equal(ip.key_value_memory_dict[1][1][:4, :B], fp8_kv.quantize(v, want[1]))
    for s0, b0, sq in ((4, 0, 4), (4, 0, 1), (0, 1, 4)):  # continued, a step, a later micro-batch
        ip.sequence_len_offset, ip.batch_size_offset = s0, b0
        _layer(ip, sq, B).write(k[:sq] * 4, v[:sq] * 4)
        assert torch.equal(ip.kv_scale_dict[1], want), (s0, b0, sq)


# ------------------------------------------------- step kinds and refusals

_PAGED = ("paged KV cache: {} is not supported (only the whole-prompt prefill of one row and the "
          "ragged decode step are); use kv_pages=None")
_ONE_SLOT_PER_ROW = (
    "paged KV cache: a decode step needs one device cache slot per row (the ragged decoders of "
    "inference/continuous.py); the eager loop and the lockstep decoders of "
    "inference/hip_graph.py are not paged; use kv_pages=None")
_NO_SLOTS = _PAGED.format("a decode step without device slots (the eager KV-cached loop)")
_CONTINUES = _PAGED.format("a prefill that continues a cached sequence (sequence_len_offset > 0)")
_ROWS = _PAGED.format("a prefill of more than one row")
_CALIBRATE = _PAGED.format("prompt calibration of the FP8 KV scales (--inference_fp8_kv_calibrate)")
_HIP_GRAPH = ("hipGraph decode needs the native decode attention kernel (GPU, bf16/fp16, "
              "head_dim 64 or 128)")

# (paged, dict(s0, slots, cont), sq, b, fused) -> the kind, or the refusal's text
_STEPS = (
    (False, dict(slots=[5]), 1, B, False, DEVICE_DECODE),
    (False, dict(slots=[5]), 1, B, True, DEVICE_DECODE),
    (False, dict(slots=[5, 1, 9]), 1, B, False, DEVICE_DECODE),
    (False, dict(slots=[5, 1, 9]), 1, B, True, DEVICE_DECODE),
    (False, dict(s0=5), 1, B, False, EAGER_DECODE),
    (False, dict(s0=5), 1, B, True, EAGER_DECODE),
    (False, dict(s0=0), 1, B, False, EAGER_DECODE),
    (False, dict(s0=0), 4, B, False, RESTART_PREFILL),
    (False, dict(s0=0, slots=[5]), 4, B, False, RESTART_PREFILL),  # slots count at sq == 1 only
    (False, dict(s0=3), 4, B, False, CONTINUED_PREFILL),
    (False, dict(s0=3, cont=True), 4, B, False, CONTINUED_PREFILL),
    (True, dict(slots=[5, 1, 9]), 1, B, False, DEVICE_DECODE),
    (True, dict(slots=[5, 1, 9]), 1, B, True, DEVICE_DECODE),
    (True, dict(slots=[5]), 1, B, False, _ONE_SLOT_PER_ROW),
    (True, dict(slots=[5]), 1, B, True, _ONE_SLOT_PER_ROW),
    (True, dict(slots=[5]), 1, 1, False, DEVICE_DECODE),  # one row: its one slot
    (True, dict(s0=5), 1, B, False, _NO_SLOTS),
    (True, dict(s0=5, cont=True), 1, 1, False, _NO_SLOTS),
    (True, dict(s0=5), 1, B, True, _ONE_SLOT_PER_ROW),
    (True, dict(s0=0), 4, 1, False, RESTART_PREFILL),
    (True, dict(s0=0, slots=[5, 1, 9]), 4, 1, False, RESTART_PREFILL),
    (True, dict(s0=0), 4, B, False, _ROWS),
    (True, dict(s0=3), 4, 1, False, _CONTINUES),
    (True, dict(s0=3), 4, B, False, _CONTINUES),
    (True, dict(s0=3, cont=True), 4, 1, False, CONTINUED_PREFILL),
    (True, dict(s0=3, cont=True), 4, B, False, _ROWS),
)


def _kind_or_refusal(make):
    try:
        return make().kind
    except NotImplementedError as e:
        return str(e)


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
def test_step_kinds_and_refusals(fp8_switch, fp8):
    fp8_switch(fp8)
    for paged, at, sq, b, fused, want in _STEPS:
        ip = _params(paged, **at)
        assert _kind_or_refusal(lambda: _layer(ip, sq, b, fused)) == want, (paged, at, sq, b, fused)
        assert kv_cache.step_kind(ip, sq) == want or want not in (
            DEVICE_DECODE, EAGER_DECODE, RESTART_PREFILL, CONTINUED_PREFILL)


def test_calibration_is_refused_on_a_paged_prefill_only(fp8_switch):
    fp8_switch(True, calibrate=True)
    assert _kind_or_refusal(lambda: _layer(_params(True), 4, 1)) == _CALIBRATE
    assert _kind_or_refusal(lambda: _layer(_params(True, slots=[5, 1, 9]), 1, B)) == DEVICE_DECODE
    assert _kind_or_refusal(lambda: _layer(_params(False), 4, B)) == RESTART_PREFILL
    fp8_switch(False, calibrate=True)  # a 16-bit pool has no scales to calibrate
    assert _kind_or_refusal(lambda: _layer(_params(True), 4, 1)) == RESTART_PREFILL


@pytest.mark.parametrize("paged", (False, True), ids=("columns", "paged"))
def test_device_slot_decode_on_the_gpu_needs_the_native_kernel(paged):
    """Classified from the device and the head dim alone: no GPU is touched (the
    cache is in place already, on the CPU)."""
    gpu = torch.device("cuda")
    ip = _params(paged, slots=[5, 1, 9])
    _layer(ip, 1, B)  # allocates
    assert _kind_or_refusal(lambda: _layer(ip, 1, B, device=gpu)) == _HIP_GRAPH
    assert _kind_or_refusal(lambda: _layer(ip, 1, B, fused=True, device=gpu)) == _HIP_GRAPH
    ip.device_offset = None
    ip.sequence_len_offset = 2
    if not paged:
        assert _kind_or_refusal(lambda: _layer(ip, 1, B, device=gpu)) == EAGER_DECODE
    ip64 = _params(paged, slots=[5, 1, 9])
    _layer(ip64, 1, B, hd=64)
    assert _kind_or_refusal(lambda: _layer(ip64, 1, B, device=gpu, hd=64)) == DEVICE_DECODE
