"""The device-slot multi-row cell of ``inference/kv_cache.py`` on the CPU: it is
opt-in (without ``ip.device_multi`` every call classifies as before), its
``write`` fills the cells that ``sq`` single-row device-slot writes fill, and
the combinations that are not built are refused."""
import pytest
import torch

from epfl_megatron_amd.inference import kv_cache
from epfl_megatron_amd.inference.forward_step import InferenceParams
from epfl_megatron_amd.inference.kv_cache import (CONTINUED_PREFILL, DEVICE_DECODE, DEVICE_MULTI,
                                                  EAGER_DECODE, RESTART_PREFILL, LayerKV, step_kind)
from epfl_megatron_amd.inference.paged import KV_PAGE

NKV, HD, B, CAP, PAGES, SQ = 2, 8, 3, 2 * KV_PAGE, 7, 4
CPU = torch.device("cpu")
TABLE = ((4, 2), (6, 1), (3, 5))  # two pages per row, neither adjacent nor in order
# first new position per row: mid-page, a page's last slot (the rows cross a page edge), 0
FIRST = (7, KV_PAGE - 1, 0)


@pytest.fixture
def fp8_switch():
    def switch(on, calibrate=False):
        kv_cache.set_fp8_kv_cache(on, calibrate=calibrate)
    yield switch
    kv_cache.set_fp8_kv_cache(False, calibrate=False)


def _params(paged, multi):
    ip = InferenceParams(B, CAP, kv_pages=PAGES if paged else None, table_device=CPU)
    if paged:
        ip.page_table[:B] = torch.tensor(TABLE, dtype=torch.int32)
    ip.device_multi = multi
    return ip


def _slot(paged, m, pos):
    return TABLE[m][pos // KV_PAGE] * KV_PAGE + pos % KV_PAGE if paged else pos


@pytest.mark.parametrize("sq", (1, 4))
@pytest.mark.parametrize("s0", (0, 5))
@pytest.mark.parametrize("slots", (None, [3]))
def test_without_the_flag_every_call_classifies_as_before(sq, s0, slots):
    want = (EAGER_DECODE if slots is None else DEVICE_DECODE) if sq == 1 else \
        (RESTART_PREFILL if s0 == 0 else CONTINUED_PREFILL)
    for multi in (False, True):
        ip = _params(False, multi)
        ip.sequence_len_offset = s0
        if slots is not None:
            ip.device_offset = torch.tensor(slots)
        if multi and sq > 1 and slots is not None:
            assert step_kind(ip, sq) == DEVICE_MULTI
        else:
            assert step_kind(ip, sq) == want


@pytest.mark.parametrize("fp8", (False, True), ids=("16bit", "e4m3"))
@pytest.mark.parametrize("paged", (False, True), ids=("columns", "paged"))
def test_multirow_write_fills_the_cells_of_single_row_writes(fp8_switch, fp8, paged):
    fp8_switch(fp8)
    g = torch.Generator().manual_seed(3)
    k, v = (torch.randn(SQ, B, NKV, HD, generator=g) * 3 for _ in range(2))
    mems = []
    for multi in (True, False):
        ip = _params(paged, multi)
        ip.device_kv_len = torch.tensor([f + SQ for f in FIRST], dtype=torch.int32)
        steps = [(0, SQ)] if multi else [(t, 1) for t in range(SQ)]
        for t, n in steps:
            ip.device_offset = torch.tensor([_slot(paged, m, FIRST[m] + t) for m in range(B)])
            kv = LayerKV(ip, 1, NKV, HD, torch.float32, CPU, n, B)
            assert kv.kind == (DEVICE_MULTI if multi else DEVICE_DECODE)
            if t == 0:
                for mem in ip.key_value_memory_dict[1]:
                    mem.fill_(7)
                if fp8:
                    kv.scales.copy_(torch.tensor([[0.5, 2.0], [4.0, 1.0]]))
            kv.write(k[t:t + n], v[t:t + n])
        mems.append(ip.key_value_memory_dict[1])
    for got, want in zip(*mems):
        assert got.dtype == (torch.uint8 if fp8 else torch.float32)
        assert torch.equal(got, want) and int((want != 7).sum()) > SQ * B * NKV * HD // 2


def test_one_slot_for_the_batch_writes_every_column():
    ip = _params(False, True)
    ip.device_offset, ip.device_kv_len = torch.tensor([9]), torch.tensor([9 + SQ], dtype=torch.int32)
    kv = LayerKV(ip, 1, NKV, HD, torch.float32, CPU, SQ, B)
    k, v = (torch.randn(SQ, B, NKV, HD) for _ in range(2))
    kv.write(k, v)
    assert torch.equal(kv.kmem[9:9 + SQ], k) and torch.equal(kv.vmem[9:9 + SQ], v)


@pytest.mark.parametrize("case", ("fused", "calibrate", "rows", "paged-one-slot"))
def test_refused_cells(fp8_switch, case):
    fp8_switch(case == "calibrate", calibrate=case == "calibrate")
    ip = _params(case == "paged-one-slot", True)
    ip.device_offset = torch.tensor([3] if case == "paged-one-slot" else [3, 4, 5])
    ip.device_kv_len = torch.full((B,), 9, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        LayerKV(ip, 1, NKV, HD, torch.float32, CPU, 17 if case == "rows" else SQ, B,
                fused=case == "fused")
