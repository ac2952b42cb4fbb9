"""Paged KV cache for ragged decode: the page size, the host page allocator
and the index helpers shared by the model code, the decoders and the tests.

With ``InferenceParams(..., kv_pages=N)`` a layer's cache is one pool of ``N``
pages of ``KV_PAGE`` keys (``[N * KV_PAGE, 1, nkv, hd]`` for K and for V) in
place of a full-capacity column per row, and ``ip.page_table`` (device int32
``[max_batch_size, pages_per_row]``) says where a row's keys live: key ``i`` of
row ``b`` is pool row ``page_table[b, i // KV_PAGE] * KV_PAGE + i % KV_PAGE``.

Page 0 is the null page: never handed out, the target of every table entry
nobody owns and of the K / V write an idle row (``slot = 0``, ``kv_len = 0``)
still performs on every replay of the captured step.

``KV_PAGE`` is fixed at 256 keys, the largest chunk of the decode attention
kernel (4 waves x 64 keys) and a multiple of the smaller ones, so that no chunk
straddles a page and the indirection is one uniform table load per workgroup
(``csrc/flash_decode.hip``; ``csrc/kernels.h`` holds the same constant).

Out of scope here: prefix sharing and copy-on-write, growing a row page by
page and preemption (a request's pages are all reserved at admission), paged
lockstep decoders and beam search, a configurable page size, a server flag.
"""
import torch

KV_PAGE = 256


def pages_for(n_tokens):
    """Pages that hold ``n_tokens`` keys."""
    return (int(n_tokens) + KV_PAGE - 1) // KV_PAGE


def physical_slots(table_row, positions):
    """Pool rows of the logical ``positions`` (int64 tensor) of the sequence
    whose pages ``table_row`` (int32 ``[pages_per_row]``) lists; device-side
    torch ops only."""
    return table_row[positions // KV_PAGE].long() * KV_PAGE + positions % KV_PAGE


def gather_rows(pool, table_row, n):
    """The first ``n`` keys of a sequence as a contiguous ``[n, ...]`` tensor
    gathered from ``pool [n_pages * KV_PAGE, ...]``."""
    pos = torch.arange(int(n), device=pool.device)
    return pool[physical_slots(table_row.to(pool.device), pos)]


class PagePool:
    """Host free list over the pages ``1 .. n_pages - 1`` (page 0 is the null
    page).  Pages are handed out lowest first, so a run is reproducible."""

    def __init__(self, n_pages):
        if n_pages < 2:
            raise ValueError("a page pool needs the null page and at least one more")
        self.n_pages = int(n_pages)
        self._free = list(range(self.n_pages - 1, 0, -1))  # pop() takes the lowest
        self._out = set()
        self.peak = 0

    @property
    def available(self):
        return len(self._free)

    @property
    def in_use(self):
        return len(self._out)

    def alloc(self, n):
        """``n`` pages as a list, or None when fewer are free (nothing is taken)."""
        if n < 0:
            raise ValueError("cannot allocate a negative number of pages")
        if n > len(self._free):
            return None
        pages = [self._free.pop() for _ in range(n)]
        self._out.update(pages)
        self.peak = max(self.peak, len(self._out))
        return pages

    def free(self, pages):
        """Return ``pages``; a page that is not out (a double free, page 0, a
        page outside the pool) raises and nothing is returned."""
        pages = list(pages)
        for p in pages:
            if p == 0:
                raise ValueError("page 0 is the null page: it is never allocated or freed")
            if p not in self._out or pages.count(p) > 1:
                raise ValueError(f"page {p} is not allocated (double free?)")
        for p in pages:
            self._out.remove(p)
            self._free.append(p)
        self._free.sort(reverse=True)
