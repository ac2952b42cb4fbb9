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

Prefix sharing (``PrefixCache``): a full page of prompt tokens whose K / V a
prefill has written can serve every later prompt that starts with the same
tokens.  The cache is a host-side index over such pages, a trie whose edges are
the exact 256 token ids of a page, with a reference count per page (the rows
reading it now).  A page the cache holds is simply "out" for the ``PagePool``;
``evict`` hands unreferenced leaves back, least recently used first.  A row that
shares ``m`` pages starts its prefill at position ``m * KV_PAGE`` and attends
over the shared keys through its table (the paged forms of the forward
attention kernel, ``ops.attention.flash_attn_paged``).  Shared pages are never
written: only full prompt pages are shared, a continued prefill writes at
positions ``>= m * KV_PAGE`` and the decoder at positions ``>= len(prompt)``.

Out of scope here: copy-on-write and sharing of partial pages, sharing
generated tokens, growing a row page by page and preemption (a request's pages
are all reserved at admission), paged lockstep decoders and beam search, a
configurable page size, a server flag.
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


class _PrefixEntry:
    """One cached page: a full page of prompt tokens below ``parent``."""
    __slots__ = ("parent", "key", "page", "refs", "tick", "children")

    def __init__(self, parent, key, page, tick):
        self.parent, self.key, self.page = parent, key, page
        self.refs, self.tick, self.children = 0, tick, 0


def _page_bytes(prompt, i):
    return prompt[i * KV_PAGE:(i + 1) * KV_PAGE].numpy().tobytes()


def _token_ids(prompt):
    return torch.as_tensor(prompt, dtype=torch.long).view(-1).cpu()


class PrefixCache:
    """Host index of the full prompt pages whose K / V are in the pool, for
    prefix sharing.  An entry's key is ``(parent entry, the bytes of the
    page's KV_PAGE token ids)``, exact (the root's parent is None), its value
    the page id; it counts the rows reading it (``refs``) and remembers when
    it was last acquired or released (``tick``).  The cache owns its pages:
    they stay allocated in ``pool`` until ``evict`` / ``clear`` frees them."""

    def __init__(self, pool):
        self.pool = pool
        self._index = {}
        self._tick = 0

    def __len__(self):
        return len(self._index)

    def pages(self):
        """The page ids the cache holds."""
        return sorted(e.page for e in self._index.values())

    def _touch(self, e):
        self._tick += 1
        e.tick = self._tick

    def match(self, prompt):
        """The longest chain of cached entries for the leading full pages of
        ``prompt``, at most ``(len(prompt) - 2) // KV_PAGE`` of them: at least
        two tokens stay to be prefilled (a one-token prefill would take the
        decode step's branch).  Moves no reference count."""
        prompt = _token_ids(prompt)
        chain, parent = [], None
        for i in range(max(0, (prompt.numel() - 2) // KV_PAGE)):
            e = self._index.get((parent, _page_bytes(prompt, i)))
            if e is None:
                break
            chain.append(e)
            parent = e
        return chain

    def acquire(self, chain):
        """A row starts reading the chain's pages."""
        for e in chain:
            e.refs += 1
            self._touch(e)

    def release(self, chain):
        """A row stops reading the chain's pages."""
        for e in chain:
            if e.refs < 1:
                raise ValueError(f"page {e.page} is released more often than acquired")
        for e in chain:
            e.refs -= 1
            self._touch(e)

    def insert(self, prompt, pages, n_matched):
        """After the prefill of ``prompt`` into the row whose table lists
        ``pages`` (the ``n_matched`` acquired pages of ``match`` first):
        register the row's further full prompt pages, ``i >= n_matched`` with
        ``(i + 1) * KV_PAGE <= len(prompt)``.  Returns the new entries; the row
        holds a reference to each and the cache owns their pages from now on.
        Where an identical entry exists already the row keeps its page private
        (and the walk goes on below the existing entry)."""
        prompt = _token_ids(prompt)
        parent = None
        for i in range(n_matched):
            parent = self._index[(parent, _page_bytes(prompt, i))]
            if parent.page != pages[i]:
                raise ValueError(f"page {pages[i]} is not the cached page of the prompt's page {i}")
        added = []
        for i in range(n_matched, min(prompt.numel() // KV_PAGE, len(pages))):
            key = (parent, _page_bytes(prompt, i))
            e = self._index.get(key)
            if e is None:
                self._tick += 1
                e = self._index[key] = _PrefixEntry(parent, key, int(pages[i]), self._tick)
                e.refs = 1
                if parent is not None:
                    parent.children += 1
                added.append(e)
            parent = e
        return added

    def evict(self, n):
        """Free up to ``n`` pages to the pool: entries nobody reads and no
        cached page continues, least recently used first (a parent becomes
        eligible once its last child has gone).  Returns the pages freed."""
        freed = []
        while len(freed) < n:
            idle = [e for e in self._index.values() if e.refs == 0 and e.children == 0]
            if not idle:
                break
            for e in sorted(idle, key=lambda e: e.tick)[:n - len(freed)]:
                del self._index[e.key]
                if e.parent is not None:
                    e.parent.children -= 1
                freed.append(e.page)
        if freed:
            self.pool.free(freed)
        return freed

    def clear(self):
        """Evict everything unreferenced."""
        return self.evict(len(self._index))
