"""Guarded, offset buffers for the tests of the C ABI's BUFFER CONTRACT (include/p3hip.h).

Torch's allocator hands out 512-byte-aligned blocks and rounds sizes up, so a kernel that needs an alignment it never checks, or that
stores a few words past its output, goes unnoticed on fresh tensors.  The buffers here sit INSIDE one allocation, a chosen number of
words past a 512-byte boundary, with sentinel words all round:

    | guard_words .. (alignment slack) | offset gap | the view: n_words | guard_words .. |
      ^ allocation start                 ^ 512-byte boundary            ^ everything from here to the allocation's end is guard

The sentinel 0xDEADBEEF is >= P = 0x78000001, so no field output equals it; the view is pre-filled with it as well, so a word a kernel
was supposed to write and did not shows up too.  A plain module (no fixtures): CPU tensors serve the host test of the helper itself."""
import numpy as np

SENTINEL = 0xDEADBEEF
_SENTINEL_I32 = SENTINEL - (1 << 32)  # the same bits as an int32
ALIGN_WORDS = 128                     # 512 bytes


def _default_device():
    import torch
    return "cuda" if torch.cuda.is_available() else "cpu"


class Guarded:
    """`n_words` 32-bit words whose data_ptr() is `offset_words * 4` bytes past a 512-byte boundary, inside one allocation with at least
    `guard_words` sentinel words before and after.  The offset gap counts as guard."""

    def __init__(self, n_words, offset_words=0, guard_words=4096, device=None):
        import torch
        assert n_words >= 0 and 0 <= offset_words < ALIGN_WORDS and guard_words >= 1
        self.n, self.offset, self.guard = int(n_words), int(offset_words), int(guard_words)
        total = self.guard + (ALIGN_WORDS - 1) + self.offset + self.n + self.guard
        self.base = torch.full((total,), _SENTINEL_I32, dtype=torch.int32, device=device or _default_device())
        assert self.base.data_ptr() % 4 == 0
        first = self.base.data_ptr() // 4 + self.guard          # word address of the earliest admissible boundary
        self.boundary = self.guard + (-first) % ALIGN_WORDS      # index of the 512-byte boundary in `base`
        self.start = self.boundary + self.offset
        self.view = self.base[self.start:self.start + self.n]
        assert self.view.data_ptr() == self.base.data_ptr() + 4 * self.start
        assert (self.view.data_ptr() - 4 * self.offset) % (4 * ALIGN_WORDS) == 0
        self._expected = None  # place(): the words the buffer must still hold afterwards

    # ---- access ----
    def data_ptr(self):
        return self.view.data_ptr()

    def host(self):
        """the view's words as a numpy uint32 array (a copy)"""
        return self.view.cpu().numpy().view(np.uint32).copy()

    def fill(self, words):
        import torch
        w = np.array(words, dtype=np.uint32).reshape(-1)  # a copy: torch takes writable arrays only
        assert w.size == self.n, (w.size, self.n)
        self.view.copy_(torch.from_numpy(w.view(np.int32)))
        return self

    # ---- checks ----
    def assert_guards_intact(self, what="buffer"):
        """Fails naming the first damaged guard word on each side and its distance from the view."""
        b = self.base.cpu().numpy().view(np.uint32)
        end = self.start + self.n
        before = np.nonzero(b[:self.start] != SENTINEL)[0]
        after = np.nonzero(b[end:] != SENTINEL)[0]
        msgs = []
        if before.size:
            i = int(before[-1])  # the damaged word nearest to the view
            where = "inside the offset gap, " if i >= self.boundary else ""
            msgs.append("%d guard word(s) damaged BEFORE %s: nearest is %s%d word(s) before its first word (guard index %d of %d, value 0x%08x)"
                        % (before.size, what, where, self.start - i, i, self.start, int(b[i])))
        if after.size:
            i = int(after[0])
            msgs.append("%d guard word(s) damaged AFTER %s: first is %d word(s) past its last word (guard index %d of %d, value 0x%08x)"
                        % (after.size, what, i + 1, i, b.size - end, int(b[end + i])))
        assert not msgs, "; ".join(msgs)

    def assert_fully_written(self, what="buffer"):
        """Fails naming the first word of the view that still holds the sentinel (outputs never equal it: it is >= P)."""
        left = np.nonzero(self.host() == SENTINEL)[0]
        assert not left.size, "%d word(s) of %s were never written: first is word %d of %d" % (left.size, what, int(left[0]), self.n)

    def assert_unchanged(self, what="input"):
        """place()d buffers: every word still as placed, bit for bit, and the guards intact."""
        assert self._expected is not None, "assert_unchanged is for buffers made by place()"
        got = self.host()
        bad = np.nonzero(got != self._expected)[0]
        assert not bad.size, "%d word(s) of %s were modified: first is word %d of %d (0x%08x, was 0x%08x)" % (
            bad.size, what, int(bad[0]), self.n, int(got[bad[0]]), int(self._expected[bad[0]]))
        self.assert_guards_intact(what)


def guarded(n_words, offset_words=0, guard_words=4096, device=None):
    """An OUTPUT buffer: sentinel everywhere, the view included."""
    return Guarded(n_words, offset_words, guard_words, device)


def place(words, offset_words=0, guard_words=4096, device=None):
    """An INPUT: `words` (any uint32 array) at the given offset; assert_unchanged() later proves the call read it in place and only read."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    g = Guarded(w.size, offset_words, guard_words, device).fill(w)
    g._expected = w.copy()
    return g
