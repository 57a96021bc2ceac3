"""The guarded-buffer helper of the buffer-contract tests (tests/dev_buffers.py) on CPU tensors: every kind of damage the GPU tests rely on
it to see is planted and must be reported, at the right position.  This is the proof that tests/test_gpu_buffer_contract.py can fail."""
import numpy as np
import pytest

import dev_buffers as db

N, OFF, G = 37, 3, 64


def _buf(offset=OFF):
    return db.guarded(N, offset_words=offset, guard_words=G, device="cpu")


@pytest.mark.parametrize("offset", [0, 1, 2, 3, 127])
def test_layout(offset):
    g = _buf(offset)
    assert g.view.numel() == N and g.view.dtype.itemsize == 4
    assert (g.data_ptr() - 4 * offset) % 512 == 0           # `offset` words past a 512-byte boundary
    assert g.data_ptr() % 16 == (4 * offset) % 16
    assert g.start >= G + offset and g.base.numel() - (g.start + N) >= G  # at least G guard words on both sides, the gap extra
    assert (g.host() == db.SENTINEL).all()                  # the view starts as sentinel too
    assert db.SENTINEL >= 0x78000001
    g.assert_guards_intact()


def test_clean_buffer_passes():
    g = _buf()
    g.fill(np.arange(N))
    g.assert_guards_intact()
    g.assert_fully_written()
    assert np.array_equal(g.host(), np.arange(N, dtype=np.uint32))


@pytest.mark.parametrize("where,index,text", [
    ("word just before the view", lambda g: g.start - 1, r"BEFORE out: nearest is inside the offset gap, 1 word\(s\) before its first word"),
    ("word just after the view", lambda g: g.start + N, r"AFTER out: first is 1 word\(s\) past its last word"),
    ("first guard word", lambda g: 0, r"BEFORE out: nearest is %d word\(s\) before"),
    ("last guard word", lambda g: g.base.numel() - 1, r"AFTER out: first is %d word\(s\) past"),
    ("inside the offset gap", lambda g: g.boundary + 1, r"BEFORE out: nearest is inside the offset gap, 2 word\(s\) before"),
])
def test_planted_stray_write_is_reported(where, index, text):
    g = _buf()
    g.fill(np.arange(N))
    i = index(g)
    g.base[i] = 7
    if "%d" in text:
        text = text % (g.start if i == 0 else g.base.numel() - (g.start + N))
    with pytest.raises(AssertionError, match=text):
        g.assert_guards_intact("out")
    g.base[i] = db.SENTINEL - (1 << 32)
    g.assert_guards_intact("out")


def test_a_stray_sentinel_free_write_of_zero_is_seen_too():
    g = _buf(0)  # no gap: the word before the view is the last word of the leading guard
    g.base[g.start - 1] = 0
    with pytest.raises(AssertionError, match=r"nearest is 1 word\(s\) before its first word \(guard index %d of %d, value 0x00000000\)" % (g.start - 1, g.start)):
        g.assert_guards_intact()


def test_unwritten_output_word_is_reported():
    g = _buf()
    w = np.arange(N, dtype=np.uint32)
    g.fill(w)
    g.view[N - 2] = db.SENTINEL - (1 << 32)  # a kernel that skipped one word
    with pytest.raises(AssertionError, match=r"1 word\(s\) of out were never written: first is word %d of %d" % (N - 2, N)):
        g.assert_fully_written("out")


def test_placed_input_unchanged_and_modified():
    w = (np.arange(N, dtype=np.uint64) * 0x9E3779B1 % 0x78000001).astype(np.uint32)
    g = db.place(w, offset_words=1, guard_words=G, device="cpu")
    assert np.array_equal(g.host(), w)
    g.assert_unchanged()
    g.view[5] = int(w[5]) ^ 1
    with pytest.raises(AssertionError, match=r"1 word\(s\) of trace were modified: first is word 5 of %d" % N):
        g.assert_unchanged("trace")
    g.view[5] = int(w[5])
    g.base[g.start + N] = 1  # a read-only input whose neighbour was written
    with pytest.raises(AssertionError, match=r"AFTER trace: first is 1 word"):
        g.assert_unchanged("trace")


def test_assert_unchanged_needs_a_placed_buffer():
    with pytest.raises(AssertionError, match="place"):
        _buf().assert_unchanged()
