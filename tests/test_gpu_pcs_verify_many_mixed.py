"""GPU tests of the device PCS batch verifier over MIXED heights (include/p3hip.h p3hip_pcs_verifier_create_mixed): proofs come from
TwoAdicFriPcs(mixed_heights=True).open, the expected status of every member from the host verifier p3hip_pcs_verify_mixed through the
contract of tests/pcs_many.py.  The shapes are the smallest at which each roll-in, injection and index shift can go wrong; one is
past the small-layer thresholds."""
import gc

import numpy as np
import pytest

import pcs_many as M
import pcs_many_mixed as MM
import pcs_ref as R

pytestmark = pytest.mark.gpu
HASHES = M.HASHES
P = M.P


def host_entry(case, v, members):
    chals = []
    for m in members:
        ch = case.p3.Challenger(case.hash)
        try:
            ch.import_state(m["state"])
        except case.p3.P3HipError:  # a state no challenger can hold reaches the device entry only
            return None, None
        chals.append(ch)
    st = v.verify_many([m["proof"] for m in members], np.stack([m["roots"] for m in members]), np.stack([m["points"] for m in members]),
                       np.stack([m["opened"] for m in members]), chals)
    return st, chals


def dev_entry(case, v, members):
    """-> (statuses, rejected count, exported transcripts) through p3hip_pcs_verifier_verify_dev"""
    import torch
    p3, n = case.p3, len(members)
    stride = v.proof_len
    buf = np.zeros(n * stride, dtype=np.uint8)
    for i, m in enumerate(members):
        b = np.frombuffer(m["proof"], dtype=np.uint8)[:stride]
        buf[i * stride:i * stride + len(b)] = b
    lens = p3.dev_u32(np.array([len(m["proof"]) for m in members], dtype=np.uint32))
    st, rej, out = v.verify_many_dev(torch.from_numpy(buf).cuda(), p3.dev_u32(np.stack([m["roots"] for m in members])),
                                     p3.dev_u32(np.stack([m["points"] for m in members])), p3.dev_u32(np.stack([m["opened"] for m in members])),
                                     p3.dev_u32(np.stack([m["state"] for m in members])), lens=lens, n=n, stride=stride)
    torch.cuda.synchronize()
    return p3.host_u32(st), int(p3.host_u32(rej)[0]), p3.host_u32(out)


def same_transcript(a, b):
    return np.array_equal(a.sample_ext(), b.sample_ext()) and a.sample_bits(19) == b.sample_bits(19)


def imported(p3, hash, words):
    ch = p3.Challenger(hash)
    ch.import_state(words)
    return ch


# ---- 1. accept ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("name", list(MM.SHAPES))
def test_accepts_what_the_device_open_proves(p3, oracle, hash, kind, name):
    lfp, spec = MM.SHAPES[name]
    i = list(MM.SHAPES).index(name)
    case = MM.Case(p3, hash, (1 + (i + kind) % 2, lfp, 5, 4), spec, 3, 9000 + 10 * i + kind)  # both hashes see both blowups
    v = case.verifier(3)
    assert all(len(m["proof"]) == v.proof_len for m in case.members)
    left = []
    for m in case.members:  # the host verifier accepts and stands where the prover stands
        h, ch = case.host(m)
        assert h == 0 and same_transcript(ch.clone(), m["after"].clone())
        left.append(ch)
    st, rej, out = dev_entry(case, v, case.members)
    assert not st.any() and rej == 0, (st, rej)
    for ch, words in zip(left, out):  # the exported transcript is the one p3.pcs.verify leaves
        assert same_transcript(imported(p3, hash, words), ch.clone())
    if name == "consecutive folds":
        st, chals = host_entry(case, v, case.members)
        assert not st.any(), st
        for ch, mine in zip(left, chals):
            assert same_transcript(mine, ch.clone())
    v.close()


# ---- 2. every word ----------------------------------------------------------------------------------------------------------------
_every = {}


def _every_word_case(p3, hash):
    if hash not in _every:
        fp, spec = MM.EVERY_WORD
        case = MM.Case(p3, hash, fp, spec, 1, 9200)
        assert case.expected(case.members[0]) == (0, True)
        _every[hash] = case
    return _every[hash]


def _check_tampered(case, v, field, entry):
    """one member per tampered word of `field`, one member at a time; -> (members, members under the equality clause)"""
    base = case.members[0]
    n = inside = 0
    flat = np.frombuffer(base[field], dtype=np.uint32) if field == "proof" else base[field].reshape(-1)
    for i in range(len(flat)):
        t = flat.copy()
        t[i] = M.tampered(t[i])
        m = dict(base)
        m[field] = t.tobytes() if field == "proof" else t.reshape(base[field].shape)
        want, eq = case.expected(m)
        st = host_entry(case, v, [m])[0] if entry == "host" else None
        if st is None:
            st = dev_entry(case, v, [m])[0]
        assert st[0] == want, "%s word %d: status %d, the contract says %d" % (field, i, st[0], want)
        n += 1
        inside += eq
    return n, inside


@pytest.mark.parametrize("hash,kind", HASHES)
def test_every_word_of_the_proof(p3, oracle, hash, kind):
    case = _every_word_case(p3, hash)
    v = case.verifier(1)
    assert len(case.classes) * 4 == v.proof_len
    assert v.proof_len != p3.pcs_proof_len(case.params, hash, 3, MM.verifier_shape(case.spec), case.n_slots)  # round 1's tree is shorter
    n, inside = _check_tampered(case, v, "proof", "host")
    print("mixed shape %s: %d of %d tampered proofs under the equality clause (%.3f)" % (hash, inside, n, inside / n))
    v.close()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_every_argument_word(p3, oracle, hash, kind):
    case = _every_word_case(p3, hash)
    v = case.verifier(1)
    for field in ("opened", "roots", "points", "state"):
        n, inside = _check_tampered(case, v, field, "host" if field != "state" else "dev")
        print("mixed shape %s %s: %d of %d under the equality clause (%.3f)" % (hash, field, inside, n, inside / n))
    v.close()


# ---- 3. both forms ----------------------------------------------------------------------------------------------------------------
def _final_poly_mismatch(case, m):
    """m with one word of the final polynomial replaced so that the host verifier answers 15.  The final polynomial is observed before
    the query indices are drawn, so most replacements move the indices and the input openings fail first (13): the first value that
    leaves both 4-bit indices where they were is taken (one in 256; the search is the host verifier's and deterministic)."""
    i = len(case.classes) - 3
    # a replacement keeps the indices with probability 2^-(num_queries * log_big) = 2^-8 here: 6000 tries miss with probability
    # (255/256)^6000 < 1e-10.  With more queries or a taller shape the bound, and this loop, grow by that factor.
    for d in range(1, 6000):
        t = MM.with_proof_word(m, i, lambda v: (int(v) + d) % P)
        if case.expected(t)[0] == 15:
            return t
    raise AssertionError("no replacement of final-polynomial word %d leaves the query indices in place" % i)


@pytest.mark.parametrize("w", [255, 256, 257])
def test_row_words_on_both_sides_of_the_form_switch(p3, oracle, w):
    """a tall matrix and a short one at two points: the row words of a query are w, the switch is at pcs.WAVE_FORM_MIN_COLUMNS"""
    assert p3.pcs.WAVE_FORM_MIN_COLUMNS == 256
    spec = [[(3, w - 10, [0]), (1, 10, [0, 1])]]
    for hash, kind in HASHES:
        case = MM.Case(p3, hash, (1, 0, 2, 0), spec, 3, 9300 + w + kind)
        v = case.verifier(3)
        assert v.wave_form == (w >= 256) and v.total == w + 10
        good = case.members[0]
        row = MM.with_proof_word(case.members[1], case.word(0, "row", mat=1, k=7, query=1))  # a row word of the short matrix
        fin = _final_poly_mismatch(case, case.members[2])
        assert [case.expected(m)[0] for m in (good, row, fin)] == [0, 13, 15]
        st, rej, _ = dev_entry(case, v, [good, row, fin])
        assert list(st) == [0, 13, 15] and rej == 2, (st, rej)
        v.close()


# ---- 4. deeper indices ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", HASHES)
def test_a_shape_past_the_small_layer_thresholds(p3, oracle, hash, kind):
    fp, spec = MM.DEEP
    case = MM.Case(p3, hash, fp, spec, 3, 9400 + kind)
    v = case.verifier(4)
    assert v.wave_form is False
    # a digest of round 1's path, five levels up: that tree has depth 11 under a 14-bit index
    bad = MM.with_proof_word(case.members[1], case.word(1, "path", k=8 * 5 + 3, query=2))
    batch = [case.members[0], bad, case.members[1], case.members[2]]
    want = [case.expected(m)[0] for m in batch]
    assert want == [0, 13, 0, 0]
    st, rej, out = dev_entry(case, v, batch)
    assert list(st) == want and rej == 1, (st, rej)
    for m, words in zip(batch, out):
        if m is not bad:
            assert same_transcript(imported(p3, hash, words), m["after"].clone())
    v.close()


# ---- 5. equal heights through the mixed entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", HASHES)
def test_equal_heights_through_the_mixed_entry(p3, oracle, hash, kind):
    """shape A of tests/pcs_many.py: a verifier from the mixed entry and one from the same-height entry answer alike"""
    spec = [[(M.LOG_H_AB, w, sl) for w, sl in zip(ws, ss)] for ws, ss in zip(M.WIDTHS_AB, M.SLOTS_AB)]
    case = MM.Case(p3, hash, M.FP_AB, spec, 1, 9500 + kind)  # a same-height open on a mixed-enabled object is the plain open
    shape = M.verifier_shape(M.WIDTHS_AB, M.SLOTS_AB)
    old = p3.PcsVerifier(M.LOG_H_AB, shape, 2, case.params, hash, False, 11)
    new = p3.PcsVerifier(MM.heights_of(spec), shape, 2, case.params, hash, False, 11)
    assert new.proof_len == old.proof_len == 322 * 4 and new.wave_form == old.wave_form
    good = case.members[0]
    picks = np.linspace(0, len(case.classes) - 1, 10).astype(int)  # ten words from the first to the last, of every kind
    batch = [good] + [MM.with_proof_word(good, int(i)) for i in picks]
    want = [case.expected(m)[0] for m in batch]
    assert want[0] == 0 and all(want[1:]), want
    a, b = dev_entry(case, old, batch), dev_entry(case, new, batch)
    assert list(a[0]) == want and list(b[0]) == want and a[1] == b[1] == 10
    assert np.array_equal(a[2][0], b[2][0])  # the accepted member's exported transcript
    sa, ca = host_entry(case, old, batch)
    sb, cb = host_entry(case, new, batch)
    assert list(sa) == want and list(sb) == want
    for x, y in zip(ca, cb):  # accepted: advanced alike; rejected: left alone alike
        assert np.array_equal(x.export_state(), y.export_state())
    old.close()
    new.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------------
def test_create_verify_destroy_cycles_return_their_memory(p3, oracle):
    import psutil
    import torch
    cases = [_every_word_case(p3, "poseidon2"), _every_word_case(p3, "keccak")]

    def cycle():
        for c in cases:
            v = c.verifier(8)
            assert not host_entry(c, v, c.members * 3)[0].any()
            assert not dev_entry(c, v, c.members * 8)[0].any()
            v.close()
        gc.collect()
        torch.cuda.empty_cache()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for _ in range(3):
        cycle()
    me = psutil.Process()
    base, rss0 = free_bytes(), me.memory_info().rss
    for _ in range(25):
        cycle()
    lost, grown = base - free_bytes(), me.memory_info().rss - rss0
    MIB = 1 << 20
    # 50 verifiers with 15 device buffers and a stream each: the smallest leaked buffer costs a 2 MiB granule per cycle
    assert lost < 8 * MIB, "free device memory fell by %.1f MiB over 25 create / verify / destroy cycles" % (lost / MIB)
    assert grown < 64 * MIB, "resident host memory grew by %.1f MiB over 25 create / verify / destroy cycles" % (grown / MIB)
