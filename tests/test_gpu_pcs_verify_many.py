"""GPU tests of the device PCS batch verifier (include/p3hip.h "batches of PCS proofs verified ON THE DEVICE"): proofs come from the
device open of TwoAdicFriPcs / HidingFriPcs, the expected status of every member from the host verifiers p3hip_pcs_verify[_hiding]
through the contract of tests/pcs_many.py."""
import gc

import numpy as np
import pytest

import pcs_many as M
import pcs_ref as R

pytestmark = pytest.mark.gpu
HASHES = M.HASHES
P = M.P


class Case:
    """n members of one shape, proved on the device; widths are the caller's, cw the committed ones"""

    def __init__(self, p3, hash, hiding, log_h, fp, widths, slots, n, seed, nrc=2, base_point=False):
        rng = np.random.default_rng(seed)
        self.p3, self.hash, self.hiding, self.log_h, self.fp, self.slots = p3, hash, hiding, log_h, fp, slots
        self.n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
        self.params = p3.FriParameters(*fp)
        pcs = (p3.HidingFriPcs(self.params, hash, num_random_codewords=nrc, mmcs_seed=seed + 1, pcs_seed=seed + 2) if hiding
               else p3.TwoAdicFriPcs(self.params, hash))
        self.members = []
        for j in range(n):
            pts = np.stack([R.rand_point(rng) for _ in range(self.n_slots)])
            if base_point:
                pts[0] = R.ext_from_base(R.ONE)  # a base-field point no LDE coset holds
            mat_points = M.expand(pts, slots)
            rounds, roots = [], []
            for ws, mps in zip(widths, mat_points):
                root, data = pcs.commit([(R.rand_matrix(rng, log_h, w), R.rand_shift(rng) if rng.integers(0, 2) else None) for w in ws])
                rounds.append((data, mps))
                roots.append(root)
            ch = M.prefix(p3.Challenger(hash), seed + j)
            state = ch.export_state()
            opened, proof = pcs.open(rounds, ch)
            self.cw = [[d.dims[i][1] for i in range(len(ws))] for (d, _), ws in zip(rounds, widths)]
            self.members.append(dict(proof=proof, roots=np.stack(roots), points=pts, opened=opened.copy(), state=state, after=ch))
            for d, _ in rounds:
                d.free()
        pcs.free()
        self.classes = M.word_classes(0 if hash == "poseidon2" else 1, fp, log_h + (1 if hiding else 0), self.cw, 4 if hiding else 0)

    def verifier(self, max_proofs):
        return self.p3.PcsVerifier(self.log_h, M.verifier_shape(self.cw, self.slots), self.n_slots, self.params, self.hash, self.hiding, max_proofs)

    def expected(self, m):
        """the contract's status for a (possibly tampered) member, and whether the equality clause decides it"""
        h, _ = M.host_code(self.p3, self.fp, self.hash, self.hiding, self.log_h, self.cw, m["roots"], M.expand(m["points"], self.slots),
                           m["opened"], m["proof"], m["state"])
        words = np.frombuffer(m["proof"][:len(m["proof"]) // 4 * 4], dtype=np.uint32)
        canon = (len(words) == len(self.classes) and M.canonical(words, self.classes) and not np.any(m["opened"] >= P)
                 and not np.any(m["points"] >= P))
        return M.expected_status(h, canon), M.in_equality_clause(h, canon)


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


def dev_entry(case, v, members, with_lens=True, pad=0):
    """-> (statuses, rejected count, exported transcripts) through p3hip_pcs_verifier_verify_dev; the buffer is exactly as large as
    the stride requires"""
    import torch
    p3, n = case.p3, len(members)
    stride = v.proof_len + pad
    buf = np.zeros(n * stride, dtype=np.uint8)
    for i, m in enumerate(members):
        b = np.frombuffer(m["proof"], dtype=np.uint8)[:stride]
        buf[i * stride:i * stride + len(b)] = b
    lens = p3.dev_u32(np.array([len(m["proof"]) for m in members], dtype=np.uint32)) if with_lens else None
    st, rej, out = v.verify_many_dev(torch.from_numpy(buf).cuda(), p3.dev_u32(np.stack([m["roots"] for m in members])),
                                     p3.dev_u32(np.stack([m["points"] for m in members])), p3.dev_u32(np.stack([m["opened"] for m in members])),
                                     p3.dev_u32(np.stack([m["state"] for m in members])), lens=lens, n=n, stride=stride)
    torch.cuda.synchronize()
    return p3.host_u32(st), int(p3.host_u32(rej)[0]), p3.host_u32(out)


def same_transcript(a, b):
    return np.array_equal(a.sample_ext(), b.sample_ext()) and a.sample_bits(19) == b.sample_bits(19)


# ---- 1. accept ----------------------------------------------------------------------------------------------------------------
def _random_shape(log_h, kind, hiding):
    rng = np.random.default_rng(4000 + 10 * log_h + 2 * kind + hiding)
    rounds = R.random_case(rng, log_h, max_cols=300)
    if hiding:
        rounds = [mats[:4] for mats in rounds]
        if not any(pts for mats in rounds for _, _, pts in mats):
            m, s, _ = rounds[0][0]
            rounds[0][0] = (m, s, [R.rand_point(rng)])
    _, slots = M.slots_of([[pts for _, _, pts in mats] for mats in rounds])
    fp = (int(rng.integers(1, 3)), int(rng.integers(0, log_h)), int(rng.integers(1, 4)), int(rng.integers(0, 4)))
    return [[m.shape[1] for m, _, _ in mats] for mats in rounds], slots, fp


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("log_h", range(1, 7))
def test_accepts_what_the_device_open_proves(p3, oracle, hash, kind, hiding, log_h):
    widths, slots, fp = _random_shape(log_h, kind, hiding)
    case = Case(p3, hash, hiding, log_h, fp, widths, slots, 4, 5000 + log_h)
    v = case.verifier(4)
    assert all(len(m["proof"]) == v.proof_len for m in case.members)
    for m in case.members:  # the host verifier accepts and leaves the prover's transcript
        assert case.expected(m) == (0, True)
    st, chals = host_entry(case, v, case.members)
    assert not st.any(), st
    for m, ch in zip(case.members, chals):
        assert same_transcript(ch, m["after"].clone())
    for with_lens, pad in ((True, 0), (False, 20)):
        st, rej, out = dev_entry(case, v, case.members, with_lens, pad)
        assert not st.any() and rej == 0, (st, rej)
        for m, words in zip(case.members, out):
            ch = p3.Challenger(hash)
            ch.import_state(words)
            assert same_transcript(ch, m["after"].clone())
    v.close()


# ---- 2 / 3. every word ----------------------------------------------------------------------------------------------------------
_ab = {}


def _shape_ab(p3, hash, hiding):
    key = (hash, hiding)
    if key not in _ab:
        case = Case(p3, hash, hiding, M.LOG_H_AB, M.FP_AB, M.WIDTHS_AB, M.SLOTS_AB, 1, 6000 + hiding, nrc=M.NRC_B)
        assert case.expected(case.members[0]) == (0, True)
        _ab[key] = case
    return _ab[key]


def _check_tampered(case, v, field, entry):
    """one batch of one member per tampered word of `field`; -> (members, members under the equality clause)"""
    base = case.members[0]
    n = inside = 0
    flat = np.frombuffer(base[field], dtype=np.uint32) if field == "proof" else base[field].reshape(-1)
    for i in range(len(flat)):
        t = flat.copy()
        t[i] = M.tampered(t[i])
        m = dict(base)
        m[field] = t.tobytes() if field == "proof" else t.reshape(base[field].shape)
        want, eq = case.expected(m)
        if entry == "host":
            st, _ = host_entry(case, v, [m])
            if st is None:
                st = dev_entry(case, v, [m])[0]
        else:
            st = dev_entry(case, v, [m])[0]
        assert st[0] == want, "%s word %d: status %d, the contract says %d" % (field, i, st[0], want)
        n += 1
        inside += eq
    return n, inside


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("hiding", [False, True])
def test_every_word_of_the_proof(p3, oracle, hash, kind, hiding):
    case = _shape_ab(p3, hash, hiding)
    v = case.verifier(1)
    assert v.proof_len == (512 if hiding else 322) * 4
    n, inside = _check_tampered(case, v, "proof", "host")
    print("shape %s %s: %d of %d tampered proofs under the equality clause" % ("B" if hiding else "A", hash, inside, n))
    assert inside / n >= 0.90
    v.close()


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("hiding", [False, True])
def test_every_argument_word(p3, oracle, hash, kind, hiding):
    case = _shape_ab(p3, hash, hiding)
    v = case.verifier(1)
    for field in ("opened", "roots", "points", "state"):
        n, inside = _check_tampered(case, v, field, "host" if field != "state" else "dev")
        print("shape %s %s %s: %d of %d under the equality clause" % ("B" if hiding else "A", hash, field, inside, n))
    v.close()


# ---- 4. malformed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("hiding", [False, True])
def test_malformed_members_and_their_neighbours(p3, oracle, hash, kind, hiding):
    case = _shape_ab(p3, hash, hiding)
    good = case.members[0]
    words = np.frombuffer(good["proof"], dtype=np.uint32)
    felt = int(np.nonzero(case.classes == M.FELT)[0][10])  # a field word inside the first query

    def with_word(field, i, val):
        m = dict(good)
        if field == "proof":
            t = words.copy()
            t[i] = val
            m["proof"] = t.tobytes()
        else:
            t = good[field].copy()
            t.reshape(-1)[i] = val
            m[field] = t
        return m

    bad = [with_word("proof", felt, P), with_word("proof", felt, 0xFFFFFFFF), with_word("proof", len(words) - 1, P),
           with_word("opened", 5, P), with_word("opened", 5, 0xFFFFFFFF), with_word("points", 2, P), with_word("points", 2, 0xFFFFFFFF)]
    # a point on the LDE coset GENERATOR * <g_big>: GENERATOR itself
    m = dict(good)
    m["points"] = good["points"].copy()
    m["points"][1] = R.ext_from_base(R.GEN)
    bad.append(m)
    for off, val in ([(32, 8), (33, 9)] if kind == 0 else [(84, 136), (85, 33), (84, 0xFFFFFFF0)]):  # a state counter out of range
        bad.append(with_word("state", off, val))
    bad += [dict(good, proof=good["proof"][:-4]), dict(good, proof=good["proof"] + b"\0\0\0\0")]  # one word short, one word long
    batch = []
    for m in bad:
        assert case.expected(m)[0] == M.MALFORMED
        batch += [good, m]
    batch.append(good)
    v = case.verifier(len(batch))
    for pad in (0, 8):
        st, rej, _ = dev_entry(case, v, batch, True, pad)
        assert list(st) == [0, M.MALFORMED] * len(bad) + [0], st
        assert rej == len(bad)
    v.close()


# ---- 5. forms and bounds ----------------------------------------------------------------------------------------------------------
def _one_matrix(p3, hash, hiding, w, seed, log_h=2, fp=(1, 0, 2, 0), slots=None, widths=None, n=2, **kw):
    case = Case(p3, hash, hiding, log_h, fp, widths or [[w]], slots or [[[0]]], n, seed, **kw)
    v = case.verifier(n)
    good, tampered = case.members[0], dict(case.members[1])
    t = np.frombuffer(tampered["proof"], dtype=np.uint32).copy()
    i = int(np.nonzero(case.classes == M.FELT)[0][-6])  # a field word near the end of the proof
    t[i] = M.tampered(t[i])
    tampered["proof"] = t.tobytes()
    want = case.expected(tampered)[0]
    assert want in M.EQUALITY_CODES
    st, rej, _ = dev_entry(case, v, [good, tampered])
    assert list(st) == [0, want], (st, want)
    return case, v


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129, 255, 256, 257])
def test_columns_on_both_sides_of_the_form_switch(p3, oracle, w):
    """one matrix at one point: the batched columns are the row words; the switch is at pcs.WAVE_FORM_MIN_COLUMNS"""
    assert p3.pcs.WAVE_FORM_MIN_COLUMNS == 256
    for hash, hiding in (("poseidon2", False), ("keccak", True)):
        nrc = 2 if hiding else 0  # the random columns are batched columns too
        if w <= nrc:
            continue
        case, v = _one_matrix(p3, hash, hiding, w - nrc, 7000 + w, nrc=2)
        assert v.total == w and v.wave_form == (w >= 256)
        v.close()


def test_8192_batched_columns_and_the_8193rd(p3, oracle):
    slots = [[[0, 1, 2, 3]]]
    case, v = _one_matrix(p3, "poseidon2", False, 2048, 7100, slots=slots)
    assert v.total == 8192 and v.wave_form
    v.close()
    with pytest.raises(p3.P3HipError, match="round 0 matrix 1 point 0: more than 8192 batched columns"):
        p3.PcsVerifier(2, [[(2048, [0, 1, 2, 3]), (1, [0])]], 4, case.params, "poseidon2", False, 1)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_four_rounds_of_eight_matrices(p3, oracle, hash, kind):
    widths = [[1 + (3 * r + m) % 7 for m in range(8)] for r in range(4)]
    slots = [[[(r + m) % 4] * (1 + (m == 0)) if (r + m) % 3 else [] for m in range(8)] for r in range(4)]
    slots[0][0] = [0, 1, 2, 3]
    _one_matrix(p3, hash, False, 0, 7200 + kind, log_h=3, fp=(2, 1, 3, 2), widths=widths, slots=slots)[1].close()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_four_hiding_matrices_a_repeated_slot_and_equal_slot_values(p3, oracle, hash, kind):
    widths, slots = [[3, 1, 5, 2], [4]], [[[0, 0], [1], [], [2, 0]], [[1, 2]]]
    case, v = _one_matrix(p3, hash, True, 0, 7300 + kind, log_h=3, fp=(1, 1, 2, 1), widths=widths, slots=slots, nrc=3)
    v.close()
    # two slots holding one value: the host form repeats the point, which its distinct-points rule counts once
    case = Case(p3, hash, False, 3, (1, 0, 2, 0), [[2, 3]], [[[0, 1], [1]]], 1, 7310 + kind)
    v = case.verifier(1)
    pcs = p3.TwoAdicFriPcs(case.params, hash)
    rng = np.random.default_rng(7320)
    z = R.rand_point(rng)
    root, data = pcs.commit([(R.rand_matrix(rng, 3, 2), None), (R.rand_matrix(rng, 3, 3), None)])
    ch = M.prefix(p3.Challenger(hash), 1)
    state = ch.export_state()
    opened, proof = pcs.open([(data, [[z, z], [z]])], ch)
    m = dict(proof=proof, roots=root[None, :], points=np.stack([z, z]), opened=opened, state=state)
    assert case.expected(m) == (0, True)
    assert list(dev_entry(case, v, [m])[0]) == [0]
    v.close()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_log_h_1_with_one_fri_round_and_blowup_3(p3, oracle, hash, kind):
    _one_matrix(p3, hash, False, 5, 7400 + kind, log_h=1, fp=(1, 0, 3, 0))[1].close()
    _one_matrix(p3, hash, False, 5, 7410 + kind, log_h=3, fp=(3, 0, 2, 1), base_point=True)[1].close()
    _one_matrix(p3, hash, True, 5, 7420 + kind, log_h=2, fp=(3, 1, 2, 0))[1].close()


# ---- 6. batch mechanics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", HASHES)
def test_batch_mechanics(p3, oracle, hash, kind):
    import torch
    case = Case(p3, hash, kind == 1, 3, (1, 0, 3, 2), [[2, 5], [3]], [[[0, 1], [0]], [[1]]], 5, 8000 + kind)
    members, want = [], []
    for j in range(11):  # accepted and rejected members interleaved
        m = dict(case.members[j % 5])
        if j % 3 == 1:
            t = np.frombuffer(m["proof"], dtype=np.uint32).copy()
            i = int(np.nonzero(case.classes != M.SHAPE)[0][(37 * j) % int((case.classes != M.SHAPE).sum())])
            t[i] = M.tampered(t[i])
            m["proof"] = t.tobytes()
        members.append(m)
        want.append(case.expected(m)[0])
    assert want.count(0) == 7 and len(set(want)) > 1
    v = case.verifier(11)
    st, rej, _ = dev_entry(case, v, members)  # n = max_proofs
    assert list(st) == want and rej == 4
    st, rej, _ = dev_entry(case, v, members[1:2])  # n = 1, a rejected member; back to back on one verifier
    assert list(st) == want[1:2] and rej == 1
    st, rej, _ = dev_entry(case, v, members[:1])
    assert list(st) == [0] and rej == 0
    v.close()
    v = case.verifier(4)
    with pytest.raises(p3.P3HipError, match="more proofs than the verifier was created for"):
        dev_entry(case, v, members[:5])
    st, chals = host_entry(case, v, members)  # split into rounds of 4 by the host entry
    assert list(st) == want
    for m, ch, w in zip(members, chals, want):  # accepted: advanced; rejected: unchanged
        other = m["after"].clone() if w == 0 else p3.Challenger(hash)
        if w:
            other.import_state(m["state"])
        assert same_transcript(ch, other)
    # batch-level arguments are refused before any launch
    n = 2
    buf = torch.zeros(n * v.proof_len + 8, dtype=torch.uint8, device="cuda")
    args = [p3.dev_u32(np.stack([m[k] for m in members[:n]])) for k in ("roots", "points", "opened", "state")]
    with pytest.raises(p3.P3HipError, match="stride"):
        v.verify_many_dev(buf, *args, n=n, stride=v.proof_len - 4)
    with pytest.raises(p3.P3HipError, match="stride"):
        v.verify_many_dev(buf, *args, n=n, stride=v.proof_len + 2)
    with pytest.raises(p3.P3HipError, match="aligned"):
        v.verify_many_dev(buf[1:], *args, n=n, stride=v.proof_len)
    state4 = torch.zeros(n * p3.pcs.STATE_WORDS + 1, dtype=torch.int32, device="cuda")[1:]
    with pytest.raises(p3.P3HipError, match="8-byte aligned"):
        v.verify_many_dev(buf, args[0], args[1], args[2], state4, n=n, stride=v.proof_len)
    v.close()


# ---- 7. lifetime ------------------------------------------------------------------------------------------------------------------
def test_create_verify_destroy_cycles_return_their_memory(p3, oracle):
    import psutil
    import torch
    case = _shape_ab(p3, "poseidon2", False)
    kcase = _shape_ab(p3, "keccak", True)

    def cycle():
        for c in (case, kcase):
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
