"""CPU tests of the device PCS batch verifier's host half: p3hip_pcs_proof_len against the reference provers' proofs and the host
verifiers' gates, the challenger state's export / import, and the share of tampered members the code-equality clause covers, measured
with the host verifier alone on the two shapes the GPU tests tamper word by word."""
import numpy as np
import pytest

import pcs_hiding_ref as H
import pcs_many as M
import pcs_ref as R

HASHES = M.HASHES


def _plain_len_case(p3, hash, kind, log_h, rounds, fp):
    opened, proof = R.open(kind, fp, log_h, rounds, M.prefix(R.RefChallenger(kind), log_h))
    _, slots = M.slots_of([[pts for _, _, pts in mats] for mats in rounds])
    widths = [[m.shape[1] for m, _, _ in mats] for mats in rounds]
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    got = p3.pcs_proof_len(p3.FriParameters(*fp), hash, log_h, M.verifier_shape(widths, slots), n_slots)
    assert got == len(proof), (hash, log_h, fp, got, len(proof))
    assert len(M.word_classes(kind, fp, log_h, widths, 0)) * 4 == got


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_h", range(1, 8))
def test_proof_len_equals_the_reference_provers_plain(p3, oracle, hash, kind, log_h):
    rng = np.random.default_rng(100 + 2 * log_h + kind)
    fp = (int(rng.integers(1, 3)), int(rng.integers(0, log_h)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    _plain_len_case(p3, hash, kind, log_h, R.random_case(rng, log_h, max_cols=200), fp)
    # a matrix without points and a whole round without points
    _plain_len_case(p3, hash, kind, log_h, R.empty_point_case(rng, log_h), (1, 0, 2, 0))


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_h", range(1, 8))
def test_proof_len_equals_the_reference_provers_hiding(p3, oracle, hash, kind, log_h):
    rng = np.random.default_rng(200 + 2 * log_h + kind)
    fp = (int(rng.integers(1, 3)), int(rng.integers(0, log_h + 1)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    pcs = H.HidingPcs(kind, fp, (1, 3, 4)[log_h % 3], mmcs_seed=log_h, pcs_seed=7 + kind)
    _, rounds = H.random_rounds(rng, pcs, log_h, (1, 2, 17), max_rounds=3, max_mats=3, randomization=log_h % 2 == 1, max_cols=200)
    if len(rounds) > 1:  # a whole round without points, unless it held the only one
        keep = [mp for _, mp in rounds]
        if any(p for mp in keep[1:] for p in mp):
            rounds[0] = (rounds[0][0], [[] for _ in rounds[0][1]])
    opened, proof = pcs.open(rounds, M.prefix(R.RefChallenger(kind), log_h))
    _, slots = M.slots_of([mp for _, mp in rounds])
    widths = [com.widths for com, _ in rounds]
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    got = p3.pcs_proof_len(p3.FriParameters(*fp), hash, log_h, M.verifier_shape(widths, slots), n_slots, hiding=True)
    assert got == len(proof), (hash, log_h, fp, got, len(proof))
    assert len(M.word_classes(kind, fp, log_h + 1, widths, 4)) * 4 == got


def test_proof_len_refuses_what_the_host_verifiers_refuse(p3, oracle):
    """each refusal once through the host verifier and once through proof_len: the same message"""
    fp = p3.FriParameters
    ok = fp(1, 0, 2, 0)
    z = R.rand_point(np.random.default_rng(1))
    root = np.zeros(8, dtype=np.uint32)
    # (params, log_h, widths per round, points per matrix, hiding)
    cases = [(fp(0, 0, 2, 0), 3, [[2]], [[1]], False), (fp(1, 3, 2, 0), 3, [[2]], [[1]], False), (fp(1, 0, 2, 31), 3, [[2]], [[1]], False),
             (fp(1, 0, 0, 0), 3, [[2]], [[1]], False), (ok, 27, [[2]], [[1]], False), (ok, 3, [], [], False),
             (ok, 3, [[1]] * 5, [[1]] * 5, False), (ok, 3, [[]], [[]], False), (ok, 3, [[1] * 9], [[1] * 9], False),
             (ok, 3, [[1] * 5], [[1] * 5], True), (ok, 3, [[0]], [[1]], False), (ok, 3, [[8193]], [[1]], False),
             (ok, 3, [[2]], [[5]], False), (ok, 3, [[4096, 4096, 1]], [[1, 1, 1]], False), (ok, 3, [[2049]], [[4]], False),
             (ok, 3, [[2], [3]], [[0], [0]], False), (ok, 27, [[2]], [[1]], True), (fp(1, 3, 2, 0), 2, [[2]], [[1]], True),
             (ok, 0, [[2]], [[1]], True)]
    seen = set()
    for params, log_h, widths, counts, hiding in cases:
        vr = [((root, ws), [[z] * c for c in cs]) for ws, cs in zip(widths, counts)]
        total = sum(w * c for ws, cs in zip(widths, counts) for w, c in zip(ws, cs))
        with pytest.raises(p3.P3HipError) as host:
            p3.pcs.verify(params, "poseidon2", vr, log_h, np.zeros((total, 4), np.uint32), b"\0" * 8, p3.Challenger("poseidon2"), hiding=hiding)
        assert host.value.code == -1
        shape = [[(w, [0] * c) for w, c in zip(ws, cs)] for ws, cs in zip(widths, counts)]
        with pytest.raises(p3.P3HipError) as mine:
            p3.pcs_proof_len(params, "poseidon2", log_h, shape, 1, hiding=hiding)
        assert mine.value.code == -1 and mine.value.message == host.value.message, (mine.value.message, host.value.message)
        seen.add(mine.value.message)
    assert len(seen) >= 14, sorted(seen)  # the cases name different gates
    assert any("more than 8192 batched columns" in m for m in seen)
    # the slots are the batch verifier's own
    for n_slots, slot, what in ((0, 0, "n_slots"), (5, 0, "n_slots"), (2, 2, "slot 2 of 2")):
        with pytest.raises(p3.P3HipError, match=what):
            p3.pcs_proof_len(ok, "poseidon2", 3, [[(2, [slot])]], n_slots)


def _states(kind):
    """every pending state tests/test_gpu_pcs_states.py names, as (name, prepare)"""
    w = lambda n, seed=0: R.O.to_monty(np.arange(seed + 1, seed + n + 1, dtype=np.uint64) * 1000003 % M.P)
    out = []
    if kind == 0:
        for k in range(8):
            out.append(("%d pending, fresh" % k, lambda ch, k=k: ch.observe(w(k, k)) if k else None))
        for k in range(1, 8):
            out.append(("%d pending after a sample" % k, lambda ch, k=k: (ch.observe(w(3, 50)), ch.sample_ext(), ch.observe(w(k, k)))))
        for m in range(1, 8):
            out.append(("%d outputs left" % m, lambda ch, m=m: (ch.observe(w(11, 70)), [ch.sample_bits(20) for _ in range(8 - m)])))
        return out
    for n in (33, 34, 35, 67, 68, 69, 100):
        out.append(("%d words, fresh" % n, lambda ch, n=n: ch.observe(w(n, n))))
    for n in (25, 26, 27):  # behind the 32-byte chaining value: 132 / 136 / 140 bytes
        out.append(("%d words after a sample" % n, lambda ch, n=n: (ch.observe(w(4, 9)), ch.sample_ext(), ch.observe(w(n, n)))))
    for want in (4, 16, 28):
        for seed in range(200):  # rejection sampling may take more bytes: the first prefix that leaves exactly `want`
            ref = R.RefChallenger(1)
            ref.observe(w(5, seed))
            for _ in range((32 - want) // 4):
                ref.sample_bits(16)
            if len(ref.obuf) == want:
                break
        else:
            raise AssertionError(want)
        out.append(("%d output bytes left" % want, lambda ch, seed=seed, want=want: (ch.observe(w(5, seed)), [ch.sample_bits(16) for _ in range((32 - want) // 4)])))
    return out


@pytest.mark.parametrize("hash,kind", HASHES)
def test_challenger_export_then_import_is_the_identity(p3, oracle, hash, kind):
    for name, prepare in _states(kind):
        a, ref = p3.Challenger(hash), R.RefChallenger(kind)
        prepare(a)
        prepare(ref)
        words = a.export_state()
        assert words.shape == (p3.pcs.STATE_WORDS,) and words.dtype == np.uint32
        b = p3.Challenger(hash)
        b.observe([5, 6, 7])  # whatever it held is replaced
        b.import_state(words)
        assert np.array_equal(b.export_state(), words), name
        for c in (a, b):  # the source is not disturbed by the export
            r = ref.clone()
            assert np.array_equal(c.sample_ext(), r.sample_ext()), name
            assert c.sample_bits(17) == r.sample_bits(17), name
            w = R.O.to_monty(np.arange(1, 40, dtype=np.uint64))
            c.observe(w)
            r.observe(w)
            assert np.array_equal(c.sample_ext(), r.sample_ext()), name


@pytest.mark.parametrize("hash,kind", HASHES)
def test_challenger_import_refuses_counters_out_of_range(p3, oracle, hash, kind):
    ch = M.prefix(p3.Challenger(hash), 3)
    good = ch.export_state()
    # word offsets of the counters (include/p3hip.h p3hip_challenger_export): n_in, n_out; fill level, output bytes left
    bad = [(32, 8), (32, 0xFFFFFFFF), (33, 9), (33, 1 << 31)] if kind == 0 else [(84, 136), (84, 1 << 20), (85, 33), (85, 0xFFFFFFFF)]
    edge = [(32, 7), (33, 8)] if kind == 0 else [(84, 132), (85, 32)]
    for off, val in bad:
        w = good.copy()
        w[off] = val
        with pytest.raises(p3.P3HipError, match="challenger_import") as e:
            ch.import_state(w)
        assert e.value.code == -1
        assert np.array_equal(ch.export_state(), good)  # a refused import changes nothing
    for off, val in edge:  # the largest value each counter can hold is taken
        w = good.copy()
        w[off] = val
        p3.Challenger(hash).import_state(w)
    with pytest.raises(ValueError):
        ch.import_state(good[:-1])


def _share(p3, hash, kind, hiding):
    """tampers every proof word of shape A / B in turn; -> (members under the equality clause, members, structural words)"""
    rng = np.random.default_rng(900 + kind + 2 * hiding)
    fp, log_h = M.FP_AB, M.LOG_H_AB
    pts = np.stack([R.rand_point(rng) for _ in range(2)])
    mat_points = M.expand(pts, M.SLOTS_AB)
    evals = [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng)) for w in ws] for ws in M.WIDTHS_AB]
    ref = M.prefix(R.RefChallenger(kind), 5)
    if hiding:
        pcs = H.HidingPcs(kind, fp, M.NRC_B, 3, 4)
        rounds = [(pcs.commit(mats), mp) for mats, mp in zip(evals, mat_points)]
        opened, proof = pcs.open(rounds, ref)
        roots, widths = [com.root for com, _ in rounds], [com.widths for com, _ in rounds]
    else:
        rounds = [[(m, s, mp) for (m, s), mp in zip(mats, mps)] for mats, mps in zip(evals, mat_points)]
        opened, proof, roots = R.open_with_roots(kind, fp, log_h, rounds, ref)
        widths = M.WIDTHS_AB
    state = M.prefix(p3.Challenger(hash), 5).export_state()
    classes = M.word_classes(kind, fp, log_h + (1 if hiding else 0), widths, 4 if hiding else 0)
    words = np.frombuffer(proof, dtype=np.uint32)
    assert len(words) == len(classes)
    h, ch = M.host_code(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, proof, state)
    assert h == 0 and np.array_equal(ch.sample_ext(), ref.sample_ext())
    inside, codes = 0, set()
    for i in range(len(words)):
        t = words.copy()
        t[i] = M.tampered(t[i])
        h, _ = M.host_code(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, t.tobytes(), state)
        assert h != 0, i  # every word of a proof matters
        codes.add(h)
        inside += M.in_equality_clause(h, M.canonical(t, classes))
    return inside, len(words), int((classes == M.SHAPE).sum()), codes


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("hiding", [False, True])
def test_share_of_tampered_members_under_the_equality_clause(p3, oracle, hash, kind, hiding):
    """Shape A (plain) and B (hiding, one random codeword): 322 words of which 27 structural, 512 of which 43 (header 34, two queries of 236, tail 6)."""
    inside, n, structural, codes = _share(p3, hash, kind, hiding)
    print("shape %s %s: %d of %d members under the equality clause (%.3f), %d structural words, host codes %s"
          % ("B" if hiding else "A", hash, inside, n, inside / n, structural, sorted(codes)))
    assert (n, structural) == ((512, 43) if hiding else (322, 27))
    assert inside / n >= 0.90
    assert {13, 14} <= codes
