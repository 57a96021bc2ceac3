"""CPU tests of the mixed-height TwoAdicFriPcs: the reference prover and verifier of tests/pcs_mixed_ref.py, and through them the
library's host verifier p3hip_pcs_verify_mixed (p3.pcs.verify with per-matrix log heights).

(a) with all heights equal the reference prover gives pcs_ref.open's bytes (itself pinned to the oracle's fib_air proofs), and
    p3hip_pcs_verify_mixed returns what p3hip_pcs_verify returns, on accepted and tampered proofs;
(b) the low-degree test at EVERY point of the final domain on the three shapes of the design's table: the beta^2 roll-in, the
    per-class alpha counters and the class at log_final_poly_len are consistent;
(c) the library's verifier and the Python verifier accept the reference prover's proofs on those shapes and on seeded mixed
    shapes, leave the prover's transcript, and reject with EQUAL codes one perturbed word of every proof section, of the opened
    values and of a root;
(d) the refusals, by message."""
import numpy as np
import pytest

import pcs_mixed_ref as M
import pcs_ref as R

P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
PREFIX = np.arange(1, 6, dtype=np.uint32)  # some transcript before the open


def _lib_code(p3, t, hash, vr, log_h, opened, fri):
    """log_h: an int (p3hip_pcs_verify) or per-matrix lists (p3hip_pcs_verify_mixed)"""
    ch = p3.Challenger(hash)
    ch.observe(PREFIX)
    try:
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, ch)
    except p3.PcsRejected as e:
        return e.code, ch
    return 0, ch


def _ref_code(kind, t, lhs, vr, opened, fri):
    ch = R.RefChallenger(kind)
    ch.observe(PREFIX)
    return M.verify(kind, t, lhs, vr, opened, fri, ch), ch


def _prove(kind, t, rounds):
    pch = R.RefChallenger(kind)
    pch.observe(PREFIX)
    d = M.prove(kind, t, rounds, pch)
    vr, lhs = M.verifier_rounds(d["roots"], rounds)
    return d, vr, lhs, pch


def _tampers(rng, t, vr, opened, fri):
    """(name, rounds, opened, proof): one perturbed word of the opened values, of an input root, of every proof section"""
    bump = lambda v: (int(v) + 1) % P
    out = []
    bad = opened.copy().reshape(-1)
    pos = int(rng.integers(0, bad.size))
    bad[pos] = bump(bad[pos])
    out.append(("opened %d" % pos, vr, bad.reshape(-1, 4), fri))
    r = int(rng.integers(0, len(vr)))
    root = vr[r][0][0].copy()
    root[int(rng.integers(0, 8))] ^= 1
    out.append(("root of round %d" % r, [((root, ws), mp) if i == r else ((rt, ws), mp) for i, ((rt, ws), mp) in enumerate(vr)], opened, fri))
    words = np.frombuffer(fri, dtype=np.uint32)
    n_fr, fpl = int(words[0]), 1 << t[1]
    q0, q1 = 2 + 8 * n_fr, len(words) - 2 - 4 * fpl  # commit-phase roots | queries | final polynomial | witness
    for name, (lo, hi) in {"roots": (1, 1 + 8 * n_fr), "queries": (q0, q1), "final polynomial": (q1 + 1, len(words) - 1),
                           "witness": (len(words) - 1, len(words))}.items():
        assert hi > lo, name
        pos = int(rng.integers(lo, hi))
        b = words.copy()
        b[pos] = bump(b[pos])
        out.append(("%s %d" % (name, pos), vr, opened, b.tobytes()))
    return out


def _prove_and_verify(p3, rng, hash, kind, t, rounds, perturb=True):
    d, vr, lhs, pch = _prove(kind, t, rounds)
    opened, fri = d["opened"], d["proof"]
    assert M.final_vector_is_the_final_polynomial(t, d)
    code, lch = _lib_code(p3, t, hash, vr, lhs, opened, fri)
    assert code == 0
    code, rch = _ref_code(kind, t, lhs, vr, opened, fri)
    assert code == 0
    want = pch.sample_ext()  # prover and both verifiers stand after the last query index
    assert np.array_equal(lch.sample_ext(), want) and np.array_equal(rch.sample_ext(), want)
    for name, v, o, f in _tampers(rng, t, vr, opened, fri) if perturb else []:
        lib, ref = _lib_code(p3, t, hash, v, lhs, o, f)[0], _ref_code(kind, t, lhs, v, o, f)[0]
        assert lib != 0 and lib == ref, (name, lib, ref)


def _queries(t, log_h_max):
    """as many queries as 20 bits of indices take (tests/test_pcs_ref_host.py _fri: a perturbed word that moves the transcript is
    rejected because the indices move with it)"""
    return (t[0], t[1], max(t[2], -(-20 // (log_h_max + t[0]))), t[3])


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_h", range(1, 7))
def test_equal_heights_give_the_same_height_bytes_and_codes(p3, oracle, hash, kind, log_h):
    """pcs_mixed_ref.open == pcs_ref.open byte for byte, two parameter sets; p3hip_pcs_verify_mixed == p3hip_pcs_verify on the
    accepted proof and on every tamper"""
    for i, t in enumerate([(1, 0, 3, 2), (2, min(1, log_h - 1), 2, 0)]):
        rng = np.random.default_rng(100 * log_h + 10 * kind + i)
        rounds = R.random_case(rng, log_h, 200)
        a, b = R.RefChallenger(kind), R.RefChallenger(kind)
        o1, p1 = R.open(kind, t, log_h, rounds, a)
        o2, p2 = M.open(kind, t, rounds, b)
        assert np.array_equal(o1, o2) and p1 == p2
        assert np.array_equal(a.sample_ext(), b.sample_ext())
        t = _queries(t, log_h)
        d, vr, lhs, _ = _prove(kind, t, rounds)
        assert lhs == [[log_h] * len(mats) for mats in rounds]
        for name, v, o, f in [("accepted", vr, d["opened"], d["proof"])] + _tampers(rng, t, vr, d["opened"], d["proof"]):
            (c1, ch1), (c2, ch2) = _lib_code(p3, t, hash, v, log_h, o, f), _lib_code(p3, t, hash, v, lhs, o, f)
            assert c1 == c2 and (c1 == 0) == (name == "accepted"), (name, c1, c2)
            assert np.array_equal(ch1.sample_ext(), ch2.sample_ext()), name


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("case", range(3))
def test_table_shapes_are_low_degree_and_accepted(p3, oracle, hash, kind, case):
    t, log_hs = M.TABLE[case]
    rng = np.random.default_rng(70 + case)
    rounds = M.table_case(rng, log_hs)
    d, vr, lhs, _ = _prove(kind, t, rounds)  # the table's own parameters: every point of the final domain
    assert lhs == log_hs and M.final_vector_is_the_final_polynomial(t, d)
    assert _lib_code(p3, t, hash, vr, lhs, d["opened"], d["proof"])[0] == 0
    _prove_and_verify(p3, rng, hash, kind, _queries(t, max(max(r) for r in log_hs)), rounds)


def test_seeded_mixed_shapes(p3, oracle):
    """eight seeded shapes: log_h 1..7, up to 4 rounds, widths 1..129, 0..4 points per matrix, classes repeated across rounds"""
    seen = set()
    for seed in range(8):
        rng = np.random.default_rng(9000 + seed)
        hash, kind = HASHES[seed % 2]
        rounds = M.random_mixed_case(rng)
        lhs = [M._log2(m.shape[0]) for mats in rounds for m, _, _ in mats]
        lfp = int(rng.integers(0, min(min(lhs), max(lhs) - 1, 3) + 1))
        t = _queries((int(rng.integers(1, 4)), lfp, int(rng.integers(1, 5)), int(rng.integers(0, 5))), max(lhs))
        _prove_and_verify(p3, rng, hash, kind, t, rounds)
        # what the generator reached
        seen.add("mixed" if len(set(lhs)) > 1 else "equal")
        seen.add("rounds%d" % len(rounds))
        per_round = [{m.shape[0] for m, _, _ in mats} for mats in rounds]
        if any(a & b for i, a in enumerate(per_round) for b in per_round[i + 1:]):
            seen.add("class across rounds")
        if any(max(r) < (1 << max(lhs)) for r in per_round):
            seen.add("short round")
        if any(not pts for mats in rounds for _, _, pts in mats):
            seen.add("np0")
        if any(m.shape[1] >= 63 and pts for mats in rounds for m, _, pts in mats):
            seen.add("wide")
    # (a class AT log_final_poly_len is the table's second shape)
    assert {"mixed", "rounds4", "class across rounds", "short round", "np0", "wide"} <= seen, seen


def test_refusals_by_message(p3, oracle):
    rng = np.random.default_rng(11)
    z = R.rand_point(rng)
    root = np.zeros(8, dtype=np.uint32)

    def refused(t, lhs, vr, match):
        ch = p3.Challenger()
        n = sum(w * len(pts) for (_, ws), mp in vr for w, pts in zip(ws, mp))
        with pytest.raises(p3.P3HipError, match=match) as e:
            p3.pcs.verify(p3.FriParameters(*t), "poseidon2", vr, lhs, np.zeros((n, 4), dtype=np.uint32), b"\0" * 64, ch)
        assert e.value.code == -1 and not isinstance(e.value, p3.PcsRejected)
        assert np.array_equal(ch.sample_ext(), p3.Challenger().sample_ext())  # the challenger is unchanged

    # the tallest class has no opening point
    refused((1, 0, 2, 0), [[3, 2]], [((root, [2, 2]), [[], [z]])], "no matrix of the tallest height 2\\^3 has an opening point")
    with pytest.raises(M.Refused, match="tallest"):
        M.check_shape((1, 0, 2, 0), [[3, 2]], [[0, 1]])
    # a class below log_final_poly_len
    refused((1, 2, 2, 0), [[4], [1]], [((root, [2]), [[z]]), ((root, [3]), [[z]])], "round 1 matrix 0 has height 2\\^1, below the final polynomial's 2\\^2")
    with pytest.raises(M.Refused, match="below the final polynomial"):
        M.check_shape((1, 2, 2, 0), [[4], [1]], [[1], [1]])
    # a point on the TALLEST LDE coset, asked of a shorter matrix: GENERATOR g_16^3 is on GENERATOR <g_16> and not on GENERATOR <g_4>
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(4), 3)))
    refused((1, 0, 2, 0), [[3, 1]], [((root, [2, 2]), [[z], [z, on]])], "round 0 matrix 1 point 1 lies on the LDE coset")
    # the capacities, with the tallest height
    refused((1, 0, 2, 0), [[3, 1]] * 5, [((root, [2, 2]), [[z], [z]])] * 5, "5 rounds, at most 4")
    refused((1, 0, 2, 0), [[3] * 9], [((root, [1] * 9), [[z]] * 9)], "round 0 has more than 8 matrices")
    refused((1, 0, 2, 0), [[3, 0]], [((root, [2, 2]), [[z], [z]])], "LDE height outside")
    refused((2, 0, 2, 0), [[26, 3]], [((root, [2, 2]), [[z], [z]])], "LDE height outside")
    refused((1, 3, 2, 0), [[3, 3]], [((root, [2, 2]), [[z], [z]])], "log_final_poly_len must be below")
    pts = [R.ext_from_base(int(R.O.to_monty(k))) for k in range(2, 7)]
    refused((1, 0, 2, 0), [[3, 1]], [((root, [2, 2]), [pts[:3], pts[3:]])], "more than 4 distinct opening points")
    refused((1, 0, 2, 0), [[3, 1]], [((root, [8000, 200]), [[z], [z]])], "more than 8192 batched columns")
    with pytest.raises(ValueError, match="one log height per matrix"):
        p3.pcs.verify(p3.FriParameters(1, 0, 2, 0), "poseidon2", [((root, [2, 2]), [[z], [z]])], [[3]], np.zeros((4, 4), np.uint32), b"", p3.Challenger())
    with pytest.raises(ValueError, match="a hiding PCS takes one log height"):
        p3.pcs.verify(p3.FriParameters(1, 0, 2, 0), "poseidon2", [((root, [2]), [[z]])], [[3]], np.zeros((2, 4), np.uint32), b"", p3.Challenger(), hiding=True)
