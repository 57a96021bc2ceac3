"""CPU tests of the PCS's host half: the C challengers and p3hip_pcs_verify against the oracle's fib_air proofs
(oracle/stark.c), taken apart into roots, opened values and the FriProof section, with the uni-stark prefix of the transcript
replayed through Challenger.  Reject codes: include/p3hip.h p3hip_pcs_verify."""
import numpy as np
import pytest

import pcs_ref as R

HASHES = [("poseidon2", 0), ("keccak", 1)]
# (log_blowup, log_final_poly_len, num_queries, proof_of_work_bits); a set applies where log_final_poly_len < log_n
FRI_SETS = [(1, 0, 3, 2), (2, 0, 4, 4), (2, 1, 2, 1), (1, 2, 5, 0), (3, 1, 2, 3), (1, 0, 10, 8), (1, 3, 2, 5)]
DOCUMENTED = {5, 6, 7, 8, 9, 11, 12, 13, 14, 15}
FIRST_ROWS = [(0, 1), (7, 11), (R.P - 1, 1)]


def _sets(log_n):
    return [t for t in FRI_SETS if t[1] < log_n]


_proofs = {}


def _instance(oracle, kind, log_n, t):
    """the oracle's proof of one instance, split, computed once"""
    key = (kind, log_n, t)
    if key not in _proofs:
        a, b = FIRST_ROWS[(log_n + kind) % 3]
        proof = oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind)
        assert oracle.verify_fib_air(proof, a, b, oracle.fib_public_x(a, b, 1 << log_n), log_n, oracle.FriParams(*t), hash=kind) == 0
        _proofs[key] = (R.fib_pis(a, b, log_n),) + R.split_fib_proof(proof)
    return _proofs[key]


def _rounds(root_t, root_q, zeta, zeta_next):
    return [((root_t, [2]), [[zeta, zeta_next]]), ((root_q, [4]), [[zeta]])]


def _prefix(p3, hash, log_n, pis, root_t, root_q):
    ch = p3.Challenger(hash)
    _, zeta, zeta_next = R.fib_prefix(ch, log_n, root_t, pis, root_q)
    return ch, zeta, zeta_next


def _code(p3, t, hash, rounds, log_h, opened, fri, ch):
    """0 on accept, the reject code otherwise; the challenger is a clone, the caller's stays"""
    c = ch.clone()
    try:
        p3.pcs.verify(p3.FriParameters(*t), hash, rounds, log_h, opened, fri, c)
    except p3.PcsRejected as e:
        assert e.code in DOCUMENTED and e.message.startswith("pcs verification failed: "), (e.code, e.message)
        return e.code
    return 0


def test_numpy_extension_product_matches_the_oracle():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, R.P, (64, 4), dtype=np.uint64), rng.integers(0, R.P, (64, 4), dtype=np.uint64)
    got = R.O.to_monty(R._canon_ext_mul(a, b))
    for i in range(64):
        assert np.array_equal(got[i], R.ext_mul(R.O.to_monty(a[i]), R.O.to_monty(b[i])))


@pytest.mark.parametrize("hash,kind", HASHES)
def test_challenger_equals_the_python_restatement(p3, oracle, hash, kind):
    rng = np.random.default_rng(11 + kind)
    ch, ref = p3.Challenger(hash), R.RefChallenger(kind)
    for step in range(60):
        n = int(rng.integers(1, 40))
        w = oracle.to_monty(rng.integers(0, R.P, n, dtype=np.uint64))
        ch.observe(w)
        ref.observe(w)
        if step % 3 == 0:
            d = rng.integers(0, R.P if kind == 0 else 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
            ch.observe_digest(d)
            ref.observe_digest(d)
        for _ in range(int(rng.integers(0, 4))):
            assert np.array_equal(ch.sample_ext(), ref.sample_ext())
        if step % 4 == 1:
            bits = int(rng.integers(0, 31))
            assert ch.sample_bits(bits) == ref.sample_bits(bits)
    c2 = ch.clone()
    assert np.array_equal(c2.sample_ext(), ch.sample_ext())
    with pytest.raises(p3.P3HipError, match="not a canonical field element"):
        ch.observe([R.P])
    with pytest.raises(p3.P3HipError, match="at most 30 bits"):
        ch.sample_bits(31)
    with pytest.raises(ValueError):
        p3.Challenger("sha2")


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_n", range(1, 11))
def test_verify_accepts_and_leaves_the_transcript_of_the_restatement(p3, oracle, hash, kind, log_n):
    for t in _sets(log_n):
        pis, ln, root_t, root_q, opened, fri = _instance(oracle, kind, log_n, t)
        assert ln == log_n
        ch, zeta, zeta_next = _prefix(p3, hash, log_n, pis, root_t, root_q)
        rounds = _rounds(root_t, root_q, zeta, zeta_next)
        p3.pcs.verify(p3.FriParameters(*t), hash, rounds, log_n, opened, fri, ch)  # accepts, advances ch
        ref = R.RefChallenger(kind)
        _, z2, _ = R.fib_prefix(ref, log_n, root_t, pis, root_q)
        assert np.array_equal(z2, zeta)
        assert R.verify(kind, t, log_n, rounds, opened, fri, ref) == 0
        for _ in range(3):  # the two transcripts stand at the same place: after the last query index
            assert np.array_equal(ch.sample_ext(), ref.sample_ext())
        assert ch.sample_bits(13) == ref.sample_bits(13)


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_n", range(1, 11))
def test_verify_rejects_every_tampering_with_its_documented_code(p3, oracle, hash, kind, log_n):
    sets = _sets(log_n)
    t = sets[(log_n + kind) % len(sets)]
    pis, _, root_t, root_q, opened, fri = _instance(oracle, kind, log_n, t)
    ch, zeta, zeta_next = _prefix(p3, hash, log_n, pis, root_t, root_q)
    rounds = _rounds(root_t, root_q, zeta, zeta_next)
    assert _code(p3, t, hash, rounds, log_n, opened, fri, ch) == 0
    rng = np.random.default_rng(100 * log_n + kind)
    bump = lambda v: (int(v) + 1) % R.P
    # every single-word perturbation of the opened values: the transcript moves (witness, indices), or the reduced opening does
    flat = opened.reshape(-1)
    for pos in range(flat.size):
        bad = flat.copy()
        bad[pos] = bump(bad[pos])
        assert _code(p3, t, hash, rounds, log_n, bad, fri, ch) in {11, 13, 14, 15}, pos
    # ... and of the FriProof section: all words up to log_n 4, a seeded sample of 200 above
    words = np.frombuffer(fri, dtype=np.uint32)
    where = range(len(words)) if log_n <= 4 else rng.choice(len(words), size=min(200, len(words)), replace=False)
    for pos in where:
        bad = words.copy()
        bad[pos] = bump(bad[pos])
        assert _code(p3, t, hash, rounds, log_n, opened, bad.tobytes(), ch) != 0, pos
    # every truncation (every byte length up to log_n 4, every word boundary above), and trailing bytes
    for cut in range(0, len(fri), 1 if log_n <= 4 else 4):
        assert _code(p3, t, hash, rounds, log_n, opened, fri[:cut], ch) in {5, 6, 7, 8, 9}, cut
    assert _code(p3, t, hash, rounds, log_n, opened, fri + b"\0\0\0\0", ch) == 8
    # a wrong root: the input opening fails
    for which in (0, 1):
        r = [root_t.copy(), root_q.copy()]
        r[which][int(rng.integers(0, 8))] ^= 1
        assert _code(p3, t, hash, _rounds(r[0], r[1], zeta, zeta_next), log_n, opened, fri, ch) == 13
    # a wrong point: the points are not part of the PCS transcript, so the reduced opening is what differs
    zb = zeta.copy()
    zb[2] = bump(zb[2])
    assert _code(p3, t, hash, _rounds(root_t, root_q, zb, zeta_next), log_n, opened, fri, ch) in {14, 15}
    assert _code(p3, t, hash, _rounds(root_t, root_q, zeta, zeta), log_n, opened, fri, ch) in {14, 15}
    # swapped rounds (with their opened values): the observation order, hence everything after it, differs
    swapped = [rounds[1], rounds[0]]
    assert _code(p3, t, hash, swapped, log_n, np.concatenate([opened[4:], opened[:4]]), fri, ch) in {11, 12, 13}
    # the other hash configuration's verifier
    other = "keccak" if hash == "poseidon2" else "poseidon2"
    assert _code(p3, t, other, rounds, log_n, opened, fri, p3.Challenger(other)) != 0
    # wrong parameters
    assert _code(p3, (t[0], t[1], t[2] + 1, t[3]), hash, rounds, log_n, opened, fri, ch) == 6
    assert _code(p3, t, hash, rounds, log_n + 1, opened, fri, ch) == 5


def test_argument_gates_name_the_offender(p3, oracle):
    t, log_n = (1, 0, 3, 2), 3
    pis, _, root_t, root_q, opened, fri = _instance(oracle, 0, log_n, t)
    ch, zeta, zeta_next = _prefix(p3, "poseidon2", log_n, pis, root_t, root_q)
    fp = p3.FriParameters(*t)

    def refused(match, rounds, op=opened, params=fp, log_h=log_n):
        c = ch.clone()
        with pytest.raises(p3.P3HipError, match=match) as e:
            p3.pcs.verify(params, "poseidon2", rounds, log_h, op, fri, c)
        assert e.value.code == -1 and not isinstance(e.value, p3.PcsRejected)
        assert np.array_equal(c.sample_ext(), ch.clone().sample_ext())  # a refused call leaves the transcript alone

    # a point on the LDE coset GENERATOR * <g_big>: base-field, (z / GENERATOR)^big = 1
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_n + 1), 5)))
    refused("round 0 matrix 0 point 1 lies on the LDE coset", _rounds(root_t, root_q, zeta, on))
    refused("round 1 matrix 0 point 0 lies on the LDE coset", [((root_t, [2]), [[zeta, zeta_next]]), ((root_q, [4]), [[on]])])
    off = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_n + 2), 5)))  # on the next finer coset only: fine
    assert _code(p3, t, "poseidon2", _rounds(root_t, root_q, off, zeta_next), log_n, opened, fri, ch) != 0
    # zero matrices, zero rounds, no point at all
    refused("round 1 has zero matrices", [((root_t, [2]), [[zeta, zeta_next]]), ((root_q, []), [])], op=opened[:4])
    refused("zero rounds", [], op=np.zeros((0, 4), np.uint32))
    refused("no opening point", [((root_t, [2]), [[]])], op=np.zeros((0, 4), np.uint32))
    # capacities
    refused("round 0 has more than 8 matrices", [((root_t, [1] * 9), [[zeta]] * 9)], op=np.zeros((9, 4), np.uint32))
    refused("5 rounds, at most 4", [((root_t, [1]), [[zeta]])] * 5, op=np.zeros((5, 4), np.uint32))
    pts = [R.ext_from_base(int(oracle.to_monty(k))) for k in range(2, 7)]
    refused("round 0 matrix 0: more than 4 opening points", [((root_t, [1]), [pts])], op=np.zeros((5, 4), np.uint32))
    refused("round 1 matrix 0 point 0: more than 4 distinct opening points",
            [((root_t, [1]), [pts[:4]]), ((root_q, [1]), [pts[4:]])], op=np.zeros((5, 4), np.uint32))
    refused("round 0 matrix 1 point 0: more than 8192 batched columns", [((root_t, [8000, 193]), [[zeta], [zeta]])],
            op=np.zeros((8193, 4), np.uint32))
    refused(r"round 0 matrix 0: width must be in \[1, 8192\]", [((root_t, [0]), [[zeta]])], op=np.zeros((0, 4), np.uint32))
    # values that are no field elements, FRI parameters outside the prover's gates
    refused("round 0 matrix 0 point 0 is not a canonical field element", _rounds(root_t, root_q, np.array([R.P, 0, 0, 0], np.uint32), zeta_next))
    bad = opened.copy()
    bad[3, 1] = R.P
    refused("opened value word 13 is not a canonical", _rounds(root_t, root_q, zeta, zeta_next), op=bad)
    rounds = _rounds(root_t, root_q, zeta, zeta_next)
    refused("log_final_poly_len must be below", rounds, params=p3.FriParameters(1, 3, 3, 2))
    refused("num_queries must be positive", rounds, params=p3.FriParameters(1, 0, 0, 2))
    refused("proof_of_work_bits too large", rounds, params=p3.FriParameters(1, 0, 3, 31))
    refused("LDE height outside", rounds, params=p3.FriParameters(0, 0, 3, 2))
    refused("LDE height outside", rounds, log_h=0)
    with pytest.raises(p3.P3HipError, match="another hash configuration"):
        p3.pcs.verify(fp, "keccak", rounds, log_n, opened, fri, ch.clone())
