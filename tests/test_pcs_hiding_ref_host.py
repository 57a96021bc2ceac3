"""CPU tests of the reference prover of tests/pcs_hiding_ref.py (oracle/stark_hiding.c:94-295 restated for any shape) and, through it,
of the library's host verifier of hiding PCS proofs, p3hip_pcs_verify_hiding.

(a) hiding fib_air proofs assembled from the reference prover's commit / commit_quotient / commit_randomization / open equal
    oracle.prove_fib_air_hiding byte for byte: the pin of the draw order of the three streams, the blinding, the alpha ordering and the
    wire format, which lets the reference prover's bytes stand for the oracle's on every other shape;
(b) the oracle's hiding proofs, split into roots, opened values and the FriProof section, and reference proofs of seeded general
    shapes: the library's verifier and the Python one accept, end on the prover's transcript, and both reject a perturbed word of every
    section (opened value, commit-phase root, opened row, salt of an input opening, salt of a FRI layer, path, final polynomial,
    witness)."""
import numpy as np
import pytest

import pcs_hiding_ref as H
import pcs_ref as R
from test_pcs_verify_host import FIRST_ROWS, FRI_SETS, HASHES

P = R.P
PREFIX = np.arange(1, 6, dtype=np.uint32)  # some transcript before the open
SEEDS = (1, 7)


def _sets(log_n):
    return [t for t in FRI_SETS if t[1] < log_n + 1]  # the committed polynomials have degree < 2^(log_n + 1)


def _ref_low_rows(com, log_size):
    return com.ldes[0][:1 << log_size]


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_n", range(1, 8))
def test_reference_prover_gives_the_oracle_hiding_fib_bytes(oracle, hash, kind, log_n):
    sets = _sets(log_n)
    assert sets
    for i, t in enumerate(sets):
        for seed in SEEDS:
            a, b = FIRST_ROWS[(log_n + kind + i) % 3]
            ref = oracle.prove_fib_air_hiding(a, b, log_n, oracle.FriParams(*t), hash=kind, seed=seed)
            got = H.fib_through(H.HidingPcs(kind, t, 4, seed, seed), R.RefChallenger(kind), log_n, oracle.generate_trace_rows(a, b, 1 << log_n),
                                R.fib_pis(a, b, log_n), _ref_low_rows)
            assert len(got) == len(ref), (t, seed, len(got), len(ref))
            if got != ref:
                w1, w2 = np.frombuffer(got, np.uint32), np.frombuffer(ref, np.uint32)
                pytest.fail("%s log_n %d fri %s seed %d: words differ first at %d of %d" % (hash, log_n, t, seed, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


# ---- the two verifiers ----
def _lib_code(p3, t, hash, vr, log_h, opened, fri, prefix):
    ch = p3.Challenger(hash)
    prefix(ch)
    try:
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, ch, hiding=True)
    except p3.PcsRejected as e:
        assert e.message.startswith("pcs verification failed: "), e.message
        return e.code, ch
    return 0, ch


def _ref_code(kind, t, log_h, vr, opened, fri, prefix):
    ch = R.RefChallenger(kind)
    prefix(ch)
    return H.verify(kind, t, log_h, vr, opened, fri, ch), ch


def _sections(t, log_h, vr, fri):
    """word positions of the FriProof bytes by section, from the call's dimensions (never from the bytes)"""
    log_blowup, lfp, nq, _ = t
    log_big, n_fr, fpl = log_h + 1 + log_blowup, log_h + 1 - lfp, 1 << lfp
    sec = {k: [] for k in ("roots", "row", "input salt", "path", "sibling", "fri salt", "final polynomial", "witness")}
    pos = 1
    sec["roots"] += range(pos, pos + 8 * n_fr)
    pos += 8 * n_fr + 1
    for _ in range(nq):
        pos += 1
        for (_, ws), _ in vr:
            pos += 1
            for w in ws:
                sec["row"] += range(pos + 1, pos + 1 + w)
                pos += 1 + w
            for _ in ws:
                sec["input salt"] += range(pos + 1, pos + 1 + H.SALT)
                pos += 1 + H.SALT
            sec["path"] += range(pos + 1, pos + 1 + 8 * log_big)
            pos += 1 + 8 * log_big
        pos += 1
        for r in range(n_fr):
            sec["sibling"] += range(pos, pos + 4)
            sec["fri salt"] += range(pos + 5, pos + 5 + H.SALT)
            pos += 5 + H.SALT
            sec["path"] += range(pos + 1, pos + 1 + 8 * (log_big - 1 - r))
            pos += 1 + 8 * (log_big - 1 - r)
    sec["final polynomial"] += range(pos + 1, pos + 1 + 4 * fpl)
    pos += 1 + 4 * fpl
    sec["witness"].append(pos)
    assert pos + 1 == len(fri) // 4, (pos, len(fri))
    return sec


def _check(p3, rng, hash, kind, t, log_h, vr, opened, fri, prefix, want):
    """both verifiers accept and end where the prover ended (want: its next sample); both reject a perturbed word of every section"""
    code, lch = _lib_code(p3, t, hash, vr, log_h, opened, fri, prefix)
    assert code == 0
    code, rch = _ref_code(kind, t, log_h, vr, opened, fri, prefix)
    assert code == 0
    assert np.array_equal(lch.sample_ext(), want) and np.array_equal(rch.sample_ext(), want)
    bump = lambda v: (int(v) + 1) % P

    def both_reject(o, f):
        a, b = _lib_code(p3, t, hash, vr, log_h, o, f, prefix)[0], _ref_code(kind, t, log_h, vr, o, f, prefix)[0]
        return a != 0 and b != 0

    bad = opened.copy().reshape(-1)
    pos = int(rng.integers(0, bad.size))
    bad[pos] = bump(bad[pos])
    assert both_reject(bad.reshape(-1, 4), fri), ("opened", pos)
    words = np.frombuffer(fri, dtype=np.uint32)
    for name, where in _sections(t, log_h, vr, fri).items():
        assert where, name
        pos = int(where[int(rng.integers(0, len(where)))])
        b = words.copy()
        b[pos] = bump(b[pos])
        assert both_reject(opened, b.tobytes()), (name, pos)


def _queries(t, log_h):
    """raise the query count until the indices carry 20 bits (tests/test_pcs_ref_host.py _fri: a perturbed word that moves the transcript
    is rejected because the indices move with it)"""
    return (t[0], t[1], max(t[2], -(-20 // (log_h + 1 + t[0]))), t[3])


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_n", range(1, 8))
def test_both_verifiers_on_the_oracle_hiding_proofs(p3, oracle, hash, kind, log_n):
    sets = _sets(log_n)
    t = _queries(sets[(log_n + kind) % len(sets)], log_n)
    a, b = FIRST_ROWS[(log_n + kind) % 3]
    seed = SEEDS[log_n % 2]
    proof = oracle.prove_fib_air_hiding(a, b, log_n, oracle.FriParams(*t), hash=kind, seed=seed)
    assert oracle.verify_fib_air_hiding(proof, a, b, oracle.fib_public_x(a, b, 1 << log_n), log_n, oracle.FriParams(*t), hash=kind) == 0
    ln, root_t, root_q, root_r, opened, fri = H.split_fib_proof(proof)
    assert ln == log_n and len(opened) == 36
    pis = R.fib_pis(a, b, log_n)
    state = {}

    def prefix(ch):
        H.fib_begin(ch, log_n, root_t, pis)
        state["z"] = H.fib_zeta(ch, log_n, root_q, root_r)

    prefix(R.RefChallenger(kind))
    zeta, zeta_next = state["z"]
    vr = [((root_r, [8]), [[zeta]]), ((root_t, [6]), [[zeta, zeta_next]]), ((root_q, [4] * 4), [[zeta]] * 4)]
    # the prover's transcript after the last query index: the reference prover gives these very bytes (test (a)), so its challenger is the
    # oracle's
    pch = R.RefChallenger(kind)
    got = H.fib_through(H.HidingPcs(kind, t, 4, seed, seed), pch, log_n, oracle.generate_trace_rows(a, b, 1 << log_n), pis, _ref_low_rows)
    assert got == proof
    _check(p3, np.random.default_rng(300 + 2 * log_n + kind), hash, kind, t, log_n, vr, opened, fri, prefix, pch.sample_ext())


WIDTHS = (1, 2, 17, 60, 61, 129)
NRCS = (1, 3, 4)


def _general_case(case, log_h):
    rng = np.random.default_rng(7000 + case)
    hash, kind = HASHES[case % 2]
    nrc = NRCS[case % 3]
    log_blowup = int(rng.integers(1, 4))
    t = _queries((log_blowup, int(rng.integers(0, min(log_h + 1, 4))), int(rng.integers(1, 5)), int(rng.integers(0, 6))), log_h)
    pcs = H.HidingPcs(kind, t, nrc, mmcs_seed=int(rng.integers(1, 1 << 30)), pcs_seed=int(rng.integers(1, 1 << 30)))
    quotient = (2 if case % 4 < 2 else 4, int(rng.choice((1, 4, 5)))) if case % 3 != 2 else None
    plan, rounds = H.random_rounds(rng, pcs, log_h, WIDTHS, max_rounds=1 if case % 4 == 0 else 4, quotient=quotient, randomization=case % 2 == 1,
                                   max_cols=500)
    return rng, hash, kind, t, pcs, plan, rounds


@pytest.mark.parametrize("log_h", range(1, 7))
def test_general_shapes_are_accepted_and_every_section_is_checked(p3, oracle, log_h):
    for i in range(2):
        rng, hash, kind, t, pcs, plan, rounds = _general_case(2 * log_h + i, log_h)
        prefix = lambda ch: ch.observe(PREFIX)
        pch = R.RefChallenger(kind)
        prefix(pch)
        opened, fri = pcs.open(rounds, pch)
        vr = H.verifier_rounds(rounds)
        assert len(opened) == sum(w * len(pts) for (_, ws), mp in vr for w, pts in zip(ws, mp))
        _check(p3, rng, hash, kind, t, log_h, vr, opened, fri, prefix, pch.sample_ext())


def test_general_cases_reach_what_they_are_meant_to():
    """over the twelve cases: 1 and 4 rounds, 1 and 4 matrices, every width and NRC, C = 2 and 4, a matrix without points, four points, a
    repeated point"""
    seen = set()
    for log_h in range(1, 7):
        for i in range(2):
            _, _, _, _, pcs, plan, rounds = _general_case(2 * log_h + i, log_h)
            seen.add("rounds%d" % len(rounds))
            seen.add("nrc%d" % pcs.nrc)
            for what, arg, mpts in plan:
                if what == "commit":
                    seen.add("mats%d" % len(arg))
                    seen |= {"w%d" % m.shape[1] for m, _ in arg}
                if what == "quotient":
                    seen.add("C%d" % len(arg))
                for pts in mpts:
                    seen.add("np%d" % len(pts))
                    if len({bytes(z) for z in pts}) < len(pts):
                        seen.add("repeat")
    want = {"rounds1", "rounds4", "mats1", "mats4", "C2", "C4", "np0", "np4", "repeat"} | {"w%d" % w for w in WIDTHS} | {"nrc%d" % n for n in NRCS}
    assert want <= seen, sorted(want - seen)


def test_hiding_verify_argument_gates(p3, oracle):
    t, log_h, kind = (1, 0, 10, 1), 2, 0
    pcs = H.HidingPcs(kind, t, 3)
    rng = np.random.default_rng(9)
    z = R.rand_point(rng)
    com = pcs.commit([(R.rand_matrix(rng, log_h, 2), None)])
    pch = R.RefChallenger(kind)
    opened, fri = pcs.open([(com, [[z]])], pch)
    fp = p3.FriParameters(*t)

    def refused(match, vr, op=opened, params=fp, lh=log_h):
        ch = p3.Challenger("poseidon2")
        with pytest.raises(p3.P3HipError, match=match) as e:
            p3.pcs.verify(params, "poseidon2", vr, lh, op, fri, ch, hiding=True)
        assert e.value.code == -1 and not isinstance(e.value, p3.PcsRejected)
        assert np.array_equal(ch.sample_ext(), p3.Challenger("poseidon2").sample_ext())  # a refused call leaves the transcript alone

    vr = [((com.root, [5]), [[z]])]
    p3.pcs.verify(fp, "poseidon2", vr, log_h, opened, fri, p3.Challenger("poseidon2"), hiding=True)
    refused("round 0 has more than 4 matrices", [((com.root, [1] * 5), [[z]] * 5)], op=np.zeros((5, 4), np.uint32))
    refused("log_final_poly_len must be below", vr, params=p3.FriParameters(1, 3, 10, 1))
    refused(r"log_h must be in \[1, 26\]", vr, lh=0)
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_h + 2), 3)))  # the LDE coset has 2^(log_h + 1 + log_blowup) points
    refused("round 0 matrix 0 point 0 lies on the LDE coset", [((com.root, [5]), [[on]])])
    # the plain verifier does not take these bytes: its query section has another length
    with pytest.raises(p3.PcsRejected):
        p3.pcs.verify(fp, "poseidon2", vr, log_h + 1, opened, fri, p3.Challenger("poseidon2"))
