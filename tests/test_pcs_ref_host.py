"""CPU tests of the reference prover of tests/pcs_ref.py (open: oracle/stark.c:71-154 restated for any shape) and, through it, of
the library's host verifier on shapes other than the fib_air instance.

(a) the reference prover driven through the fib_air instance gives oracle.prove_fib_air's bytes: the pin that lets its bytes stand
    for the oracle's on every other shape;
(b) seeded general shapes: p3.pcs.verify (host code of the library) and pcs_ref.verify accept what it proves, leave the same
    transcript, and both reject a perturbed word of every section;
(c) the shapes that must not be left to chance: four points on one matrix, matrices and a whole round without points, the same
    point twice in one list."""
import numpy as np
import pytest

import pcs_ref as R
from test_pcs_verify_host import FIRST_ROWS, FRI_SETS, HASHES

P = R.P
PREFIX = np.arange(1, 6, dtype=np.uint32)  # some transcript before the open


def test_numpy_extension_inverse_and_powers_match_the_oracle():
    rng = np.random.default_rng(6)
    a = rng.integers(0, P, (64, 4), dtype=np.uint64)
    a[0] = [P - 1, 0, 0, 0]
    a[1] = [0, 0, 0, 1]
    a[2] = [0, P - 1, 0, 0]
    got = R.O.to_monty(R._canon_ext_inv(a))
    for i in range(64):
        assert np.array_equal(got[i], R.ext_inv(R.O.to_monty(a[i]))), i
    pw, acc = R.O.to_monty(R._ext_powers(a[5], 37)), R.ext_from_base(R.ONE)
    for i in range(37):
        assert np.array_equal(pw[i], acc), i
        acc = R.ext_mul(acc, R.O.to_monty(a[5]))


def test_reference_challenger_clone_is_independent():
    for kind in (0, 1):
        ch = R.RefChallenger(kind)
        ch.observe(PREFIX)
        ch.sample_ext()
        ch.observe([7, 8, 9])
        c = ch.clone()
        c.observe([1])
        c.sample_ext()
        d = ch.clone()
        assert np.array_equal(ch.sample_ext(), d.sample_ext()) and not np.array_equal(c.sample_ext(), d.sample_ext())


def _fib_through_the_reference(oracle, kind, log_n, t, a, b):
    """tests/test_gpu_pcs.py _fib_through_pcs with the reference prover in the device PCS's place"""
    trace, pis = oracle.generate_trace_rows(a, b, 1 << log_n), R.fib_pis(a, b, log_n)
    root_t, _, (lde_t,) = R.commit(kind, t[0], [(trace, None)])
    ch = R.RefChallenger(kind)
    ch.observe([int(oracle.to_monty(log_n))] * 2)
    ch.observe_digest(root_t)
    ch.observe(pis)
    alpha = ch.sample_ext()
    quot = R.fib_quotient(lde_t[:1 << log_n], log_n, pis, alpha)
    root_q, _, _ = R.commit(kind, t[0], [(quot, R.GEN)])
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    zeta_next = R.ext_scale(zeta, R.two_adic_generator(log_n))
    opened, fri, roots = R.open_with_roots(kind, t, log_n, [[(trace, None, [zeta, zeta_next])], [(quot, R.GEN, [zeta])]], ch)
    assert np.array_equal(roots[0], root_t) and np.array_equal(roots[1], root_q)
    return R.fib_header(log_n, root_t, root_q, opened) + fri


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_n", range(1, 9))
def test_reference_prover_gives_the_oracle_fib_bytes(oracle, hash, kind, log_n):
    sets = [t for t in FRI_SETS if t[1] < log_n]
    assert sets
    for i, t in enumerate(sets):
        a, b = FIRST_ROWS[(log_n + kind + i) % 3]
        ref = oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind)
        got = _fib_through_the_reference(oracle, kind, log_n, t, a, b)
        assert len(got) == len(ref), (t, len(got), len(ref))
        if got != ref:
            w1, w2 = np.frombuffer(got, np.uint32), np.frombuffer(ref, np.uint32)
            pytest.fail("%s log_n %d fri %s: words differ first at %d of %d" % (hash, log_n, t, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


def _lib_code(p3, t, hash, vr, log_h, opened, fri):
    ch = p3.Challenger(hash)
    ch.observe(PREFIX)
    try:
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, ch)
    except p3.PcsRejected as e:
        return e.code, ch
    return 0, ch


def _ref_code(kind, t, log_h, vr, opened, fri):
    ch = R.RefChallenger(kind)
    ch.observe(PREFIX)
    return R.verify(kind, t, log_h, vr, opened, fri, ch), ch


def _prove_and_verify(p3, rng, hash, kind, t, log_h, rounds, perturb=True):
    pch = R.RefChallenger(kind)
    pch.observe(PREFIX)
    opened, fri, roots = R.open_with_roots(kind, t, log_h, rounds, pch)
    assert len(opened) == sum(m.shape[1] * len(pts) for mats in rounds for m, _, pts in mats)
    vr = R.verifier_rounds(roots, rounds)
    code, lch = _lib_code(p3, t, hash, vr, log_h, opened, fri)
    assert code == 0
    code, rch = _ref_code(kind, t, log_h, vr, opened, fri)
    assert code == 0
    want = pch.sample_ext()  # prover and both verifiers stand after the last query index
    assert np.array_equal(lch.sample_ext(), want) and np.array_equal(rch.sample_ext(), want)
    if not perturb:
        return
    bump = lambda v: (int(v) + 1) % P
    both_reject = lambda o, f: _lib_code(p3, t, hash, vr, log_h, o, f)[0] != 0 and _ref_code(kind, t, log_h, vr, o, f)[0] != 0
    bad = opened.copy().reshape(-1)
    pos = int(rng.integers(0, bad.size))
    bad[pos] = bump(bad[pos])
    assert both_reject(bad.reshape(-1, 4), fri), ("opened", pos)
    words = np.frombuffer(fri, dtype=np.uint32)
    n_fr, fpl = int(words[0]), 1 << t[1]
    q0, q1 = 2 + 8 * n_fr, len(words) - 2 - 4 * fpl  # commit-phase roots | queries | final polynomial | witness
    for name, (lo, hi) in {"roots": (1, 1 + 8 * n_fr), "queries": (q0, q1), "final polynomial": (q1 + 1, len(words) - 1),
                           "witness": (len(words) - 1, len(words))}.items():
        assert hi > lo, name
        pos = int(rng.integers(lo, hi))
        b = words.copy()
        b[pos] = bump(b[pos])
        assert both_reject(opened, b.tobytes()), (name, pos)


def _fri(rng, log_h, max_queries=6, max_bits=6):
    """blowup 1..3, any final polynomial length, 1..max_queries queries or as many as 20 bits of query indices take: a perturbed
    word that moves the transcript (a root, the final polynomial, the witness) is rejected because the indices move with it, and
    on an LDE of 4 rows one index in four stays"""
    log_blowup = int(rng.integers(1, 4))
    nq = max(int(rng.integers(1, max_queries + 1)), -(-20 // (log_h + log_blowup)))
    return (log_blowup, int(rng.integers(0, min(log_h, 4))), nq, int(rng.integers(0, max_bits + 1)))


@pytest.mark.parametrize("log_h", range(1, 8))
def test_general_shapes_are_accepted_by_both_verifiers(p3, oracle, log_h):
    """Three seeded shapes per height (pcs_ref.random_case): the first CPU run of the library's pcs_verify beyond the fib shape."""
    for i in range(3):
        case = 3 * log_h + i
        rng = np.random.default_rng(4000 + case)
        hash, kind = HASHES[case % 2]
        rounds = R.random_case(rng, log_h)
        _prove_and_verify(p3, rng, hash, kind, _fri(rng, log_h), log_h, rounds)


def test_generator_reaches_what_it_is_meant_to():
    """the generator keeps its limits, and over 70 seeds draws repeats, empty lists, four points, 4 rounds, 8 matrices, wide matrices"""
    seen = set()
    for seed in range(5000, 5070):
        rng = np.random.default_rng(seed)
        rounds = R.random_case(rng, 3)
        cols = sum(m.shape[1] * len(pts) for mats in rounds for m, _, pts in mats)
        assert 0 < cols <= 600 and 1 <= len(rounds) <= 4 and all(1 <= len(mats) <= 8 for mats in rounds)
        distinct = {bytes(z) for mats in rounds for _, _, pts in mats for z in pts}
        assert len(distinct) <= 4
        seen.add("rounds%d" % len(rounds))
        for mats in rounds:
            seen.add("mats%d" % len(mats))
            for m, s, pts in mats:
                seen.add("np%d" % len(pts))
                if len({bytes(z) for z in pts}) < len(pts):
                    seen.add("repeat")
                if m.shape[1] >= 63 and pts:
                    seen.add("wide")
    assert {"rounds1", "rounds4", "mats1", "mats8", "np0", "np4", "repeat", "wide"} <= seen, seen


@pytest.mark.parametrize("hash,kind", HASHES)
def test_four_points_on_one_matrix(p3, oracle, hash, kind):
    rng = np.random.default_rng(41 + kind)
    for log_h, w in ((2, 1), (5, 17)):
        _prove_and_verify(p3, rng, hash, kind, (1 + kind, 0, 8, 2), log_h, R.four_point_case(rng, log_h, w))


@pytest.mark.parametrize("hash,kind", HASHES)
def test_matrices_and_a_round_without_points(p3, oracle, hash, kind):
    rng = np.random.default_rng(43 + kind)
    rounds = R.empty_point_case(rng, 4)
    assert not rounds[0][0][2] and not rounds[-1][-1][2] and all(not pts for _, _, pts in rounds[1])
    _prove_and_verify(p3, rng, hash, kind, (2 - kind, 1, 4, 2), 4, rounds)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_the_same_point_twice_in_one_list(p3, oracle, hash, kind):
    rng = np.random.default_rng(45 + kind)
    rounds = R.repeated_point_case(rng, 3)
    pch = R.RefChallenger(kind)
    opened, _ = R.open(kind, (1, 0, 2, 1), 3, rounds, pch)
    assert np.array_equal(opened[0:2], opened[2:4]) and np.array_equal(opened[4:21], opened[38:55])  # z0 z0 | z1 z0 z1
    _prove_and_verify(p3, rng, hash, kind, (1, 0, 5, 1), 3, rounds)
