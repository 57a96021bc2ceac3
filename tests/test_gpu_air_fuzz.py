"""GPU tests of the AIR interpreter (csrc/air.hip air_kernel<0> quotient, air_kernel<1> check) on the programs of tests/air_fuzz.py:
random raw three-address code of every log_quotient_degree — shapes the builder's compiler never emits —, programs without a slot,
the program at every capacity, extreme operand words, and calls on one Air that follow each other without a synchronisation, on
one stream and on two.  Every comparison is word for word (or byte for byte) with tests/air_ref.py.  Every program reaches the
device through p3.Air, that is through air_create's validation; no test aims at a fault."""
import numpy as np
import pytest

import air_fuzz as F
import air_ref as A
import pcs_ref as R

pytestmark = pytest.mark.gpu
P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
CASES = F.FUZZ_CASES
CHECK_LOG_N = 9


def _heights(case):
    """log_n 1: `next` wraps inside one stride, with 8 chunks the domain has 16 rows, one partial workgroup; 3; and for a quarter of
    the programs — another slot span for every degree — 9: several workgroups, 4096 rows with 8 chunks"""
    return (1, 3, 9) if case.index % 4 == (case.index // 12) % 4 else (1, 3)


def _compare(p3, air, case, lde, log_n, pis, alpha, blowups, what):
    import torch
    qn = (1 << log_n) << case.lqd
    want = A.quotient_chunks(air.code, air.consts, lde[:qn], log_n, pis, alpha)
    assert len(want) == air.n_chunks == 1 << case.lqd
    for log_blowup in blowups:
        d_lde = p3.dev_u32(np.ascontiguousarray(lde[:(1 << log_n) << log_blowup]))
        got = air.quotient(d_lde, log_n, log_blowup, pis, alpha)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for c, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == (1 << log_n, 4)
            assert np.array_equal(p3.host_u32(g), w), "%s %r log_n %d log_blowup %d chunk %d" % (what, case, log_n, log_blowup, c)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "case%d" % c.index)
def test_quotient_of_every_program_equals_the_reference(p3, oracle, case):
    """log_blowup = log_quotient_degree: the quotient domain is the whole LDE; + 2: its first quarter"""
    air = case.air(p3)
    rng = np.random.default_rng([11, case.index])
    for log_n in _heights(case):
        trace = R.rand_matrix(rng, log_n, case.width)
        pis, alpha = F.rand_words(rng, case.n_public), R.rand_point(rng)
        lde = oracle.coset_lde_batch(trace, case.lqd + 2, p3.GENERATOR_MONTY, True)  # bit-reversed: a smaller LDE is its first rows
        _compare(p3, air, case, lde, log_n, pis, alpha, (case.lqd, case.lqd + 2), "random")
    air.free()


EXTREME_WORDS = [("0", 0), ("ONE", int(R.ONE)), ("P-1", P - 1)]
EXTREME_CASES = [next(c for c in CASES[:48] if c.K % 2 == 0 and c.lqd == 3 and c.n_public and len(c.consts)), next(c for c in CASES[48:] if c.K == 2)]


@pytest.mark.parametrize("name,word", EXTREME_WORDS)
@pytest.mark.parametrize("case", EXTREME_CASES, ids=lambda c: "case%d" % c.index)
def test_quotient_on_matrices_of_one_extreme_word(p3, oracle, case, name, word):
    """The quotient is defined for any matrix, so one whose every word is 0, ONE or P - 1 is handed in as the LDE, with the public
    values, the constants and alpha at the same word: bb::mul / add / sub at their edges, and under dot2 three of the four factors
    at P - 1 (2 (P - 1)^2 is the sum its 2 P^2 < 2^32 P margin is for)."""
    log_n = 3
    full = lambda *shape: np.full(shape, word, dtype=np.uint32)
    air = p3.Air(case.width, case.n_public, case.code, full(len(case.consts)))
    lde = full((1 << log_n) << case.lqd, case.width)
    _compare(p3, air, case, lde, log_n, full(case.n_public), full(4), (case.lqd,), "every word " + name)
    air.free()


# ---- check_trace ----
def check_inputs(case):
    """-> [(what, consts, trace, pis)]: a random trace; the zero trace with zero public values; the same with the constants zeroed"""
    rng = np.random.default_rng([13, case.index])
    n = 1 << CHECK_LOG_N
    zero_t, zero_p = np.zeros((n, case.width), dtype=np.uint32), np.zeros(case.n_public, dtype=np.uint32)
    return [("random", case.consts, R.rand_matrix(rng, CHECK_LOG_N, case.width), F.rand_words(rng, case.n_public)),
            ("zero", case.consts, zero_t, zero_p), ("all zero", np.zeros_like(case.consts), zero_t, zero_p)]


def test_check_trace_of_every_program_equals_the_reference(p3, oracle):
    wanted = []
    for case in CASES:
        airs = {}
        for what, consts, trace, pis in check_inputs(case):
            key = consts.tobytes()
            if key not in airs:
                airs[key] = p3.Air(case.width, case.n_public, case.code, consts)
            air = airs[key]
            want = A.check_trace(case.code, consts, trace, pis)
            assert air.check_trace(trace, pis) == want, "%r %s trace" % (case, what)
            wanted.append(want)
        for air in airs.values():
            air.free()
    # what the reference alone says the kernel was asked: every kind of answer occurs
    last = (1 << CHECK_LOG_N) - 1
    assert None in wanted
    assert any(w is not None and w[0] != 0 for w in wanted)
    assert any(w is not None and w[0] == last for w in wanted)
    assert any(w is not None and w[1] != 0 for w in wanted)


# ---- every capacity at once ----
def test_capacity_program_runs_at_every_limit(p3, oracle):
    """width 8192, 4096 public values, 65536 constants, 65536 instructions, 4096 constraints, 64 slots: the table of the call, its
    offsets and the pinned staging at the sizes they were dimensioned for"""
    import torch
    code, consts = F.capacity_program()
    air = p3.Air(F.CAP_WIDTH, F.CAP_PUBLIC, code, consts)
    assert (air.n_instructions, air.n_constraints, air.n_slots, air.n_chunks) == (65536, 4096, 64, 1)
    rng = np.random.default_rng(4096)
    for log_n in (1, 2):
        trace = R.rand_matrix(rng, log_n, air.width)
        pis, alpha = F.rand_words(rng, air.n_public), R.rand_point(rng)
        lde = oracle.coset_lde_batch(trace, 1, p3.GENERATOR_MONTY, True)
        want = A.quotient_chunks(code, consts, lde[:1 << log_n], log_n, pis, alpha)
        for log_blowup in (0, 1):
            got = air.quotient(p3.dev_u32(np.ascontiguousarray(lde[:(1 << log_n) << log_blowup])), log_n, log_blowup, pis, alpha)
            torch.cuda.synchronize()
            assert len(got) == 1 and np.array_equal(p3.host_u32(got[0]), want[0]), (log_n, log_blowup)
    want = A.check_trace(code, consts, trace, pis)
    assert want is not None and air.check_trace(trace, pis) == want
    zero_t, zero_p = np.zeros_like(trace), np.zeros_like(pis)
    assert air.check_trace(zero_t, zero_p) == A.check_trace(code, consts, zero_t, zero_p)
    air.free()


# ---- one Air, calls that follow each other without a synchronisation ----
def _air_b_inputs(p3, oracle, log_n):
    air = A.air_b(p3)
    rng = np.random.default_rng(17)
    trace = R.rand_matrix(rng, log_n, air.width)
    lde = oracle.coset_lde_batch(trace, 1, p3.GENERATOR_MONTY, True)
    args = [(F.rand_words(rng, air.n_public), R.rand_point(rng)) for _ in range(3)]
    wants = [A.quotient_chunks(air.code, air.consts, lde, log_n, pis, alpha) for pis, alpha in args]
    assert not np.array_equal(wants[0][0], wants[1][0])  # the table of one call is no good to the other
    return air, trace, lde, args, wants


def test_calls_on_one_air_follow_each_other_on_one_stream(p3, oracle):
    """quotient, quotient, check_trace, quotient on one stream with nothing between them: every call restages the object's ONE table
    through its ONE pinned buffer, and the two entry points lay that table out differently.  Each result is its own call's."""
    import torch
    log_n = 10
    air, trace, lde, args, wants = _air_b_inputs(p3, oracle, log_n)
    d_lde, d_trace = p3.dev_u32(lde), p3.dev_u32(trace)
    want_check = A.check_trace(air.code, air.consts, trace, args[2][0])
    torch.cuda.synchronize()
    q0 = air.quotient(d_lde, log_n, 1, *args[0])
    q1 = air.quotient(d_lde, log_n, 1, *args[1])
    got_check = air.check_trace(d_trace, args[2][0])
    q2 = air.quotient(d_lde, log_n, 1, *args[2])
    torch.cuda.synchronize()
    assert got_check == want_check and want_check is not None
    for i, got in enumerate((q0, q1, q2)):
        for c in range(2):
            assert np.array_equal(p3.host_u32(got[c]), wants[i][c]), ("call", i, "chunk", c)
    air.free()


def test_calls_on_one_air_from_two_streams_are_serialised(p3, oracle):
    """include/p3hip.h: a call on another stream than the one before it is ordered behind that call's kernel, so the second stream's
    upload cannot replace the table the first stream's kernel is still reading.  The capacity program makes the window wide: its
    one wave interprets 65536 instructions, tens of milliseconds in which it reads public values and alpha powers from the table
    all along and the chunk pointer at the very end, while the host needs microseconds to enqueue the next call.  Each result is
    read after its own stream alone."""
    import torch
    log_n = 1
    code, consts = F.capacity_program()
    air = p3.Air(F.CAP_WIDTH, F.CAP_PUBLIC, code, consts)
    rng = np.random.default_rng(23)
    lde = oracle.coset_lde_batch(R.rand_matrix(rng, log_n, air.width), 1, p3.GENERATOR_MONTY, True)
    args = [(F.rand_words(rng, air.n_public), R.rand_point(rng)) for _ in range(2)]
    wants = [A.quotient_chunks(code, consts, lde[:1 << log_n], log_n, pis, alpha)[0] for pis, alpha in args]
    assert not np.array_equal(wants[0], wants[1])  # the table of one call is no good to the other
    d_lde = p3.dev_u32(lde)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for rounds in range(3):  # s0, s1, s0
        i = rounds & 1
        with torch.cuda.stream(streams[i]):
            got.append((i, air.quotient(d_lde, log_n, 1, *args[i])[0]))
    for i in (0, 1):
        streams[i].synchronize()
        for n, (s, chunk) in enumerate(got):
            if s == i:
                assert np.array_equal(p3.host_u32(chunk), wants[s]), ("call", n, "stream", s)
    torch.cuda.synchronize()
    air.free()


# ---- prove_air of programs nobody wrote ----
PROVE_CASES = [next(c for c in CASES if c.lqd == 3 and c.n_public), next(c for c in CASES if c.lqd == 2 and c.n_public)]


@pytest.mark.parametrize("case", PROVE_CASES, ids=lambda c: "case%d" % c.index)
def test_prove_air_of_fuzz_programs_gives_the_reference_provers_bytes(p3, oracle, case):
    """the prover does not judge: a random trace satisfies no such program, the bytes are the reference prover's all the same, and
    both verifiers answer OodEvaluationMismatch"""
    log_n, t = 3, (3, 0, 3, 1)
    air = case.air(p3)
    rng = np.random.default_rng([19, case.index])
    trace, pis = R.rand_matrix(rng, log_n, case.width), F.rand_words(rng, case.n_public)
    for hash, kind in HASHES:
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
        proof = p3.prove_air(air, pcs, p3.dev_u32(trace), pis)
        pcs.free()
        ref = A.prove(kind, t, case.code, case.consts, trace, pis)
        assert len(proof) == len(ref), (case, hash)
        if proof != ref:
            w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
            pytest.fail("%r %s: proof words differ first at %d of %d" % (case, hash, int(np.nonzero(w1 != w2)[0][0]), len(w1)))
        with pytest.raises(p3.AirRejected) as e:
            p3.verify_air(air, proof, pis, log_n, p3.FriParameters(*t), hash)
        assert e.value.code == 10
        assert A.verify(kind, t, case.code, case.consts, case.width, proof, pis, log_n) == 10
    air.free()
