"""GPU tests of caller-defined AIRs (include/p3hip.h "caller-defined AIRs", csrc/air.hip, plonky3-mobile_amd/air.py): the quotient
kernel word for word against the independent evaluator of tests/air_ref.py on random matrices; prove_air byte for byte against the
oracle and FibAirProver on the fib program and against the reference prover on three other AIRs; check_trace; lifetime.  No test
provokes a fault: a program the library refuses never reaches a launch (tests/test_air_host.py)."""
import gc

import numpy as np
import pytest

import air_ref as A
import pcs_ref as R

pytestmark = pytest.mark.gpu
P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
FRI_SETS = [(1, 0, 100, 16), (2, 0, 10, 4), (2, 2, 6, 5), (1, 3, 9, 0), (3, 1, 4, 10), (1, 0, 0, 0), (1, 8, 3, 2), (4, 0, 2, 1)]  # tests/test_gpu_pcs.py
FIRST_ROWS = [(0, 1), (7, 11), (P - 1, 1)]
NAMES = ["fib", "B", "C", "D"]


@pytest.fixture(scope="module")
def airs(p3, oracle):
    return A.all_airs(p3)


def _same(proof, ref, what):
    assert len(proof) == len(ref), (what, len(proof), len(ref))
    if proof != ref:
        w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
        pytest.fail("%s: proof words differ first at %d of %d" % (what, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


@pytest.mark.parametrize("name", NAMES)
def test_quotient_chunks_equal_the_reference_on_random_matrices(p3, oracle, airs, name):
    """The quotient is defined for any matrix: random ones enter every opcode and operand kind.  log_n 1: `next` wraps inside one
    stride; log_n 9 with 4 chunks: 2048 rows, several workgroups; log_blowup = log_quotient_degree: the quotient domain is the
    whole LDE, + 1: its first half."""
    import torch
    air = airs[name][0]
    lqd = air.log_quotient_degree
    rng = np.random.default_rng(100 + len(name))
    for log_n in (1, 2, 5, 9):
        trace = R.rand_matrix(rng, log_n, air.width)
        pis, alpha = R.O.to_monty(rng.integers(0, P, air.n_public, dtype=np.uint64)), R.rand_point(rng)
        lde = oracle.coset_lde_batch(trace, lqd + 1, p3.GENERATOR_MONTY, True)  # bit-reversed: the smaller LDE is its first half
        qn = (1 << log_n) << lqd
        want = A.quotient_chunks(air.code, air.consts, lde[:qn], log_n, pis, alpha)
        assert len(want) == air.n_chunks
        for log_blowup, rows in ((lqd, qn), (lqd + 1, 2 * qn)):
            d_lde = p3.dev_u32(np.ascontiguousarray(lde[:rows]))
            got = air.quotient(d_lde, log_n, log_blowup, pis, alpha)
            torch.cuda.synchronize()
            assert len(got) == len(want)
            for c, (g, w) in enumerate(zip(got, want)):
                assert tuple(g.shape) == (1 << log_n, 4)
                assert np.array_equal(p3.host_u32(g), w), (name, log_n, log_blowup, c)
    if lqd:
        d_lde = p3.dev_u32(np.ascontiguousarray(lde))
        with pytest.raises(p3.P3HipError, match="log_blowup %d is below log_quotient_degree %d" % (lqd - 1, lqd)):
            air.quotient(d_lde, 9, lqd - 1, pis, alpha)


def test_quotient_of_a_program_that_fills_the_slots(p3, oracle):
    """the test AIRs live in two or three slots at the most; a right-leaning sum keeps every term alive, so this program writes and reads slots
    up to the cap (degree 3, two chunks), at 2^9 rows: several workgroups with 63 KiB of LDS each"""
    import torch
    b = p3.AirBuilder(66, 1)
    terms = [b.local(c) * b.next(c + 1) + b.public(0) for c in range(A.MAX_SLOTS - 1)]
    inner = terms[-1]
    for t in reversed(terms[:-1]):
        inner = t - inner
    b.when_transition().assert_zero(inner)
    b.when_last_row().assert_zero(b.local(65) * b.local(65) - b.const(5))
    air = b.build()
    assert air.n_slots >= A.MAX_SLOTS - 1 and air.log_quotient_degree == 1
    rng = np.random.default_rng(64)
    for log_n in (1, 9):
        trace = R.rand_matrix(rng, log_n, air.width)
        pis, alpha = R.O.to_monty(rng.integers(0, P, 1, dtype=np.uint64)), R.rand_point(rng)
        lde = oracle.coset_lde_batch(trace, 1, p3.GENERATOR_MONTY, True)
        want = A.quotient_chunks(air.code, air.consts, lde, log_n, pis, alpha)
        got = air.quotient(p3.dev_u32(lde), log_n, 1, pis, alpha)
        torch.cuda.synchronize()
        for c in range(2):
            assert np.array_equal(p3.host_u32(got[c]), want[c]), (log_n, c)
    trace = R.rand_matrix(rng, 9, air.width)
    assert air.check_trace(trace, pis) == A.check_trace(air.code, air.consts, trace, pis) == (0, 0)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_fib_program_proves_the_oracles_and_the_fib_provers_bytes(p3, oracle, airs, hash, kind):
    air = airs["fib"][0]
    off = 3 * kind
    cases = []
    for log_n in range(1, 11):  # every log_n with one applicable set and one first row, rotating
        valid = [t for t in FRI_SETS if t[1] < log_n]
        cases.append((log_n, valid[(log_n + off) % len(valid)], FIRST_ROWS[(log_n + off) % 3]))
    cases += [(9, t, FIRST_ROWS[(i + off) % 3]) for i, t in enumerate(FRI_SETS)]  # every set, where all eight apply
    for log_n, t, (a, b) in cases:
        what = "%s log_n %d fri %s first row (%d, %d)" % (hash, log_n, t, a, b)
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
        pis = R.fib_pis(a, b, log_n)
        proof = p3.prove_air(air, pcs, p3.generate_trace_rows(a, b, 1 << log_n), pis)
        pcs.free()
        _same(proof, oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind), what + " against the oracle")
        pr = p3.FibAirProver(log_n, params=p3.FriParameters(*t), hash=hash)
        _same(proof, pr.prove(a, b), what + " against FibAirProver")
        pr.close()
        if t[2]:  # the PCS verifier refuses a proof without queries by name
            p3.verify_air(air, proof, pis, log_n, p3.FriParameters(*t), hash)


CASES_BC = [("B", 3, (1, 0, 5, 3)), ("B", 6, (2, 1, 4, 2)), ("B", 6, (1, 2, 6, 0)), ("B", 3, (2, 0, 3, 4)), ("C", 3, (2, 0, 4, 3)), ("C", 6, (2, 2, 3, 1)),
            ("D", 1, (3, 0, 2, 1)), ("D", 3, (3, 0, 3, 1)), ("D", 4, (4, 1, 2, 0)), ("D", 6, (3, 2, 4, 2))]  # 8 chunk matrices, 8 shifts


@pytest.mark.parametrize("name,log_n,t", CASES_BC)
def test_other_airs_prove_the_reference_provers_bytes(p3, oracle, airs, name, log_n, t):
    air, gen = airs[name]
    trace, pis = gen(log_n)
    assert air.check_trace(trace, pis) is None
    for hash, kind in HASHES:
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
        proof = p3.prove_air(air, pcs, p3.dev_u32(trace), pis)
        pcs.free()
        _same(proof, A.prove(kind, t, air.code, air.consts, trace, pis), "%s log_n %d %s %s" % (name, log_n, t, hash))
        p3.verify_air(air, proof, pis, log_n, p3.FriParameters(*t), hash)
        assert A.verify(kind, t, air.code, air.consts, air.width, proof, pis, log_n) == 0


@pytest.mark.parametrize("name,t", [("fib", (1, 0, 4, 2)), ("B", (1, 1, 4, 2)), ("C", (2, 0, 3, 1)), ("D", (3, 0, 3, 1))])
def test_proofs_of_broken_statements_are_rejected_by_both_verifiers(p3, oracle, airs, name, t):
    air, gen = airs[name]
    log_n = 4
    trace, pis = gen(log_n)
    bad_trace = trace.copy()
    bad_trace[5, 0] = (int(bad_trace[5, 0]) + 1) % P
    bad_pis = pis.copy()
    bad_pis[-1] = (int(bad_pis[-1]) + 1) % P
    for hash, kind in HASHES:
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
        for tr, pi in ((bad_trace, pis), (trace, bad_pis)):
            proof = p3.prove_air(air, pcs, tr, pi)  # the prover does not judge: the quotient is no polynomial of the degree
            with pytest.raises(p3.AirRejected) as e:
                p3.verify_air(air, proof, pi, log_n, p3.FriParameters(*t), hash)
            assert e.value.code == 10
            assert A.verify(kind, t, air.code, air.consts, air.width, proof, pi, log_n) == 10
        good = p3.prove_air(air, pcs, trace, pis)
        with pytest.raises(p3.AirRejected) as e:  # a right proof against another public value
            p3.verify_air(air, good, bad_pis, log_n, p3.FriParameters(*t), hash)
        assert e.value.code == 10 and A.verify(kind, t, air.code, air.consts, air.width, good, bad_pis, log_n) == 10
        pcs.free()


@pytest.mark.parametrize("name", NAMES)
def test_check_trace_names_the_smallest_failing_row_and_constraint(p3, airs, name):
    air, gen = airs[name]
    log_n = 9
    trace, pis = gen(log_n)
    n = 1 << log_n
    assert air.check_trace(trace, pis) is None  # in particular the wrap from the last row to row 0 is no transition
    assert air.check_trace(p3.dev_u32(trace), pis) is None
    small, spis = gen(1)
    assert air.check_trace(small, spis) is None
    for row in (0, n - 1, 300):
        for col in (0, air.width - 1):
            bad = trace.copy()
            bad[row, col] = (int(bad[row, col]) + 1) % P
            want = A.check_trace(air.code, air.consts, bad, pis)
            assert want is not None and want[0] in ((row - 1, row) if row else (0,))
            assert air.check_trace(bad, pis) == want, (name, row, col)
    wrong = pis.copy()
    wrong[-1] = (int(wrong[-1]) + 1) % P
    want = A.check_trace(air.code, air.consts, trace, wrong)
    assert want is not None and air.check_trace(trace, wrong) == want
    # two rows broken: the smaller one is named
    bad = trace.copy()
    bad[400, 0] = (int(bad[400, 0]) + 1) % P
    bad[77, air.width - 1] = (int(bad[77, air.width - 1]) + 1) % P
    want = A.check_trace(air.code, air.consts, bad, pis)
    assert want[0] in (76, 77) and air.check_trace(bad, pis) == want


AIRS_PER_CYCLE = 200


def test_device_memory_is_unchanged_over_cycles_of_two_airs_on_one_pcs(p3, oracle):
    """Two AIRs created, used alternately on ONE PCS and freed, 10 cycles; every cycle also creates, uses on the device and frees
    AIRS_PER_CYCLE further Airs of each program, so that the library's own allocation per Air — its device block of program, constants,
    per-call table and result word, a raw device allocation that torch's counter does not see — is what the free-memory figure weighs.
    After the first cycle (which builds the cached root tables and fills torch's allocator) torch's allocated bytes do not move, and
    free device memory does not fall by 288 KiB.  One leaked block per Air would take, over the nine measured cycles, 9 x 200 blocks of
    (B) (23 instructions of 16 bytes, 2 constants, a table of 60 words: 0.6 KiB before any rounding by the runtime) = 1.1 MiB and 9 x
    200 blocks of (C) (770 instructions, a table of 2.3 KiB: 15 KiB) = 26 MiB; one leaked chunk LDE of (C) per cycle (the smallest
    matrix of a cycle, 2^12 rows x 4 words = 64 KiB) would take 576 KiB.  The bound is half of the smallest of these.  The device is shared, so the
    figure is not asserted to be exactly equal: another process may allocate between the two readings."""
    import torch
    t, log_n = (2, 1, 4, 2), 10
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t))
    traces = {"B": A.trace_b(log_n), "C": A.trace_c(log_n)}
    dev = {k: p3.dev_u32(v[0]) for k, v in traces.items()}
    small = {k: (p3.dev_u32(v[0]), v[1]) for k, v in (("B", A.trace_b(1)), ("C", A.trace_c(1)))}
    alpha = R.rand_point(np.random.default_rng(3))

    def cycle():
        made = {"B": A.air_b(p3), "C": A.air_c(p3)}
        for k in ("B", "C", "B", "C"):
            assert made[k].check_trace(dev[k], traces[k][1]) is None
            proof = p3.prove_air(made[k], pcs, dev[k], traces[k][1])
            p3.verify_air(made[k], proof, traces[k][1], log_n, p3.FriParameters(*t))
        for i in range(AIRS_PER_CYCLE):  # from the compiled programs: creation is the library's, not the builder's
            for k in ("B", "C"):
                a = p3.Air(made[k].width, made[k].n_public, made[k].code, made[k].consts)
                if i & 1:  # either device entry makes the device block
                    assert a.check_trace(small[k][0], small[k][1]) is None
                else:
                    a.quotient(dev[k], 1, t[0], traces[k][1], alpha)
                a.free()
        for a in made.values():
            a.free()
        gc.collect()

    def state():
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]

    cycle()
    alloc0, free0 = state()
    for _ in range(9):
        cycle()
    alloc1, free1 = state()
    pcs.free()
    assert alloc1 == alloc0, "torch's allocated bytes moved by %d" % (alloc1 - alloc0)
    assert free0 - free1 < 288 * 1024, "free device memory fell by %d bytes over 9 cycles" % (free0 - free1)
