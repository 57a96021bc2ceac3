"""CPU tests of caller-defined AIRs (include/p3hip.h "caller-defined AIRs", plonky3-mobile_amd/air.py): the program format and its
validation, the builder's compiler and slot allocator, the host evaluation over extension operands and verify_air, against the
independent evaluator, prover and verifier of tests/air_ref.py — which is itself pinned on the oracle's fib_air proofs first."""
import numpy as np
import pytest

import air_ref as A
import pcs_ref as R

P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
NAMES = ["fib", "B", "C", "D"]


@pytest.fixture(scope="module")
def airs(p3, oracle):
    return A.all_airs(p3)


def op(kind, idx):
    return (kind << 24) | idx


def test_fibonacci_air_figures(p3, airs):
    air = airs["fib"][0]
    assert (air.width, air.n_public, air.n_constraints, air.max_degree, air.log_quotient_degree, air.n_chunks) == (2, 3, 5, 2, 0, 1)
    assert A.degrees(air.code) == ([2] * 5, 0)
    assert air.n_slots <= 2 and len(air.consts) == 0


@pytest.mark.parametrize("hash,kind", HASHES)
def test_reference_prover_reproduces_the_oracle_on_fib(oracle, airs, hash, kind):
    """pins air_ref itself: the generic reference prover, run on the fib program, gives the oracle's fib_air bytes"""
    air = airs["fib"][0]
    for log_n in range(1, 8):
        for t in [(1, 0, 6, 3), (2, 0, 4, 5)]:
            a, b = (0, 1) if log_n & 1 else (7, P - 2)
            trace, pis = A.trace_fib(log_n, a, b)
            proof = A.prove(kind, t, air.code, air.consts, trace, pis)
            assert proof == oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind), (log_n, t)


def test_degrees_and_chunks_of_the_test_airs(airs):
    b, c, d = airs["B"][0], airs["C"][0], airs["D"][0]
    assert (b.width, b.n_constraints, b.max_degree, b.log_quotient_degree, b.n_chunks) == (3, 6, 3, 1, 2)
    assert (c.width, c.n_constraints, c.max_degree, c.log_quotient_degree, c.n_chunks) == (70, 140, 4, 2, 4)
    assert A.degrees(b.code)[1] == 1 and A.degrees(c.code)[1] == 2 and max(A.degrees(c.code)[0]) == 4
    assert len(b.consts) == 2
    # (D): three squarings and the transition filter give degree 9, the most a constraint may have: all 8 chunks
    assert (d.width, d.n_public, d.n_constraints, d.max_degree, d.log_quotient_degree, d.n_chunks) == (2, 1, 3, 9, 3, 8)
    assert A.degrees(d.code) == ([9, 2, 2], 3)
    # (C) has several times more value nodes than there are slots: its program exists only because slots are reused
    assert int((c.code[:, 0] != A.ASSERT_ZERO).sum()) > 4 * A.MAX_SLOTS and c.n_slots <= A.MAX_SLOTS


@pytest.mark.parametrize("name", NAMES)
def test_compiled_programs_hold_on_their_traces(airs, name):
    """the compiler and its slot reuse, by the independent evaluator: a generated trace satisfies the program, a trace with one
    word changed does not, and the first failure is where the change is"""
    air, gen = airs[name]
    trace, pis = gen(4)
    assert A.check_trace(air.code, air.consts, trace, pis) is None
    bad = trace.copy()
    bad[9, air.width - 1] = (int(bad[9, air.width - 1]) + 1) % P
    got = A.check_trace(air.code, air.consts, bad, pis)
    assert got is not None and got[0] == 8  # row 8's transition reads row 9
    wrong = pis.copy()
    wrong[0] = (int(wrong[0]) + 1) % P
    assert A.check_trace(air.code, air.consts, trace, wrong)[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_eval_ext_equals_the_reference(airs, name):
    air = airs[name][0]
    rng = np.random.default_rng(len(name))
    for _ in range(3):
        r = lambda *s: R.O.to_monty(rng.integers(0, P, s, dtype=np.uint64))
        local, nxt, pis, sels, alpha = r(air.width, 4), r(air.width, 4), r(air.n_public), r(3, 4), r(4)
        assert np.array_equal(air.eval_ext(local, nxt, pis, sels, alpha), A.eval_ext(air.code, air.consts, local, nxt, pis, sels, alpha))


def _code_of(p3, call):
    try:
        call()
        return 0
    except p3.AirRejected as e:
        return e.code


@pytest.mark.parametrize("name,log_n,t", [("fib", 4, (1, 1, 3, 2)), ("B", 3, (1, 0, 3, 2)), ("B", 4, (2, 1, 2, 1)), ("C", 3, (2, 0, 2, 1)), ("D", 3, (3, 0, 3, 1))])
def test_verify_air_accepts_reference_proofs_and_rejects_changes(p3, airs, name, log_n, t):
    air, gen = airs[name]
    trace, pis = gen(log_n)
    w, lqd = air.width, air.log_quotient_degree
    head = A.header_words(w, lqd)
    for hash, kind in HASHES:
        proof = A.prove(kind, t, air.code, air.consts, trace, pis)
        fp = p3.FriParameters(*t)
        p3.verify_air(air, proof, pis, log_n, fp, hash)  # accepts
        assert A.verify(kind, t, air.code, air.consts, w, proof, pis, log_n) == 0
        words = np.frombuffer(proof, dtype=np.uint32)

        def both(pw, pp=pis, ln=log_n):
            lib = _code_of(p3, lambda: p3.verify_air(air, pw.tobytes(), pp, ln, fp, hash))
            assert lib == A.verify(kind, t, air.code, air.consts, w, pw.tobytes(), pp, ln)
            return lib

        def bumped(pos, to=None):
            b = words.copy()
            b[pos] = (int(b[pos]) + 1) % P if to is None else to
            return b

        # an opened local value, an opened next value, a value of every chunk, a public value: OodEvaluationMismatch
        chunk0 = 19 + 2 * (1 + 4 * w) + 1
        for pos in [20 + 4 * (w - 1) + 1, 21 + 4 * w + 2] + [chunk0 + 17 * c + 1 + 5 for c in range(1 << lqd)]:
            assert both(bumped(pos)) == 10, pos
        for i in range(air.n_public):
            wrong = pis.copy()
            wrong[i] = (int(wrong[i]) + 1) % P
            assert both(words, wrong) == 10, i
        # every header word that is not a value: magic and version 1, log_n 2, the counts 3; a word that is no field element and a
        # truncated header 4
        assert both(bumped(0)) == 1 and both(bumped(1)) == 1
        assert both(bumped(2)) == 2 and both(words, ln=log_n + 1) == 2
        for pos in [19, 20 + 4 * w, 21 + 8 * w] + [chunk0 + 17 * c for c in range(1 << lqd)]:
            assert both(bumped(pos)) == 3, pos
            assert both(bumped(pos, 0x7fffffff)) == 3, pos  # a count is never followed
        assert both(bumped(20, P)) == 4 and both(bumped(chunk0 + 3, 0xffffffff)) == 4
        assert both(words[:head - 1]) == 4 and both(words[:21]) == 3 and both(words[:2]) == 2 and both(words[:0]) == 1
        # behind the header the PCS verifier's codes come through
        assert both(bumped(head)) == 5
        assert both(bumped(len(words) - 1)) in (11, 13, 14, 15)


def _refused(p3, match, width, n_public, code, consts=()):
    with pytest.raises(p3.P3HipError, match=match) as e:
        p3.Air(width, n_public, np.array(code, dtype=np.uint32).reshape(-1, 4), np.array(consts, dtype=np.uint32))
    assert e.value.code == -1


def test_create_refuses_by_name(p3):
    L, N, PUB, CON, SEL, SLOT = A.LOCAL, A.NEXT, A.PUBLIC, A.CONST, A.SELECTOR, A.SLOT
    ok = [[A.SUB, 0, op(L, 0), op(PUB, 0)], [A.ASSERT_ZERO, 0, op(SLOT, 0), 0]]
    p3.Air(1, 1, ok, []).free()
    one = int(R.ONE)
    _refused(p3, r"instruction 1: operand a: column 2 out of range \(width 2\)", 2, 1, [ok[0], [A.ADD, 1, op(L, 2), op(L, 0)], ok[1]])
    _refused(p3, r"instruction 0: operand b: column 3 out of range \(width 3\)", 3, 1, [[A.ADD, 0, op(L, 0), op(N, 3)], ok[1]])
    _refused(p3, r"instruction 0: operand b: public value 1 out of range \(1 public values\)", 1, 1, [[A.SUB, 0, op(L, 0), op(PUB, 1)], ok[1]])
    _refused(p3, r"instruction 0: operand a: constant 1 out of range \(1 constants\)", 1, 1, [[A.MUL, 0, op(CON, 1), op(L, 0)], ok[1]], [one])
    _refused(p3, r"instruction 0: operand a: selector 3 out of range", 1, 1, [[A.MUL, 0, op(SEL, 3), op(L, 0)], ok[1]])
    _refused(p3, r"instruction 1: operand a: slot 1 is read before any instruction wrote it", 1, 1, [ok[0], [A.ASSERT_ZERO, 0, op(SLOT, 1), 0]])
    _refused(p3, r"instruction 0: operand b: slot 0 is read before any instruction wrote it", 1, 1, [[A.ADD, 0, op(L, 0), op(SLOT, 0)], ok[1]])
    _refused(p3, r"instruction 1: unknown opcode 4", 1, 1, [ok[0], [4, 0, op(SLOT, 0), 0]])
    _refused(p3, r"instruction 0: operand b: unknown kind 6", 1, 1, [[A.ADD, 0, op(L, 0), op(6, 0)], ok[1]])
    _refused(p3, r"instruction 0: operand a: unknown kind 255", 1, 1, [[A.ADD, 0, 0xffffffff, op(L, 0)], ok[1]])
    _refused(p3, r"zero constraints", 1, 1, [ok[0]])
    _refused(p3, r"zero constraints", 1, 1, np.zeros((0, 4)))
    _refused(p3, r"instruction 1: assert_zero takes one operand", 1, 1, [ok[0], [A.ASSERT_ZERO, 0, op(SLOT, 0), op(L, 0)]])
    _refused(p3, r"instruction 0: slot 64 out of range \(capacity exceeded: at most 64 slots\)", 1, 1, [[A.SUB, 64, op(L, 0), op(PUB, 0)], ok[1]])
    _refused(p3, r"instruction 0: operand a: slot 64 out of range \(capacity exceeded", 1, 1, [[A.ASSERT_ZERO, 0, op(SLOT, 64), 0]])
    _refused(p3, r"constant 1 is not a canonical field element", 1, 1, ok, [one, P])
    _refused(p3, r"width 0: a trace has 1 to 8192 columns", 0, 1, ok)
    _refused(p3, r"width 8193", 8193, 1, ok)
    _refused(p3, r"capacity exceeded: 4097 public values", 1, 4097, ok)
    _refused(p3, r"capacity exceeded: 65537 instructions, at most 65536", 1, 1, [ok[0]] * 65536 + [ok[1]])
    _refused(p3, r"instruction 4097: capacity exceeded: at most 4096 constraints", 1, 1, [ok[0]] + [ok[1]] * 4097)
    # degree: x^10 asserted is beyond what the quotient's commitment can hold; as an intermediate value it is only a value
    powers = [[A.MUL, 0, op(L, 0), op(L, 0)]] + [[A.MUL, 0, op(SLOT, 0), op(L, 0)]] * 8  # slot 0 = x^10
    _refused(p3, r"instruction 9: capacity exceeded: constraint 0 has degree 10, at most 9", 1, 1, powers + [ok[1]])
    air = p3.Air(1, 1, powers[:8] + [ok[1]], [])  # x^9
    assert (air.max_degree, air.log_quotient_degree) == (9, 3)
    squarings = [[A.MUL, 0, op(L, 0), op(L, 0)]] + [[A.MUL, 0, op(SLOT, 0), op(SLOT, 0)]] * 40  # x^(2^41): the degree saturates
    _refused(p3, r"instruction 41: capacity exceeded: constraint 0 has degree >= ", 1, 1, squarings + [ok[1]])
    air = p3.Air(1, 1, squarings + [[A.SUB, 1, op(L, 0), op(PUB, 0)], [A.ASSERT_ZERO, 0, op(SLOT, 1), 0]], [])
    assert (air.max_degree, air.n_slots, air.n_constraints) == (1, 2, 1)
    assert p3.take_last_error() is None  # every message was taken by its exception


def test_slot_capacity_boundary(p3):
    """a program that keeps 64 values alive at once is accepted; one more is refused"""
    def program(k):
        code = [[A.ADD, s, op(A.LOCAL, 0), op(A.LOCAL, 0)] for s in range(k)]
        code += [[A.ADD, 0, op(A.SLOT, 0), op(A.SLOT, s)] for s in range(1, k)]
        return code + [[A.ASSERT_ZERO, 0, op(A.SLOT, 0), 0]]
    air = p3.Air(1, 0, program(A.MAX_SLOTS), [])
    assert air.n_slots == A.MAX_SLOTS == p3.air.MAX_SLOTS
    _refused(p3, r"instruction 64: slot 64 out of range \(capacity exceeded: at most 64 slots\)", 1, 0, program(A.MAX_SLOTS + 1))
    # the same through the builder: a right-leaning sum needs every term before its first addition
    for terms, fits in ((A.MAX_SLOTS - 1, True), (A.MAX_SLOTS + 1, False)):
        b = p3.AirBuilder(70, 0)
        sums = [b.local(c) * b.local(c + 1) for c in range(terms)]
        inner = sums[-1]
        for s in reversed(sums[:-1]):
            inner = s + inner
        b.assert_zero(inner)
        if fits:
            assert b.build().n_slots <= A.MAX_SLOTS
        else:
            with pytest.raises(p3.P3HipError, match="capacity exceeded: at most 64 slots"):
                b.build()


def test_slot_allocator_on_a_chain_of_500_dependent_products(p3):
    """acc <- acc * (public + k) + column, 500 times: every product depends on the one before; the values die as fast as they are
    made, so the program needs a handful of slots, not a thousand"""
    b = p3.AirBuilder(5, 2)
    acc = b.local(0)
    for k in range(500):
        acc = acc * (b.public(k & 1) + b.const(k)) + b.local(k % 5)
    b.when_transition().assert_zero(acc - b.next(0))
    air = b.build()
    assert air.n_instructions == 3 * 500 + 3 and air.n_slots <= 3 and air.max_degree == 2
    # the program computes what the recurrence says, by the independent evaluator on integers
    rng = np.random.default_rng(5)
    loc, pub = [int(v) for v in rng.integers(0, P, 5)], [int(v) for v in rng.integers(0, P, 2)]
    v = loc[0]
    for k in range(500):
        v = (v * (pub[k & 1] + k) + loc[k % 5]) % P
    consts = A._canon_list(air.consts)
    leaf = {A.LOCAL: lambda i: loc[i], A.NEXT: lambda i: 0, A.PUBLIC: lambda i: pub[i], A.CONST: lambda i: consts[i], A.SELECTOR: lambda i: 1}
    assert A.run(air.code, lambda kind, idx: leaf[kind](idx), A._VEC) == [v]


def test_common_subexpressions_are_emitted_once(p3):
    b = p3.AirBuilder(2, 0)
    s = b.local(0) + b.local(1)
    b.assert_zero(s * s - (b.local(1) + b.local(0)) * s)  # one sum, one product
    air = b.build()
    assert air.n_instructions == 4 and air.max_degree == 2  # add, mul, sub (x - x is not folded), assert


def test_verify_air_refuses_a_log_n_no_domain_has(p3, airs):
    air = airs["C"][0]  # two more bits for the quotient domain: 25 is the last log_n
    for bad in (0, -1, 26, 40):
        with pytest.raises(ValueError, match=r"verify_air: log_n must lie in 1\.\.25"):
            p3.verify_air(air, b"", [int(R.ONE)], bad, p3.FriParameters(2, 0, 2, 1))
    with pytest.raises(p3.AirRejected) as e:  # in range: the empty proof is judged
        p3.verify_air(air, b"", [int(R.ONE)], 25, p3.FriParameters(2, 0, 2, 1))
    assert e.value.code == 1
