"""CPU tests of the AIR fuzz suite (tests/air_fuzz.py): that the suite holds the shapes it is there for; air_create's figures and
the host evaluation on every one of its programs against tests/air_ref.py; AirBuilder.compile() against values computed without
it; the program at every capacity.  The device side of the same programs is tests/test_gpu_air_fuzz.py."""
import numpy as np
import pytest

import air_fuzz as F
import air_ref as A
import pcs_ref as R

P = R.P
CASES = F.FUZZ_CASES
N_SHADOW = 200


def test_the_suite_holds_the_shapes_it_is_there_for():
    assert len(CASES) == 52 and [c.index for c in CASES] == list(range(52))
    for lqd in range(4):
        assert sum(c.lqd == lqd for c in CASES) >= 12, lqd
    for j, c in enumerate(CASES[:48]):  # the tail pins the degree
        assert max(c.degrees) == F.MAX_DEGS[j // 12] and c.lqd == F.LOG_QUOTIENT_DEGREE[max(c.degrees)]
        assert 1 <= c.width <= 8 and c.n_public <= 3 and len(c.consts) <= 3 and 1 <= c.K <= 12
    assert sum(c.K & 1 for c in CASES) >= 15 and sum(not c.K & 1 for c in CASES) >= 15
    assert any(c.K == 1 for c in CASES)
    assert {0, 1, 2, 64} <= {c.n_slots for c in CASES}
    # the shapes the compiler never emits
    rows = [r for c in CASES for r in c.code.tolist()]
    slot = lambda s: F.op(A.SLOT, s)
    assert any(r[0] != A.ASSERT_ZERO and r[2] == r[3] == slot(r[1]) for r in rows), "op s, s, s"
    assert any(r[0] == A.MUL and r[2] == r[3] == slot(r[1]) for r in rows), "MUL s, s, s"
    assert any(r[0] == A.ASSERT_ZERO and r[2] >> 24 == A.SELECTOR for r in rows), "a selector asserted as it is"
    assert any(r[0] != A.ASSERT_ZERO and r[3] >> 24 == A.SELECTOR for r in rows), "a selector as operand b"
    assert any(c.n_slots == 64 and len(set(c.code[c.code[:, 0] != A.ASSERT_ZERO, 1].tolist())) < 64 for c in CASES), "high slots with low ones unwritten"
    assert any(c.K == 1 and c.n_slots == 0 and c.code[0, 2] >> 24 == A.SELECTOR for c in CASES), "a selector alone"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "case%d" % c.index)
def test_figures_and_eval_ext_of_every_program(p3, oracle, case):
    air = case.air(p3)
    assert (air.width, air.n_public, air.n_instructions) == (case.width, case.n_public, len(case.code))
    assert (air.n_constraints, air.max_degree, air.log_quotient_degree) == (case.K, max(case.degrees), case.lqd)
    assert air.n_slots == case.n_slots
    rng = np.random.default_rng([7, case.index])
    for _ in range(2):
        local, nxt, pis = F.rand_words(rng, air.width, 4), F.rand_words(rng, air.width, 4), F.rand_words(rng, air.n_public)
        sels, alpha = F.rand_words(rng, 3, 4), F.rand_words(rng, 4)
        want = A.eval_ext(case.code, case.consts, local, nxt, pis, sels, alpha)
        assert np.array_equal(air.eval_ext(local, nxt, pis, sels, alpha), want), case
    air.free()


def test_compiled_builder_dags_give_the_shadow_values(p3, oracle):
    """the compiler and its slot allocator against integers nobody ran through it: a slot freed one use early, or two distinct
    nodes merged, changes a value here.  The DAGs are sized so that the 64 slots suffice for nearly all: at most 5 % may be refused,
    and only by that name."""
    refused, most_slots = 0, 0
    for seed in range(N_SHADOW):
        b, values, asg = F.shadow_case(p3, seed)
        code, consts = b.compile()
        cw = A._canon_list(consts)
        leaf = lambda kind, idx: cw[idx] if kind == A.CONST else asg[kind][idx]
        assert A.run(code, leaf, A._VEC) == values, seed
        try:
            air = p3.Air(b.width, b.n_public, code, consts)
        except p3.P3HipError as e:
            assert "capacity exceeded: at most 64 slots" in str(e), (seed, str(e))
            refused += 1
            continue
        assert air.n_constraints == len(values)
        most_slots = max(most_slots, air.n_slots)
        air.free()
    assert refused <= N_SHADOW // 20, refused
    assert most_slots >= 8  # the pool keeps values alive: the allocator is not idle


@pytest.fixture(scope="module")
def capacity(p3, oracle):
    code, consts = F.capacity_program()
    return p3.Air(F.CAP_WIDTH, F.CAP_PUBLIC, code, consts), code, consts


def test_capacity_program_stands_at_every_limit(p3, capacity):
    air, code, consts = capacity
    assert (air.width, air.n_public, len(air.consts)) == (p3.air.MAX_WIDTH, p3.air.MAX_PUBLIC, p3.air.MAX_CONSTS) == (8192, 4096, 65536)
    assert (air.n_instructions, air.n_constraints, air.n_slots) == (p3.air.MAX_INSTRUCTIONS, p3.air.MAX_CONSTRAINTS, p3.air.MAX_SLOTS) == (65536, 4096, 64)
    assert (air.max_degree, air.log_quotient_degree) == (1, 0) and A.degrees(code) == ([1] * 4096, 0)
    value = code[code[:, 0] != A.ASSERT_ZERO]
    assert set(value[:, 0].tolist()) == {A.ADD, A.SUB}
    for col, name in ((2, "a"), (3, "b")):  # every kind in both positions; every index range from its first to its last
        kinds, idx = value[:, col] >> 24, value[:, col] & 0xFFFFFF
        assert set(kinds.tolist()) == {A.SLOT, A.LOCAL, A.NEXT, A.PUBLIC, A.CONST, A.SELECTOR}, name
    both = np.concatenate([value[:, 2], value[:, 3]])
    kinds, idx = both >> 24, both & 0xFFFFFF
    for kind, count in ((A.LOCAL, 8192), (A.NEXT, 8192), (A.PUBLIC, 4096), (A.SELECTOR, 3), (A.SLOT, 64)):
        assert set(idx[kinds == kind].tolist()) == set(range(count)), kind
    used = idx[kinds == A.CONST]
    assert used.min() == 0 and used.max() == 65535 and len(set(used.tolist())) == 7 * 4096


def test_capacity_program_eval_ext_equals_the_reference(capacity):
    air, code, consts = capacity
    rng = np.random.default_rng(8192)
    local, nxt, pis = F.rand_words(rng, air.width, 4), F.rand_words(rng, air.width, 4), F.rand_words(rng, air.n_public)
    sels, alpha = F.rand_words(rng, 3, 4), F.rand_words(rng, 4)
    assert np.array_equal(air.eval_ext(local, nxt, pis, sels, alpha), A.eval_ext(code, consts, local, nxt, pis, sels, alpha))
