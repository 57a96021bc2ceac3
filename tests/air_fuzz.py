"""Seeded generators of AIR programs for the fuzz tests (tests/test_air_fuzz_host.py, tests/test_gpu_air_fuzz.py): random valid
three-address code written straight in the encoding of include/p3hip.h — the shapes AirBuilder.compile() never emits —, programs
that assert leaves only, random builder DAGs that carry the integer value of every node (a shadow evaluation made without the
compiler), and one fixed program at every capacity at once.  Nothing here runs a program: the answers come from tests/air_ref.py.
Every generator is a function of its seed alone, so a case index names a failure completely."""
import numpy as np

import air_ref as A
from pcs_ref import O, P

LEAF_DEGREE = {A.LOCAL: 1, A.NEXT: 1, A.SELECTOR: 1, A.PUBLIC: 0, A.CONST: 0}
LOG_QUOTIENT_DEGREE = {2: 0, 3: 1, 5: 2, 9: 3}  # of a program whose largest constraint degree is the key


def op(kind, idx):
    return (kind << 24) | int(idx)


def _leaf_kinds(n_public, n_consts):
    """a kind with no instances is left out: the draw is uniform over the others"""
    return [A.LOCAL, A.NEXT] + ([A.PUBLIC] if n_public else []) + ([A.CONST] if n_consts else []) + [A.SELECTOR]


def _draw_leaf(rng, width, n_public, n_consts):
    kinds = _leaf_kinds(n_public, n_consts)
    kind = kinds[int(rng.integers(len(kinds)))]
    count = {A.LOCAL: width, A.NEXT: width, A.PUBLIC: n_public, A.CONST: n_consts, A.SELECTOR: 3}[kind]
    return op(kind, rng.integers(count)), LEAF_DEGREE[kind]


def _draw_operand(rng, width, n_public, n_consts, slot_deg):
    """-> (operand word, degree): a written slot with probability 0.6, else a leaf of a uniformly drawn kind"""
    if slot_deg and rng.random() < 0.6:
        s = sorted(slot_deg)[int(rng.integers(len(slot_deg)))]
        return op(A.SLOT, s), slot_deg[s]
    return _draw_leaf(rng, width, n_public, n_consts)


def raw_program(rng, width, n_public, n_consts, n_instr, n_constraints, max_deg, slot_span, tail=True, extra=False):
    """-> (n, 4) uint32 code: n_instr random ADD / SUB / MUL instructions with dst uniform in range(slot_span), among them, at
    random places, the assertions: n_constraints in all when `tail` (the last one is the tail's), n_constraints without.  Degrees
    follow air_ref.degrees' rules; whatever would exceed max_deg is drawn again.  The tail pins the largest degree to max_deg
    exactly: MUL dst, local, next; max_deg - 2 times MUL dst, dst, local; ASSERT_ZERO dst.  `extra` appends one more assertion, so
    that either parity of the constraint count can be asked for."""
    assert max_deg >= 2 and slot_span >= 1 and n_constraints >= 1
    body_asserts = n_constraints - 1 if tail else n_constraints
    steps = np.array([0] * n_instr + [1] * body_asserts)
    rng.shuffle(steps)
    slot_deg, code = {}, []
    draw = lambda: _draw_operand(rng, width, n_public, n_consts, slot_deg)

    def assertion():
        while True:
            o, d = draw()
            if d <= max_deg:
                return [A.ASSERT_ZERO, 0, o, 0]

    for is_assert in steps.tolist():
        if is_assert:
            code.append(assertion())
            continue
        while True:
            opc = int(rng.integers(3))  # ADD, SUB, MUL
            (oa, da), (ob, db) = draw(), draw()
            d = da + db if opc == A.MUL else max(da, db)
            if d <= max_deg:
                break
        dst = int(rng.integers(slot_span))
        slot_deg[dst] = d
        code.append([opc, dst, oa, ob])
    if tail:
        dst = int(rng.integers(slot_span))
        code.append([A.MUL, dst, op(A.LOCAL, rng.integers(width)), op(A.NEXT, rng.integers(width))])
        for _ in range(max_deg - 2):
            code.append([A.MUL, dst, op(A.SLOT, dst), op(A.LOCAL, rng.integers(width))])
        slot_deg[dst] = max_deg
        code.append([A.ASSERT_ZERO, 0, op(A.SLOT, dst), 0])
    if extra:
        code.append(assertion())
    return np.array(code, dtype=np.uint32).reshape(-1, 4)


def leaf_program(rng, width, n_public, n_consts, K, first=None):
    """-> (K, 4) code that asserts leaves only: no instruction writes a slot (n_slots == 0).  `first`: the first assertion's operand"""
    code = []
    for k in range(K):
        o = first if k == 0 and first is not None else _draw_leaf(rng, width, n_public, n_consts)[0]
        code.append([A.ASSERT_ZERO, 0, o, 0])
    return np.array(code, dtype=np.uint32).reshape(-1, 4)


def rand_words(rng, *shape):
    return O.to_monty(rng.integers(0, P, shape, dtype=np.uint64))


# ---- builder DAGs with a shadow evaluation ----
SHADOW_MAX_DEGREE = 9
_SPECIAL = (0, 1, P - 1, 7)


def shadow_dag(rng, builder, n_nodes, n_asserts):
    """Builds a random DAG with `builder`'s own operators and asserts n_asserts of its values.  Every node carries the integer a
    direct evaluation gives it on ONE drawn assignment of local, next, public and the three selectors, and its degree, so that
    nothing asserted exceeds degree 9.  Operands come from a pool that only grows, the newest values preferred: chains grow deep, values are shared and live long.
    -> (the asserted values in assertion order, the assignment {kind: [integers]})"""
    w, n_pub = builder.width, builder.n_public
    word = lambda: int(_SPECIAL[rng.integers(4)]) if rng.random() < 0.2 else int(rng.integers(P))
    asg = {A.LOCAL: [word() for _ in range(w)], A.NEXT: [word() for _ in range(w)], A.PUBLIC: [word() for _ in range(n_pub)],
           A.SELECTOR: [word() for _ in range(3)]}
    pool = [(builder.local(c), asg[A.LOCAL][c], 1) for c in range(w)] + [(builder.next(c), asg[A.NEXT][c], 1) for c in range(w)]
    pool += [(builder.public(i), asg[A.PUBLIC][i], 0) for i in range(n_pub)]
    pool += [(e, asg[A.SELECTOR][i], 1) for i, e in enumerate((builder.is_first_row, builder.is_last_row, builder.is_transition))]
    # half of the draws take one of the newest eight values, so that chains grow deep; the other half reach back anywhere
    pick = lambda: pool[int(rng.integers(max(len(pool) - 8, 0), len(pool)))] if rng.random() < 0.5 else pool[int(rng.integers(len(pool)))]
    const = lambda: int(_SPECIAL[rng.integers(4)]) if rng.random() < 0.5 else int(rng.integers(P))
    while len(pool) < n_nodes:
        how = int(rng.integers(10))
        (a, va, da), (b, vb, db), c = pick(), pick(), const()
        if how == 0:
            node = (a + b, va + vb, max(da, db))
        elif how == 1:
            node = (a - b, va - vb, max(da, db))
        elif how in (2, 3):
            if da + db > SHADOW_MAX_DEGREE:
                continue
            node = (a * b, va * vb, da + db)
        elif how == 4:
            node = (-a, -va, da)
        elif how == 5:
            node = (c + a, c + va, da)
        elif how == 6:
            node = (c - a, c - va, da)
        elif how == 7:
            node = (c * a, c * va, da)
        elif how == 8:
            node = (a - c, va - c, da)
        else:
            node = (builder.const(c), c, 0)
        pool.append((node[0], node[1] % P, node[2]))
    values = []
    filters = (builder.when_first_row, builder.when_last_row, builder.when_transition)
    while len(values) < n_asserts:
        how = int(rng.integers(4))
        (a, va, da), (b, vb, db) = pick(), pick()
        if how == 0:
            builder.assert_zero(a)
            values.append(va)
        elif how == 1:
            builder.assert_eq(a, b)
            values.append((va - vb) % P)
        else:
            if max(da, db) + 1 > SHADOW_MAX_DEGREE:
                continue
            f = int(rng.integers(3))
            if how == 2:
                filters[f]().assert_zero(a)
                values.append(asg[A.SELECTOR][f] * va % P)
            else:
                filters[f]().assert_eq(a, b)
                values.append(asg[A.SELECTOR][f] * (va - vb) % P)
    return values, asg


def shadow_case(p3, seed):
    """the builder of shadow DAG number `seed` with its asserted values and assignment"""
    rng = np.random.default_rng([0x5AD0, seed])
    b = p3.AirBuilder(int(rng.integers(1, 6)), int(rng.integers(0, 3)))
    values, asg = shadow_dag(rng, b, int(rng.integers(10, 301)), int(rng.integers(1, 13)))
    return b, values, asg


# ---- the capacities, all at once ----
CAP_WIDTH, CAP_PUBLIC, CAP_CONSTS, CAP_INSTRUCTIONS, CAP_CONSTRAINTS = 8192, 4096, 65536, 65536, 4096


def capacity_program():
    """-> (code, consts): width 8192, 4096 public values, 65536 constants, 65536 instructions, 4096 constraints, 64 slots; add and
    sub only, so degree 1 and one chunk.  4096 groups of 15 value instructions and one assertion; group g sums 16 leaves into slot
    g mod 64: seven constants, three local and three next columns, two public values and a selector, in an order that turns with g,
    so that every kind stands in both operand positions.  Each kind's index counts on from group to group: columns and public
    values run through their whole range, the constants' indices are spread from 0 to 65535, both ends included."""
    rng = np.random.default_rng(0xCA9)
    consts = rand_words(rng, CAP_CONSTS)
    groups = CAP_CONSTRAINTS
    kinds = [A.CONST, A.LOCAL, A.NEXT, A.PUBLIC, A.CONST, A.SELECTOR, A.CONST, A.LOCAL, A.NEXT, A.CONST, A.CONST, A.LOCAL, A.NEXT, A.CONST,
             A.PUBLIC, A.CONST]
    n_const_uses = 7 * groups
    used = {k: 0 for k in set(kinds)}
    ops = rng.integers(0, 2, (groups, 15))  # ADD or SUB

    def leaf(kind, g):
        u = used[kind]
        used[kind] += 1
        if kind == A.CONST:
            return op(kind, u * (CAP_CONSTS - 1) // (n_const_uses - 1))
        if kind == A.SELECTOR:
            return op(kind, g % 3)
        return op(kind, u % (CAP_PUBLIC if kind == A.PUBLIC else CAP_WIDTH))

    code = np.zeros((CAP_INSTRUCTIONS, 4), dtype=np.uint32)
    pc = 0
    for g in range(groups):
        slot = g % A.MAX_SLOTS
        order = [kinds[(m + g) % 16] for m in range(16)]
        code[pc] = (ops[g, 0], slot, leaf(order[0], g), leaf(order[1], g))
        pc += 1
        for t in range(1, 15):
            o = leaf(order[t + 1], g)
            code[pc] = (ops[g, t], slot, o, op(A.SLOT, slot)) if (g + t) & 1 else (ops[g, t], slot, op(A.SLOT, slot), o)
            pc += 1
        code[pc] = (A.ASSERT_ZERO, 0, op(A.SLOT, slot), 0)
        pc += 1
    assert pc == CAP_INSTRUCTIONS
    return code, consts


# ---- the suite ----
class Case:
    """one program of the suite with everything a test hands to p3.Air"""

    def __init__(self, index, what, width, n_public, consts, code):
        self.index, self.what, self.width, self.n_public, self.consts, self.code = index, what, width, n_public, consts, code
        self.degrees, self.lqd = A.degrees(code)
        self.K = len(self.degrees)
        written = code[code[:, 0] != A.ASSERT_ZERO, 1]
        self.n_slots = int(written.max()) + 1 if len(written) else 0

    def air(self, p3):
        return p3.Air(self.width, self.n_public, self.code, self.consts)

    def __repr__(self):
        return "case %d (%s)" % (self.index, self.what)


SLOT_SPANS = (1, 2, 8, 64)
MAX_DEGS = (2, 3, 5, 9)
SEED = 2


def _cases():
    out = []
    for j in range(48):  # 12 per max_deg; the slot span turns once per three programs of a degree
        max_deg, i = MAX_DEGS[j // 12], j % 12
        rng = np.random.default_rng([SEED, j])
        span = SLOT_SPANS[i % 4]
        width, n_public, n_consts = int(rng.integers(1, 9)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
        # a span of 64 with 200 instructions writes slot 63 almost surely; the others take 5..200
        n_instr = 200 if span == 64 and i < 4 else int(rng.integers(5, 201))
        K = 1 if j == 5 else int(rng.integers(1, 13))
        extra = bool(rng.integers(2)) and j != 5 and K < 12
        code = raw_program(rng, width, n_public, n_consts, n_instr, K, max_deg, span, extra=extra)
        what = "raw max_deg %d span %d width %d publics %d consts %d" % (max_deg, span, width, n_public, n_consts)
        out.append(Case(j, what, width, n_public, rand_words(rng, n_consts), code))
    leaves = [(1, 0, 0, 1, op(A.SELECTOR, 1)), (3, 2, 2, 2, None), (5, 0, 3, 5, op(A.SELECTOR, 0)), (8, 3, 0, 8, None)]
    for j, (width, n_public, n_consts, K, first) in enumerate(leaves, 48):
        rng = np.random.default_rng([SEED, j])
        code = leaf_program(rng, width, n_public, n_consts, K, first)
        out.append(Case(j, "leaves only, K %d" % K, width, n_public, rand_words(rng, n_consts), code))
    return out


FUZZ_CASES = _cases()
