"""What the tests of caller-defined AIRs compare the library with (include/p3hip.h "caller-defined AIRs"): an independent evaluator
of the instruction list in canonical integers (numpy uint64 over a domain, the oracle's extension arithmetic at a point), and a
reference prover and verifier for any program built on pcs_ref.commit / open / verify and RefChallenger, following
oracle/stark.c:37-70, 130-134 and 170-215 with the quotient split into chunks as p3_uni_stark does.  It shares nothing with the
package's compiler but the instruction list itself: the encoding is restated here from include/p3hip.h.

The four test AIRs and their trace generators are at the end; they are written with the package's AirBuilder, whose output —
the instruction list — is what both sides then run."""
import numpy as np

import pcs_ref as R
from pcs_ref import O, P

ADD, SUB, MUL, ASSERT_ZERO = 0, 1, 2, 3
SLOT, LOCAL, NEXT, PUBLIC, CONST, SELECTOR = range(6)
MAX_SLOTS = 64
MAGIC = 0x42463350


def _split(o):
    return int(o) >> 24, int(o) & 0xFFFFFF


# ---- the program over any ring: `ring` = (add, sub, mul); leaves come from `leaf(kind, index)` ----
def run(code, leaf, ring):
    """-> the constraint values, in assertion order"""
    add, sub, mul = ring
    slots, out = {}, []

    def get(o):
        kind, idx = _split(o)
        return slots[idx] if kind == SLOT else leaf(kind, idx)

    for op, dst, a, b in np.asarray(code, dtype=np.uint32).reshape(-1, 4).tolist():
        if op == ASSERT_ZERO:
            out.append(get(a))
        else:
            slots[dst] = (add, sub, mul)[op](get(a), get(b))
    return out


def degrees(code):
    """-> (degree of every constraint, log_quotient_degree) by upstream's SymbolicExpression rules"""
    d = run(code, lambda kind, idx: 1 if kind in (LOCAL, NEXT, SELECTOR) else 0, (max, max, lambda x, y: x + y))
    m, lqd = max(max(d), 2) - 1, 0
    while (1 << lqd) < m:
        lqd += 1
    return d, lqd


_VEC = (lambda a, b: (a + b) % P, lambda a, b: (a + P - b) % P, lambda a, b: a * b % P)  # canonical uint64 arrays / Python ints


def _vec_leaf(loc, nxt, pis, consts, sels):
    tables = {LOCAL: lambda i: loc[:, i], NEXT: lambda i: nxt[:, i], PUBLIC: lambda i: np.full(1, pis[i], dtype=np.uint64), CONST: lambda i: np.full(1, consts[i], dtype=np.uint64),
              SELECTOR: lambda i: sels[i]}
    return lambda kind, idx: tables[kind](idx)


def _canon_list(words):
    return [int(v) for v in O.from_monty(np.asarray(words, dtype=np.uint32).reshape(-1))] if len(words) else []


def quotient_chunks(code, consts, lde_low, log_n, pis, alpha):
    """quotient_values on GENERATOR * <g_qn>: lde_low the LDE's first qn rows (bit-reversed, Montgomery words) -> the C chunk
    matrices, (n, 4) Montgomery words; chunk c row r is natural row r C + c."""
    _, lqd = degrees(code)
    C, n = 1 << lqd, 1 << log_n
    log_qn, qn = log_n + lqd, n << lqd
    assert lde_low.shape[0] == qn
    t = O.from_monty(lde_low).astype(np.uint64)[R._bitrev(log_qn)]
    loc, nxt = t, np.roll(t, -C, axis=0)
    g_qn = int(O.from_monty(R.two_adic_generator(log_qn)))
    ginv = pow(int(O.from_monty(R.two_adic_generator(log_n))), P - 2, P)
    x = R._geom(g_qn, qn) * np.uint64(31) % P
    zh = (R._npow(x, n) + P - 1) % P
    zh_inv = R._npow(zh, P - 2)
    first = zh * R._npow((x + P - 1) % P, P - 2) % P
    last = zh * R._npow((x + P - ginv) % P, P - 2) % P
    trans = (x + P - ginv) % P
    cons = run(code, _vec_leaf(loc, nxt, _canon_list(pis), _canon_list(consts), [first, last, trans]), _VEC)
    K = len(cons)
    ap = R._ext_powers(O.from_monty(R.ext(alpha)), K)
    q = np.zeros((qn, 4), dtype=np.uint64)
    for k in range(K):  # the first constraint takes the highest power
        q = (q + (cons[k] * np.ones(qn, dtype=np.uint64))[:, None] * ap[K - 1 - k][None, :]) % P
    q = O.to_monty(q * zh_inv[:, None] % P)
    return [np.ascontiguousarray(q[c::C]) for c in range(C)]


def check_trace(code, consts, trace, pis):
    """check_constraints -> None, or the smallest failing (row, constraint)"""
    t = O.from_monty(trace).astype(np.uint64)
    n = len(t)
    i = np.arange(n)
    sels = [(i == 0).astype(np.uint64), (i == n - 1).astype(np.uint64), (i != n - 1).astype(np.uint64)]
    cons = run(code, _vec_leaf(t, np.roll(t, -1, axis=0), _canon_list(pis), _canon_list(consts), sels), _VEC)
    bad = np.stack([c * np.ones(n, dtype=np.uint64) != 0 for c in cons], axis=1)  # (row, constraint)
    rows = np.nonzero(bad.any(axis=1))[0]
    if not len(rows):
        return None
    return int(rows[0]), int(np.nonzero(bad[rows[0]])[0][0])


_EXT = (R.ext_add, R.ext_sub, R.ext_mul)  # Montgomery words, the oracle's products


def eval_ext(code, consts, local, nxt, pis, sels, alpha):
    """the constraints over extension operands (Montgomery words), folded by Horner's rule"""
    local, nxt, sels = (np.asarray(v, dtype=np.uint32).reshape(-1, 4) for v in (local, nxt, sels))
    tables = {LOCAL: lambda i: local[i], NEXT: lambda i: nxt[i], PUBLIC: lambda i: R.ext_from_base(pis[i]),
              CONST: lambda i: R.ext_from_base(consts[i]), SELECTOR: lambda i: sels[i]}
    acc = np.zeros(4, dtype=np.uint32)
    for c in run(code, lambda kind, idx: tables[kind](idx), _EXT):
        acc = R.ext_add(R.ext_mul(acc, alpha), c)
    return acc


# ---- p3_uni_stark::prove / verify ----
def _prefix(ch, log_n, root_t, pis):
    ch.observe([int(O.to_monty(log_n))] * 2)
    ch.observe_digest(root_t)
    ch.observe(pis)
    return ch.sample_ext()


def chunk_shifts(log_n, lqd):
    g = R.two_adic_generator(log_n + lqd)
    return [R.bmul(R.GEN, R.bpow(g, c)) for c in range(1 << lqd)]


def prove(kind, fp, code, consts, trace, pis):
    """fp = (log_blowup, log_final_poly_len, num_queries, pow_bits); trace (n, width) Montgomery words -> proof bytes"""
    trace = np.ascontiguousarray(trace, dtype=np.uint32)
    n, w = trace.shape
    log_n = n.bit_length() - 1
    _, lqd = degrees(code)
    assert fp[0] >= lqd
    pis = np.asarray(pis, dtype=np.uint32).reshape(-1)
    root_t, _, ldes = R.commit(kind, fp[0], [(trace, None)])
    ch = R.RefChallenger(kind)
    alpha = _prefix(ch, log_n, root_t, pis)
    chunks = quotient_chunks(code, consts, ldes[0][:n << lqd], log_n, pis, alpha)
    shifts = chunk_shifts(log_n, lqd)
    root_q, _, _ = R.commit(kind, fp[0], list(zip(chunks, shifts)))
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    zeta_next = R.ext_scale(zeta, R.two_adic_generator(log_n))
    rounds = [[(trace, None, [zeta, zeta_next])], [(c, s, [zeta]) for c, s in zip(chunks, shifts)]]
    opened, fri = R.open(kind, fp, log_n, rounds, ch)
    u = lambda *v: np.array(v, dtype=np.uint32)
    o = opened.reshape(-1)
    head = [u(MAGIC, 1, log_n), root_t, root_q, u(w), o[:4 * w], u(w), o[4 * w:8 * w], u(len(chunks))]
    for c in range(len(chunks)):
        head += [u(4), o[8 * w + 16 * c:8 * w + 16 * (c + 1)]]
    return np.concatenate(head).astype(np.uint32).tobytes() + fri


def header_words(width, lqd):
    return 3 + 16 + 2 * (1 + 4 * width) + 1 + 17 * (1 << lqd)


def verify(kind, fp, code, consts, width, proof, pis, log_n):
    """0 = accept, else the code of the failed check: 1-4 header, 10 OodEvaluationMismatch, pcs_ref.verify's otherwise"""
    _, lqd = degrees(code)
    C, n = 1 << lqd, 1 << log_n
    rd = R._Rd(proof)
    if rd.u32() != MAGIC or rd.u32() != 1:
        return 1
    if rd.u32() != log_n:
        return 2
    root_t, root_q = rd.words(8, field=(kind == 0)), rd.words(8, field=(kind == 0))
    if rd.u32() != width:
        return 3
    local = rd.words(4 * width)
    if rd.u32() != width:
        return 3
    nxt = rd.words(4 * width)
    if rd.u32() != C:
        return 3
    chunks = []
    for _ in range(C):
        if rd.u32() != 4:
            return 3
        chunks.append(rd.words(16))
    if rd.bad:
        return 4
    pis = np.asarray(pis, dtype=np.uint32).reshape(-1)
    ch = R.RefChallenger(kind)
    alpha = _prefix(ch, log_n, root_t, pis)
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    g_n = R.two_adic_generator(log_n)
    zeta_next = R.ext_scale(zeta, g_n)
    one, ginv = R.ext_from_base(R.ONE), R.ext_from_base(R.binv(g_n))
    zn = one
    for _ in range(n):  # zeta^n by n products: no shared power routine
        zn = R.ext_mul(zn, zeta)
    zh = R.ext_sub(zn, one)
    sels = [R.ext_mul(zh, R.ext_inv(R.ext_sub(zeta, one))), R.ext_mul(zh, R.ext_inv(R.ext_sub(zeta, ginv))), R.ext_sub(zeta, ginv)]
    folded = eval_ext(code, consts, local, nxt, pis, sels, alpha)
    shifts = chunk_shifts(log_n, lqd)
    quot = np.zeros(4, dtype=np.uint32)
    for c in range(C):
        zps = one
        for j in range(C):
            if j == c:
                continue
            sjn_inv = R.binv(R.bpow(shifts[j], n))  # Z_{D_j}(x) = (x / s_j)^n - 1
            num = R.ext_sub(R.ext_scale(zn, sjn_inv), one)
            den = R.ext_sub(R.ext_from_base(R.bmul(R.bpow(shifts[c], n), sjn_inv)), one)
            zps = R.ext_mul(zps, R.ext_mul(num, R.ext_inv(den)))
        val = np.zeros(4, dtype=np.uint32)
        for e in range(4):
            be = np.zeros(4, dtype=np.uint32)
            be[e] = R.ONE
            val = R.ext_add(val, R.ext_mul(be, chunks[c][4 * e:4 * e + 4]))
        quot = R.ext_add(quot, R.ext_mul(zps, val))
    if not np.array_equal(folded, R.ext_mul(quot, zh)):
        return 10
    opened = np.concatenate([local, nxt] + chunks).reshape(-1, 4)
    rounds = [((root_t, [width]), [[zeta, zeta_next]]), ((root_q, [4] * C), [[zeta]] * C)]
    return R.verify(kind, fp, log_n, rounds, opened, proof[4 * header_words(width, lqd):], ch)


# ---- the test AIRs: (A) fib is the package's fibonacci_air(); (B), (C) and (D) below ----
B_K, B_K2 = 7, 3
C_WIDTH = 70


def air_b(p3):
    """width 3 (x, y, z), publics (x0, y0, x_last), degree 3: next.x = x y + 7; next.y = y + 3 z; next.z = y + z; first row x = x0,
    y = y0; last row x = x_last"""
    b = p3.AirBuilder(3, 3)
    x, y, z = (b.local(c) for c in range(3))
    t = b.when_transition()
    t.assert_eq(b.next(0), x * y + b.const(B_K))
    t.assert_eq(b.next(1), y + z * b.const(B_K2))
    t.assert_eq(b.next(2), y + z)
    f = b.when_first_row()
    f.assert_eq(x, b.public(0))
    f.assert_eq(y, b.public(1))
    b.when_last_row().assert_eq(x, b.public(2))
    return b.build()


def trace_b(log_n, x0=5, y0=11, z0=2):
    """-> (trace as Montgomery words, public values as Montgomery words)"""
    rows, (x, y, z) = [], (x0 % P, y0 % P, z0 % P)
    for _ in range(1 << log_n):
        rows.append((x, y, z))
        x, y, z = (x * y + B_K) % P, (y + B_K2 * z) % P, (y + z) % P
    t = np.array(rows, dtype=np.uint64)
    return O.to_monty(t), O.to_monty(np.array([x0 % P, y0 % P, rows[-1][0]], dtype=np.uint64))


def air_c(p3):
    """width 70, public (s), degree 4: next[c] = (local[c] + local[(c + 1) % 70] + c + 1)^3 on every column; first row local[c] = s +
    c.  630 product / sum nodes: ten times as many as there are slots."""
    b = p3.AirBuilder(C_WIDTH, 1)
    t, f = b.when_transition(), b.when_first_row()
    for c in range(C_WIDTH):
        s = b.local(c) + b.local((c + 1) % C_WIDTH) + b.const(c + 1)
        t.assert_eq(b.next(c), s * s * s)
    for c in range(C_WIDTH):
        f.assert_eq(b.local(c), b.public(0) + b.const(c))
    return b.build()


def trace_c(log_n, s=9):
    row = [(s + c) % P for c in range(C_WIDTH)]
    rows = []
    for _ in range(1 << log_n):
        rows.append(row)
        row = [pow(row[c] + row[(c + 1) % C_WIDTH] + c + 1, 3, P) for c in range(C_WIDTH)]
    return O.to_monty(np.array(rows, dtype=np.uint64)), O.to_monty(np.array([s % P], dtype=np.uint64))


def air_d(p3):
    """width 2 (x, y), public (x0), degree 9 under the transition filter, 8 quotient chunks: next.x = x^8 + y (three squarings);
    next.y = y + x; first row x = x0"""
    b = p3.AirBuilder(2, 1)
    x, y = b.local(0), b.local(1)
    x2 = x * x
    x4 = x2 * x2
    t = b.when_transition()
    t.assert_eq(b.next(0), x4 * x4 + y)
    t.assert_eq(b.next(1), y + x)
    b.when_first_row().assert_eq(x, b.public(0))
    return b.build()


def trace_d(log_n, s=3, y0=5):
    rows, (x, y) = [], (s % P, y0 % P)
    for _ in range(1 << log_n):
        rows.append((x, y))
        x, y = (pow(x, 8, P) + y) % P, (y + x) % P
    return O.to_monty(np.array(rows, dtype=np.uint64)), O.to_monty(np.array([s % P], dtype=np.uint64))


def trace_fib(log_n, a=0, b=1):
    return O.generate_trace_rows(a, b, 1 << log_n), R.fib_pis(a, b, log_n)


def all_airs(p3):
    """-> {name: (Air, trace generator)}"""
    return {"fib": (p3.fibonacci_air(), trace_fib), "B": (air_b(p3), trace_b), "C": (air_c(p3), trace_c), "D": (air_d(p3), trace_d)}
