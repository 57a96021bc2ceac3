"""Python restatements the PCS tests compare the library with: the two challengers, extension-field helpers, polynomial
evaluation, and an independent verifier of TwoAdicFriPcs proofs following oracle/stark.c:216-294 generalised to any number of
rounds, matrices, widths and points.  Field and hash primitives come from the oracle (oracle/oracle.py): p3o_poseidon2_permute,
p3o_keccak256, p3o_ext_mul / p3o_ext_inv, p3o_mul / p3o_inv / p3o_pow, p3o_mmcs_verify_batch_kind.  Words are Montgomery words.
Only the bulk polynomial evaluation is numpy (canonical residues, uint64 products), cross-checked against p3o_ext_mul in the
tests that use it.

The second half is a reference PROVER: open() restates oracle/stark.c:71-154 for any number of rounds, matrices, widths and
points from the oracle's primitives (coset_lde_batch, mmcs_commit, idft_batch, the hashes) and numpy, so that the bytes of a
device open can be pinned on shapes other than the fib_air instance.  It knows nothing of the library."""
import ctypes as C

import numpy as np

from oracle import oracle as O

P = O.P
GEN = int(O.to_monty(31))
ONE = int(O.to_monty(1))


# ---- field ----
def _L():
    L = O.lib()
    if not getattr(L, "_pcs_ref_ready", False):
        L.p3o_ext_mul.argtypes = [O._u32p, O._u32p, O._u32p]
        L.p3o_ext_mul.restype = None
        L.p3o_ext_inv.argtypes = [O._u32p, O._u32p]
        L.p3o_ext_inv.restype = None
        L._pcs_ref_ready = True
    return L


def bmul(a, b):
    return int(_L().p3o_mul(int(a), int(b)))


def binv(a):
    return int(_L().p3o_inv(int(a)))


def bpow(a, e):
    return int(_L().p3o_pow(int(a), int(e)))


def two_adic_generator(bits):
    return int(_L().p3o_two_adic_generator(bits))


def ext(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(4).copy()


def ext_from_base(b):
    return np.array([int(b), 0, 0, 0], dtype=np.uint32)


def ext_add(a, b):
    return ((a.astype(np.uint64) + b) % P).astype(np.uint32)


def ext_sub(a, b):
    return ((a.astype(np.uint64) + P - b) % P).astype(np.uint32)


def ext_mul(a, b):
    a, b, out = ext(a), ext(b), np.zeros(4, dtype=np.uint32)
    _L().p3o_ext_mul(O._p(a), O._p(b), O._p(out))
    return out


def ext_inv(a):
    a, out = ext(a), np.zeros(4, dtype=np.uint32)
    _L().p3o_ext_inv(O._p(a), O._p(out))
    return out


def ext_scale(a, b):
    return ext_mul(a, ext_from_base(b))


def rev_bits(x, bits):
    y = 0
    for _ in range(bits):
        y = (y << 1) | (x & 1)
        x >>= 1
    return y


# ---- challengers (oracle/stark_common.h chal_*) ----
class RefChallenger:
    """kind 0: DuplexChallenger<BabyBear, Poseidon2-16, 16, 8>; kind 1: SerializingChallenger32 over HashChallenger<u8, Keccak256, 32>."""

    def __init__(self, kind):
        self.kind = kind
        self.state, self.inb, self.out = [0] * 16, [], []
        self.ibuf, self.obuf = bytearray(), bytearray()

    def _duplex(self):
        for i, v in enumerate(self.inb):
            self.state[i] = v
        self.inb = []
        self.state = [int(v) for v in O.poseidon2_permute(np.array(self.state, dtype=np.uint32))]
        self.out = self.state[:8]

    def observe(self, words):
        for v in np.asarray(words, dtype=np.uint32).reshape(-1):
            v = int(v)
            if self.kind:
                self.obuf = bytearray()
                self.ibuf += v.to_bytes(4, "little")
                continue
            self.out = []
            self.inb.append(v)
            if len(self.inb) == 8:
                self._duplex()

    observe_digest = observe

    def _sample(self):
        if self.kind:
            while True:
                v = 0
                for i in range(4):
                    if not self.obuf:
                        d = O.keccak256(bytes(self.ibuf))
                        self.obuf, self.ibuf = bytearray(d), bytearray(d)
                    v |= self.obuf.pop() << (8 * i)
                v &= 0x7FFFFFFF
                if v < P:
                    return int(O.to_monty(v))
        if self.inb or not self.out:
            self._duplex()
        return self.out.pop()

    def sample_ext(self):
        return np.array([self._sample() for _ in range(4)], dtype=np.uint32)

    def sample_bits(self, bits):
        return int(O.from_monty(self._sample())) & ((1 << bits) - 1)

    def clone(self):
        c = RefChallenger(self.kind)
        c.state, c.inb, c.out = list(self.state), list(self.inb), list(self.out)
        c.ibuf, c.obuf = bytearray(self.ibuf), bytearray(self.obuf)
        return c


# ---- polynomial evaluation ----
def _canon_ext_mul(a, b):
    """(…, 4) x (…, 4) canonical residues, x^4 = 11, numpy uint64."""
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.uint64)
    for i in range(4):
        for j in range(4):
            t = (a[..., i] * b[..., j]) % P
            if i + j >= 4:
                t = (t * 11) % P
            out[..., (i + j) % 4] = (out[..., (i + j) % 4] + t) % P
    return out


def eval_columns(coeffs, z):
    """Horner evaluation (in blocks of 256 coefficients) of every column of `coeffs` (n x w Montgomery words, degree ascending)
    at the extension point z (4 Montgomery words) -> (w, 4) Montgomery words."""
    c = O.from_monty(coeffs).astype(np.uint64)
    zc = O.from_monty(ext(z)).astype(np.uint64)
    n, w = c.shape
    B = min(n, 256)
    pw = np.zeros((B + 1, 4), dtype=np.uint64)
    pw[0, 0] = 1
    for i in range(1, B + 1):
        pw[i] = _canon_ext_mul(pw[i - 1], zc)
    acc = np.zeros((w, 4), dtype=np.uint64)
    for hi in range(n - B, -1, -B):  # acc = acc * z^B + block(z)
        blk = c[hi:hi + B]  # (B, w)
        val = np.zeros((w, 4), dtype=np.uint64)
        for k in range(4):
            val[:, k] = ((blk * pw[:B, k][:, None]) % P).sum(axis=0) % P
        acc = (_canon_ext_mul(acc, pw[B][None, :]) + val) % P
    return O.to_monty(acc)


def opened_value(evals, shift, z):
    """The value at z of the columns' interpolants: evals (h x w) over shift * <g_h>, natural order; p3o_idft_batch gives the
    coefficients of p(shift x), evaluated at z / shift."""
    co = O.idft_batch(evals)
    return eval_columns(co, ext_scale(z, binv(shift)))


# ---- proof bytes ----
class _Rd:
    def __init__(self, b):
        self.w = np.frombuffer(bytes(b[:len(b) // 4 * 4]), dtype=np.uint32)
        self.pos, self.bad, self.tail = 0, False, len(b) % 4

    def u32(self):
        if self.pos >= len(self.w):
            self.bad = True
            return 0
        self.pos += 1
        return int(self.w[self.pos - 1])

    def words(self, n, field=True):
        out = np.zeros(n, dtype=np.uint32)
        for i in range(n):
            out[i] = self.u32()
        if field and np.any(out >= P):
            self.bad = True
        return out


def verify(kind, fp, log_h, rounds, opened, proof, ch):
    """rounds = [((root, widths), points per matrix)]; fp = (log_blowup, log_final_poly_len, num_queries, pow_bits); ch a
    RefChallenger in the state before the opened values.  0 = accept, else the code of the failed check (stark.c numbering)."""
    log_blowup, lfp, nq, pow_bits = fp
    log_big = log_h + log_blowup
    opened = np.asarray(opened, dtype=np.uint32).reshape(-1, 4)
    ch.observe(opened)
    al = ch.sample_ext()
    alp = [ext_from_base(ONE)]
    for _ in range(1, len(opened)):
        alp.append(ext_mul(alp[-1], al))
    rd = _Rd(proof)
    n_rounds = rd.u32()
    if rd.bad or n_rounds != log_big - log_blowup - lfp:
        return 5
    digest = lambda n: rd.words(8 * n, field=(kind == 0)).reshape(n, 8)
    froots = digest(n_rounds)
    betas = []
    for r in range(n_rounds):
        ch.observe_digest(froots[r])
        betas.append(ch.sample_ext())
    if rd.u32() != nq:
        return 6
    qstart = rd.pos
    qwords = 1 + sum(1 + sum(1 + w for w in ws) + 1 + 8 * log_big for (_, ws), _ in rounds) + 1 + sum(4 + 1 + 8 * (log_big - 1 - r) for r in range(n_rounds))
    rd.pos += qwords * nq
    fpl = rd.u32()
    if rd.bad or fpl != (1 << lfp):
        return 7
    fpoly = rd.words(4 * fpl).reshape(fpl, 4)
    ch.observe(fpoly)
    witness = rd.u32()
    if rd.bad or witness >= P or rd.pos != len(rd.w) or rd.tail:
        return 8
    ch.observe([witness])
    if ch.sample_bits(pow_bits) != 0:
        return 11
    rd.pos = qstart
    g_big = two_adic_generator(log_big)
    for _ in range(nq):
        index = ch.sample_bits(log_big)
        if rd.u32() != len(rounds):
            return 12
        xi = bmul(GEN, bpow(g_big, rev_bits(index, log_big)))
        ro, k = np.zeros(4, dtype=np.uint32), 0
        for ((root, ws), mpoints) in rounds:
            if rd.u32() != len(ws):
                return 12
            rows = []
            for w in ws:
                if rd.u32() != w:
                    return 12
                rows.append(rd.words(w))
            if rd.u32() != log_big:
                return 12
            path = digest(log_big)
            if rd.bad:
                return 9
            if not O.mmcs_verify_batch(root, [(1 << log_big, w) for w in ws], index, np.concatenate(rows), path, kind=kind):
                return 13
            for row, pts in zip(rows, mpoints):
                for z in pts:
                    dz = ext_inv(ext_sub(ext(z), ext_from_base(xi)))
                    for c in range(len(row)):
                        ro = ext_add(ro, ext_mul(alp[k], ext_mul(ext_sub(opened[k], ext_from_base(row[c])), dz)))
                        k += 1
        if rd.u32() != n_rounds:
            return 12
        folded, idx = ro, index
        for r in range(n_rounds):
            lfh = log_big - 1 - r
            sib = rd.words(4)
            if rd.u32() != lfh:
                return 12
            path = digest(lfh)
            if rd.bad:
                return 9
            ev = [None, None]
            ev[idx & 1], ev[(idx & 1) ^ 1] = folded, sib
            pair = idx >> 1
            if not O.mmcs_verify_batch(froots[r], [(1 << lfh, 8)], pair, np.concatenate(ev), path, kind=kind):
                return 14
            s = bpow(two_adic_generator(lfh + 1), rev_bits(pair, lfh))
            num = ext_mul(ext_sub(betas[r], ext_from_base(s)), ext_sub(ev[1], ev[0]))
            folded = ext_add(ev[0], ext_scale(num, binv((2 * (P - s)) % P)))
            idx = pair
        lfin = log_blowup + lfp
        xf = bpow(two_adic_generator(lfin), rev_bits(idx, lfin))
        acc = np.zeros(4, dtype=np.uint32)
        for i in range(fpl - 1, -1, -1):
            acc = ext_add(ext_scale(acc, xf), fpoly[i])
        if not np.array_equal(acc, folded):
            return 15
    return 0


# ---- the fib_air proof of the oracle (stark.c:130-154) taken apart ----
def split_fib_proof(proof):
    """-> (log_n, root_t, root_q, opened (8, 4) in observation order, FriProof bytes)."""
    w = np.frombuffer(proof, dtype=np.uint32)
    assert w[0] == 0x42463350 and w[1] == 1 and w[19] == 2 and w[28] == 2 and w[37] == 1 and w[38] == 4
    opened = np.concatenate([w[20:28], w[29:37], w[39:55]]).reshape(8, 4).copy()
    return int(w[2]), w[3:11].copy(), w[11:19].copy(), opened, bytes(proof[55 * 4:])


def fib_header(log_n, root_t, root_q, opened):
    o = np.asarray(opened, dtype=np.uint32).reshape(-1)
    u = lambda *v: np.array(v, dtype=np.uint32)
    return np.concatenate([u(0x42463350, 1, log_n), root_t, root_q, u(2), o[:8], u(2), o[8:16], u(1, 4), o[16:32]]).astype(np.uint32).tobytes()


def fib_prefix(ch, log_n, root_t, pis, root_q):
    """p3_uni_stark's transcript up to the PCS (stark.c:37-42, 68-70): -> (alpha, zeta, zeta * g_n)."""
    ch.observe([int(O.to_monty(log_n))] * 2)
    ch.observe_digest(root_t)
    ch.observe(pis)
    alpha = ch.sample_ext()
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    return alpha, zeta, ext_scale(zeta, two_adic_generator(log_n))


def fib_pis(a, b, log_n):
    return O.to_monty(np.array([a % P, b % P, O.fib_public_x(a, b, 1 << log_n)], dtype=np.uint64))


# ---- the fib_air quotient (stark.c:44-60), for driving the instance through a PCS ----
def _npow(a, e):
    r, a = np.ones_like(a), a.copy()
    while e:
        if e & 1:
            r = (r * a) % P
        a = (a * a) % P
        e >>= 1
    return r


def _bitrev(log_n):
    i = np.arange(1 << log_n)
    r = np.zeros_like(i)
    for b in range(log_n):
        r |= ((i >> b) & 1) << (log_n - 1 - b)
    return r


def fib_quotient(lde_low, log_n, pis, alpha):
    """quotient_values on GENERATOR * <g_n> (stark.c:44-60) in canonical numpy integers -> n x 4 Montgomery words, natural order"""
    n = 1 << log_n
    t = O.from_monty(lde_low).astype(np.uint64)[_bitrev(log_n)]  # natural order
    loc, nxt = t, np.roll(t, -1, axis=0)
    pc = [int(v) for v in O.from_monty(pis)]
    g = int(O.from_monty(two_adic_generator(log_n)))
    ginv = pow(g, P - 2, P)
    x = np.zeros(n, dtype=np.uint64)
    acc = 31
    for i in range(n):
        x[i] = acc
        acc = acc * g % P
    zh = (pow(31, n, P) - 1) % P
    zh_inv = pow(zh, P - 2, P)
    first = zh * _npow((x + P - 1) % P, P - 2) % P
    last = zh * _npow((x + P - ginv) % P, P - 2) % P
    trans = (x + P - ginv) % P
    c = [first * ((loc[:, 0] + P - pc[0]) % P) % P, first * ((loc[:, 1] + P - pc[1]) % P) % P,
         trans * ((loc[:, 1] + P - nxt[:, 0]) % P) % P, trans * ((loc[:, 0] + loc[:, 1] + P - nxt[:, 1]) % P) % P,
         last * ((loc[:, 1] + P - pc[2]) % P) % P]
    apow = [ext_from_base(ONE)]
    for _ in range(4):
        apow.append(ext_mul(apow[-1], alpha))
    ap = [O.from_monty(a).astype(np.uint64) for a in apow]
    q = np.zeros((n, 4), dtype=np.uint64)
    for k in range(5):  # the first constraint takes the highest power (stark_common.h fib_fold_base)
        q = (q + c[k][:, None] * ap[4 - k][None, :]) % P
    return O.to_monty(q * zh_inv % P)


# ---- reference prover (stark.c:71-154 for any shape) ----
def _canon_ext_inv(a):
    """(…, 4) canonical residues, nonzero -> inverses.  With Y = X^2: a = A + B X, A and B in F_p[Y]/(Y^2 - 11); a conj(a) = A^2 -
    Y B^2 = D lies in F_p[Y], D conj_Y(D) = n lies in F_p, so 1/a = conj(a) conj_Y(D) / n."""
    a = a.astype(np.uint64)
    conj = a.copy()
    conj[..., 1], conj[..., 3] = (P - a[..., 1]) % P, (P - a[..., 3]) % P
    d = _canon_ext_mul(a, conj)  # coordinates 1 and 3 vanish
    dbar = d.copy()
    dbar[..., 2] = (P - d[..., 2]) % P
    n = _canon_ext_mul(d, dbar)[..., 0]
    return _canon_ext_mul(_canon_ext_mul(conj, dbar), _npow(n, P - 2)[..., None] * np.array([1, 0, 0, 0], dtype=np.uint64))


def _geom(q, n):
    """[q^0 .. q^(n-1)] canonical, by doubling"""
    out, step = np.ones(1, dtype=np.uint64), int(q) % P
    while out.size < n:
        out = np.concatenate([out, out * np.uint64(step) % P])
        step = step * step % P
    return out[:n]


def _ext_powers(al, n):
    """[al^0 .. al^(n-1)] of a canonical extension element, by doubling -> (n, 4)"""
    out = np.array([[1, 0, 0, 0]], dtype=np.uint64)
    step = al.astype(np.uint64)
    while len(out) < n:
        out = np.concatenate([out, _canon_ext_mul(out, step[None, :])])
        step = _canon_ext_mul(step, step)
    return out[:n]


def commit(kind, log_blowup, mats):
    """Pcs::commit (stark.c:31-36, 62-67): mats = [(evals h x w, shift or None)] -> (root, oracle Tree, [LDE])"""
    ldes = [O.coset_lde_batch(m, log_blowup, GEN if s is None else bmul(GEN, binv(s)), True) for m, s in mats]
    root, tree = O.mmcs_commit(ldes, kind)
    return root, tree, ldes


def _fold(v, beta, one_half):
    """fold_matrix (stark_common.h): v (len, 4) canonical, bit-reversed pairs -> (len / 2, 4)"""
    half = len(v) // 2
    lh = half.bit_length() - 1
    ginv = pow(int(O.from_monty(two_adic_generator(lh + 1))), P - 2, P)
    hb = beta.astype(np.uint64) * np.uint64(one_half) % P
    power = _geom(ginv, half)[_bitrev(lh)][:, None] * hb[None, :] % P
    oh = np.array([one_half, 0, 0, 0], dtype=np.uint64)
    return (_canon_ext_mul((oh + power) % P, v[0::2]) + _canon_ext_mul((oh + P - power) % P, v[1::2])) % P


def open_with_roots(kind, fp, log_h, rounds, ch):
    """-> (opened (n, 4) Montgomery words in observation order, FriProof bytes, [root of each round]); see open."""
    log_blowup, lfp, nq, pow_bits = fp
    log_big = log_h + log_blowup
    big = 1 << log_big
    com = [commit(kind, log_blowup, [(m, s) for m, s, _ in mats]) for mats in rounds]
    # opened values, observed round -> matrix -> point -> column (stark.c:72-78); the batching challenge (:79-80)
    opened = [opened_value(m, ONE if s is None else s, z) for mats in rounds for m, s, pts in mats for z in pts]
    opened = np.concatenate(opened).reshape(-1, 4)
    ch.observe(opened)
    alp = _ext_powers(O.from_monty(ch.sample_ext()), len(opened))
    opc = O.from_monty(opened).astype(np.uint64)
    # reduced openings over GENERATOR * <g_big>, bit-reversed (:82-100): every (matrix, point) pair takes `width` powers
    g_big = int(O.from_monty(two_adic_generator(log_big)))
    x = np.zeros((big, 4), dtype=np.uint64)
    x[:, 0] = (_geom(g_big, big) * np.uint64(31) % P)[_bitrev(log_big)]
    ro, k = np.zeros((big, 4), dtype=np.uint64), 0
    for (_, _, ldes), mats in zip(com, rounds):
        for lde, (_, _, pts) in zip(ldes, mats):
            v, w = O.from_monty(lde).astype(np.uint64), lde.shape[1]
            for z in pts:
                a = alp[k:k + w]
                y = _canon_ext_mul(a, opc[k:k + w]).sum(axis=0) % P
                s = np.stack([(v * a[:, c][None, :] % P).sum(axis=1) % P for c in range(4)], axis=1)
                dz = _canon_ext_inv((O.from_monty(ext(z)).astype(np.uint64)[None, :] + P - x) % P)
                ro = (ro + _canon_ext_mul((y[None, :] + P - s) % P, dz)) % P
                k += w
    # FRI commit phase (:102-119): each layer committed as rows of two extension elements
    n_fr = log_h - lfp
    one_half = pow(2, P - 2, P)
    folded, ftrees, froots = ro, [], []
    for _ in range(n_fr):
        root, tree = O.mmcs_commit([O.to_monty(folded).reshape(len(folded) // 2, 8)], kind)
        ftrees.append(tree)
        froots.append(root)
        ch.observe_digest(root)
        folded = _fold(folded, O.from_monty(ch.sample_ext()), one_half)
    # final polynomial (:120-127), proof of work (:128, chal_grind: the smallest witness)
    fpl = 1 << lfp
    fpoly = O.idft_batch(O.to_monty(folded[_bitrev(lfp)]))
    ch.observe(fpoly)
    for i in range(P):
        t, wit = ch.clone(), int(O.to_monty(i))
        t.observe([wit])
        if t.sample_bits(pow_bits) == 0:
            break
    ch.observe([wit])
    ch.sample_bits(pow_bits)
    # serialise (:135-154)
    u = lambda *vals: np.array(vals, dtype=np.uint32)
    out = [u(n_fr)] + froots + [u(nq)]
    for _ in range(nq):
        index = ch.sample_bits(log_big)
        out.append(u(len(rounds)))
        for (_, tree, ldes) in com:
            rows, path = tree.open_batch(index)
            out.append(u(len(ldes)))
            pos = 0
            for lde in ldes:
                out += [u(lde.shape[1]), rows[pos:pos + lde.shape[1]]]
                pos += lde.shape[1]
            out += [u(log_big), path.reshape(-1)]
        out.append(u(n_fr))
        for r in range(n_fr):
            idx = index >> r
            rows, path = ftrees[r].open_batch(idx >> 1)
            out += [rows[4 * ((idx ^ 1) & 1):][:4], u(log_big - 1 - r), path.reshape(-1)]
    out += [u(fpl), fpoly.reshape(-1), u(wit)]
    return opened, np.concatenate([np.asarray(o, dtype=np.uint32).reshape(-1) for o in out]).tobytes(), [c[0] for c in com]


def open(kind, fp, log_h, rounds, ch):
    """TwoAdicFriPcs::open restated: rounds = [[(evals h x w Montgomery words, domain shift or None, [points])]], fp = (log_blowup,
    log_final_poly_len, num_queries, pow_bits), ch a RefChallenger in the caller's state, advanced to the state after the last query
    index.  -> (opened values, FriProof bytes).  A matrix may have no point; some matrix must have one."""
    return open_with_roots(kind, fp, log_h, rounds, ch)[:2]


def verifier_rounds(roots, rounds):
    """what verify() and the library's verifier take, from the prover's rounds and roots"""
    return [((root, [m.shape[1] for m, _, _ in mats]), [pts for _, _, pts in mats]) for root, mats in zip(roots, rounds)]


# ---- seeded shapes shared by the CPU and the GPU tests ----
WIDTHS = list(range(1, 49)) + [63, 64, 65, 128, 129]


def rand_matrix(rng, log_h, w):
    return O.to_monty(rng.integers(0, P, (1 << log_h, w), dtype=np.uint64))


def rand_point(rng):
    return O.to_monty(rng.integers(0, P, 4, dtype=np.uint64))


def rand_shift(rng):
    return int(O.to_monty(int(rng.integers(1, P))))


def random_case(rng, log_h, max_cols=600):
    """1-4 rounds of 1-8 matrices, widths from WIDTHS, 0-4 points per matrix drawn WITH repeats from a pool of 1-4 (one of them
    sometimes the base-field point 1, which no LDE coset holds), random domain shifts; at most max_cols batched columns: a
    matrix that would pass the limit loses points."""
    pool = [rand_point(rng) for _ in range(int(rng.integers(1, 5)))]
    if rng.integers(0, 3) == 0:
        pool[0] = ext_from_base(ONE)
    rounds, total = [], 0
    for _ in range(int(rng.integers(1, 5))):
        mats = []
        for _ in range(int(rng.integers(1, 9))):
            w = WIDTHS[int(rng.integers(0, len(WIDTHS)))]
            pts = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(0, 5)))]
            while pts and total + w * len(pts) > max_cols:
                pts.pop()
            total += w * len(pts)
            mats.append((rand_matrix(rng, log_h, w), rand_shift(rng) if rng.integers(0, 4) else None, pts))
        rounds.append(mats)
    if total == 0:  # an open needs a point somewhere
        m, s, _ = rounds[-1][-1]
        rounds[-1][-1] = (m, s, [pool[0]])
    return rounds


def empty_point_case(rng, log_h, widths=(3, 17, 5)):
    """first matrix, last matrix and a whole middle round without points (2(c) of the issue)"""
    z0, z1 = rand_point(rng), rand_point(rng)
    mk = lambda w, pts, s=None: (rand_matrix(rng, log_h, w), s, pts)
    return [[mk(widths[0], []), mk(widths[1], [z0, z1], rand_shift(rng))], [mk(widths[2], []), mk(widths[0], [])],
            [mk(widths[1], [z1]), mk(widths[2], [z0], rand_shift(rng)), mk(widths[0], [])]]


def repeated_point_case(rng, log_h, widths=(2, 17)):
    """the same point twice in one matrix's list, and again on another matrix"""
    z0, z1 = rand_point(rng), rand_point(rng)
    return [[(rand_matrix(rng, log_h, widths[0]), None, [z0, z0]), (rand_matrix(rng, log_h, widths[1]), rand_shift(rng), [z1, z0, z1])]]


def four_point_case(rng, log_h, w):
    """four distinct points on one matrix of width w, and a second matrix at the last of them"""
    pts = [rand_point(rng) for _ in range(3)] + [ext_from_base(ONE)]
    return [[(rand_matrix(rng, log_h, w), rand_shift(rng), pts), (rand_matrix(rng, log_h, 3), None, [pts[3], pts[0]])]]
