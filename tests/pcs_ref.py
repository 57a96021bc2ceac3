"""Python restatements the PCS tests compare the library with: the two challengers, extension-field helpers, polynomial
evaluation, and an independent verifier of TwoAdicFriPcs proofs following oracle/stark.c:216-294 generalised to any number of
rounds, matrices, widths and points.  Field and hash primitives come from the oracle (oracle/oracle.py): p3o_poseidon2_permute,
p3o_keccak256, p3o_ext_mul / p3o_ext_inv, p3o_mul / p3o_inv / p3o_pow, p3o_mmcs_verify_batch_kind.  Words are Montgomery words.
Only the bulk polynomial evaluation is numpy (canonical residues, uint64 products), cross-checked against p3o_ext_mul in the
tests that use it."""
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
