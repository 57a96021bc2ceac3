"""Reference prover and verifier of HidingFriPcs over caller matrices: oracle/stark_hiding.c:94-295 (prover) and :380-457 (verifier)
restated for any number of rounds, matrices, widths, points, random codewords NRC and C in {2, 4} quotient chunks, from tests/pcs_ref.py
and the oracle's primitives (rng_seed_from_u64, rng_fill_field, coset_lde_batch, idft_batch, coset_dft_batch, mmcs_commit with the salts
as matrices) and numpy.  It knows nothing of the library.

Conventions (h = 2^log_h the caller's height, h2 = 2 h, big = h2 << log_blowup, SALT = 4):
  streams   `mmcs` and `fri` from mmcs_seed, `pcs` from pcs_seed; they advance from call to call
  commit    matrix m (h x w), in input order: h (w + 2 NRC) draws of `pcs` row by row; rows 2i = evals[i] || d[:NRC], 2i+1 = d[NRC:];
            LDE = coset_lde_batch(., log_blowup, GENERATOR / shift), bit-reversed; then per matrix a big x 4 salt of `mmcs`; one tree
            over m0, s0, m1, s1, ...
  quotient  chunk c on s_c <g_h>, s_c = GENERATOR g_(C h)^c; t_c (c < C - 1) h x wq draws of `pcs`, the last cancels them
  random    h2 x (NRC + 4) draws of `pcs`, committed like a trace
  open      every committed column, over h2 rows; FRI layers salted from `fri`; BatchOpening = values, salts, path"""
import numpy as np

import pcs_ref as R
from oracle import oracle as O

P, GEN, ONE, SALT = R.P, R.GEN, R.ONE, 4
_u = lambda *vals: np.array(vals, dtype=np.uint32)


class Commitment:
    def __init__(self, root, tree, ldes, salts):
        self.root, self.tree, self.ldes, self.salts = root, tree, ldes, salts

    @property
    def widths(self):
        return [l.shape[1] for l in self.ldes]


def _log2(n):
    assert n > 0 and n & (n - 1) == 0
    return n.bit_length() - 1


class HidingPcs:
    def __init__(self, kind, fp, nrc=4, mmcs_seed=1, pcs_seed=1):
        self.kind, self.fp, self.nrc = kind, tuple(fp), nrc
        self.mmcs, self.fri, self.pcs = O.rng_seed_from_u64(mmcs_seed), O.rng_seed_from_u64(mmcs_seed), O.rng_seed_from_u64(pcs_seed)

    def _salted(self, ldes):
        """stark_hiding.c:50-63"""
        salts = [O.rng_fill_field(self.mmcs, len(l) * SALT).reshape(len(l), SALT) for l in ldes]
        root, tree = O.mmcs_commit([m for pair in zip(ldes, salts) for m in pair], self.kind)
        return Commitment(root, tree, ldes, salts)

    def commit(self, mats):
        """mats = [(evals h x w, domain shift or None)]; stark_hiding.c:105-124"""
        ldes = []
        for m, s in mats:
            h, w = m.shape
            d = O.rng_fill_field(self.pcs, h * (w + 2 * self.nrc)).reshape(h, w + 2 * self.nrc)
            rt = np.concatenate([np.asarray(m, dtype=np.uint32), d], axis=1).reshape(2 * h, w + self.nrc)
            ldes.append(O.coset_lde_batch(rt, self.fp[0], GEN if s is None else R.bmul(GEN, R.binv(s)), True))
        return self._salted(ldes)

    def commit_quotient(self, chunks):
        """chunks: C matrices h x wq, chunk c on GENERATOR g_(C h)^c <g_h>; stark_hiding.c:152-188"""
        C = len(chunks)
        h, wq = chunks[0].shape
        log_h, log_c = _log2(h), _log2(C)
        big = (2 * h) << self.fp[0]
        gq = R.two_adic_generator(log_h + log_c)
        s = [R.bmul(GEN, R.bpow(gq, c)) for c in range(C)]
        sh = [int(O.from_monty(R.bpow(sc, h))) for sc in s]
        kc = []
        for c in range(C):
            k = 1
            for j in range(C):
                if j != c:
                    k = k * ((sh[c] - sh[j]) % P) % P
            kc.append(k)
        t = [O.from_monty(O.rng_fill_field(self.pcs, h * wq)).astype(np.uint64).reshape(h, wq) for _ in range(C - 1)]
        acc = np.zeros((h, wq), dtype=np.uint64)
        for c in range(C - 1):
            acc = (acc + t[c] * np.uint64(pow(kc[c], P - 2, P))) % P
        t.append((P - acc * np.uint64(kc[C - 1]) % P) % P)
        ldes = []
        for c in range(C):
            co = O.from_monty(O.idft_batch(np.asarray(chunks[c], dtype=np.uint32))).astype(np.uint64)  # coefficients of q_c(s_c X)
            spw = R._geom(pow(int(O.from_monty(s[c])), P - 2, P), h)[:, None]
            ext = np.zeros((big, wq), dtype=np.uint64)
            ext[:h] = (co * spw % P + P - t[c] * np.uint64(sh[c]) % P) % P
            ext[h:2 * h] = t[c]
            nat = O.coset_dft_batch(O.to_monty(ext), GEN)
            ldes.append(O.bit_reverse_rows(nat))
        return self._salted(ldes)

    def commit_randomization(self, log_h):
        """stark_hiding.c:190-194"""
        h2, w = 2 << log_h, self.nrc + 4
        rm = O.rng_fill_field(self.pcs, h2 * w).reshape(h2, w)
        return self._salted([O.coset_lde_batch(rm, self.fp[0], GEN, True)])

    def open(self, rounds, ch):
        """rounds = [(Commitment, [points of matrix 0, ...])]; ch a RefChallenger, advanced to the state after the last query index.
        -> (opened (n, 4) in observation order, FriProof bytes).  stark_hiding.c:198-285"""
        log_blowup, lfp, nq, pow_bits = self.fp
        kind = self.kind
        big = len(rounds[0][0].ldes[0])
        log_big = _log2(big)
        log_h2 = log_big - log_blowup
        h2 = 1 << log_h2
        ginv = R.binv(GEN)
        opened = []
        for com, mpts in rounds:
            assert len(mpts) == len(com.ldes)
            for lde, pts in zip(com.ldes, mpts):
                assert len(lde) == big
                if pts:
                    co = O.idft_batch(lde[:h2][R._bitrev(log_h2)])  # coefficients of p(GENERATOR X)
                    opened += [R.eval_columns(co, R.ext_scale(z, ginv)) for z in pts]
        opened = np.concatenate(opened).reshape(-1, 4)
        ch.observe(opened)
        alp = R._ext_powers(O.from_monty(ch.sample_ext()), len(opened))
        opc = O.from_monty(opened).astype(np.uint64)
        g_big = int(O.from_monty(R.two_adic_generator(log_big)))
        x = np.zeros((big, 4), dtype=np.uint64)
        x[:, 0] = (R._geom(g_big, big) * np.uint64(31) % P)[R._bitrev(log_big)]
        ro, k = np.zeros((big, 4), dtype=np.uint64), 0
        for com, mpts in rounds:
            for lde, pts in zip(com.ldes, mpts):
                v, w = O.from_monty(lde).astype(np.uint64), lde.shape[1]
                for z in pts:
                    a = alp[k:k + w]
                    y = R._canon_ext_mul(a, opc[k:k + w]).sum(axis=0) % P
                    s = np.stack([(v * a[:, c][None, :] % P).sum(axis=1) % P for c in range(4)], axis=1)
                    dz = R._canon_ext_inv((O.from_monty(R.ext(z)).astype(np.uint64)[None, :] + P - x) % P)
                    ro = (ro + R._canon_ext_mul((y[None, :] + P - s) % P, dz)) % P
                    k += w
        n_fr = log_h2 - lfp
        one_half = pow(2, P - 2, P)
        folded, ftrees, froots = ro, [], []
        for _ in range(n_fr):
            half = len(folded) // 2
            salt = O.rng_fill_field(self.fri, half * SALT).reshape(half, SALT)
            root, tree = O.mmcs_commit([O.to_monty(folded).reshape(half, 8), salt], kind)
            ftrees.append(tree)
            froots.append(root)
            ch.observe_digest(root)
            folded = R._fold(folded, O.from_monty(ch.sample_ext()), one_half)
        fpl = 1 << lfp
        fpoly = O.idft_batch(O.to_monty(folded[R._bitrev(lfp)]))
        ch.observe(fpoly)
        for i in range(P):
            t, wit = ch.clone(), int(O.to_monty(i))
            t.observe([wit])
            if t.sample_bits(pow_bits) == 0:
                break
        ch.observe([wit])
        ch.sample_bits(pow_bits)
        out = [_u(n_fr)] + froots + [_u(nq)]
        for _ in range(nq):
            index = ch.sample_bits(log_big)
            out.append(_u(len(rounds)))
            for com, _ in rounds:
                _, path = com.tree.open_batch(index)
                out.append(_u(len(com.ldes)))
                for lde in com.ldes:
                    out += [_u(lde.shape[1]), lde[index]]
                for salt in com.salts:
                    out += [_u(SALT), salt[index]]
                out += [_u(log_big), path.reshape(-1)]
            out.append(_u(n_fr))
            for r in range(n_fr):
                idx = index >> r
                rows, path = ftrees[r].open_batch(idx >> 1)
                out += [rows[4 * ((idx ^ 1) & 1):][:4], _u(SALT), rows[8:8 + SALT], _u(log_big - 1 - r), path.reshape(-1)]
        out += [_u(fpl), fpoly.reshape(-1), _u(wit)]
        return opened, np.concatenate([np.asarray(o, dtype=np.uint32).reshape(-1) for o in out]).tobytes()


def verifier_rounds(rounds):
    """what verify() and the library's verifier take: [((root, committed widths), points per matrix)]"""
    return [((com.root, com.widths), mpts) for com, mpts in rounds]


def verify(kind, fp, log_h, rounds, opened, proof, ch):
    """HidingFriPcs::verify restated (stark_hiding.c:380-457 for any shape); log_h the caller's log height; arguments and codes as
    pcs_ref.verify."""
    log_blowup, lfp, nq, pow_bits = fp
    log_big = log_h + 1 + log_blowup
    opened = np.asarray(opened, dtype=np.uint32).reshape(-1, 4)
    ch.observe(opened)
    al = ch.sample_ext()
    alp = [R.ext_from_base(ONE)]
    for _ in range(1, len(opened)):
        alp.append(R.ext_mul(alp[-1], al))
    rd = R._Rd(proof)
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
    qwords = (1 + sum(1 + sum(1 + w + 1 + SALT for w in ws) + 1 + 8 * log_big for (_, ws), _ in rounds) + 1 +
              sum(4 + 1 + SALT + 1 + 8 * (log_big - 1 - r) for r in range(n_rounds)))
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
    g_big = R.two_adic_generator(log_big)
    for _ in range(nq):
        index = ch.sample_bits(log_big)
        if rd.u32() != len(rounds):
            return 12
        xi = R.bmul(GEN, R.bpow(g_big, R.rev_bits(index, log_big)))
        ro, k = np.zeros(4, dtype=np.uint32), 0
        for ((root, ws), mpoints) in rounds:
            if rd.u32() != len(ws):
                return 12
            rows, salts = [], []
            for w in ws:
                if rd.u32() != w:
                    return 12
                rows.append(rd.words(w))
            for _ in ws:
                if rd.u32() != SALT:
                    return 12
                salts.append(rd.words(SALT))
            if rd.u32() != log_big:
                return 12
            path = digest(log_big)
            if rd.bad:
                return 9
            leaf = np.concatenate([p for pair in zip(rows, salts) for p in pair])
            dims = [d for w in ws for d in ((1 << log_big, w), (1 << log_big, SALT))]
            if not O.mmcs_verify_batch(root, dims, index, leaf, path, kind=kind):
                return 13
            for row, pts in zip(rows, mpoints):
                for z in pts:
                    dz = R.ext_inv(R.ext_sub(R.ext(z), R.ext_from_base(xi)))
                    for c in range(len(row)):
                        ro = R.ext_add(ro, R.ext_mul(alp[k], R.ext_mul(R.ext_sub(opened[k], R.ext_from_base(row[c])), dz)))
                        k += 1
        if rd.u32() != n_rounds:
            return 12
        folded, idx = ro, index
        for r in range(n_rounds):
            lfh = log_big - 1 - r
            sib = rd.words(4)
            if rd.u32() != SALT:
                return 12
            salt = rd.words(SALT)
            if rd.u32() != lfh:
                return 12
            path = digest(lfh)
            if rd.bad:
                return 9
            ev = [None, None]
            ev[idx & 1], ev[(idx & 1) ^ 1] = folded, sib
            pair = idx >> 1
            if not O.mmcs_verify_batch(froots[r], [(1 << lfh, 8), (1 << lfh, SALT)], pair, np.concatenate(ev + [salt]), path, kind=kind):
                return 14
            s = R.bpow(R.two_adic_generator(lfh + 1), R.rev_bits(pair, lfh))
            num = R.ext_mul(R.ext_sub(betas[r], R.ext_from_base(s)), R.ext_sub(ev[1], ev[0]))
            folded = R.ext_add(ev[0], R.ext_scale(num, R.binv((2 * (P - s)) % P)))
            idx = pair
        lfin = log_blowup + lfp
        xf = R.bpow(R.two_adic_generator(lfin), R.rev_bits(idx, lfin))
        acc = np.zeros(4, dtype=np.uint32)
        for i in range(fpl - 1, -1, -1):
            acc = R.ext_add(R.ext_scale(acc, xf), fpoly[i])
        if not np.array_equal(acc, folded):
            return 15
    return 0


# ---- the oracle's hiding fib_air proof (stark_hiding.c:257-285) taken apart, and the instance driven through a hiding PCS ----
FIB_NRC, FIB_D = 4, 4
_RW, _TW = FIB_NRC + FIB_D, 2 + FIB_NRC
FIB_HEADER_WORDS = 27 + 1 + 4 * _RW + 2 * (1 + 4 * _TW) + 1 + 4 * (1 + 4 * FIB_D)


def split_fib_proof(proof):
    """-> (log_n, root_t, root_q, root_r, opened (36, 4) in observation order: random, trace @ zeta, trace @ zeta g, chunks; FriProof bytes)"""
    w = np.frombuffer(proof, dtype=np.uint32)
    assert w[0] == 0x42463350 and w[1] == 2
    pos, parts = 27, []

    def take(n):
        nonlocal pos
        assert w[pos] == n, (pos, int(w[pos]), n)
        parts.append(w[pos + 1:pos + 1 + 4 * n])
        pos += 1 + 4 * n
    take(_RW), take(_TW), take(_TW)
    assert w[pos] == 4
    pos += 1
    for _ in range(4):
        take(FIB_D)
    assert pos == FIB_HEADER_WORDS
    return int(w[2]), w[3:11].copy(), w[11:19].copy(), w[19:27].copy(), np.concatenate(parts).reshape(-1, 4).copy(), bytes(proof[4 * pos:])


def fib_header(log_n, root_t, root_q, root_r, opened):
    o = np.asarray(opened, dtype=np.uint32).reshape(-1)
    parts = [_u(0x42463350, 2, log_n), root_t, root_q, root_r, _u(_RW), o[:4 * _RW]]
    pos = 4 * _RW
    for _ in range(2):
        parts += [_u(_TW), o[pos:pos + 4 * _TW]]
        pos += 4 * _TW
    parts.append(_u(4))
    for _ in range(4):
        parts += [_u(FIB_D), o[pos:pos + 4 * FIB_D]]
        pos += 4 * FIB_D
    assert pos == o.size
    return np.concatenate(parts).astype(np.uint32).tobytes()


def fib_begin(ch, log_n, root_t, pis):
    """stark_hiding.c:126-130 -> alpha"""
    ch.observe([int(O.to_monty(log_n + 1)), int(O.to_monty(log_n))])
    ch.observe_digest(root_t)
    ch.observe(pis)
    return ch.sample_ext()


def fib_zeta(ch, log_n, root_q, root_r):
    """stark_hiding.c:189-197 -> (zeta, zeta g_h)"""
    ch.observe_digest(root_q)
    ch.observe_digest(root_r)
    zeta = ch.sample_ext()
    return zeta, R.ext_scale(zeta, R.two_adic_generator(log_n))


def fib_quotient_chunks(lde_low, log_n, pis, alpha):
    """stark_hiding.c:131-151 in canonical numpy integers: lde_low = the first 4h rows of the randomized trace's bit-reversed LDE (any
    width >= 2: the trace's own columns come first) -> the four chunk matrices, h x 4 Montgomery words, natural order"""
    h, qn, log_q = 1 << log_n, 4 << log_n, log_n + 2
    t = O.from_monty(np.asarray(lde_low, dtype=np.uint32)[:, :2]).astype(np.uint64)[R._bitrev(log_q)]  # natural order
    loc, nxt = t, np.roll(t, -4, axis=0)
    pc = [int(v) for v in O.from_monty(pis)]
    ginv = pow(int(O.from_monty(R.two_adic_generator(log_n))), P - 2, P)
    x = R._geom(int(O.from_monty(R.two_adic_generator(log_q))), qn) * np.uint64(31) % P
    zh = (R._npow(x, h) + P - 1) % P
    first = zh * R._npow((x + P - 1) % P, P - 2) % P
    last = zh * R._npow((x + P - ginv) % P, P - 2) % P
    trans = (x + P - ginv) % P
    c = [first * ((loc[:, 0] + P - pc[0]) % P) % P, first * ((loc[:, 1] + P - pc[1]) % P) % P,
         trans * ((loc[:, 1] + P - nxt[:, 0]) % P) % P, trans * ((loc[:, 0] + loc[:, 1] + P - nxt[:, 1]) % P) % P,
         last * ((loc[:, 1] + P - pc[2]) % P) % P]
    apow = [R.ext_from_base(ONE)]
    for _ in range(4):
        apow.append(R.ext_mul(apow[-1], alpha))
    ap = [O.from_monty(a).astype(np.uint64) for a in apow]
    q = np.zeros((qn, 4), dtype=np.uint64)
    for k in range(5):  # the first constraint takes the highest power (stark_common.h fib_fold_base)
        q = (q + c[k][:, None] * ap[4 - k][None, :]) % P
    q = O.to_monty(q * R._npow(zh, P - 2)[:, None] % P)
    return [np.ascontiguousarray(q[k::4]) for k in range(4)]  # split_evals: chunk k takes rows k, k + 4, ...


def fib_through(pcs, ch, log_n, trace, pis, low_rows):
    """the hiding fib_air proof assembled from a PCS's calls (this module's HidingPcs, or an adapter of the library's with the same five
    methods); low_rows(commitment, log_size) -> the first 2^log_size rows of its matrix 0's LDE as numpy"""
    ct = pcs.commit([(trace, None)])
    alpha = fib_begin(ch, log_n, ct.root, pis)
    chunks = fib_quotient_chunks(low_rows(ct, log_n + 2), log_n, pis, alpha)
    cq = pcs.commit_quotient(chunks)
    cr = pcs.commit_randomization(log_n)
    zeta, zeta_next = fib_zeta(ch, log_n, cq.root, cr.root)
    opened, fri = pcs.open([(cr, [[zeta]]), (ct, [[zeta, zeta_next]]), (cq, [[zeta]] * 4)], ch)
    return fib_header(log_n, ct.root, cq.root, cr.root, opened) + fri


# ---- seeded general shapes ----
def random_points(rng, n_pool):
    return [R.rand_point(rng) for _ in range(n_pool)]


def random_rounds(rng, pcs, log_h, widths, max_rounds=4, max_mats=4, quotient=None, randomization=False, shifts=True, max_cols=1200):
    """1..max_rounds commits of 1..max_mats matrices with widths drawn from `widths`, 0..4 points per matrix drawn WITH repeats from a
    pool of 1..4 (at most max_cols batched columns, the random ones counted: a matrix that would pass the limit loses points);
    quotient = (C, wq): one more round of C chunks; randomization: one more round.  Calls pcs.commit / commit_quotient /
    commit_randomization in a fixed order and returns (plan, rounds): the plan replays the same calls on another PCS."""
    pool = random_points(rng, int(rng.integers(1, 5)))
    total = [0]

    def pick(w):
        pts = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(0, 5)))]
        while pts and total[0] + w * len(pts) > max_cols:
            pts.pop()
        total[0] += w * len(pts)
        return pts
    plan = []
    n_commits = int(rng.integers(1, max_rounds + 1)) - (1 if quotient else 0) - (1 if randomization else 0)
    for _ in range(max(n_commits, 1)):
        mats = []
        for _ in range(int(rng.integers(1, max_mats + 1))):
            w = int(widths[int(rng.integers(0, len(widths)))])
            mats.append((R.rand_matrix(rng, log_h, w), R.rand_shift(rng) if shifts and rng.integers(0, 2) else None))
        plan.append(("commit", mats, [pick(m.shape[1] + pcs.nrc) for m, _ in mats]))
    if quotient:
        C, wq = quotient
        plan.append(("quotient", [R.rand_matrix(rng, log_h, wq) for _ in range(C)], [pick(wq) for _ in range(C)]))
    if randomization:
        plan.append(("random", log_h, [pick(pcs.nrc + 4)]))
    if not any(p for _, _, mp in plan for p in mp):
        plan[-1][2][-1].append(pool[0])
        if len(plan) > 1:
            plan[0][2][0].extend([pool[0], pool[0]])  # and a repeat
    return plan, run_plan(pcs, plan)


def run_plan(pcs, plan):
    rounds = []
    for kind, arg, mpts in plan:
        com = pcs.commit(arg) if kind == "commit" else pcs.commit_quotient(arg) if kind == "quotient" else pcs.commit_randomization(arg)
        rounds.append((com, mpts))
    return rounds
