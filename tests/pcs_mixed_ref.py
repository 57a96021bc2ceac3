"""Reference prover and verifier of TwoAdicFriPcs over matrices of MIXED heights, built on tests/pcs_ref.py's helpers and the
oracle's primitives (coset_lde_batch, mmcs_commit with injected shorter matrices, mmcs_verify_batch, idft_batch, the hashes).  It
knows nothing of the library.  The protocol (upstream TwoAdicFriPcs from recall, parity unpinned: DESIGN.md section 3):

  class     the matrices of an open whose LDEs share log_big_m = log_h_m + log_blowup; log_big is the tallest class
  commit    one mmcs_commit per round over LDEs of their own heights, in input order
  opened    observed round -> matrix -> point -> column; each from the matrix's own height
  alpha     one counter per class: a (matrix, point) pair of width w takes alpha^c .. alpha^(c + w - 1), c its class's counter
  ro_c      one reduced-opening vector of 2^log_big_c elements per class with a point, over GENERATOR * <g_big_c>, bit-reversed
  folding   starts from the tallest class's vector; after the fold that reaches 2^log_big_c elements: folded += beta^2 ro_c, beta
            that round's challenge; a class with log_h_c == log_final_poly_len is rolled into the final vector
  queries   an index of log_big bits; round r's BatchOpening at index >> (log_big - log_big_r), log_big_r the round's tallest LDE:
            its depth word and path length

With all heights equal this is pcs_ref.open byte for byte (tests/test_pcs_mixed_ref_host.py), and pcs_ref.open is pinned to the
oracle's fib_air proofs."""
import numpy as np

import pcs_ref as R
from pcs_ref import O, P


class Refused(ValueError):
    """a shape the protocol has no proof for"""


def _log2(n):
    lg = int(n).bit_length() - 1
    if n < 2 or (1 << lg) != n:
        raise Refused("height must be a power of two >= 2")
    return lg


def check_shape(fp, log_heights, point_counts):
    """log_heights, point_counts: [[per matrix] per round] -> (log_big, sorted list of the classes with a point)"""
    log_blowup, lfp = fp[0], fp[1]
    log_h_max = max(lh for r in log_heights for lh in r)
    with_points = {lh for r, c in zip(log_heights, point_counts) for lh, n in zip(r, c) if n}
    if log_h_max not in with_points:
        raise Refused("the tallest matrices have no opening point")
    if min(lh for r in log_heights for lh in r) < lfp:
        raise Refused("a matrix lies below the final polynomial")
    if lfp >= log_h_max:
        raise Refused("log_final_poly_len must be below the tallest log height")
    return log_h_max + log_blowup, sorted(lh + log_blowup for lh in with_points)


def _domain(log_big):
    """GENERATOR * <g_big> bit-reversed, canonical, as (big, 4) extension elements"""
    g = int(O.from_monty(R.two_adic_generator(log_big)))
    x = np.zeros((1 << log_big, 4), dtype=np.uint64)
    x[:, 0] = (R._geom(g, 1 << log_big) * np.uint64(31) % P)[R._bitrev(log_big)]
    return x


def prove(kind, fp, rounds, ch):
    """rounds = [[(evals h_m x w Montgomery words, domain shift or None, [points])]].  -> dict with opened, proof, roots, and for
    the low-degree test the final folded vector (canonical) and the final polynomial (Montgomery words)."""
    log_blowup, lfp, nq, pow_bits = fp
    lhs = [[_log2(m.shape[0]) for m, _, _ in mats] for mats in rounds]
    log_big, classes = check_shape(fp, lhs, [[len(pts) for _, _, pts in mats] for mats in rounds])
    com = [R.commit(kind, log_blowup, [(m, s) for m, s, _ in mats]) for mats in rounds]
    opened = [R.opened_value(m, R.ONE if s is None else s, z) for mats in rounds for m, s, pts in mats for z in pts]
    opened = np.concatenate(opened).reshape(-1, 4)
    ch.observe(opened)
    alp = R._ext_powers(O.from_monty(ch.sample_ext()), len(opened))
    opc = O.from_monty(opened).astype(np.uint64)
    ro = {lb: np.zeros((1 << lb, 4), dtype=np.uint64) for lb in classes}
    xs = {lb: _domain(lb) for lb in classes}
    cnt = {lb: 0 for lb in classes}
    k = 0
    for (_, _, ldes), mats in zip(com, rounds):
        for lde, (_, _, pts) in zip(ldes, mats):
            v, w = O.from_monty(lde).astype(np.uint64), lde.shape[1]
            lb = _log2(lde.shape[0])
            for z in pts:
                a = alp[cnt[lb]:cnt[lb] + w]
                y = R._canon_ext_mul(a, opc[k:k + w]).sum(axis=0) % P
                s = np.stack([(v * a[:, c][None, :] % P).sum(axis=1) % P for c in range(4)], axis=1)
                dz = R._canon_ext_inv((O.from_monty(R.ext(z)).astype(np.uint64)[None, :] + P - xs[lb]) % P)
                ro[lb] = (ro[lb] + R._canon_ext_mul((y[None, :] + P - s) % P, dz)) % P
                k += w
                cnt[lb] += w
    n_fr = log_big - log_blowup - lfp
    one_half = pow(2, P - 2, P)
    folded, ftrees, froots = ro[log_big], [], []
    for _ in range(n_fr):
        root, tree = O.mmcs_commit([O.to_monty(folded).reshape(len(folded) // 2, 8)], kind)
        ftrees.append(tree)
        froots.append(root)
        ch.observe_digest(root)
        beta = O.from_monty(ch.sample_ext()).astype(np.uint64)
        folded = R._fold(folded, beta, one_half)
        lb = len(folded).bit_length() - 1
        if lb in ro:
            b2 = R._canon_ext_mul(beta, beta)
            folded = (folded + R._canon_ext_mul(ro[lb], b2[None, :])) % P
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
    u = lambda *vals: np.array(vals, dtype=np.uint32)
    out = [u(n_fr)] + froots + [u(nq)]
    for _ in range(nq):
        index = ch.sample_bits(log_big)
        out.append(u(len(rounds)))
        for (_, tree, ldes) in com:
            lbr = max(_log2(lde.shape[0]) for lde in ldes)
            rows, path = tree.open_batch(index >> (log_big - lbr))
            out.append(u(len(ldes)))
            pos = 0
            for lde in ldes:
                out += [u(lde.shape[1]), rows[pos:pos + lde.shape[1]]]
                pos += lde.shape[1]
            out += [u(lbr), path.reshape(-1)]
        out.append(u(n_fr))
        for r in range(n_fr):
            idx = index >> r
            rows, path = ftrees[r].open_batch(idx >> 1)
            out += [rows[4 * ((idx ^ 1) & 1):][:4], u(log_big - 1 - r), path.reshape(-1)]
    out += [u(fpl), fpoly.reshape(-1), u(wit)]
    proof = np.concatenate([np.asarray(o, dtype=np.uint32).reshape(-1) for o in out]).tobytes()
    return {"opened": opened, "proof": proof, "roots": [c[0] for c in com], "final": folded, "fpoly": fpoly, "log_heights": lhs}


def open(kind, fp, rounds, ch):
    """-> (opened values, FriProof bytes), as pcs_ref.open without its log_h"""
    d = prove(kind, fp, rounds, ch)
    return d["opened"], d["proof"]


def final_vector_is_the_final_polynomial(fp, d):
    """the low-degree test at EVERY point of the final domain: folded[i] == fpoly(g_lfin^bitrev(i)), lfin = log_blowup + lfp"""
    lfin = fp[0] + fp[1]
    g = int(O.from_monty(R.two_adic_generator(lfin)))
    x = (R._geom(g, 1 << lfin))[R._bitrev(lfin)]
    co = O.from_monty(d["fpoly"]).astype(np.uint64).reshape(-1, 4)
    acc = np.zeros((1 << lfin, 4), dtype=np.uint64)
    for i in range(len(co) - 1, -1, -1):
        acc = (acc * x[:, None] % P + co[i][None, :]) % P
    return len(d["final"]) == (1 << lfin) and np.array_equal(acc, d["final"])


def verifier_rounds(roots, rounds):
    """-> (what verify takes, the per-matrix log heights round -> matrix)"""
    return R.verifier_rounds(roots, rounds), [[_log2(m.shape[0]) for m, _, _ in mats] for mats in rounds]


def verify(kind, fp, log_heights, rounds, opened, proof, ch):
    """pcs_ref.verify with a log height per matrix (log_heights = [[per matrix] per round]).  0 = accept, else the failed check."""
    log_blowup, lfp, nq, pow_bits = fp
    log_big, classes = check_shape(fp, log_heights, [[len(p) for p in mp] for _, mp in rounds])
    opened = np.asarray(opened, dtype=np.uint32).reshape(-1, 4)
    ch.observe(opened)
    al = ch.sample_ext()
    alp = [R.ext_from_base(R.ONE)]
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
    lbr = [max(lhs) + log_blowup for lhs in log_heights]
    qwords = 1 + sum(1 + sum(1 + w for w in ws) + 1 + 8 * lb for ((_, ws), _), lb in zip(rounds, lbr)) + 1 + sum(4 + 1 + 8 * (log_big - 1 - r) for r in range(n_rounds))
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
    for _ in range(nq):
        index = ch.sample_bits(log_big)
        if rd.u32() != len(rounds):
            return 12
        xi = {lb: R.bmul(R.GEN, R.bpow(R.two_adic_generator(lb), R.rev_bits(index >> (log_big - lb), lb))) for lb in classes}
        ro = {lb: np.zeros(4, dtype=np.uint32) for lb in classes}
        cnt = {lb: 0 for lb in classes}
        k = 0
        for ((root, ws), mpoints), lhs, lb_r in zip(rounds, log_heights, lbr):
            if rd.u32() != len(ws):
                return 12
            rows = []
            for w in ws:
                if rd.u32() != w:
                    return 12
                rows.append(rd.words(w))
            if rd.u32() != lb_r:
                return 12
            path = digest(lb_r)
            if rd.bad:
                return 9
            dims = [(1 << (lh + log_blowup), w) for lh, w in zip(lhs, ws)]
            if not O.mmcs_verify_batch(root, dims, index >> (log_big - lb_r), np.concatenate(rows), path, kind=kind):
                return 13
            for row, pts, lh in zip(rows, mpoints, lhs):
                lb = lh + log_blowup
                for z in pts:
                    dz = R.ext_inv(R.ext_sub(R.ext(z), R.ext_from_base(xi[lb])))
                    for c in range(len(row)):
                        t = R.ext_mul(R.ext_sub(opened[k], R.ext_from_base(row[c])), dz)
                        ro[lb] = R.ext_add(ro[lb], R.ext_mul(alp[cnt[lb]], t))
                        k += 1
                        cnt[lb] += 1
        if rd.u32() != n_rounds:
            return 12
        folded, idx = ro[log_big], index
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
            s = R.bpow(R.two_adic_generator(lfh + 1), R.rev_bits(pair, lfh))
            num = R.ext_mul(R.ext_sub(betas[r], R.ext_from_base(s)), R.ext_sub(ev[1], ev[0]))
            folded = R.ext_add(ev[0], R.ext_scale(num, R.binv((2 * (P - s)) % P)))
            if lfh in ro:
                folded = R.ext_add(folded, R.ext_mul(R.ext_mul(betas[r], betas[r]), ro[lfh]))
            idx = pair
        lfin = log_blowup + lfp
        xf = R.bpow(R.two_adic_generator(lfin), R.rev_bits(idx, lfin))
        acc = np.zeros(4, dtype=np.uint32)
        for i in range(fpl - 1, -1, -1):
            acc = R.ext_add(R.ext_scale(acc, xf), fpoly[i])
        if not np.array_equal(acc, folded):
            return 15
    return 0


# ---- shapes shared by the CPU and the GPU tests ----
def mats_of(rng, spec, points):
    """spec = [[(log_h, width, [index into points]) per matrix] per round] -> rounds for prove; every third matrix with a random shift"""
    rounds, n = [], 0
    for r in spec:
        mats = []
        for log_h, w, pidx in r:
            mats.append((R.rand_matrix(rng, log_h, w), R.rand_shift(rng) if n % 3 == 1 else None, [points[i] for i in pidx]))
            n += 1
        rounds.append(mats)
    return rounds


# the three shapes of the issue's table: (fp, log_h per round -> matrix)
TABLE = [((1, 0, 4, 0), [[3, 1], [2]]), ((2, 1, 4, 0), [[4, 1], [3, 4]]), ((1, 2, 3, 0), [[5, 2, 3]])]


def table_case(rng, log_hs, widths=(3, 5, 2, 7)):
    z = [R.rand_point(rng), R.rand_point(rng)]
    n = 0
    spec = []
    for r in log_hs:
        row = []
        for lh in r:
            row.append((lh, widths[n % len(widths)], [0, 1] if n % 2 == 0 else [1]))
            n += 1
        spec.append(row)
    return mats_of(rng, spec, z)


def random_mixed_case(rng, max_log_h=7, max_cols=400):
    """1-4 rounds of 1-4 matrices, log_h 1..max_log_h drawn from a pool of 2-3 heights so that classes repeat across rounds, widths
    from pcs_ref.WIDTHS, 0-4 points per matrix from a pool of 1-4; the tallest matrix always has a point"""
    pool = [R.rand_point(rng) for _ in range(int(rng.integers(1, 5)))]
    hs = sorted({int(v) for v in rng.integers(1, max_log_h + 1, int(rng.integers(2, 4)))})
    rounds, total = [], 0
    for _ in range(int(rng.integers(1, 5))):
        mats = []
        for _ in range(int(rng.integers(1, 5))):
            w = R.WIDTHS[int(rng.integers(0, len(R.WIDTHS)))]
            lh = hs[int(rng.integers(0, len(hs)))]
            pts = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(0, 5)))]
            while pts and total + w * len(pts) > max_cols:
                pts.pop()
            total += w * len(pts)
            mats.append((R.rand_matrix(rng, lh, w), R.rand_shift(rng) if rng.integers(0, 4) else None, pts))
        rounds.append(mats)
    top = max(m.shape[0] for mats in rounds for m, _, _ in mats)
    if not any(pts for mats in rounds for m, _, pts in mats if m.shape[0] == top):
        for mats in rounds:
            for i, (m, s, pts) in enumerate(mats):
                if m.shape[0] == top:
                    mats[i] = (m, s, [pool[0]])
                    return rounds
    return rounds
