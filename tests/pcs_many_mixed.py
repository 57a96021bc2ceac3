"""What the CPU and the GPU tests of the device PCS batch verifier over MIXED heights share (include/p3hip.h
p3hip_pcs_verifier_create_mixed): the shapes, the word classes of a proof whose rounds have trees of their own depths (walked from the
wire format, independently of the library), where single words of a query lie, and members proved on the device.  The tampering rule,
the host verifier's answer and the status contract are tests/pcs_many.py's."""
import numpy as np

import pcs_many as M
import pcs_mixed_ref as MR
import pcs_ref as R

P = R.P
HASHES = M.HASHES

# the shapes of tests/test_gpu_pcs_mixed.py, restated: name -> (log_final_poly_len, [[(log_h, width, [slot of each point]) per matrix] per round])
SHAPES = {
    "first fold": (0, [[(2, 3, [0]), (1, 2, [0, 1])]]),
    "consecutive folds": (0, [[(3, 2, [0, 1]), (1, 5, [1])], [(2, 3, [0])]]),
    "final vector": (1, [[(4, 3, [0]), (1, 2, [0, 1])], [(3, 5, [1]), (4, 2, [1, 0])]]),
    "gap": (2, [[(5, 2, [0]), (2, 3, [1]), (3, 7, [0, 1])]]),
    "wide small class": (0, [[(4, 3, [0]), (2, 17, [0, 1]), (4, 2, [1]), (1, 5, [0])]]),
    "no points beside points": (0, [[(4, 3, [0]), (2, 5, []), (2, 4, [0, 1])]]),
    "class without points": (0, [[(4, 3, [0, 1]), (2, 5, []), (2, 2, [])], [(3, 2, [1]), (2, 19, [])]]),
    "four points": (0, [[(4, 2, [0]), (2, 3, [0, 1, 2, 3])]]),
}
# every word is tampered on this one: a round whose tree is shorter than the index, two roll-ins, and a pair (round 1's) whose alpha
# exponent, 0, differs from its position among the opened values, 9
EVERY_WORD = ((1, 0, 2, 1), SHAPES["consecutive folds"][1])
# trees, folds and roll-ins past the small-layer thresholds; round 1's tree has depth 11 under a 14-bit index
DEEP = ((1, 1, 5, 4), [[(13, 4, [0, 1]), (10, 20, [0])], [(5, 64, [1]), (10, 3, [1])]])


def heights_of(spec):
    return [[lh for lh, _, _ in r] for r in spec]


def widths_of(spec):
    return [[w for _, w, _ in r] for r in spec]


def slots_of(spec):
    return [[list(sl) for _, _, sl in r] for r in spec]


def n_slots_of(spec):
    return 1 + max(s for r in spec for _, _, sl in r for s in sl)


def verifier_shape(spec):
    """-> the `rounds` argument of PcsVerifier / pcs_proof_len"""
    return [[(w, list(sl)) for _, w, sl in r] for r in spec]


def word_classes(kind, fp, log_heights, widths):
    """the class of every word of a plain proof whose round r has a tree of depth max(log_heights[r]) + log_blowup"""
    log_blowup, lfp, nq, _ = fp
    top = max(lh for r in log_heights for lh in r)
    log_big, n_fri = top + log_blowup, top - lfp
    dg = M.FELT if kind == 0 else M.DIGEST
    out = [M.SHAPE] + [dg] * (8 * n_fri) + [M.SHAPE]
    for _ in range(nq):
        out.append(M.SHAPE)
        for ws, lhs in zip(widths, log_heights):
            out.append(M.SHAPE)
            for w in ws:
                out += [M.SHAPE] + [M.FELT] * w
            out += [M.SHAPE] + [dg] * (8 * (max(lhs) + log_blowup))
        out.append(M.SHAPE)
        for r in range(n_fri):
            out += [M.FELT] * 4 + [M.SHAPE] + [dg] * (8 * (log_big - 1 - r))
    return np.array(out + [M.SHAPE] + [M.FELT] * (4 << lfp) + [M.FELT], dtype=np.uint8)


def query_word(fp, log_heights, widths, rnd, what, mat=0, k=0, query=0):
    """the index, among a proof's words, of word k of matrix `mat`'s row (what = "row") or of the path (what = "path") of round `rnd`'s
    BatchOpening in query `query`"""
    log_blowup, lfp, _, _ = fp
    top = max(lh for r in log_heights for lh in r)
    log_big, n_fri = top + log_blowup, top - lfp
    qlen = 1 + sum(1 + sum(1 + w for w in ws) + 1 + 8 * (max(lhs) + log_blowup) for ws, lhs in zip(widths, log_heights))
    qlen += 1 + sum(4 + 1 + 8 * (log_big - 1 - r) for r in range(n_fri))
    p = 1 + 8 * n_fri + 1 + query * qlen + 1
    for r, (ws, lhs) in enumerate(zip(widths, log_heights)):
        p += 1
        for m, w in enumerate(ws):
            if r == rnd and what == "row" and m == mat:
                assert k < w
                return p + 1 + k
            p += 1 + w
        if r == rnd:
            assert what == "path" and k < 8 * (max(lhs) + log_blowup)
            return p + 1 + k
        p += 1 + 8 * (max(lhs) + log_blowup)
    raise AssertionError(rnd)


class Case:
    """n members of one mixed shape with different data and transcript prefixes, proved by TwoAdicFriPcs(mixed_heights=True)"""

    def __init__(self, p3, hash, fp, spec, n, seed):
        rng = np.random.default_rng(seed)
        self.p3, self.hash, self.fp, self.spec = p3, hash, fp, spec
        self.lhs, self.widths, self.slots, self.n_slots = heights_of(spec), widths_of(spec), slots_of(spec), n_slots_of(spec)
        self.params = p3.FriParameters(*fp)
        pcs = p3.TwoAdicFriPcs(self.params, hash, mixed_heights=True)
        self.members = []
        for j in range(n):
            pts = np.stack([R.rand_point(rng) for _ in range(self.n_slots)])
            rounds, roots = [], []
            for mats in MR.mats_of(rng, spec, pts):
                root, data = pcs.commit([(m, s) for m, s, _ in mats])
                rounds.append((data, [zs for _, _, zs in mats]))
                roots.append(root)
            ch = M.prefix(p3.Challenger(hash), seed + j)
            state = ch.export_state()
            opened, proof = pcs.open(rounds, ch)
            self.members.append(dict(proof=proof, roots=np.stack(roots), points=pts, opened=opened.copy(), state=state, after=ch))
            for d, _ in rounds:
                d.free()
        pcs.free()
        self.classes = word_classes(0 if hash == "poseidon2" else 1, fp, self.lhs, self.widths)

    def verifier(self, max_proofs):
        return self.p3.PcsVerifier(self.lhs, verifier_shape(self.spec), self.n_slots, self.params, self.hash, False, max_proofs)

    def host(self, m):
        """the host verifier's answer for the member's expanded arguments, and the challenger where it left it (None unless accepted)"""
        return M.host_code(self.p3, self.fp, self.hash, False, self.lhs, self.widths, m["roots"], M.expand(m["points"], self.slots),
                           m["opened"], m["proof"], m["state"])

    def expected(self, m):
        """the contract's status for a (possibly tampered) member, and whether the equality clause decides it"""
        h, _ = self.host(m)
        words = np.frombuffer(m["proof"][:len(m["proof"]) // 4 * 4], dtype=np.uint32)
        canon = (len(words) == len(self.classes) and M.canonical(words, self.classes) and not np.any(m["opened"] >= P)
                 and not np.any(m["points"] >= P))
        return M.expected_status(h, canon), M.in_equality_clause(h, canon)

    def word(self, rnd, what, mat=0, k=0, query=0):
        return query_word(self.fp, self.lhs, self.widths, rnd, what, mat, k, query)


def with_proof_word(m, i, tamper=M.tampered):
    t = np.frombuffer(m["proof"], dtype=np.uint32).copy()
    t[i] = tamper(t[i])
    return dict(m, proof=t.tobytes())
