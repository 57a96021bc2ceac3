"""What the CPU and the GPU tests of the device PCS batch verifier share: slots from a case's points, the word classes of a proof of
one shape (walked from the wire format, DESIGN.md "proof bytes", independently of the library), the tampering rule, the host
verifier's answer for a member, and the contract between that answer and a device status (include/p3hip.h "batches of PCS proofs
verified ON THE DEVICE")."""
import numpy as np

import pcs_ref as R

P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
EQUALITY_CODES = (11, 13, 14, 15)
MALFORMED = 16
BAD_ARG = -1
SHAPE, FELT, DIGEST = 0, 1, 2

# the two shapes whose every word is tampered: (log_blowup, log_final_poly_len, num_queries, pow_bits), log_h, the caller's widths
FP_AB, LOG_H_AB, WIDTHS_AB = (1, 0, 2, 1), 3, [[2, 3], [4]]
SLOTS_AB = [[[0, 1], [0]], [[1]]]  # trace-like: matrix 0 at both slots, the others at one each
NRC_B = 1


def slots_of(mat_points):
    """[[points of a matrix]] per round -> (slot points (n_slots, 4), [[slots of a matrix]] per round): one slot per distinct value"""
    pool, out = [], []
    for mats in mat_points:
        rs = []
        for pts in mats:
            ms = []
            for z in pts:
                z = np.asarray(z, dtype=np.uint32)
                k = next((i for i, q in enumerate(pool) if np.array_equal(q, z)), None)
                if k is None:
                    k = len(pool)
                    pool.append(z)
                ms.append(k)
            rs.append(ms)
        out.append(rs)
    return np.stack(pool), out


def verifier_shape(widths, slots):
    """-> the `rounds` argument of PcsVerifier / pcs_proof_len"""
    return [[(w, sl) for w, sl in zip(ws, ss)] for ws, ss in zip(widths, slots)]


def expand(points, slots):
    """a member's slot points -> the host form: [[points of a matrix]] per round"""
    return [[[np.asarray(points[s], dtype=np.uint32) for s in ms] for ms in rs] for rs in slots]


def word_classes(kind, fp, log_big_minus_blowup, widths, salt):
    """the class of every word of a proof: widths = committed widths per round; log_big_minus_blowup the committed log height"""
    log_blowup, lfp, nq, _ = fp
    log_big = log_big_minus_blowup + log_blowup
    n_fri = log_big_minus_blowup - lfp
    dg = FELT if kind == 0 else DIGEST
    out = [SHAPE] + [dg] * (8 * n_fri) + [SHAPE]
    for _ in range(nq):
        out.append(SHAPE)
        for ws in widths:
            out.append(SHAPE)
            for w in ws:
                out += [SHAPE] + [FELT] * w
            if salt:
                for _ in ws:
                    out += [SHAPE] + [FELT] * salt
            out += [SHAPE] + [dg] * (8 * log_big)
        out.append(SHAPE)
        for r in range(n_fri):
            out += [FELT] * 4 + ([SHAPE] + [FELT] * salt if salt else []) + [SHAPE] + [dg] * (8 * (log_big - 1 - r))
    return np.array(out + [SHAPE] + [FELT] * (4 << lfp) + [FELT], dtype=np.uint8)


def tampered(w):
    w = int(w)
    return (w + 1) % P if w < P else w ^ 1


def canonical(words, classes):
    return not np.any((np.asarray(words) >= P) & (classes == FELT))


def host_code(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, proof, state):
    """the host verifier's answer for one member in its expanded form: 0, a reject code, or BAD_ARG.  state: the transcript before
    verification as exported words.  Also returns the challenger where the verifier left it (None unless accepted)."""
    ch = p3.Challenger(hash)
    try:
        ch.import_state(state)
        vr = [((np.asarray(root, dtype=np.uint32), ws), pts) for root, ws, pts in zip(roots, widths, mat_points)]
        p3.pcs.verify(p3.FriParameters(*fp), hash, vr, log_h, opened, proof, ch, hiding=hiding)
    except p3.PcsRejected as e:
        return e.code, None
    except p3.P3HipError as e:
        assert e.code == BAD_ARG, e
        return BAD_ARG, None
    return 0, ch


def in_equality_clause(h, canon):
    return h == 0 or (h in EQUALITY_CODES and canon)


def expected_status(h, canon):
    """the contract, member by member"""
    if h == 0:
        return 0
    return h if (h in EQUALITY_CODES and canon) else MALFORMED


def prefix(ch, seed):
    """some words and, for odd seeds, a sample and more words into a transcript: the same on a Challenger and a RefChallenger"""
    ch.observe(R.O.to_monty(np.arange(seed + 1, seed + 4 + seed % 5, dtype=np.uint64) * 1000003 % P))
    if seed % 2:
        ch.sample_ext()
        ch.observe(R.O.to_monty(np.arange(1, 2 + seed % 3, dtype=np.uint64)))
    return ch
