"""What the CPU and the GPU tests of the AIR verifiers share (include/p3hip.h p3hip_air_verify, p3hip_air_verifier_*): proofs from the
reference prover of tests/air_ref.py, kept for the session; the kinds of word a proof's header has, walked from the wire format
independently of the library; the class of every word of a whole proof; the tampering rule and the contract between the host
verifier's answer and a device status."""
import numpy as np

import air_ref as A
import pcs_many as M
import pcs_ref as R

P = R.P
HASHES = M.HASHES
NAMES = ["fib", "B", "C", "D"]
OOD, MALFORMED, BAD_ARG = 10, M.MALFORMED, M.BAD_ARG
EQUALITY_CODES = (OOD,) + M.EQUALITY_CODES

_PROOFS = {}


def ref_proof(airs, name, kind, log_n, t, **gen_args):
    """-> (proof bytes, public values) of the reference prover for test AIR `name`; made once per session"""
    key = (name, kind, log_n, tuple(t), tuple(sorted(gen_args.items())))
    if key not in _PROOFS:
        air, gen = airs[name]
        trace, pis = gen(log_n, **gen_args)
        _PROOFS[key] = (A.prove(kind, t, air.code, air.consts, trace, pis), pis)
    return _PROOFS[key]


def applies(air, log_n, t):
    """the FRI tuple suits the AIR at this size: the final polynomial below the height, the LDE holds the quotient domain, queries"""
    return t[1] < log_n and t[0] >= air.log_quotient_degree and t[2] > 0


def header_kinds(width, C):
    """-> {kind: [word offsets]} of a proof's header: 'magic', 'version', 'log_n', 'root' (16 words), 'count' (the two widths, the
    chunk count, every chunk's 4), 'local', 'next', 'chunk'"""
    k = {"magic": [0], "version": [1], "log_n": [2], "root": list(range(3, 19)), "count": [19, 20 + 4 * width, 21 + 8 * width]}
    k["local"] = list(range(20, 20 + 4 * width))
    k["next"] = list(range(21 + 4 * width, 21 + 8 * width))
    k["chunk"] = []
    for c in range(C):
        base = 22 + 8 * width + 17 * c
        k["count"].append(base)
        k["chunk"] += list(range(base + 1, base + 17))
    assert base + 17 == A.header_words(width, C.bit_length() - 1)
    return k


def word_classes(kind, t, log_n, width, C):
    """the class (pcs_many.SHAPE / FELT / DIGEST) of every word of a whole proof"""
    hk = header_kinds(width, C)
    head = np.full(A.header_words(width, C.bit_length() - 1), M.FELT, dtype=np.uint8)
    head[hk["magic"] + hk["version"] + hk["log_n"] + hk["count"]] = M.SHAPE
    if kind != 0:
        head[hk["root"]] = M.DIGEST
    return np.concatenate([head, M.word_classes(kind, t, log_n, [[width], [4] * C], 0)])


def with_word(proof, off, value=None):
    """the proof with word `off` changed by pcs_many's rule, or set to `value`"""
    w = np.frombuffer(proof, dtype=np.uint32).copy()
    w[off] = M.tampered(w[off]) if value is None else value
    return w.tobytes()


def host_code(air, proof, pis, log_n, fp, hash):
    """p3hip_air_verify's answer: 0, a reject code, or BAD_ARG for refused values"""
    try:
        return air.verify(proof, pis, log_n, fp, hash)
    except RuntimeError as e:  # P3HipError
        assert getattr(e, "code", None) == BAD_ARG, e
        return BAD_ARG


def expected_status(h, proof, pis, classes, good):
    """the contract, member by member: status = H when H accepts, or when H is 10 / 11 / 13 / 14 / 15 and the proof has the length,
    every dictated word (those of `good`, any accepted proof of the configuration) and every field word in range; everything else is
    malformed"""
    if h == 0:
        return 0
    if h not in EQUALITY_CODES or len(proof) != 4 * len(classes) or np.any(np.asarray(pis, dtype=np.uint64) >= P):
        return MALFORMED
    w, g = np.frombuffer(proof, dtype=np.uint32), np.frombuffer(good, dtype=np.uint32)
    if np.any((w != g) & (classes == M.SHAPE)):
        return MALFORMED
    return h if M.canonical(w, classes) else MALFORMED
