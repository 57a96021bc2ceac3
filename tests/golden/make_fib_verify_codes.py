#!/usr/bin/env python3
"""What the fib_air host verifiers (p3hip_verify_fib_air_hash, wire format 1; p3hip_verify_fib_air_hiding, wire format 2) answer, code
AND message, recorded so that a later build can be held against an earlier one:
    python3 tests/golden/make_fib_verify_codes.py   ->   tests/golden/fib_verify_codes.json

Oracle proofs of (a, b) = (3, 4), both hashes and both formats, at CONFIGS.  Per proof:
  tamper     every word w in turn -> (w + 1) mod P, or w ^ 1 for a digest word >= P (pcs_many.tampered)
  plus_p     every word w in turn -> w + P where that fits 32 bits ('.' where it does not)
  truncated  the first 0, 4, 8 ... len - 4 bytes, then the whole proof with 4 zero bytes behind it
  other      a, b, x off by one; the proof of the other wire format; the proof of the other hash; log_n - 1 and log_n + 1
Every answer is one character: its index in "answers", the table of the distinct [code, message] pairs (message without the entry's
"fib_air verification failed: ").  tests/test_fib_verify_parent_host.py recomputes record() on the current build."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import pcs_many as M  # noqa: E402

OUT = os.path.join(HERE, "fib_verify_codes.json")
P = 2013265921
CONFIGS = [(1, (1, 0, 2, 0)), (3, (1, 0, 10, 4)), (5, (2, 2, 6, 5))]  # log_n, (log_blowup, log_final_poly_len, num_queries, pow_bits)
A, B = 3, 4
ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!#$%&()*+,-/:;<=>?@[]^_{|}~"  # '.' = no answer
PREFIX = "fib_air verification failed: "
PLAIN_HEADER_WORDS = 3 + 16 + (1 + 8) + (1 + 8) + (2 + 16)  # magic, version, log_n; two roots; the opened values


def name(hash, hiding, log_n):
    return "%s %s %d" % (hash, "hiding" if hiding else "plain", log_n)


def record(p3, oracle):
    lib = p3._lib.lib()
    answers = []

    def ask(hiding, kind, proof, a, b, x, log_n, t):
        fn = lib.p3hip_verify_fib_air_hiding if hiding else lib.p3hip_verify_fib_air_hash
        buf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(proof or b"\0")
        rc = fn(kind, buf, len(proof), a, b, x, log_n, C.cast(p3.FriParameters(*t)._c(), C.c_void_p))
        msg = p3.take_last_error() if rc else ""
        assert rc == 0 or msg.startswith(PREFIX), (rc, msg)
        ans = [int(rc), msg[len(PREFIX):]]
        if ans not in answers:
            answers.append(ans)
        return ALPHABET[answers.index(ans)]

    proofs = {}
    for log_n, t in CONFIGS:
        for hash, kind in M.HASHES:
            for hiding in (False, True):
                prove = oracle.prove_fib_air_hiding if hiding else oracle.prove_fib_air
                proofs[name(hash, hiding, log_n)] = prove(A, B, log_n, oracle.FriParams(*t), hash=kind)
    out = {}
    for log_n, t in CONFIGS:
        x = oracle.fib_public_x(A, B, 1 << log_n)
        for hash, kind in M.HASHES:
            for hiding in (False, True):
                proof = proofs[name(hash, hiding, log_n)]
                q = lambda bytes_, a=A, b=B, x=x, log_n=log_n: ask(hiding, kind, bytes_, a, b, x, log_n, t)  # noqa: E731
                assert q(proof) == ALPHABET[answers.index([0, ""])]
                w = np.frombuffer(proof, np.uint32)
                rec = {"words": len(w), "tamper": "", "plus_p": "", "truncated": ""}
                for i in range(len(w)):
                    bad = w.copy()
                    bad[i] = M.tampered(w[i])
                    rec["tamper"] += q(bad.tobytes())
                    if int(w[i]) + P < 2 ** 32:
                        bad[i] = int(w[i]) + P
                        rec["plus_p"] += q(bad.tobytes())
                    else:
                        rec["plus_p"] += "."
                    rec["truncated"] += q(proof[:4 * i])
                rec["truncated"] += q(proof + b"\0" * 4)
                rec["other"] = (q(proof, a=A + 1) + q(proof, b=B + 1) + q(proof, x=x + 1) + q(proofs[name(hash, not hiding, log_n)])
                                + q(proofs[name(M.HASHES[1 - kind][0], hiding, log_n)]) + q(proof, log_n=log_n - 1) + q(proof, log_n=log_n + 1))
                out[name(hash, hiding, log_n)] = rec
    assert len(answers) <= len(ALPHABET)
    return json.loads(json.dumps({"answers": answers, "proofs": out}))


def check(rec):
    """what the recording is for: every reject code a fib verifier can give occurs (5 and 6 are not asked for, they occur all the same),
    and so do the two places where the plain verifier differs from the general PCS walk"""
    code = lambda ch: rec["answers"][ALPHABET.index(ch)][0]  # noqa: E731
    seen = {code(ch) for p in rec["proofs"].values() for k in ("tamper", "plus_p", "truncated", "other") for ch in p[k] if ch != "."}
    assert seen >= set(range(1, 16)) - {5, 6}, sorted(seen)
    assert len(rec["proofs"]) == 12
    for log_n, t in CONFIGS:
        for hash, _ in M.HASHES:
            p = rec["proofs"][name(hash, False, log_n)]
            # the plain verifier follows the count words to the final polynomial: a tampered count of a query's openings is a 7
            # there, where the general walk compares it with the shape and says 12
            first_query = PLAIN_HEADER_WORDS + 1 + 8 * (log_n - t[1]) + 1
            assert code(p["tamper"][first_query]) == 7, (hash, log_n)
            # and it hashes an opening before it asks whether its words were canonical: 13 where the general walk says 9
            assert 13 in {code(ch) for ch in p["plus_p"] if ch != "."}, (hash, log_n)
            for k in ("tamper", "plus_p"):
                assert len(p[k]) == p["words"] and len(p["truncated"]) == p["words"] + 1


if __name__ == "__main__":
    from conftest import load_package
    from oracle import oracle as o
    o.build()
    rec = record(load_package(), o)
    check(rec)
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rec["answers"]), "answers")
