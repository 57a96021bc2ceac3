#!/usr/bin/env python3
"""What the fib_air DEVICE batch verifier (FibAirVerifier: p3hip_fib_verifier_verify and _verify_dev) answers, member by member, recorded
on an MI355X so that a later build can be held against an earlier one:
    python3 tests/golden/make_fib_verify_many_codes.py   ->   tests/golden/fib_verify_many_codes.json

Oracle proofs of (a, b) = (3, 4), both hashes and both wire formats, at CONFIGS.  Per proof ONE batch whose members are:
  tamper   every word w in turn -> (w + 1) mod P, or w ^ 1 for a digest word >= P
  plus_p   every word w in turn -> w + P where that fits 32 bits ('.' where it does not, no member)
  lengths  the proof without its last 4 bytes; the proof with 4 zero bytes behind it
  double   two faults in one member, where the ORDER of the verifier's checks decides the answer (DOUBLE below)
Every answer is one character, the status in base 17 ("g" = 16, VERIFY_MALFORMED).  Both entries must give the same status for every
member.  tests/test_gpu_fib_verify_many_parent.py recomputes record_one() on the current build."""
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

OUT = os.path.join(HERE, "fib_verify_many_codes.json")
P = 0x78000001
A, B = 3, 4
DIGITS = "0123456789abcdefg"
HASHES = [("poseidon2", 0), ("keccak", 1)]
FRIS = [(5, (1, 0, 5, 3)), (4, (2, 1, 3, 2))]  # log_n, (log_blowup, log_final_poly_len, num_queries, pow_bits)
CONFIGS = [(hash, kind, hiding, log_n, t) for log_n, t in FRIS for hash, kind in HASHES for hiding in (False, True)]
# the double faults and the answer read from the verifier's order of checks (header and canonicity, the constraints at zeta, the count
# words of the tail and -- plain format -- of the queries, the proof of work, the queries): (plain, hiding)
DOUBLE = {
    "x_count": (10, 10),         # wrong x + the commit-phase round count, the query count or the final-polynomial length word
    "x_depth": (10, 10),         # wrong x + a depth word inside a query
    "x_plus_p": (16, 16),        # wrong x + a sibling or a final-polynomial word + P
    "x_header_count": (16, 16),  # wrong x + a count word of the header
    "pow_depth": (16, 11),       # a witness the host answers with 11 + query 0's first depth word
    "pow_tail": (16, 16),        # the same witness + a count word of the tail
    "path_depth": (16, 13),      # a word of query 0's first commitment path (13) + query 1's first depth word
}


def name(cfg):
    hash, _, hiding, log_n, _ = cfg
    return "%s %s %d" % (hash, "hiding" if hiding else "plain", log_n)


def tampered(w):
    w = int(w)
    return (w + 1) % P if w < P else w ^ 1


def layout(hiding, log_n, t):
    """word offsets of one proof (DESIGN.md "proof bytes")"""
    log_blowup, lfp, nq, _ = t
    rounds = [[8], [6], [4, 4, 4, 4]] if hiding else [[2], [4]]
    salt = 4 if hiding else 0
    log_big = log_n + (1 if hiding else 0) + log_blowup
    n_fri = log_big - log_blowup - lfp
    head = 3 + 8 * len(rounds) + ((1 + 32) + (1 + 24) + (1 + 24) + 1 + 4 * (1 + 16) if hiding else (1 + 8) + (1 + 8) + (2 + 16))
    L = {"head": head, "header_count": 3 + 8 * len(rounds), "n_fri": head, "nq": head + 1 + 8 * n_fri}
    L["q_base"] = L["nq"] + 1
    p = 1
    L["depth"], L["path"] = [], []
    for widths in rounds:
        p += 1 + sum(1 + w for w in widths) + (len(widths) * (1 + salt) if salt else 0)
        L["depth"].append(p)
        L["path"].append(p + 1)
        p += 1 + 8 * log_big
    L["nr"] = p
    p += 1
    L["sib"], L["fri_depth"] = [], []
    for r in range(n_fri):
        L["sib"].append(p)
        p += 4 + (1 + salt if salt else 0)
        L["fri_depth"].append(p)
        p += 1 + 8 * (log_big - 1 - r)
    L["q_len"] = p
    L["fpl"] = L["q_base"] + nq * p
    L["fpoly"] = L["fpl"] + 1
    L["witness"] = L["fpoly"] + 4 * (1 << lfp)
    L["words"] = L["witness"] + 1
    return L


def host_code(p3, kind, hiding, proof, inst, log_n, t):
    lib = p3._lib.lib()
    fn = lib.p3hip_verify_fib_air_hiding if hiding else lib.p3hip_verify_fib_air_hash
    buf = (C.c_uint8 * len(proof)).from_buffer_copy(proof)
    rc = fn(kind, buf, len(proof), inst[0], inst[1], inst[2], log_n, C.cast(p3.FriParameters(*t)._c(), C.c_void_p))
    p3.take_last_error()
    return rc


def members(p3, oracle, cfg):
    """-> (proofs, instances, classes): classes = [(class name, first member, count)] in batch order"""
    hash, kind, hiding, log_n, t = cfg
    prove = oracle.prove_fib_air_hiding if hiding else oracle.prove_fib_air
    proof = prove(A, B, log_n, oracle.FriParams(*t), hash=kind)
    inst = (A, B, oracle.fib_public_x(A, B, 1 << log_n))
    wrong = (A, B, (inst[2] + 1) % P)
    w = np.frombuffer(proof, np.uint32)
    L = layout(hiding, log_n, t)
    assert L["words"] == len(w), (name(cfg), L["words"], len(w))
    assert host_code(p3, kind, hiding, proof, inst, log_n, t) == 0 and host_code(p3, kind, hiding, proof, wrong, log_n, t) == 10

    def with_words(changes):
        bad = w.copy()
        for i, v in changes:
            bad[i] = v
        return bad.tobytes()

    t1 = lambda i: (i, tampered(w[i]))  # noqa: E731
    plus_p = lambda i: (i, int(w[i]) + P)  # noqa: E731
    batch, insts, classes = [], [], []

    def add(cls, items):
        classes.append((cls, len(batch), len(items)))
        for bytes_, i in items:
            batch.append(bytes_)
            insts.append(i)

    add("tamper", [(with_words([t1(i)]), inst) for i in range(len(w))])
    add("plus_p", [(with_words([plus_p(i)]), inst) for i in range(len(w)) if int(w[i]) + P < 2 ** 32])
    add("lengths", [(proof[:-4], inst), (proof + b"\0" * 4, inst)])
    q0, q1 = L["q_base"], L["q_base"] + L["q_len"]
    last = L["q_base"] + (t[2] - 1) * L["q_len"]
    # a witness the host verifier answers with 11, and a path word it answers with 13
    witness = next(v for v in ((int(w[L["witness"]]) + k) % P for k in range(1, 200))
                   if host_code(p3, kind, hiding, with_words([(L["witness"], v)]), inst, log_n, t) == 11)
    pow_bad = (L["witness"], witness)
    path_bad = t1(q0 + L["path"][0] + 8 + 3)
    assert host_code(p3, kind, hiding, with_words([path_bad]), inst, log_n, t) == 13
    add("x_count", [(with_words([t1(L[k])]), wrong) for k in ("n_fri", "nq", "fpl")])
    add("x_depth", [(with_words([t1(i)]), wrong) for i in (q0 + L["depth"][0], q0 + L["depth"][-1], q0 + L["fri_depth"][0], last + L["depth"][0],
                                                          last + L["fri_depth"][-1])])
    add("x_plus_p", [(with_words([plus_p(i)]), wrong) for i in (q0 + L["sib"][0] + 1, last + L["sib"][-1], L["fpoly"], L["fpoly"] + 3)])
    add("x_header_count", [(with_words([t1(L["header_count"])]), wrong)])
    add("pow_depth", [(with_words([pow_bad, t1(q0 + L["depth"][0])]), inst)])
    add("pow_tail", [(with_words([pow_bad, t1(L[k])]), inst) for k in ("n_fri", "nq", "fpl")])
    add("path_depth", [(with_words([path_bad, t1(q1 + L["depth"][0])]), inst)])
    return batch, insts, classes, [int(w[i]) + P < 2 ** 32 for i in range(len(w))]


def monty(v):
    return ((v % P) << 32) % P


def statuses(p3, cfg, batch, insts):
    """the two entries' statuses of one batch, each as a list of ints"""
    import torch
    hash, _, hiding, log_n, t = cfg
    ver = p3.FibAirVerifier(log_n, p3.FriParameters(*t), hash, hiding, max_proofs=len(batch))
    try:
        stride = ver.proof_len + 4
        host = np.zeros((len(batch), stride), dtype=np.uint8)
        for i, p in enumerate(batch):
            host[i, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        pis = np.array([[monty(v) for v in i] for i in insts], dtype=np.uint32).view(np.int32)
        lens = np.array([len(p) for p in batch], dtype=np.uint32).view(np.int32)
        status, rejected = ver.verify_many_dev(torch.from_numpy(host).cuda(), torch.from_numpy(pis).cuda(), torch.from_numpy(lens).cuda(), n=len(batch))
        dev = status.cpu().numpy().view(np.uint32).tolist()
        assert int(rejected.cpu()[0]) == sum(1 for s in dev if s)
        return ver.verify_many(batch, insts).tolist(), dev
    finally:
        ver.close()


def encode(cfg, classes, fits, status):
    rec = {"words": len(fits)}
    for cls, first, count in classes:
        s = "".join(DIGITS[v] for v in status[first:first + count])
        if cls == "plus_p":  # '.' where the word + P does not fit
            it = iter(s)
            s = "".join(next(it) if f else "." for f in fits)
        rec[cls] = s
    return rec


def record_one(p3, oracle, cfg):
    """-> (the host entry's recording, the device entry's) of one configuration"""
    batch, insts, classes, fits = members(p3, oracle, cfg)
    many, dev = statuses(p3, cfg, batch, insts)
    return encode(cfg, classes, fits, many), encode(cfg, classes, fits, dev)


def check(rec):
    """what the recording is for: no class is empty, and every double fault has the answer read from the order of the checks"""
    assert sorted(rec) == sorted(name(c) for c in CONFIGS)
    for cfg in CONFIGS:
        r = rec[name(cfg)]
        assert len(r["tamper"]) == r["words"] == len(r["plus_p"]) and len(r["lengths"]) == 2, name(cfg)
        assert sum(ch != "." for ch in r["plus_p"]) >= r["words"] // 2 and "0" not in r["tamper"] + r["plus_p"] + r["lengths"], name(cfg)
        assert r["lengths"] == "gg", name(cfg)
        for cls, want in DOUBLE.items():
            assert r[cls] and set(r[cls]) == {DIGITS[want[1 if cfg[2] else 0]]}, (name(cfg), cls, r[cls])


if __name__ == "__main__":
    from conftest import load_package
    from oracle import oracle as o
    o.build()
    p3 = load_package()
    rec = {}
    for cfg in CONFIGS:
        many, dev = record_one(p3, o, cfg)
        assert many == dev, name(cfg)
        rec[name(cfg)] = dev
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    check(rec)
