"""The host-only half of the batch verifier (include/p3hip.h "batches of proofs verified ON THE DEVICE"): p3hip_fib_proof_len against the
oracle provers' proofs over a sweep of configurations, the parameters it refuses, and the new symbols in the header, the library, the
ctypes table and the Rust shim.  No GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("p3hip_fib_proof_len", "p3hip_fib_verifier_create", "p3hip_fib_verifier_verify_dev", "p3hip_fib_verifier_verify",
       "p3hip_fib_verifier_destroy")


def _sweep():
    for hiding in (False, True):
        for hash_name in ("poseidon2", "keccak"):
            for log_n in range(1, 11):
                for log_blowup in (1, 2, 3):
                    for log_fpl in (0, 1, 2):
                        if log_fpl >= (log_n + 1 if hiding else log_n):
                            continue  # not admitted: the final polynomial stays below the (randomized) trace
                        yield hiding, hash_name, log_n, log_blowup, log_fpl


def test_proof_len_equals_the_oracle_provers_proofs(p3, oracle):
    n = 0
    for hiding, hash_name, log_n, log_blowup, log_fpl in _sweep():
        kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
        for queries in (1, 5, 24):
            t = (log_blowup, log_fpl, queries, 1)
            want = p3.proof_len(log_n, p3.FriParameters(*t), hash_name, hiding)
            for a, b in ((0, 1), (12345, 678910)):  # a second instance of the same configuration has the same length
                if hiding:
                    proof = oracle.prove_fib_air_hiding(a, b, log_n, oracle.FriParams(*t), hash=kind, seed=3)
                else:
                    proof = oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind)
                assert len(proof) == want, (hiding, hash_name, log_n, t, a, b)
            n += 1
    # every admitted point: (27 plain + 29 hiding) (log_n, log_final_poly_len) pairs x 3 blowups x 2 hashes x 3 query counts
    assert n == (27 + 29) * 3 * 2 * 3


def _host_message(p3, hash_kind, hiding, log_n, t):
    """what the host verifier says about these parameters (any bytes: parameters are checked first)"""
    lib = p3._lib.lib()
    fn = lib.p3hip_verify_fib_air_hiding if hiding else lib.p3hip_verify_fib_air_hash
    buf = (C.c_uint8 * 16)()
    rc = fn(hash_kind, buf, 16, 0, 1, 1, log_n, C.cast(p3.FriParameters(*t)._c(), C.c_void_p))
    return rc, p3.take_last_error()


@pytest.mark.parametrize("hiding", [False, True])
def test_proof_len_refuses_what_check_parameters_refuses(p3, hiding):
    lib = p3._lib.lib()
    refused = [(0, 0, (1, 0, 5, 1)), (0, 5, (0, 0, 5, 1)), (0, 27, (1, 0, 5, 1)), (0, 20, (8, 0, 5, 1)), (0, 4, (1, 4 + hiding, 5, 1)),
               (0, 4, (1, 9, 5, 1)), (0, 5, (1, 0, 5, 31)), (0, 5, (1, 0, 0, 1)), (2, 5, (1, 0, 5, 1)), (-1, 5, (1, 0, 5, 1))]
    for hash_kind, log_n, t in refused:
        out = C.c_size_t(0)
        rc = lib.p3hip_fib_proof_len(hash_kind, int(hiding), log_n, C.cast(p3.FriParameters(*t)._c(), C.c_void_p), C.byref(out))
        msg = p3.take_last_error()
        hrc, hmsg = _host_message(p3, hash_kind, hiding, log_n, t)
        assert rc == -1 and hrc == -1, (hash_kind, log_n, t, rc, hrc)
        assert msg and hmsg.endswith(msg), (msg, hmsg)  # the same message (the host entry prefixes "fib_air verification failed: ")
    # the largest admitted domain is admitted, and a null argument is an error, not a crash
    top = 26 - hiding
    assert p3.proof_len(top, p3.FriParameters(1, 0, 1, 0), "keccak", hiding) > 0
    assert lib.p3hip_fib_proof_len(0, int(hiding), 5, None, None) == -1
    assert p3.take_last_error()
    with pytest.raises(p3.P3HipError, match="num_queries must be positive"):
        p3.proof_len(5, p3.FriParameters(1, 0, 0, 1), "poseidon2", hiding)


def test_new_symbols_are_declared_exported_and_bound(p3):
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert "#define P3HIP_VERIFY_MALFORMED 16" in hdr and "typedef struct p3hip_fib_verifier p3hip_fib_verifier_t;" in hdr
    protos = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    arity = {}
    for m in re.finditer(r"\b(p3hip_\w+)\s*\(([^;{]*?)\)\s*;", protos, flags=re.S):
        arity[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    assert [arity.get(s) for s in NEW] == [5, 6, 9, 8, 1]
    lib = C.CDLL(p3._lib.LIB_PATH)
    shim = open(os.path.join(ROOT, "integration", "native", "src", "hip_front_end.rs")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in p3._lib.declared_symbols(), s
        assert len(p3._lib._SIGS[s][1]) == arity[s], s
        m = re.search(r"fn\s+%s\s*\((.*?)\)\s*(?:->\s*[^;]+)?;" % s, re.sub(r"//[^\n]*", "", shim), flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity[s], s
    assert p3.VERIFY_MALFORMED == 16 and callable(p3.proof_len) and hasattr(p3.FibAirVerifier, "verify_many_dev")
    hpp = open(os.path.join(ROOT, "include", "p3hip.hpp")).read()
    assert "class FibVerifier" in hpp and "p3hip_fib_verifier_destroy(h_)" in hpp
