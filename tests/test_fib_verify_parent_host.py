"""The fib_air host verifiers against what an EARLIER build answered.  Both wire formats are verified by one function over a table, and
their PCS half is the walk of the PCS host verifiers (csrc/verifier.hip: verify_fib, pcs_walk); what the three callers of that walk answer
differently is a table too (Dialect).  tests/golden/fib_verify_codes.json was recorded by tests/golden/make_fib_verify_codes.py on a
build of commit 78776af, the last one with a hand-written query loop per wire format.  CPU only."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import GOLDEN, golden
from test_verify_many_host import _host_message, _sweep

_spec = importlib.util.spec_from_file_location("make_fib_verify_codes", os.path.join(GOLDEN, "make_fib_verify_codes.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)


@pytest.fixture(scope="module")
def want():
    return golden("fib_verify_codes.json")


@pytest.fixture(scope="module")
def got(p3, oracle):
    return make.record(p3, oracle)


def test_the_recording_holds_what_it_is_for(want):
    """every reject code of a fib verifier (1-4, 7-15; 5 and 6 too), a 7 on a count word of a plain query and a 13 on a + P word of
    every plain proof: no class is empty at the three configurations, so none was added"""
    make.check(want)
    assert {a[0] for a in want["answers"]} >= set(range(1, 16))


def test_every_answer_is_the_parents_code_and_message(got, want):
    """per proof (2 hashes x 2 formats x 3 configurations): every word tampered, every word + P, every truncation and 4 trailing
    bytes, a / b / x / log_n off by one, the other format's and the other hash's proof"""
    assert sorted(got["proofs"]) == sorted(want["proofs"])
    for name, w in want["proofs"].items():
        g = got["proofs"][name]
        assert g["words"] == w["words"], name
        for kind in ("tamper", "plus_p", "truncated", "other"):
            assert len(g[kind]) == len(w[kind]), (name, kind)
            diff = [(i, got["answers"][make.ALPHABET.index(a)], want["answers"][make.ALPHABET.index(b)])
                    for i, (a, b) in enumerate(zip(g[kind], w[kind]))
                    if (a == ".") != (b == ".") or (a != "." and got["answers"][make.ALPHABET.index(a)] != want["answers"][make.ALPHABET.index(b)])]
            assert not diff, (name, kind, len(diff), diff[:8])


def test_no_pcs_refusal_leaks_out_of_a_fib_verifier(p3):
    """pcs_layout takes every parameter set verify_check_parameters admits: over the sweep of test_verify_many_host and at the largest
    admitted domains, 16 zero bytes are a bad header (1), never a refused argument of the PCS"""
    points = [(hiding, hash_name == "keccak", log_n, (log_blowup, log_fpl, q, pow_bits))
              for hiding, hash_name, log_n, log_blowup, log_fpl in _sweep() for q, pow_bits in ((1, 0), (24, 30))]
    for hiding in (False, True):
        for kind in (0, 1):
            top = 27 - hiding
            points += [(hiding, kind, top - lb, (lb, lfp, 1, 0)) for lb in (1, 2, top - 1) for lfp in (0, top - lb - 1 + hiding)]
    assert len(points) == (27 + 29) * 3 * 2 * 2 + 2 * 2 * 6
    for hiding, kind, log_n, t in points:
        rc, msg = _host_message(p3, int(kind), hiding, log_n, t)
        assert rc == 1 and msg.endswith("bad header") and "pcs verify" not in msg, (hiding, kind, log_n, t, rc, msg)
