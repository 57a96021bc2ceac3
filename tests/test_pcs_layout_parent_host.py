"""The PCS host verifiers and pcs_proof_len against what an EARLIER build answered.  Since the host verifier (pcs_verify_any) and the
device batch verifier's host half read one layout (csrc/pcs_layout.hip), the tests that compare the two with each other hold by
construction; this one pins both against tests/golden/pcs_verify_codes.json, which tests/golden/make_pcs_verify_codes.py recorded on a
build of commit f76056e, the last one with two hand-written copies of the gates and of the proof's offsets.  CPU only."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, golden

_spec = importlib.util.spec_from_file_location("make_pcs_verify_codes", os.path.join(GOLDEN, "make_pcs_verify_codes.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)


@pytest.fixture(scope="module")
def want():
    return golden("pcs_verify_codes.json")


def test_every_refusal_has_the_parents_code_and_message(p3, oracle, want):
    """one refused argument a case: the host verifier's (code, message) and pcs_proof_len's"""
    got = make.record(p3, oracle, "refusals")
    assert len(got) == len(want["refusals"]) >= 70
    for i, (g, w) in enumerate(zip(got, want["refusals"])):
        assert g == w, (i, g, w)


def test_proof_lengths_are_the_parents(p3, oracle, want):
    got = make.record(p3, oracle, "lens")
    assert got == want["lens"] and len(got) >= 2 * (7 * 3 + 2 * 8 + 1)


def test_every_tampered_word_gets_the_parents_code(p3, oracle, want):
    """shapes A (322 words), B (512) and EVERY_WORD (mixed heights), both hashes: one host code per tampered word"""
    got = make.record(p3, oracle, "tampered")
    assert sorted(got) == sorted(want["tampered"]) and len(got) == 6
    for name, codes in got.items():
        assert len(codes) == len(want["tampered"][name]) == {"A": 322, "B": 512, "E": 308}[name[0]], name
        diff = [(i, g, w) for i, (g, w) in enumerate(zip(codes, want["tampered"][name])) if g != w]
        assert not diff, (name, diff[:8])
        assert all(c != 0 for c in codes), name


def test_two_refused_arguments_keep_the_parents_code(p3, oracle, want):
    """a shape fault behind a point that is no field element or lies on the LDE coset: the code only (of several refused arguments the
    verifier may name another one than the parent did: csrc/prover.h)"""
    got = make.record(p3, oracle, "two_faults")
    assert got == want["two_faults"] and len(got) >= 4
