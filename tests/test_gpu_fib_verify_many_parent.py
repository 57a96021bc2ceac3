"""The fib_air device batch verifier against what an EARLIER build answered, member by member.  FibVerifierDev is a front kernel and an
owned PcsVerifierDev (csrc/verifier_dev.hip); tests/golden/fib_verify_many_codes.json was recorded on an MI355X by
tests/golden/make_fib_verify_many_codes.py on a build of commit e86c7e3, the last one whose fib verifier had a query kernel and an
opening kernel of its own.  What the order of the checks decides (two faults in one member) is part of the recording."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, golden

_spec = importlib.util.spec_from_file_location("make_fib_verify_many_codes", os.path.join(GOLDEN, "make_fib_verify_many_codes.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)


@pytest.fixture(scope="module")
def want():
    return golden("fib_verify_many_codes.json")


def test_the_recording_holds_what_it_is_for(want):
    """no class of members is empty, and every double fault has the answer the order of the checks dictates: wrong public values win
    over a count or depth word behind the header but not over a non-canonical word or a header count; the plain format reports a
    query's count words before the proof of work and before every query, the hiding format in query order"""
    make.check(want)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", make.CONFIGS, ids=make.name)
def test_every_status_is_the_parents(p3, oracle, want, cfg):
    """one batch per configuration: every word tampered, every word + P, the lengths +- 4, the double faults; both entries"""
    w = want[make.name(cfg)]
    for entry, g in zip(("verify_many", "verify_many_dev"), make.record_one(p3, oracle, cfg)):
        assert sorted(g) == sorted(w), entry
        assert g["words"] == w["words"], entry
        for cls in w:
            if cls == "words":
                continue
            assert len(g[cls]) == len(w[cls]), (entry, cls)
            diff = [(i, a, b) for i, (a, b) in enumerate(zip(g[cls], w[cls])) if a != b]
            assert not diff, (entry, cls, len(diff), diff[:8])
