"""CPU tests of tests/poseidon2_dyadic_ref.py, the exact model of p2f::internal_rounds with dyadic lanes (csrc/poseidon2_f64.hip.h):
congruent to big-integer rounds and exact (no step rounds: asserted inside the model) on the sign patterns at the three magnitudes,
the all-zero and single-lane +-(2^37 - 1) entries, the 103 seam-3 family entries and 300 random ones; the ledger of fractional bits;
the exit bound; the whole permutation on the family and the edge states; the operation count against the header and
profiles/hash_instruction_floor_dyadic.txt; and the fold-edge entries of the GPU test, which must show the fractional parts they were
built for IN THE MODEL.  No GPU.  About 450 entries of ~8 ms and 828 whole permutations of ~35 ms."""
import math
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

import field_ref as F
import poseidon2_dyadic_ref as D
import poseidon2_sched_ref as S
import pyref

P = D.P


@pytest.fixture(scope="module")
def runs():
    """every listed entry through the model once: ((entry, raw doubles out), ...) and the Run that saw them all"""
    run = D.Run()
    entries = D.pattern_entries() + D.seam3_entries() + D.random_entries(300, 20)
    rows = []
    for e in entries:
        before = run.ops
        rows.append((e, D.internal_rounds(run, e)))
        assert run.ops - before == D.OPS_PER_PERMUTATION, e
    return rows, run


def test_entry_sets():
    pat, fam = D.pattern_entries(), D.seam3_entries()
    assert len(pat) == 15 + 1 + 32 and len(fam) == 103 == len(S.targets())
    assert max(abs(v) for e in pat for v in e) == 2 ** 37 - 1 and (0,) * 16 in pat
    assert {max(abs(v) for v in e) for e in pat[:15]} == {P - 1, 35 * (P // 2 + 2 ** 9), 2 ** 37 - 1}
    assert fam[0] == (35 * S.H,) * 16 and fam[1] == (-35 * S.H,) * 16  # one external layer of all +-h: 35 y
    for (n, y), e in zip(S.targets(), fam):
        assert [v % P for v in e] == pyref._ext([v % P for v in y]), n
    assert len(set(D.random_entries(300, 20))) == 300


def test_model_is_congruent_to_the_integers(runs):
    """internal_rounds of the model against thirteen big-integer rounds; every step was exact (asserted where it is made)"""
    rows, run = runs
    print(run.pk.text())
    for e, out in rows:
        assert all(v.is_integer() for v in out) and [int(v) % P for v in out] == D.reference_rounds(e), e


def test_ledger_and_bounds(runs):
    """Fractional bits never pass the budget at a sum (14 is the most a sum sees: a lane that reaches 16 is folded in the round that
    takes it there); magnitude + fraction fits 53 bits at every site (asserted by Peaks.recd); exit below 2^37.  The figures are the
    ones the header quotes."""
    _, run = runs
    pk = run.pk
    assert run.ledger_peak == 14 <= D.BUDGET == 16
    assert pk["exit"] < 2.0 ** 37 and pk["exit"] < 2.0 ** 31.7
    assert pk["dyadic partial sum"] < 2.0 ** 39.9 and pk["integer partial sum"] < 2.0 ** 50.3 and pk["lane before a fold"] < 2.0 ** 52.7
    assert pk["reduced lane sum"] <= P / 2 + 1
    assert D.DYADIC_FOLDS == {3: (12,), 6: (12,), 9: (1, 3, 5, 7, 9, 11, 12), 10: (7, 12), 11: (4, 9, 12), 13: (1, 3, 5, 7, 9, 11, 12),
                              14: (3, 7, 11, 12)}


def test_a_wider_budget_is_exact_too():
    """18 fractional bits (the k = 8 lanes still fold every second round, k = 2 after nine rounds, k = 3 after six): exact on the
    largest entries, so 16 has margin."""
    run = D.Run(budget=18)
    for e in D.pattern_entries():
        assert [int(v) % P for v in D.internal_rounds(run, e)] == D.reference_rounds(e)
    assert run.ledger_peak == 16


def test_simulate_agrees_with_the_integers_and_the_model(runs):
    """simulate(), the integer form of the same schedule that builds the fold-edge entries: its residues are big-integer rounds, and
    the numerators it reports before each fold are the doubles the model forms there"""
    rows, _ = runs
    ents = [e for e, _ in rows[:80]]
    res, folds, sums = D.simulate(np.array(ents, dtype=np.int64))
    for j, e in enumerate(ents):
        assert res[j].tolist() == D.reference_rounds(e)
    run = D.Run()
    for j in (0, 5, 14, 20, 60):
        D.internal_rounds(run, ents[j])
        for (what, lane, r), (v, bits) in run.seen.items():
            n, f = sums[r] if what == "sum" else folds[(lane, r)]
            assert Fr(v) == Fr(int(n[j]), 1 << f) and f == bits, (what, lane, r)


def test_fold_edge_entries_hit_their_fractions_in_the_model():
    """Each entry of the GPU test's fold-edge family, through the model: the double entering the named fold_dyadic has the fractional
    part and the sign it was built for, and the rounds stay exact and congruent."""
    fe = D.fold_edge_entries()
    assert len(fe) == 7 * 3 * 2 + 2 * 2 * 2
    seen = set()
    for what, lane, r, want, sign, e in fe:
        run = D.Run()
        out = D.internal_rounds(run, e)
        assert [int(v) % P for v in out] == D.reference_rounds(e)
        v, _ = run.seen[(what, lane, r)]
        f = D.DYADIC_K[lane] * (r + 1) if what == "lane" else {1: 8, 7: 14}[r]
        assert Fr(v) - math.floor(v) == Fr(want, 1 << f) and (v > 0) == (sign > 0) and abs(v) > 1, (what, lane, r, want, sign, v)
        assert max(abs(x) for x in e) < 2 ** 37
        seen.add((what, lane, r, Fr(want, 1 << f), sign))
    for lane, k in D.DYADIC_K.items():
        r = D.DYADIC_FOLDS[lane][0]
        f = k * (r + 1)
        assert {(fr, sg) for w, ln, rr, fr, sg in seen if w == "lane" and ln == lane} == {(x, s) for x in (0, Fr(1, 1 << f), 1 - Fr(1, 1 << f)) for s in (1, -1)}
    assert {(rr, fr, sg) for w, ln, rr, fr, sg in seen if w == "sum"} == {(r, x, s) for r, f in ((1, 8), (7, 14)) for x in (0, 1 - Fr(1, 1 << f)) for s in (1, -1)}


def test_whole_permutation_on_the_family_and_the_edge_states():
    """poseidon2_sched_ref._permute with the dyadic internal rounds plugged in, on the WHOLE family() (every target at every seam: 824
    states) and on EDGE_STATES, against family_expected() and pyref.poseidon2.  About half a minute: the longest test of this file."""
    exp = S.family_expected()
    fam = S.family()
    assert len(fam) == 8 * 103 == len(exp)
    run = D.Run()
    for j, (n, seam, y, st) in enumerate(fam):
        raw, _ = D.model_d(st, run)
        assert S.words(raw) == exp[j].tolist(), (n, seam)
    for st in S.EDGE_STATES:
        assert S.words(D.model_d(st, run)[0]) == pyref.poseidon2(list(st))
    assert run.pk["store_elem operand"] < 2.0 ** 37 and run.ledger_peak == 14


def test_operation_count_is_what_the_documents_state():
    """566 operations outside the S-box, 720 before: the model's counter (asserted per entry in the fixture), the formula, the
    header's comment and the profiles file agree, so a schedule change cannot leave the documents behind"""
    assert (D.OPS_PER_PERMUTATION, D.OPS_PREVIOUS) == (566, 720)
    n_dy = sum(len(v) for v in D.DYADIC_FOLDS.values())
    n_int = sum(len(v) for v in D.INTEGER_FOLDS.values())
    assert (n_dy, n_int, D.OPS_PER_ROUND) == (25, 16, 36)
    hdr = open(os.path.join(F.ROOT, "plonky3-mobile_amd", "csrc", "poseidon2_f64.hip.h")).read()
    assert "= 468, + 25 dyadic folds x 2 + 16 reduces x 3" in hdr and "= 566 (it was 13 x 48 + 96 = 720" in hdr
    assert "constexpr int FRAC_BUDGET = %d;" % D.BUDGET in hdr
    masks = {k: sum(1 << r for r in D.dyadic_folds(k)) for k in (1, 2, 3, 4, 8)}
    m = re.search(r"static_assert\(FOLD_K1 == (\w+) && FOLD_K2 == (\w+) && FOLD_K3 == (\w+) && FOLD_K4 == (\w+) && FOLD_K8 == (\w+),", hdr)
    assert [int(v, 16) for v in m.groups()] == [masks[k] for k in (1, 2, 3, 4, 8)]
    m = re.search(r"FOLD_X2 = (.*?), FOLD_X4 = (.*?), FOLD_X15 = (.*?);", hdr)
    rounds = [sorted(int(r) for r in re.findall(r"1u << (\d+)", g)) for g in m.groups()]
    assert rounds == [list(D.INTEGER_FOLDS[i]) for i in (1, 4, 12)]
    assert all(D.INTEGER_FOLDS[a] == D.INTEGER_FOLDS[b] for a, b in ((1, 2), (4, 5), (4, 7), (4, 8), (12, 15)))
    prof = open(os.path.join(F.ROOT, "profiles", "hash_instruction_floor_dyadic.txt")).read()
    assert re.search(r"internal rounds, linear part and folds[^\n]*\b566\b", prof) and re.search(r"\b720\b", prof)
    assert re.search(r"arithmetic count of this formulation\s+%d\b" % (4152 - 720 + 566), prof)
