"""CPU tests of tests/poseidon2_sched_ref.py: the exact models of the two fp64 schedules of Poseidon2 (p2f::permute, one state per lane;
p2q::permute, one state per DPP quad) against big-integer arithmetic, the pre-image builder, the magnitude-bound pass over both
schedules, the operand classes of the two probe ops added for the quad form, and the argument checks of the new test entries.  No GPU.

About 220 states go through the models (~0.025 s each per form); everything in bulk is compared through pyref."""
import ctypes as C
import math

import numpy as np
import pytest

import field_ref as F
import poseidon2_sched_ref as S
import pyref

P, H = S.P, S.H


def _modelled():
    """the family entries that go through both models: the structured targets at every seam, the single-lane ones at the seam that
    enters the internal rounds and at the last, eight random sign vectors per seam"""
    out = []
    names = [n for n, _ in S.targets()]
    for f in S.family():
        i = names.index(f[0])
        if i < S.NAMED or (i < S.NAMED + 32 and f[1] in (3, 7)) or (i >= S.NAMED + 32 and (i - S.NAMED - 32) % 8 == f[1]):
            out.append(f)
    return out


@pytest.fixture(scope="module")
def modelled():
    """((name, seam, state, raw_f, entry_f, raw_q, entry_q), ...) and the peaks of each form, computed once"""
    pf, pq, rows = S.Peaks(), S.Peaks(), []
    fam = [(n, seam, st) for n, seam, _, st in _modelled()]
    fam += [("edge %d" % st[0], None, tuple(st)) for st in S.EDGE_STATES]
    rng = np.random.default_rng([F.SEED, 17])
    fam += [("random %d" % i, None, tuple(int(v) for v in rng.integers(0, P, size=16))) for i in range(32)]
    for n, seam, st in fam:
        rf, ef = S.model_f(st, pf)
        rq, eq = S.model_q(st, pq)
        rows.append((n, seam, st, rf, ef, rq, eq))
    return rows, pf, pq


def test_family_shape():
    t = S.targets()
    assert len(t) == S.NAMED + 32 + 64 and len({n for n, _ in t}) == len(t)
    assert [n for n, _ in t[:S.NAMED]] == ["all +h", "all -h", "all (P+1)/2", "signs of V", "-signs of V", "alternating", "integer lanes"]
    assert t[0][1] == (H,) * 16 and t[1][1] == (-H,) * 16 and all((a - b) % P == 0 for a, b in zip(t[1][1], t[2][1]))
    assert t[3][1] == tuple(H * s for s in (-1, 1, 1, 1, 1, 1, -1, -1, -1, 1, 1, 1, -1, -1, -1, 1))
    assert t[6][1] == tuple(H if i in (1, 2, 4, 5, 7, 8, 12, 15) else 0 for i in range(16))
    for n, y in t[S.NAMED + 32:]:
        assert all(H - 3 <= abs(v) <= H for v in y) and len(set(np.sign(y))) == 2, n
    fam = S.family()
    assert len(fam) == 8 * len(t) and {f[1] for f in fam} == set(range(8))
    assert 180 <= len(_modelled()) <= 200


def test_preimages_are_canonical_and_invert():
    """seam_outputs (the forward permutation in plain integers, stopped at a seam) of preimage(y, seam) is y mod P, for every family
    state; and the builder is not the identity in disguise: two seams give different states for one target."""
    for n, seam, y, st in S.family():
        assert all(0 <= v < P for v in st) and len(st) == 16, (n, seam)
        assert S.seam_outputs(st, seam) == [v % P for v in y], (n, seam)
    assert len({f[3] for f in S.family()}) == 8 * (len(S.targets()) - 1)  # 'all -h' and 'all (P+1)/2' coincide mod P, nothing else does
    assert S.SBOX_INV_EXP * 7 % (P - 1) == 1 and pow(pow(12345, 7, P), S.SBOX_INV_EXP, P) == 12345
    ext_inv, int_inv = S._inverses()
    v = list(range(1, 17))
    assert S._apply(ext_inv, pyref._ext(v)) == v and S._apply(int_inv, pyref._int(v)) == v


def test_seam7_closed_form():
    """When the S-box outputs of the LAST external round are chosen, the permutation's output is one linear layer of them: for the
    all-+-h targets 35 h mod P (resp. -35 h) in every element.  No reference is involved."""
    exp = S.family_expected()
    for i, (n, seam, y, st) in enumerate(S.family()):
        if seam == 7:
            assert exp[i].tolist() == S.seam7_closed_form(y), n
            if n == "all +h":
                assert exp[i].tolist() == [35 * H % P] * 16
            if n in ("all -h", "all (P+1)/2"):
                assert exp[i].tolist() == [-35 * H % P] * 16


def test_models_equal_the_integers(modelled):
    """Both schedule models against pyref.poseidon2 on the modelled family states, the edge states and 32 random ones; every value the
    models formed was an integer below 2^53 (asserted where it is formed).  The peaks go into the failure message."""
    rows, pf, pq = modelled
    peaks = "p2f: %s; p2q: %s" % (pf.text(), pq.text())
    print(peaks)
    for n, seam, st, rf, ef, rq, eq in rows:
        want = pyref.poseidon2(list(st))
        assert S.words(rf) == want, ("p2f", n, seam, peaks)
        assert S.words(rq) == want, ("p2q", n, seam, peaks)
        assert [int(a) % P for a in ef] == [int(b) % P for b in eq], (n, seam)  # the same state enters the internal rounds
    for pk in (pf, pq):
        assert max(pk.values()) < 2.0 ** 53, peaks


def test_recorded_peaks(modelled):
    """The peaks DESIGN.md quotes (section 'Test strategy: the permutation forms').  The only CONDITION on a peak is < 2^53; the figures
    are compared so that the document follows the models.  The largest value either schedule forms is a x15 lane before a fold,
    2^50.66; the quad form passes 2^46.76 through add_scaled_pow2, outside the |x| < 2^44 the primitive states for its fractional
    multipliers (exact all the same: an integer multiplier leaves no fraction; op 48 of the field probe pins it there)."""
    _, pf, pq = modelled
    lg = lambda pk, k: round(math.log2(pk[k]), 2)  # noqa: E731
    assert (lg(pf, "lane before a fold"), lg(pq, "lane before a fold")) == (50.66, 50.66)
    assert (lg(pf, "lane sum before reduce"), lg(pq, "lane sum before reduce")) == (45.45, 45.45)  # 2^44.02 on the all-+-h states alone
    assert (lg(pf, "S-box input"), lg(pq, "S-box input")) == (36.08, 36.08)  # the first round on the all-(P - 1) state
    assert lg(pq, "add_scaled_pow2 operand") == 46.76 and lg(pf, "add_scaled_pow2 operand") < 36
    assert lg(pf, "S-box input") < 36.1 and lg(pq, "S-box input") < 36.1 and lg(pf, "store_elem operand") < 37
    assert pq["add_scaled_pow2 operand"] <= F.ASI_X and pq["reduced lane sum"] <= F.ASI_TOT and pf["S-box input"] <= F.SBOX_WIDE_IN


def test_worst_case_entry_of_the_internal_rounds(modelled):
    """The all-+-h targets at seam 3 enter the thirteen internal rounds at the header's worst case in ALL SIXTEEN elements, from words in
    [0, P) alone — asserted on the models' own values.  Which representative of +-h mod P sbox7 returns is a result of its rounding:
    in these models it is the far one, -+(h + 1) = +-h -+ P, so the entry is -+35 (h + 1) = -+35 (P + 1) / 2, which is 17.5 short of
    35 (P/2 + 1).  (A model that rounded the other way would enter at +-35 h; both are accepted, nothing smaller is.)"""
    rows, _, _ = modelled
    seen = 0
    for n, seam, st, rf, ef, rq, eq in rows:
        if seam == 3 and n in ("all +h", "all -h", "all (P+1)/2"):
            sign = 1 if n == "all +h" else -1
            for e in (ef, eq):
                assert len(set(e)) == 1 and e[0] in (sign * 35.0 * H, -sign * 35.0 * (H + 1)), (n, e[:2])
                assert abs(e[0]) >= 35 * H and (int(e[0]) - sign * 35 * H) % P == 0
            assert ef == eq
            seen += 1
    assert seen == 3


@pytest.mark.parametrize("form", ["p2f", "p2q"])
def test_magnitude_bounds_and_documented_preconditions(form):
    """|value| bounds pushed through each schedule from every entry contract that occurs: words in [0, P) (load_elem), |s| <= P/2 + eps
    (the reduce between two absorptions), 2^32 (what the headers now state) and 2^33 (what they used to state; the probe's modes 0 and
    3 still run it).  Every bound is below 2^53 (asserted inside the pass), and every call site meets the documented precondition of
    the primitive it calls — mulmod_m: |b aP| < 2^51, |ab| < 2^76; add_scaled_pow2 with a fractional multiplier: |x| < 2^44, |tot| < 2^40;
    store_elem: |v| < 2^37 — with ONE exception, listed here and not relaxed: from 2^33 the first round's x * x reaches 2^76.28.
    Two header comments were corrected on this evidence (csrc/poseidon2_f64.hip.h): the largest S-box input is the first round's
    35 (P - 1) + rc = 2^36.08, not 35 (P/2 + 1) < 2^36; and the entry bound the S-box contract supports is 2^32.  The integer
    multipliers of the quad form take add_scaled_pow2 to |x| = 2^46.76: no fraction arises, the bound that matters there is
    |tot + m x| < 2^53 (csrc/poseidon2_q4.hip.h now says so)."""
    for name, entry in S.ENTRY_CONTRACTS.items():
        bp = S.bound_pass(form, entry)
        if name == "the header's 2^33":
            assert [(e[1], e[2]) for e in bp.exceeded] == [("sbox7 x * x", "mulmod_m |ab| < 2^76")], bp.exceeded
            assert (1 << 76) <= bp.exceeded[0][3] < (1 << 77)
        else:
            assert bp.exceeded == [], (name, bp.exceeded)
        assert max(bp.peak.values()) < 1 << 53
    words = S.bound_pass(form, P - 1)
    assert words.peak["S-box input"] == 35 * (P - 1) + P - 1 <= F.SBOX_WIDE_IN and 36.0 < math.log2(words.peak["S-box input"]) < 36.1
    assert words.peak["add_scaled_pow2 operand"] <= (F.ASI_X if form == "p2q" else 1 << 44)


def test_sbox_model_is_exact_beyond_its_documented_bound():
    """The one exceeded precondition above, checked where it is exceeded: sbox7's exact model against x^7 mod P at 300 operands each
    around 2^36.2, 2^37.15 (entry 2^32), 2^38.14 (entry 2^33: the largest, 35 * 2^33 + P - 1, included) and 2^39; and both schedule
    models on +-2^33 in all sixteen elements against big-integer arithmetic."""
    rng = np.random.default_rng([F.SEED, 18])
    for top in (int(2 ** 36.2), 35 * 2 ** 32 + P - 1, 35 * 2 ** 33 + P - 1, 2 ** 39):
        for x in [top, -top] + [int(v) * (1, -1)[i & 1] for i, v in enumerate(rng.integers(top - (top >> 4), top + 1, size=298))]:
            w = F.m_sbox7(float(x))
            assert w.is_integer() and (int(w) - pow(x, 7, P)) % P == 0 and abs(w) <= P / 2 + 2 ** 9, x
    for st in ([2 ** 33] * 16, [-2 ** 33] * 16, [(2 ** 33) * (1, -1)[i & 1] for i in range(16)]):
        want = pyref.poseidon2([v % P for v in st])
        assert S.words(S.model_f(st)[0]) == want and S.words(S.model_q(st)[0]) == want


def test_new_probe_classes_follow_from_the_operands_and_their_models_are_exact():
    """Op 48, add_scaled_pow2 with the integer multipliers of the quad form's diagonal: |x| up to 15^3 35 (P/2 + 2^9) + 241 (P/2 + 1)
    (the bound pass's largest operand: 15^3 35 (P/2 + 1) and the lane sums three rounds add to it), |tot| <= P/2 + 1, every sign
    pattern; the model returns tot + m x itself.  Op 49, sbox7 up to 35 (P - 1) + P."""
    x, lab = F.lanes("add_scaled_int")
    assert F.ASI_X >= S.bound_pass("p2q", P - 1).peak["add_scaled_pow2 operand"] > 15 ** 3 * 35 * (P // 2 + 1) and F.ASI_TOT == P // 2 + 1
    for m in F.ASI_MULTIPLIERS:
        sel = x[lab == "m = %d" % m]
        assert np.all(sel[:, 2] == m) and np.abs(sel[:, 1]).max() == F.ASI_X and np.abs(sel[:, 0]).max() == F.ASI_TOT
        assert {(a, b) for a, b in zip(np.sign(sel[:, 0]), np.sign(sel[:, 1]))} >= {(s, t) for s in (-1, 1) for t in (-1, 1)}
        assert np.count_nonzero(np.abs(sel[:, 1]) >= 2.0 ** 46) >= F.MIN_LANES
    assert sorted(set(x[:, 2].tolist())) == sorted(float(m) for m in F.ASI_MULTIPLIERS)
    assert sorted(F.ASI_MULTIPLIERS) == sorted(int(v) for v in S.V if float(v).is_integer())
    for (tot, xx, m), w in zip(x.tolist(), F.model("add_scaled_int").tolist()):
        assert w == tot + m * xx and int(w) == int(tot) + int(m) * int(xx) and abs(w) < 2.0 ** 53
    x, lab = F.lanes("sbox7_wide")
    assert np.abs(x).max() == F.SBOX_WIDE_IN == 35 * (P - 1) + P
    assert np.abs(x[lab == "above 35 (P/2 + 1) + P"]).min() > F.SBOX_IN + P
    for v, w in zip(x[:, 0].tolist(), F.model("sbox7_wide").tolist()):
        assert w.is_integer() and (int(w) - pow(int(v), 7, P)) % P == 0 and abs(w) <= P / 2 + 2 ** 9, v


def test_new_entries_refuse_bad_arguments_before_any_gpu_call(p3):
    """The argument checks of the test entries added for the permutation forms come before the device context is looked up: an unknown
    variant, mode or hash, a null pointer, a layer the levels kernels cannot take.  n = 0 is a no-op."""
    from plonky3_mobile_amd import _lib
    lib = _lib.lib()
    assert {"p3hip_keccak_f_variant_dev", "p3hip_compress_layer_variant_dev"} <= set(_lib.declared_symbols())
    buf = np.zeros(64, np.uint64)
    ptr = C.c_void_p(buf.ctypes.data)  # never dereferenced: every call below is refused, or n = 0
    for v in (-1, 4, 1 << 20):
        assert lib.p3hip_poseidon2_permute_variant_dev(ptr, 1, v, None) == -1 and "poseidon2 variant" in p3.take_last_error()
    for m in (-1, 4):
        assert lib.p3hip_poseidon2_f64_probe_dev(ptr, ptr, 1, m, None) == -1 and "probe mode" in p3.take_last_error()
    for v in (-1, 3):
        assert lib.p3hip_keccak_f_variant_dev(ptr, 1, v, None) == -1 and "keccak_f variant" in p3.take_last_error()
    assert lib.p3hip_keccak_f_variant_dev(None, 1, 0, None) == -1 and "null" in p3.take_last_error()
    for v in range(4):
        assert lib.p3hip_poseidon2_permute_variant_dev(None, 1, v, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_poseidon2_permute_variant_dev(None, 0, v, None) == 0
        assert lib.p3hip_poseidon2_f64_probe_dev(None, None, 0, v, None) == 0
    for v in range(3):
        assert lib.p3hip_keccak_f_variant_dev(None, 0, v, None) == 0
    for hash, v in ((2, 0), (-1, 0), (0, 4), (0, -1), (1, 3)):
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, 1, None) == -1 and "compress_layer_variant" in p3.take_last_error()
    for hash, v in ((0, 3), (1, 1), (1, 2)):
        for n in (3, 6, 65, 257):
            assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, n, None) == -1 and "power-of-two" in p3.take_last_error()
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, 1 << 16, None) == -1 and "2^15" in p3.take_last_error()
    for hash, v in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2)):
        assert lib.p3hip_compress_layer_variant_dev(hash, v, None, ptr, 1, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, None, 1, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, (1 << 24) + 1, None) == -1
        p3.take_last_error()
        assert lib.p3hip_compress_layer_variant_dev(hash, v, None, None, 0, None) == 0
    assert p3.take_last_error() is None and not buf.any()
