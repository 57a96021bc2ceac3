"""CPU tests of the field probe's reference, exact fp64 model and operand classes (tests/field_ref.py), and of the HOST branches of
the integer and extension primitives through p3hip_field_probe_host.  No GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import field_ref as F
from conftest import ROOT

P = F.P
HALF = P / 2.0


def probe_host(p3, name, x):
    from plonky3_mobile_amd import _lib
    op, k, m, _ = F.OPS[name]
    x = np.ascontiguousarray(x)
    assert x.shape[1] == k
    out = np.zeros((len(x), m), dtype=x.dtype)
    _lib.check(_lib.lib().p3hip_field_probe_host(op, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), len(x)))
    return out


# ---- the operand classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.OPS))
def test_every_class_is_populated(name):
    """A condition, not a measurement: every class named for an op holds at least MIN_LANES lanes, and no lane is unlabelled."""
    x, lab = F.lanes(name)
    cnt = collections.Counter(lab.tolist())
    assert set(cnt) == set(F.CLASSES[name])
    assert all(cnt[c] >= F.MIN_LANES for c in F.CLASSES[name]), {c: cnt[c] for c in F.CLASSES[name] if cnt[c] < F.MIN_LANES}
    x2, lab2 = F.lanes.__wrapped__(name)  # a function of the seed alone
    assert np.array_equal(x, x2) and np.array_equal(lab, lab2)
    ids = [F.class_id(c) for c in F.CLASSES[name]]
    assert len(set(ids)) == len(ids)


def test_edge_set():
    e = set(F.E)
    assert {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, F.ONE, F.R2, F.W_MONTY} <= e and max(e) < P
    for k in range(31):
        assert {v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v < P} <= e
    assert 1 << 30 in e and (1 << 30) + 1 in e and 1 << 31 not in e


def _sel(name, cls):
    x, lab = F.lanes(name)
    return x[lab == cls].astype(np.uint64)


def test_mul_labels_follow_from_the_operands():
    near = {"r' = P-2": P - 2, "r' = P-1": P - 1, "r' = P+1": P + 1, "r' = P+2": P + 2}
    for cls, v in near.items():
        s = _sel("mul", cls)
        assert np.all(F.v_rprime(s[:, 0] * s[:, 1])[0] == np.uint64(v)), cls
    s = _sel("mul", "lo(ab) = 0 (t = 0)")
    rp, t = F.v_rprime(s[:, 0] * s[:, 1])
    assert np.all((s[:, 0] * s[:, 1]) & np.uint64(F.M32) == 0) and np.all(t == 0) and np.all(s > 0)
    s = _sel("mul", "t = 2^32-1")
    assert np.all(F.v_rprime(s[:, 0] * s[:, 1])[1] == np.uint64(F.M32)) and len(np.unique(s, axis=0)) >= F.MIN_LANES
    s = _sel("mul", "ab = 0 (mod P)")
    assert np.all(s[:, 0] * s[:, 1] == 0)
    s = _sel("mul", "largest r' of the search")
    top = F.v_rprime(s[:, 0] * s[:, 1])[0]
    # r' < (P^2 + 2^32 P) / 2^32 = 1.469 P: the search comes within a thousandth of that bound, on the far side of P
    assert np.all(top > np.uint64(1.468 * P)) and np.all(top < np.uint64((P * P + (P << 32)) >> 32))
    x, _ = F.lanes("mul")
    assert np.all(x < P)


def test_mul_cannot_reach_r_prime_equal_to_p():
    """r' = (ab + tP) / 2^32 is congruent to ab 2^-32: r' = P needs ab = 0 (mod P), so a = 0 or b = 0 (P is prime and a, b < P), and then
    x = 0, t = 0, r' = 0.  A search over every lane of the op, and over the construction that reaches P for dot2, finds none."""
    x, _ = F.lanes("mul")
    x = x.astype(np.uint64)
    assert not np.any(F.v_rprime(x[:, 0] * x[:, 1])[0] == np.uint64(P))
    rng = np.random.default_rng(F.SEED)
    a = rng.integers(0, P, size=1 << 20, dtype=np.uint64)
    b = np.where(rng.integers(0, 2, size=1 << 20) == 0, np.uint64(0), rng.integers(0, P, size=1 << 20, dtype=np.uint64))
    assert not np.any(F.v_rprime(a * b)[0] == np.uint64(P))


def test_dot2_labels_follow_from_the_operands():
    def xs(cls):
        s = _sel("dot2", cls)
        return s, s[:, 0] * s[:, 1] + s[:, 2] * s[:, 3]
    s, x = xs("cancelling (r' = P)")
    # the one class in which the value before the correction is P itself: x a nonzero multiple of P
    assert np.all(x % np.uint64(P) == 0) and np.all(x > 0) and np.all(F.v_rprime(x)[0] == np.uint64(P))
    assert len(np.unique(s, axis=0)) >= F.MIN_LANES and np.all(s > 0)
    for cls, v in {"r' = P-2": P - 2, "r' = P-1": P - 1, "r' = P+1": P + 1, "r' = P+2": P + 2}.items():
        assert np.all(F.v_rprime(xs(cls)[1])[0] == np.uint64(v)), cls
    s, x = xs("lo(x) = 0")
    assert np.all(x & np.uint64(F.M32) == 0) and np.all(x > 0) and np.all(F.v_rprime(x)[1] == 0)
    assert np.all(xs("x >= 2^62")[1] >= np.uint64(1 << 62))
    assert np.all(xs("all P-1")[0] == np.uint64(P - 1))
    top = F.v_rprime(xs("largest r' of the search")[1])[0]
    assert np.all(top > np.uint64(1.936 * P)) and np.all(top < np.uint64(2 * P))  # bound: (2 (P-1)^2 + 2^32 P) / 2^32 = 1.9375 P
    assert np.count_nonzero(F.lanes("dot2")[1] == "uniform") == 1 << 18
    assert np.all(F.lanes("dot2")[0] < P)


def test_dot2_sum_cannot_reach_2_63():
    """The issue asked for the class x >= 2^63.  It is empty: x <= 2 (P-1)^2 = 0.879 * 2^63, which is also why the 64-bit sum cannot
    wrap.  The nearest class that exists, x >= 2^62 (no single product reaches it: (P-1)^2 < 2^62), stands in for it."""
    assert 2 * (P - 1) ** 2 < 1 << 63 and (P - 1) ** 2 < 1 << 62 <= 2 * (P - 1) ** 2
    x = F.lanes("dot2")[0].astype(np.uint64)
    assert not np.any(x[:, 0] * x[:, 1] + x[:, 2] * x[:, 3] >= np.uint64(1 << 63))


def test_smul_and_sbox7_add_labels_follow_from_the_operands():
    x, lab = F.lanes("smul")
    s = x.view(np.int32).astype(np.int64)
    assert np.all(np.abs(s) < P)
    lo = (s[:, 0] * s[:, 1]) & F.M32
    for cls, v in (("lo(ab) = 0", 0), ("lo(ab) = 0x80000000", 1 << 31), ("lo(ab) = 0xffffffff", F.M32)):
        assert np.all(lo[lab == cls] == v) and np.all(s[lab == cls] != 0), cls
    assert {tuple(r) for r in s[lab == "edges {0, +-1, +-(P-1)}^2"].tolist()} == {(a, b) for a in (0, 1, -1, P - 1, 1 - P) for b in (0, 1, -1, P - 1, 1 - P)}
    x, lab = F.lanes("sbox7_add")
    x = x.astype(np.int64)
    assert np.all(x < P)
    for t, v in (("-P", -P), ("-P+1", -P + 1), ("-1", -1), ("0", 0), ("1", 1), ("P-2", P - 2)):
        assert np.all(x[lab == "s + rc - P = " + t].sum(axis=1) - P == v), t
    assert (0, 0) in {tuple(r) for r in x[lab == "s + rc - P = -P"].tolist()}  # the closed end of the S-box's input interval [-P, P)
    assert {tuple(r) for r in x[lab == "rc16 x E"].tolist()} == {(s, rc) for rc in F.rc16_words() for s in F.E}


def test_extension_labels_follow_from_the_operands():
    x, lab = F.lanes("ext_inv")
    can = F.v_canon(x)
    for cls, want in (("norm d = 0", (True, False)), ("norm c = 0", (False, True))):  # (c != 0, d != 0)
        for row in can[lab == cls]:
            c, d = F.ext_norm_canon(row)
            assert (c != 0, d != 0) == (want[0], want[1]) and all(int(v) for v in row), cls
    assert np.all(x[lab == "base field"][:, 1:] == 0) and np.all(x[lab == "base field"][:, 0] != 0)
    s = x[lab == "c1 = c3 = 0"]
    assert np.all(s[:, [1, 3]] == 0) and np.all(s[:, [0, 2]] != 0)
    s = x[lab == "c0 = c2 = 0"]
    assert np.all(s[:, [0, 2]] == 0) and np.all(s[:, [1, 3]] != 0)
    assert np.all(x[lab == "zero"] == 0)
    g = {tuple(r) for r in x[lab == "grid 625"].tolist()}
    assert len(g) == 625 and all(v in F.GRID5 for r in g for v in r)
    x, lab = F.lanes("ext_mul")
    pairs = {tuple(r) for r in x[lab == "grid 625 x 625"].tolist()}
    assert len(pairs) == 390625 and np.count_nonzero(lab == "uniform") == 1 << 14
    for name, w in (("pow", 1), ("ext_pow", 4)):
        x, lab = F.lanes(name)
        e = x[:, w].astype(np.uint64) | (x[:, w + 1].astype(np.uint64) << np.uint64(32))
        for ex in F.EXPONENTS:
            s = lab == "e = %d" % ex
            assert np.all(e[s] == np.uint64(ex))
            b = {tuple(r) for r in x[s][:, :w].tolist()}
            assert {(0,) * w, (F.ONE,) + (0,) * (w - 1), (P - 1,) * w} <= b and len(b) >= F.MIN_LANES
    assert sorted(set(F.lanes("two_adic_generator")[0][:, 0].tolist())) == list(range(28))


@pytest.mark.parametrize("name", ["mulmod", "mulmod_p", "mulmod_p_dev", "mulmod_m", "mulmod_m_dev", "mulm", "mulm_dev"])
def test_product_labels_follow_from_the_operands(name):
    a, b, aP = F.product_operands(name)
    _, lab = F.lanes(name)
    ai, bi = [int(v) for v in a], [int(v) for v in b]
    assert all(float(u) == v for u, v in zip(ai, a)) and all(float(u) == v for u, v in zip(bi, b))
    if aP is not None:
        assert np.array_equal(aP, a / F.PD)
    half = P // 2 + 2
    seen = set()
    for u, v, cls in zip(ai, bi, lab.tolist()):
        assert abs(u * v) < 1 << 76 and abs(v * u) < (P << 51), (u, v)  # |ab| < 2^76, |b a/P| < 2^51
        m = re.match(r"(canonical|centred) a, \|b\| in 2\^(\d+), (uniform|ab = (.*) \(mod P\))$", cls)
        if m:
            assert (0 < u < P) if m.group(1) == "canonical" else (0 < abs(u) <= half), cls
            assert abs(v).bit_length() - 1 == int(m.group(2)), cls
            if m.group(4):
                assert (u * v - F.NEAR_TIE[m.group(4)]) % P == 0, cls  # ab / P is within 2 / P < 2^-29 of a half-integer
            seen.add((cls, v > 0))
        elif cls == "a = 0":
            assert u == 0 and v != 0
        elif cls == "b = 0":
            assert v == 0 and u % P
        elif cls == "b = kP":
            assert v and v % P == 0 and u % P
        else:
            assert cls == "both up to 35 (P/2 + 1)" and max(abs(u), abs(v)) <= F.SBOX_IN
    assert len(seen) == 2 * 2 * len(F.BINADES) * (1 + len(F.NEAR_TIE))  # every class with b of both signs
    if name.startswith("mulmod_m"):
        s = lab == "both up to 35 (P/2 + 1)"
        assert {(F.SBOX_IN, F.SBOX_IN), (-F.SBOX_IN, F.SBOX_IN), (F.SBOX_IN, -F.SBOX_IN), (-F.SBOX_IN, -F.SBOX_IN)} <= set(zip(a[s].tolist(), b[s].tolist()))


def test_other_fp64_labels_follow_from_the_operands():
    x, lab = F.lanes("word_any")
    v = [int(t) for t in x[:, 0]]
    assert max(abs(t) for t in v) < 1 << 43 and max(v) + P >= 1 << 43 and min(v) - P <= -(1 << 43)  # up to the stated limit, both signs
    for t, cls in zip(v, lab.tolist()):
        off, sign = cls.split(", k ")
        d = {"kP": 0, "kP+1": 1, "kP-1": -1, "kP+(P-1)": P - 1}[off]
        assert (t - d) % P == 0 and (((t - d) // P < 0) == (sign == "< 0")), cls
    x, lab = F.lanes("word_centered")
    top = (P - 1) // 2 + (1 << 22)
    assert {0, 1, -1, (P - 1) // 2, -(P - 1) // 2, (P + 1) // 2, -(P + 1) // 2, top, -top} == set(x[lab == "edges"][:, 0].tolist())
    assert np.abs(x).max() == top
    x, lab = F.lanes("add_scaled_pow2")
    assert len({(int(np.log2(abs(i))), i > 0) for i in x[:, 2]}) == len(F.ASP_FORMS)
    for k, s in F.ASP_FORMS:
        sel = x[lab == "K = %d, inv %s 0" % (k, "<>"[s > 0])]
        assert np.all(sel[:, 2] == s * 2.0 ** -k) and np.abs(sel[:, 0]).max() < 2 ** 40 and np.abs(sel[:, 1]).max() < 2 ** 44
        assert np.abs(sel[:, 0]).min() >= 2 ** 39 and np.abs(sel[:, 1]).min() >= 2 ** 43  # the stated magnitudes
        for sx in (-1, 1):
            for st in (-1, 1):
                q = sel[(np.sign(sel[:, 1]) == sx) & (np.sign(sel[:, 0]) == st)]
                assert {int(t) % (1 << k) for t in q[:, 1]} == set(range(1 << k)), (k, s, sx, st)  # every residue, every sign pattern
    x, lab = F.lanes("store_elem")
    assert np.abs(x).max() == 2 ** 37 - 1
    for t, rho in F.NEAR_TIE.items():
        for s in "<>":
            sel = x[lab == "v 2^32 = %s (mod P), v %s 0" % (t, s)][:, 0]
            assert all((int(v) * F.R - rho) % P == 0 for v in sel) and np.all((sel > 0) == (s == ">")) and len(set(sel.tolist())) >= F.MIN_LANES
    x, lab = F.lanes("sbox7")
    assert np.abs(x).max() == F.SBOX_IN + P and {0.0, float(-P), float(F.SBOX_IN + P), float(-F.SBOX_IN - P)} <= set(x[:, 0].tolist())


# ---- the reference against itself -------------------------------------------------------------------------------------------------
def test_reference_against_plain_integers():
    rng = np.random.default_rng(3)
    for a, b, c, d in rng.integers(0, P, size=(200, 4)).tolist() + [[P - 1] * 4, [0, 0, 0, 0], [1, P - 1, P - 1, 1]]:
        row = np.array([[a, b, c, d]], np.uint64)
        assert int(F.reference("mul", row[:, :2])[0, 0]) == a * b * F.RINV % P
        assert int(F.reference("dot2", row)[0, 0]) == (a * b + c * d) * F.RINV % P
        assert int(F.reference("sbox7_add", row[:, :2])[0, 0]) == F.monty(pow(F.canon(a) + F.canon(b), 7, P))
        assert int(F.reference("pow7", row[:, :1])[0, 0]) == F.monty(pow(F.canon(a), 7, P))
        assert int(F.reference("inv", row[:, :1])[0, 0]) == (F.monty(pow(F.canon(a), -1, P)) if a else 0)
        assert int(F.reference("from_monty", row[:, :1])[0, 0]) == F.canon(a) and int(F.reference("to_monty", row[:, :1])[0, 0]) == F.monty(a)
        e = (c << 32) | d
        assert int(F.reference("pow", np.array([[a, d, c]], np.uint64))[0, 0]) == F.monty(pow(F.canon(a), e, P))
    for a in (-(P - 1), -1, 0, 1, P - 1, 12345, -(1 << 30)):
        for b in (-(P - 1), -1, 0, 1, P - 1, -54321, 1 << 30):
            r = F.smul_ref(a, b)
            assert abs(r) < P and (r * F.R - a * b) % P == 0  # Seiler: (-P, P) in, (-P, P) out
    assert F.smul_ref(-P, -P) == 0  # the S-box's closed end: x = -P from s = rc = 0 squares to 0


def test_extension_reference():
    x, lab = F.lanes("ext_inv")
    can = F.v_canon(x)
    inv = F.v_canon(F.reference("ext_inv", x))
    prod = F.v_ext_mul_canon(can, inv)
    nz = np.any(x != 0, axis=1)
    assert np.all(prod[nz] == np.array([1, 0, 0, 0], np.uint64)) and np.all(inv[~nz] == 0)  # a a^-1 = 1 on every lane; inv(0) = 0
    rng = np.random.default_rng(4)
    for i in rng.choice(np.flatnonzero(nz), size=40, replace=False).tolist() + np.flatnonzero(np.isin(lab, ["norm d = 0", "norm c = 0"]))[:8].tolist():
        assert F.ext_inv_linear([int(v) for v in can[i]]) == [int(v) for v in inv[i]]  # a^(P^4 - 2) against the linear solve
    # x^4 = 11, and the product is the schoolbook one
    xx = np.array([[0, 1, 0, 0]], np.uint64)
    assert F.v_ext_pow_canon(xx, 4).tolist() == [[11, 0, 0, 0]]
    a, b = [3, 5, 7, 9], [2, 4, 6, 8]
    want = [0] * 7
    for i in range(4):
        for j in range(4):
            want[i + j] += a[i] * b[j]
    want = [(want[k] + 11 * (want[k + 4] if k + 4 < 7 else 0)) % P for k in range(4)]
    assert F.v_ext_mul_canon(np.array([a], np.uint64), np.array([b], np.uint64)).tolist() == [want]
    # two_adic_generator(b): g^(2^b) = 1 and g^(2^(b-1)) = -1
    for b in range(28):
        g = F.canon(int(F.reference("two_adic_generator", np.array([[b]], np.uint64))[0, 0]))
        assert pow(g, 1 << b, P) == 1 and (b == 0 or pow(g, 1 << (b - 1), P) == P - 1), b


# ---- the exact fp64 models against the integers ------------------------------------------------------------------------------------
def _ints(v):
    assert all(float(t).is_integer() for t in v)
    return [int(t) for t in v]


@pytest.mark.parametrize("name", ["mulmod", "mulmod_p", "mulmod_p_dev", "mulmod_m", "mulmod_m_dev", "mulm", "mulm_dev"])
def test_product_models_are_exact_and_within_their_stated_bounds(name):
    a, b, _ = F.product_operands(name)
    a, b, r = _ints(a), _ints(b), _ints(F.model(name))  # every result is an integer
    worst = 0.0
    for u, v, w in zip(a, b, r):
        assert (w - u * v) % P == 0, (u, v, w)
        if name == "mulmod":
            assert abs(w) < 1.1 * P, (u, v, w)                      # poseidon2_f64.hip.h, head comment
        else:
            assert abs(w) <= HALF + 1 + abs(u * v) * 2.0 ** -52, (u, v, w)  # mulmod_p's comment; mulmod_m is "the same product"; mulm's
        if name.startswith("mulm") and not name.startswith("mulmod") and abs(v) <= 1 << 43:
            assert abs(w) <= (0.5 + 2.0 ** -9) * P                  # ntt_narrow_f64.hip.h
        if name.startswith("mulm") and not name.startswith("mulmod") and abs(v) < 1 << 42:
            assert abs(w) <= HALF + 2 ** 22                         # what word_centered is told (the kernels' |b| stay below 2^41)
        worst = max(worst, abs(w) - HALF)
    print("%s: %d lanes, worst |result| = P/2 + %.1f" % (name, len(r), worst))


def test_mulm_domain_needs_ab_below_2_76():
    """The named case behind the corrected head comment of mulm: |b a/P| < 2^51 alone does not make the product exact.  At |ab| = 2^81.4
    the constant M - q (P - 1) is not a double any more and the result with aP = a * (1 / P) is off by 2^27; inside |ab| < 2^76 the same
    near-tie construction stays exact (the class lanes above).  The kernels' largest |b| is 2^41."""
    a, b = 1482960300, 1702156248324275
    aP = F.fmul(float(a), F.PINV)
    assert abs(b * aP) < 2 ** 51 and abs(a * b) >= 1 << 80
    r = F.m_mulm(float(a), aP, float(b))
    assert (int(r) - a * b) % P == 1 << 27


def test_mulmod_bound_needs_ab_below_2_80():
    """The named case behind the corrected head comment of mulmod: exact up to 2^84, but |r| < 1.1 P only while |ab| < 2^80."""
    a, b = 4205480592310, 4374933538571
    r = F.m_mulmod(float(a), float(b))
    assert r.is_integer() and (int(r) - a * b) % P == 0 and 1 << 83 < a * b < 1 << 84 and abs(r) > 1.5 * P


def test_other_fp64_models_are_exact_and_within_their_stated_bounds():
    x = _ints(F.lanes("word_any")[0][:, 0])
    for v, w in zip(x, _ints(F.model("word_any"))):
        q, _ = F.m_word_any_parts(float(v))
        assert q == v // P and w == v % P, v                        # floor(x / P) exactly, r in [0, P)
    x = _ints(F.lanes("word_centered")[0][:, 0])
    assert _ints(F.model("word_centered")) == [v % P for v in x]
    x = _ints(F.lanes("store_elem")[0][:, 0])
    for v, w in zip(x, _ints(F.model("store_elem"))):
        r = F.m_store_elem_remainder(float(v))
        assert r.is_integer() and (int(r) - v * F.R) % P == 0 and abs(r) < HALF + 2 ** 12 and w == v * F.R % P, v
    x = F.lanes("add_scaled_pow2")[0]
    for (tot, xx, inv), w in zip(x.tolist(), _ints(F.model("add_scaled_pow2"))):
        k = int(round(-np.log2(abs(inv))))
        s = pow(2, -k, P) * (1 if inv > 0 else -1)
        assert (w - (int(tot) + int(xx) * s)) % P == 0 and abs(w) < 1 << 45, (tot, xx, inv)
    x = _ints(F.lanes("sbox7")[0][:, 0])
    for v, w in zip(x, _ints(F.model("sbox7"))):
        # each product leaves P/2 + 1 + |ab| 2^-52 with |ab| < 2^36.2 * 2^30 for the first three and 2^60 for the last: P/2 + 2^9 at most
        assert (w - pow(v, 7, P)) % P == 0 and abs(w) <= HALF + 2 ** 9, v


# ---- the host branches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.INT_OPS)
def test_host_branch_equals_the_reference(p3, name):
    x, lab = F.lanes(name)
    got, want = probe_host(p3, name, x), F.expected(name)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, [(lab[i], x[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]


def test_host_probe_refuses_what_it_cannot_run(p3):
    from plonky3_mobile_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(8, np.float64)
    ptr = C.c_void_p(buf.ctypes.data)
    for name in F.F64_OPS:
        assert lib.p3hip_field_probe_host(F.OPS[name][0], ptr, ptr, 1) == -1
        msg = p3.take_last_error()
        assert "__device__ only" in msg and "op %d" % F.OPS[name][0] in msg, msg
    for op in (0, -1, 21, 31, 44, 1 << 20):
        assert lib.p3hip_field_probe_host(op, ptr, ptr, 1) == -1 and "unknown op %d" % op in p3.take_last_error()
        assert lib.p3hip_field_probe_dev(op, ptr, ptr, 1, None) == -1 and "unknown op %d" % op in p3.take_last_error()  # before any GPU call
    assert lib.p3hip_field_probe_host(1, ptr, ptr, (1 << 22) + 1) == -1 and "2^22" in p3.take_last_error()
    assert lib.p3hip_field_probe_dev(1, ptr, ptr, (1 << 22) + 1, None) == -1 and "2^22" in p3.take_last_error()
    assert lib.p3hip_field_probe_host(1, None, ptr, 1) == -1 and "null" in p3.take_last_error()
    assert lib.p3hip_field_probe_host(1, None, None, 0) == 0 and p3.take_last_error() is None
    assert buf.tolist() == [0.0] * 8


def test_header_carries_the_op_table():
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define P3HIP_FP_(\w+) (\d+)\n", hdr)}
    want = {n.upper(): o[0] for n, o in F.OPS.items()}
    assert defs == want
    table = {int(m.group(1)): m.group(2).strip() for m in re.finditer(r"^ \*\s+(\d+)  (\S.*?)\s{2,}", hdr, flags=re.M)}
    assert sorted(table) == sorted(want.values())
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert re.search(r"int p3hip_field_probe_dev\(int op, const void \*d_in, void \*d_out, size_t n, void \*stream\);", code)
    assert re.search(r"int p3hip_field_probe_host\(int op, const void \*in, void \*out, size_t n\);", code)
    for f in ("include/p3hip.hpp", "integration/native/src/hip_front_end.rs", "integration/native/src/backend_hip.rs"):
        assert "field_probe" not in open(os.path.join(ROOT, f)).read()  # a test entry: no mirror, no shim
