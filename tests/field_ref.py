"""Reference, exact fp64 model and operand classes of the field probe (include/p3hip.h, P3HIP_FP_*).  Pure Python / numpy: no oracle,
no library.

REFERENCE: plain integers mod P; a Montgomery word is x * 2^32 mod P; the extension is F[x] / (x^4 - 11) with inverses as
a^(P^4 - 2) (ext_inv_linear solves the 4 x 4 system instead: the two are compared in the host tests; neither is the library's norm
formula).  The bulk forms work on numpy uint64 arrays (every intermediate below 2^64), the scalar forms on Python integers.

EXACT MODEL of each fp64 primitive: one correctly rounded step per operation, in the order of the header
(csrc/poseidon2_f64.hip.h, csrc/ntt_narrow_f64.hip.h).  float(Fraction) is round-to-nearest-even, so fma(a, b, c) =
float(Fraction(a) * Fraction(b) + Fraction(c)) is the device's v_fma_f64 bit for bit; rint is round-half-even, fract(x) = x - floor(x).

OPERAND CLASSES: lanes(name) returns (operands, labels) for a probe op, a function of SEED alone; labels[i] is the class of lane i,
computed here in Python from the operands (never from a result of the code under test).  CLASSES[name] lists the classes a test may
ask for; tests/test_field_ref_host.py asserts that every one of them holds at least MIN_LANES lanes.  A class with fewer than
MIN_LANES distinct operand tuples lists all of them and repeats them up to MIN_LANES lanes.
"""
import functools
import math
import os
import re
from fractions import Fraction as Fr

import numpy as np

P = 0x78000001
MU = 0x88000001
NMU = (-MU) & 0xffffffff
M32 = 0xffffffff
R = 1 << 32
RINV = pow(R, -1, P)
ONE = R % P
R2 = R * R % P
W_CANON = 11
W_MONTY = 11 * R % P
assert (ONE, R2, W_MONTY, MU * P & M32) == (0x0ffffffe, 0x45dddde3, 0x37ffffe9, 1)
SEED = 20261019
MIN_LANES = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (op number, operands per lane, results per lane, fp64)
OPS = {
    "add": (1, 2, 1, False), "sub": (2, 2, 1, False), "neg": (3, 1, 1, False), "dbl": (4, 1, 1, False), "mul": (5, 2, 1, False),
    "sqr": (6, 1, 1, False), "dot2": (7, 4, 1, False), "to_monty": (8, 1, 1, False), "from_monty": (9, 1, 1, False),
    "pow7": (10, 1, 1, False), "pow": (11, 3, 1, False), "inv": (12, 1, 1, False), "two_adic_generator": (13, 1, 1, False),
    "smul": (14, 2, 1, False), "sbox7_add": (15, 2, 1, False), "ext_mul": (16, 8, 4, False), "ext_sqr": (17, 4, 4, False),
    "ext_inv": (18, 4, 4, False), "ext_pow": (19, 6, 4, False), "ext_scale": (20, 5, 4, False),
    "mulmod": (32, 2, 1, True), "mulmod_p": (33, 3, 1, True), "mulmod_p_dev": (34, 2, 1, True), "mulmod_m": (35, 3, 1, True),
    "mulmod_m_dev": (36, 2, 1, True), "add_scaled_pow2": (37, 3, 1, True), "sbox7": (38, 1, 1, True), "store_elem": (39, 1, 1, True),
    "mulm": (40, 3, 1, True), "mulm_dev": (41, 2, 1, True), "word_centered": (42, 1, 1, True), "word_any": (43, 1, 1, True),
    "add_scaled_int": (48, 3, 1, True), "sbox7_wide": (49, 1, 1, True),
}
INT_OPS = [n for n, o in OPS.items() if not o[3]]
F64_OPS = [n for n, o in OPS.items() if o[3]]


# ---------------------------------------------------------------------------------------------------------------------------------
# reference: integers
def monty(x):
    return x * R % P


def canon(m):
    return m * RINV % P


def smul_ref(a, b):
    """The signed Montgomery product as a number: t = the signed 32-bit word with t P = a b (mod 2^32); (a b - t P) / 2^32."""
    x = a * b
    t = (x & M32) * MU & M32
    if t >= 1 << 31:
        t -= R
    assert (x - t * P) % R == 0
    return (x - t * P) >> 32


def rc16_words():
    """Every round constant of csrc/poseidon2_rc16.h (Montgomery words), in file order: 64 + 13 + 64."""
    text = open(os.path.join(ROOT, "plonky3-mobile_amd", "csrc", "poseidon2_rc16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{8})u", text)]
    assert len(words) == 141 and all(w < P for w in words)
    return words


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


_P, _RINV, _R = np.uint64(P), np.uint64(RINV), np.uint64(ONE)


def v_canon(m):
    return _u64(m) % _P * _RINV % _P


def v_monty(c):
    return _u64(c) % _P * _R % _P


def v_mul(a, b):  # Montgomery product of words
    return _u64(a) * _u64(b) % _P * _RINV % _P


def v_pow_canon(c, e):  # canonical c ** e, e one Python integer
    c = _u64(c) % _P
    r = np.ones_like(c)
    while e:
        if e & 1:
            r = r * c % _P
        c = c * c % _P
        e >>= 1
    return r


def v_ext_mul_canon(a, b):  # (n, 4) canonical coefficients
    a, b = _u64(a), _u64(b)
    out = np.zeros_like(a)
    for k in range(4):
        lo = np.zeros(a.shape[0], np.uint64)
        hi = np.zeros(a.shape[0], np.uint64)
        for i in range(4):
            for j in range(4):
                if i + j == k:
                    lo = lo + a[:, i] * b[:, j] % _P
                elif i + j == k + 4:
                    hi = hi + a[:, i] * b[:, j] % _P
        out[:, k] = (lo + hi % _P * np.uint64(W_CANON)) % _P
    return out


def v_ext_pow_canon(a, e):
    a = _u64(a) % _P
    r = np.zeros_like(a)
    r[:, 0] = 1
    while e:
        if e & 1:
            r = v_ext_mul_canon(r, a)
        a = v_ext_mul_canon(a, a)
        e >>= 1
    return r


def v_ext_inv_canon(a):
    return v_ext_pow_canon(a, P ** 4 - 2)  # 0 -> 0


def ext_inv_linear(a):
    """Inverse of one canonical element by linear algebra: solve M(a) y = e0, M(a) the matrix of multiplication by a."""
    cols = []
    for j in range(4):
        e = [0, 0, 0, 0]
        e[j] = 1
        cols.append([int(v) for v in v_ext_mul_canon(np.array([a], np.uint64), np.array([e], np.uint64))[0]])
    m = [[cols[j][i] for j in range(4)] + [1 if i == 0 else 0] for i in range(4)]
    for c in range(4):
        piv = next(r for r in range(c, 4) if m[r][c])
        m[c], m[piv] = m[piv], m[c]
        iv = pow(m[c][c], -1, P)
        m[c] = [v * iv % P for v in m[c]]
        for r in range(4):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % P for x, y in zip(m[r], m[c])]
    return [m[i][4] for i in range(4)]


def reference(name, x):
    """Expected output words of an integer or extension op for operand rows x (n, k): uint32 array (n, m)."""
    x = _u64(x)
    n = x.shape[0]
    c = lambda i: x[:, i]  # noqa: E731
    if name == "add":
        r = (c(0) + c(1)) % _P
    elif name == "sub":
        r = (c(0) + _P - c(1)) % _P
    elif name == "neg":
        r = (_P - c(0)) % _P
    elif name == "dbl":
        r = c(0) * np.uint64(2) % _P
    elif name == "mul":
        r = v_mul(c(0), c(1))
    elif name == "sqr":
        r = v_mul(c(0), c(0))
    elif name == "dot2":
        r = (c(0) * c(1) % _P + c(2) * c(3) % _P) % _P * _RINV % _P
    elif name == "to_monty":
        r = v_monty(c(0))
    elif name == "from_monty":
        r = v_canon(c(0))
    elif name == "pow7":
        r = v_monty(v_pow_canon(v_canon(c(0)), 7))
    elif name == "pow":
        r = np.zeros(n, np.uint64)
        es = c(1) | (c(2) << np.uint64(32))
        for e in np.unique(es):
            sel = es == e
            r[sel] = v_monty(v_pow_canon(v_canon(c(0)[sel]), int(e)))
    elif name == "inv":
        r = v_monty(v_pow_canon(v_canon(c(0)), P - 2))
    elif name == "two_adic_generator":
        r = _u64([monty(pow(31, 15 << (27 - int(b)), P)) for b in c(0)])
    elif name == "smul":
        s = x.astype(np.uint32).view(np.int32)
        r = _u64([smul_ref(int(a), int(b)) & M32 for a, b in s])
    elif name == "sbox7_add":
        r = v_monty(v_pow_canon((v_canon(c(0)) + v_canon(c(1))) % _P, 7))
    elif name in ("ext_mul", "ext_sqr", "ext_inv", "ext_scale"):
        a = v_canon(x[:, :4])
        if name == "ext_mul":
            r = v_ext_mul_canon(a, v_canon(x[:, 4:8]))
        elif name == "ext_sqr":
            r = v_ext_mul_canon(a, a)
        elif name == "ext_inv":
            r = v_ext_inv_canon(a)
        else:
            r = a * v_canon(x[:, 4:5]) % _P
        r = v_monty(r)
    elif name == "ext_pow":
        r = np.zeros((n, 4), np.uint64)
        es = c(4) | (c(5) << np.uint64(32))
        for e in np.unique(es):
            sel = es == e
            r[sel] = v_monty(v_ext_pow_canon(v_canon(x[sel, :4]), int(e)))
    else:
        raise KeyError(name)
    return r.reshape(n, -1).astype(np.uint32)


# the device forms of mul / dot2 up to the value BEFORE the correction: r' = (x + t P) >> 32, t = lo(x) * -P^-1 mod 2^32
def v_rprime(x):
    x = _u64(x)
    t = (x & np.uint64(M32)) * np.uint64(NMU) & np.uint64(M32)
    return (x + t * _P) >> np.uint64(32), t


# ---------------------------------------------------------------------------------------------------------------------------------
# exact model of the fp64 primitives
PD = 2013265921.0
PINV = 1.0 / 2013265921.0
PM1 = 2013265920.0
NEG_PM1 = -2013265920.0
MAGIC = 6755399441055744.0
MAGIC_P = 6755399441055744.0 * 2013265921.0
assert int(MAGIC_P) == 3 * 2 ** 51 * P  # exactly representable
R_MOD_P = 268435454.0
R_MOD_P_OVER_P = 268435454.0 / 2013265921.0
FBIAS = -0.5 + 1.0 / 8589934592.0
assert Fr(FBIAS) == Fr(-1, 2) + Fr(1, 2 ** 33)


def fma(a, b, c):
    if a.is_integer() and b.is_integer() and c.is_integer():
        return float(int(a) * int(b) + int(c))  # int -> float is correctly rounded too
    return float(Fr(a) * Fr(b) + Fr(c))


def fmul(a, b):
    return fma(a, b, 0.0)


def fadd(a, b):
    return float(Fr(a) + Fr(b))


def rint(x):
    return float(round(x))  # round-half-even


def fract(x):
    f = float(Fr(x) - math.floor(x))
    return min(f, 1.0 - 2.0 ** -53)  # v_fract_f64 clamps below 1


def m_mulmod(a, b):
    h = fmul(a, b)
    lo = fma(a, b, -h)
    q = rint(fmul(h, PINV))
    r = fma(-q, PD, h)
    return fadd(r, lo)


def m_mulmod_p(a, b, aP):
    q = rint(fmul(b, aP))
    t = fma(a, b, -fmul(q, PM1))
    return fadd(t, -q)


def m_mulmod_m(a, b, aP):
    qb = fma(b, aP, MAGIC)
    c = fma(qb, NEG_PM1, MAGIC_P)
    t = fma(a, b, c)
    return fadd(t, -qb)


def m_mulm(a, aP, b):
    return m_mulmod_m(a, b, aP)


def m_add_scaled_pow2(tot, x, inv):
    xt = fma(x, inv, tot)
    return fma(fract(xt), -PD, xt)


def m_sbox7(x):
    xP = fmul(x, PINV)
    x2 = m_mulmod_m(x, x, xP)
    x3 = m_mulmod_m(x, x2, xP)
    x4 = m_mulmod_m(x, x3, xP)
    return m_mulmod_m(x3, x4, fmul(x3, PINV))


def _word_of_centered(r):
    assert r.is_integer() and abs(r) < 2 ** 31, r
    w = int(r) & M32
    return float(min(w, (w + P) & M32))


def m_store_elem(v):
    return _word_of_centered(m_mulmod_m(R_MOD_P, v, R_MOD_P_OVER_P))


def m_store_elem_remainder(v):
    return m_mulmod_m(R_MOD_P, v, R_MOD_P_OVER_P)


def m_word_centered(r):
    return _word_of_centered(r)


def m_word_any_parts(x):
    q = rint(fma(x, PINV, FBIAS))
    return q, fma(q, -PD, x)


def m_word_any(x):
    _, v = m_word_any_parts(x)
    assert v.is_integer() and 0 <= v < 2 ** 32, (x, v)  # the conversion to uint32 saturates outside
    return v


MODELS = {
    "mulmod": m_mulmod, "mulmod_p": m_mulmod_p, "mulmod_p_dev": lambda a, b: m_mulmod_p(a, b, fmul(a, PINV)),
    "mulmod_m": m_mulmod_m, "mulmod_m_dev": lambda a, b: m_mulmod_m(a, b, fmul(a, PINV)), "add_scaled_pow2": m_add_scaled_pow2,
    "sbox7": m_sbox7, "store_elem": m_store_elem, "mulm": m_mulm, "mulm_dev": lambda a, b: m_mulm(a, fmul(a, PINV), b),
    "word_centered": m_word_centered, "word_any": m_word_any, "add_scaled_int": m_add_scaled_pow2, "sbox7_wide": m_sbox7,
}


@functools.lru_cache(maxsize=None)
def model(name):
    """The exact model's result of every lane of lanes(name): float64 array (n,).  Computed once per process."""
    x, _ = lanes(name)
    f = MODELS[name]
    return np.array([f(*[float(v) for v in row]) for row in x], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# operand classes
def _edge_words():
    e = {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, ONE, R2, W_MONTY}
    for k in range(31):
        e |= {v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v < P}
    return sorted(e)


E = _edge_words()
BINADES = (31, 36, 41, 44)     # |b| in [2^e, 2^(e+1)): up to |ab| < 2^76 and |b aP| < 2^51 for |a| < P
SBOX_IN = 35 * (P // 2 + 1)    # the largest S-box input of the permutation before its round constant
NEAR_TIE = {"(P-1)/2": (P - 1) // 2, "(P+1)/2": (P + 1) // 2, "-(P-1)/2": -((P - 1) // 2), "(P-3)/2": (P - 3) // 2,
            "(P+3)/2": (P + 3) // 2}
ASP_FORMS = ((1, 1), (1, -1), (8, 1), (2, 1), (3, 1), (8, -1), (4, -1))  # (K, sign of inv) of internal_rounds, lanes 3 6 9 10 11 13 14
ASI_MULTIPLIERS = (-2, 1, 2, 3, 4, -3, -4, -15, 15)  # the integer entries of V: p2q::permute passes them through add_scaled_pow2
# a x15 lane three rounds after the internal rounds are entered at b = 35 (P/2 + 2^9), every lane sum at t = P/2 + 1: 15^3 b + (15^2 + 15 + 1) t
ASI_X = 15 ** 3 * 35 * (P // 2 + 2 ** 9) + 241 * (P // 2 + 1)
ASI_TOT = P // 2 + 1                   # reduce's |result|
SBOX_WIDE_IN = 35 * (P - 1) + P        # the first external round on a state of words in [0, P), + its round constant
EXPONENTS = (0, 1, 2, P - 2, P - 1, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1)


def _product_classes():
    out = []
    for kind in ("canonical", "centred"):
        for e in BINADES:
            out.append("%s a, |b| in 2^%d, uniform" % (kind, e))
            out += ["%s a, |b| in 2^%d, ab = %s (mod P)" % (kind, e, t) for t in NEAR_TIE]
    return out + ["a = 0", "b = 0", "b = kP"]


_PAIR = ["grid E x E", "uniform"]
_ONE = ["E", "uniform"]
_EXT_STRUCT = ["base field", "c1 = c3 = 0", "c0 = c2 = 0", "norm d = 0", "norm c = 0", "zero"]
CLASSES = {
    "add": _PAIR, "sub": _PAIR, "neg": _ONE, "dbl": _ONE, "sqr": _ONE, "to_monty": _ONE, "pow7": _ONE,
    "from_monty": _ONE + ["words >= P"],
    "mul": _PAIR + ["r' = P-2", "r' = P-1", "r' = P+1", "r' = P+2", "largest r' of the search", "lo(ab) = 0 (t = 0)", "t = 2^32-1",
                    "ab = 0 (mod P)"],
    "dot2": ["all P-1", "x >= 2^62", "lo(x) = 0", "cancelling (r' = P)", "r' = P-2", "r' = P-1", "r' = P+1", "r' = P+2",
             "largest r' of the search", "uniform"],
    "smul": ["edges {0, +-1, +-(P-1)}^2", "lo(ab) = 0", "lo(ab) = 0x80000000", "lo(ab) = 0xffffffff", "uniform"],
    "sbox7_add": ["s + rc - P = %s" % t for t in ("-P", "-P+1", "-1", "0", "1", "P-2")] + ["rc16 x E", "uniform"],
    "pow": ["e = %d" % e for e in EXPONENTS] + ["uniform e"],
    "inv": _ONE + ["zero"],
    "two_adic_generator": ["bits 0..27"],
    "ext_mul": ["grid 625 x 625", "uniform"],
    "ext_sqr": ["grid 625", "uniform"],
    "ext_inv": ["grid 625", "uniform"] + _EXT_STRUCT,
    "ext_pow": ["e = %d" % e for e in EXPONENTS] + ["uniform e"],
    "ext_scale": ["grid 625 x E5", "uniform"],
    "mulmod": _product_classes(), "mulmod_p": _product_classes(), "mulmod_p_dev": _product_classes(),
    "mulmod_m": _product_classes() + ["both up to 35 (P/2 + 1)"], "mulmod_m_dev": _product_classes() + ["both up to 35 (P/2 + 1)"],
    "mulm": _product_classes(), "mulm_dev": _product_classes(),
    "add_scaled_pow2": ["K = %d, inv %s 0" % (k, "<>"[s > 0]) for k, s in ASP_FORMS],
    "sbox7": ["edges", "canonical", "uniform up to 35 (P/2 + 1) + P"],
    "store_elem": ["edges", "uniform"] + ["v 2^32 = %s (mod P), v %s 0" % (t, s) for t in NEAR_TIE for s in "<>"],
    "word_centered": ["edges", "uniform"],
    "word_any": ["%s, k %s 0" % (o, s) for o in ("kP", "kP+1", "kP-1", "kP+(P-1)") for s in ("<", ">=")],
    "add_scaled_int": ["m = %d" % m for m in ASI_MULTIPLIERS],
    "sbox7_wide": ["edges", "above 35 (P/2 + 1) + P", "uniform up to 35 (P - 1) + P"],
}
assert sorted(CLASSES) == sorted(OPS)


def _rng(name):
    return np.random.default_rng([SEED, OPS[name][0]])


def _pad(rows, n=MIN_LANES):
    rows = list(rows)
    assert rows
    return [rows[i % len(rows)] for i in range(max(n, len(rows)))]


class _Acc:
    def __init__(self):
        self.rows, self.labels = [], []

    def add(self, label, rows, pad=True):
        rows = _pad(rows) if pad else list(rows)
        self.rows += [tuple(r) if isinstance(r, (tuple, list, np.ndarray)) else (r,) for r in rows]
        self.labels += [label] * len(rows)

    def done(self, dtype):
        return np.array(self.rows, dtype=dtype), np.array(self.labels)


def _uniform_words(rng, n, k):
    return rng.integers(0, P, size=(n, k), dtype=np.uint64)


GRID5 = (0, ONE, P - 1, (P - 1) // 2, (P + 1) // 2)


def _grid625():
    return np.array([(a, b, c, d) for a in GRID5 for b in GRID5 for c in GRID5 for d in GRID5], dtype=np.uint64)


def _search(label_of, make, want, tries=4000):
    """Draw candidate batches from make() until every label in `want` has MIN_LANES rows (label_of: batch -> array of labels or '')."""
    got = {w: [] for w in want}
    for _ in range(tries):
        batch = make()
        lab = label_of(batch)
        for w in want:
            if len(got[w]) < MIN_LANES:
                got[w] += [tuple(int(v) for v in r) for r in batch[lab == w]][:MIN_LANES - len(got[w])]
        if all(len(v) >= MIN_LANES for v in got.values()):
            return got
    raise AssertionError("operand search left a class short: %r" % {w: len(v) for w, v in got.items()})


def _near_p_label(rp):
    lab = np.full(rp.shape, "", dtype=object)
    for d, t in ((-2, "r' = P-2"), (-1, "r' = P-1"), (1, "r' = P+1"), (2, "r' = P+2")):
        lab[rp == np.uint64(P + d)] = t
    return lab


def _inv_mod_2_32(a):
    return pow(int(a), -1, R)


def _lanes_mul(rng):
    acc = _Acc()
    acc.add("grid E x E", [(a, b) for a in E for b in E])
    acc.add("uniform", _uniform_words(rng, 4096, 2))
    # r' in {rho, rho + P} for b = rho 2^32 / a: scan a until both sides of P, within 2 of it, have their lanes
    def make():
        a = rng.integers(1, P, size=4096, dtype=np.uint64)
        rho = rng.choice(np.array([P - 2, P - 1, 1, 2], dtype=np.uint64), size=4096)
        b = np.array([int(r) * R % P * pow(int(x), -1, P) % P for r, x in zip(rho, a)], dtype=np.uint64)
        return np.stack([a, b], axis=1)
    near = _search(lambda ab: _near_p_label(v_rprime(ab[:, 0] * ab[:, 1])[0]), make, ["r' = P-2", "r' = P-1", "r' = P+1", "r' = P+2"])
    for k, v in near.items():
        acc.add(k, v)
    cand = P - 1 - rng.integers(0, 1 << 12, size=(1 << 16, 2)).astype(np.uint64)
    rp = v_rprime(cand[:, 0] * cand[:, 1])[0]
    acc.add("largest r' of the search", cand[np.argsort(rp)[-MIN_LANES:]])
    hw = rng.integers(1, P >> 16, size=(MIN_LANES, 2), dtype=np.uint64) << np.uint64(16)
    acc.add("lo(ab) = 0 (t = 0)", hw)
    rows = []
    while len(rows) < MIN_LANES:  # t = 2^32 - 1 exactly when lo(ab) = P: b = P / a (mod 2^32), kept when it is a field word
        a = int(rng.integers(0, P >> 1)) * 2 + 1
        b = P * _inv_mod_2_32(a) % R
        if b < P:
            rows.append((a, b))
    acc.add("t = 2^32-1", rows)
    acc.add("ab = 0 (mod P)", [(0, e) for e in E] + [(e, 0) for e in E])
    return acc.done(np.uint32)


def _lanes_dot2(rng):
    acc = _Acc()
    acc.add("all P-1", [(P - 1,) * 4])
    big = P - 1 - rng.integers(0, P // 64, size=(MIN_LANES, 4)).astype(np.uint64)
    assert np.all(big[:, 0] * big[:, 1] + big[:, 2] * big[:, 3] >= np.uint64(1 << 62))
    acc.add("x >= 2^62", big)

    def solve_b1(q, target_of, modulus):
        rows = []
        for a0, b0, a1 in q:
            a0, b0, a1 = int(a0), int(b0), int(a1)
            rows.append((a0, b0, a1, (target_of() - a0 * b0) * pow(a1, -1, modulus) % modulus))
        return np.array(rows, dtype=np.uint64)

    def odd_triples(n):
        q = rng.integers(1, P, size=(n, 3), dtype=np.uint64)
        q[:, 2] |= np.uint64(1)
        return q
    lo0 = _search(lambda r: np.where((r[:, 3] < _P) & (r[:, 3] > 0), "lo(x) = 0", ""), lambda: solve_b1(odd_triples(512), lambda: 0, R),
                  ["lo(x) = 0"])
    acc.add("lo(x) = 0", lo0["lo(x) = 0"])
    canc = solve_b1(rng.integers(1, P, size=(1024, 3), dtype=np.uint64), lambda: 0, P)  # a1 b1 = -a0 b0 (mod P), x = a multiple of P > 0
    acc.add("cancelling (r' = P)", canc)
    rhos = [P - 2, P - 1, 1, 2]
    near = _search(lambda r: _near_p_label(v_rprime(r[:, 0] * r[:, 1] + r[:, 2] * r[:, 3])[0]),
                   lambda: solve_b1(rng.integers(1, P, size=(1024, 3), dtype=np.uint64), lambda: rhos[int(rng.integers(0, 4))] * R, P),
                   ["r' = P-2", "r' = P-1", "r' = P+1", "r' = P+2"])
    for k, v in near.items():
        acc.add(k, v)
    cand = P - 1 - rng.integers(0, 1 << 12, size=(1 << 16, 4)).astype(np.uint64)
    rp = v_rprime(cand[:, 0] * cand[:, 1] + cand[:, 2] * cand[:, 3])[0]
    acc.add("largest r' of the search", cand[np.argsort(rp)[-MIN_LANES:]])
    x, lab = acc.done(np.uint64)
    u = _uniform_words(rng, 1 << 18, 4)
    return np.concatenate([x, u]).astype(np.uint32), np.concatenate([lab, np.full(1 << 18, "uniform")])


def _signed_rows(rows):
    return [(a & M32, b & M32) for a, b in rows]


def _lanes_smul(rng):
    acc = _Acc()
    ed = (0, 1, -1, P - 1, -(P - 1))
    acc.add("edges {0, +-1, +-(P-1)}^2", _signed_rows([(a, b) for a in ed for b in ed]))
    sgn = lambda n: rng.choice(np.array([-1, 1]), size=n)  # noqa: E731
    u = rng.integers(0, P >> 17, size=(MIN_LANES, 2)) * 2 + 1  # odd, and (u << 16) < P
    a = (u[:, 0] << 16) * sgn(len(u))
    acc.add("lo(ab) = 0", _signed_rows(zip(a.tolist(), ((u[:, 1] << 16) * sgn(len(u))).tolist())))
    acc.add("lo(ab) = 0x80000000", _signed_rows(zip(((u[:, 0] << 15) * sgn(len(u))).tolist(), ((u[:, 1] << 16) * sgn(len(u))).tolist())))
    rows = []
    while len(rows) < MIN_LANES:
        a = (int(rng.integers(0, P >> 1)) * 2 + 1) * int(rng.choice([-1, 1]))
        b = -_inv_mod_2_32(a % R) % R
        if b >= 1 << 31:
            b -= R
        if abs(b) < P:
            rows.append((a, b))
    acc.add("lo(ab) = 0xffffffff", _signed_rows(rows))
    acc.add("uniform", _signed_rows(rng.integers(-(P - 1), P, size=(4096, 2)).tolist()))
    x, lab = acc.done(np.uint32)
    # the labels, recomputed from the operands
    s = x.view(np.int32).astype(np.int64)
    lo = (s[:, 0] * s[:, 1]) & M32
    for t, v in (("lo(ab) = 0", 0), ("lo(ab) = 0x80000000", 1 << 31), ("lo(ab) = 0xffffffff", M32)):
        assert np.all(lo[lab == t] == v), t
    return x, lab


def _lanes_sbox7_add(rng):
    acc = _Acc()
    for t, v in (("-P", -P), ("-P+1", -P + 1), ("-1", -1), ("0", 0), ("1", 1), ("P-2", P - 2)):
        tot = v + P  # s + rc
        lo, hi = max(0, tot - (P - 1)), min(P - 1, tot)
        ss = sorted({lo, hi, (lo + hi) // 2} | {int(s) for s in rng.integers(lo, hi + 1, size=MIN_LANES)})
        acc.add("s + rc - P = " + t, [(s, tot - s) for s in ss])
    acc.add("rc16 x E", [(s, rc) for rc in rc16_words() for s in E])
    acc.add("uniform", _uniform_words(rng, 4096, 2))
    return acc.done(np.uint32)


def _exp_rows(rng, bases, width):
    """bases: (n, width) words; rows (base.., e_lo, e_hi) for every pinned exponent over `bases`, then uniform 64-bit exponents"""
    acc = _Acc()
    for e in EXPONENTS:
        acc.add("e = %d" % e, [tuple(b) + (e & M32, e >> 32) for b in bases.tolist()])
    es = rng.integers(0, 1 << 64, size=len(bases), dtype=np.uint64)
    acc.add("uniform e", [tuple(b) + (int(e) & M32, int(e) >> 32) for b, e in zip(bases.tolist(), es)])
    return acc.done(np.uint32)


def _ext_struct(rng):
    """(label, canonical rows) of the structural classes of the extension inverse"""
    n = MIN_LANES
    u = lambda: rng.integers(1, P, size=n, dtype=np.uint64)  # noqa: E731
    z = np.zeros(n, np.uint64)
    a1, a2, a3, a0 = u(), u(), u(), u()
    i2 = pow(2, -1, P)
    d0 = [(int(x1) ** 2 + 11 * int(x3) ** 2) * i2 * pow(int(x2), -1, P) % P for x1, x2, x3 in zip(a1, a2, a3)]   # 2 a0 a2 = a1^2 + 11 a3^2
    c0 = [(int(x0) ** 2 + 11 * int(x2) ** 2) * pow(22 * int(x3), -1, P) % P for x0, x2, x3 in zip(a0, a2, a3)]  # 22 a1 a3 = a0^2 + 11 a2^2
    return [("base field", np.stack([a0, z, z, z], 1)), ("c1 = c3 = 0", np.stack([a0, z, a2, z], 1)), ("c0 = c2 = 0", np.stack([z, a1, z, a3], 1)),
            ("norm d = 0", np.stack([_u64(d0), a1, a2, a3], 1)), ("norm c = 0", np.stack([a0, _u64(c0), a2, a3], 1)),
            ("zero", np.zeros((1, 4), np.uint64))]


def ext_norm_canon(a):
    """(c, d) of a * conj(a) = c + d x^2, canonical: c = a0^2 + 11 a2^2 - 22 a1 a3, d = 2 a0 a2 - a1^2 - 11 a3^2"""
    a0, a1, a2, a3 = (int(v) for v in a)
    return (a0 * a0 + 11 * a2 * a2 - 22 * a1 * a3) % P, (2 * a0 * a2 - a1 * a1 - 11 * a3 * a3) % P


def _product_rows(rng, name):
    """(a, b) integer pairs and labels of the fp64 products"""
    acc = _Acc()
    per = 512
    half = P // 2 + 2

    def draw_a(kind):
        while True:
            a = int(rng.integers(0, P)) if kind == "canonical" else int(rng.integers(-half, half + 1))
            if a % P:
                return a

    def in_binade(e, sign):
        m = int(rng.integers(1 << e, 1 << (e + 1)))
        return sign * m

    for kind in ("canonical", "centred"):
        for e in BINADES:
            rows = [(draw_a(kind), in_binade(e, 1 if i & 1 else -1)) for i in range(per)]
            acc.add("%s a, |b| in 2^%d, uniform" % (kind, e), rows)
            for t, rho in NEAR_TIE.items():
                rows = []
                for i in range(per):
                    a = draw_a(kind)
                    b0 = rho * pow(a % P, -1, P) % P
                    lo, hi = ((1 << e), (1 << (e + 1)) - 1) if i & 1 else (-(1 << (e + 1)) + 1, -(1 << e))
                    kmin, kmax = -((b0 - lo) // P), (hi - b0) // P  # lo <= b0 + k P <= hi
                    assert kmin <= kmax
                    rows.append((a, b0 + int(rng.integers(kmin, kmax + 1)) * P))
                acc.add("%s a, |b| in 2^%d, ab = %s (mod P)" % (kind, e, t), rows)
    acc.add("a = 0", [(0, in_binade(e, s)) for e in BINADES for s in (-1, 1) for _ in range(8)])
    acc.add("b = 0", [(draw_a(k), 0) for k in ("canonical", "centred") for _ in range(32)])
    acc.add("b = kP", [(draw_a(k), s * int(rng.integers(1, 1 << 14)) * P) for k in ("canonical", "centred") for s in (-1, 1) for _ in range(16)])
    if name.startswith("mulmod_m"):
        acc.add("both up to 35 (P/2 + 1)", [(s * SBOX_IN, t * SBOX_IN) for s in (-1, 1) for t in (-1, 1)] +
                rng.integers(-SBOX_IN, SBOX_IN + 1, size=(252, 2)).tolist(), pad=False)
    return acc.rows, np.array(acc.labels)


def _lanes_products(rng, name):
    rows, lab = _product_rows(rng, name)
    a = np.array([r[0] for r in rows], dtype=np.float64)
    b = np.array([r[1] for r in rows], dtype=np.float64)
    assert all(int(x) == r[0] and int(y) == r[1] for x, y, r in zip(a, b, rows))  # exactly representable
    if name in ("mulmod", "mulmod_p_dev", "mulmod_m_dev", "mulm_dev"):
        return np.stack([a, b], 1), lab
    aP = a / PD  # the host's division, as the twiddle tables form a / P (context.hip)
    return (np.stack([a, aP, b], 1) if name == "mulm" else np.stack([a, b, aP], 1)), lab


def _lanes_add_scaled_pow2(rng):
    acc = _Acc()
    for k, s in ASP_FORMS:
        rows = []
        for res in range(256):
            for sx in (-1, 1):
                for st in (-1, 1):
                    x = (int(rng.integers(1 << 43, 1 << 44)) >> k << k) + res % (1 << k)
                    tot = int(rng.integers(1 << 39, 1 << 40))
                    rows.append((float(st * tot), float(sx * x), s * 2.0 ** -k))
        acc.add("K = %d, inv %s 0" % (k, "<>"[s > 0]), rows)
    return acc.done(np.float64)


def _lanes_sbox7(rng):
    acc = _Acc()
    top = SBOX_IN + P
    acc.add("edges", [0, 1, -1, P - 1, P, P + 1, -P, (P - 1) // 2, (P + 1) // 2, -(P - 1) // 2, top, -top, top - 1, 1 - top, SBOX_IN, -SBOX_IN])
    acc.add("canonical", rng.integers(0, P, size=512).tolist())
    acc.add("uniform up to 35 (P/2 + 1) + P", rng.integers(-top, top + 1, size=1024).tolist())
    return acc.done(np.float64)


def _lanes_add_scaled_int(rng):
    acc = _Acc()
    for m in ASI_MULTIPLIERS:
        rows = [(float(st * t), float(sx * x), float(m)) for t in (ASI_TOT, 0) for x in (ASI_X, 15 ** 3 * SBOX_IN, 0) for sx in (-1, 1) for st in (-1, 1)]
        for i in range(512):  # the top binade of |x| at the largest |tot|, every sign pattern; then both uniform
            x = int(rng.integers(ASI_X >> 1, ASI_X + 1)) if i < 256 else int(rng.integers(0, ASI_X + 1))
            t = ASI_TOT - int(rng.integers(0, 4)) if i < 256 else int(rng.integers(0, ASI_TOT + 1))
            rows.append((float((1, -1)[i & 1] * t), float((1, -1)[i >> 1 & 1] * x), float(m)))
        acc.add("m = %d" % m, rows)
    return acc.done(np.float64)


def _lanes_sbox7_wide(rng):
    acc = _Acc()
    top, old = SBOX_WIDE_IN, SBOX_IN + P
    acc.add("edges", [top, -top, top - 1, 1 - top, 35 * (P - 1), -35 * (P - 1), old + 1, -old - 1, 35 * ((P - 1) // 2) + P - 1, 1 << 36, -(1 << 36)])
    acc.add("above 35 (P/2 + 1) + P", [int(v) * (1, -1)[i & 1] for i, v in enumerate(rng.integers(old + 1, top + 1, size=1024))])
    acc.add("uniform up to 35 (P - 1) + P", rng.integers(-top, top + 1, size=1024).tolist())
    return acc.done(np.float64)


def _lanes_store_elem(rng):
    acc = _Acc()
    top = (1 << 37) - 1
    acc.add("edges", [0, 1, -1, top, -top, P, -P, P - 1, 1 - P, (P - 1) // 2, -(P - 1) // 2])
    acc.add("uniform", rng.integers(-top, top + 1, size=1024).tolist())
    rinv = pow(ONE, -1, P)
    for t, rho in NEAR_TIE.items():
        v0 = rho * rinv % P
        kmax = (top - v0) // P
        acc.add("v 2^32 = %s (mod P), v > 0" % t, [v0 + k * P for k in range(0, kmax + 1)])
        acc.add("v 2^32 = %s (mod P), v < 0" % t, [v0 - k * P for k in range(1, kmax + 1)])
    return acc.done(np.float64)


def _lanes_word_centered(rng):
    acc = _Acc()
    top = (P - 1) // 2 + (1 << 22)
    acc.add("edges", [0, 1, -1, (P - 1) // 2, -(P - 1) // 2, (P + 1) // 2, -(P + 1) // 2, top, -top])
    acc.add("uniform", rng.integers(-top, top + 1, size=1024).tolist())
    return acc.done(np.float64)


def _lanes_word_any(rng):
    acc = _Acc()
    kmax = ((1 << 43) - P) // P  # 4368: kmax P + (P - 1) < 2^43 < (kmax + 2) P, and -(kmax + 1) P - 1 > -2^43
    for o, d in (("kP", 0), ("kP+1", 1), ("kP-1", -1), ("kP+(P-1)", P - 1)):
        acc.add("%s, k < 0" % o, [k * P + d for k in range(-kmax - 1, 0)])
        acc.add("%s, k >= 0" % o, [k * P + d for k in range(0, kmax + 1)])
    return acc.done(np.float64)


@functools.lru_cache(maxsize=None)
def lanes(name):
    """(operands, labels): operands (n, k) uint32 or float64, labels (n,) strings.  A function of SEED and the op alone; cached."""
    rng = _rng(name)
    k = OPS[name][1]
    if name == "mul":
        out = _lanes_mul(rng)
    elif name == "dot2":
        out = _lanes_dot2(rng)
    elif name == "smul":
        out = _lanes_smul(rng)
    elif name == "sbox7_add":
        out = _lanes_sbox7_add(rng)
    elif name in ("add", "sub"):
        acc = _Acc()
        acc.add("grid E x E", [(a, b) for a in E for b in E])
        acc.add("uniform", _uniform_words(rng, 4096, 2))
        out = acc.done(np.uint32)
    elif name in ("neg", "dbl", "sqr", "to_monty", "pow7", "from_monty", "inv"):
        acc = _Acc()
        acc.add("E", E)
        acc.add("uniform", _uniform_words(rng, 4096, 1))
        if name == "from_monty":
            acc.add("words >= P", [P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 1 << 31, M32 - 1, M32] + rng.integers(P, R, size=248).tolist())
        if name == "inv":
            acc.add("zero", [0])
        out = acc.done(np.uint32)
    elif name == "pow":
        bases = np.concatenate([np.array([[0], [ONE], [P - 1]], np.uint64), _uniform_words(rng, 61, 1)])
        out = _exp_rows(rng, bases, 1)
    elif name == "two_adic_generator":
        acc = _Acc()
        acc.add("bits 0..27", list(range(28)))
        out = acc.done(np.uint32)
    elif name == "ext_mul":
        g = _grid625()
        u = _uniform_words(rng, 1 << 14, 8)
        x = np.concatenate([np.concatenate([np.repeat(g, 625, axis=0), np.tile(g, (625, 1))], axis=1), u])
        out = x.astype(np.uint32), np.concatenate([np.full(625 * 625, "grid 625 x 625"), np.full(1 << 14, "uniform")])
    elif name == "ext_sqr":
        out = (np.concatenate([_grid625(), _uniform_words(rng, 1 << 14, 4)]).astype(np.uint32),
               np.concatenate([np.full(625, "grid 625"), np.full(1 << 14, "uniform")]))
    elif name == "ext_inv":
        acc = _Acc()
        acc.add("grid 625", _grid625())
        acc.add("uniform", _uniform_words(rng, 1 << 16, 4))
        for t, rows in _ext_struct(rng):
            acc.add(t, v_monty(rows))
        out = acc.done(np.uint32)
    elif name == "ext_pow":
        bases = np.concatenate([np.array([[0, 0, 0, 0], [ONE, 0, 0, 0], [P - 1] * 4, [P - 1, 0, 0, 0], [0, ONE, 0, 0]], np.uint64),
                                _uniform_words(rng, 59, 4)])
        out = _exp_rows(rng, bases, 4)
    elif name == "ext_scale":
        acc = _Acc()
        acc.add("grid 625 x E5", [tuple(g) + (s,) for g in _grid625().tolist() for s in GRID5])
        acc.add("uniform", _uniform_words(rng, 4096, 5))
        out = acc.done(np.uint32)
    elif name in ("mulmod", "mulmod_p", "mulmod_p_dev", "mulmod_m", "mulmod_m_dev", "mulm", "mulm_dev"):
        out = _lanes_products(rng, name)
    elif name == "add_scaled_pow2":
        out = _lanes_add_scaled_pow2(rng)
    elif name == "sbox7":
        out = _lanes_sbox7(rng)
    elif name == "store_elem":
        out = _lanes_store_elem(rng)
    elif name == "word_centered":
        out = _lanes_word_centered(rng)
    elif name == "word_any":
        out = _lanes_word_any(rng)
    elif name == "add_scaled_int":
        out = _lanes_add_scaled_int(rng)
    elif name == "sbox7_wide":
        out = _lanes_sbox7_wide(rng)
    else:
        raise KeyError(name)
    x, lab = out
    x = np.ascontiguousarray(x.reshape(len(lab), k))
    assert x.dtype == (np.float64 if OPS[name][3] else np.uint32) and len(x) <= 1 << 20
    x.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def expected(name):
    """What the probe must return for lanes(name): reference words (n, m) uint32, or the exact model's doubles (n, 1).  Read-only."""
    r = model(name).reshape(-1, 1) if OPS[name][3] else reference(name, lanes(name)[0])
    r.setflags(write=False)
    return r


def class_id(cls):
    """a pytest id of a class label that selects on a command line"""
    for a, b in ((">=", "ge"), ("<", "lt"), (">", "gt"), ("=", "eq"), ("+-", "pm"), ("+", "plus"), ("-", "minus")):
        cls = cls.replace(a, b)
    return re.sub(r"[^A-Za-z0-9]+", "_", cls).strip("_")


def product_operands(name):
    """(a, b, aP) columns of an fp64 product's lanes, whatever the op's operand order (aP None when formed on the device)."""
    x, _ = lanes(name)
    if x.shape[1] == 2:
        return x[:, 0], x[:, 1], None
    return (x[:, 0], x[:, 2], x[:, 1]) if name == "mulm" else (x[:, 0], x[:, 1], x[:, 2])
