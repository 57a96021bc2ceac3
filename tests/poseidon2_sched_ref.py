"""Exact models of the two fp64 SCHEDULES of Poseidon2 (csrc/poseidon2_f64.hip.h p2f::permute, one state per lane, and
csrc/poseidon2_q4.hip.h p2q::permute, one state per DPP quad), a pre-image builder, the adversarial state families built with it,
and a magnitude-bound pass over both schedules.  Pure Python: no library, no oracle; the primitives' models come from field_ref, the
round constants and the big-integer permutation from pyref.

MODELS.  One correctly rounded step per operation, in the order and grouping of the headers: mat4, the four-block column sum
((s[k] + s[k+4]) + (s[k+8] + s[k+12]) in p2f; v + v^1, then + v^2, lane by lane, in p2q), the lane sum of the internal round in each
form's own bracketing, reduce, sbox7, add_scaled_pow2, and each form's fold schedule.  A Python float addition is the device's
v_add_f64; fma goes through field_ref.fma.  Every value a model forms is asserted to be an integer below 2^53 in magnitude and is
recorded, per named SITE, as the largest |value| seen there (Peaks).

PRE-IMAGES.  Every layer of the permutation is invertible (x -> x^7 is a bijection of the field, both linear layers are
non-singular), so preimage(y, seam) is the canonical state whose S-box OUTPUTS of external round `seam` (0 .. 7; 4 .. 7 are the
final rounds, reached back through the thirteen internal rounds) are y mod P.  With y = +-(P - 1) / 2 in all sixteen elements at seam
3 the internal rounds are entered at 35 times the S-box's representative of y in every element: -+35 (P + 1) / 2 in these models (the
fourth product's quotient estimate rounds up, so sbox7 returns (P - 1) / 2 - P), the header's worst case 35 (P/2 + 1) to within 18 —
from words in [0, P) alone.
"""
import functools

import numpy as np

import field_ref as F
import pyref

P = F.P
H = (P - 1) // 2
LIMIT = 2.0 ** 53
EI, IT, EF = pyref.DEFAULT_RC
EXT_RC = [[float(v) for v in row] for row in list(EI) + list(EF)]  # d_c.ext[0..8): canonical values
INT_RC = [float(v) for v in IT]
# V of the internal diagonal as the headers write it: an integer, or +-2^-k (2^-27 = -15 mod P)
V = (-2.0, 1.0, 2.0, 0.5, 3.0, 4.0, -0.5, -3.0, -4.0, 0.00390625, 0.25, 0.125, -15.0, -0.00390625, -0.0625, 15.0)
INTEGER_LANES = (1, 2, 4, 5, 7, 8, 12, 15)  # the lanes p2f folds (lane 0 is re-entered through the S-box every round)
V_SIGN = tuple(1 if v > 0 else -1 for v in V)
assert all((int(v) if v.is_integer() else pow(int(1 / abs(v)), -1, P) * (1 if v > 0 else -1)) % P == d for v, d in zip(V, pyref._D))
SITES = ("linear layer", "S-box input", "S-box input of a lane that discards it", "lane sum before reduce", "add_scaled_pow2 operand",
         "lane before a fold", "fma lane result", "store_elem operand")


class Peaks(dict):
    """site -> largest |value| seen; rec() also asserts the value is an integer below 2^53"""

    def rec(self, site, v):
        assert v.is_integer() and abs(v) < LIMIT, (site, v)
        if abs(v) > self.get(site, 0.0):
            self[site] = abs(v)
        return v

    def text(self):
        return ", ".join("%s 2^%.2f" % (k, np.log2(self[k])) for k in SITES if self.get(k))


def reduce(x):
    return F.fma(-F.rint(F.fmul(x, F.PINV)), F.PD, x)


def mat4(pk, a, b, c, d):
    r = pk.rec
    t01, t23 = r("linear layer", a + b), r("linear layer", c + d)
    t0123 = r("linear layer", t01 + t23)
    t01123, t01233 = r("linear layer", t0123 + b), r("linear layer", t0123 + d)
    nd, nb = r("linear layer", F.fma(a, 2.0, t01233)), r("linear layer", F.fma(c, 2.0, t01123))
    na, nc = r("linear layer", t01123 + t01), r("linear layer", t01233 + t23)
    return na, nb, nc, nd


def _sbox(pk, x):
    return pk.rec("S-box output", F.m_sbox7(pk.rec("S-box input", x)))


# ---- p2f: one state per lane ------------------------------------------------------------------------------------------------------
def _f_external_linear(pk, s):
    s = [v for i in range(0, 16, 4) for v in mat4(pk, *s[i:i + 4])]
    t = [pk.rec("linear layer", pk.rec("linear layer", s[k] + s[k + 4]) + pk.rec("linear layer", s[k + 8] + s[k + 12])) for k in range(4)]
    return [pk.rec("linear layer", s[i] + t[i & 3]) for i in range(16)]


def _f_internal_round(pk, s, r):
    s = list(s)
    s[0] = _sbox(pk, s[0] + INT_RC[r])
    q = [pk.rec("lane sum before reduce", (s[k] + s[k + 1]) + (s[k + 2] + s[k + 3])) for k in range(0, 16, 4)]
    tot = reduce(pk.rec("lane sum before reduce", (q[0] + q[1]) + (q[2] + q[3])))
    pk.rec("reduced lane sum", tot)
    out = []
    for i in range(16):
        if i == 1:
            out.append(pk.rec("fma lane result", tot + s[1]))
        elif V[i].is_integer():
            out.append(pk.rec("fma lane result", F.fma(s[i], V[i], tot)))
        else:
            out.append(pk.rec("add_scaled_pow2 result", F.m_add_scaled_pow2(tot, pk.rec("add_scaled_pow2 operand", s[i]), V[i])))
    return out


def _f_fold(pk, s):
    return [reduce(pk.rec("lane before a fold", v)) if i in INTEGER_LANES else v for i, v in enumerate(s)]


def f_internal_rounds(pk, s):
    for blk in range(3):
        for r in range(4):
            s = _f_internal_round(pk, s, 4 * blk + r)
        s = _f_fold(pk, s)
    return _f_fold(pk, _f_internal_round(pk, s, 12))


# ---- p2q: one state per quad, lane q holds elements 4q .. 4q+3 -------------------------------------------------------------------------
def _quad_sum(pk, site, v):
    """v[q] of the four lanes -> what each lane ends with: v += v[q ^ 1], then v + v[q ^ 2]"""
    a = [pk.rec(site, v[q] + v[q ^ 1]) for q in range(4)]
    return [pk.rec(site, a[q] + a[q ^ 2]) for q in range(4)]


def _q_external_linear(pk, s):
    s = [v for i in range(0, 16, 4) for v in mat4(pk, *s[i:i + 4])]
    for i in range(4):
        t = _quad_sum(pk, "linear layer", [s[4 * q + i] for q in range(4)])
        for q in range(4):
            s[4 * q + i] = pk.rec("linear layer", s[4 * q + i] + t[q])
    return s


def _q_internal_round(pk, s, r):
    s = list(s)
    for q in (1, 2, 3):
        pk.rec("S-box input of a lane that discards it", s[4 * q] + INT_RC[r])  # every lane computes x^7, lane 0 alone keeps it
    s[0] = _sbox(pk, s[0] + INT_RC[r])
    part = [pk.rec("lane sum before reduce", (s[4 * q] + s[4 * q + 1]) + (s[4 * q + 2] + s[4 * q + 3])) for q in range(4)]
    tot = [reduce(v) for v in _quad_sum(pk, "lane sum before reduce", part)]
    assert len(set(tot)) == 1  # exact integers: every lane of the quad ends with the same sum
    pk.rec("reduced lane sum", tot[0])
    s = [pk.rec("add_scaled_pow2 result", F.m_add_scaled_pow2(tot[i >> 2], pk.rec("add_scaled_pow2 operand", s[i]), V[i])) for i in range(16)]
    if (r & 3) == 3 or r == 12:
        s = [reduce(pk.rec("lane before a fold", v)) for v in s]
    return s


def q_internal_rounds(pk, s):
    for r in range(13):
        s = _q_internal_round(pk, s, r)
    return s


def _permute(pk, state, ext, internal):
    s = [float(v) for v in state]
    assert all(int(a) == b for a, b in zip(s, state))
    s = ext(pk, s)
    for r in range(4):
        s = ext(pk, [_sbox(pk, s[i] + EXT_RC[r][i]) for i in range(16)])
    entry = list(s)
    s = internal(pk, s)
    for r in range(4, 8):
        s = ext(pk, [_sbox(pk, s[i] + EXT_RC[r][i]) for i in range(16)])
    for v in s:
        pk.rec("store_elem operand", v)
    return s, entry


def model_f(state, pk=None):
    """p2f::permute on integer-valued `state`: (raw doubles out, the state entering the internal rounds).  pk: a Peaks to fill."""
    return _permute(Peaks() if pk is None else pk, state, _f_external_linear, f_internal_rounds)


def model_q(state, pk=None):
    return _permute(Peaks() if pk is None else pk, state, _q_external_linear, q_internal_rounds)


def words(raw):
    """canonical values of a model's raw doubles, through the exact model of store_elem (Montgomery word -> canonical)"""
    out = [F.canon(int(F.m_store_elem(v))) for v in raw]
    assert out == [int(v) % P for v in raw]
    return out


# ---- pre-images ------------------------------------------------------------------------------------------------------------------------
def _solve_inverse(fn):
    """inverse mod P of the 16 x 16 matrix of the linear map fn, by one Gauss-Jordan solve"""
    cols = [fn([1 if i == j else 0 for i in range(16)]) for j in range(16)]
    m = [[cols[j][i] for j in range(16)] + [1 if i == k else 0 for k in range(16)] for i in range(16)]
    for c in range(16):
        piv = next(r for r in range(c, 16) if m[r][c])
        m[c], m[piv] = m[piv], m[c]
        iv = pow(m[c][c], -1, P)
        m[c] = [v * iv % P for v in m[c]]
        for r in range(16):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % P for x, y in zip(m[r], m[c])]
    return [row[16:] for row in m]


@functools.lru_cache(maxsize=None)
def _inverses():
    return _solve_inverse(pyref._ext), _solve_inverse(pyref._int)


def _apply(m, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in m]


SBOX_INV_EXP = pow(7, -1, P - 1)


def _unsbox(v):
    return pow(v % P, SBOX_INV_EXP, P)


def preimage(y, seam):
    """The canonical state (16 integers in [0, P)) whose S-box outputs of external round `seam` (0 .. 7) are y mod P."""
    assert 0 <= seam < 8 and len(y) == 16
    ext_inv, int_inv = _inverses()
    u = [int(v) % P for v in y]
    if seam >= 4:
        for j in range(seam - 4, -1, -1):  # u = the S-box outputs of final round j
            s = [(_unsbox(u[i]) - EF[j][i]) % P for i in range(16)]
            if j:
                u = _apply(ext_inv, s)
        for r in range(12, -1, -1):  # s = the state after internal round r
            s = _apply(int_inv, s)
            s[0] = (_unsbox(s[0]) - IT[r]) % P
        u = _apply(ext_inv, s)  # the S-box outputs of initial round 3
        seam = 3
    for j in range(seam, -1, -1):
        s = [(_unsbox(u[i]) - EI[j][i]) % P for i in range(16)]
        u = _apply(ext_inv, s)  # the S-box outputs of round j - 1, or (j = 0) the permutation's input
    return u


def seam_outputs(state, seam):
    """the S-box outputs of external round `seam` on `state`, in plain integers: the inverse of preimage"""
    s = pyref._ext(list(state))
    for r in range(4):
        u = [pow((s[i] + EI[r][i]) % P, 7, P) for i in range(16)]
        if r == seam:
            return u
        s = pyref._ext(u)
    for r in range(13):
        s[0] = pow((s[0] + IT[r]) % P, 7, P)
        s = pyref._int(s)
    for r in range(4):
        u = [pow((s[i] + EF[r][i]) % P, 7, P) for i in range(16)]
        if r + 4 == seam:
            return u
        s = pyref._ext(u)
    raise AssertionError(seam)


def seam7_closed_form(y):
    """the permutation's output when the S-box outputs of the last external round are y: one external linear layer"""
    return pyref._ext([int(v) % P for v in y])


# ---- the target families -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def targets():
    """(name, y): the S-box output vectors (signed integers; a pre-image takes them mod P).  'all -h' and 'all (P+1)/2' are one vector
    mod P and are both listed, as the two signed representatives an S-box may return."""
    t = [("all +h", [H] * 16), ("all -h", [-H] * 16), ("all (P+1)/2", [(P + 1) // 2] * 16),
         ("signs of V", [H * s for s in V_SIGN]), ("-signs of V", [-H * s for s in V_SIGN]),
         ("alternating", [H if i % 2 else -H for i in range(16)]),
         ("integer lanes", [H if i in INTEGER_LANES else 0 for i in range(16)])]
    for i in range(16):
        for s in (1, -1):
            t.append(("%sh on lane %d" % ("+-"[s < 0], i), [s * H if j == i else 0 for j in range(16)]))
    rng = np.random.default_rng([F.SEED, 16])
    for n in range(64):
        k = int(rng.integers(0, 4))
        t.append(("random signs %d, h - %d" % (n, k), [int(s) * (H - k) for s in rng.choice([-1, 1], size=16)]))
    return tuple((n, tuple(y)) for n, y in t)


NAMED = 7  # the first NAMED targets are the structured ones


@functools.lru_cache(maxsize=None)
def family():
    """((name, seam, y, state), ...): every target at every seam, state = preimage(y, seam) as canonical integers.  Read-only."""
    return tuple((n, seam, y, tuple(preimage(y, seam))) for seam in range(8) for n, y in targets())


def family_states():
    return np.array([f[3] for f in family()], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def family_expected():
    """pyref.poseidon2 of every family state (canonical), computed once"""
    a = np.array([pyref.poseidon2(list(f[3])) for f in family()], dtype=np.uint64)
    a.setflags(write=False)
    return a


EDGE_STATES = ([0] * 16, [P - 1] * 16, [P // 2] * 16, [P // 2 + 1] * 16)


# ---- the magnitude-bound pass ---------------------------------------------------------------------------------------------------------
# |value| bounds (integers, rounded up) pushed through both schedules from an entry bound.  Every bound is checked against 2^53 and
# every call site against the documented precondition of the primitive it calls; a precondition that does not hold is RECORDED (form,
# site, what, bound) instead of raised, so that the test can list exactly which ones a given entry contract exceeds.
HALF_UP = P // 2 + 1                 # reduce: |result| <= P/2 + eps
SBOX_OUT = P // 2 + 2 ** 9           # sbox7: |result| <= P/2 + 2^9 (include/p3hip.h, op 38)
ENTRY_CONTRACTS = {"words in [0, P) (load_elem)": P - 1, "after a reduce between absorptions": HALF_UP, "2^32": 2 ** 32, "the header's 2^33": 2 ** 33}


class BoundPass:
    def __init__(self, form):
        self.form, self.peak, self.exceeded = form, {}, []

    def see(self, site, b):
        assert b < 2 ** 53, (self.form, site, b)
        self.peak[site] = max(self.peak.get(site, 0), b)
        return b

    def need(self, site, what, ok, b):
        if not ok:
            self.exceeded.append((self.form, site, what, b))

    def mulmod_m(self, site, a, b):
        """mulmod_m(a, b, a / P): |b aP| < 2^51 and |ab| < 2^76; |result| <= P/2 + 1 + |ab| 2^-52"""
        self.need(site, "mulmod_m |b aP| < 2^51", a * b < (P << 51), a * b)
        self.need(site, "mulmod_m |ab| < 2^76", a * b < 1 << 76, a * b)
        return HALF_UP + (a * b >> 52) + 1

    def sbox7(self, x):
        self.see("S-box input", x)
        x2 = self.mulmod_m("sbox7 x * x", x, x)
        x3 = self.mulmod_m("sbox7 x * x2", x, x2)
        x4 = self.mulmod_m("sbox7 x * x3", x, x3)
        out = self.mulmod_m("sbox7 x3 * x4", x3, x4)
        assert out <= SBOX_OUT or self.exceeded, (x, out)
        return out

    def external_linear(self, b):
        self.see("linear layer", 7 * b)   # mat4: the largest row is 2 + 3 + 1 + 1
        self.see("linear layer", 28 * b)  # the four-block column sum, whatever its bracketing
        return self.see("linear layer", 35 * b)

    def asp(self, tot, x, v):
        if float(v).is_integer():
            return self.see("add_scaled_pow2 result", tot + int(abs(v)) * x)  # xt = tot + m x is an integer: fract = 0, result = xt
        self.need("add_scaled_pow2", "|x| < 2^44", x < 1 << 44, x)
        self.need("add_scaled_pow2", "|tot| < 2^40", tot < 1 << 40, tot)
        k = int(round(-np.log2(abs(v))))
        return self.see("add_scaled_pow2 result", tot + (x >> k) + 1 + P)  # xt - fract P

    def internal(self, b):
        lanes = [b] * 16
        for r in range(13):
            if self.form == "p2q":
                for q in (1, 2, 3):
                    self.see("S-box input of a lane that discards it", lanes[4 * q] + P - 1)
            lanes[0] = self.sbox7(lanes[0] + P - 1)
            self.see("lane sum before reduce", sum(lanes))
            tot = HALF_UP
            for i in range(16):
                if self.form == "p2f" and float(V[i]).is_integer():
                    lanes[i] = self.see("fma lane result", tot + int(abs(V[i])) * lanes[i])
                else:
                    self.see("add_scaled_pow2 operand", lanes[i])
                    lanes[i] = self.asp(tot, lanes[i], V[i])
            if (r & 3) == 3 or r == 12:
                for i in (range(16) if self.form == "p2q" else INTEGER_LANES):
                    self.see("lane before a fold", lanes[i])
                    lanes[i] = HALF_UP
        return max(lanes)

    def permute(self, entry):
        b = self.external_linear(entry)
        for _ in range(4):
            b = self.external_linear(self.sbox7(b + P - 1))
        b = self.internal(b)
        for _ in range(4):
            b = self.external_linear(self.sbox7(b + P - 1))
        self.see("store_elem operand", b)
        self.need("store_elem", "|v| < 2^37", b < 1 << 37, b)
        return b


def bound_pass(form, entry):
    bp = BoundPass(form)
    bp.permute(entry)
    return bp
