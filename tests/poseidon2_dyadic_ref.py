"""Exact model of the thirteen internal rounds of csrc/poseidon2_f64.hip.h as p2f::internal_rounds runs them now: the seven lanes
whose diagonal entry is +-2^-k are carried as DYADIC FRACTIONS (an integer over 2^F) for several rounds at one fma per round, and
every lane is folded on a compile-time schedule of its own.  Pure Python: the primitives' models come from field_ref, the constants,
the external layers and the pre-image builder from poseidon2_sched_ref.  poseidon2_sched_ref.model_f remains the model of the
PREVIOUS schedule (add_scaled_pow2 on every fractional lane in every round, all eight integer lanes folded after rounds 3, 7, 11 and
12); nothing on the device runs it any more, the quad form p2q keeps its own schedule (model_q).

One correctly rounded step per operation (field_ref.fma / fmul / rint / fract / m_sbox7; a Python float addition is the device's
v_add_f64), in the order and bracketing of the header.  Every step outside the S-box is compared with the same step in rational
arithmetic: the model asserts that NOTHING rounds.  A value congruent to n / 2^F means n * (2^F)^-1 mod P; residue() returns it.

LEDGER.  frac[i] is an upper bound of lane i's fractional bits: + k per round, 0 after a fold; every dyadic value is asserted to be
an integer over 2^frac, and frac <= BUDGET at every sum.  PEAKS per site: "dyadic partial sum", "integer partial sum", "lane before
a fold", "exit" (and "reduced lane sum").  OPS counts the operations outside the S-box (the S-box and the addition of its round
constant are what they were): OPS_PER_PERMUTATION is what the header and profiles/hash_instruction_floor_dyadic.txt state.
"""
import functools
from fractions import Fraction as Fr

import numpy as np

import field_ref as F
import poseidon2_sched_ref as S

P = F.P
V = S.V
INT_RC = S.INT_RC
ROUNDS = 13
BUDGET = 16                                              # fractional bits a lane may hold beside its magnitude
DYADIC_K = {3: 1, 6: 1, 9: 8, 10: 2, 11: 3, 13: 8, 14: 4}   # lane -> k of its multiplier +-2^-k
DYADIC_LANES = tuple(sorted(DYADIC_K))
SUM_INTEGER_LANES = (0, 1, 2, 4, 5, 7, 8, 12, 15)          # the lanes of the integer partial sum (lane 0 is the S-box output)
# integer-multiplier lane -> the rounds after which it is folded (reduce): each by its own growth, x1 / x2 once, x3 / x4 twice, x15
# three times
INTEGER_FOLDS = {1: (12,), 2: (12,), 4: (6, 12), 5: (6, 12), 7: (6, 12), 8: (6, 12), 12: (3, 7, 12), 15: (3, 7, 12)}
assert sorted(INTEGER_FOLDS) == sorted(S.INTEGER_LANES) and all(not V[i].is_integer() and abs(V[i]) == 2.0 ** -k for i, k in DYADIC_K.items())


def dyadic_folds(k, budget=BUDGET):
    """the rounds after which a 2^-k lane is folded: whenever one more round would pass the budget, and after the last"""
    out, f = [], 0
    for r in range(ROUNDS):
        f += k
        if f + k > budget or r == ROUNDS - 1:
            out.append(r)
            f = 0
    return tuple(out)


DYADIC_FOLDS = {i: dyadic_folds(k) for i, k in DYADIC_K.items()}
# per round: 8 + 6 additions, fold_dyadic (2), 1 addition, reduce (3), 16 lane updates; a dyadic fold is 2 operations, a reduce 3
OPS_PER_ROUND = 8 + 6 + 2 + 1 + 3 + 16
OPS_PER_PERMUTATION = ROUNDS * OPS_PER_ROUND + 2 * sum(len(v) for v in DYADIC_FOLDS.values()) + 3 * sum(len(v) for v in INTEGER_FOLDS.values())
OPS_PREVIOUS = ROUNDS * 48 + 4 * 8 * 3                    # add_scaled_pow2 on seven lanes per round, eight reduces after rounds 3, 7, 11, 12
SITES = ("dyadic partial sum", "integer partial sum", "reduced lane sum", "lane before a fold", "exit")


class Peaks(S.Peaks):
    """poseidon2_sched_ref.Peaks with a record for dyadic values: recd() asserts v is an integer over 2^bits, below 2^53 / 2^bits"""

    def recd(self, site, v, bits):
        assert (Fr(v) * (1 << bits)).denominator == 1 and abs(v) * 2.0 ** bits < S.LIMIT, (site, v, bits)
        if abs(v) > self.get(site, 0.0):
            self[site] = abs(v)
        return v

    def text(self):
        return ", ".join("%s 2^%.2f" % (k, np.log2(self[k])) for k in SITES if self.get(k))


class Run:
    """what one pass of the model accumulates: peaks, the operation count, the largest ledger entry at a sum"""

    def __init__(self, pk=None, budget=BUDGET):
        self.pk, self.ops, self.budget, self.ledger_peak = (Peaks() if pk is None else pk), 0, budget, 0
        self.seen = {}  # ("sum", None, round) / ("lane", lane, round) -> (the double entering that fold_dyadic, its ledger bits), last pass

    def add(self, a, b):
        self.ops += 1
        r = a + b
        assert Fr(r) == Fr(a) + Fr(b), ("add rounds", a, b)
        return r

    def fma(self, a, b, c):
        self.ops += 1
        r = F.fma(a, b, c)
        assert Fr(r) == Fr(a) * Fr(b) + Fr(c), ("fma rounds", a, b, c)
        return r

    def fold_dyadic(self, x):
        """x - fract(x) P: the integer congruent to the dyadic fraction x"""
        self.ops += 1
        fr = F.fract(x)
        assert Fr(fr) == Fr(x) - (Fr(x).numerator // Fr(x).denominator), ("fract rounds", x)
        r = self.fma(-fr, F.PD, x)
        assert r.is_integer(), (x, r)
        return r

    def reduce(self, x):
        """the one step allowed to round is the quotient estimate x * (1 / P); the fma that follows is exact"""
        self.ops += 2
        q = F.rint(F.fmul(x, F.PINV))
        r = self.fma(-q, F.PD, x)
        assert abs(r) <= P / 2 + 1, (x, r)
        return r


def residue(v):
    """the field element of a dyadic value n / 2^F"""
    f = Fr(v)
    return f.numerator * pow(f.denominator, -1, P) % P


def internal_round(run, s, frac, r):
    """one round on doubles s with ledger frac; returns (s, frac) after the round's folds"""
    pk = run.pk
    s = list(s)
    s[0] = S._sbox(pk, s[0] + INT_RC[r])
    assert max(frac) <= run.budget, (r, frac)
    run.ledger_peak = max(run.ledger_peak, max(frac))
    a = run.add
    ti = a(a(a(a(s[0], s[1]), a(s[2], s[4])), a(a(s[5], s[7]), a(s[8], s[12]))), s[15])
    tf = a(a(a(s[3], s[6]), a(s[9], s[10])), a(a(s[11], s[13]), s[14]))
    pk.rec("integer partial sum", ti)
    pk.recd("dyadic partial sum", tf, max(frac))
    run.seen[("sum", None, r)] = (tf, max(frac))
    tot = pk.rec("reduced lane sum", run.reduce(a(ti, run.fold_dyadic(tf))))
    out, nf = [], list(frac)
    for i in range(16):
        if i == 1:
            v = a(tot, s[1])
        else:
            v = run.fma(s[i], V[i], tot)
        if i in DYADIC_K:
            nf[i] = frac[i] + DYADIC_K[i]
            pk.recd("dyadic lane", v, nf[i])
            if r in dyadic_folds(DYADIC_K[i], run.budget):
                run.seen[("lane", i, r)] = (v, nf[i])
                v = run.fold_dyadic(pk.recd("lane before a fold", v, nf[i]))
                nf[i] = 0
        else:
            pk.rec("integer lane", v)
            if r in INTEGER_FOLDS.get(i, ()):
                v = run.reduce(pk.rec("lane before a fold", v))
        out.append(v)
    return out, nf


def internal_rounds(run, s):
    """p2f::internal_rounds on integer-valued doubles |s_i| <= 2^37: integers |.| < 2^37 out"""
    s, frac = [float(v) for v in s], [0] * 16
    assert all(v.is_integer() and abs(v) <= 2.0 ** 37 for v in s)
    for r in range(ROUNDS):
        s, frac = internal_round(run, s, frac, r)
    assert frac == [0] * 16
    for v in s:
        assert abs(run.pk.rec("exit", v)) < 2.0 ** 37
    return s


def reference_rounds(state):
    """the thirteen internal rounds in plain integers mod P (pyref's S-box exponent and matrix)"""
    import pyref
    s = [int(v) % P for v in state]
    for r in range(ROUNDS):
        s[0] = pow((s[0] + S.IT[r]) % P, 7, P)
        s = pyref._int(s)
    return s


# ---- entries of the internal rounds ----------------------------------------------------------------------------------------------
M37 = 2 ** 37 - 1
MAGNITUDES = (P - 1, 35 * (P // 2 + 2 ** 9), M37)
SIGN_PATTERNS = (("all +", (1,) * 16), ("all -", (-1,) * 16), ("signs of V", S.V_SIGN), ("-signs of V", tuple(-s for s in S.V_SIGN)),
                 ("alternating", tuple(1 if i % 2 else -1 for i in range(16))))


def pattern_entries():
    """every sign pattern at every magnitude, the all-zero entry, +-(2^37 - 1) on one lane at a time: 15 + 1 + 32 entries"""
    out = [tuple(m * s for s in sg) for _, sg in SIGN_PATTERNS for m in MAGNITUDES] + [(0,) * 16]
    return out + [tuple(s * M37 if j == i else 0 for j in range(16)) for i in range(16) for s in (1, -1)]


def seam3_entries():
    """what the internal rounds are entered with when the S-box outputs of external round 3 are the family's targets y (the signed
    representatives themselves): one external linear layer of y, in exact integers.  103 entries, |.| <= 35 (P + 1) / 2"""
    pk = S.Peaks()
    return [tuple(int(v) for v in S._f_external_linear(pk, [float(v) for v in y])) for _, y in S.targets()]


def random_entries(n, seed):
    rng = np.random.default_rng([F.SEED, seed])
    return [tuple(int(v) for v in row) for row in rng.integers(-M37, M37 + 1, size=(n, 16))]


# ---- the same schedule in integers: lane i is the pair (numerator n_i, bits f_i) ---------------------------------------------------
def simulate(entries):
    """The thirteen rounds on an (N, 16) int64 array of entries, in integer arithmetic: an integer lane is kept as its residue, a
    dyadic lane as the exact numerator of value = n / 2^f (|n| < 2^53), the reduced lane sum as the centred representative (what
    reduce returns away from its rounding ties).  No floating point.  Returns (residues (N, 16) after round 12,
    {(lane, round): (numerators before that fold, bits)}, {round: (numerators of the dyadic partial sum, bits)})."""
    e = np.asarray(entries, dtype=np.int64)
    assert e.ndim == 2 and e.shape[1] == 16 and np.abs(e).max(initial=0) <= 2 ** 37
    lane = [e[:, i].copy() for i in range(16)]
    for i in range(16):
        if i not in DYADIC_K:
            lane[i] %= P
    bits = {i: 0 for i in DYADIC_K}
    folds, sums = {}, {}

    def fold(n, f):
        return (n - (n & ((1 << f) - 1)) * P) >> f

    for r in range(ROUNDS):
        x = (lane[0] + int(S.IT[r])) % P
        x2 = x * x % P
        x3 = x2 * x % P
        lane[0] = x3 * (x2 * x2 % P) % P
        fmax = max(bits.values())
        tf = sum(lane[i] << (fmax - bits[i]) for i in DYADIC_LANES)
        sums[r] = (tf, fmax)
        tot = (sum(lane[i] for i in SUM_INTEGER_LANES) + fold(tf, fmax)) % P
        tot = np.where(tot > P // 2, tot - P, tot)
        for i in range(16):
            if i in DYADIC_K:
                k = DYADIC_K[i]
                lane[i] = (lane[i] if V[i] > 0 else -lane[i]) + (tot << (bits[i] + k))
                bits[i] += k
                assert np.abs(lane[i]).max(initial=0) < 2 ** 53
                if r in DYADIC_FOLDS[i]:
                    folds[(i, r)] = (lane[i], bits[i])
                    lane[i], bits[i] = fold(lane[i], bits[i]), 0
            else:
                lane[i] = (tot + int(V[i]) * lane[i]) % P
    return np.stack([v % P for v in lane], axis=1), folds, sums


@functools.lru_cache(maxsize=None)
def fold_edge_entries():
    """((what, lane or None, round, fraction numerator, sign, entry), ...): entries at which a dyadic lane reaches its FIRST fold, or
    the dyadic partial sum a round's fold, on a chosen fractional part with a chosen sign of the value.  For every dyadic lane: its
    first fold (F = the lane's bits there) at fractions 0, 2^-F and 1 - 2^-F; for the partial sum: the sum of round 1 (F = 8, the
    first with a fraction) and of round 7 (F = 14, where the ledger peaks) at fractions 0 and 1 - 2^-F; each with a positive and with a
    negative value (fract of a negative number is where a wrong identity shows).
    Built from a seeded pool of entries of magnitude 2^35: simulate() gives the numerator the site would see; adding m P, |m| <= 31, to
    the steering lane (the lane itself; lane 9 resp. 10 for the sums, the lanes that hold the sum's lowest bit) keeps every residue,
    hence every reduced lane sum, and moves the numerator by +-m (P = 1 mod 2^F): the pool entries within reach of a target are
    taken and simulated again, and the property is asserted on that second pass."""
    rng = np.random.default_rng([F.SEED, 19])
    pool = rng.integers(-2 ** 35, 2 ** 35 + 1, size=(1 << 14, 16), dtype=np.int64)
    _, folds, sums = simulate(pool)
    sites = [("lane", i, DYADIC_FOLDS[i][0], i, (0, 1, -1)) for i in DYADIC_LANES] + [("sum", None, 1, 9, (0, -1)), ("sum", None, 7, 10, (0, -1))]
    picked = []
    for what, lane, r, steer, fracs in sites:
        n, f = folds[(lane, r)] if what == "lane" else sums[r]
        # the steering lane's value enters the numerator with the sign of V^(rounds so far), at the numerator's lowest bit
        sg = 1 if V[steer] > 0 or (r + (what == "lane")) % 2 == 0 else -1
        for fr in fracs:
            want = fr % (1 << f)
            d = (want - n + (1 << (f - 1))) % (1 << f) - (1 << (f - 1))  # the centred distance to the target
            for sign in (1, -1):
                ok = np.flatnonzero((np.abs(d) <= 31) & ((n + d * P > 0) == (sign > 0)) & (np.abs(n + d * P) >> f > 2 ** 20))
                assert len(ok), (what, lane, r, fr, sign)
                entry = pool[ok[0]].copy()
                entry[steer] += sg * int(d[ok[0]]) * P
                picked.append((what, lane, r, want, sign, tuple(int(v) for v in entry)))
    _, folds, sums = simulate(np.array([p[5] for p in picked], dtype=np.int64))
    for j, (what, lane, r, want, sign, _) in enumerate(picked):
        n, f = folds[(lane, r)] if what == "lane" else sums[r]
        assert int(n[j]) & ((1 << f) - 1) == want and (n[j] > 0) == (sign > 0) and abs(int(n[j])) >> f >= 1, (what, lane, r, want, sign)
    return tuple(picked)


def model_d(state, run=None):
    """p2f::permute with the dyadic internal rounds on integer-valued `state`: (raw doubles out, the state entering the internal
    rounds), through poseidon2_sched_ref._permute and its model of the external layers"""
    run = Run() if run is None else run
    return S._permute(run.pk, state, S._f_external_linear, lambda pk, s: internal_rounds(run, s))
