// Poseidon2 (same permutation as poseidon2.hip.h) evaluated in DOUBLE PRECISION integer arithmetic.
// On gfx950 int32 and fp64 VALU ops issue at the same rate, but in fp64 a modular addition is ONE exact
// v_add_f64 (no reduction while |v| < 2^53) instead of add/sub/min, which removes ~25% of the permutation's
// instructions.  State elements are doubles holding integers congruent (mod P) to CANONICAL field values
// (not Montgomery): the kernel converts at load/store.
//   mulmod(a, b): h = a*b; l = fma(a, b, -h) (exact error); q = rint(h / P); r = fma(-q, P, h) + l
//     exact for |a*b| < 2^84: h - qP is an integer below 2^33, l an integer below 2^31.  |r| < 1.1 P holds while |a*b| < 2^80 only
//     (q is within 1/2 + |ab| 2^-52 / P of ab / P and |l| <= ulp(ab) / 2; at 2^83 the exact model reaches 1.6 P:
//     tests/test_field_ref_host.py).  No kernel calls mulmod or mulmod_p any more; the field probe pins them to |ab| < 2^76.
#pragma once
#include "poseidon2.hip.h"

namespace p2f {

constexpr double PD = 2013265921.0;
constexpr double PINV = 1.0 / 2013265921.0;

__device__ __forceinline__ double mulmod(double a, double b) {
    double h = a * b;
    double l = __fma_rn(a, b, -h);
    double q = __builtin_rint(h * PINV);
    double r = __fma_rn(-q, PD, h);
    return r + l;
}
// a * b (mod P) when aP = a / P is already known: q = rint(b * aP) is within 1 of a*b/P; q * (P - 1) =
// q * 15 * 2^27 is exact, so t = fma(a, b, -q(P-1)) = (ab - qP) + q is an integer below 2^33, hence exact.
// Five ops, |result| <= P/2 + 1 + |ab| 2^-52.  Exact while |ab| < 2^76.
constexpr double PM1 = 2013265920.0;
__device__ __forceinline__ double mulmod_p(double a, double b, double aP) {
    double q = __builtin_rint(b * aP);
    double t = __fma_rn(a, b, -(q * PM1));
    return t - q;
}
__device__ __forceinline__ double reduce(double x) {  // |result| <= P/2 + eps
    return __fma_rn(-__builtin_rint(x * PINV), PD, x);
}
// tot + x * 2^-K (mod P), K <= 8, for integers |x| < 2^44, |tot| < 2^40: xt = tot + x / 2^K is exact (K fractional
// bits), fract(xt) = (x mod 2^K) / 2^K because tot is an integer, and xt - fract * P = tot + (x - (x mod 2^K) P) / 2^K
// is an integer (P = 1 mod 2^K) below 2^45: three exact ops.  inv = +-2^-K.
// With an INTEGER multiplier inv = m (the quad form passes -2, 1, 2, 3, 4, -3, -4, -15, 15 through here too) xt = tot + m x is an
// integer, fract(xt) = 0 and the result is xt itself: exact while |tot + m x| < 2^53, whatever |x| (the quad form reaches
// |x| = 2^46.8 on the x15 lanes before a fold; tests/poseidon2_sched_ref.py).
__device__ __forceinline__ double add_scaled_pow2(double tot, double x, double inv) {
    double xt = __fma_rn(x, inv, tot);
    double fr = __builtin_amdgcn_fract(xt);
    return __fma_rn(fr, -PD, xt);
}
// The same product in FOUR ops, none of them a rounding instruction: with M = 1.5 * 2^52 (ulp 1),
//   qb = fma(b, aP, M)           = M + rint(b * aP) = M + q                  (the classic magic-number rounding)
//   c  = fma(-qb, P - 1, M * P)  = M - q (P - 1)                             (exact: a multiple of 2^27 below 2^71 plus M; M * P is a double)
//   t  = fma(a, b, c)            = M + (ab - qP) + q                         (exact: M plus an integer below 2^40)
//   t - qb                       = ab - qP                                   (exact difference of two integers below 2^53)
// Valid for |b * aP| < 2^51 and |ab| < 2^76, i.e. for every product of the permutation on canonical inputs: the largest S-box
// input is the FIRST round's, 35 (P - 1) + rc < 2^36.1 (states of words in [0, P)); the later rounds see 35 (P/2 + 2^9) + rc < 2^35.2.
// Under an entry bound |s_i| <= 2^32 it is 35 * 2^32 + P < 2^37.2 and x * x < 2^76 still holds; at 2^33 it is 2^38.14 and x * x =
// 2^76.3 is past the bound stated here.  The algebra has room left (c stays a double while |q| (P - 1) < 2^80) and the exact model
// is right at those operands (tests/test_poseidon2_sched_host.py), but only |ab| < 2^76 is pinned class by class on the device.
// One op less than mulmod_p, two less than mulmod: the S-box drops from 23 to 19 fp64 ops.
constexpr double MAGIC = 6755399441055744.0;                 // 1.5 * 2^52
constexpr double MAGIC_P = 6755399441055744.0 * 2013265921.0;  // 45 * 2^78 + 3 * 2^51: exactly representable
// Operand placement matters: a VOP3 fp64 op reads at most ONE scalar / literal operand on gfx950, and hipcc turns
// fma(x, literal, constant) into v_fmac + a v_mov_b64 copy of the constant per use.  So M and M * P live in VGPR pairs
// the compiler cannot rematerialise (MagicRegs, pinned once per kernel), -(P - 1) comes from an SGPR pair: every line
// below is ONE v_fma_f64 / v_add_f64.
struct MagicRegs { double m, mp; };
__device__ __forceinline__ MagicRegs magic_regs() {
    MagicRegs r{MAGIC, MAGIC_P};
    asm volatile("" : "+v"(r.m), "+v"(r.mp));
    return r;
}
__device__ __forceinline__ double mulmod_m(double a, double b, double aP, const MagicRegs& k, double neg_pm1) {
    const double qb = __fma_rn(b, aP, k.m);
    const double c = __fma_rn(qb, neg_pm1, k.mp);
    const double t = __fma_rn(a, b, c);
    return t - qb;
}
// x^7: x2 = x*x, x3 = x2*x, x4 = x3*x share xP = x / P; the last product x3 * x4 uses x3 / P.
__device__ __forceinline__ double sbox7(double x, const MagicRegs& k, double neg_pm1, double pinv) {
    const double xP = x * pinv;
    const double x2 = mulmod_m(x, x, xP, k, neg_pm1), x3 = mulmod_m(x, x2, xP, k, neg_pm1), x4 = mulmod_m(x, x3, xP, k, neg_pm1);
    return mulmod_m(x3, x4, x3 * pinv, k, neg_pm1);
}

struct ConstsF64 {
    double ext[8][16];
    double in[13];
    // multipliers of the internal diagonal that are not fp64 inline constants, kept in SGPRs (as literals the
    // compiler would pick v_fmac + a copy of the addend): 3, 15, 2^-2, 2^-3, 2^-4, 2^-8
    double k3, k15, i4, i8, i16, i256;
    double neg_pm1, pinv;  // -(P - 1), 1 / P
};
constexpr uint32_t c_from_monty(uint32_t m) {  // m * 2^-32 mod P
    uint32_t t = m * bb::MU;
    uint64_t u = (uint64_t)t * bb::P;
    uint32_t uh = (uint32_t)(u >> 32);
    return uh ? bb::P - uh : 0;  // (m - t*P) >> 32 with hi(m) = 0
}
constexpr uint64_t c_powmod(uint64_t b, uint64_t e) { uint64_t r = 1; b %= bb::P; while (e) { if (e & 1) r = r * b % bb::P; b = b * b % bb::P; e >>= 1; } return r; }
constexpr ConstsF64 make_consts() {
    ConstsF64 c{};
    for (int r = 0; r < 4; r++)
        for (int i = 0; i < 16; i++) {
            c.ext[r][i] = (double)c_from_monty(P3_RC16_EXT_INIT_MONTY[r][i]);
            c.ext[4 + r][i] = (double)c_from_monty(P3_RC16_EXT_FINAL_MONTY[r][i]);
        }
    for (int r = 0; r < 13; r++) c.in[r] = (double)c_from_monty(P3_RC16_INTERNAL_MONTY[r]);
    c.k3 = 3.0; c.k15 = 15.0; c.i4 = 0.25; c.i8 = 0.125; c.i16 = 0.0625; c.i256 = 0.00390625;
    c.neg_pm1 = -2013265920.0; c.pinv = 1.0 / 2013265921.0;
    return c;
}
static __device__ __constant__ ConstsF64 d_c = make_consts();

__device__ __forceinline__ void mat4(double& a, double& b, double& c, double& d) {
    double t01 = a + b, t23 = c + d, t0123 = t01 + t23;
    double t01123 = t0123 + b, t01233 = t0123 + d;
    double nd = __fma_rn(a, 2.0, t01233), nb = __fma_rn(c, 2.0, t01123);
    double na = t01123 + t01, nc = t01233 + t23;
    a = na; b = nb; c = nc; d = nd;
}
__device__ __forceinline__ void external_linear(double (&s)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i += 4) mat4(s[i], s[i + 1], s[i + 2], s[i + 3]);
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = (s[k] + s[k + 4]) + (s[k + 8] + s[k + 12]);
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] += t[i & 3];
}

// The integer congruent (mod P) to a DYADIC FRACTION x = n / 2^F, F <= FRAC_BUDGET: fract(x) = (n mod 2^F) / 2^F is exact, and
// x - fract(x) P = (n - (n mod 2^F) P) / 2^F is an integer because P = 1 (mod 2^27), congruent to n (2^F)^-1.  Two exact ops while
// the result stays below 2^53: |result| < |x| + P.  For an integer x it returns x.
__device__ __forceinline__ double fold_dyadic(double x) {
    return __fma_rn(__builtin_amdgcn_fract(x), -PD, x);
}

// The 13 internal rounds.  Entry: integers |s_i| <= 2^37 (what the fourth external round leaves: 35 (P/2 + 2^9) < 2^35.1).
// Exit: integers |s_i| < 2^37 (2^31.7 at most: a folded dyadic lane is below tot + its share of the entry + P).
// V = [-2, 1, 2, 1/2, 3, 4, -1/2, -3, -4, 2^-8, 1/4, 1/8, 2^-27, -2^-8, -1/16, -2^-27]; 2^-27 = -15 (mod P)
// because P - 1 = 15 * 2^27.  EVERY lane update is one op, fma(s_i, V_i, tot):
//   * the seven lanes with V_i = +-2^-k (3, 6, 9, 10, 11, 13, 14; k = 1, 1, 8, 2, 3, 8, 4) are carried as dyadic fractions: a double
//     holds x 2^-k exactly, so the lane gains k fractional bits per round and is made an integer again (fold_dyadic) only after the
//     round from which one more would pass FRAC_BUDGET = 16 bits, and after round 12.  Magnitudes shrink as the bits grow (a lane
//     is below |entry| 2^-F + 2 |tot|), so magnitude + fraction stays inside 53 bits: 2^37 at F = 0 down to 2^31 at F = 16.
//   * the round's lane sum is formed in two parts: ti over the nine integer lanes, tf over the seven dyadic ones (an integer over
//     2^14 at most; |tf| < 2^39.9 in the first round, where F = 0, 2^37.6 in the second and falling: magnitude and fraction together
//     stay below 48 bits at a sum); tot = reduce(ti + fold_dyadic(tf)).
//   * the integer-multiplier lanes are folded (reduce) each by its own growth: x1, x2 (lanes 1, 2) after round 12 only (2^13 2^37
//     = 2^50); x+-3, x+-4 (4, 5, 7, 8) after rounds 6 and 12 (4^7 2^37 = 2^51); x+-15 (12, 15) after rounds 3, 7 and 12 (15^4 2^37
//     < 2^52.7, then 15^5 2^30 < 2^49.6).  |ti| < 2^50.3.
// Operations outside the S-box: 13 x (8 + 6 adds, fold 2, add 1, reduce 3, 16 lanes) = 468, + 25 dyadic folds x 2 + 16 reduces x 3
// = 566 (it was 13 x 48 + 96 = 720 with add_scaled_pow2 on the seven lanes every round and all eight integer lanes folded after
// rounds 3, 7, 11, 12).  tests/poseidon2_dyadic_ref.py is the exact model of this schedule, step by step; the schedule differs from
// round to round, so the thirteen rounds are unrolled (the folds below are compile-time decisions).
constexpr int FRAC_BUDGET = 16;
constexpr uint32_t dyadic_fold_rounds(int k) {  // bit r: fold the 2^-k lane after round r
    uint32_t m = 0;
    for (int r = 0, f = 0; r < 13; r++) {
        f += k;
        if (f + k > FRAC_BUDGET || r == 12) { m |= 1u << r; f = 0; }
    }
    return m;
}
constexpr uint32_t FOLD_K1 = dyadic_fold_rounds(1), FOLD_K2 = dyadic_fold_rounds(2), FOLD_K3 = dyadic_fold_rounds(3),
                   FOLD_K4 = dyadic_fold_rounds(4), FOLD_K8 = dyadic_fold_rounds(8);
constexpr uint32_t FOLD_X2 = 1u << 12, FOLD_X4 = (1u << 6) | (1u << 12), FOLD_X15 = (1u << 3) | (1u << 7) | (1u << 12);
static_assert(FOLD_K1 == 0x1000 && FOLD_K2 == 0x1080 && FOLD_K3 == 0x1210 && FOLD_K4 == 0x1888 && FOLD_K8 == 0x1aaa, "fold schedule");
__device__ __forceinline__ void internal_rounds(double (&s)[16], const MagicRegs& mk) {
    const double npm1 = d_c.neg_pm1, pinv = d_c.pinv;
    const double k3 = d_c.k3, k15 = d_c.k15, i4 = d_c.i4, i8 = d_c.i8, i16 = d_c.i16, i256 = d_c.i256;
    // A lambda on purpose, as before: a lambda is a host-device function, and a __constant__ table that such a function reads is
    // emitted as externally initialised, so its entries are LOADED (s_load into SGPR pairs, one VOP3 operand each).  Read from
    // device functions only, d_c becomes a private constant of the translation unit whose values the compiler writes as literals:
    // v_fmac + a v_mov_b64 copy of the addend per use (see MagicRegs), in every kernel that reads d_c, the quad form's included.
    auto internal_round = [&](int r) {
        s[0] = sbox7(s[0] + d_c.in[r], mk, npm1, pinv);
        const double ti = (((s[0] + s[1]) + (s[2] + s[4])) + ((s[5] + s[7]) + (s[8] + s[12]))) + s[15];
        const double tf = ((s[3] + s[6]) + (s[9] + s[10])) + ((s[11] + s[13]) + s[14]);
        const double tot = reduce(ti + fold_dyadic(tf));
        s[0] = __fma_rn(s[0], -2.0, tot);
        s[1] = tot + s[1];
        s[2] = __fma_rn(s[2], 2.0, tot);
        s[3] = __fma_rn(s[3], 0.5, tot);
        s[4] = __fma_rn(s[4], k3, tot);
        s[5] = __fma_rn(s[5], 4.0, tot);
        s[6] = __fma_rn(s[6], -0.5, tot);
        s[7] = __fma_rn(s[7], -k3, tot);
        s[8] = __fma_rn(s[8], -4.0, tot);
        s[9] = __fma_rn(s[9], i256, tot);
        s[10] = __fma_rn(s[10], i4, tot);
        s[11] = __fma_rn(s[11], i8, tot);
        s[12] = __fma_rn(s[12], -k15, tot);
        s[13] = __fma_rn(s[13], -i256, tot);
        s[14] = __fma_rn(s[14], -i16, tot);
        s[15] = __fma_rn(s[15], k15, tot);
        if (FOLD_K1 >> r & 1) { s[3] = fold_dyadic(s[3]); s[6] = fold_dyadic(s[6]); }
        if (FOLD_K8 >> r & 1) { s[9] = fold_dyadic(s[9]); s[13] = fold_dyadic(s[13]); }
        if (FOLD_K2 >> r & 1) s[10] = fold_dyadic(s[10]);
        if (FOLD_K3 >> r & 1) s[11] = fold_dyadic(s[11]);
        if (FOLD_K4 >> r & 1) s[14] = fold_dyadic(s[14]);
        if (FOLD_X2 >> r & 1) { s[1] = reduce(s[1]); s[2] = reduce(s[2]); }
        if (FOLD_X4 >> r & 1) { s[4] = reduce(s[4]); s[5] = reduce(s[5]); s[7] = reduce(s[7]); s[8] = reduce(s[8]); }
        if (FOLD_X15 >> r & 1) { s[12] = reduce(s[12]); s[15] = reduce(s[15]); }
    };
#pragma unroll
    for (int r = 0; r < 13; r++) internal_round(r);
}

// Entry: integers |s_i| <= 2^32.  That is what the S-box's stated contract (mulmod_m: |ab| < 2^76) supports: the first round's
// x = 35 s + rc gives x * x < 2^74.3.  Every caller is far inside it: words in [0, P) from load_elem, or |s_i| <= P/2 + eps after the
// reduce between two absorptions.  (This comment used to say 2^33: every intermediate still stays below 2^53 there and the exact
// model agrees with the integers, the probe's modes 0 and 3 run it, but x * x = 2^76.3 is outside what mulmod_m states.)
__device__ __forceinline__ void permute(double (&s)[16]) {
    const MagicRegs mk = magic_regs();
    const double npm1 = d_c.neg_pm1, pinv = d_c.pinv;
    external_linear(s);  // <= 35 * 2^32 < 2^38
    _Pragma("clang loop unroll(disable)")
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox7(s[i] + d_c.ext[r][i], mk, npm1, pinv);  // |.| <= P/2 + 2^9
        external_linear(s);                                                // <= 35 (P/2 + 2^9) < 2^35.1
    }
    internal_rounds(s, mk);
    _Pragma("clang loop unroll(disable)")
    for (int r = 4; r < 8; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox7(s[i] + d_c.ext[r][i], mk, npm1, pinv);
        external_linear(s);
    }
}

// Montgomery word <-> canonical double
__device__ __forceinline__ double load_elem(uint32_t monty) { return (double)bb::from_monty(monty); }
// The Montgomery word of an (unreduced) result, v * 2^32 mod P, straight from the four-op product with the constant
// 2^32 mod P: |v| < 2^37 here, so the signed remainder lies within (-P/2 - 2^12, P/2 + 2^12); one conversion, and
// min(w, w + P) on the unsigned bit pattern adds P exactly to the negative ones: 7 instructions, where reduce + sign fix +
// convert + the integer to_monty took 15.
constexpr double R_MOD_P = 268435454.0;                        // 2^32 mod P
constexpr double R_MOD_P_OVER_P = 268435454.0 / 2013265921.0;
__device__ __forceinline__ uint32_t store_elem(double v, const MagicRegs& k) {
    const double r = mulmod_m(R_MOD_P, v, R_MOD_P_OVER_P, k, d_c.neg_pm1);
    const uint32_t w = (uint32_t)(int32_t)r;
    return min(w, w + bb::P);
}
__device__ __forceinline__ uint32_t store_elem(double v) { return store_elem(v, magic_regs()); }

}  // namespace p2f
