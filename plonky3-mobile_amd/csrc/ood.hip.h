// The arithmetic of the out-of-domain check of p3_uni_stark::verify, ONE statement for the host and the device and for every verifier:
// air_verifier_dev.hip (a caller-defined AIR: air_verify on the host, av_eval_kernel on the device), verifier.hip (verify_fib) and
// verifier_dev.hip (fv_front_kernel).  The selectors at zeta, the quotient recomposed from its chunks, and FibonacciAir's five
// constraints.  Each caller keeps its own final comparison: the AIR side asks folded == quotient Z_H, the fib side folded / Z_H ==
// quotient (inv(0) = 0: they differ only where Z_H(zeta) = 0).
#pragma once
#include <cstring>

#include "air.h"  // AIR_MAX_CHUNKS
#include "bb31.hip.h"

namespace p3 {

constexpr uint32_t CODE_OOD = 10;  // OodEvaluationMismatch, the reject code of every verifier, host and device

// ---- what depends only on (log_n, log_quotient_degree): the trace domain's generator and the quotient chunks' cosets D_j = s_j <g_n>,
// s_j = GENERATOR g_qn^j (so s_j^n = GENERATOR^n w^j, w of order 2^lqd).  ONE routine for the host verifiers and the device layouts. ----
struct OodDomain {
    uint32_t g_n, g_n_inv;
    uint32_t sn[AIR_MAX_CHUNKS];       // s_j^n
    uint32_t sn_inv[AIR_MAX_CHUNKS];   // its inverse: Z_{D_j}(x) = x^n / s_j^n - 1
    uint32_t izd[AIR_MAX_CHUNKS][AIR_MAX_CHUNKS];  // [c][j] = 1 / Z_{D_j}(s_c), j != c
};

inline void ood_domain(uint32_t log_n, uint32_t lqd, OodDomain* d) {
    memset(d, 0, sizeof(*d));
    const uint32_t C = 1u << lqd;
    const uint64_t n = 1ull << log_n;
    d->g_n = bb::two_adic_generator(log_n);
    d->g_n_inv = bb::inv(d->g_n);
    const uint32_t g_qn = bb::two_adic_generator(log_n + lqd);
    uint32_t s = bb::to_monty(bb::GEN);
    for (uint32_t j = 0; j < C; j++) {
        d->sn[j] = bb::pow(s, n);
        d->sn_inv[j] = bb::inv(d->sn[j]);
        s = bb::mul(s, g_qn);
    }
    for (uint32_t c = 0; c < C; c++)
        for (uint32_t j = 0; j < C; j++)
            if (j != c) d->izd[c][j] = bb::inv(bb::sub(bb::mul(d->sn[c], d->sn_inv[j]), bb::ONE));
}

// selectors_at_point on the trace domain: Z_H = zeta^n - 1, first = Z_H / (zeta - 1), last = Z_H / (zeta - g_n^-1), trans = zeta -
// g_n^-1; inv(0) = 0 as bb::inv has it
BB_HD void ood_selectors(const bb::Ext& zeta, uint32_t log_n, uint32_t g_n_inv, bb::Ext& first, bb::Ext& last, bb::Ext& trans, bb::Ext& zn, bb::Ext& zh) {
    zn = zeta;
    for (uint32_t k = 0; k < log_n; k++) zn = bb::sqr(zn);
    zh = bb::sub(zn, bb::ext_one());
    trans = bb::sub(zeta, bb::ext_from_base(g_n_inv));
    first = bb::mul(zh, bb::inv(bb::sub(zeta, bb::ext_one())));
    last = bb::mul(zh, bb::inv(trans));
}

// quotient(zeta) = sum_c zps_c sum_e X^e chunk_c[e], zps_c = prod_{j != c} Z_{D_j}(zeta) / Z_{D_j}(s_c) (with one chunk the product is
// empty; a hiding proof's blinding cancels in the sum).  chunks: 16 words per chunk, an extension element's 4 coordinates each, chunk c at
// chunks + c stride (16: contiguous; 17: in a proof's header, each chunk behind its count word)
BB_HD bb::Ext ood_quotient(const OodDomain& d, uint32_t n_chunks, const bb::Ext& zn, const uint32_t* chunks, uint32_t stride = 16) {
    bb::Ext quot = bb::ext_zero();
    for (uint32_t c = 0; c < n_chunks; c++) {
        bb::Ext zps = bb::ext_one();
        for (uint32_t j = 0; j < n_chunks; j++) {
            if (j == c) continue;
            const bb::Ext num = bb::sub(bb::scale(zn, d.sn_inv[j]), bb::ext_one());
            zps = bb::mul(zps, bb::scale(num, d.izd[c][j]));
        }
        bb::Ext val = bb::ext_zero();
        for (uint32_t e = 0; e < 4; e++) {
            bb::Ext be = bb::ext_zero();
            be.c[e] = bb::ONE;
            const uint32_t* p = chunks + stride * c + 4 * e;
            val = bb::add(val, bb::mul(be, bb::Ext{{p[0], p[1], p[2], p[3]}}));
        }
        quot = bb::add(quot, bb::mul(zps, val));
    }
    return quot;
}

// FibonacciAir (fib_air.rs:232-264) at zeta, folded with alpha by Horner's rule: the two columns of the trace at zeta (loc) and at
// zeta g_n (nxt), 4 words a column; pis = [a, b, x] in Montgomery form
BB_HD bb::Ext fib_constraints_folded(const uint32_t* loc, const uint32_t* nxt, const uint32_t pis[3], const bb::Ext& first, const bb::Ext& last,
                                     const bb::Ext& trans, const bb::Ext& alpha) {
    const bb::Ext l0{{loc[0], loc[1], loc[2], loc[3]}}, l1{{loc[4], loc[5], loc[6], loc[7]}};
    const bb::Ext n0{{nxt[0], nxt[1], nxt[2], nxt[3]}}, n1{{nxt[4], nxt[5], nxt[6], nxt[7]}};
    const bb::Ext c[5] = {bb::mul(first, bb::sub(l0, bb::ext_from_base(pis[0]))), bb::mul(first, bb::sub(l1, bb::ext_from_base(pis[1]))),
                          bb::mul(trans, bb::sub(l1, n0)), bb::mul(trans, bb::sub(bb::add(l0, l1), n1)),
                          bb::mul(last, bb::sub(l1, bb::ext_from_base(pis[2])))};
    bb::Ext folded = bb::ext_zero();
    for (int k = 0; k < 5; k++) folded = bb::add(bb::mul(folded, alpha), c[k]);
    return folded;
}

}  // namespace p3
