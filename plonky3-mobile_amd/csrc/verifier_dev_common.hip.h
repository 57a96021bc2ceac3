// What the device batch verifiers share besides the opening walk (lane_walk.hip.h): pcs_verifier_dev.hip (PCS proofs) and its two owners,
// verifier_dev.hip (fib_air proofs) and air_verifier_dev.hip (a caller-defined AIR's), each a front kernel over the header that hands
// the FRI section to an owned PcsVerifierDev.  Here: the ONE scale of order keys every check reports through and the reject codes, the
// readers of proof words, the export of a challenger, FriCheck's fold step and final polynomial, and the FRI tail of the transcript.
// Each verifier keeps its own args and layout structs: the helpers that read them are templates over the fields they name (key, lens,
// proofs, stride; proof_words).
#pragma once
#include <cstddef>

#include "bb31.hip.h"
#include "lane_walk.hip.h"
#include "prover.h"
#include "transcript.hip.h"

namespace p3 {
namespace vdev {

using bb::Ext;

// The first failure in the HOST's order decides the code: every check does atomicMin on a per-proof word (order key << 8 | code).
// The scale, smaller = earlier:
//   KEY_HEADER  a wrong length, a dictated word of an owner's header, ANY word that is no canonical field element (wherever it lies:
//               the host's readers flag it where they meet it, the device answers MALFORMED whatever else is wrong), a member's values
//   KEY_OWNER   the check an owner makes between its header and the FRI section: the constraints at zeta (CODE_OOD, ood.hip.h)
//   KEY_SHAPE   the count words of the FRI section outside the queries (rounds, queries, final polynomial length) and, for a shape
//               with PLayout::counts, the count words inside the queries that wire format 1's host follows to the final polynomial
//   KEY_POW     the proof of work
//   KEY_QUERY0  the queries, STEPS_PER_QUERY keys each: opening s of query q reports its count words at 2 s and its path at 2 s + 1
// A member whose key is at KEY_HEADER is DECIDED: every key-0 report is MALFORMED and nothing precedes it, so the later kernels skip it
// (an owner hands such a member on unread).  A member at any later key is walked to the end, whatever it holds so far: a word that is
// no field element, found by the opening kernel, still precedes an owner's 10, a count word's 16 and the proof of work's 11.
constexpr uint64_t KEY_HEADER = 0, KEY_OWNER = 1, KEY_SHAPE = 2, KEY_POW = 3, KEY_QUERY0 = 4, KEY_NONE = ~0ull;
constexpr uint32_t STEPS_PER_QUERY = 64;  // 2 (openings + FRI rounds) + 1 <= 2 (4 + 27) + 1
constexpr uint32_t CODE_POW = 11, CODE_INPUT_OPENING = 13, CODE_FRI_OPENING = 14, CODE_FINAL_POLY = 15;

__device__ __forceinline__ uint64_t make_key(uint64_t order, uint32_t code) { return (order << 8) | code; }
__device__ __forceinline__ uint64_t kmin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ bool decided(uint64_t key) { return (key >> 8) == KEY_HEADER; }
template <typename A>
__device__ __forceinline__ void report(const A& a, uint32_t i, uint64_t order, uint32_t code) {
    atomicMin(a.key + i, (unsigned long long)make_key(order, code));
}
// a proof whose length differs from the layout's is rejected unread
template <typename A, typename LY>
__device__ __forceinline__ bool length_ok(const A& a, const LY& L, uint32_t i) { return !a.lens || a.lens[i] == 4u * L.proof_words; }
template <typename A>
__device__ __forceinline__ const uint32_t* proof_words(const A& a, uint32_t i) {
    return reinterpret_cast<const uint32_t*>(a.proofs + (size_t)i * a.stride);
}
__device__ __forceinline__ Ext ldx(const uint32_t* w, size_t off) { return Ext{{w[off], w[off + 1], w[off + 2], w[off + 3]}}; }
__device__ __forceinline__ void stx(uint32_t* w, size_t off, const Ext& e) { for (int c = 0; c < 4; c++) w[off + c] = e.c[c]; }
__device__ __forceinline__ uint32_t rev_bits_dev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32u - bits) : 0u; }

// order key -> status, count of rejected proofs: the body of pv_finish_kernel
__device__ __forceinline__ void finish(const unsigned long long* key, uint32_t n, uint32_t* status, uint32_t* d_rejected) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < n;
    const uint32_t st = act && key[i] != KEY_NONE ? (uint32_t)(key[i] & 0xffu) : 0u;
    if (act) status[i] = st;
    count_rejected(st != 0u, d_rejected);
}

// A challenger's state written where the next verifier imports it (one wavefront; the state ends there).  The other configuration's
// half is zero, as challenger_export leaves it.
constexpr uint32_t SW_KC = offsetof(DevState, kc) / 4;  // where the Keccak half begins (transcript.hip.h DevState)
static_assert(offsetof(DevState, pis) == (size_t)CHALLENGER_STATE_WORDS * 4 && CHALLENGER_STATE_WORDS % 2 == 0, "state words");
__device__ __forceinline__ void export_challenger(DevChal& ch, int hash, uint32_t* out, uint32_t lane) {
    const uint32_t lo = hash == HASH_POSEIDON2 ? SW_KC : 0u, hi = hash == HASH_POSEIDON2 ? CHALLENGER_STATE_WORDS : SW_KC;
    for (uint32_t j = lo + lane; j < hi; j += 64) out[j] = 0u;
    ch.ds = reinterpret_cast<DevState*>(out);
    ch.end();
}

// One step of FriCheck::query's walk, from 2^(lfh + 1) to 2^lfh elements: the pair (ev0, ev1) this query's leaf of the round must
// hold (`folded` at the index's parity, the proof's sibling at the other) and the fold at beta; the next index is idx >> 1.
__device__ __forceinline__ Ext fri_fold_step(const Ext& folded, uint32_t idx, const Ext& sib, const Ext& beta, uint32_t lfh, const uint32_t* gens,
                                             const uint32_t* gens_inv, uint32_t neg_half, Ext& ev0, Ext& ev1) {
    const bool odd = idx & 1u;
    ev0 = odd ? sib : folded;
    ev1 = odd ? folded : sib;
    const uint32_t e = rev_bits_dev(idx >> 1, lfh);
    const uint32_t s = bb::pow(gens[lfh + 1], e), s_inv = bb::pow(gens_inv[lfh + 1], e);
    const Ext num = bb::mul(bb::sub(beta, bb::ext_from_base(s)), bb::sub(ev1, ev0));
    return bb::add(ev0, bb::scale(num, bb::mul(neg_half, s_inv)));  // 1 / (-s - s)
}
// the final polynomial (fpl coefficients at w + fpoly_off) at g_lfinal^bitrev(idx), where the walk ends
__device__ __forceinline__ Ext final_poly_eval(const uint32_t* w, uint32_t fpoly_off, uint32_t fpl, uint32_t g_lfinal, uint32_t lfinal, uint32_t idx) {
    const uint32_t xf = bb::pow(g_lfinal, rev_bits_dev(idx, lfinal));
    Ext evf = bb::ext_zero();
    for (uint32_t k = fpl; k-- > 0;) evf = bb::add(bb::scale(evf, xf), ldx(w, fpoly_off + 4 * (size_t)k));
    return evf;
}

// The FRI tail of the transcript (one wavefront, `lane` its lane): per round observe the root and sample beta; observe the final
// polynomial and the witness; the proof-of-work sample; the nq query indices.  FriTail: where the commit-phase roots, the final
// polynomial and the witness are among the proof's words, and the parameters.  Lane 0 leaves the betas and the indices at `beta` and
// `idx`.  Returns whether the proof of work holds.
struct FriTail {
    uint32_t froots_off, n_rounds, fpoly_off, fpl, witness_off, pow_bits, nq, log_big;
};
__device__ __forceinline__ bool fri_transcript_tail(DevChal& ch, const uint32_t* w, uint32_t lane, const FriTail& t, Ext* beta, uint32_t* idx) {
    for (uint32_t r = 0; r < t.n_rounds; r++) {
        ch.observe_n(w + t.froots_off + 8 * r, 8);
        const Ext b = ch.sample_ext();
        if (lane == 0) beta[r] = b;
    }
    for (uint32_t k = 0; k < 4 * t.fpl; k++) ch.observe(w[t.fpoly_off + k]);
    ch.observe(w[t.witness_off]);
    const bool pow_ok = ch.sample_bits(t.pow_bits) == 0;
    for (uint32_t q = 0; q < t.nq; q++) {
        const uint32_t index = ch.sample_bits(t.log_big);
        if (lane == 0) idx[q] = index;
    }
    return pow_ok;
}

}  // namespace vdev
}  // namespace p3
