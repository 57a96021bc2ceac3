// The layout of one PCS shape: pcs_layout.h.  Host code only.  What a verifier checks on a member's VALUES (points, opened values) is
// not here: the host verifier does it behind this, the device verifier in its kernels.
// EVERY ARRAY WRITE BELOW IS BEHIND THE GATE THAT BOUNDS ITS INDEX, the counts being the caller's (p3hip_pcs_verify* reach this):
//   r < n_rounds <= PCS_MAX_ROUNDS = PV_MAX_IN;  mi < sum of mats_per_round <= PCS_MAX_ROUNDS max_mats <= PV_MAX_ALLMATS;
//   pi < sum of points_per_mat <= PV_MAX_ALLMATS PCS_MAX_POINTS = PV_MAX_PAIRS;  a class lb <= log_big <= TWO_ADICITY < PV_MAX_FRI;
//   total and every class counter <= PCS_MAX_COLS when stored in 16 bits.
#include <algorithm>
#include <cstring>

#include "bb31.hip.h"
#include "common.h"
#include "mmcs.h"
#include "pcs_layout.h"

namespace p3 {

static_assert(bb::TWO_ADICITY < 32 && PV_MAX_FRI > bb::TWO_ADICITY, "a class is a bit of a 32-bit mask and an index of gens[]");

int pcs_layout(int hash, bool hiding, const FriParams& fp, const PcsShape& sh, PLayout* out, uint64_t* proof_words, std::string* why) {
    auto bad = [&](const std::string& msg) { if (why) *why = msg; return (int)ERR_BAD_ARG; };
    if (!sh.mats_per_round || !sh.widths || !sh.points_per_mat) return bad("pcs verify: null argument");
    if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return bad("pcs verify: unknown hash configuration");
    uint32_t log_h = sh.log_h;
    const size_t n_rounds = sh.n_rounds, max_mats = hiding ? PCS_HIDING_MAX_MATS : PCS_MAX_MATS;
    auto rounds_gate = [&]() {
        if (n_rounds == 0) return bad("pcs verify: zero rounds");
        return n_rounds > PCS_MAX_ROUNDS ? bad("pcs verify: " + std::to_string(n_rounds) + " rounds, at most " + std::to_string(PCS_MAX_ROUNDS)) : 0;
    };
    auto mats_gate = [&](size_t r) {
        if (sh.mats_per_round[r] == 0) return bad("pcs verify: round " + std::to_string(r) + " has zero matrices");
        return sh.mats_per_round[r] > max_mats ? bad("pcs verify: round " + std::to_string(r) + " has more than " + std::to_string(max_mats) + " matrices") : 0;
    };
    const char* lde_msg = "pcs verify: LDE height outside [2^2, 2^27]";
    uint32_t lh[PV_MAX_ALLMATS];  // per matrix, filled either way
    if (sh.log_heights) {
        if (hiding) return bad("pcs verifier: mixed heights are not covered for HidingFriPcs (no hiding prover produces them): hiding must be 0");
        if (int rc = rounds_gate()) return rc;
        size_t nm = 0;
        for (size_t r = 0; r < n_rounds; nm += sh.mats_per_round[r++])
            if (int rc = mats_gate(r)) return rc;
        uint32_t lo = ~0u;
        log_h = 0;
        for (size_t m = 0; m < nm; m++) { lh[m] = sh.log_heights[m]; log_h = std::max(log_h, lh[m]); lo = std::min(lo, lh[m]); }
        // (log_h and log_blowup bounded alone: a class is log_h_m + log_blowup, an index below, and must not wrap)
        if (lo < 1 || log_h > bb::TWO_ADICITY || fp.log_blowup > bb::TWO_ADICITY) return bad(lde_msg);
    }
    if (hiding) {
        if (log_h < 1 || log_h >= bb::TWO_ADICITY)
            return bad("pcs verify: log_h must be in [1, " + std::to_string(bb::TWO_ADICITY - 1) + "] (the caller's log height; the committed polynomials have degree < 2^(log_h + 1))");
        log_h++;
    }
    if (log_h < 1 || fp.log_blowup < 1 || log_h + fp.log_blowup > bb::TWO_ADICITY) return bad(lde_msg);
    if (fp.log_final_poly_len >= log_h) return bad("pcs verify: log_final_poly_len must be below the matrices' log height");
    if (fp.proof_of_work_bits > 30) return bad("pcs verify: proof_of_work_bits too large");
    if (fp.num_queries == 0) return bad("pcs verify: num_queries must be positive");
    if (int rc = rounds_gate()) return rc;
    if (sh.slots && (sh.n_slots < 1 || sh.n_slots > PCS_MAX_SLOTS)) return bad("pcs verifier: n_slots must be in [1, " + std::to_string(PCS_MAX_SLOTS) + "]");
    PLayout& L = *out;
    memset(&L, 0, sizeof(L));
    L.hash = hash;
    L.salt = hiding ? PCS_SALT : 0;
    L.log_big = log_h + fp.log_blowup;
    L.lfinal = fp.log_blowup + fp.log_final_poly_len;
    L.n_fri = L.log_big - L.lfinal;
    L.nq = fp.num_queries;
    L.fpl = 1u << fp.log_final_poly_len;
    L.pow_bits = fp.proof_of_work_bits;
    L.n_in = (uint32_t)n_rounds;
    L.n_slots = sh.slots ? (uint32_t)sh.n_slots : 0;
    L.counts = sh.counts ? 1 : 0;
    const uint32_t D = 8;
    size_t mi = 0, pi = 0, total = 0;
    uint32_t cnt[bb::TWO_ADICITY + 1] = {0};  // alpha powers consumed so far, per class
    uint64_t p = 1;  // within a query, behind the count of rounds
    for (size_t r = 0; r < n_rounds; r++) {
        if (int rc = mats_gate(r)) return rc;
        const size_t nm = sh.mats_per_round[r];
        L.nm[r] = (uint32_t)nm;
        L.mat0[r] = (uint32_t)mi;
        L.open_off[r] = (uint32_t)p++;
        uint32_t leaf[bb::TWO_ADICITY + 1] = {0};  // the row of each class of the round so far
        for (size_t m = 0; m < nm; m++, mi++) {
            const std::string who = "pcs verify: round " + std::to_string(r) + " matrix " + std::to_string(m);
            const size_t wd = sh.widths[mi], np = sh.points_per_mat[mi];
            if (wd < 1 || wd > PCS_MAX_COLS) return bad(who + ": width must be in [1, " + std::to_string(PCS_MAX_COLS) + "]");
            if (np > PCS_MAX_POINTS) return bad(who + ": more than " + std::to_string(PCS_MAX_POINTS) + " opening points");
            if (!sh.log_heights) lh[mi] = log_h;
            if (lh[mi] < fp.log_final_poly_len)
                return bad(who + " has height 2^" + std::to_string(lh[mi]) + ", below the final polynomial's 2^" + std::to_string(fp.log_final_poly_len));
            const uint32_t lb = lh[mi] + fp.log_blowup;  // <= log_big <= TWO_ADICITY
            L.log_big_m[mi] = (uint8_t)lb;
            L.log_big_r[r] = std::max(L.log_big_r[r], lb);
            L.round_mask[r] |= 1u << lb;
            if (np) L.class_mask |= 1u << lb;
            if (lb != L.log_big) L.mixed = 1;
            L.width[mi] = (uint32_t)wd;
            L.np[mi] = (uint32_t)np;
            L.val_off[mi] = (uint32_t)(p + 1);
            p += 1 + wd;
            L.leaf_start[mi] = leaf[lb];
            leaf[lb] += (uint32_t)wd + L.salt;
            L.wmax = std::max(L.wmax, (uint32_t)wd);
            L.row_words += (uint32_t)wd;
            for (size_t k = 0; k < np; k++, pi++) {
                const std::string pw = who + " point " + std::to_string(k);
                if (sh.slots) {
                    if (sh.slots[pi] >= sh.n_slots) return bad(pw + ": slot " + std::to_string(sh.slots[pi]) + " of " + std::to_string(sh.n_slots));
                    L.pair_slot[pi] = (uint8_t)sh.slots[pi];
                }
                L.pair_off[pi] = (uint16_t)total;
                L.pair_aoff[pi] = (uint16_t)cnt[lb];
                cnt[lb] += (uint32_t)wd;
                L.pair_mat[pi] = (uint8_t)mi;
                total += wd;
                if (total > PCS_MAX_COLS) return bad(pw + ": more than " + std::to_string(PCS_MAX_COLS) + " batched columns");
            }
        }
        if (L.salt)
            for (size_t m = 0; m < nm; m++) { L.salt_off[L.mat0[r] + m] = (uint32_t)(p + 1); p += 1 + L.salt; }
        L.leaf_len[r] = leaf[L.log_big_r[r]];
        L.depth_off[r] = (uint32_t)p;
        p += 1 + (uint64_t)D * L.log_big_r[r];
    }
    if (total == 0) return bad("pcs verify: no opening point");
    if (!((L.class_mask >> L.log_big) & 1u))
        return bad("pcs verify: no matrix of the tallest height 2^" + std::to_string(log_h) + " has an opening point: the FRI input would be missing");
    L.n_pairs = (uint32_t)pi;
    L.total = (uint32_t)total;
    L.nr_off = (uint32_t)p++;
    for (uint32_t r = 0; r < L.n_fri; r++) {
        L.fri_off[r] = (uint32_t)p;
        p += 4 + (L.salt ? 1 + L.salt : 0) + 1 + (uint64_t)D * (L.log_big - 1 - r);
    }
    L.q_len = (uint32_t)p;  // a query is below 2^19 words at the caps; only what lies behind nq of them can pass 32 bits
    L.nq_off = 1 + D * L.n_fri;
    L.q_base = L.nq_off + 1;
    const uint64_t after = (uint64_t)L.q_base + p * L.nq;
    if (proof_words) *proof_words = after + 2 + 4ull * L.fpl;
    L.fpl_off = (uint32_t)after;
    L.fpoly_off = L.fpl_off + 1;
    L.witness_off = L.fpoly_off + 4 * L.fpl;
    L.proof_words = L.witness_off + 1;
    L.gen = bb::to_monty(bb::GEN);
    L.gen_inv = bb::inv(L.gen);
    L.neg_half = bb::inv(bb::neg(bb::dbl(bb::ONE)));
    for (uint32_t b = 0; b < PV_MAX_FRI; b++) { L.gens[b] = bb::two_adic_generator(b); L.gens_inv[b] = bb::inv(L.gens[b]); }
    return OK;
}

}  // namespace p3
