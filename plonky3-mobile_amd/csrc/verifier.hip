// fib_air verifier (host only): p3_uni_stark::verify + TwoAdicFriPcs::verify + p3_fri::verifier for FibonacciAir,
// the second half of the reference's run_fib_air_zk (native/src/fib_air.rs:70-72: prove, then verify, then
// "fib_air zk ok").  Verification is a few thousand permutations — it is the verifier's role, runs on the host
// exactly as in the reference, and is not a fallback for any device kernel.  Written against the wire format
// of prover.hip; independent of the test oracle.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bb31.hip.h"
#include "challenger.h"
#include "common.h"
#include "mmcs.h"
#include "pcs_layout.h"
#include "poseidon2.hip.h"
#include "prover.h"

namespace p3 {

using bb::Ext;

namespace {

struct Reader {
    const uint8_t* p; size_t len, pos = 0; bool bad = false;
    uint32_t u32() { uint32_t v = 0; if (pos + 4 > len) { bad = true; return 0; } memcpy(&v, p + pos, 4); pos += 4; return v; }
    uint32_t felt() { uint32_t v = u32(); if (v >= bb::P) bad = true; return v; }
    void felts(uint32_t* w, size_t n) { for (size_t i = 0; i < n; i++) w[i] = felt(); }
    Ext ext() { Ext e; felts(e.c, 4); return e; }
    // n digests: 8 field elements each (Poseidon2) or raw [u64; 4] bytes (Keccak)
    void digests(int hash, uint32_t* w, size_t n) { if (hash == HASH_POSEIDON2) felts(w, 8 * n); else for (size_t i = 0; i < 8 * n; i++) w[i] = u32(); }
};

// MerkleTreeMmcs::verify_batch (mmcs_verify.hip) of ONE matrix of 2^depth rows: the leaf row (every opened matrix's values, each followed by
// its salt under the hiding MMCS, all of one height) up the path.  Words are hashed as they are: the Reader flags a word >= P (rd.bad),
// and which reject code such a proof gets is this file's business, unchanged.
bool verify_opening(int hash, const uint32_t root[8], size_t index, const uint32_t* row, size_t width, const uint32_t* path, unsigned depth) {
    const size_t height = (size_t)1 << depth;
    return mmcs_verify_batch(hash, root, &height, &width, 1, index, row, path, depth, nullptr, false) == 0;
}
size_t rev_bits_host(size_t x, unsigned bits) { size_t y = 0; for (unsigned i = 0; i < bits; i++) { y = (y << 1) | (x & 1); x >>= 1; } return y; }

int reject(std::string* why, int code, const char* msg) { if (why) *why = msg; return code; }

// the widest opening: the hiding quotient's four chunk matrices of 4 columns, each with a 4-word salt (a leaf of 32 words)
constexpr uint32_t MAX_MATS = 4, MAX_SALT = 4, MAX_LEAF = MAX_MATS * (4 + MAX_SALT);

// The parameter gates both verifiers share, as the provers' inits state them: nothing below may shift by >= 32 or leave the two-adic
// subgroup.  log_height: the committed trace's log height; the two messages are each wire format's own.
int check_parameters(int hash, uint32_t log_n, uint32_t log_height, const FriParams& fp, std::string* why, const char* lde_msg,
                     const char* lfp_msg) {
    if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return reject(why, -1, "unknown hash configuration");
    if (log_n < 1 || fp.log_blowup < 1 || log_height + fp.log_blowup > bb::TWO_ADICITY) return reject(why, -1, lde_msg);
    if (fp.log_final_poly_len >= log_height) return reject(why, -1, lfp_msg);
    if (fp.proof_of_work_bits > 30) return reject(why, -1, "bad parameters: proof_of_work_bits too large");
    if (fp.num_queries == 0) return reject(why, -1, "bad parameters: num_queries must be positive");
    return 0;
}

// Reads one BatchOpening — n_mats (width, values) pairs, then one salt per matrix when salt_words > 0, then the sibling path — and
// assembles the leaf row it hashes to: m0 || s0 || m1 || s1 ...  False on a shape mismatch (the caller checks the path: verify_opening).
bool read_opening(Reader& rd, int hash, uint32_t n_mats, const uint32_t* widths, uint32_t salt_words, unsigned depth, uint32_t* vals,
                  uint32_t* leaf, size_t* leaf_len, uint32_t* path) {
    uint32_t salts[MAX_MATS * MAX_SALT];
    if (rd.u32() != n_mats) return false;
    size_t off = 0;
    for (uint32_t m = 0; m < n_mats; m++) {
        if (rd.u32() != widths[m]) return false;
        rd.felts(vals + off, widths[m]);
        off += widths[m];
    }
    if (salt_words)
        for (uint32_t m = 0; m < n_mats; m++) {
            if (rd.u32() != salt_words) return false;
            rd.felts(salts + m * salt_words, salt_words);
        }
    if (rd.u32() != depth) return false;
    rd.digests(hash, path, depth);
    size_t p = 0;
    off = 0;
    for (uint32_t m = 0; m < n_mats; m++) {
        memcpy(leaf + p, vals + off, widths[m] * 4); p += widths[m]; off += widths[m];
        memcpy(leaf + p, salts + m * salt_words, salt_words * 4); p += salt_words;
    }
    *leaf_len = p;
    return true;
}

// The FRI half both wire formats share (TwoAdicFriPcs / HidingFriPcs with p3_fri::verifier): the commit phase, the final polynomial and
// the proof of work, and per query the walk from the reduced opening down to the final polynomial.  salt_words: the salt of an FRI
// leaf (0: the plain MMCS).  Each step returns 0 or its reject code, the reason in *why.
struct FriCheck {
    int hash;
    FriParams fp;
    uint32_t log_big, salt_words;
    std::string* why;
    uint32_t n_rounds = 0;
    std::vector<uint32_t> froots;
    std::vector<Ext> betas, fpoly;

    // the commitments of the rounds, observed with their betas sampled; the query count
    int commit_phase(Reader& rd, Challenger& ch) {
        n_rounds = rd.u32();
        if (rd.bad || n_rounds != log_big - fp.log_blowup - fp.log_final_poly_len) return reject(why, 5, "commit phase length");
        froots.resize((size_t)n_rounds * 8);
        betas.resize(n_rounds);
        rd.digests(hash, froots.data(), n_rounds);
        for (uint32_t r = 0; r < n_rounds; r++) { ch.observe_digest(&froots[(size_t)r * 8]); betas[r] = ch.sample_ext(); }
        if (rd.u32() != fp.num_queries) return reject(why, 6, "query count");
        return 0;
    }
    // from the final polynomial to the end of the proof: the final polynomial, the witness and its check
    int final_poly(Reader& rd, Challenger& ch) {
        const uint32_t fpl = rd.u32();
        if (rd.bad || fpl != (1u << fp.log_final_poly_len)) return reject(why, 7, "final polynomial length");
        fpoly.resize(fpl);
        for (auto& e : fpoly) { e = rd.ext(); ch.observe_ext(e); }
        const uint32_t witness = rd.felt();
        if (rd.bad || rd.pos != rd.len) return reject(why, 8, "trailing or missing bytes");
        ch.observe(witness);
        if (ch.sample_bits(fp.proof_of_work_bits) != 0) return reject(why, 11, "InvalidPowWitness");
        return 0;
    }
    // one query's FRI walk: per round the sibling, its salt, the path to the round's root and the fold; then the final polynomial at
    // the point the walk ends on against the folded value.  rolls (mixed heights: pcs_verify_mixed; empty for everyone else): the
    // reduced opening ro_c of every shorter class by its log_big_c, added as beta^2 ro_c right after the fold that reaches 2^log_big_c
    int query(Reader& rd, size_t index, Ext folded, uint32_t* path, const std::vector<std::pair<uint32_t, Ext>>& rolls = {}) {
        if (rd.u32() != n_rounds) return reject(why, 12, "query shape");
        size_t idx = index;
        for (uint32_t r = 0; r < n_rounds; r++) {
            const uint32_t lfh = log_big - 1 - r;
            Ext sib = rd.ext();
            uint32_t row[8 + MAX_SALT];
            if (salt_words) {
                if (rd.u32() != salt_words) return reject(why, 12, "query shape");
                rd.felts(row + 8, salt_words);
            }
            if (rd.u32() != lfh) return reject(why, 12, "query shape");
            rd.digests(hash, path, lfh);
            Ext ev[2];
            ev[idx & 1] = folded; ev[(idx & 1) ^ 1] = sib;
            const size_t pair = idx >> 1;
            memcpy(row, ev[0].c, 16); memcpy(row + 4, ev[1].c, 16);
            if (!verify_opening(hash, &froots[(size_t)r * 8], pair, row, 8 + salt_words, path, lfh)) return reject(why, 14, "FRI layer opening");
            const uint32_t s = bb::pow(bb::two_adic_generator(lfh + 1), rev_bits_host(pair, lfh));
            Ext num = bb::mul(bb::sub(betas[r], bb::ext_from_base(s)), bb::sub(ev[1], ev[0]));
            folded = bb::add(ev[0], bb::scale(num, bb::inv(bb::sub(bb::neg(s), s))));
            for (const auto& rl : rolls)
                if (rl.first == lfh) folded = bb::add(folded, bb::mul(bb::sqr(betas[r]), rl.second));
            idx = pair;
        }
        const uint32_t lfinal = fp.log_blowup + fp.log_final_poly_len;
        const uint32_t xf = bb::pow(bb::two_adic_generator(lfinal), rev_bits_host(idx, lfinal));
        Ext evf = bb::ext_zero();
        for (size_t i = fpoly.size(); i-- > 0;) evf = bb::add(bb::scale(evf, xf), fpoly[i]);
        if (rd.bad) return reject(why, 9, "truncated proof");
        if (!bb::eq(evf, folded)) return reject(why, 15, "FinalPolyMismatch");
        return 0;
    }
};

}  // namespace

// check_parameters for either wire format, with that format's own messages (the device verifier refuses what these refuse)
int verify_check_parameters(int hash, bool hiding, uint32_t log_n, const FriParams& fp, std::string* why) {
    if (hiding)
        return check_parameters(hash, log_n, log_n + 1, fp, why, "bad parameters: LDE height outside the two-adic subgroup",
                                "bad parameters: log_final_poly_len must be below the randomized trace's log height");
    return check_parameters(hash, log_n, log_n, fp, why, "bad parameters: LDE height outside [2^2, 2^27]",
                            "bad parameters: log_final_poly_len must be below the trace's log height");
}

// 0 = accept; otherwise a positive code naming the failed check (same numbering as the error strings below).
int verify_fib_air(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n,
                   const FriParams& fp, std::string* why, int hash) {
    if (int rc = verify_check_parameters(hash, false, log_n, fp, why)) return rc;
    Reader rd{proof, len};
    const uint32_t log_big = log_n + fp.log_blowup;
    const uint64_t n = 1ull << log_n;
    const uint32_t gen = bb::to_monty(bb::GEN);
    if (rd.u32() != 0x42463350u || rd.u32() != 1) return reject(why, 1, "bad header");
    if (rd.u32() != log_n) return reject(why, 2, "degree_bits mismatch");
    uint32_t root_t[8], root_q[8];
    rd.digests(hash, root_t, 1); rd.digests(hash, root_q, 1);
    Ext t_loc[2], t_nxt[2], q_z[4];
    if (rd.u32() != 2) return reject(why, 3, "opened values shape");
    for (auto& e : t_loc) e = rd.ext();
    if (rd.u32() != 2) return reject(why, 3, "opened values shape");
    for (auto& e : t_nxt) e = rd.ext();
    if (rd.u32() != 1 || rd.u32() != 4) return reject(why, 3, "opened values shape");
    for (auto& e : q_z) e = rd.ext();
    if (rd.bad) return reject(why, 4, "truncated proof");
    uint32_t pis[3] = {bb::to_monty((uint32_t)(a_pub % bb::P)), bb::to_monty((uint32_t)(b_pub % bb::P)), bb::to_monty((uint32_t)(x_pub % bb::P))};
    Challenger ch(hash);
    ch.observe(bb::to_monty(log_n)); ch.observe(bb::to_monty(log_n));
    ch.observe_digest(root_t); ch.observe_n(pis, 3);
    Ext alpha = ch.sample_ext();
    ch.observe_digest(root_q);
    Ext zeta = ch.sample_ext();
    const uint32_t g_n = bb::two_adic_generator(log_n);
    Ext zeta_next = bb::scale(zeta, g_n);
    {   // constraints at zeta (FibonacciAir, fib_air.rs:232-264) against the opened quotient
        Ext zh = bb::sub(bb::pow(zeta, n), bb::ext_one());
        Ext ginv = bb::ext_from_base(bb::inv(g_n));
        Ext first = bb::mul(zh, bb::inv(bb::sub(zeta, bb::ext_one())));
        Ext last = bb::mul(zh, bb::inv(bb::sub(zeta, ginv)));
        Ext trans = bb::sub(zeta, ginv);
        Ext c[5] = {bb::mul(first, bb::sub(t_loc[0], bb::ext_from_base(pis[0]))), bb::mul(first, bb::sub(t_loc[1], bb::ext_from_base(pis[1]))),
                    bb::mul(trans, bb::sub(t_loc[1], t_nxt[0])), bb::mul(trans, bb::sub(bb::add(t_loc[0], t_loc[1]), t_nxt[1])),
                    bb::mul(last, bb::sub(t_loc[1], bb::ext_from_base(pis[2])))};
        Ext folded = bb::ext_zero();
        for (auto& ck : c) folded = bb::add(bb::mul(folded, alpha), ck);
        Ext quot = bb::ext_zero();
        for (int e = 0; e < 4; e++) { Ext be = bb::ext_zero(); be.c[e] = bb::ONE; quot = bb::add(quot, bb::mul(be, q_z[e])); }
        if (!bb::eq(bb::mul(folded, bb::inv(zh)), quot)) return reject(why, 10, "OodEvaluationMismatch");
    }
    for (auto& e : t_loc) ch.observe_ext(e);
    for (auto& e : t_nxt) ch.observe_ext(e);
    for (auto& e : q_z) ch.observe_ext(e);
    Ext al = ch.sample_ext();
    Ext alp[8]; alp[0] = bb::ext_one();
    for (int k = 1; k < 8; k++) alp[k] = bb::mul(alp[k - 1], al);
    FriCheck fri{hash, fp, log_big, 0, why};
    if (int rc = fri.commit_phase(rd, ch)) return rc;
    const size_t qstart = rd.pos;
    for (uint32_t q = 0; q < fp.num_queries && !rd.bad; q++) {  // skip to the final polynomial
        if (rd.u32() != 2) rd.bad = true;
        for (int m = 0; m < 2 && !rd.bad; m++) { rd.u32(); uint32_t w = rd.u32(); rd.pos += 4 * (size_t)w; uint32_t pl = rd.u32(); rd.pos += 32 * (size_t)pl; }
        uint32_t nr = rd.u32();
        for (uint32_t r = 0; r < nr && !rd.bad; r++) { rd.pos += 16; uint32_t pl = rd.u32(); rd.pos += 32 * (size_t)pl; }
    }
    if (int rc = fri.final_poly(rd, ch)) return rc;
    rd.pos = qstart;
    std::vector<uint32_t> path((size_t)(log_big + 1) * 8);
    const uint32_t w_t = 2, w_q = 4;
    for (uint32_t q = 0; q < fp.num_queries; q++) {
        const size_t index = ch.sample_bits(log_big);
        uint32_t trow[2], qrow[4], leaf[MAX_LEAF];
        size_t leaf_len = 0;
        if (rd.u32() != 2) return reject(why, 12, "query shape");  // one BatchOpening per commitment round
        if (!read_opening(rd, hash, 1, &w_t, 0, log_big, trow, leaf, &leaf_len, path.data())) return reject(why, 12, "query shape");
        if (!verify_opening(hash, root_t, index, leaf, leaf_len, path.data(), log_big)) return reject(why, 13, "trace opening");
        if (!read_opening(rd, hash, 1, &w_q, 0, log_big, qrow, leaf, &leaf_len, path.data())) return reject(why, 12, "query shape");
        if (!verify_opening(hash, root_q, index, leaf, leaf_len, path.data(), log_big)) return reject(why, 13, "quotient opening");
        const uint32_t xi = bb::mul(gen, bb::pow(bb::two_adic_generator(log_big), rev_bits_host(index, log_big)));
        Ext d0 = bb::inv(bb::sub(zeta, bb::ext_from_base(xi))), d1 = bb::inv(bb::sub(zeta_next, bb::ext_from_base(xi)));
        Ext ro = bb::ext_zero();
        int k = 0;
        for (int j = 0; j < 2; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(t_loc[j], bb::ext_from_base(trow[j])), d0)));
        for (int j = 0; j < 2; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(t_nxt[j], bb::ext_from_base(trow[j])), d1)));
        for (int j = 0; j < 4; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(q_z[j], bb::ext_from_base(qrow[j])), d0)));
        if (int rc = fri.query(rd, index, ro, path.data())) return rc;
    }
    if (why) why->clear();
    return 0;
}


// ---- verifier of HIDING proofs (wire format version 2; prover_hiding.hip.inc): p3_uni_stark::verify with SC::Pcs::ZK over
// HidingFriPcs + MerkleTreeHidingMmcs as the reference configures them (native/src/fib_air.rs:40-72).  Leaves are the
// opened values followed by their salts, matrix by matrix; the quotient is recomposed from the four blinded chunks
// (the blinding cancels in sum_c zps_c(zeta) chunk_c(zeta)); every opened column, the random ones included, enters the
// FRI batch.  [UPSTREAM-RECALL] in structure, parity unpinned.
namespace {
constexpr uint32_t VH_NRC = 4, VH_SALT = 4, VH_D = 4, VH_TW = 2 + VH_NRC, VH_RW = VH_NRC + VH_D, VH_CH = 4;
constexpr uint32_t VH_OPEN = VH_RW + 2 * VH_TW + VH_CH * VH_D;
static_assert(VH_CH <= MAX_MATS && VH_SALT <= MAX_SALT && VH_CH * (VH_D + VH_SALT) <= MAX_LEAF && VH_RW + VH_SALT <= MAX_LEAF,
              "hiding openings fit the opening reader's buffers");
}  // namespace

int verify_fib_air_hiding(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n,
                          const FriParams& fp, std::string* why, int hash) {
    const uint32_t log_ext = log_n + 1, log_big = log_ext + fp.log_blowup;
    if (int rc = verify_check_parameters(hash, true, log_n, fp, why)) return rc;
    Reader rd{proof, len};
    const uint64_t h = 1ull << log_n;
    const uint32_t gen = bb::to_monty(bb::GEN);
    if (rd.u32() != 0x42463350u || rd.u32() != 2) return reject(why, 1, "bad header");
    if (rd.u32() != log_n) return reject(why, 2, "degree_bits mismatch");
    uint32_t root_t[8], root_q[8], root_r[8];
    rd.digests(hash, root_t, 1); rd.digests(hash, root_q, 1); rd.digests(hash, root_r, 1);
    Ext opened[VH_OPEN];  // random (8), trace @ zeta (6), trace @ zeta g (6), chunks (4 x 4)
    {
        uint32_t k = 0;
        if (rd.u32() != VH_RW) return reject(why, 3, "opened values shape");
        for (uint32_t i = 0; i < VH_RW; i++) opened[k++] = rd.ext();
        if (rd.u32() != VH_TW) return reject(why, 3, "opened values shape");
        for (uint32_t i = 0; i < VH_TW; i++) opened[k++] = rd.ext();
        if (rd.u32() != VH_TW) return reject(why, 3, "opened values shape");
        for (uint32_t i = 0; i < VH_TW; i++) opened[k++] = rd.ext();
        if (rd.u32() != VH_CH) return reject(why, 3, "opened values shape");
        for (uint32_t c = 0; c < VH_CH; c++) {
            if (rd.u32() != VH_D) return reject(why, 3, "opened values shape");
            for (uint32_t i = 0; i < VH_D; i++) opened[k++] = rd.ext();
        }
    }
    if (rd.bad) return reject(why, 4, "truncated proof");
    const Ext* t_z = opened + VH_RW;
    const Ext* t_zn = t_z + VH_TW;
    const Ext* q_z = t_zn + VH_TW;
    uint32_t pis[3] = {bb::to_monty((uint32_t)(a_pub % bb::P)), bb::to_monty((uint32_t)(b_pub % bb::P)), bb::to_monty((uint32_t)(x_pub % bb::P))};
    Challenger ch(hash);
    ch.observe(bb::to_monty(log_ext)); ch.observe(bb::to_monty(log_n));
    ch.observe_digest(root_t); ch.observe_n(pis, 3);
    Ext alpha = ch.sample_ext();
    ch.observe_digest(root_q);
    ch.observe_digest(root_r);
    Ext zeta = ch.sample_ext();
    const uint32_t g_h = bb::two_adic_generator(log_n);
    Ext zeta_next = bb::scale(zeta, g_h);
    {   // constraints at zeta against the quotient recomposed from the blinded chunks
        Ext zh_pow = bb::pow(zeta, h);
        Ext zh = bb::sub(zh_pow, bb::ext_one());
        Ext ginv = bb::ext_from_base(bb::inv(g_h));
        Ext first = bb::mul(zh, bb::inv(bb::sub(zeta, bb::ext_one())));
        Ext last = bb::mul(zh, bb::inv(bb::sub(zeta, ginv)));
        Ext trans = bb::sub(zeta, ginv);
        Ext c[5] = {bb::mul(first, bb::sub(t_z[0], bb::ext_from_base(pis[0]))), bb::mul(first, bb::sub(t_z[1], bb::ext_from_base(pis[1]))),
                    bb::mul(trans, bb::sub(t_z[1], t_zn[0])), bb::mul(trans, bb::sub(bb::add(t_z[0], t_z[1]), t_zn[1])),
                    bb::mul(last, bb::sub(t_z[1], bb::ext_from_base(pis[2])))};
        Ext folded = bb::ext_zero();
        for (auto& ck : c) folded = bb::add(bb::mul(folded, alpha), ck);
        // chunk cosets D_c = s_c <g_h>: s_c^h = GENERATOR^h w4^c; zps_c(zeta) = prod_{j != c} (zeta^h - s_j^h) / (s_c^h - s_j^h)
        uint32_t sh[VH_CH];
        { uint32_t gh = bb::pow(gen, h), w4 = bb::two_adic_generator(2), p = bb::ONE;
          for (uint32_t k = 0; k < VH_CH; k++) { sh[k] = bb::mul(gh, p); p = bb::mul(p, w4); } }
        Ext quot = bb::ext_zero();
        for (uint32_t ci = 0; ci < VH_CH; ci++) {
            uint32_t kc = bb::ONE;
            Ext zp = bb::ext_one();
            for (uint32_t j = 0; j < VH_CH; j++)
                if (j != ci) { kc = bb::mul(kc, bb::sub(sh[ci], sh[j])); zp = bb::mul(zp, bb::sub(zh_pow, bb::ext_from_base(sh[j]))); }
            zp = bb::scale(zp, bb::inv(kc));
            Ext v = bb::ext_zero();
            for (int e = 0; e < 4; e++) { Ext be = bb::ext_zero(); be.c[e] = bb::ONE; v = bb::add(v, bb::mul(be, q_z[ci * VH_D + e])); }
            quot = bb::add(quot, bb::mul(zp, v));
        }
        if (!bb::eq(bb::mul(folded, bb::inv(zh)), quot)) return reject(why, 10, "OodEvaluationMismatch");
    }
    for (uint32_t k = 0; k < VH_OPEN; k++) ch.observe_ext(opened[k]);
    Ext al = ch.sample_ext();
    Ext alp[VH_OPEN]; alp[0] = bb::ext_one();
    for (uint32_t k = 1; k < VH_OPEN; k++) alp[k] = bb::mul(alp[k - 1], al);
    FriCheck fri{hash, fp, log_big, VH_SALT, why};
    if (int rc = fri.commit_phase(rd, ch)) return rc;
    const size_t qstart = rd.pos;
    {   // every query has the same length: skip to the final polynomial
        const uint32_t nm[3] = {1, 1, VH_CH}, wsum[3] = {VH_RW, VH_TW, VH_CH * VH_D};
        size_t qlen = 4 + 4;
        for (int k = 0; k < 3; k++) qlen += 4 + 4 * (size_t)(nm[k] + wsum[k]) + 4 * (size_t)nm[k] * (1 + VH_SALT) + 4 + 32 * (size_t)log_big;
        for (uint32_t r = 0; r < fri.n_rounds; r++) qlen += 16 + 4 + 4 * VH_SALT + 4 + 32 * (size_t)(log_big - 1 - r);
        rd.pos += qlen * fp.num_queries;
        if (rd.pos > len) rd.bad = true;
    }
    if (int rc = fri.final_poly(rd, ch)) return rc;
    rd.pos = qstart;
    std::vector<uint32_t> path((size_t)(log_big + 1) * 8);
    const uint32_t w_r[1] = {VH_RW}, w_t[1] = {VH_TW}, w_q[VH_CH] = {VH_D, VH_D, VH_D, VH_D};
    for (uint32_t q = 0; q < fp.num_queries; q++) {
        const size_t index = ch.sample_bits(log_big);
        uint32_t rrow[VH_RW], trow[VH_TW], qrow[VH_CH * VH_D];
        // one salted BatchOpening: a truncated or non-canonical read rejects before the path is hashed
        auto open = [&](const uint32_t* root, uint32_t n_mats, const uint32_t* widths, uint32_t* vals, const char* what) -> int {
            uint32_t leaf[MAX_LEAF];
            size_t leaf_len = 0;
            if (!read_opening(rd, hash, n_mats, widths, VH_SALT, log_big, vals, leaf, &leaf_len, path.data())) return reject(why, 12, what);
            if (rd.bad) return reject(why, 9, what);
            if (!verify_opening(hash, root, index, leaf, leaf_len, path.data(), log_big)) return reject(why, 13, what);
            return 0;
        };
        if (rd.u32() != 3) return reject(why, 12, "query shape");
        if (int rc = open(root_r, 1, w_r, rrow, "randomization opening")) return rc;
        if (int rc = open(root_t, 1, w_t, trow, "trace opening")) return rc;
        if (int rc = open(root_q, VH_CH, w_q, qrow, "quotient opening")) return rc;
        const uint32_t xi = bb::mul(gen, bb::pow(bb::two_adic_generator(log_big), rev_bits_host(index, log_big)));
        Ext d0 = bb::inv(bb::sub(zeta, bb::ext_from_base(xi))), d1 = bb::inv(bb::sub(zeta_next, bb::ext_from_base(xi)));
        Ext ro = bb::ext_zero();
        uint32_t k = 0;
        for (uint32_t j = 0; j < VH_RW; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(opened[k], bb::ext_from_base(rrow[j])), d0)));
        for (uint32_t j = 0; j < VH_TW; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(opened[k], bb::ext_from_base(trow[j])), d0)));
        for (uint32_t j = 0; j < VH_TW; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(opened[k], bb::ext_from_base(trow[j])), d1)));
        for (uint32_t j = 0; j < VH_CH * VH_D; j++, k++) ro = bb::add(ro, bb::mul(alp[k], bb::mul(bb::sub(opened[k], bb::ext_from_base(qrow[j])), d0)));
        if (int rc = fri.query(rd, index, ro, path.data())) return rc;
    }
    if (why) why->clear();
    return 0;
}

// ---- Pcs::verify of TwoAdicFriPcs over caller matrices (the prover half: pcs.hip.inc), host only.  The opened values arrive beside
// the proof bytes (the FriProof section of the wire format); the FRI half is FriCheck, shared with the two fib verifiers.  The
// transcript follows the test oracle's verifier (stark.c:216-294) generalised to the call's dimensions: opened values observed
// round -> matrix -> point -> column, alpha sampled, and per query
//   ro = sum over (matrix, point) pairs in that order, over columns c:  alpha^k (opened_k - row[c]) / (z - x),  k running on.
// Everything that is a function of the SHAPE comes from pcs_layout (pcs_layout.h), which the device batch verifier reads too: the gates on
// the arguments and their messages, each matrix's class, each round's tree depth, the classes with a point, each pair's matrix, place among
// the opened values and alpha exponent, where the final polynomial lies.  Left here: what depends on a member's VALUES (canonical points off
// the LDE coset, at most PCS_MAX_POINTS distinct; canonical opened values), the transcript, and the walk, which reads with Reader and
// compares every count, width, depth and salt-length word with the layout's: nothing is followed.
// hiding: HidingFriPcs::verify over the MerkleTreeHidingMmcs (the test oracle's hiding verifier, stark_hiding.c:380-457, generalised
// likewise): log_h is the CALLER's log height, each input BatchOpening carries its matrices' salts (read_opening; stark_hiding.c:300-322),
// each commit-phase opening its salt (FriCheck).  log_heights: mixed heights (pcs_layout.h), the tallest matrix's class starts the walk.
static int pcs_verify_any(int hash, bool hiding, const FriParams& fp, uint32_t log_h, const unsigned* log_heights, const uint32_t* roots,
                          const size_t* mats_per_round, const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points,
                          const uint32_t* opened, const uint8_t* proof, size_t len, Challenger* chal, std::string* why) {
    auto bad = [&](const std::string& msg) { if (why) *why = msg; return (int)ERR_BAD_ARG; };
    if (!roots || !mats_per_round || !widths || !points_per_mat || !points || !opened || !proof || !chal) return bad("pcs verify: null argument");
    // (a hash that is neither is pcs_layout's to name, as it was named before this: a challenger's kind is always one of the two)
    if ((hash == HASH_POSEIDON2 || hash == HASH_KECCAK) && chal->kind != hash) return bad("pcs verify: the challenger belongs to another hash configuration");
    PLayout L;
    const PcsShape shape{log_h, n_rounds, mats_per_round, widths, points_per_mat, 0, nullptr, log_heights};
    if (int rc = pcs_layout(hash, hiding, fp, shape, &L, nullptr, why)) return rc;
    const uint32_t log_big = L.log_big, salt_words = L.salt;
    const size_t total = L.total;
    Ext zs[PCS_MAX_POINTS];  // the distinct points; pair_slot: which of them a pair is opened at
    size_t n_points = 0, pi = 0;
    for (uint32_t r = 0; r < L.n_in; r++)
        for (uint32_t m = 0; m < L.nm[r]; m++)
            for (uint32_t p = 0; p < L.np[L.mat0[r] + m]; p++, pi++) {
                const uint32_t* z = points + 4 * pi;
                auto pw = [&] { return "pcs verify: round " + std::to_string(r) + " matrix " + std::to_string(m) + " point " + std::to_string(p); };
                for (int c = 0; c < 4; c++) if (z[c] >= bb::P) return bad(pw() + " is not a canonical field element");
                if (pcs_point_on_lde_coset(z, log_big)) return bad(pw() + " lies on the LDE coset GENERATOR * <g_big>");
                size_t k = 0;
                while (k < n_points && memcmp(zs[k].c, z, 16)) k++;
                if (k == n_points) {
                    if (n_points == PCS_MAX_POINTS) return bad(pw() + ": more than " + std::to_string(PCS_MAX_POINTS) + " distinct opening points");
                    memcpy(zs[n_points++].c, z, 16);
                }
                L.pair_slot[pi] = (uint8_t)k;
            }
    for (size_t i = 0; i < 4 * total; i++) if (opened[i] >= bb::P) return bad("pcs verify: opened value word " + std::to_string(i) + " is not a canonical field element");
    Challenger& ch = *chal;
    std::vector<Ext> ov(total), alp(total);
    for (size_t i = 0; i < total; i++) { memcpy(ov[i].c, opened + 4 * i, 16); ch.observe_ext(ov[i]); }
    const Ext al = ch.sample_ext();
    alp[0] = bb::ext_one();
    for (size_t k = 1; k < total; k++) alp[k] = bb::mul(alp[k - 1], al);
    Reader rd{proof, len};
    FriCheck fri{hash, fp, log_big, salt_words, why};
    if (int rc = fri.commit_phase(rd, ch)) return rc;
    const size_t qstart = rd.pos;
    // the final polynomial lies behind the queries: PLayout::fpl_off, in 64 bits (its own holds a proof of less than 2^32 bytes)
    const uint64_t fpl_off = (uint64_t)L.q_base + (uint64_t)L.q_len * L.nq;
    if (4 * fpl_off > len) return reject(why, 9, "truncated proof");
    rd.pos = (size_t)(4 * fpl_off);
    if (int rc = fri.final_poly(rd, ch)) return rc;
    rd.pos = qstart;
    static_assert(PCS_HIDING_MAX_MATS <= MAX_MATS && PCS_SALT <= MAX_SALT, "a salted round fits the opening reader's buffers");
    std::vector<uint32_t> path((size_t)(log_big + 1) * 8), row(L.row_words), leaf(L.row_words + PCS_MAX_MATS * salt_words);
    std::vector<size_t> hh(2 * PCS_MAX_MATS), lw(2 * PCS_MAX_MATS);
    size_t leaf_len = 0;
    const uint32_t gen = bb::to_monty(bb::GEN);
    // one reduced opening per class (by log_big_c); the tallest class is the walk's start, the others roll in
    Ext ro_c[bb::TWO_ADICITY + 1];
    uint32_t xi_c[bb::TWO_ADICITY + 1];
    std::vector<std::pair<uint32_t, Ext>> rolls;
    for (uint32_t q = 0; q < fp.num_queries; q++) {
        const size_t index = ch.sample_bits(log_big);
        for (uint32_t lb = 0; lb <= log_big; lb++) {
            if (!((L.class_mask >> lb) & 1u)) continue;
            ro_c[lb] = bb::ext_zero();
            xi_c[lb] = bb::mul(gen, bb::pow(bb::two_adic_generator(lb), rev_bits_host(index >> (log_big - lb), lb)));
        }
        if (rd.u32() != L.n_in) return reject(why, 12, "query shape");  // one BatchOpening per commitment round
        size_t pair = 0;
        for (uint32_t r = 0; r < L.n_in; r++) {
            const size_t nm = L.nm[r], m0 = L.mat0[r];
            const uint32_t log_big_r = L.log_big_r[r];  // this round's tree
            const size_t index_r = index >> (log_big - log_big_r);
            if (!read_opening(rd, hash, (uint32_t)nm, L.width + m0, salt_words, log_big_r, row.data(), leaf.data(), &leaf_len, path.data()))
                return reject(why, 12, "query shape");
            if (rd.bad) return reject(why, 9, "truncated proof");
            size_t n = 0;  // the salts as width-4 matrices, each behind its matrix
            for (size_t m = m0; m < m0 + nm; m++) {
                hh[n] = (size_t)1 << L.log_big_m[m]; lw[n++] = L.width[m];
                if (salt_words) { hh[n] = hh[n - 1]; lw[n++] = salt_words; }
            }
            if (mmcs_verify_batch(hash, roots + 8 * r, hh.data(), lw.data(), n, index_r, leaf.data(), path.data(), log_big_r, nullptr, false) != 0)
                return reject(why, 13, "input opening");
            size_t off = 0;
            for (size_t mi = m0; mi < m0 + nm; mi++) {
                const uint32_t lb = L.log_big_m[mi];
                for (uint32_t p = 0; p < L.np[mi]; p++, pair++) {
                    const Ext dz = bb::inv(bb::sub(zs[L.pair_slot[pair]], bb::ext_from_base(xi_c[lb])));
                    const Ext *a_k = &alp[L.pair_aoff[pair]], *o_k = &ov[L.pair_off[pair]];  // the pair's alpha powers (its class's counter) and opened values
                    for (size_t c = 0; c < L.width[mi]; c++)
                        ro_c[lb] = bb::add(ro_c[lb], bb::mul(a_k[c], bb::mul(bb::sub(o_k[c], bb::ext_from_base(row[off + c])), dz)));
                }
                off += L.width[mi];
            }
        }
        rolls.clear();
        for (uint32_t lb = 0; lb < log_big; lb++) if ((L.class_mask >> lb) & 1u) rolls.emplace_back(lb, ro_c[lb]);
        if (int rc = fri.query(rd, index, ro_c[log_big], path.data(), rolls)) return rc;
    }
    if (why) why->clear();
    return 0;
}

int pcs_verify(int hash, const FriParams& fp, uint32_t log_h, const uint32_t* roots, const size_t* mats_per_round, const size_t* widths,
               size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened, const uint8_t* proof,
               size_t len, Challenger* chal, std::string* why) {
    return pcs_verify_any(hash, false, fp, log_h, nullptr, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, chal, why);
}
int pcs_verify_mixed(int hash, const FriParams& fp, const unsigned* log_heights, const uint32_t* roots, const size_t* mats_per_round,
                     const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened,
                     const uint8_t* proof, size_t len, Challenger* chal, std::string* why) {
    if (!log_heights) { if (why) *why = "pcs verify: null argument"; return (int)ERR_BAD_ARG; }
    return pcs_verify_any(hash, false, fp, 0, log_heights, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, chal, why);
}
int pcs_verify_hiding(int hash, const FriParams& fp, uint32_t log_h, const uint32_t* roots, const size_t* mats_per_round, const size_t* widths,
                      size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened, const uint8_t* proof,
                      size_t len, Challenger* chal, std::string* why) {
    if (log_h < 1 || log_h >= bb::TWO_ADICITY) {
        if (why) *why = "pcs verify: log_h must be in [1, " + std::to_string(bb::TWO_ADICITY - 1) + "] (the caller's log height; the committed polynomials have degree < 2^(log_h + 1))";
        return (int)ERR_BAD_ARG;
    }
    return pcs_verify_any(hash, true, fp, log_h, nullptr, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, chal, why);
}

}  // namespace p3
