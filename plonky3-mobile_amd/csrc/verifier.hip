// fib_air verifier (host only): p3_uni_stark::verify + TwoAdicFriPcs::verify + p3_fri::verifier for FibonacciAir,
// the second half of the reference's run_fib_air_zk (native/src/fib_air.rs:70-72: prove, then verify, then
// "fib_air zk ok").  Verification is a few thousand permutations — it is the verifier's role, runs on the host
// exactly as in the reference, and is not a fallback for any device kernel.  Written against the wire format
// of prover.hip; independent of the test oracle.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bb31.hip.h"
#include "challenger.h"
#include "common.h"
#include "fib_format.h"
#include "mmcs.h"
#include "ood.hip.h"
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
// assembles the leaf row it hashes to: m0 || s0 || m1 || s1 ...  False on a shape mismatch (the caller checks the path).
bool read_opening(Reader& rd, int hash, uint32_t n_mats, const uint32_t* widths, uint32_t salt_words, unsigned depth, uint32_t* vals,
                  uint32_t* leaf, size_t* leaf_len, uint32_t* path) {
    uint32_t salts[PCS_HIDING_MAX_MATS * PCS_SALT];  // a salted round has at most PCS_HIDING_MAX_MATS matrices (pcs_layout's gate)
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
            uint32_t row[8 + PCS_SALT];
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

// (Dialect: fib_format.h) what pcs_verify_any's members answer
constexpr Dialect DIALECT_PCS{{}, 0, true, Dialect::LAYOUT_CHECKED};

// Wire format 1 finds its final polynomial by FOLLOWING the queries' count words (widths, path lengths, round counts), as its first
// verifier did, not from the shape: a tampered count moves the final polynomial and the proof is a 7 (or 8) there, before the query walk
// compares that word with the layout and would say 12.  One matrix a round and no salts: format 1's shape.  A count may carry pos far past
// len; the next u32 flags that (pos is 64 bits: 2^32 counts of 2^37 bytes do not wrap it).
void skip_queries_by_counts(Reader& rd, const PLayout& L) {
    for (uint32_t q = 0; q < L.nq && !rd.bad; q++) {
        if (rd.u32() != L.n_in) rd.bad = true;
        for (uint32_t r = 0; r < L.n_in && !rd.bad; r++) { rd.u32(); uint32_t w = rd.u32(); rd.pos += 4 * (size_t)w; uint32_t pl = rd.u32(); rd.pos += 32 * (size_t)pl; }
        uint32_t nr = rd.u32();
        for (uint32_t r = 0; r < nr && !rd.bad; r++) { rd.pos += 16; uint32_t pl = rd.u32(); rd.pos += 32 * (size_t)pl; }
    }
}

// Pcs::verify behind the gates: the walk over a finished layout.  zs: the distinct points (L.pair_slot indexes them), ov: the L.total
// opened values in observation order, roots: one per input round, proof: the FriProof section.  The transcript follows the test oracle's
// verifier (stark.c:216-294) generalised to the layout: opened values observed round -> matrix -> point -> column, alpha sampled, and per query
//   ro = sum over (matrix, point) pairs in that order, over columns c:  alpha^k (opened_k - row[c]) / (z - x),  k running on
// per class (by log_big_c); the tallest class starts the FRI walk, the others roll in.  Every count, width, depth and salt-length word is
// compared with the layout's: nothing is followed (but Dialect::COUNTS).  Hiding: each input BatchOpening carries its matrices' salts
// (read_opening; stark_hiding.c:300-322, 380-457), each commit-phase opening its salt (FriCheck).
int pcs_walk(const PLayout& L, const FriParams& fp, const Dialect& d, const Ext* zs, const Ext* ov, const uint32_t* roots, const uint8_t* proof,
             size_t len, Challenger& ch, std::string* why) {
    const uint32_t log_big = L.log_big, salt_words = L.salt;
    const size_t total = L.total;
    auto at_round = [&](int code, uint32_t r, const char* general) { return reject(why, code, (d.named >> code) & 1u ? d.round_name[r] : general); };
    std::vector<Ext> alp(total);
    for (size_t i = 0; i < total; i++) ch.observe_ext(ov[i]);
    const Ext al = ch.sample_ext();
    alp[0] = bb::ext_one();
    for (size_t k = 1; k < total; k++) alp[k] = bb::mul(alp[k - 1], al);
    Reader rd{proof, len};
    FriCheck fri{L.hash, fp, log_big, salt_words, why};
    if (int rc = fri.commit_phase(rd, ch)) return rc;
    const size_t qstart = rd.pos;
    if (d.final_at == Dialect::COUNTS) skip_queries_by_counts(rd, L);
    else {  // behind the queries: PLayout::fpl_off, in 64 bits (its own holds a proof of less than 2^32 bytes)
        const uint64_t fpl_off = (uint64_t)L.q_base + (uint64_t)L.q_len * L.nq;
        if (d.final_at == Dialect::LAYOUT_CHECKED && 4 * fpl_off > len) return reject(why, 9, "truncated proof");
        rd.pos = (size_t)(4 * fpl_off);
    }
    if (int rc = fri.final_poly(rd, ch)) return rc;
    rd.pos = qstart;
    std::vector<uint32_t> path((size_t)(log_big + 1) * 8), row(L.row_words), leaf(L.row_words + PCS_MAX_MATS * salt_words);
    std::vector<size_t> hh(2 * PCS_MAX_MATS), lw(2 * PCS_MAX_MATS);
    size_t leaf_len = 0;
    const uint32_t gen = bb::to_monty(bb::GEN);
    // per class (by log_big_c): its reduced opening, its point x, and 1 / (z - x) of each distinct point, inverted when a pair first asks
    Ext ro_c[bb::TWO_ADICITY + 1], dz_c[bb::TWO_ADICITY + 1][PCS_MAX_POINTS];
    uint32_t xi_c[bb::TWO_ADICITY + 1], have_c[bb::TWO_ADICITY + 1];
    std::vector<std::pair<uint32_t, Ext>> rolls;
    for (uint32_t q = 0; q < fp.num_queries; q++) {
        const size_t index = ch.sample_bits(log_big);
        for (uint32_t lb = 0; lb <= log_big; lb++) {
            if (!((L.class_mask >> lb) & 1u)) continue;
            ro_c[lb] = bb::ext_zero();
            have_c[lb] = 0;
            xi_c[lb] = bb::mul(gen, bb::pow(bb::two_adic_generator(lb), rev_bits_host(index >> (log_big - lb), lb)));
        }
        if (rd.u32() != L.n_in) return reject(why, 12, "query shape");  // one BatchOpening per commitment round
        size_t pair = 0;
        for (uint32_t r = 0; r < L.n_in; r++) {
            const size_t nm = L.nm[r], m0 = L.mat0[r];
            const uint32_t log_big_r = L.log_big_r[r];  // this round's tree
            const size_t index_r = index >> (log_big - log_big_r);
            if (!read_opening(rd, L.hash, (uint32_t)nm, L.width + m0, salt_words, log_big_r, row.data(), leaf.data(), &leaf_len, path.data()))
                return at_round(12, r, "query shape");
            if (d.stop_on_flag && rd.bad) return at_round(9, r, "truncated proof");
            size_t n = 0;  // the salts as width-4 matrices, each behind its matrix
            for (size_t m = m0; m < m0 + nm; m++) {
                hh[n] = (size_t)1 << L.log_big_m[m]; lw[n++] = L.width[m];
                if (salt_words) { hh[n] = hh[n - 1]; lw[n++] = salt_words; }
            }
            if (mmcs_verify_batch(L.hash, roots + 8 * r, hh.data(), lw.data(), n, index_r, leaf.data(), path.data(), log_big_r, nullptr, false) != 0)
                return at_round(13, r, "input opening");
            size_t off = 0;
            for (size_t mi = m0; mi < m0 + nm; mi++) {
                const uint32_t lb = L.log_big_m[mi];
                for (uint32_t p = 0; p < L.np[mi]; p++, pair++) {
                    const uint32_t s = L.pair_slot[pair];
                    if (!((have_c[lb] >> s) & 1u)) { dz_c[lb][s] = bb::inv(bb::sub(zs[s], bb::ext_from_base(xi_c[lb]))); have_c[lb] |= 1u << s; }
                    const Ext dz = dz_c[lb][s];
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

}  // namespace

// check_parameters for either wire format, with that format's own messages (the device verifier refuses what these refuse)
int verify_check_parameters(int hash, bool hiding, uint32_t log_n, const FriParams& fp, std::string* why) {
    if (hiding)
        return check_parameters(hash, log_n, log_n + 1, fp, why, "bad parameters: LDE height outside the two-adic subgroup",
                                "bad parameters: log_final_poly_len must be below the randomized trace's log height");
    return check_parameters(hash, log_n, log_n, fp, why, "bad parameters: LDE height outside [2^2, 2^27]",
                            "bad parameters: log_final_poly_len must be below the trace's log height");
}

// ---- the fib_air verifiers: p3_uni_stark::verify for FibonacciAir over TwoAdicFriPcs (wire format 1, prover.hip) and, with SC::Pcs::ZK,
// over HidingFriPcs + MerkleTreeHidingMmcs as the reference configures them (wire format 2, prover_hiding.hip.inc;
// native/src/fib_air.rs:40-72; [UPSTREAM-RECALL] in structure, parity unpinned).  A fib_air proof is a PCS proof of a fixed shape behind a
// header: magic, version, log_n, the roots, the opened values.  What the two formats do not share is a table (fib_format.h); verify_fib does
// the rest.
namespace {
// 0 = accept; otherwise a positive code naming the failed check (1-4 the header, 10 the constraints, the others pcs_walk's and FriCheck's).
int verify_fib(const FibFormat& f, const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n,
               const FriParams& fp, std::string* why, int hash) {
    if (int rc = verify_check_parameters(hash, f.hiding, log_n, fp, why)) return rc;
    // pcs_layout's gates are verify_check_parameters' over again and refuse nothing it admits (before the first byte is read, so that
    // any bytes show it: test_no_pcs_refusal_leaks_out_of_a_fib_verifier)
    PLayout L;
    if (int rc = pcs_layout(hash, f.hiding, fp, fib_pcs_shape(f, log_n), &L, nullptr, why)) return rc;
    Reader rd{proof, len};
    if (rd.u32() != PROOF_MAGIC || rd.u32() != f.version) return reject(why, 1, "bad header");
    if (rd.u32() != log_n) return reject(why, 2, "degree_bits mismatch");
    uint32_t hdr_roots[FIB_MAX_ROUNDS][8], roots[FIB_MAX_ROUNDS * 8];
    for (uint32_t r = 0; r < f.n_rounds; r++) rd.digests(hash, hdr_roots[r], 1);
    Ext opened[FIB_MAX_OPENED];
    uint32_t k = 0;
    for (const int* g = f.grammar; *g; g++) {
        if (rd.u32() != (uint32_t)std::abs(*g)) return reject(why, 3, "opened values shape");
        for (int i = 0; i < *g; i++) opened[k++] = rd.ext();
    }
    if (rd.bad) return reject(why, 4, "truncated proof");
    const uint32_t pis[3] = {bb::to_monty((uint32_t)(a_pub % bb::P)), bb::to_monty((uint32_t)(b_pub % bb::P)), bb::to_monty((uint32_t)(x_pub % bb::P))};
    Challenger ch(hash);
    ch.observe(bb::to_monty(log_n + f.hiding)); ch.observe(bb::to_monty(log_n));
    ch.observe_digest(hdr_roots[0]); ch.observe_n(pis, 3);
    const Ext alpha = ch.sample_ext();
    for (uint32_t r = 1; r < f.n_rounds; r++) ch.observe_digest(hdr_roots[r]);
    const Ext zeta = ch.sample_ext();
    {   // the FibonacciAir constraints at zeta, folded with alpha, against the quotient recomposed from its chunks (ood.hip.h)
        OodDomain dom;
        ood_domain(log_n, f.log_chunks, &dom);
        Ext first, last, trans, zn, zh;
        ood_selectors(zeta, log_n, dom.g_n_inv, first, last, trans, zn, zh);
        const Ext folded = fib_constraints_folded(opened[f.t_loc].c, opened[f.t_nxt].c, pis, first, last, trans, alpha);
        if (!bb::eq(bb::mul(folded, bb::inv(zh)), ood_quotient(dom, 1u << f.log_chunks, zn, opened[f.chunks].c)))
            return reject(why, CODE_OOD, "OodEvaluationMismatch");
    }
    // The PCS half, entered below pcs_verify_any's gates on the points: zeta comes from the proof's own bytes, and where it lies is no
    // argument of this call.
    const Ext zs[2] = {zeta, bb::scale(zeta, bb::two_adic_generator(log_n))};
    for (uint32_t r = 0; r < f.n_rounds; r++) memcpy(roots + 8 * r, hdr_roots[f.root_of[r]], 32);
    return pcs_walk(L, fp, f.dialect, zs, opened, roots, proof + rd.pos, len - rd.pos, ch, why);
}
}  // namespace

int verify_fib_air(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n, const FriParams& fp,
                   std::string* why, int hash) {
    return verify_fib(FIB_PLAIN, proof, len, a_pub, b_pub, x_pub, log_n, fp, why, hash);
}
int verify_fib_air_hiding(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n, const FriParams& fp,
                          std::string* why, int hash) {
    return verify_fib(FIB_HIDING, proof, len, a_pub, b_pub, x_pub, log_n, fp, why, hash);
}

// ---- Pcs::verify of TwoAdicFriPcs / HidingFriPcs over caller matrices (the prover half: pcs.hip.inc, pcs_hiding.hip.inc), host only.  The
// opened values arrive beside the proof bytes (the FriProof section of the wire format).  Everything that is a function of the SHAPE comes
// from pcs_layout (pcs_layout.h), which the device batch verifier reads too: the gates on the arguments and their messages, each matrix's
// class, each round's tree depth, the classes with a point, each pair's matrix, place among the opened values and alpha exponent, where
// the final polynomial lies.  Here: the gates on the arguments and on a member's VALUES (canonical points off the LDE coset, at most
// PCS_MAX_POINTS distinct; canonical opened values); then pcs_walk.  hiding: log_h is the CALLER's log height.  log_heights: mixed
// heights (pcs_layout.h).
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
    Ext zs[PCS_MAX_POINTS];  // the distinct points; pair_slot: which of them a pair is opened at
    size_t n_points = 0, pi = 0;
    for (uint32_t r = 0; r < L.n_in; r++)
        for (uint32_t m = 0; m < L.nm[r]; m++)
            for (uint32_t p = 0; p < L.np[L.mat0[r] + m]; p++, pi++) {
                const uint32_t* z = points + 4 * pi;
                auto pw = [&] { return "pcs verify: round " + std::to_string(r) + " matrix " + std::to_string(m) + " point " + std::to_string(p); };
                for (int c = 0; c < 4; c++) if (z[c] >= bb::P) return bad(pw() + " is not a canonical field element");
                if (pcs_point_on_lde_coset(z, L.log_big)) return bad(pw() + " lies on the LDE coset GENERATOR * <g_big>");
                size_t k = 0;
                while (k < n_points && memcmp(zs[k].c, z, 16)) k++;
                if (k == n_points) {
                    if (n_points == PCS_MAX_POINTS) return bad(pw() + ": more than " + std::to_string(PCS_MAX_POINTS) + " distinct opening points");
                    memcpy(zs[n_points++].c, z, 16);
                }
                L.pair_slot[pi] = (uint8_t)k;
            }
    for (size_t i = 0; i < 4 * (size_t)L.total; i++) if (opened[i] >= bb::P) return bad("pcs verify: opened value word " + std::to_string(i) + " is not a canonical field element");
    std::vector<Ext> ov(L.total);
    memcpy(ov.data(), opened, 16 * (size_t)L.total);
    return pcs_walk(L, fp, DIALECT_PCS, zs, ov.data(), roots, proof, len, *chal, why);
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
