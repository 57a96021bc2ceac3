// Batch verifier of fib_air proofs on the device: p3_uni_stark::verify + TwoAdicFriPcs / HidingFriPcs::verify + p3_fri::verifier for
// FibonacciAir (the second half of the reference's run_fib_air_zk, native/src/fib_air.rs:70-72) for MANY proofs of one configuration
// at once.  verifier.hip (host, one proof) is the specification: every phase below restates verify_fib_air / verify_fib_air_hiding /
// FriCheck, and the reject codes are the host's.
//
// All proofs of one configuration have the same layout, so every offset is a function of the parameters: VLayout is computed on the
// host when the verifier is created and passed to the kernels by value.  NO LOAD ADDRESS AND NO LOOP BOUND DEPENDS ON A BYTE OF A
// PROOF: a proof whose length differs from the configuration's is rejected unread, every count / width / length word is compared with
// the value the parameters dictate (and never followed), and the query indices are sample_bits(log_big), in range by construction.
//
//   vd_transcript_kernel  one wavefront per proof: shape and canonicity of the header, the commit phase and the tail; the transcript
//                         (DevChal, transcript.hip.h); the constraints at zeta; the proof of work; the query indices.  Leaves the
//                         challenges and indices in HBM (VState).
//   vd_query_kernel       one lane per (proof, query): the reduced opening over the 8 / 36 opened columns and the fold walk down the
//                         rounds; writes every round's (ev0, ev1) leaf and compares the final polynomial with the folded value.
//   vd_open_kernel        one lane per (opening slot, proof, query), slot-major so that the lanes of a wave walk paths of one depth:
//                         assembles the leaf (salts included; FRI leaves from vd_query_kernel's pairs), hashes it up the path in the
//                         proof (lane_walk.hip.h, the form without injection: one height class) and compares with the root.
//   vd_finish_kernel      order key -> status, count of rejected proofs.
// The first failure in the HOST's order decides the code: every check does atomicMin on a per-proof word (order key << 8 | code).
#include <cstring>
#include <memory>

#include "common.h"
#include "mmcs.h"
#include "prover.h"
#include "verifier_dev.h"
#include "verifier_dev_common.hip.h"
#include "verifier_dev_host.h"

namespace p3 {

using bb::Ext;

namespace {

using namespace vdev;

constexpr uint32_t VD_MAX_OPENED = 36, VD_MAX_OPEN = 3, VD_MAX_SHAPE = 24, VD_MAX_CANON = 16, VD_MAX_ROUNDS = 28;
constexpr uint32_t CODE_OOD = 10, CODE_COMMIT_OPENING = 13;
// order keys (smaller = earlier in the host verifier's order) behind KEY_HEADER
constexpr uint64_t KEY_OOD = 1, KEY_TAIL_SHAPE = 2, KEY_POW = 3, KEY_QUERY0 = 4;

struct VLayout {
    int hash, hiding;
    uint32_t log_n, log_ext, log_big, lfinal, n_rounds, nq, fpl, pow_bits, salt;
    uint32_t proof_words;
    // words with a dictated value outside the queries; the first shape_early of them precede the constraint check in the host's order
    uint32_t n_shape, shape_early, shape_off[VD_MAX_SHAPE], shape_val[VD_MAX_SHAPE];
    // ranges of field words outside the queries (digests only under Poseidon2)
    uint32_t n_canon, canon_lo[VD_MAX_CANON], canon_hi[VD_MAX_CANON];
    uint32_t n_roots, root_off[3];  // transcript order: trace, quotient, randomization
    // the opened values in transcript order; col_off: the query's row value of the same column (offset within a query)
    uint32_t n_opened, op_off[VD_MAX_OPENED], col_off[VD_MAX_OPENED];
    uint64_t d1_mask;               // columns opened at zeta * g
    uint32_t i_tz, i_tzn, i_q, n_chunks;
    uint32_t froots_off, fpoly_off, witness_off;
    uint32_t q_base, q_len;
    // one query: the commitment openings in proof order, then the FRI rounds
    uint32_t n_open, open_off[VD_MAX_OPEN], open_nmats[VD_MAX_OPEN], open_width[VD_MAX_OPEN], open_root[VD_MAX_OPEN];
    uint32_t nr_off, fri_off[VD_MAX_ROUNDS];
    // constants of the field
    uint32_t gen, g_n, g_n_inv, neg_half, gens[VD_MAX_ROUNDS], gens_inv[VD_MAX_ROUNDS], sh[4], inv_kc[4];
};
static_assert(sizeof(VLayout) <= 3072, "passed by value in the kernel arguments");

struct VState {
    Ext zeta, zeta_next, al;
    Ext beta[VD_MAX_ROUNDS];
};

struct VArgs {
    const uint8_t* proofs;
    size_t stride;
    const uint32_t* lens;
    const uint32_t* pis;
    uint32_t n;
    VState* st;
    uint32_t* idx;            // n x nq
    uint32_t* evs;            // n x nq x n_rounds x 8
    unsigned long long* key;  // n
};

__device__ __forceinline__ uint64_t kmin(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- 1. transcript: one wavefront per proof ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) vd_transcript_kernel(VArgs a, VLayout L) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (!length_ok(a, L, i)) {  // rejected without being read
        if (lane == 0) a.key[i] = make_key(KEY_HEADER, VERIFY_MALFORMED);
        return;
    }
    const uint32_t* w = proof_words(a, i);
    uint64_t key = KEY_NONE;
    {   // shape words and canonicity, the lanes side by side
        bool early = false, late = false;
        for (uint32_t k = lane; k < L.n_shape; k += 64)
            if (w[L.shape_off[k]] != L.shape_val[k]) { if (k < L.shape_early) early = true; else late = true; }
        uint32_t hi = 0;
        for (uint32_t r = 0; r < L.n_canon; r++)
            for (uint32_t j = L.canon_lo[r] + lane; j < L.canon_hi[r]; j += 64) hi = max(hi, w[j]);
        if (lane < 3) hi = max(hi, a.pis[3 * (size_t)i + lane]);
        if (__builtin_amdgcn_ballot_w64(early || hi >= bb::P)) key = kmin(key, make_key(KEY_HEADER, VERIFY_MALFORMED));
        if (__builtin_amdgcn_ballot_w64(late)) key = kmin(key, make_key(KEY_TAIL_SHAPE, VERIFY_MALFORMED));
    }
    DevChal ch;
    ch.begin(L.hash, nullptr, &ks, true);
    uint32_t pis[3];
    for (int k = 0; k < 3; k++) pis[k] = a.pis[3 * (size_t)i + k];
    ch.observe(bb::to_monty(L.log_ext));
    ch.observe(bb::to_monty(L.log_n));
    ch.observe_n(w + L.root_off[0], 8);
    ch.observe_n(pis, 3);
    const Ext alpha = ch.sample_ext();
    for (uint32_t r = 1; r < L.n_roots; r++) ch.observe_n(w + L.root_off[r], 8);
    const Ext zeta = ch.sample_ext();
    const Ext zeta_next = bb::scale(zeta, L.g_n);
    {   // constraints at zeta (FibonacciAir, fib_air.rs:232-264) against the quotient, recomposed from its chunks
        Ext zh_pow = zeta;
        for (uint32_t k = 0; k < L.log_n; k++) zh_pow = bb::sqr(zh_pow);
        const Ext zh = bb::sub(zh_pow, bb::ext_one());
        const Ext ginv = bb::ext_from_base(L.g_n_inv);
        const Ext first = bb::mul(zh, bb::inv(bb::sub(zeta, bb::ext_one())));
        const Ext trans = bb::sub(zeta, ginv);
        const Ext last = bb::mul(zh, bb::inv(trans));
        const Ext tz0 = ldx(w, L.op_off[L.i_tz]), tz1 = ldx(w, L.op_off[L.i_tz + 1]);
        const Ext tn0 = ldx(w, L.op_off[L.i_tzn]), tn1 = ldx(w, L.op_off[L.i_tzn + 1]);
        Ext c[5] = {bb::mul(first, bb::sub(tz0, bb::ext_from_base(pis[0]))), bb::mul(first, bb::sub(tz1, bb::ext_from_base(pis[1]))),
                    bb::mul(trans, bb::sub(tz1, tn0)), bb::mul(trans, bb::sub(bb::add(tz0, tz1), tn1)),
                    bb::mul(last, bb::sub(tz1, bb::ext_from_base(pis[2])))};
        Ext folded = bb::ext_zero();
        for (int k = 0; k < 5; k++) folded = bb::add(bb::mul(folded, alpha), c[k]);
        Ext quot = bb::ext_zero();
        for (uint32_t ci = 0; ci < L.n_chunks; ci++) {
            Ext v = bb::ext_zero();
            for (uint32_t e = 0; e < 4; e++) {
                Ext be = bb::ext_zero();
                be.c[e] = bb::ONE;
                v = bb::add(v, bb::mul(be, ldx(w, L.op_off[L.i_q + 4 * ci + e])));
            }
            if (L.n_chunks > 1) {  // zps_c(zeta) = prod_{j != c} (zeta^h - s_j^h) / (s_c^h - s_j^h)
                Ext zp = bb::ext_one();
                for (uint32_t j = 0; j < L.n_chunks; j++)
                    if (j != ci) zp = bb::mul(zp, bb::sub(zh_pow, bb::ext_from_base(L.sh[j])));
                v = bb::mul(bb::scale(zp, L.inv_kc[ci]), v);
            }
            quot = bb::add(quot, v);
        }
        if (!bb::eq(bb::mul(folded, bb::inv(zh)), quot)) key = kmin(key, make_key(KEY_OOD, CODE_OOD));
    }
    for (uint32_t k = 0; k < L.n_opened; k++) ch.observe_n(w + L.op_off[k], 4);
    const Ext al = ch.sample_ext();
    VState* st = a.st + i;
    if (lane == 0) { st->zeta = zeta; st->zeta_next = zeta_next; st->al = al; }
    const FriTail tail{L.froots_off, L.n_rounds, L.fpoly_off, L.fpl, L.witness_off, L.pow_bits, L.nq, L.log_big};
    if (!fri_transcript_tail(ch, w, lane, tail, st->beta, a.idx + (size_t)i * L.nq)) key = kmin(key, make_key(KEY_POW, CODE_POW));
    if (lane == 0) a.key[i] = key;
}

// ---- 2. query arithmetic: one lane per (proof, query) -----------------------------------------------------------------------
__global__ void __launch_bounds__(256) vd_query_kernel(VArgs a, VLayout L) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)a.n * L.nq) return;
    const uint32_t i = (uint32_t)(t / L.nq), q = (uint32_t)(t % L.nq);
    if (!length_ok(a, L, i)) return;
    const uint32_t* w = proof_words(a, i);
    const uint32_t* qw = w + L.q_base + (size_t)q * L.q_len;
    const VState* st = a.st + i;
    const uint32_t index = a.idx[t];
    const uint32_t xi = bb::mul(L.gen, bb::pow(L.gens[L.log_big], rev_bits_dev(index, L.log_big)));
    const Ext d0 = bb::inv(bb::sub(st->zeta, bb::ext_from_base(xi))), d1 = bb::inv(bb::sub(st->zeta_next, bb::ext_from_base(xi)));
    const Ext al = st->al;
    Ext folded = bb::ext_zero(), alk = bb::ext_one();
    for (uint32_t k = 0; k < L.n_opened; k++) {
        const Ext diff = bb::sub(ldx(w, L.op_off[k]), bb::ext_from_base(qw[L.col_off[k]]));
        folded = bb::add(folded, bb::mul(alk, bb::mul(diff, ((L.d1_mask >> k) & 1ull) ? d1 : d0)));
        alk = bb::mul(alk, al);
    }
    uint32_t idx = index;
    uint32_t* evs = a.evs + t * L.n_rounds * 8;
    for (uint32_t r = 0; r < L.n_rounds; r++) {
        Ext ev0, ev1;
        folded = fri_fold_step(folded, idx, ldx(qw, L.fri_off[r]), st->beta[r], L.log_big - 1 - r, L.gens, L.gens_inv, L.neg_half, ev0, ev1);
        stx(evs, 8 * r, ev0);
        stx(evs, 8 * r + 4, ev1);
        idx >>= 1;
    }
    const Ext evf = final_poly_eval(w, L.fpoly_off, L.fpl, L.gens[L.lfinal], L.lfinal, idx);
    if (!bb::eq(evf, folded)) report(a, i, KEY_QUERY0 + (uint64_t)q * STEPS_PER_QUERY + 2 * (L.n_open + L.n_rounds), CODE_FINAL_POLY);
}

// ---- 3. openings: one lane per (slot, proof, query) -------------------------------------------------------------------------
// What one lane opens: leaf word e is evs[e] for e < n_ev (an FRI leaf's pair), else word `e - n_ev` of n_mats matrices of
// `width` values at `vals` (each behind its width word) with their salts at `salts` (each behind its length word).
struct LaneOpening {
    const uint32_t* evs;
    const uint32_t* vals;
    const uint32_t* salts;
    const uint32_t* path;
    const uint32_t* root;
    uint32_t n_ev, width, salt, leaf_len, depth, index;
    // lane_walk's word source, one height class: only level 0 has a row
    __device__ __forceinline__ uint32_t len(uint32_t) const { return leaf_len; }
    __device__ __forceinline__ uint32_t word(uint32_t, uint32_t e) const { return leaf_word(e); }
    __device__ __forceinline__ uint32_t leaf_word(uint32_t e) const {
        if (e < n_ev) return evs[e];
        e -= n_ev;
        const uint32_t per = width + salt, m = e / per, c = e % per;
        return c < width ? vals[m * (1 + width) + 1 + c] : salts[m * (1 + salt) + 1 + (c - width)];
    }
};

template <int HASH>
__global__ void __launch_bounds__(256) vd_open_kernel(VArgs a, VLayout L) {
    const uint64_t per_slot = (uint64_t)a.n * L.nq, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per_slot * (L.n_open + L.n_rounds)) return;
    const uint32_t slot = (uint32_t)(t / per_slot);
    const uint64_t pq = t % per_slot;
    const uint32_t i = (uint32_t)(pq / L.nq), q = (uint32_t)(pq % L.nq);
    if (!length_ok(a, L, i)) return;
    const uint32_t* w = proof_words(a, i);
    const uint32_t* qw = w + L.q_base + (size_t)q * L.q_len;
    const uint32_t index = a.idx[pq];
    const uint64_t qkey = KEY_QUERY0 + (uint64_t)q * STEPS_PER_QUERY;
    // a word of a query the parameters dictate.  The plain format's host parser follows the width / depth / count words of the
    // queries while it skips to the final polynomial (codes 7 / 8, before the proof of work); the hiding format's computes the skip
    // and meets them in query order (code 12).
    bool shape_tail = false, shape_here = false;
    LaneOpening o{};
    o.salt = L.salt;
    uint32_t hi = 0, code;
    if (slot < L.n_open) {
        const uint32_t* p = qw + L.open_off[slot];
        const uint32_t n_mats = L.open_nmats[slot];
        o.width = L.open_width[slot];
        if (slot == 0 && qw[0] != L.n_open) (L.hiding ? shape_here : shape_tail) = true;
        if (p[0] != n_mats) shape_here = true;
        o.vals = p + 1;
        for (uint32_t m = 0; m < n_mats; m++)
            if (o.vals[m * (1 + o.width)] != o.width) (L.hiding ? shape_here : shape_tail) = true;
        o.salts = o.vals + n_mats * (1 + o.width);
        if (L.salt)
            for (uint32_t m = 0; m < n_mats; m++)
                if (o.salts[m * (1 + L.salt)] != L.salt) shape_here = true;
        const uint32_t* dp = o.salts + (L.salt ? n_mats * (1 + L.salt) : 0u);
        o.depth = L.log_big;
        if (dp[0] != o.depth) (L.hiding ? shape_here : shape_tail) = true;
        o.path = dp + 1;
        o.leaf_len = n_mats * (o.width + L.salt);
        o.index = index;
        o.root = w + L.open_root[slot];
        code = CODE_COMMIT_OPENING;
    } else {
        const uint32_t r = slot - L.n_open;
        const uint32_t* p = qw + L.fri_off[r];
        if (r == 0 && qw[L.nr_off] != L.n_rounds) (L.hiding ? shape_here : shape_tail) = true;
        for (int c = 0; c < 4; c++) hi = max(hi, p[c]);  // the sibling: a field element of the proof
        o.evs = a.evs + (pq * L.n_rounds + r) * 8;
        o.n_ev = 8;
        o.width = 0;
        o.salts = p + 4;
        if (L.salt && p[4] != L.salt) shape_here = true;
        const uint32_t* dp = p + 4 + (L.salt ? 1 + L.salt : 0u);
        o.depth = L.log_big - 1 - r;
        if (dp[0] != o.depth) (L.hiding ? shape_here : shape_tail) = true;
        o.path = dp + 1;
        o.leaf_len = 8 + L.salt;
        o.index = index >> (r + 1);
        o.root = w + L.froots_off + 8 * r;
        code = CODE_FRI_OPENING;
    }
    const bool mismatch = lane_walk::walk<HASH, false>(o, lane_walk::PathWords{o.path}, o.depth, o.index, o.root, hi);
    if (shape_tail) report(a, i, KEY_TAIL_SHAPE, VERIFY_MALFORMED);
    if (shape_here) report(a, i, qkey + 2 * slot, VERIFY_MALFORMED);
    if (hi >= bb::P) report(a, i, KEY_HEADER, VERIFY_MALFORMED);
    if (mismatch) report(a, i, qkey + 2 * slot + 1, code);
}

// ---- 4. order key -> status -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vd_finish_kernel(const unsigned long long* key, uint32_t n, uint32_t* status, uint32_t* d_rejected) {
    finish(key, n, status, d_rejected);
}

// ---- host: the layout of one configuration ------------------------------------------------------------------------------------
struct Cursor {  // walks the wire format as the provers write it (DESIGN.md "proof bytes"), recording where things are
    VLayout& L;
    uint32_t pos = 0;
    bool early = true;
    void shape(uint32_t val) {
        L.shape_off[L.n_shape] = pos; L.shape_val[L.n_shape] = val; L.n_shape++;
        if (early) L.shape_early = L.n_shape;
        pos++;
    }
    void felts(uint32_t n) {  // merges with the previous range when adjacent
        if (L.n_canon && L.canon_hi[L.n_canon - 1] == pos) L.canon_hi[L.n_canon - 1] = pos + n;
        else { L.canon_lo[L.n_canon] = pos; L.canon_hi[L.n_canon] = pos + n; L.n_canon++; }
        pos += n;
    }
    void digests(uint32_t n) { if (L.hash == HASH_POSEIDON2) felts(8 * n); else pos += 8 * n; }
    void opened(uint32_t n) { for (uint32_t k = 0; k < n; k++) L.op_off[L.n_opened++] = pos + 4 * k; felts(4 * n); }
};

int make_layout(int hash, bool hiding, uint32_t log_n, const FriParams& fp, VLayout* out) {
    std::string why;
    if (verify_check_parameters(hash, hiding, log_n, fp, &why)) return fail(ERR_BAD_ARG, why);
    VLayout& L = *out;
    memset(&L, 0, sizeof(L));
    L.hash = hash; L.hiding = hiding ? 1 : 0;
    L.log_n = log_n;
    L.log_ext = hiding ? log_n + 1 : log_n;
    L.log_big = L.log_ext + fp.log_blowup;
    L.lfinal = fp.log_blowup + fp.log_final_poly_len;
    L.n_rounds = L.log_big - L.lfinal;
    L.nq = fp.num_queries;
    L.fpl = 1u << fp.log_final_poly_len;
    L.pow_bits = fp.proof_of_work_bits;
    L.salt = hiding ? 4 : 0;
    Cursor c{L};
    c.shape(0x42463350u); c.shape(hiding ? 2 : 1); c.shape(log_n);
    L.n_roots = hiding ? 3 : 2;
    for (uint32_t r = 0; r < L.n_roots; r++) { L.root_off[r] = c.pos; c.digests(1); }
    if (!hiding) {  // trace at zeta, trace at zeta g, one round of one quotient matrix
        c.shape(2); c.opened(2); c.shape(2); c.opened(2); c.shape(1); c.shape(4); c.opened(4);
        L.i_tz = 0; L.i_tzn = 2; L.i_q = 4; L.n_chunks = 1;
        L.d1_mask = 0xcull;
    } else {  // randomization (8), trace at zeta (6), trace at zeta g (6), four quotient chunks
        c.shape(8); c.opened(8); c.shape(6); c.opened(6); c.shape(6); c.opened(6); c.shape(4);
        for (int k = 0; k < 4; k++) { c.shape(4); c.opened(4); }
        L.i_tz = 8; L.i_tzn = 14; L.i_q = 20; L.n_chunks = 4;
        L.d1_mask = 0x3full << 14;
    }
    c.early = false;
    c.shape(L.n_rounds);
    L.froots_off = c.pos; c.digests(L.n_rounds);
    c.shape(L.nq);
    L.q_base = c.pos;
    {   // one query, offsets relative to its first word
        uint32_t p = 1;  // behind the count of commitment openings
        const uint32_t D = 8;
        auto opening = [&](uint32_t root, uint32_t n_mats, uint32_t width) {
            const uint32_t o = L.n_open++;
            L.open_off[o] = p; L.open_nmats[o] = n_mats; L.open_width[o] = width; L.open_root[o] = root;
            const uint32_t vals = p + 1;
            p = vals + n_mats * (1 + width) + (L.salt ? n_mats * (1 + L.salt) : 0) + 1 + D * L.log_big;
            return vals;
        };
        if (!hiding) {
            const uint32_t vt = opening(L.root_off[0], 1, 2), vq = opening(L.root_off[1], 1, 4);
            for (uint32_t j = 0; j < 2; j++) { L.col_off[j] = vt + 1 + j; L.col_off[2 + j] = vt + 1 + j; }
            for (uint32_t j = 0; j < 4; j++) L.col_off[4 + j] = vq + 1 + j;
        } else {
            const uint32_t vr = opening(L.root_off[2], 1, 8), vt = opening(L.root_off[0], 1, 6), vq = opening(L.root_off[1], 4, 4);
            for (uint32_t j = 0; j < 8; j++) L.col_off[j] = vr + 1 + j;
            for (uint32_t j = 0; j < 6; j++) { L.col_off[8 + j] = vt + 1 + j; L.col_off[14 + j] = vt + 1 + j; }
            for (uint32_t j = 0; j < 16; j++) L.col_off[20 + j] = vq + (j / 4) * 5 + 1 + (j % 4);
        }
        L.nr_off = p++;
        for (uint32_t r = 0; r < L.n_rounds; r++) {
            L.fri_off[r] = p;
            p += 4 + (L.salt ? 1 + L.salt : 0) + 1 + D * (L.log_big - 1 - r);
        }
        L.q_len = p;
    }
    const uint64_t after = (uint64_t)L.q_base + (uint64_t)L.q_len * L.nq;
    if (after + 2 + 4ull * L.fpl > 0x3fffffffull) return fail(ERR_BAD_ARG, "fib_verifier: a proof of this configuration exceeds 2^32 bytes");
    c.pos = (uint32_t)after;
    c.shape(L.fpl);
    L.fpoly_off = c.pos; c.felts(4 * L.fpl);
    L.witness_off = c.pos; c.felts(1);
    L.proof_words = c.pos;
    // constants
    L.gen = bb::to_monty(bb::GEN);
    L.g_n = bb::two_adic_generator(log_n);
    L.g_n_inv = bb::inv(L.g_n);
    L.neg_half = bb::inv(bb::neg(bb::dbl(bb::ONE)));
    for (uint32_t b = 0; b < VD_MAX_ROUNDS; b++) { L.gens[b] = bb::two_adic_generator(b); L.gens_inv[b] = bb::inv(L.gens[b]); }
    if (hiding) {  // chunk cosets D_c = s_c <g_h>: s_c^h = GENERATOR^h w4^c
        const uint32_t gh = bb::pow(L.gen, 1ull << log_n), w4 = bb::two_adic_generator(2);
        uint32_t p = bb::ONE;
        for (int k = 0; k < 4; k++) { L.sh[k] = bb::mul(gh, p); p = bb::mul(p, w4); }
        for (int ci = 0; ci < 4; ci++) {
            uint32_t kc = bb::ONE;
            for (int j = 0; j < 4; j++)
                if (j != ci) kc = bb::mul(kc, bb::sub(L.sh[ci], L.sh[j]));
            L.inv_kc[ci] = bb::inv(kc);
        }
    }
    return OK;
}

}  // namespace

int fib_proof_len(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t* len_out) {
    VLayout L;
    if (int rc = make_layout(hash, hiding, log_n, fp, &L)) return rc;
    *len_out = 4 * (size_t)L.proof_words;
    return OK;
}

struct FibVerifierDev::Impl : VerifierDevHost {
    VLayout L;
    VState* st = nullptr;
    uint32_t *idx = nullptr, *evs = nullptr, *d_pis = nullptr;  // d_pis: staging of the host entry
    unsigned long long* key = nullptr;
};

FibVerifierDev::FibVerifierDev() : im(new Impl()) {}
FibVerifierDev::~FibVerifierDev() { delete im; }
size_t FibVerifierDev::proof_len() const { return 4 * (size_t)im->L.proof_words; }
size_t FibVerifierDev::max_proofs() const { return im->max_proofs; }
int FibVerifierDev::device() const { return im->device; }

int FibVerifierDev::init(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t max_proofs) {
    if (int rc = make_layout(hash, hiding, log_n, fp, &im->L)) return rc;
    const VLayout& L = im->L;
    if (max_proofs == 0) return fail(ERR_BAD_ARG, "fib_verifier_create: max_proofs must be positive");
    if (max_proofs * (uint64_t)L.nq * (L.n_open + L.n_rounds) > 0x7fffffffull * 256ull || max_proofs > 0x7fffffffull)
        return fail(ERR_BAD_ARG, "fib_verifier_create: max_proofs x num_queries too large");
    Context* cx = nullptr;
    if (int rc = get_context(&cx)) return rc;
    im->device = cx->device;
    im->max_proofs = max_proofs;
    return im->alloc({Impl::buf(&im->st, max_proofs * sizeof(VState)), Impl::buf(&im->idx, max_proofs * L.nq * 4),
                      Impl::buf(&im->evs, max_proofs * L.nq * (size_t)L.n_rounds * 32), Impl::buf(&im->key, max_proofs * 8)});
}

int FibVerifierDev::verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_pis, size_t n,
                               uint32_t* d_status, uint32_t* d_rejected, hipStream_t stream) {
    const VLayout& L = im->L;
    if (int rc = im->check_batch("fib_verifier_verify_dev", n, !d_proofs || !d_pis || !d_status, stride, proof_len())) return rc;
    if (reinterpret_cast<uintptr_t>(d_proofs) & 3u) return fail(ERR_BAD_ARG, "fib_verifier_verify_dev: d_proofs must be 4-byte aligned");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    if (d_rejected) P3_HIP(hipMemsetAsync(d_rejected, 0, 4, stream));
    if (!n) return OK;
    VArgs a{d_proofs, stride, d_lens, d_pis, (uint32_t)n, im->st, im->idx, im->evs, im->key};
    hipLaunchKernelGGL(vd_transcript_kernel, dim3((uint32_t)n), dim3(64), 0, stream, a, L);
    const uint64_t pq = (uint64_t)n * L.nq;
    hipLaunchKernelGGL(vd_query_kernel, dim3((uint32_t)((pq + 255) / 256)), dim3(256), 0, stream, a, L);
    const uint64_t lanes = pq * (L.n_open + L.n_rounds);
    if (L.hash == HASH_KECCAK)
        hipLaunchKernelGGL(vd_open_kernel<HASH_KECCAK>, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, a, L);
    else
        hipLaunchKernelGGL(vd_open_kernel<HASH_POSEIDON2>, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, a, L);
    hipLaunchKernelGGL(vd_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, im->key, (uint32_t)n, d_status, d_rejected);
    P3_HIP(hipGetLastError());
    return OK;
}

int FibVerifierDev::verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint64_t* a, const uint64_t* b,
                                const uint64_t* x, uint32_t* status_out) {
    if (n && (!proofs || !lens || !a || !b || !x || !status_out)) return fail(ERR_BAD_ARG, "fib_verifier_verify: null argument");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    const size_t plen = proof_len(), cap = im->max_proofs;
    if (int rc = im->stage(plen, {Impl::buf(&im->d_pis, cap * 12)})) return rc;
    std::vector<uint32_t> hp(3 * cap);
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = std::min(cap, n - base);
        if (int rc = im->upload("fib_verifier_verify", m, proofs + base, lens + base, plen)) return rc;
        for (size_t k = 0; k < m; k++) {
            const uint64_t v[3] = {a[base + k], b[base + k], x[base + k]};
            for (int j = 0; j < 3; j++) hp[3 * k + j] = bb::to_monty((uint32_t)(v[j] % bb::P));
        }
        P3_HIP(hipMemcpyAsync(im->d_pis, hp.data(), m * 12, hipMemcpyHostToDevice, im->stream));
        if (int rc = verify_dev(im->d_proofs, plen, im->d_lens, im->d_pis, m, im->d_status, nullptr, im->stream)) return rc;
        if (int rc = im->download_status(status_out + base, m)) return rc;
        P3_HIP(hipStreamSynchronize(im->stream));
    }
    return OK;
}

}  // namespace p3
