// Batch verifier of PCS proofs on the device: TwoAdicFriPcs::verify / HidingFriPcs::verify + p3_fri::verifier over caller matrices for
// MANY members of one shape at once.  verifier.hip's pcs_verify_any (host, one proof) is the specification: every phase below restates
// it and FriCheck, and the reject codes are the host's.  verifier_dev.hip (fib_air proofs) and air_verifier_dev.hip (a caller-defined AIR's)
// each own one of these for the FRI section behind their header.
//
// A SHAPE fixes the layout of every proof: the FRI parameters, the committed log height, per round the matrices' widths, per matrix
// its opening points as SLOTS (a member supplies n_slots points; pair (matrix, point) -> slot).  Every offset is then a function of
// the shape: PLayout is computed on the host when the verifier is created and passed to the kernels by value (2.0 kB: it fits).  It is
// pcs_layout's (pcs_layout.h), the one layout pcs_verify_any reads too: the shape gates and the offsets exist once.
//
// SAFETY RULE.  NO LOAD ADDRESS AND NO LOOP BOUND DEPENDS ON A PROOF BYTE, AN OPENED VALUE, A POINT OR A CHALLENGER STATE WORD.  A
// proof whose length differs from the shape's is rejected unread; every count / width / depth / salt-length word is compared with the
// value the shape dictates and never followed; the imported state is loaded ONCE (registers, the sponge's copy in LDS) and the counters
// of that copy are compared with their ranges before anything uses them (a Keccak fill level indexes the sponge's block in LDS);
// the query indices are sample_bits(log_big), in range by construction, and select bits and exponents, never addresses.
//
//   pv_transcript_kernel  one wavefront per member.  A member its owner decided (d_owner_key at KEY_HEADER) is skipped unread; any other
//                         starts from its owner's key.  First the checks, before any arithmetic: length, the three header count words
//                         (KEY_SHAPE: compared, never followed, so the member is walked on and an owner's 10 still precedes them),
//                         canonicity of the proof's field words outside the queries (those of the queries are scanned by
//                         pv_open_kernel, AFTER pv_query_kernel's arithmetic has consumed them: harmless, they never reach an
//                         address, and key 0 wins), of the opened values, the points and (Poseidon2)
//                         the roots, a base-field point on GENERATOR <g_big>, the state counters.  Then the transcript (DevChal,
//                         transcript.hip.h) from the imported state: opened values, alpha, the commit-phase betas, the final
//                         polynomial, the witness, the proof of work, the query indices; the state is exported.  Leaves in HBM per
//                         member: alpha^c for c below the widest matrix, and per (matrix, point) pair alpha^aoff and
//                         alpha^aoff Y, Y = sum_c alpha^c opened_c, aoff the pair's alpha exponent.  The coset gate is against the
//                         TALLEST coset, which contains every smaller one.
//   pv_query_kernel       per (member, query): S_m = sum_c alpha^c row[c] ONCE per matrix, shared by its points;
//                         ro = sum_pairs (alpha^off Y - alpha^off S_m) / (z - x) with the <= 4 slot denominators inverted together
//                         (one inversion per query); then FriCheck::query's walk: writes every round's (ev0, ev1) leaf and compares
//                         the final polynomial with the folded value.  Two forms:
//                           <false>  one lane per query;
//                           <true>   one wavefront per query, lanes along the columns, S_m summed across the wave.
//                         THE SWITCH is PV_WAVE_MIN_COLS = 256 row words per query (sum of the widths of all matrices).  Instruction
//                         counts, estimated from the source (not measured): the column loop is ~50 VALU instructions per column (an
//                         extension element scaled by a base word is 4 Montgomery products of ~9 instructions, plus 4 modular additions
//                         of 3 and the loads), everything behind it ~3k (the <= 4 denominators with ONE inversion, 31 squarings and
//                         ~20 products of the norm, ~1.5k; two extension products per pair; ~150 per fold round).  A batch of 64 members
//                         x 100 queries is 100 waves in the lane form and 6400 in the wave form on 1024 SIMDs; per SIMD the lane form
//                         issues 50 W + 3k instructions, the wave form 6.25 x (0.8 W + 3k + 0.15k of cross-lane sums): equal near
//                         W = 370, and a lone member's latency favours the wave form earlier still.  256 is the power of two below the
//                         crossing.
//   pv_open_kernel        one lane per (opening slot, member, query), slot-major so that the lanes of a wave walk paths of one depth:
//                         an input round's leaf is m0 || m1 ... (with salts m0 || s0 || m1 || s1 ...), an FRI leaf the 8 words of
//                         pv_query_kernel's pair plus its salt; hashed up the path in the proof (lane_walk.hip.h) and compared
//                         with the member's root / the round's root in the proof.
//   pv_finish_kernel      order key -> status, count of rejected members.
// MIXED HEIGHTS (a verifier from p3hip_pcs_verifier_create_mixed whose matrices are not all of one height; pcs_verify_any with
// log_heights is the specification).  A CLASS is the set of matrices of one log_big_c = log_h_c + log_blowup.  The layout knows
// log_big_m per matrix, per round the tree depth log_big_r (its tallest matrix: path length, depth word), per pair its position among
// the opened values AND its alpha exponent (its class's counter, which runs across rounds), and which classes have a point.  The
// query and opening kernels take a compile-time MIXED parameter, so that a same-height shape runs the arithmetic it ran before; every
// height, depth, injection level and shift below comes from PLayout, none from a member.
//   pv_query_kernel<_, true>   one reduced opening per class, computed when the walk reaches its height (one batched inversion of the
//                              slot denominators per class; one reduced opening live; nothing indexed by a runtime class number): the
//                              tallest class starts the walk, and after the fold that reaches 2^log_big_c: folded += beta_r^2 ro_c.
//   pv_open_kernel<_, true>    an input round's opening walks log_big_r levels from index >> (log_big - log_big_r); the leaf is the
//                              round's tallest matrices in input order; a shorter class's row is hashed and compressed in (right
//                              operand) at the level whose size equals its height, before that level's sibling.
// A roll-in or an injection adds no check of its own: order keys and codes are where they were.
// The first failure in the HOST's order decides the code: every check does atomicMin on a per-member word (order key << 8 | code), on
// the one scale of verifier_dev_common.hip.h.  Anything the host answers with 5..9 or 12, or refuses for a member's VALUES, is
// VERIFY_MALFORMED here: key 0, or KEY_SHAPE for a count word outside the queries, or for a shape word inside a query its place in the
// order, so that an earlier query's 13 / 14 / 15 still wins -- unless the shape has `counts` (PcsShape: wire format 1 of fib_air), which
// sends the words that format's host follows to KEY_SHAPE.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>

#include "challenger.h"
#include "common.h"
#include "mmcs.h"
#include "pcs_verifier_dev.h"
#include "prover.h"
#include "verifier_dev_common.hip.h"
#include "verifier_dev_host.h"

namespace p3 {

using bb::Ext;

namespace {

using namespace vdev;

constexpr uint32_t PV_WAVE_MIN_COLS = 256;
static_assert(PV_MAX_PAIRS <= 128, "the transcript kernel keeps two pair powers per lane");

struct PState {
    Ext beta[PV_MAX_FRI];
};

struct PArgs {
    const uint8_t* proofs;
    size_t stride;
    const uint32_t* lens;
    const uint32_t* roots;    // n x n_in x 8
    const uint32_t* points;   // n x n_slots x 4
    const uint32_t* opened;   // n x total x 4
    const uint32_t* chal_in;  // n x CHALLENGER_STATE_WORDS
    uint32_t* chal_out;       // the same, or null
    uint32_t n;
    PState* st;
    uint32_t* idx;            // n x nq
    uint32_t* evs;            // n x nq x n_fri x 8
    uint32_t* alp;            // n x wmax x 4
    uint32_t* pa;             // n x n_pairs x 4: alpha^off
    uint32_t* pb;             // n x n_pairs x 4: alpha^off Y
    unsigned long long* key;  // n
    const unsigned long long* owner;  // n: the key an owner's own checks left each member at, or null
};

static_assert(sizeof(PLayout) + sizeof(PArgs) <= 4096, "both are passed by value: the kernel-argument segment holds 4 KB");

// the owner or the transcript kernel decided the member (verifier_dev_common.hip.h) before it produced anything the later kernels read
__device__ __forceinline__ bool header_rejected(const PArgs& a, uint32_t i) { return decided(a.key[i]); }
__device__ __forceinline__ Ext wave_sum(Ext v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int c = 0; c < 4; c++) v.c[c] = bb::add(v.c[c], (uint32_t)__shfl_xor((int)v.c[c], o, 64));
    return v;
}

// ---- 1. transcript: one wavefront per member --------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) pv_transcript_kernel(PArgs a, PLayout L) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint64_t own = a.owner ? a.owner[i] : KEY_NONE;  // the member's key starts from its owner's
    if (decided(own) || !length_ok(a, L, i)) {  // rejected without being read
        if (lane == 0) a.key[i] = make_key(KEY_HEADER, VERIFY_MALFORMED);
        return;
    }
    const uint32_t* w = proof_words(a, i);
    const uint32_t* op = a.opened + (size_t)i * L.total * 4;
    const uint32_t* pts = a.points + (size_t)i * L.n_slots * 4;
    const uint32_t* roots = a.roots + (size_t)i * L.n_in * 8;
    const uint32_t* cs = a.chal_in + (size_t)i * CHALLENGER_STATE_WORDS;
    const uint32_t nw = 4 * L.total;
    DevChal ch;  // a copy of fixed size and no arithmetic: the counters are not followed before the check below
    ch.begin(L.hash, reinterpret_cast<DevState*>(const_cast<uint32_t*>(cs)), &ks, false);
    bool counts = false;  // a count word outside the queries: compared, never followed, so the transcript goes on
    {   // every check that needs no challenge, the lanes side by side
        bool bad = false;
        uint32_t hi = 0;
        if (lane == 0) counts = w[0] != L.n_fri || w[L.nq_off] != L.nq || w[L.fpl_off] != L.fpl;
        if (L.hash == HASH_POSEIDON2) {
            for (uint32_t j = 1 + lane; j < 1 + 8 * L.n_fri; j += 64) hi = max(hi, w[j]);
            if (lane < 8 * L.n_in) hi = max(hi, roots[lane]);
        }
        for (uint32_t j = L.fpoly_off + lane; j <= L.witness_off; j += 64) hi = max(hi, w[j]);  // the witness follows the final polynomial
        for (uint32_t j = lane; j < nw; j += 64) hi = max(hi, op[j]);
        if (lane < 4 * L.n_slots) hi = max(hi, pts[lane]);
        if (lane < L.n_slots) {  // a base-field point with (z / GENERATOR)^big = 1: 1 / (z - x) has no value on the LDE coset
            const uint32_t* z = pts + 4 * lane;
            if (!(z[1] | z[2] | z[3])) {
                uint32_t q = bb::mul(z[0], L.gen_inv);
                for (uint32_t k = 0; k < L.log_big; k++) q = bb::sqr(q);
                bad |= q == bb::ONE;
            }
        }
        // the state's counters, as the challenger holds them after its ONE load of the state (registers; the LDS copy of the sponge):
        // what is compared here is what is used below, whatever becomes of d_chal_in during the call
        if (L.hash == HASH_POSEIDON2) bad |= ch.n_in >= 8u || ch.n_out > 8u;
        else bad |= ks.blen >= 136u || ks.n_obuf > 32u;
        if (__builtin_amdgcn_ballot_w64(bad || hi >= bb::P)) {
            if (lane == 0) a.key[i] = make_key(KEY_HEADER, VERIFY_MALFORMED);
            return;
        }
    }
    uint64_t key = own;
    if (__builtin_amdgcn_ballot_w64(counts)) key = kmin(key, make_key(KEY_SHAPE, VERIFY_MALFORMED));
    for (uint32_t base = 0; base < nw; base += 64) {  // 64 words per load, observed one by one
        const uint32_t v = base + lane < nw ? op[base + lane] : 0u;
        const uint32_t cnt = min(64u, nw - base);
        for (uint32_t k = 0; k < cnt; k++) ch.observe((uint32_t)__shfl((int)v, (int)k, 64));
    }
    const Ext al = ch.sample_ext();
    {   // alpha^c for c < wmax, and per pair alpha^aoff and alpha^aoff Y: lane l walks the columns l, l + 64, ...
        Ext a64 = al;
        for (int k = 0; k < 6; k++) a64 = bb::sqr(a64);
        const Ext pl = bb::pow(al, (uint64_t)lane);
        {
            Ext p = pl;
            uint32_t* t = a.alp + (size_t)i * L.wmax * 4;
            for (uint32_t c = lane; c < L.wmax; c += 64) { stx(t, 4 * (size_t)c, p); p = bb::mul(p, a64); }
        }
        Ext mine[2];
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t pr = lane + 64 * h;
            mine[h] = pr < L.n_pairs ? bb::pow(al, (uint64_t)L.pair_aoff[pr]) : bb::ext_one();
        }
        for (uint32_t pr = 0; pr < L.n_pairs; pr++) {
            const uint32_t off = L.pair_off[pr], wd = L.width[L.pair_mat[pr]];
            Ext p = pl, y = bb::ext_zero();
            for (uint32_t c = lane; c < wd; c += 64) { y = bb::add(y, bb::mul(p, ldx(op, 4 * (size_t)(off + c)))); p = bb::mul(p, a64); }
            y = wave_sum(y);
            Ext ao;
            for (int c = 0; c < 4; c++) ao.c[c] = (uint32_t)__shfl((int)(pr < 64 ? mine[0].c[c] : mine[1].c[c]), (int)(pr & 63u), 64);
            if (lane == 0) {
                stx(a.pa, 4 * ((size_t)i * L.n_pairs + pr), ao);
                stx(a.pb, 4 * ((size_t)i * L.n_pairs + pr), bb::mul(ao, y));
            }
        }
    }
    const FriTail tail{1, L.n_fri, L.fpoly_off, L.fpl, L.witness_off, L.pow_bits, L.nq, L.log_big};  // the roots follow the round count
    if (!fri_transcript_tail(ch, w, lane, tail, a.st[i].beta, a.idx + (size_t)i * L.nq)) key = kmin(key, make_key(KEY_POW, CODE_POW));
    if (a.chal_out) export_challenger(ch, L.hash, a.chal_out + (size_t)i * CHALLENGER_STATE_WORDS, lane);
    if (lane == 0) a.key[i] = key;
}

// ---- 2. reduced opening and fold walk: per (member, query) ------------------------------------------------------------------
__device__ __forceinline__ Ext pick4(const Ext d[4], uint32_t s) { return s == 0 ? d[0] : s == 1 ? d[1] : s == 2 ? d[2] : d[3]; }

// The reduced opening of ONE class at one query: sum over the class's (matrix, point) pairs of (alpha^aoff Y - alpha^aoff S_m) / (z - x),
// x = GENERATOR g_lb^bitrev(index >> (log_big - lb)).  MIXED = false: lb is log_big and every matrix belongs (the one-class form, as it
// always ran).  Which matrices belong is the layout's word: in the wave form the branch is wave-uniform.
template <bool WAVE, bool MIXED>
__device__ __forceinline__ Ext class_opening(const PArgs& a, const PLayout& L, uint32_t i, const uint32_t* qw, const uint32_t* pts,
                                             const uint32_t* alp, uint32_t index, uint32_t lb, uint32_t lane, uint32_t step) {
    const uint32_t xi = bb::mul(L.gen, bb::pow(L.gens[lb], rev_bits_dev(MIXED ? index >> (L.log_big - lb) : index, lb)));
    Ext dz[4];
    {   // 1 / (z_s - x) for the slots, one inversion
        Ext d[4], pre[4], acc = bb::ext_one();
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            d[s] = s < L.n_slots ? bb::sub(ldx(pts, 4 * s), bb::ext_from_base(xi)) : bb::ext_one();
            pre[s] = acc;
            acc = bb::mul(acc, d[s]);
        }
        Ext inv = bb::inv(acc);
#pragma unroll
        for (int s = 3; s >= 0; s--) { dz[s] = bb::mul(inv, pre[s]); inv = bb::mul(inv, d[s]); }
    }
    Ext ro = bb::ext_zero();
    uint32_t pair = 0;
    for (uint32_t r = 0; r < L.n_in; r++)
        for (uint32_t m = L.mat0[r]; m < L.mat0[r] + L.nm[r]; m++) {
            if (MIXED && (L.log_big_m[m] != lb || L.np[m] == 0)) { pair += L.np[m]; continue; }
            const uint32_t* vals = qw + L.val_off[m];
            const uint32_t wd = L.width[m];
            Ext s = bb::ext_zero();
            for (uint32_t c = lane; c < wd; c += step) s = bb::add(s, bb::scale(ldx(alp, 4 * (size_t)c), vals[c]));
            if (WAVE) s = wave_sum(s);
            for (uint32_t p = 0; p < L.np[m]; p++, pair++) {
                const size_t po = 4 * ((size_t)i * L.n_pairs + pair);
                const Ext num = bb::sub(ldx(a.pb, po), bb::mul(ldx(a.pa, po), s));
                ro = bb::add(ro, bb::mul(num, pick4(dz, L.pair_slot[pair])));
            }
        }
    return ro;
}

template <bool WAVE, bool MIXED>
__global__ void __launch_bounds__(256) pv_query_kernel(PArgs a, PLayout L) {
    const uint64_t gt = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t = WAVE ? gt >> 6 : gt;  // WAVE: the same for every lane of a wave, so every branch below is wave-uniform
    const uint32_t lane = WAVE ? (threadIdx.x & 63u) : 0u, step = WAVE ? 64u : 1u;
    if (t >= (uint64_t)a.n * L.nq) return;
    const uint32_t i = (uint32_t)(t / L.nq), q = (uint32_t)(t % L.nq);
    if (!length_ok(a, L, i) || header_rejected(a, i)) return;
    const uint32_t* w = proof_words(a, i);
    const uint32_t* qw = w + L.q_base + (size_t)q * L.q_len;
    const uint32_t* pts = a.points + (size_t)i * L.n_slots * 4;
    const uint32_t* alp = a.alp + (size_t)i * L.wmax * 4;
    const PState* st = a.st + i;
    const uint32_t index = a.idx[t];
    Ext folded = class_opening<WAVE, MIXED>(a, L, i, qw, pts, alp, index, L.log_big, lane, step);  // the tallest class starts the walk
    uint32_t idx = index;
    uint32_t* evs = a.evs + t * L.n_fri * 8;
    for (uint32_t r = 0; r < L.n_fri; r++) {
        const uint32_t lfh = L.log_big - 1 - r;
        const Ext beta = st->beta[r];
        Ext ev0, ev1;
        folded = fri_fold_step(folded, idx, ldx(qw, L.fri_off[r]), beta, lfh, L.gens, L.gens_inv, L.neg_half, ev0, ev1);
        if (lane == 0) { stx(evs, 8 * r, ev0); stx(evs, 8 * r + 4, ev1); }
        // the fold has reached 2^lfh elements: the class of that height rolls in (the fold onto the final vector included)
        if (MIXED && ((L.class_mask >> lfh) & 1u))
            folded = bb::add(folded, bb::mul(bb::sqr(beta), class_opening<WAVE, true>(a, L, i, qw, pts, alp, index, lfh, lane, step)));
        idx >>= 1;
    }
    const Ext evf = final_poly_eval(w, L.fpoly_off, L.fpl, L.gens[L.lfinal], L.lfinal, idx);
    if (lane == 0 && !bb::eq(evf, folded)) report(a, i, KEY_QUERY0 + (uint64_t)q * STEPS_PER_QUERY + 2 * (L.n_in + L.n_fri), CODE_FINAL_POLY);
}

// ---- 3. openings: one lane per (slot, member, query) ------------------------------------------------------------------------
// What one lane opens.  n_ev = 8: an FRI leaf, evs[0..8) then `salt` words at tail.  n_ev = 0: an input round's leaf over the
// matrices m0 .. m0 + nm of the layout, each followed by its salt, the words gathered from the query at qw.  Mixed heights: the
// leaf is the round's tallest class (log_big_c = depth); inj has a bit per shorter class of the round, by log_big_c.
struct LaneOpening {
    const uint32_t* evs;
    const uint32_t* qw;
    const uint32_t* tail;
    const uint32_t* path;
    const uint32_t* root;
    uint32_t n_ev, m0, nm, leaf_len, depth, index, inj;
    __device__ __forceinline__ uint32_t leaf_word(const PLayout& L, uint32_t e) const {
        if (n_ev) return e < n_ev ? evs[e] : tail[e - n_ev];
        uint32_t m = m0;
        for (uint32_t k = 1; k < nm; k++)
            if (e >= L.leaf_start[m0 + k]) m = m0 + k;
        const uint32_t c = e - L.leaf_start[m];
        return c < L.width[m] ? qw[L.val_off[m] + c] : qw[L.salt_off[m] + (c - L.width[m])];
    }
    // word e of the row of the round's class lb: the round's matrices of that height, in input order
    __device__ __forceinline__ uint32_t class_word(const PLayout& L, uint32_t lb, uint32_t e) const {
        uint32_t m = m0;
        for (uint32_t k = 0; k < nm; k++)
            if (L.log_big_m[m0 + k] == lb && e >= L.leaf_start[m0 + k]) m = m0 + k;
        const uint32_t c = e - L.leaf_start[m];  // the class's first matrix starts at 0: one of them was taken
        return c < L.width[m] ? qw[L.val_off[m] + c] : qw[L.salt_off[m] + (c - L.width[m])];
    }
    __device__ __forceinline__ uint32_t class_len(const PLayout& L, uint32_t lb) const {
        uint32_t n = 0;
        for (uint32_t k = 0; k < nm; k++)
            if (L.log_big_m[m0 + k] == lb) n += L.width[m0 + k] + L.salt;
        return n;
    }
};

// lane_walk's word source.  MIXED = false: one height class, only level 0 has a row.  MIXED = true: level l's nodes are 2^(depth - l), and
// the round's class of that height is hashed there.
template <bool MIXED>
struct OpeningWords {
    const PLayout& L;
    const LaneOpening& o;
    __device__ __forceinline__ bool has(uint32_t l) const { return l == 0 || ((o.inj >> (o.depth - l)) & 1u); }
    __device__ __forceinline__ uint32_t len(uint32_t l) const { return !MIXED || l == 0 ? o.leaf_len : o.class_len(L, o.depth - l); }
    __device__ __forceinline__ uint32_t word(uint32_t l, uint32_t e) const {
        return !MIXED || o.n_ev ? o.leaf_word(L, e) : o.class_word(L, o.depth - l, e);
    }
};

template <int HASH, bool MIXED>
__global__ void __launch_bounds__(256) pv_open_kernel(PArgs a, PLayout L) {
    const uint64_t per_slot = (uint64_t)a.n * L.nq, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per_slot * (L.n_in + L.n_fri)) return;
    const uint32_t slot = (uint32_t)(t / per_slot);
    const uint64_t pq = t % per_slot;
    const uint32_t i = (uint32_t)(pq / L.nq), q = (uint32_t)(pq % L.nq);
    if (!length_ok(a, L, i) || header_rejected(a, i)) return;
    const uint32_t* w = proof_words(a, i);
    const uint32_t* qw = w + L.q_base + (size_t)q * L.q_len;
    const uint32_t index = a.idx[pq];
    const uint64_t qkey = KEY_QUERY0 + (uint64_t)q * STEPS_PER_QUERY;
    // a word of the query the shape dictates (the host's 12), met in query order; unless the shape has `counts`: then the words wire
    // format 1's host FOLLOWS to the final polynomial (skip_queries_by_counts: the opening count, widths, depths, the round count;
    // its 7 / 8, before the proof of work) report at KEY_SHAPE
    bool shape = false, followed = false;
    LaneOpening o{};
    o.qw = qw;
    uint32_t hi = 0, code;
    if (slot < L.n_in) {
        const uint32_t m0 = L.mat0[slot], nm = L.nm[slot];
        if (slot == 0 && qw[0] != L.n_in) followed = true;
        if (qw[L.open_off[slot]] != nm) shape = true;
        for (uint32_t m = m0; m < m0 + nm; m++) {
            if (qw[L.val_off[m] - 1] != L.width[m]) followed = true;
            if (L.salt && qw[L.salt_off[m] - 1] != L.salt) shape = true;
        }
        o.depth = MIXED ? L.log_big_r[slot] : L.log_big;  // the round's own tree: the layout's word, compared with the proof's
        if (qw[L.depth_off[slot]] != o.depth) followed = true;
        o.path = qw + L.depth_off[slot] + 1;
        o.m0 = m0; o.nm = nm;
        o.leaf_len = L.leaf_len[slot];
        o.index = MIXED ? index >> (L.log_big - o.depth) : index;
        if (MIXED) o.inj = L.round_mask[slot] & ~(1u << o.depth);  // the shorter classes of the round, by log_big_c
        o.root = a.roots + ((size_t)i * L.n_in + slot) * 8;
        code = CODE_INPUT_OPENING;
    } else {
        const uint32_t r = slot - L.n_in;
        const uint32_t* p = qw + L.fri_off[r];
        if (r == 0 && qw[L.nr_off] != L.n_fri) followed = true;
        for (int c = 0; c < 4; c++) hi = max(hi, p[c]);  // the sibling: a field element of the proof
        o.evs = a.evs + (pq * L.n_fri + r) * 8;
        o.n_ev = 8;
        o.tail = p + 5;
        if (L.salt && p[4] != L.salt) shape = true;
        const uint32_t* dp = p + 4 + (L.salt ? 1 + L.salt : 0u);
        o.depth = L.log_big - 1 - r;
        if (dp[0] != o.depth) followed = true;
        o.path = dp + 1;
        o.leaf_len = 8 + L.salt;
        o.index = index >> (r + 1);
        o.root = w + 1 + 8 * r;
        code = CODE_FRI_OPENING;
    }
    // (the FRI lanes of a mixed shape take the injecting walk too, with nothing to inject: sending them to the other form puts both
    // walks into one kernel, which took the Poseidon2 form from 118 to 134 VGPRs when it was tried, below four waves per SIMD)
    OpeningWords<MIXED> src{L, o};
    const bool mismatch = lane_walk::walk<HASH, MIXED>(src, lane_walk::PathWords{o.path}, o.depth, o.index, o.root, hi);
    if (followed && L.counts) report(a, i, KEY_SHAPE, VERIFY_MALFORMED);
    if (shape || (followed && !L.counts)) report(a, i, qkey + 2 * slot, VERIFY_MALFORMED);
    if (hi >= bb::P) report(a, i, KEY_HEADER, VERIFY_MALFORMED);
    if (mismatch) report(a, i, qkey + 2 * slot + 1, code);
}

// ---- 4. order key -> status -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pv_finish_kernel(const unsigned long long* key, uint32_t n, uint32_t* status, uint32_t* d_rejected) {
    finish(key, n, status, d_rejected);
}

// ---- host: the layout of one shape ------------------------------------------------------------------------------------------
// pcs_layout (pcs_layout.hip) derives it, for this verifier and for pcs_verify_any alike: the shape gates and their messages are there, once.
// What pcs_verify_any checks on a member's values (canonical points, the LDE coset, canonical opened values) is the kernels' business; slots
// take the place of its "distinct points" rule.  Only this verifier needs a proof to fit PLayout's 32-bit words.
int make_layout(int hash, bool hiding, const FriParams& fp, const PcsShape& sh, PLayout* out) {
    if (!sh.slots) return fail(ERR_BAD_ARG, "pcs verify: null argument");
    std::string why;
    uint64_t words = 0;
    if (int rc = pcs_layout(hash, hiding, fp, sh, out, &words, &why)) return fail(rc, why);
    if (words > 0x3fffffffull) return fail(ERR_BAD_ARG, "pcs verifier: a proof of this shape exceeds 2^32 bytes");
    return OK;
}

}  // namespace

int pcs_proof_len(int hash, bool hiding, const FriParams& fp, const PcsShape& shape, size_t* len_out) {
    PLayout L;
    if (int rc = make_layout(hash, hiding, fp, shape, &L)) return rc;
    *len_out = 4 * (size_t)L.proof_words;
    return OK;
}

struct PcsVerifierDev::Impl : VerifierDevHost {
    PLayout L;
    PState* st = nullptr;
    uint32_t *idx = nullptr, *evs = nullptr, *alp = nullptr, *pa = nullptr, *pb = nullptr;
    unsigned long long* key = nullptr;
    uint32_t *d_roots = nullptr, *d_points = nullptr, *d_opened = nullptr, *d_cin = nullptr, *d_cout = nullptr;  // staging of the host entry
};

PcsVerifierDev::PcsVerifierDev() : im(new Impl()) {}
PcsVerifierDev::~PcsVerifierDev() { delete im; }
size_t PcsVerifierDev::proof_len() const { return 4 * (size_t)im->L.proof_words; }
size_t PcsVerifierDev::max_proofs() const { return im->max_proofs; }
size_t PcsVerifierDev::total_columns() const { return im->L.total; }
bool PcsVerifierDev::wave_form() const { return im->L.row_words >= PV_WAVE_MIN_COLS; }
int PcsVerifierDev::hash() const { return im->L.hash; }
int PcsVerifierDev::device() const { return im->device; }

int PcsVerifierDev::init(int hash, bool hiding, const FriParams& fp, const PcsShape& shape, size_t max_proofs) {
    if (int rc = make_layout(hash, hiding, fp, shape, &im->L)) return rc;
    const PLayout& L = im->L;
    if (max_proofs == 0) return fail(ERR_BAD_ARG, "pcs_verifier_create: max_proofs must be positive");
    // the widest grid: one wavefront per (member, query), or one lane per opening
    if (max_proofs > 0x7fffffffull || max_proofs * (uint64_t)L.nq * std::max(64u, L.n_in + L.n_fri) > 0x7fffffffull * 256ull)
        return fail(ERR_BAD_ARG, "pcs_verifier_create: max_proofs x num_queries too large");
    Context* cx = nullptr;
    if (int rc = get_context(&cx)) return rc;
    im->device = cx->device;
    im->max_proofs = max_proofs;
    return im->alloc({Impl::buf(&im->st, max_proofs * sizeof(PState)), Impl::buf(&im->idx, max_proofs * L.nq * 4),
                      Impl::buf(&im->evs, max_proofs * L.nq * (size_t)L.n_fri * 32), Impl::buf(&im->alp, max_proofs * (size_t)L.wmax * 16),
                      Impl::buf(&im->pa, max_proofs * (size_t)L.n_pairs * 16), Impl::buf(&im->pb, max_proofs * (size_t)L.n_pairs * 16),
                      Impl::buf(&im->key, max_proofs * 8)});
}

int PcsVerifierDev::verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_roots, const uint32_t* d_points,
                               const uint32_t* d_opened, const uint32_t* d_chal_in, size_t n, uint32_t* d_status, uint32_t* d_rejected,
                               uint32_t* d_chal_out, hipStream_t stream, const unsigned long long* d_owner_key) {
    const PLayout& L = im->L;
    if (int rc = im->check_batch("pcs_verifier_verify_dev", n, !d_proofs || !d_roots || !d_points || !d_opened || !d_chal_in || !d_status, stride, proof_len())) return rc;
    if (misaligned(d_proofs, 4) || misaligned(d_lens, 4) || misaligned(d_roots, 4) || misaligned(d_points, 4) || misaligned(d_opened, 4) ||
        misaligned(d_status, 4) || misaligned(d_rejected, 4))
        return fail(ERR_BAD_ARG, "pcs_verifier_verify_dev: d_proofs, d_lens, d_roots, d_points, d_opened, d_status and d_rejected must be 4-byte aligned");
    if (misaligned(d_chal_in, 8) || misaligned(d_chal_out, 8)) return fail(ERR_BAD_ARG, "pcs_verifier_verify_dev: d_chal_in and d_chal_out must be 8-byte aligned");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    if (d_rejected) P3_HIP(hipMemsetAsync(d_rejected, 0, 4, stream));
    if (!n) return OK;
    PArgs a{d_proofs, stride, d_lens, d_roots, d_points, d_opened, d_chal_in, d_chal_out, (uint32_t)n, im->st, im->idx, im->evs, im->alp, im->pa, im->pb, im->key, d_owner_key};
    hipLaunchKernelGGL(pv_transcript_kernel, dim3((uint32_t)n), dim3(64), 0, stream, a, L);
    const uint64_t pq = (uint64_t)n * L.nq;
    const dim3 qgrid((uint32_t)(wave_form() ? (pq + 3) / 4 : (pq + 255) / 256));
    if (wave_form() && L.mixed) hipLaunchKernelGGL((pv_query_kernel<true, true>), qgrid, dim3(256), 0, stream, a, L);
    else if (wave_form()) hipLaunchKernelGGL((pv_query_kernel<true, false>), qgrid, dim3(256), 0, stream, a, L);
    else if (L.mixed) hipLaunchKernelGGL((pv_query_kernel<false, true>), qgrid, dim3(256), 0, stream, a, L);
    else hipLaunchKernelGGL((pv_query_kernel<false, false>), qgrid, dim3(256), 0, stream, a, L);
    const dim3 ogrid((uint32_t)((pq * (L.n_in + L.n_fri) + 255) / 256));
    if (L.hash == HASH_KECCAK && L.mixed) hipLaunchKernelGGL((pv_open_kernel<HASH_KECCAK, true>), ogrid, dim3(256), 0, stream, a, L);
    else if (L.hash == HASH_KECCAK) hipLaunchKernelGGL((pv_open_kernel<HASH_KECCAK, false>), ogrid, dim3(256), 0, stream, a, L);
    else if (L.mixed) hipLaunchKernelGGL((pv_open_kernel<HASH_POSEIDON2, true>), ogrid, dim3(256), 0, stream, a, L);
    else hipLaunchKernelGGL((pv_open_kernel<HASH_POSEIDON2, false>), ogrid, dim3(256), 0, stream, a, L);
    hipLaunchKernelGGL(pv_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, im->key, (uint32_t)n, d_status, d_rejected);
    P3_HIP(hipGetLastError());
    return OK;
}

int PcsVerifierDev::verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* roots, const uint32_t* points,
                                const uint32_t* opened, Challenger* const* chals, uint32_t* status_out) {
    const PLayout& L = im->L;
    if (n && (!proofs || !lens || !roots || !points || !opened || !chals || !status_out)) return fail(ERR_BAD_ARG, "pcs_verifier_verify: null argument");
    for (size_t g = 0; g < n; g++) {
        if (!chals[g]) return fail(ERR_BAD_ARG, "pcs_verifier_verify: null challenger");
        if (chals[g]->kind != L.hash) return fail(ERR_BAD_ARG, "pcs verify: the challenger belongs to another hash configuration");
    }
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    const size_t plen = proof_len(), cap = im->max_proofs, SW = CHALLENGER_STATE_WORDS;
    const size_t rw = (size_t)L.n_in * 8, pw = (size_t)L.n_slots * 4, ow = (size_t)L.total * 4;
    if (int rc = im->stage(plen, {Impl::buf(&im->d_roots, cap * rw * 4), Impl::buf(&im->d_points, cap * pw * 4), Impl::buf(&im->d_opened, cap * ow * 4),
                                  Impl::buf(&im->d_cin, cap * SW * 4), Impl::buf(&im->d_cout, cap * SW * 4)}))
        return rc;
    std::vector<uint32_t> hc(cap * SW), ho(cap * SW);
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = std::min(cap, n - base);
        if (int rc = im->upload("pcs_verifier_verify", m, proofs + base, lens + base, plen)) return rc;
        for (size_t k = 0; k < m; k++) challenger_export(*chals[base + k], hc.data() + k * SW);
        P3_HIP(hipMemcpyAsync(im->d_roots, roots + base * rw, m * rw * 4, hipMemcpyHostToDevice, im->stream));
        P3_HIP(hipMemcpyAsync(im->d_points, points + base * pw, m * pw * 4, hipMemcpyHostToDevice, im->stream));
        P3_HIP(hipMemcpyAsync(im->d_opened, opened + base * ow, m * ow * 4, hipMemcpyHostToDevice, im->stream));
        P3_HIP(hipMemcpyAsync(im->d_cin, hc.data(), m * SW * 4, hipMemcpyHostToDevice, im->stream));
        if (int rc = verify_dev(im->d_proofs, plen, im->d_lens, im->d_roots, im->d_points, im->d_opened, im->d_cin, m, im->d_status, nullptr,
                                im->d_cout, im->stream))
            return rc;
        if (int rc = im->download_status(status_out + base, m)) return rc;
        P3_HIP(hipMemcpyAsync(ho.data(), im->d_cout, m * SW * 4, hipMemcpyDeviceToHost, im->stream));
        P3_HIP(hipStreamSynchronize(im->stream));
        for (size_t k = 0; k < m; k++)
            if (status_out[base + k] == 0)
                if (int rc = challenger_import(ho.data() + k * SW, chals[base + k])) return rc;
    }
    return OK;
}

}  // namespace p3
