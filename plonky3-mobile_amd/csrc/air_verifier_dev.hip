// p3_uni_stark::verify for a caller-defined AIR (air.h): ONE proof on the host (air_verify: plonky3-mobile_amd/air.py verify_air
// restated step for step, the specification of everything below) and BATCHES of proofs of one (AIR, log_n, FRI parameters, hash) on
// the device (AirVerifierDev).  The structure is verifier_dev.hip's (a front over the header); the PCS half IS pcs_verifier_dev.hip:
// the object owns a PcsVerifierDev of the shape a prove_air proof has and hands it each member's roots, points, opened values and
// challenger state in device memory.
//
// A proof is the header (magic, 1, log_n, the two roots, width and the local values, width and the next values, the chunk count and
// per chunk 4 and its 16 words) and the PCS's FriProof section.  All proofs of one configuration have one layout: AvLayout is
// computed on the host when the verifier is created and passed to the kernels by value; the words with a dictated value (the
// header's and the FRI section's, walked from the PCS layout) are a table in device memory made at the same time.
//
// SAFETY RULE.  NO LOAD ADDRESS, NO LDS INDEX AND NO LOOP BOUND DEPENDS ON A PROOF BYTE, A PUBLIC VALUE OR A CHALLENGE.  A proof
// whose length differs from the configuration's is rejected unread; every count / width / depth word is compared with the value the
// shape dictates and never followed; slot, column, public and constant indices come from the program that air_create validated.
//
//   av_transcript_kernel  one wavefront per member: the length, every dictated word, canonicity of the header's field words (the
//                         roots under Poseidon2 only) and of the public values; then DevChal from a fresh state: log_n, log_n, the
//                         trace root, the publics, alpha, the quotient root, zeta.  Leaves per member what the owned PCS verifier
//                         reads — the 2 x 8 root words, the points zeta and zeta g_n, the opened values made contiguous (local |
//                         next | chunks), the exported challenger state, the length of the FRI section (0 when the whole length is
//                         wrong: the PCS verifier then rejects the member unread) — and alpha.  A header-rejected member gets
//                         all-zero roots, points, opened values and state (zero counters are in range).
//   av_eval_kernel        one LANE per member, 64-lane workgroups: the selectors at zeta (ood.hip.h), the program over bb::Ext operands with
//                         Horner's fold by alpha (air_eval_core, air.hip's air_kernel restated for extension operands: program,
//                         constants and opcode / kind dispatch wave-uniform, the value slots in dynamic LDS, slot-major, (slot 4 +
//                         coefficient) 64 + lane, 1 KiB per slot), the quotient recomposed from its chunks; folded != quotient(zeta)
//                         Z_H(zeta) is recorded as "OOD failed" in a per-member word.
//   the owned PcsVerifierDev on d_proofs + 4 head_words, the caller's stride, the scratch lengths: four launches, status to scratch.
//   av_finish_kernel      MALFORMED if the front or the PCS says so, else 10 if the OOD check failed, else the PCS status; counts the
//                         rejected members.
// A MEMBER WHOSE HEADER VALUES FAIL THE OOD CHECK AND WHOSE FRI SECTION IS MALFORMED IS MALFORMED: the host stops at 10 there and never
// looks at the FRI section.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "air_verifier_dev.h"
#include "challenger.h"
#include "common.h"
#include "mmcs.h"
#include "ood.hip.h"
#include "pcs_layout.h"
#include "pcs_verifier_dev.h"
#include "verifier_dev_common.hip.h"
#include "verifier_dev_host.h"

namespace p3 {

using bb::Ext;

namespace {

using namespace vdev;

constexpr uint32_t AV_BLOCK = 64;  // lanes per workgroup of the evaluator: a value slot costs 4 x 64 x 4 = 1 KiB of LDS
static_assert(P3HIP_AIR_MAX_SLOTS * 4 * AV_BLOCK * 4 <= 64 * 1024, "the slots of the largest program fit a workgroup's 64 KiB");
constexpr uint32_t OPND_INDEX_MASK = (1u << P3HIP_AIR_KIND_SHIFT) - 1u;
constexpr size_t EVAL_MANY_MAX = (size_t)1 << 20;

// ---- the interpreter over extension operands (VerifierConstraintFolder).  Operands are read where they lie: local and next as 4
// words per column, publics and constants lifted from base words, the selectors from registers.  `Slots` holds the value slots: LDS
// on the device (never a per-thread array, which would be placed in scratch), a vector on the host. ----
struct ExtOperands {
    const uint32_t *local, *next, *pis, *consts;
    Ext first, last, trans;
};
struct LdsSlots {  // slot-major: consecutive lanes on consecutive banks
    uint32_t* my;  // the workgroup's slots + the lane
    __device__ __forceinline__ Ext get(uint32_t s) const {
        const uint32_t* p = my + s * 4 * AV_BLOCK;
        return Ext{{p[0], p[AV_BLOCK], p[2 * AV_BLOCK], p[3 * AV_BLOCK]}};
    }
    __device__ __forceinline__ void set(uint32_t s, const Ext& v) const {
        uint32_t* p = my + s * 4 * AV_BLOCK;
        for (int c = 0; c < 4; c++) p[c * AV_BLOCK] = v.c[c];
    }
};
struct HostSlots {
    Ext* s;
    Ext get(uint32_t i) const { return s[i]; }
    void set(uint32_t i, const Ext& v) const { s[i] = v; }
};
// (every operand source is a parameter BY VALUE: a selector chosen through a reference to a struct becomes a load at a chosen address,
// and the struct then lives in scratch)
template <class Slots>
BB_HD Ext av_fetch(uint32_t o, const uint32_t* local, const uint32_t* next, const uint32_t* pis, const uint32_t* consts, Ext first, Ext last, Ext trans,
                   Slots slots) {
    const uint32_t idx = o & OPND_INDEX_MASK;
    switch (o >> P3HIP_AIR_KIND_SHIFT) {  // wave-uniform: o comes from the program
        case P3HIP_AIR_KIND_SLOT: return slots.get(idx);
        case P3HIP_AIR_KIND_LOCAL: { const uint32_t* p = local + 4 * (size_t)idx; return Ext{{p[0], p[1], p[2], p[3]}}; }
        case P3HIP_AIR_KIND_NEXT: { const uint32_t* p = next + 4 * (size_t)idx; return Ext{{p[0], p[1], p[2], p[3]}}; }
        case P3HIP_AIR_KIND_PUBLIC: return bb::ext_from_base(pis[idx]);
        case P3HIP_AIR_KIND_CONST: return bb::ext_from_base(consts[idx]);
        default: return idx == P3HIP_AIR_SEL_FIRST_ROW ? first : idx == P3HIP_AIR_SEL_LAST_ROW ? last : trans;
    }
}
template <class Slots>
BB_HD Ext air_eval_core(const uint32_t* __restrict__ code, uint32_t n_instr, const ExtOperands& x, Slots slots, Ext alpha) {
    const uint32_t *local = x.local, *next = x.next, *pis = x.pis, *consts = x.consts;
    const Ext first = x.first, last = x.last, trans = x.trans;
    Ext acc = bb::ext_zero();
    for (uint32_t pc = 0; pc < n_instr; pc++) {
        const uint32_t op = code[4 * (size_t)pc], dst = code[4 * (size_t)pc + 1], oa = code[4 * (size_t)pc + 2], ob = code[4 * (size_t)pc + 3];
        const Ext va = av_fetch(oa, local, next, pis, consts, first, last, trans, slots);
        if (op == P3HIP_AIR_OP_ASSERT_ZERO) {
            acc = bb::add(bb::mul(acc, alpha), va);  // Horner: the first constraint takes the highest power
            continue;
        }
        const Ext vb = av_fetch(ob, local, next, pis, consts, first, last, trans, slots);  // both operands are read before dst is written: dst may be an operand's slot
        slots.set(dst, op == P3HIP_AIR_OP_MUL ? bb::mul(va, vb) : op == P3HIP_AIR_OP_ADD ? bb::add(va, vb) : bb::sub(va, vb));
    }
    return acc;
}

// ---- the layout of one configuration ----
struct AvLayout {
    int hash;
    uint32_t log_n, width, n_public, n_chunks, n_instr;
    uint32_t head_words, proof_words, total;  // total: opened extension elements of a member, 2 width + 4 n_chunks
    uint32_t root_off, local_off, next_off, chunk0_off;  // the roots are adjacent; chunk c's values at chunk0_off + 17 c
    uint32_t n_shape;  // entries of the table of dictated words
    OodDomain dom;
};

struct AvArgs {
    const uint8_t* proofs;
    size_t stride;
    const uint32_t* lens;
    const uint32_t* pis;     // n x n_public
    uint32_t n;
    const uint32_t* code;    // the verifier's copy of the program
    const uint32_t* consts;
    const uint32_t* shape;   // n_shape x (word offset, dictated value)
    uint32_t* roots;         // n x 2 x 8
    uint32_t* points;        // n x 2 x 4
    uint32_t* opened;        // n x total x 4
    uint32_t* chal;          // n x CHALLENGER_STATE_WORDS
    uint32_t* alpha;         // n x 4
    uint32_t* slen;          // n: byte length of the FRI section, 0 = reject unread
    uint32_t* front;         // n: 1 = the header is malformed
    uint32_t* ood;           // n: 1 = the OOD check failed
    uint32_t* pcs_status;    // n
};

// ---- 1. transcript: one wavefront per member ----
__global__ void __launch_bounds__(64) av_transcript_kernel(AvArgs a, AvLayout L) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    uint32_t* roots = a.roots + (size_t)i * 16;
    uint32_t* points = a.points + (size_t)i * 8;
    uint32_t* opened = a.opened + (size_t)i * L.total * 4;
    uint32_t* chal = a.chal + (size_t)i * CHALLENGER_STATE_WORDS;
    const uint32_t* pis = a.pis + (size_t)i * L.n_public;
    const uint32_t* w = proof_words(a, i);
    const bool len_ok = length_ok(a, L, i);  // a proof of another length is rejected unread
    bool bad = !len_ok;
    if (len_ok) {  // every check that needs no challenge, the lanes side by side
        bool b = false;
        uint32_t hi = 0;
        for (uint32_t k = lane; k < L.n_shape; k += 64) b |= w[a.shape[2 * k]] != a.shape[2 * k + 1];
        for (uint32_t j = lane; j < 4 * L.width; j += 64) hi = max(hi, max(w[L.local_off + j], w[L.next_off + j]));
        for (uint32_t j = lane; j < 16 * L.n_chunks; j += 64) hi = max(hi, w[L.chunk0_off + 17 * (j >> 4) + (j & 15u)]);
        if (L.hash == HASH_POSEIDON2 && lane < 16) hi = max(hi, w[L.root_off + lane]);
        for (uint32_t j = lane; j < L.n_public; j += 64) hi = max(hi, pis[j]);
        bad = __builtin_amdgcn_ballot_w64(b || hi >= bb::P) != 0;
    }
    if (lane == 0) {
        a.slen[i] = len_ok ? 4u * (L.proof_words - L.head_words) : 0u;
        a.front[i] = bad ? 1u : 0u;
    }
    if (bad) {  // wave-uniform
        if (lane < 16) roots[lane] = 0u;
        if (lane < 8) points[lane] = 0u;
        if (lane < 4) a.alpha[4 * (size_t)i + lane] = 0u;
        for (uint32_t j = lane; j < 4 * L.total; j += 64) opened[j] = 0u;
        for (uint32_t j = lane; j < CHALLENGER_STATE_WORDS; j += 64) chal[j] = 0u;
        return;
    }
    DevChal ch;
    ch.begin(L.hash, nullptr, &ks, true);
    const uint32_t m = bb::to_monty(L.log_n);
    ch.observe(m);  // log_ext_degree, log_degree
    ch.observe(m);
    ch.observe_n(w + L.root_off, 8);
    ch.observe_n(pis, L.n_public);
    const Ext alpha = ch.sample_ext();
    ch.observe_n(w + L.root_off + 8, 8);
    const Ext zeta = ch.sample_ext();
    export_challenger(ch, L.hash, chal, lane);
    if (lane == 0) {
        stx(points, 0, zeta);
        stx(points, 4, bb::scale(zeta, L.dom.g_n));
        stx(a.alpha, 4 * (size_t)i, alpha);
    }
    if (lane < 16) roots[lane] = w[L.root_off + lane];
    for (uint32_t j = lane; j < 4 * L.width; j += 64) {
        opened[j] = w[L.local_off + j];
        opened[4 * L.width + j] = w[L.next_off + j];
    }
    for (uint32_t j = lane; j < 16 * L.n_chunks; j += 64) opened[8 * L.width + j] = w[L.chunk0_off + 17 * (j >> 4) + (j & 15u)];
}

// ---- 2. the constraints at zeta against the quotient: one lane per member ----
__global__ void __launch_bounds__(AV_BLOCK) av_eval_kernel(AvArgs a, AvLayout L) {
    extern __shared__ uint32_t av_slots[];
    const uint32_t i = blockIdx.x * AV_BLOCK + threadIdx.x;
    if (i >= a.n) return;  // no barrier below: a lane's slots are its own
    const uint32_t* op = a.opened + (size_t)i * L.total * 4;
    const Ext zeta = ldx(a.points, 8 * (size_t)i), alpha = ldx(a.alpha, 4 * (size_t)i);
    ExtOperands x;
    x.local = op;
    x.next = op + 4 * (size_t)L.width;
    x.pis = a.pis + (size_t)i * L.n_public;
    x.consts = a.consts;
    Ext zn, zh;
    ood_selectors(zeta, L.log_n, L.dom.g_n_inv, x.first, x.last, x.trans, zn, zh);
    const Ext folded = air_eval_core(a.code, L.n_instr, x, LdsSlots{av_slots + threadIdx.x}, alpha);
    a.ood[i] = bb::eq(folded, bb::mul(ood_quotient(L.dom, L.n_chunks, zn, op + 8 * (size_t)L.width), zh)) ? 0u : 1u;
}

// the interpreter alone at n caller points (p3hip_air_eval_ext_dev)
struct EvalManyArgs {
    const uint32_t *code, *consts, *local, *next, *pis, *sels, *alpha;
    uint32_t* out;
    uint32_t n, n_instr, width, n_public;
};
__global__ void __launch_bounds__(AV_BLOCK) air_eval_many_kernel(EvalManyArgs a) {
    extern __shared__ uint32_t av_slots[];
    const uint32_t i = blockIdx.x * AV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    ExtOperands x;
    x.local = a.local + (size_t)i * 4 * a.width;
    x.next = a.next + (size_t)i * 4 * a.width;
    x.pis = a.pis + (size_t)i * a.n_public;
    x.consts = a.consts;
    x.first = ldx(a.sels, 12 * (size_t)i);
    x.last = ldx(a.sels, 12 * (size_t)i + 4);
    x.trans = ldx(a.sels, 12 * (size_t)i + 8);
    stx(a.out, 4 * (size_t)i, air_eval_core(a.code, a.n_instr, x, LdsSlots{av_slots + threadIdx.x}, ldx(a.alpha, 4 * (size_t)i)));
}

// ---- 4. the two results -> status ----
__global__ void __launch_bounds__(256) av_finish_kernel(AvArgs a, uint32_t* status, uint32_t* d_rejected) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < a.n;
    uint32_t st = 0;
    if (act) {
        const uint32_t pcs = a.pcs_status[i];
        st = (a.front[i] || pcs == VERIFY_MALFORMED) ? VERIFY_MALFORMED : a.ood[i] ? CODE_OOD : pcs;
        status[i] = st;
    }
    count_rejected(st != 0u, d_rejected);
}

// ---- host: gates, shape, layout ----
std::string log_n_gate(const char* who, uint32_t lqd) {
    return std::string(who) + ": log_n must lie in 1.." + std::to_string(bb::TWO_ADICITY - lqd) + " for this AIR (the quotient domain has 2^(log_n + " +
           std::to_string(lqd) + ") points)";
}

// the PCS shape of a prove_air proof: the trace opened at [zeta, zeta g_n] (slots 0, 1), every chunk at [zeta] (slot 0)
struct AirPcsShape {
    size_t mats[2], widths[1 + AIR_MAX_CHUNKS], npts[1 + AIR_MAX_CHUNKS];
    uint32_t slots[2 + AIR_MAX_CHUNKS];
    PcsShape sh;
    AirPcsShape(const Air& a, uint32_t log_n) {
        const uint32_t C = 1u << a.log_quotient_degree;
        mats[0] = 1; mats[1] = C;
        widths[0] = a.width; npts[0] = 2; slots[0] = 0; slots[1] = 1;
        for (uint32_t c = 0; c < C; c++) { widths[1 + c] = 4; npts[1 + c] = 1; slots[2 + c] = 0; }
        sh = PcsShape{log_n, 2, mats, widths, npts, 2, slots, nullptr};
    }
    AirPcsShape(const AirPcsShape&) = delete;
};

uint32_t head_words_of(const Air& a) { return 3 + 16 + 2 * (1 + 4 * a.width) + 1 + 17 * (1u << a.log_quotient_degree); }

// the AIR's two gates, then the PCS verifier's (pcs_layout, with its messages): *pl the PCS layout, *words the whole proof's length
int av_gates(const char* who, const Air& a, int hash, uint32_t log_n, const FriParams& fp, PLayout* pl, uint64_t* words) {
    const uint32_t lqd = a.log_quotient_degree;
    if (log_n < 1 || log_n > bb::TWO_ADICITY - lqd) return fail(ERR_BAD_ARG, log_n_gate(who, lqd));
    if (fp.log_blowup < lqd)
        return fail(ERR_BAD_ARG, std::string(who) + ": log_blowup " + std::to_string(fp.log_blowup) + " is below the AIR's log_quotient_degree " + std::to_string(lqd));
    AirPcsShape s(a, log_n);
    std::string why;
    uint64_t pw = 0;
    if (int rc = pcs_layout(hash, false, fp, s.sh, pl, &pw, &why)) return fail(rc, why);
    *words = pw + head_words_of(a);
    return OK;
}

// every word of a proof whose value the configuration dictates, as (word offset, value): the header's, then the FRI section's walked
// from the PCS layout (the words pcs_verifier_dev.hip compares one by one in its kernels)
std::vector<uint32_t> dictated_words(const Air& a, uint32_t log_n, const PLayout& P) {
    std::vector<uint32_t> t;
    auto put = [&](uint32_t off, uint32_t val) { t.push_back(off); t.push_back(val); };
    const uint32_t w = a.width, C = 1u << a.log_quotient_degree, head = head_words_of(a);
    put(0, PROOF_MAGIC); put(1, 1); put(2, log_n);
    put(19, w); put(20 + 4 * w, w); put(21 + 8 * w, C);
    for (uint32_t c = 0; c < C; c++) put(22 + 8 * w + 17 * c, 4);
    put(head, P.n_fri); put(head + P.nq_off, P.nq); put(head + P.fpl_off, P.fpl);
    for (uint32_t q = 0; q < P.nq; q++) {
        const uint32_t qb = head + P.q_base + q * P.q_len;
        put(qb, P.n_in);
        for (uint32_t r = 0; r < P.n_in; r++) {
            put(qb + P.open_off[r], P.nm[r]);
            for (uint32_t m = P.mat0[r]; m < P.mat0[r] + P.nm[r]; m++) put(qb + P.val_off[m] - 1, P.width[m]);
            put(qb + P.depth_off[r], P.log_big);
        }
        put(qb + P.nr_off, P.n_fri);
        for (uint32_t r = 0; r < P.n_fri; r++) put(qb + P.fri_off[r] + 4, P.log_big - 1 - r);
    }
    return t;
}

}  // namespace

int air_proof_len(const Air& a, int hash, uint32_t log_n, const FriParams& fp, size_t* len_out) {
    PLayout pl;
    uint64_t words = 0;
    if (int rc = av_gates("air_proof_len", a, hash, log_n, fp, &pl, &words)) return rc;
    *len_out = 4 * (size_t)words;
    return OK;
}

int air_verify(const Air& a, int hash, uint32_t log_n, const FriParams& fp, const uint8_t* proof, size_t len, const uint32_t* pis, std::string* why) {
    auto bad = [&](const std::string& msg) { *why = msg; return (int)ERR_BAD_ARG; };
    auto reject = [&](int code, const char* msg) { *why = msg; return code; };
    const uint32_t w = a.width, lqd = a.log_quotient_degree, C = 1u << lqd;
    if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return bad("air_verify: unknown hash configuration");
    if (log_n < 1 || log_n > bb::TWO_ADICITY - lqd) return bad(log_n_gate("air_verify", lqd));
    for (uint32_t k = 0; k < a.n_public; k++)
        if (pis[k] >= bb::P) return bad("air_verify: public value " + std::to_string(k) + " is not a canonical field element");
    // the header: every count is compared with the AIR's own, none is followed.  Past the end no count and no version matches.
    const size_t nw = len / 4, head = head_words_of(a);
    size_t pos = 0;
    bool truncated = false;
    auto word = [&](size_t k) { uint32_t v; memcpy(&v, proof + 4 * k, 4); return v; };
    auto u32 = [&]() -> int64_t {
        pos++;
        if (pos > nw) { truncated = true; return -1; }
        return word(pos - 1);
    };
    auto take = [&](uint32_t* dst, size_t n) {
        for (size_t k = 0; k < n; k++) dst[k] = pos + k < nw ? word(pos + k) : 0u;
        if (pos + n > nw) truncated = true;
        pos += n;
    };
    if (u32() != PROOF_MAGIC || u32() != 1) return reject(1, "bad magic or version");
    if (u32() != log_n) return reject(2, "log_n differs");
    uint32_t roots[16];
    take(roots, 16);
    std::vector<uint32_t> opened(4 * (2 * (size_t)w + 4 * C));
    if (u32() != w) return reject(3, "local values: the count is not the AIR's width");
    take(opened.data(), 4 * (size_t)w);
    if (u32() != w) return reject(3, "next values: the count is not the AIR's width");
    take(opened.data() + 4 * (size_t)w, 4 * (size_t)w);
    if (u32() != C) return reject(3, "quotient chunks: the count is not the AIR's");
    for (uint32_t c = 0; c < C; c++) {
        if (u32() != 4) return reject(3, "a quotient chunk's width is not 4");
        take(opened.data() + 8 * (size_t)w + 16 * c, 16);
    }
    if (truncated) return reject(4, "truncated header");
    bool canon = true;
    for (uint32_t v : opened) canon &= v < bb::P;
    if (hash == HASH_POSEIDON2)
        for (uint32_t v : roots) canon &= v < bb::P;
    if (!canon) return reject(4, "a header word is not a canonical field element");
    Challenger ch(hash);
    const uint32_t m = bb::to_monty(log_n);
    ch.observe(m);  // log_ext_degree, log_degree
    ch.observe(m);
    ch.observe_digest(roots);
    ch.observe_n(pis, a.n_public);
    const Ext alpha = ch.sample_ext();
    ch.observe_digest(roots + 8);
    const Ext zeta = ch.sample_ext();
    OodDomain dom;
    ood_domain(log_n, lqd, &dom);
    ExtOperands x;
    x.local = opened.data();
    x.next = opened.data() + 4 * (size_t)w;
    x.pis = pis;
    x.consts = a.consts.data();
    Ext zn, zh;
    ood_selectors(zeta, log_n, dom.g_n_inv, x.first, x.last, x.trans, zn, zh);
    std::vector<Ext> slots(a.n_slots, bb::ext_zero());
    const Ext folded = air_eval_core(a.code.data(), (uint32_t)(a.code.size() / 4), x, HostSlots{slots.data()}, alpha);
    if (!bb::eq(folded, bb::mul(ood_quotient(dom, C, zn, opened.data() + 8 * (size_t)w), zh))) return reject(CODE_OOD, "OodEvaluationMismatch");
    AirPcsShape s(a, log_n);
    uint32_t points[4 * (2 + AIR_MAX_CHUNKS)];
    const Ext zeta_next = bb::scale(zeta, dom.g_n);
    memcpy(points, zeta.c, 16);
    memcpy(points + 4, zeta_next.c, 16);
    for (uint32_t c = 0; c < C; c++) memcpy(points + 8 + 4 * c, zeta.c, 16);
    return pcs_verify(hash, fp, log_n, roots, s.mats, s.widths, 2, s.npts, points, opened.data(), proof + 4 * head, len - 4 * head, &ch, why);
}

int air_eval_ext_dev(Air& a, hipStream_t stream, const uint32_t* d_local, const uint32_t* d_next, const uint32_t* d_pis, const uint32_t* d_sels,
                     const uint32_t* d_alpha, size_t n, uint32_t* d_out) {
    if (n > EVAL_MANY_MAX) return fail(ERR_BAD_ARG, "air_eval_ext_dev: " + std::to_string(n) + " points, at most 2^20 a call");
    if (!n) return OK;
    if (!d_local || !d_next || !d_sels || !d_alpha || !d_out || (!d_pis && a.n_public)) return fail(ERR_BAD_ARG, "air_eval_ext_dev: null argument");
    for (const void* p : {(const void*)d_local, (const void*)d_next, (const void*)d_pis, (const void*)d_sels, (const void*)d_alpha, (const void*)d_out})
        if ((uintptr_t)p & 3) return fail(ERR_BAD_ARG, "air_eval_ext_dev: every buffer must be 4-byte aligned");
    if (int rc = air_ensure_device(a)) return rc;
    DeviceScope ds(a.device);
    if (int rc = ds.enter()) return rc;
    Context* cx = nullptr;
    if (int rc = get_context(&cx)) return rc;
    if (int rc = cx->ensure_dynamic_lds(reinterpret_cast<const void*>(&air_eval_many_kernel), P3HIP_AIR_MAX_SLOTS * 4 * AV_BLOCK * 4)) return rc;
    EvalManyArgs e{a.d_code, a.d_consts, d_local, d_next, d_pis, d_sels, d_alpha, d_out, (uint32_t)n, (uint32_t)(a.code.size() / 4), a.width, a.n_public};
    hipLaunchKernelGGL(air_eval_many_kernel, dim3((uint32_t)((n + AV_BLOCK - 1) / AV_BLOCK)), dim3(AV_BLOCK), a.n_slots * 4 * AV_BLOCK * 4, stream, e);
    P3_HIP(hipGetLastError());
    return OK;
}

struct AirVerifierDev::Impl : VerifierDevHost {
    AvLayout L;
    uint32_t n_slots = 0;
    PcsVerifierDev pcs;
    uint32_t *code = nullptr, *consts = nullptr, *shape = nullptr;  // device copies made by init
    uint32_t *roots = nullptr, *points = nullptr, *opened = nullptr, *chal = nullptr, *alpha = nullptr, *slen = nullptr, *front = nullptr, *ood = nullptr,
             *pcs_status = nullptr;
    uint32_t* d_pis = nullptr;  // staging of the host entry
};

AirVerifierDev::AirVerifierDev() : im(new Impl()) {}
AirVerifierDev::~AirVerifierDev() { delete im; }
size_t AirVerifierDev::proof_len() const { return 4 * (size_t)im->L.proof_words; }
size_t AirVerifierDev::max_proofs() const { return im->max_proofs; }
int AirVerifierDev::device() const { return im->device; }

int AirVerifierDev::init(const Air& a, int hash, uint32_t log_n, const FriParams& fp, size_t max_proofs) {
    PLayout pl;
    uint64_t words = 0;
    if (int rc = av_gates("air_verifier_create", a, hash, log_n, fp, &pl, &words)) return rc;
    if (words > 0x3fffffffull) return fail(ERR_BAD_ARG, "air_verifier_create: a proof of this configuration exceeds 2^32 bytes");
    if (max_proofs == 0) return fail(ERR_BAD_ARG, "air_verifier_create: max_proofs must be positive");
    AvLayout& L = im->L;
    memset(&L, 0, sizeof(L));
    const uint32_t w = a.width, C = 1u << a.log_quotient_degree;
    L.hash = hash;
    L.log_n = log_n; L.width = w; L.n_public = a.n_public; L.n_chunks = C; L.n_instr = (uint32_t)(a.code.size() / 4);
    L.head_words = head_words_of(a);
    L.proof_words = (uint32_t)words;
    L.total = 2 * w + 4 * C;
    L.root_off = 3; L.local_off = 20; L.next_off = 21 + 4 * w; L.chunk0_off = 23 + 8 * w;
    ood_domain(log_n, a.log_quotient_degree, &L.dom);
    im->n_slots = a.n_slots;
    const std::vector<uint32_t> shape = dictated_words(a, log_n, pl);
    L.n_shape = (uint32_t)(shape.size() / 2);
    AirPcsShape s(a, log_n);
    if (int rc = im->pcs.init(hash, false, fp, s.sh, max_proofs)) return rc;  // gates max_proofs x num_queries
    Context* cx = nullptr;
    if (int rc = get_context(&cx)) return rc;
    im->device = cx->device;
    im->max_proofs = max_proofs;
    if (int rc = cx->ensure_dynamic_lds(reinterpret_cast<const void*>(&av_eval_kernel), P3HIP_AIR_MAX_SLOTS * 4 * AV_BLOCK * 4)) return rc;
    const size_t code_b = std::max<size_t>(a.code.size(), 1) * 4, const_b = std::max<size_t>(a.consts.size(), 1) * 4;
    if (int rc = im->alloc({Impl::buf(&im->code, code_b), Impl::buf(&im->consts, const_b), Impl::buf(&im->shape, shape.size() * 4),
                            Impl::buf(&im->roots, max_proofs * 64), Impl::buf(&im->points, max_proofs * 32),
                            Impl::buf(&im->opened, max_proofs * (size_t)L.total * 16), Impl::buf(&im->chal, max_proofs * (size_t)CHALLENGER_STATE_WORDS * 4),
                            Impl::buf(&im->alpha, max_proofs * 16), Impl::buf(&im->slen, max_proofs * 4), Impl::buf(&im->front, max_proofs * 4),
                            Impl::buf(&im->ood, max_proofs * 4), Impl::buf(&im->pcs_status, max_proofs * 4)}))
        return rc;
    if (!a.code.empty()) P3_HIP(hipMemcpy(im->code, a.code.data(), a.code.size() * 4, hipMemcpyHostToDevice));
    if (!a.consts.empty()) P3_HIP(hipMemcpy(im->consts, a.consts.data(), a.consts.size() * 4, hipMemcpyHostToDevice));
    P3_HIP(hipMemcpy(im->shape, shape.data(), shape.size() * 4, hipMemcpyHostToDevice));
    return OK;
}

int AirVerifierDev::verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_pis, size_t n, uint32_t* d_status,
                               uint32_t* d_rejected, hipStream_t stream) {
    const AvLayout& L = im->L;
    if (int rc = im->check_batch("air_verifier_verify_dev", n, !d_proofs || !d_status || (!d_pis && L.n_public), stride, proof_len())) return rc;
    if (misaligned(d_proofs, 4) || misaligned(d_lens, 4) || misaligned(d_pis, 4) || misaligned(d_status, 4) || misaligned(d_rejected, 4))
        return fail(ERR_BAD_ARG, "air_verifier_verify_dev: d_proofs, d_lens, d_pis, d_status and d_rejected must be 4-byte aligned");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    if (d_rejected) P3_HIP(hipMemsetAsync(d_rejected, 0, 4, stream));
    if (!n) return OK;
    AvArgs a{d_proofs, stride, d_lens, d_pis, (uint32_t)n, im->code, im->consts, im->shape, im->roots, im->points, im->opened, im->chal,
             im->alpha, im->slen, im->front, im->ood, im->pcs_status};
    hipLaunchKernelGGL(av_transcript_kernel, dim3((uint32_t)n), dim3(64), 0, stream, a, L);
    hipLaunchKernelGGL(av_eval_kernel, dim3((uint32_t)((n + AV_BLOCK - 1) / AV_BLOCK)), dim3(AV_BLOCK), im->n_slots * 4 * AV_BLOCK * 4, stream, a, L);
    P3_HIP(hipGetLastError());
    if (int rc = im->pcs.verify_dev(d_proofs + 4 * (size_t)L.head_words, stride, im->slen, im->roots, im->points, im->opened, im->chal, n,
                                    im->pcs_status, nullptr, nullptr, stream))
        return rc;
    hipLaunchKernelGGL(av_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, a, d_status, d_rejected);
    P3_HIP(hipGetLastError());
    return OK;
}

int AirVerifierDev::verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* pis, uint32_t* status_out) {
    const uint32_t np = im->L.n_public;
    if (n && (!proofs || !lens || !status_out || (!pis && np))) return fail(ERR_BAD_ARG, "air_verifier_verify: null argument");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    const size_t plen = proof_len(), cap = im->max_proofs;
    if (int rc = im->stage(plen, {Impl::buf(&im->d_pis, std::max<size_t>(cap * np, 1) * 4)})) return rc;
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = std::min(cap, n - base);
        if (int rc = im->upload("air_verifier_verify", m, proofs + base, lens + base, plen)) return rc;
        if (np) P3_HIP(hipMemcpyAsync(im->d_pis, pis + base * np, m * np * 4, hipMemcpyHostToDevice, im->stream));
        if (int rc = verify_dev(im->d_proofs, plen, im->d_lens, np ? im->d_pis : nullptr, m, im->d_status, nullptr, im->stream)) return rc;
        if (int rc = im->download_status(status_out + base, m)) return rc;
        P3_HIP(hipStreamSynchronize(im->stream));
    }
    return OK;
}

}  // namespace p3
