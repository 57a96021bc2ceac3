// Batch verifier of fib_air proofs on the device: p3_uni_stark::verify + TwoAdicFriPcs / HidingFriPcs::verify + p3_fri::verifier for
// FibonacciAir (the second half of the reference's run_fib_air_zk, native/src/fib_air.rs:70-72) for MANY proofs of one configuration
// at once.  verifier.hip's verify_fib (host, one proof) is the specification, and this is built as it is: a fib_air proof is a PCS
// proof of a fixed shape behind a header, so the object is ONE front kernel over the header and an owned PcsVerifierDev
// (pcs_verifier_dev.hip) over the FRI section.  The header's layout is read from the table verify_fib reads (fib_format.h) and the FRI
// section's from pcs_layout; the constraint check is ood.hip.h's.
//
// SAFETY RULE.  NO LOAD ADDRESS AND NO LOOP BOUND DEPENDS ON A BYTE OF A PROOF OR A PUBLIC VALUE: a proof whose length differs from
// the configuration's is rejected unread, and every count word of the header is compared with the value the format dictates, never
// followed.
//
//   fv_front_kernel  one wavefront per proof: the length, the header's dictated words, canonicity of the header's field words (the roots
//                    under Poseidon2 only) and of the public values; the transcript (DevChal, transcript.hip.h) up to zeta; the
//                    constraints at zeta.  Leaves per member what the owned PCS verifier reads: the roots in proof order, the points
//                    zeta and zeta g_n, the opened values made contiguous, the exported challenger state, the length of the FRI
//                    section (0 when the whole length is wrong) -- and the member's initial order key (verifier_dev_common.hip.h):
//                    KEY_HEADER / MALFORMED (the PCS verifier then skips the member unread: nothing else is written for it),
//                    KEY_OWNER / 10, or none.
//   the owned PcsVerifierDev on d_proofs + 4 head_words, the caller's stride, the scratch lengths, the initial keys: four launches; its
//                    finish kernel writes the caller's d_status and d_rejected.
// The first failure in the HOST's order decides the code (the one scale of order keys); the plain format's shape carries
// PcsShape::counts, its host verifier's habit of following a query's count words.
// ONE DIVERGENCE from verify_fib: the PCS verifier rejects (MALFORMED) a member whose point is a base-field element on the LDE coset.
// zeta is a transcript sample: reaching this takes three zero coordinates out of a hash.
#include <cstring>
#include <memory>

#include "common.h"
#include "fib_format.h"
#include "mmcs.h"
#include "ood.hip.h"
#include "pcs_verifier_dev.h"
#include "prover.h"
#include "verifier_dev.h"
#include "verifier_dev_common.hip.h"
#include "verifier_dev_host.h"

namespace p3 {

using bb::Ext;

namespace {

using namespace vdev;

// the header of one configuration, derived from its FibFormat: the words with a dictated value (magic, version, log_n, the grammar's
// count words), the groups of opened values (canonicity; made contiguous in the format's order), where the roots lie
struct FLayout {
    int hash;
    uint32_t log_n, log_ext, n_roots, head_words, proof_words, total;
    uint32_t n_shape, shape_off[3 + FIB_MAX_GROUPS], shape_val[3 + FIB_MAX_GROUPS];
    uint32_t n_groups, group_off[FIB_MAX_GROUPS], group_len[FIB_MAX_GROUPS];  // words
    uint32_t root_of[FIB_MAX_ROUNDS];  // proof order -> header root
    uint32_t t_loc, t_nxt, chunks, chunk_stride, n_chunks;  // word offsets from the header's first opened value
    OodDomain dom;
};
constexpr uint32_t ROOT_OFF = 3;  // the header's roots follow magic, version, log_n

struct FArgs {
    const uint8_t* proofs;
    size_t stride;
    const uint32_t* lens;
    const uint32_t* pis;      // n x 3
    uint32_t* roots;          // n x n_roots x 8, proof order
    uint32_t* points;         // n x 2 x 4
    uint32_t* opened;         // n x total x 4
    uint32_t* chal;           // n x CHALLENGER_STATE_WORDS
    uint32_t* slen;           // n: byte length of the FRI section, 0 = reject unread
    unsigned long long* key;  // n: the initial order key
};

__global__ void __launch_bounds__(64) fv_front_kernel(FArgs a, FLayout L) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t* w = proof_words(a, i);
    const uint32_t* pi = a.pis + 3 * (size_t)i;
    const bool len_ok = length_ok(a, L, i);  // a proof of another length is rejected unread
    bool bad = !len_ok;
    if (len_ok) {  // every check that needs no challenge, the lanes side by side
        bool b = false;
        uint32_t hi = 0;
        for (uint32_t k = lane; k < L.n_shape; k += 64) b |= w[L.shape_off[k]] != L.shape_val[k];
        for (uint32_t g = 0; g < L.n_groups; g++)
            for (uint32_t j = lane; j < L.group_len[g]; j += 64) hi = max(hi, w[L.group_off[g] + j]);
        if (L.hash == HASH_POSEIDON2 && lane < 8 * L.n_roots) hi = max(hi, w[ROOT_OFF + lane]);
        if (lane < 3) hi = max(hi, pi[lane]);
        bad = __builtin_amdgcn_ballot_w64(b || hi >= bb::P) != 0;
    }
    if (lane == 0) a.slen[i] = len_ok ? 4u * (L.proof_words - L.head_words) : 0u;
    if (bad) {  // wave-uniform
        if (lane == 0) a.key[i] = make_key(KEY_HEADER, VERIFY_MALFORMED);
        return;
    }
    DevChal ch;
    ch.begin(L.hash, nullptr, &ks, true);
    const uint32_t pis[3] = {pi[0], pi[1], pi[2]};
    ch.observe(bb::to_monty(L.log_ext));
    ch.observe(bb::to_monty(L.log_n));
    ch.observe_n(w + ROOT_OFF, 8);
    ch.observe_n(pis, 3);
    const Ext alpha = ch.sample_ext();
    for (uint32_t r = 1; r < L.n_roots; r++) ch.observe_n(w + ROOT_OFF + 8 * r, 8);
    const Ext zeta = ch.sample_ext();
    export_challenger(ch, L.hash, a.chal + (size_t)i * CHALLENGER_STATE_WORDS, lane);
    uint32_t* opened = a.opened + (size_t)i * L.total * 4;
    for (uint32_t g = 0, to = 0; g < L.n_groups; to += L.group_len[g++])
        for (uint32_t j = lane; j < L.group_len[g]; j += 64) opened[to + j] = w[L.group_off[g] + j];
    if (lane < 8 * L.n_roots) a.roots[(size_t)i * L.n_roots * 8 + lane] = w[ROOT_OFF + 8 * L.root_of[lane >> 3] + (lane & 7u)];
    // the constraints at zeta against the quotient, from the proof's words (the opened values of the header lie in the format's order)
    const uint32_t* ow = w + L.group_off[0];
    Ext first, last, trans, zn, zh;
    ood_selectors(zeta, L.log_n, L.dom.g_n_inv, first, last, trans, zn, zh);
    const Ext folded = fib_constraints_folded(ow + L.t_loc, ow + L.t_nxt, pis, first, last, trans, alpha);
    const bool ood_ok = bb::eq(bb::mul(folded, bb::inv(zh)), ood_quotient(L.dom, L.n_chunks, zn, ow + L.chunks, L.chunk_stride));
    if (lane == 0) {
        stx(a.points, 8 * (size_t)i, zeta);
        stx(a.points, 8 * (size_t)i + 4, bb::scale(zeta, L.dom.g_n));
        a.key[i] = ood_ok ? KEY_NONE : make_key(KEY_OWNER, CODE_OOD);
    }
}

const FibFormat& format_of(bool hiding) { return hiding ? FIB_HIDING : FIB_PLAIN; }

// the parameter gates with the fib verifiers' messages, then the two layouts: pcs_layout refuses nothing verify_check_parameters admits
int make_layout(int hash, bool hiding, uint32_t log_n, const FriParams& fp, FLayout* out, PLayout* pl) {
    std::string why;
    if (verify_check_parameters(hash, hiding, log_n, fp, &why)) return fail(ERR_BAD_ARG, why);
    const FibFormat& f = format_of(hiding);
    uint64_t words = 0;
    if (int rc = pcs_layout(hash, hiding, fp, fib_pcs_shape(f, log_n), pl, &words, &why)) return fail(rc, why);
    words += head_words_of(f);
    if (words > 0x3fffffffull) return fail(ERR_BAD_ARG, "fib_verifier: a proof of this configuration exceeds 2^32 bytes");
    FLayout& L = *out;
    memset(&L, 0, sizeof(L));
    L.hash = hash;
    L.log_n = log_n;
    L.log_ext = log_n + (hiding ? 1 : 0);
    L.n_roots = f.n_rounds;
    L.head_words = head_words_of(f);
    L.proof_words = (uint32_t)words;
    L.total = opened_of(f);
    auto dictated = [&](uint32_t off, uint32_t val) { L.shape_off[L.n_shape] = off; L.shape_val[L.n_shape++] = val; };
    dictated(0, PROOF_MAGIC); dictated(1, f.version); dictated(2, log_n);
    uint32_t pos = ROOT_OFF + 8 * f.n_rounds, at[FIB_MAX_GROUPS + 1] = {0};  // at[g]: group g's first word among the opened values
    for (const int* g = f.grammar; *g; g++) {
        dictated(pos++, (uint32_t)std::abs(*g));
        if (*g < 0) continue;
        L.group_off[L.n_groups] = pos;
        L.group_len[L.n_groups] = 4 * (uint32_t)*g;
        at[L.n_groups + 1] = at[L.n_groups] + 4 * (uint32_t)*g;
        L.n_groups++;
        pos += 4 * (uint32_t)*g;
    }
    // the kernel reads the trace and the chunks where they lie in the proof, as offsets from the first opened value: an opened value k
    // of group g lies (group_off[g] - group_off[0]) - at[g] words further on than among the contiguous ones
    auto in_proof = [&](uint32_t k) {
        uint32_t g = 0;
        while (g + 1 < L.n_groups && at[g + 1] <= 4 * k) g++;
        return 4 * k - at[g] + L.group_off[g] - L.group_off[0];
    };
    L.t_loc = in_proof(f.t_loc); L.t_nxt = in_proof(f.t_nxt); L.chunks = in_proof(f.chunks);
    L.n_chunks = 1u << f.log_chunks;
    L.chunk_stride = L.n_chunks > 1 ? in_proof(f.chunks + 4) - L.chunks : 16;  // every chunk is a group of its own
    for (uint32_t r = 0; r < f.n_rounds; r++) L.root_of[r] = f.root_of[r];
    ood_domain(log_n, f.log_chunks, &L.dom);
    return OK;
}

}  // namespace

int fib_proof_len(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t* len_out) {
    FLayout L;
    PLayout pl;
    if (int rc = make_layout(hash, hiding, log_n, fp, &L, &pl)) return rc;
    *len_out = 4 * (size_t)L.proof_words;
    return OK;
}

struct FibVerifierDev::Impl : VerifierDevHost {
    FLayout L;
    PcsVerifierDev pcs;
    uint32_t *roots = nullptr, *points = nullptr, *opened = nullptr, *chal = nullptr, *slen = nullptr;
    unsigned long long* key = nullptr;
    uint32_t* d_pis = nullptr;  // staging of the host entry
};

FibVerifierDev::FibVerifierDev() : im(new Impl()) {}
FibVerifierDev::~FibVerifierDev() { delete im; }
size_t FibVerifierDev::proof_len() const { return 4 * (size_t)im->L.proof_words; }
size_t FibVerifierDev::max_proofs() const { return im->max_proofs; }
int FibVerifierDev::device() const { return im->device; }

int FibVerifierDev::init(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t max_proofs) {
    PLayout pl;
    if (int rc = make_layout(hash, hiding, log_n, fp, &im->L, &pl)) return rc;
    const FLayout& L = im->L;
    if (max_proofs == 0) return fail(ERR_BAD_ARG, "fib_verifier_create: max_proofs must be positive");
    // the owned verifier's widest grid (pcs_verifier_dev.hip), refused here in this verifier's words
    if (max_proofs > 0x7fffffffull || max_proofs * (uint64_t)pl.nq * 64u > 0x7fffffffull * 256ull)
        return fail(ERR_BAD_ARG, "fib_verifier_create: max_proofs x num_queries too large");
    if (int rc = im->pcs.init(hash, hiding, fp, fib_pcs_shape(format_of(hiding), log_n), max_proofs)) return rc;
    Context* cx = nullptr;
    if (int rc = get_context(&cx)) return rc;
    im->device = cx->device;
    im->max_proofs = max_proofs;
    return im->alloc({Impl::buf(&im->roots, max_proofs * (size_t)L.n_roots * 32), Impl::buf(&im->points, max_proofs * 32),
                      Impl::buf(&im->opened, max_proofs * (size_t)L.total * 16), Impl::buf(&im->chal, max_proofs * (size_t)CHALLENGER_STATE_WORDS * 4),
                      Impl::buf(&im->slen, max_proofs * 4), Impl::buf(&im->key, max_proofs * 8)});
}

int FibVerifierDev::verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_pis, size_t n,
                               uint32_t* d_status, uint32_t* d_rejected, hipStream_t stream) {
    const FLayout& L = im->L;
    if (int rc = im->check_batch("fib_verifier_verify_dev", n, !d_proofs || !d_pis || !d_status, stride, proof_len())) return rc;
    if (misaligned(d_proofs, 4)) return fail(ERR_BAD_ARG, "fib_verifier_verify_dev: d_proofs must be 4-byte aligned");
    if (misaligned(d_lens, 4) || misaligned(d_pis, 4) || misaligned(d_status, 4) || misaligned(d_rejected, 4))
        return fail(ERR_BAD_ARG, "fib_verifier_verify_dev: d_lens, d_pis, d_status and d_rejected must be 4-byte aligned");
    DeviceScope ds(im->device);
    if (int rc = ds.enter()) return rc;
    if (n) {
        FArgs a{d_proofs, stride, d_lens, d_pis, im->roots, im->points, im->opened, im->chal, im->slen, im->key};
        hipLaunchKernelGGL(fv_front_kernel, dim3((uint32_t)n), dim3(64), 0, stream, a, L);
        P3_HIP(hipGetLastError());
    }
    return im->pcs.verify_dev(d_proofs + 4 * (size_t)L.head_words, stride, im->slen, im->roots, im->points, im->opened, im->chal, n, d_status,
                              d_rejected, nullptr, stream, im->key);
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
