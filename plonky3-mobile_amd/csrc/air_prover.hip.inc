// AirProver (prover.h): p3_uni_stark::prove for a caller-defined AIR in one device-resident launch chain.  Included by pcs.hip.inc
// (prover.hip's translation unit): ProverCore, the transcript kernels and the PCS open's kernels are shared, none is restated.
//
// The chain on the prover's stream, for a trace of n = 2^log_n rows, C = 2^log_quotient_degree chunks, K constraints:
//   1  ntt_coset_lde(trace) -> lde_t; ProverCore::commit -> layers_t, root into the staging buffer
//   2  ap_begin_kernel       observe log_n twice, the trace root, the publics; sample alpha; the K powers alpha^(K-1-k) into the AIR
//                            table's alpha region (the table is the copied Air's own: publics | alpha powers | Z_H, 1 / Z_H | chunk
//                            pointers; the tail is uploaded once by init — the shape is fixed — the publics per proof from pinned staging)
//   3  air_kernel<0>         (air.hip, air_quotient_launch) on that table -> the C chunk matrices
//   4  ntt_coset_lde per chunk (domain shift GENERATOR g_qn^c, as Pcs::commit takes it) -> lde_q[c]; commit -> layers_q, root
//   5  ts_zeta_kernel        (prover.hip, the fib prover's) observe the quotient root, sample zeta; zeta, zeta g_n and their den_consts
//                            into DevState
//   6  the open of Pcs::open for the shape [1, C] / [width, 4, ..] / trace at (zeta, zeta g_n), chunks at zeta, its points read from
//      DevState: pcs_inv_denoms_kernel<2, true>, pcs_bary_kernel + pcs_partial_sum_kernel per matrix, pcs_ts_open_kernel (dz),
//      pcs_y_kernel, pcs_reduced_*_kernel per matrix
//   7  ProverCore::fri_rounds, fri_final, grind_start, queries (the copy of the staging buffer into pinned memory)
// Host synchronisations: finish's one; one per continued proof-of-work range after a grind miss; check_trace's when it is asked for.
// zeta is a sampled extension element: it lies on the LDE coset (where Pcs::open refuses a point by name) only if three of its four
// words are zero, which no transcript produces; the device cannot refuse it and does not try.
#include "air_verifier_dev.h"  // air_proof_len: the gates of the proof's shape

namespace p3 {

bool take_error(std::string* out);  // context.hip

struct ApBeginArgs {
    TsArgs ts;
    uint32_t* tab;  // the AIR table: [0, n_public) the publics (read), [n_public, n_public + 4 K) the alpha powers (written)
    uint32_t log_n, n_public, K;
};
__global__ void __launch_bounds__(64) ap_begin_kernel(ApBeginArgs a) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    DevChal ch;
    ch.begin(a.ts.kind, a.ts.ds, &ks, true);
    ch.observe(bb::to_monty(a.log_n));  // log_ext_degree
    ch.observe(bb::to_monty(a.log_n));  // log_degree
    ch.observe_n(a.ts.ps + a.ts.lay.root_t, 8);
    ch.observe_n(a.tab, a.n_public);
    const Ext al = ch.sample_ext();
    // entry k = alpha^(K-1-k); lane l takes the exponents l, l + 64, ...
    Ext cur = bb::ext_one(), step = al;
    for (uint32_t i = 0; i < threadIdx.x; i++) cur = bb::mul(cur, al);
    for (int i = 0; i < 6; i++) step = bb::sqr(step);  // alpha^64
    uint32_t* ap = a.tab + a.n_public;
    for (uint32_t e = threadIdx.x; e < a.K; e += 64) { st_ext(ap + 4 * (size_t)(a.K - 1 - e), cur); cur = bb::mul(cur, step); }
    if (threadIdx.x == 0) { a.ts.ds->status = 0; a.ts.ps[a.ts.lay.status] = 0; }
    ch.end();
}

struct AirProver::Impl : ProverCore {
    Air air;  // the program's copy: its device block holds code, constants and the table
    uint32_t log_n = 0, C = 0, total = 0;
    AirTable tab{};
    // arena
    uint32_t *lde_t = nullptr, *layers_t = nullptr, *layers_q = nullptr, *trace_slot = nullptr;
    uint32_t *chunk[AIR_MAX_CHUNKS] = {nullptr}, *lde_q[AIR_MAX_CHUNKS] = {nullptr};
    uint32_t *d = nullptr, *xd = nullptr, *partials = nullptr, *sums = nullptr, *alp = nullptr, *ay = nullptr;
    PcsPair* pairs = nullptr;
    DevState* ds = nullptr;
    std::vector<uint32_t> nblk;      // per matrix (the trace, then the chunks): pcs_bary_kernel's workgroups along the rows
    std::vector<size_t> part_off;
    uint32_t* host_stage = nullptr;  // pinned: the staging buffer lands here
    size_t arena_bytes = 0, proof_len = 0;  // proof_len: p3hip_air_proof_len of the shape, what finish must have assembled
    bool in_flight = false;
    ~Impl() {
        if (host_stage) (void)hipHostFree(host_stage);
    }
    int take(uint32_t** p, size_t words) {
        arena_bytes += words * 4 + 64;
        return alloc(p, words);
    }
};

AirProver::AirProver() : im(new Impl()) {}
AirProver::~AirProver() { delete im; }
bool AirProver::pending() const { return im->in_flight; }
hipStream_t AirProver::stream() const { return im->stream; }
uint32_t AirProver::log_n() const { return im->log_n; }
uint32_t AirProver::width() const { return im->air.width; }
uint32_t AirProver::n_public() const { return im->air.n_public; }
int AirProver::device() const { return im->device; }

int AirProver::init(const Air& src, int profile, int hash, uint32_t log_n, const FriParams& fp, hipStream_t stream, bool own_stream) {
    Impl& s = *im;
    const char* who = "air_prover_create";
    int rc;
    if ((rc = s.begin(who, stream, own_stream, hash, profile))) return rc;
    // ---- the gates, each by name, before anything is allocated ----
    const uint32_t lqd = src.log_quotient_degree, C = 1u << lqd, w = src.width, total = 2 * w + 4 * C;
    if (log_n < 1 || log_n > bb::TWO_ADICITY - lqd)
        return fail(ERR_BAD_ARG, std::string(who) + ": log_n must lie in 1.." + std::to_string(bb::TWO_ADICITY - lqd) + " for this AIR (the quotient domain has 2^(log_n + " +
                                     std::to_string(lqd) + ") points)");
    if (fp.log_blowup < 1) return fail(ERR_BAD_ARG, std::string(who) + ": log_blowup must be >= 1");
    if (fp.log_blowup < lqd)
        return fail(ERR_BAD_ARG, std::string(who) + ": log_blowup " + std::to_string(fp.log_blowup) + " is below the AIR's log_quotient_degree " + std::to_string(lqd));
    if (log_n + fp.log_blowup > MAX_LOG_DOMAIN)
        return fail(ERR_BAD_ARG, std::string(who) + ": LDE domain above 2^" + std::to_string(MAX_LOG_DOMAIN) + " points (log_n + log_blowup)");
    if (total > PCS_MAX_COLS)
        return fail(ERR_BAD_ARG, std::string(who) + ": " + std::to_string(total) + " batched columns (2 width + 4 chunks), more than " + std::to_string(PCS_MAX_COLS));
    if ((rc = s.set_fri(who, fp, log_n))) return rc;
    size_t proof_len = 0;
    // the verifiers' gates of the same shape, and the length finish checks its bytes against.  A proof without queries, which prove_air
    // makes and no verifier takes, is made here too: the verifiers' layout refuses that one parameter by name
    if (fp.num_queries && (rc = air_proof_len(src, hash, log_n, fp, &proof_len))) return rc;
    // ---- the program ----
    Air& a = s.air;
    a.width = w; a.n_public = src.n_public; a.n_constraints = src.n_constraints; a.n_slots = src.n_slots;
    a.max_degree = src.max_degree; a.log_quotient_degree = lqd;
    a.code = src.code; a.consts = src.consts;
    s.log_n = log_n; s.C = C; s.total = total;
    s.tab = air_table(a, log_n);
    // ---- the arena ----
    const size_t n = (size_t)1 << log_n, big = (size_t)1 << s.log_big;
    const uint32_t n_mats = 1 + C, n_pairs = 2 + C;
    s.nblk.resize(n_mats); s.part_off.resize(n_mats);
    size_t part_words = 0;
    for (uint32_t m = 0; m < n_mats; m++) {
        const uint32_t mw = m ? 4 : w, np = m ? 1 : 2;
        s.nblk[m] = pcs_bary_blocks(mw, log_n);
        s.part_off[m] = part_words;
        part_words += (size_t)s.nblk[m] * np * mw * 4;
    }
    auto arena = [&]() -> int {
        int rc;
        if ((rc = air_ensure_device(a))) return rc;
        s.arena_bytes += (a.code.size() + a.consts.size() + a.tab_words + 8) * 4;
        if ((rc = s.take(&s.lde_t, big * w))) return rc;
        for (uint32_t c = 0; c < C; c++) {
            if ((rc = s.take(&s.chunk[c], n * 4))) return rc;
            if ((rc = s.take(&s.lde_q[c], big * 4))) return rc;
        }
        if ((rc = s.take(&s.layers_t, mmcs_layer_words(big)))) return rc;
        if ((rc = s.take(&s.layers_q, mmcs_layer_words(big)))) return rc;
        if ((rc = s.take(&s.d, 2 * big * 4))) return rc;
        if ((rc = s.take(&s.xd, 2 * n * 4))) return rc;
        if ((rc = s.take(&s.partials, part_words))) return rc;
        if ((rc = s.take(&s.sums, (size_t)total * 4))) return rc;
        if ((rc = s.take(&s.alp, (size_t)total * 4))) return rc;
        if ((rc = s.take(&s.ay, (size_t)n_pairs * 8))) return rc;
        uint32_t* p = nullptr;
        if ((rc = s.take(&p, (size_t)n_pairs * (sizeof(PcsPair) / 4)))) return rc;
        s.pairs = reinterpret_cast<PcsPair*>(p);
        if ((rc = s.take(&p, (sizeof(DevState) + 3) / 4))) return rc;
        s.ds = reinterpret_cast<DevState*>(p);
        const size_t before = s.allocs.size();
        if ((rc = s.alloc_fri())) return rc;
        s.arena_bytes += (s.fri_vec_words + s.fri_layer_words + ((size_t)4 << fp.log_final_poly_len)) * 4 + 64 * (s.allocs.size() - before);
        // the trees a query opens: the trace's, the quotient's C matrices in one, then the FRI rounds' (layout)
        QTree tt{}, tq{};
        tt.mat[0] = s.lde_t; tt.width[0] = tt.stride[0] = w; tt.n_mats = 1; tt.layers = s.layers_t; tt.log_height = s.log_big;
        for (uint32_t c = 0; c < C; c++) { tq.mat[c] = s.lde_q[c]; tq.width[c] = tq.stride[c] = 4; }
        tq.n_mats = C; tq.layers = s.layers_q; tq.log_height = s.log_big;
        static_assert(AIR_MAX_CHUNKS <= QTREE_MAX_MATS, "a quotient commitment fits one query tree");
        s.trees.push_back(tt); s.trees.push_back(tq);
        s.lay.root_t = 0; s.lay.root_q = 8; s.lay.opened = 16;
        s.lay.froots = 16 + 4 * total;
        if ((rc = s.layout(who, 0))) return rc;
        s.arena_bytes += ((size_t)s.lay.words + fp.num_queries + s.trees.size() * sizeof(QTree) / 4) * 4;
        P3_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.host_stage), (size_t)s.lay.words * 4 + 64));
        return OK;
    };
    if ((rc = arena())) {
        // the arena's size: its buffers that grow with the shape, reached or not (the query slots and the small tables come on top)
        size_t need = big * w + C * (n + big) * 4 + 2 * mmcs_layer_words(big) + 2 * (big + n) * 4 + part_words + 8 * (size_t)total;
        for (uint32_t r = 0; r <= s.n_rounds; r++) need += (big >> r) * 4 + (r < s.n_rounds ? mmcs_layer_words(big >> (r + 1)) : 0);
        std::string why;
        (void)take_error(&why);
        return fail(rc, std::string(who) + ": the arena of " + std::to_string(std::max(need * 4, s.arena_bytes)) + " bytes could not be allocated: " + why);
    }
    // ---- what the fixed shape fixes: the pairs in observation order, the table's tail, a clean transcript state ----
    const uint32_t gen = bb::to_monty(bb::GEN);
    const uint32_t sn = bb::pow(gen, 1ull << log_n), denom = bb::inv(bb::mul(bb::to_monty(1u << log_n), sn));
    std::vector<PcsPair> hp;
    hp.push_back(PcsPair{0, w, 0, 0, log_n, sn, denom, 0});
    hp.push_back(PcsPair{w, w, 1, w, log_n, sn, denom, 0});
    for (uint32_t c = 0; c < C; c++) hp.push_back(PcsPair{2 * w + 4 * c, 4, 0, 2 * w + 4 * c, log_n, sn, denom, 0});
    std::vector<uint32_t> tail(s.tab.words - s.tab.zh);
    air_table_tail(a, log_n, s.chunk, tail.data());
    P3_HIP(hipMemcpy(s.pairs, hp.data(), hp.size() * sizeof(PcsPair), hipMemcpyHostToDevice));
    P3_HIP(hipMemcpy(a.d_tab + s.tab.zh, tail.data(), tail.size() * 4, hipMemcpyHostToDevice));
    P3_HIP(hipMemset(s.ds, 0, sizeof(DevState)));
    s.proof_len = proof_len;
    return OK;
}

uint32_t* AirProver::arena_trace() {
    Impl& s = *im;
    if (!s.trace_slot && s.alloc(&s.trace_slot, ((size_t)1 << s.log_n) * s.air.width)) return nullptr;
    return s.trace_slot;
}

int AirProver::check_trace(const uint32_t* d_trace, const uint32_t* pis, long long* row, int* constraint) {
    Impl& s = *im;
    if (s.in_flight) return fail(ERR_BAD_ARG, "air prover: a proof is in flight (finish it first)");
    return air_check_trace(s.air, s.stream, d_trace, s.log_n, pis, row, constraint);
}

int AirProver::enqueue(const uint32_t* d_trace, const uint32_t* pis) {
    Impl& s = *im;
    Air& a = s.air;
    if (s.in_flight) return fail(ERR_BAD_ARG, "air prover: a proof is already in flight (finish it before the next enqueue)");
    if (!d_trace || (!pis && a.n_public)) return fail(ERR_BAD_ARG, "air prover: null trace or public values");
    if ((uintptr_t)d_trace & 3) return fail(ERR_BAD_ARG, "air prover: the trace must be 4-byte aligned");
    for (uint32_t k = 0; k < a.n_public; k++)
        if (pis[k] >= bb::P) return fail(ERR_BAD_ARG, "air prover: public value " + std::to_string(k) + " is not a canonical field element");
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device)
        return fail(ERR_BAD_ARG, "air prover: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cx.device));
    hipStream_t st = s.stream;
    const uint32_t log_n = s.log_n, log_big = s.log_big, n = 1u << log_n, big = 1u << log_big, w = a.width, C = s.C;
    const uint32_t gen = bb::to_monty(bb::GEN), lb = s.fp.log_blowup;
    const StageLayout& L = s.lay;
    const TsArgs ts{s.ds, s.pstage, s.hash, L};
    // the publics: pinned staging of the Air copy, rewritten only once the previous upload has run (the event discipline of air.hip)
    if (a.n_public) {
        P3_HIP(hipEventSynchronize((hipEvent_t)a.up_done));
        memcpy(a.h_pin, pis, a.n_public * 4);
        P3_HIP(hipMemcpyAsync(a.d_tab, a.h_pin, a.n_public * 4, hipMemcpyHostToDevice, st));
        P3_HIP(hipEventRecord((hipEvent_t)a.up_done, st));
    }
    // 1: the trace commitment
    const size_t wt = w, w4[AIR_MAX_CHUNKS] = {4, 4, 4, 4, 4, 4, 4, 4};
    static_assert(AIR_MAX_CHUNKS == 8, "w4 lists every chunk's width");
    if ((rc = ntt_coset_lde(cx, st, d_trace, s.lde_t, n, w, lb, gen, true))) return rc;
    if ((rc = s.commit(1, &s.lde_t, &wt, nullptr, big, s.layers_t, L.root_t))) return rc;
    // 2, 3: alpha and the quotient
    hipLaunchKernelGGL(ap_begin_kernel, dim3(1), dim3(64), 0, st, ApBeginArgs{ts, a.d_tab, log_n, a.n_public, a.n_constraints});
    P3_HIP(hipGetLastError());
    if ((rc = air_quotient_launch(a, st, a.d_tab, s.lde_t, log_n))) return rc;
    // 4: the quotient commitment; chunk c lives on GENERATOR g_qn^c <g_n>, its LDE's shift is GENERATOR / that (Pcs::commit)
    const uint32_t g_qn = bb::two_adic_generator(log_n + a.log_quotient_degree);
    uint32_t dom = gen;
    for (uint32_t c = 0; c < C; c++) {
        if ((rc = ntt_coset_lde(cx, st, s.chunk[c], s.lde_q[c], n, 4, lb, bb::mul(gen, bb::inv(dom)), true))) return rc;
        dom = bb::mul(dom, g_qn);
    }
    if ((rc = s.commit(C, s.lde_q, w4, nullptr, big, s.layers_q, L.root_q))) return rc;
    // 5: zeta, zeta g_n and their constants into DevState
    hipLaunchKernelGGL(ts_zeta_kernel, dim3(1), dim3(64), 0, st, ts, bb::two_adic_generator(log_n));
    P3_HIP(hipGetLastError());
    // 6: the open
    TwoLevelTable roots_big;
    if ((rc = cx.get_root_table(st, log_big, false, &roots_big))) return rc;
    {
        PcsDenArgs da{};
        da.d = s.d; da.xd = s.xd; da.big = big; da.log_big = log_big; da.h = n; da.gen = gen; da.dk = &s.ds->k0;
        static_assert(offsetof(DevState, k1) == offsetof(DevState, k0) + sizeof(DenConsts), "k0, k1 are read as an array of two");
        const uint32_t threads = (big + DEN_CHUNK - 1) / DEN_CHUNK;
        hipLaunchKernelGGL((pcs_inv_denoms_kernel<2, true>), dim3((threads + 255) / 256), dim3(256), 0, st, roots_big, da);
        P3_HIP(hipGetLastError());
    }
    for (uint32_t m = 0; m <= C; m++) {
        const uint32_t mw = m ? 4 : w, np = m ? 1 : 2, ooff = m ? 2 * w + 4 * (m - 1) : 0;
        PcsBaryArgs ba{};
        ba.lde = m ? s.lde_q[m - 1] : s.lde_t; ba.xd = s.xd; ba.partials = s.partials + s.part_off[m]; ba.w = mw; ba.h = n; ba.xstride = n;
        ba.pidx[0] = 0; ba.pidx[1] = 1;
        const dim3 grid(s.nblk[m], (mw + 63) / 64), blk(256);
        if (np == 2) hipLaunchKernelGGL(pcs_bary_kernel<2>, grid, blk, 0, st, ba);
        else hipLaunchKernelGGL(pcs_bary_kernel<1>, grid, blk, 0, st, ba);
        P3_HIP(hipGetLastError());
        const uint32_t words = np * mw * 4;
        hipLaunchKernelGGL(pcs_partial_sum_kernel, dim3((words + 7) / 8), dim3(256), 0, st, s.partials + s.part_off[m], s.nblk[m], words, s.sums + 4 * (size_t)ooff);
        P3_HIP(hipGetLastError());
    }
    {
        PcsOpenArgs oa{};
        oa.ts = ts; oa.sums = s.sums; oa.pairs = s.pairs; oa.alp = s.alp; oa.dz = &s.ds->zeta;
        static_assert(offsetof(DevState, zeta_next) == offsetof(DevState, zeta) + sizeof(Ext), "zeta, zeta_next are read as an array of two");
        oa.n_points = 2; oa.n_pairs = 2 + C; oa.total = s.total; oa.log_h = log_n;
        oa.sn = bb::pow(gen, 1ull << log_n); oa.denom = bb::inv(bb::mul(bb::to_monty(n), oa.sn));
        hipLaunchKernelGGL(pcs_ts_open_kernel, dim3(1), dim3(64), 0, st, oa);
        P3_HIP(hipGetLastError());
        hipLaunchKernelGGL(pcs_y_kernel, dim3(oa.n_pairs), dim3(256), 0, st, oa.pairs, oa.n_pairs, s.alp, s.pstage + L.opened, s.ay);
        P3_HIP(hipGetLastError());
    }
    for (uint32_t m = 0; m <= C; m++) {
        PcsReducedArgs ra{};
        ra.lde = m ? s.lde_q[m - 1] : s.lde_t; ra.alp = s.alp; ra.d = s.d; ra.ay = s.ay; ra.ro = s.fri_vec + s.fri_vec_off[0];
        ra.w = m ? 4 : w; ra.big = big; ra.dstride = big; ra.np = m ? 1 : 2; ra.first = m ? 0u : 1u;
        ra.pidx[0] = 0; ra.pidx[1] = 1;
        ra.pair[0] = m ? 1 + m : 0; ra.pair[1] = 1;
        if (ra.w <= 16) hipLaunchKernelGGL(pcs_reduced_narrow_kernel, dim3((big + 255) / 256), dim3(256), 0, st, ra);
        else hipLaunchKernelGGL(pcs_reduced_tile_kernel, dim3((big + PCS_TILE - 1) / PCS_TILE), dim3(64), 0, st, ra);
        P3_HIP(hipGetLastError());
    }
    // 7: FRI, proof of work, queries, the one copy-back
    if ((rc = s.fri_rounds(cx, ts, s.n_rounds))) return rc;
    if ((rc = s.fri_final(cx, ts))) return rc;
    if ((rc = s.grind_start(ts))) return rc;
    if ((rc = s.queries(ts, s.host_stage, L.words))) return rc;
    s.in_flight = true;
    return OK;
}

int AirProver::finish(std::vector<uint8_t>* proof) {
    Impl& s = *im;
    if (!s.in_flight) return fail(ERR_BAD_ARG, "air prover: no proof in flight (enqueue first)");
    s.in_flight = false;
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    if (cxp->device != s.device)
        return fail(ERR_BAD_ARG, "air prover: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cxp->device));
    const StageLayout& L = s.lay;
    const TsArgs ts{s.ds, s.pstage, s.hash, L};
    P3_HIP(hipStreamSynchronize(s.stream));  // the one synchronisation of a proof
    const uint32_t* hp = s.host_stage;
    if (hp[L.status] == ST_GRIND_MISS && (rc = s.continue_grind(ts, s.host_stage, L.words))) return rc;  // one synchronisation per range
    if (hp[L.status] != 0) return fail(ERR_INTERNAL, "air prover: witness rejected by the device transcript");
    const uint32_t w = s.air.width, C = s.C;
    proof->clear();
    proof->reserve(4 * (size_t)(22 + 8 * w + 17 * C) + 64 + (size_t)s.fp.num_queries * s.slot_words * 4 + 4096);
    put_u32(*proof, PROOF_MAGIC); put_u32(*proof, 1); put_u32(*proof, s.log_n);
    put_words(*proof, hp + L.root_t, 8); put_words(*proof, hp + L.root_q, 8);
    const uint32_t* o = hp + L.opened;
    put_u32(*proof, w); put_words(*proof, o, 4 * (size_t)w);
    put_u32(*proof, w); put_words(*proof, o + 4 * (size_t)w, 4 * (size_t)w);
    put_u32(*proof, C);
    for (uint32_t c = 0; c < C; c++) { put_u32(*proof, 4); put_words(*proof, o + 8 * (size_t)w + 16 * c, 16); }
    s.put_fri(*proof, hp);
    if (s.proof_len && proof->size() != s.proof_len)
        return fail(ERR_INTERNAL, "air prover: assembled " + std::to_string(proof->size()) + " bytes, the shape's proof has " + std::to_string(s.proof_len));
    return OK;
}

}  // namespace p3
