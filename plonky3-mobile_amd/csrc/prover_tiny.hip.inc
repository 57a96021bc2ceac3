// ONE-LAUNCH prover for instances that fit a workgroup — the reference's own (native/src/fib_air.rs:56-72: n = 8, x = 21, Keccak hashes,
// hiding MMCS / PCS seeded with 1, create_test_fri_params(_, 2)) and everything up to an LDE domain of 2^8 points whose three random
// streams each fit one wave's small fill.  Included by prover_hiding.hip.inc (same namespace, same arena, same staging layout: the host
// serialises the staging buffer exactly as after the multi-launch sequence).
//
// Why: at this size a proof through the general path is a CHAIN of ~58 dependent launches of ~9 us each (profiles/
// r04_tiny_instance_timeline_under_profiler.txt: 0.52 ms), every kernel a handful of waves.  Here the whole of
// p3_uni_stark::prove — the three SmallRng streams, trace, randomization, the coset LDEs, the salted Merkle trees, quotient, blinded
// chunks, openings, FRI commit phase, proof-of-work, queries and the Fiat-Shamir transcript — is ONE kernel of one 512-thread
// workgroup: phases separated by workgroup barriers, intermediates in the prover's arena (L2-resident at these sizes) and LDS.
// Nothing here is tuned for bandwidth or issue rate — at 2^4..2^8 points the time is the chain of dependent permutations (trees,
// transcript), so the transforms are the O(n^2) definitions (exact field arithmetic: the same words as any FFT), and the hash layers
// run one state per lane.  Statement followed: oracle/stark_hiding.c (the restatement the multi-launch prover reproduces byte for
// byte), i.e. [UPSTREAM-RECALL] of p3-uni-stark / p3-fri 0.4.2 in structure; PARITY UNPINNED against upstream like the rest.

constexpr uint32_t TINY_THREADS = 512, TINY_MAX_ROUNDS = 10, TINY_MAX_LOG_BIG = 8;
// diagnostic builds (tools/r05_tiny_stamps.sh: -DTINY_STAMPS=1 into tools/_bin/): thread 0 prints the 100 MHz wall clock at phase boundaries
#ifndef TINY_STAMPS
#define TINY_STAMPS 0
#endif
#if TINY_STAMPS
#define TINY_STAMP(name) do { if (threadIdx.x == 0 && tiny_ns < 24) { tiny_names[tiny_ns] = name; tiny_ts[tiny_ns++] = wall_clock64(); } } while (0)
#else
#define TINY_STAMP(name) ((void)0)
#endif

struct TinyArgs {
    uint32_t hash, log_n, log_blowup, log_fpl, nq, pow_bits;
    uint32_t a_monty, b_monty;        // first trace row
    uint64_t seed[4];                 // SmallRng::seed_from_u64(seed) (SplitMix64 expansion, host side): every stream starts here
    const uint64_t* jump;             // GF(2) jump matrices of the generator (context table; J_0 = one chunk)
    uint32_t n_pcs, n_mmcs, n_fri, ch_pcs, ch_mmcs, ch_fri;  // draws and small-fill chunks per stream
    uint32_t chunk_log;               // 6: chunks of 64 raw draws (jump = T^64), every stream within 64 of them; 8: chunks of 256 (jump = T^256)
    uint32_t *pcs_draws, *mmcs_draws, *fri_salts;            // pcs: rnd_t | t012 | rm;  mmcs: salt_t | salt_q[0..4) | salt_r
    uint32_t *trace, *rt, *lde_t, *salt_t, *layers_t;
    const uint32_t* in_trace;         // a caller's trace (prove_trace), read in place; nullptr: generate (a, b)'s into `trace`
    TsPis pis;                        // the caller's public values (given != 0), else read from the trace
    uint32_t *qchunks, *co, *ext, *lde_qb, *salt_q[HCH], *layers_q, *t012;
    uint32_t *rm, *lde_r, *salt_r, *layers_r;
    uint32_t *d0, *d1, *fri_vec, *fri_layers, *fp_ev;
    uint32_t fri_vec_off[TINY_MAX_ROUNDS + 1], fri_salt_off[TINY_MAX_ROUNDS], fri_layer_off[TINY_MAX_ROUNDS];
    uint32_t n_rounds;
    DevStateH* hs;
    uint32_t* pstage;
    StageLayout lay;
    uint32_t root_r_off, slot_words;
    const QTree* qtrees;
    uint32_t n_trees;
    uint32_t* qidx;
    uint32_t* err;  // the streams' shortage flag: the word behind the staging buffer
};

namespace tiny {

// ---- hashes, one state per lane ----
// leaf row of NW words (m0 || s0 || m1 || s1 ...), fetched through `word(k)`; digest -> out[0..8)
template <int NW, class F>
__device__ __forceinline__ void leaf(int kind, F&& word, uint32_t* out) {
    if (kind == HASH_KECCAK) {  // PaddingFreeSponge<KeccakF, 25, 17, 4> over pairs of field words (keccak_leaf_salted_kernel)
        static_assert(NW % 2 == 0 && NW <= 34, "one rate block");
        uint64_t st[25];
#pragma unroll
        for (int i = 0; i < 25; i++) st[i] = 0;
#pragma unroll
        for (int k = 0; k < NW / 2; k++) st[k] = (uint64_t)word(2 * k) | ((uint64_t)word(2 * k + 1) << 32);
        kk::permute_digest(st);
#pragma unroll
        for (int k = 0; k < 4; k++) { out[2 * k] = (uint32_t)st[k]; out[2 * k + 1] = (uint32_t)(st[k] >> 32); }
        return;
    }
    uint32_t s[16];  // PaddingFreeSponge<Perm16, 16, 8, 8>: overwrite-mode absorb, no padding (mmcs.hip sponge_row)
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = 0;
#pragma unroll
    for (int k = 0; k < NW; k += 8) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (k + i < NW) s[i] = word(k + i);
        p2::permute(s);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = s[k];
}
__device__ __forceinline__ void compress(int kind, const uint32_t* l, const uint32_t* r, uint32_t* out) {
    if (kind == HASH_KECCAK) {  // CompressionFunctionFromHasher<U64Hash, 2, 4>
        uint64_t st[25];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            st[k] = (uint64_t)l[2 * k] | ((uint64_t)l[2 * k + 1] << 32);
            st[4 + k] = (uint64_t)r[2 * k] | ((uint64_t)r[2 * k + 1] << 32);
        }
#pragma unroll
        for (int k = 8; k < 25; k++) st[k] = 0;
        kk::permute_digest(st);
#pragma unroll
        for (int k = 0; k < 4; k++) { out[2 * k] = (uint32_t)st[k]; out[2 * k + 1] = (uint32_t)(st[k] >> 32); }
        return;
    }
    uint32_t s[16];  // TruncatedPermutation<Perm16, 2, 8, 16>
#pragma unroll
    for (int k = 0; k < 8; k++) { s[k] = l[k]; s[8 + k] = r[k]; }
    p2::permute(s);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = s[k];
}
// the digest layers above `n_trees` leaf layers of `n` digests each, level by level, the trees side by side (same shape);
// layers[t]: leaf layer first, then n/2, ... the root.  Ends with a barrier.  A level with few nodes runs the lane-cooperative
// permutations (their latency is what a small level costs): Keccak-f with one state per WAVE (kk::f_coop, ~5 us against ~9 for a
// lane holding all 25 words) while the level fits the workgroup's waves, Poseidon2 with one state per 16-lane DPP row
// (p2c::permute, ~3 us against ~13) while it fits its rows; wider levels one state per lane.
__device__ __forceinline__ void levels(int kind, uint32_t* const* layers, uint32_t n_trees, uint32_t n) {
    constexpr uint32_t N_WAVES = TINY_THREADS / 64, N_ROWS = TINY_THREADS / 16;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, row16 = tid >> 4, lane16 = tid & 15u;
    uint32_t off = 0;
    for (uint32_t len = n >> 1; len >= 1; len >>= 1) {
        const uint32_t nodes = n_trees * len;
        if (kind == HASH_KECCAK && nodes <= N_WAVES) {
            if (wave < nodes) {  // uniform over the wave: every lane calls f_coop
                const uint32_t t = wave / len, i = wave - t * len, idx = kk::coop_index();
                const uint64_t* in = reinterpret_cast<const uint64_t*>(layers[t] + (size_t)off * 8) + 8 * (size_t)i;
                uint64_t a = idx < 8u ? in[idx] : 0ull;  // CompressionFunctionFromHasher: the eight lanes of the two children, one block
                a = kk::f_coop(a);
                if (idx < 4u) reinterpret_cast<uint64_t*>(layers[t] + (size_t)(off + 2 * len) * 8)[4 * (size_t)i + idx] = a;
            }
        } else if (kind == HASH_POSEIDON2 && nodes <= N_ROWS) {
            const uint32_t wave_first = wave * 4;  // rows of this wave: wave_first .. wave_first + 3
            if (wave_first < nodes) {  // uniform over the wave: rows past the level carry zeros
                const p2c::LaneConst lc = p2c::lane_constants(lane16);
                const bool act = row16 < nodes;
                const uint32_t t = act ? row16 / len : 0, i = act ? row16 - t * len : 0;
                uint32_t* L = layers[t] + (size_t)off * 8;
                const uint32_t v = act ? L[16 * (size_t)i + lane16] : 0u;  // left digest in lanes 0..7, right in 8..15
                const uint32_t r = p2c::permute(v, lc);
                if (act && lane16 < 8u) L[(size_t)(2 * len) * 8 + 8 * (size_t)i + lane16] = r;
            }
        } else {
            for (uint32_t j = tid; j < nodes; j += TINY_THREADS) {
                const uint32_t t = j / len, i = j - t * len;
                uint32_t* L = layers[t] + (size_t)off * 8;
                uint32_t d[8];
                compress(kind, L + 16 * i, L + 16 * i + 8, d);
                uint32_t* o = L + (size_t)(2 * len) * 8 + 8 * i;
#pragma unroll
                for (int k = 0; k < 8; k++) o[k] = d[k];
            }
        }
        __syncthreads();
        off += 2 * len;
    }
}
__device__ __forceinline__ const uint32_t* root_of(const uint32_t* layers, uint32_t n) { return layers + (size_t)(2 * n - 2) * 8; }

// ---- transforms by definition (n <= 2^8) ----
// tab[i] = first * step^i
__device__ __forceinline__ void pow_table(uint32_t* tab, uint32_t n, uint32_t first, uint32_t step) {
    for (uint32_t i = threadIdx.x; i < n; i += TINY_THREADS) tab[i] = bb::mul(first, bb::pow(step, i));
}
// dst[k][c] = (1/n) sum_j src[j][c] w^-(jk): the inverse DFT over the subgroup of order n (p3o_idft_batch); winv[m] = w^-m
__device__ __forceinline__ void idft(const uint32_t* src, uint32_t sstride, uint32_t* dst, uint32_t dstride, uint32_t n, uint32_t W,
                                     const uint32_t* winv, uint32_t ninv) {
    for (uint32_t idx = threadIdx.x; idx < n * W; idx += TINY_THREADS) {
        const uint32_t k = idx / W, c = idx - k * W;
        uint32_t acc = 0;
        for (uint32_t j = 0; j < n; j++) acc = bb::add(acc, bb::mul(src[(size_t)j * sstride + c], winv[(j * k) & (n - 1)]));
        dst[(size_t)k * dstride + c] = bb::mul(acc, ninv);
    }
}
// dst[row][c] = sum_k coef[k][c] x^k at x = xs[bitrev(row)] (coset_dft of the zero-padded coefficients, rows bit-reversed)
__device__ __forceinline__ void eval_rows(const uint32_t* coef, uint32_t cstride, uint32_t ncoef, uint32_t* dst, uint32_t dstride, uint32_t big,
                                          uint32_t log_big, uint32_t W, const uint32_t* xs) {
    for (uint32_t idx = threadIdx.x; idx < big * W; idx += TINY_THREADS) {
        const uint32_t row = idx / W, c = idx - row * W;
        const uint32_t x = xs[brev(row, log_big)];
        uint32_t acc = 0;
        for (uint32_t k = ncoef; k-- > 0;) acc = bb::add(bb::mul(acc, x), coef[(size_t)k * cstride + c]);
        dst[(size_t)row * dstride + c] = acc;
    }
}

}  // namespace tiny

__global__ void __launch_bounds__(TINY_THREADS) tiny_hiding_prover_kernel(TinyArgs a) {
    P3_LATENCY_BOUND_KERNEL();
    extern __shared__ __attribute__((aligned(16))) uint32_t tiny_lds[];  // 3 x (32 x 257) raw candidates, the domain tables behind them
    __shared__ KState ks, ks_save;
    __shared__ uint32_t osum[HOPEN][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#if TINY_STAMPS
    const uint64_t tiny_t0 = wall_clock64();
    uint64_t tiny_ts[24];
    const char* tiny_names[24];
    uint32_t tiny_ns = 0;
#endif
    const int kind = (int)a.hash;
    const uint32_t log_n = a.log_n, log_ext = log_n + 1, log_big = log_ext + a.log_blowup, log_q = log_n + 2;
    const uint32_t h = 1u << log_n, h2 = 2 * h, big = 1u << log_big, qn = 4 * h;
    const uint32_t gen = bb::to_monty(bb::GEN);
    const StageLayout L = a.lay;
    DevState* ds = &a.hs->base;
    uint32_t* ps = a.pstage;

    // ---- the three SmallRng streams, one wave each (every draw of a proof has a known place in its stream) ----
    if (tid == 0) *a.err = 0;
    __syncthreads();  // the flag is cleared before any wave can raise it
    if (wave < 3) {
        uint32_t* raw = tiny_lds + wave * (RNG_SMALL_CHUNKS * RNG_SMALL_STRIDE);
        uint32_t* out = wave == 0 ? a.mmcs_draws : wave == 1 ? a.fri_salts : a.pcs_draws;
        const uint32_t n = wave == 0 ? a.n_mmcs : wave == 1 ? a.n_fri : a.n_pcs;
        const uint32_t nch = wave == 0 ? a.ch_mmcs : wave == 1 ? a.ch_fri : a.ch_pcs;
        if (n) {
            uint64_t s_start[4];
            uint32_t my_base, cnt;
            const uint32_t total = a.chunk_log == RNG_TINY_CHUNK_LOG
                                       ? rng_small_fill_wave<RNG_TINY_CHUNK_LOG>(a.seed, a.jump, nch, raw, out, n, s_start, my_base, cnt)
                                       : rng_small_fill_wave<RNG_CHUNK_LOG>(a.seed, a.jump, nch, raw, out, n, s_start, my_base, cnt);
            if (total < n && lane == 0) atomicOr(a.err, 1u);
        }
    }
    // ---- meanwhile, on the idle waves: the trace (fib_air.rs:266-284) on one lane, the domain tables on the others.  Tables live in LDS
    // BEHIND the raw candidates: xs[i] = gen G^i (i < big), winv2[m] = w_2h^-m (m < 2h), winvh[m] = w_h^-m (m < h), spw[c][k] = s_c^-k ----
    uint32_t* xs = tiny_lds + 3 * (RNG_SMALL_CHUNKS * RNG_SMALL_STRIDE);
    uint32_t* winv2 = xs + big;
    uint32_t* winvh = winv2 + h2;
    uint32_t* spw = winvh + h;  // 4 x h
    if (tid == 3 * 64 && !a.in_trace) {
        uint32_t l = a.a_monty, r = a.b_monty;
        for (uint32_t i = 0; i < h; i++) {
            a.trace[2 * i] = l; a.trace[2 * i + 1] = r;
            const uint32_t t = bb::add(l, r); l = r; r = t;
        }
    } else if (tid > 3 * 64) {
        const uint32_t t0 = tid - (3 * 64 + 1), nt = TINY_THREADS - (3 * 64 + 1);
        const uint32_t G = bb::two_adic_generator(log_big), w2i = bb::inv(bb::two_adic_generator(log_ext)), whi = bb::inv(bb::two_adic_generator(log_n));
        const uint32_t g4 = bb::two_adic_generator(log_q);
        for (uint32_t i = t0; i < big; i += nt) xs[i] = bb::mul(gen, bb::pow(G, i));
        for (uint32_t i = t0; i < h2; i += nt) winv2[i] = bb::pow(w2i, i);
        for (uint32_t i = t0; i < h; i += nt) winvh[i] = bb::pow(whi, i);
        for (uint32_t idx = t0; idx < HCH * h; idx += nt) {
            const uint32_t c = idx / h, k = idx - c * h;
            spw[idx] = bb::pow(bb::inv(bb::mul(gen, bb::pow(g4, c))), k);
        }
    }
    __syncthreads();
    TINY_STAMP("rng+tables");
    // randomized trace: per trace row w + 2 NRC draws; the row keeps its values + the first NRC draws, the next row is the rest
    const uint32_t* tr = a.in_trace ? a.in_trace : a.trace;
    for (uint32_t i = tid; i < h; i += TINY_THREADS) {
        const uint32_t* d = a.pcs_draws + (size_t)i * (HW + 2 * HNRC);
        uint32_t* even = a.rt + (size_t)(2 * i) * HTW;
        even[0] = tr[2 * i]; even[1] = tr[2 * i + 1];
        for (uint32_t k = 0; k < HNRC; k++) even[HW + k] = d[k];
        for (uint32_t k = 0; k < HTW; k++) even[HTW + k] = d[HNRC + k];
    }
    __syncthreads();
    TINY_STAMP("randomize");
    const uint32_t inv_h2 = bb::inv(bb::to_monty(h2)), inv_h = bb::inv(bb::to_monty(h));
    // ---- coset LDEs of the randomized trace (2h x 6) and of the randomization matrix (2h x 8): coefficients, then values ----
    tiny::idft(a.rt, HTW, a.co, HTW, h2, HTW, winv2, inv_h2);            // co: 2h x 6
    tiny::idft(a.rm, HRW, a.ext, HRW, h2, HRW, winv2, inv_h2);           // ext: 2h x 8 (free until the chunks)
    __syncthreads();
    tiny::eval_rows(a.co, HTW, h2, a.lde_t, HTW, big, log_big, HTW, xs);
    tiny::eval_rows(a.ext, HRW, h2, a.lde_r, HRW, big, log_big, HRW, xs);
    __syncthreads();
    TINY_STAMP("lde t,r");
    // ---- the two hiding commitments that depend on nothing but draws: leaves m || salt, then the levels side by side ----
    for (uint32_t j = tid; j < 2 * big; j += TINY_THREADS) {
        const uint32_t t = j / big, i = j - t * big;
        uint32_t d[8];
        if (t == 0) {
            const uint32_t* m = a.lde_t + (size_t)i * HTW; const uint32_t* s = a.salt_t + (size_t)i * HSALT;
            tiny::leaf<HTW + HSALT>(kind, [&](int k) { return k < (int)HTW ? m[k] : s[k - HTW]; }, d);
        } else {
            const uint32_t* m = a.lde_r + (size_t)i * HRW; const uint32_t* s = a.salt_r + (size_t)i * HSALT;
            tiny::leaf<HRW + HSALT>(kind, [&](int k) { return k < (int)HRW ? m[k] : s[k - HRW]; }, d);
        }
        uint32_t* o = (t == 0 ? a.layers_t : a.layers_r) + (size_t)i * 8;
        for (int k = 0; k < 8; k++) o[k] = d[k];
    }
    __syncthreads();
    { uint32_t* two[2] = {a.layers_t, a.layers_r}; tiny::levels(kind, two, 2, big); }
    if (tid < 8) { ps[L.root_t + tid] = tiny::root_of(a.layers_t, big)[tid]; ps[a.root_r_off + tid] = tiny::root_of(a.layers_r, big)[tid]; }
    __syncthreads();

    TINY_STAMP("trees t,r");
    // ---- transcript: instance -> alpha (ts_begin_h_kernel) ----
    DevChal ch;
    uint32_t pis[3] = {tr[0], tr[1], tr[2 * (size_t)(h - 1) + 1]};
    if (a.pis.given) { pis[0] = a.pis.w[0]; pis[1] = a.pis.w[1]; pis[2] = a.pis.w[2]; }
    if (tid < 64) {
        ch.begin(kind, ds, &ks, true);
        ch.observe(bb::to_monty(log_n + 1));  // log_ext_degree = log_degree + is_zk
        ch.observe(bb::to_monty(log_n));      // log_degree
        ch.observe_n(ps + L.root_t, 8);
        ch.observe_n(pis, 3);
        const Ext alpha = ch.sample_ext();
        Ext ap = bb::ext_one();
        for (int k = 0; k < 5; k++) { if (tid == 0) ds->apow[k] = ap; ap = bb::mul(ap, alpha); }
        if (tid == 0) { ds->status = 0; ps[L.status] = 0; }
    }
    __syncthreads();
    TINY_STAMP("alpha");
    // ---- quotient on GENERATOR <g_4h> (the first 4h rows of the bit-reversed LDE), split into four chunks ----
    {
        const uint32_t gh_inv = bb::inv(bb::two_adic_generator(log_n));
        const Ext ap0 = ds->apow[0], ap1 = ds->apow[1], ap2 = ds->apow[2], ap3 = ds->apow[3], ap4 = ds->apow[4];
        for (uint32_t i = tid; i < qn; i += TINY_THREADS) {
            const uint32_t x = xs[i << (log_big - log_q)];
            const uint32_t* loc = a.lde_t + (size_t)brev(i, log_q) * HTW;
            const uint32_t* nxt = a.lde_t + (size_t)brev((i + 4) & (qn - 1), log_q) * HTW;
            const uint32_t zh = bb::sub(bb::pow(x, h), bb::ONE);
            const uint32_t first = bb::mul(zh, bb::inv(bb::sub(x, bb::ONE)));
            const uint32_t last = bb::mul(zh, bb::inv(bb::sub(x, gh_inv)));
            const uint32_t trans = bb::sub(x, gh_inv);
            const uint32_t c0 = bb::mul(first, bb::sub(loc[0], pis[0])), c1 = bb::mul(first, bb::sub(loc[1], pis[1]));
            const uint32_t c2 = bb::mul(trans, bb::sub(loc[1], nxt[0])), c3 = bb::mul(trans, bb::sub(bb::add(loc[0], loc[1]), nxt[1]));
            const uint32_t c4 = bb::mul(last, bb::sub(loc[1], pis[2]));
            Ext acc = bb::scale(ap4, c0);
            acc = bb::add(acc, bb::scale(ap3, c1)); acc = bb::add(acc, bb::scale(ap2, c2));
            acc = bb::add(acc, bb::scale(ap1, c3)); acc = bb::add(acc, bb::scale(ap0, c4));
            st_ext(a.qchunks + (size_t)(i >> 2) * HQS + (i & 3u) * HD, bb::scale(acc, bb::inv(zh)));
        }
    }
    __syncthreads();
    TINY_STAMP("quotient");
    // coefficients of q_c(s_c X) for the four chunks at once (h x 16), then the blinded chunk polynomials as 2h coefficients
    tiny::idft(a.qchunks, HQS, a.co, HQS, h, HQS, winvh, inv_h);
    __syncthreads();
    {
        const uint32_t gh = bb::pow(gen, h), w4 = bb::two_adic_generator(2);
        uint32_t shc[HCH], kc[HCH], p = bb::ONE;
        for (uint32_t c = 0; c < HCH; c++) { shc[c] = bb::mul(gh, p); p = bb::mul(p, w4); }
        for (uint32_t c = 0; c < HCH; c++) {
            uint32_t k = bb::ONE;
            for (uint32_t j = 0; j < HCH; j++) if (j != c) k = bb::mul(k, bb::sub(shc[c], shc[j]));
            kc[c] = k;
        }
        const uint32_t kinv0 = bb::inv(kc[0]), kinv1 = bb::inv(kc[1]), kinv2 = bb::inv(kc[2]);
        for (uint32_t idx = tid; idx < h * HD; idx += TINY_THREADS) {
            const uint32_t k = idx / HD, j = idx - k * HD;
            uint32_t t[HCH];
            for (uint32_t c = 0; c + 1 < HCH; c++) t[c] = a.t012[((size_t)c * h + k) * HD + j];
            t[HCH - 1] = bb::neg(bb::mul(kc[HCH - 1], bb::add(bb::add(bb::mul(t[0], kinv0), bb::mul(t[1], kinv1)), bb::mul(t[2], kinv2))));
            for (uint32_t c = 0; c < HCH; c++) {
                const uint32_t ak = bb::mul(a.co[(size_t)k * HQS + c * HD + j], spw[c * h + k]);
                a.ext[(size_t)k * HQS + c * HD + j] = bb::sub(ak, bb::mul(shc[c], t[c]));
                a.ext[(size_t)(h + k) * HQS + c * HD + j] = t[c];
            }
        }
    }
    __syncthreads();
    tiny::eval_rows(a.ext, HQS, h2, a.lde_qb, HQS, big, log_big, HQS, xs);
    __syncthreads();
    TINY_STAMP("chunks lde");
    for (uint32_t i = tid; i < big; i += TINY_THREADS) {  // leaf = q0 || s0 || q1 || s1 || q2 || s2 || q3 || s3
        uint32_t d[8];
        const uint32_t* m = a.lde_qb + (size_t)i * HQS;
        tiny::leaf<HCH * (HD + HSALT)>(kind, [&](int k) {
            const int c = k >> 3, o = k & 7;
            return o < (int)HD ? m[c * HD + o] : a.salt_q[c][(size_t)i * HSALT + (o - HD)];
        }, d);
        uint32_t* o = a.layers_q + (size_t)i * 8;
        for (int k = 0; k < 8; k++) o[k] = d[k];
    }
    __syncthreads();
    { uint32_t* one[1] = {a.layers_q}; tiny::levels(kind, one, 1, big); }
    if (tid < 8) ps[L.root_q + tid] = tiny::root_of(a.layers_q, big)[tid];
    __syncthreads();
    TINY_STAMP("tree q");
    // ---- zeta (ts_zeta_h_kernel) ----
    const uint32_t g_h = bb::two_adic_generator(log_n);
    if (tid < 64) {
        ch.observe_n(ps + L.root_q, 8);
        ch.observe_n(ps + a.root_r_off, 8);
        const Ext zeta = ch.sample_ext();
        if (tid == 0) { ds->zeta = zeta; ds->zeta_next = bb::scale(zeta, g_h); }
    }
    __syncthreads();
    const Ext zeta = ds->zeta, zeta_next = ds->zeta_next;
    TINY_STAMP("zeta");
    // ---- opened values: barycentric interpolation over the low coset (interpolate_low_coset) ----
    for (uint32_t i = tid; i < h2; i += TINY_THREADS) {
        const uint32_t x = xs[i << (log_big - log_ext)];
        st_ext(a.d0 + 4 * (size_t)i, bb::scale(bb::inv(bb::sub(zeta, bb::ext_from_base(x))), x));
        st_ext(a.d1 + 4 * (size_t)i, bb::scale(bb::inv(bb::sub(zeta_next, bb::ext_from_base(x))), x));
    }
    __syncthreads();
    for (uint32_t idx = tid; idx < HOPEN * 4; idx += TINY_THREADS) {  // order: random 8, trace @ zeta 6, trace @ zeta g 6, chunks 4 x 4
        const uint32_t k = idx >> 2, comp = idx & 3u;
        const uint32_t* mat; uint32_t stride, col; const uint32_t* den = a.d0;
        if (k < HRW) { mat = a.lde_r; stride = HRW; col = k; }
        else if (k < HRW + HTW) { mat = a.lde_t; stride = HTW; col = k - HRW; }
        else if (k < HRW + 2 * HTW) { mat = a.lde_t; stride = HTW; col = k - HRW - HTW; den = a.d1; }
        else { mat = a.lde_qb; stride = HQS; col = k - HRW - 2 * HTW; }
        uint32_t acc = 0;
        for (uint32_t i = 0; i < h2; i++) acc = bb::add(acc, bb::mul(den[4 * (size_t)i + comp], mat[(size_t)brev(i, log_ext) * stride + col]));
        osum[k][comp] = acc;
    }
    __syncthreads();
    if (tid < 64) {  // ts_open_h_kernel: opened values, observed; batch challenge powers; the constant sums of the reduced openings
        const uint32_t sn = bb::pow(gen, h2), denom = bb::inv(bb::mul(bb::to_monty(h2), sn));
        const Ext f0 = bb::scale(bb::sub(bb::pow(zeta, h2), bb::ext_from_base(sn)), denom);
        const Ext f1 = bb::scale(bb::sub(bb::pow(zeta_next, h2), bb::ext_from_base(sn)), denom);
        if (tid < HOPEN) {
            Ext v;
            for (int c = 0; c < 4; c++) v.c[c] = osum[tid][c];
            v = bb::mul(v, (tid >= HRW + HTW && tid < HRW + 2 * HTW) ? f1 : f0);
            for (int c = 0; c < 4; c++) { osum[tid][c] = v.c[c]; ps[L.opened + 4 * tid + c] = v.c[c]; }
        }
        lds_wave_sync();
        for (uint32_t k = 0; k < HOPEN; k++) {
            Ext v;
            for (int c = 0; c < 4; c++) v.c[c] = osum[k][c];
            ch.observe_ext(v);
        }
        const Ext al = ch.sample_ext();
        // lane k: al^k and its term al^k opened[k] (the serial chain of 36 x 2 extension products was ~11 us of one wave); the two
        // constant sums of the reduced openings by a wave reduction
        Ext y0 = bb::ext_zero(), y1 = bb::ext_zero();
        if (tid < HOPEN) {
            const Ext ap = bb::pow(al, tid);
            a.hs->alp[tid] = ap;
            Ext v;
            for (int c = 0; c < 4; c++) v.c[c] = osum[tid][c];
            const Ext term = bb::mul(ap, v);
            if (tid >= HRW + HTW && tid < HRW + 2 * HTW) y1 = term; else y0 = term;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                y0.c[c] = bb::add(y0.c[c], (uint32_t)__shfl_down((int)y0.c[c], off, 64));
                y1.c[c] = bb::add(y1.c[c], (uint32_t)__shfl_down((int)y1.c[c], off, 64));
            }
        }
        if (tid == 0) { a.hs->y0 = y0; a.hs->y1 = y1; }
    }
    __syncthreads();
    TINY_STAMP("open+alpha");
    // ---- reduced openings over the LDE domain, committed (bit-reversed) order ----
    {
        const DevStateH* hs = a.hs;
        uint32_t* ro = a.fri_vec + a.fri_vec_off[0];
        for (uint32_t i = tid; i < big; i += TINY_THREADS) {
            const uint32_t xi = xs[brev(i, log_big)];
            const Ext e0 = bb::inv(bb::sub(zeta, bb::ext_from_base(xi))), e1 = bb::inv(bb::sub(zeta_next, bb::ext_from_base(xi)));
            Ext s0 = hs->y0, s1 = hs->y1;
            uint32_t k = 0;
            for (uint32_t j = 0; j < HRW; j++, k++) s0 = bb::sub(s0, bb::scale(hs->alp[k], a.lde_r[(size_t)i * HRW + j]));
            for (uint32_t j = 0; j < HTW; j++, k++) s0 = bb::sub(s0, bb::scale(hs->alp[k], a.lde_t[(size_t)i * HTW + j]));
            for (uint32_t j = 0; j < HTW; j++, k++) s1 = bb::sub(s1, bb::scale(hs->alp[k], a.lde_t[(size_t)i * HTW + j]));
            for (uint32_t j = 0; j < HCH * HD; j++, k++) s0 = bb::sub(s0, bb::scale(hs->alp[k], a.lde_qb[(size_t)i * HQS + j]));
            st_ext(ro + 4 * (size_t)i, bb::add(bb::mul(s0, e0), bb::mul(s1, e1)));
        }
    }
    __syncthreads();
    TINY_STAMP("reduced");
    // ---- FRI commit phase: ExtensionMmcs over the hiding MMCS (salts from the `fri` stream), arity-2 folds ----
    const uint32_t one_half = bb::inv(bb::to_monty(2));
    for (uint32_t r = 0; r < a.n_rounds; r++) {
        const uint32_t half = big >> (r + 1), log_half = log_big - 1 - r;
        const uint32_t* vec = a.fri_vec + a.fri_vec_off[r];
        const uint32_t* salts = a.fri_salts + a.fri_salt_off[r];
        uint32_t* lay = a.fri_layers + a.fri_layer_off[r];
        for (uint32_t i = tid; i < half; i += TINY_THREADS) {
            uint32_t d[8];
            tiny::leaf<8 + HSALT>(kind, [&](int k) { return k < 8 ? vec[(size_t)i * 8 + k] : salts[(size_t)i * HSALT + (k - 8)]; }, d);
            for (int k = 0; k < 8; k++) lay[(size_t)i * 8 + k] = d[k];
        }
        __syncthreads();
        { uint32_t* one[1] = {lay}; tiny::levels(kind, one, 1, half); }
        if (tid < 8) ps[L.froots + 8 * r + tid] = tiny::root_of(lay, half)[tid];
        __syncthreads();
        if (tid < 64) {
            ch.observe_n(ps + L.froots + 8 * r, 8);
            const Ext beta = ch.sample_ext();
            if (tid == 0) ds->half_beta[r] = bb::scale(beta, one_half);
        }
        __syncthreads();
        {   // TwoAdicFriFolding::fold_matrix: out[i] = (1/2 + beta/(2x)) lo + (1/2 - beta/(2x)) hi, x = g^bitrev(i)
            const Ext hb = ds->half_beta[r];
            const uint32_t ginv = bb::inv(bb::two_adic_generator(log_half + 1));
            uint32_t* out = a.fri_vec + a.fri_vec_off[r + 1];
            for (uint32_t i = tid; i < half; i += TINY_THREADS) {
                const Ext lo = ld_ext(vec + 8 * (size_t)i), hi = ld_ext(vec + 8 * (size_t)i + 4);
                const uint32_t p = bb::pow(ginv, brev(i, log_half));
                st_ext(out + 4 * (size_t)i, bb::add(bb::scale(bb::add(lo, hi), one_half), bb::mul(bb::scale(hb, p), bb::sub(lo, hi))));
            }
        }
        __syncthreads();
    }
    TINY_STAMP("fri rounds");
    // ---- final polynomial: truncate, un-bit-reverse, inverse DFT of the four base coordinates; observed ----
    const uint32_t fpl = 1u << a.log_fpl;
    {
        const uint32_t* fin = a.fri_vec + a.fri_vec_off[a.n_rounds];
        for (uint32_t idx = tid; idx < fpl * 4; idx += TINY_THREADS) a.fp_ev[idx] = fin[4 * (size_t)brev(idx >> 2, a.log_fpl) + (idx & 3u)];
        uint32_t* wf = winv2;  // the table of w_2h is dead: w_fpl^-m, m < fpl (fpl <= 2h: log_final_poly_len < log_ext)
        __syncthreads();
        tiny::pow_table(wf, fpl, bb::ONE, bb::inv(bb::two_adic_generator(a.log_fpl)));
        __syncthreads();
        tiny::idft(a.fp_ev, 4, ps + L.fpoly, 4, fpl, 4, wf, bb::inv(bb::to_monty(fpl)));
    }
    __syncthreads();
    TINY_STAMP("final poly");
    // ---- proof of work (GrindingChallenger::grind, serial semantics: the smallest canonical witness), then the query indices ----
    if (tid < 64) {
        for (uint32_t i = 0; i < 4 * fpl; i++) ch.observe(ps[L.fpoly + i]);
        // candidates one after the other on a copy of the challenger: its state after the accepted witness IS the continued transcript
        uint64_t* live = reinterpret_cast<uint64_t*>(&ks);
        uint64_t* save = reinterpret_cast<uint64_t*>(&ks_save);
        if (kind == HASH_KECCAK) {
            lds_wave_sync();
            for (uint32_t i = tid; i < sizeof(KState) / 8; i += 64) save[i] = live[i];
            lds_wave_sync();
        }
        const DevChal ch0 = ch;
        uint32_t witness = 0, found = 0;
        const uint32_t limit = 64u << a.pow_bits;  // P[no witness below] = e^-64
        for (uint32_t cand = 0; cand < limit; cand++) {
            ch = ch0;
            if (kind == HASH_KECCAK) {
                lds_wave_sync();
                for (uint32_t i = tid; i < sizeof(KState) / 8; i += 64) live[i] = save[i];
                lds_wave_sync();
            }
            witness = bb::to_monty(cand);
            ch.observe(witness);
            if (ch.sample_bits(a.pow_bits) == 0) { found = 1; break; }
        }
        if (tid == 0) {
            ps[L.witness] = witness;
            ps[L.status] = found ? 0u : 2u;
            ds->status = 0;
        }
        for (uint32_t q = 0; q < a.nq; q++) {
            const uint32_t idx = ch.sample_bits(log_big);
            if (tid == 0) { a.qidx[q] = idx; ps[L.qidx + q] = idx; }
        }
    }
    __syncthreads();
    TINY_STAMP("grind+query");
    // ---- query openings: every (query, tree) pair by one wave (query_gather_kernel) ----
    for (uint32_t job = wave; job < a.nq * a.n_trees; job += TINY_THREADS / 64) {
        const uint32_t q = job / a.n_trees;
        const QTree& t = a.qtrees[job - q * a.n_trees];
        const uint32_t index = (a.qidx[q] >> t.shift) & ((1u << t.log_height) - 1u);
        uint32_t* dst = ps + L.slots + (size_t)q * a.slot_words + t.slot_off;
        uint32_t off = 0;
        for (uint32_t m = 0; m < t.n_mats; m++) {
            for (uint32_t c = lane; c < t.width[m]; c += 64) dst[off + c] = t.mat[m][(size_t)index * t.stride[m] + c];
            off += t.width[m];
        }
        uint32_t base = 0, len = 1u << t.log_height;
        for (uint32_t i = 0; i < t.log_height; i++) {
            const uint32_t sib = (index >> i) ^ 1u;
            if (lane < 8) dst[off + i * 8 + lane] = t.layers[(size_t)base + (size_t)sib * 8 + lane];
            base += len * 8;
            len >>= 1;
        }
    }
    TINY_STAMP("gather");
#if TINY_STAMPS
    if (threadIdx.x == 0) {
        uint64_t prev = tiny_t0;
        for (uint32_t i = 0; i < tiny_ns; i++) {  // integer microsecond tenths: one short record per line
            printf("tiny %s +%u at %u (0.1 us)\n", tiny_names[i], (uint32_t)((tiny_ts[i] - prev) / 10), (uint32_t)((tiny_ts[i] - tiny_t0) / 10));
            prev = tiny_ts[i];
        }
    }
#endif
}
