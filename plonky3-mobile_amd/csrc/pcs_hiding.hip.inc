// HidingFriPcs<BabyBear, GpuDft, MerkleTreeHidingMmcs, ExtensionMmcs over it, SmallRng> over CALLER-SUPPLIED matrices: the front half
// (commit, commit_quotient, the randomization commitment) of prover.h Pcs on a hiding object.  Included by pcs.hip.inc (same translation
// unit: Pcs::Impl, and Pcs::open there carries the salts).  The reference builds exactly this PCS (native/src/fib_air.rs:63-65).
//
// Conventions are the test oracle's (stark_hiding.c, cited by line), generalised from the fib shapes to any width, any number of
// random codewords NRC in 1..8 and C in {2, 4} quotient chunks; h = 2^log_h the caller's height, h2 = 2 h, big = h2 << log_blowup:
//   streams    three xoshiro256++ streams in HBM (stark_hiding.c:102-103): `mmcs` and `fri` seeded alike (the FRI MMCS is a clone of the
//              input MMCS), `pcs`; they advance from call to call; a call refused for its arguments draws nothing
//   commit     stark_hiding.c:105-124: per matrix, in input order, h (w + 2 NRC) draws of `pcs`, row by row; randomized row 2i =
//              evals[i] || d[0..NRC), row 2i+1 = d[NRC..w+2NRC): the h2 x (w + NRC) matrix over the size-h2 domain with the caller's
//              shift; LDE = coset_lde_batch(., log_blowup, GENERATOR / shift), rows bit-reversed; then per matrix, in input order, a
//              big x 4 salt matrix of `mmcs` draws; one tree, leaf rows m0 || s0 || m1 || s1 ... (stark_hiding.c:47-63)
//   quotient   stark_hiding.c:152-188: chunk c holds evaluations on s_c <g_h>, s_c = GENERATOR g_(C h)^c; sh_c = s_c^h, k_c = prod_{j != c}
//              (sh_c - sh_j); t_c (c < C - 1) = h x wq draws of `pcs` in chunk order, t_(C-1) = -k_(C-1) sum_{c < C-1} t_c / k_c; chunk c
//              becomes the h2 coefficient rows [a_k s_c^-k - sh_c t_c[k]] (k < h) then [t_c[k]] (k < h), a_k the coefficients of
//              q_c(s_c X); evaluated on GENERATOR <g_big>, rows bit-reversed; the C matrices in one salted tree
//   random     stark_hiding.c:190-194: an h2 x (NRC + 4) matrix of `pcs` draws, committed like a trace (shift 1)
//   open       stark_hiding.c:198-285 is Pcs::open (pcs.hip.inc) over the committed matrices: degree < h2, every committed column opened
//
// Kernels (both streaming: every word read once and written once):
//   pcs_randomize_kernel   rows 2i and 2i+1 of the randomized matrix lie one behind the other, and together they are evals[i] || draws[i]:
//                          a row-wise concatenation of the caller's h x w matrix and the h x (w + 2 NRC) draw buffer.  Lanes run along
//                          the OUTPUT words (narrow rows: several rows per wave step; wide rows: lanes along the columns), a workgroup
//                          takes 2048 consecutive output words; no row of any of the three matrices is assumed aligned
//   pcs_blind_kernel       the C coefficient matrices, the t draws and the two halves of every output matrix are all h x wq dense: one
//                          flat index runs over all of them, 16 bytes per lane when wq is a multiple of four

namespace p3 {

// q = n / d for n d < 2^32 (d >= 2): one multiply-high by floor(2^32 / d) + 1; d == 1 is flagged by a zero
static uint32_t pcs_div_magic(uint32_t d) { return d == 1 ? 0u : (uint32_t)((1ull << 32) / d) + 1u; }

constexpr uint32_t PCS_RND_PER = 8, PCS_RND_TILE = 256 * PCS_RND_PER;
struct PcsRandomizeArgs {
    const uint32_t* evals;  // h x w, the caller's, read in place
    const uint32_t* draws;  // h x dw
    uint32_t* out;          // 2h x (w + nrc) = h x len
    uint64_t total;         // h * len
    uint32_t w, dw, len, magic;  // dw = w + 2 nrc, len = 2 (w + nrc) <= 2^14: (len + PCS_RND_TILE) len < 2^32
};
__global__ void __launch_bounds__(256) pcs_randomize_kernel(PcsRandomizeArgs a) {
    const uint64_t start = (uint64_t)blockIdx.x * PCS_RND_TILE;
    const uint64_t row0 = start / a.len;  // uniform
    const uint32_t rem = (uint32_t)(start - row0 * a.len);
    uint32_t v[PCS_RND_PER];
#pragma unroll
    for (uint32_t k = 0; k < PCS_RND_PER; k++) {  // eight loads in flight per lane, then their eight stores
        const uint32_t o = k * 256u + threadIdx.x;
        v[k] = 0;
        if (start + o < a.total) {
            const uint32_t n = rem + o, q = __umulhi(n, a.magic), c = n - q * a.len;
            const uint64_t row = row0 + q;
            v[k] = c < a.w ? a.evals[row * a.w + c] : a.draws[row * a.dw + (c - a.w)];
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < PCS_RND_PER; k++) {
        const uint32_t o = k * 256u + threadIdx.x;
        if (start + o < a.total) a.out[start + o] = v[k];
    }
}

constexpr uint32_t PCS_BLIND_PER = 4;
template <int C>
struct PcsBlindArgs {
    const uint32_t* co[C];  // h x wq: coefficients of q_c(s_c X)
    const uint32_t* t;      // (C - 1) x (h x wq) draws
    uint32_t* ext[C];       // 2h x wq
    uint64_t n;             // h * wq
    uint32_t wq, magic;     // (wq + tile) wq < 2^32: wq <= 2048, tile <= 4096
    TwoLevelTable sp[C];    // s_c^-k
    uint32_t sh[C], kinv[C], k_last;
};
template <int V>
struct PcsVec;
template <>
struct PcsVec<1> {
    static __device__ __forceinline__ void ld(const uint32_t* p, uint32_t* v) { v[0] = *p; }
    static __device__ __forceinline__ void st(uint32_t* p, const uint32_t* v) { *p = v[0]; }
};
template <>
struct PcsVec<4> {
    static __device__ __forceinline__ void ld(const uint32_t* p, uint32_t* v) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ void st(uint32_t* p, const uint32_t* v) { *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]); }
};
// V words per lane (4: wq a multiple of four, so that a lane's words share their row k and every piece is 16-byte aligned)
template <int C, int V>
__global__ void __launch_bounds__(256) pcs_blind_kernel(PcsBlindArgs<C> a) {
    constexpr uint32_t TILE = 256u * PCS_BLIND_PER * V;
    const uint64_t start = (uint64_t)blockIdx.x * TILE;
    const uint64_t row0 = start / a.wq;  // uniform
    const uint32_t rem = (uint32_t)(start - row0 * a.wq);
    for (uint32_t it = 0; it < PCS_BLIND_PER; it++) {
        const uint32_t o = (it * 256u + threadIdx.x) * V;
        const uint64_t i = start + o;
        if (i >= a.n) break;  // n is a multiple of V
        const uint32_t nn = rem + o;
        const uint32_t k = (uint32_t)row0 + (a.magic ? __umulhi(nn, a.magic) : nn);
        uint32_t t[C][V], cw[C][V];
#pragma unroll
        for (int c = 0; c + 1 < C; c++) PcsVec<V>::ld(a.t + (size_t)c * a.n + i, t[c]);
#pragma unroll
        for (int c = 0; c < C; c++) PcsVec<V>::ld(a.co[c] + i, cw[c]);
#pragma unroll
        for (int j = 0; j < V; j++) {  // stark_hiding.c:158-164
            uint32_t s = 0;
#pragma unroll
            for (int c = 0; c + 1 < C; c++) s = bb::add(s, bb::mul(t[c][j], a.kinv[c]));
            t[C - 1][j] = bb::neg(bb::mul(a.k_last, s));
        }
#pragma unroll
        for (int c = 0; c < C; c++) {  // stark_hiding.c:173-179
            const uint32_t p = tl(a.sp[c], k);
            uint32_t lo[V];
#pragma unroll
            for (int j = 0; j < V; j++) lo[j] = bb::sub(bb::mul(cw[c][j], p), bb::mul(a.sh[c], t[c][j]));
            PcsVec<V>::st(a.ext[c] + i, lo);
            PcsVec<V>::st(a.ext[c] + a.n + i, t[c]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
bool Pcs::hiding() const { return im->hiding; }

int Pcs::init_hiding(const FriParams& fp, hipStream_t stream, bool own_stream, int hash, int profile, uint32_t nrc, uint64_t mmcs_seed,
                     uint64_t pcs_seed) {
    Impl& s = *im;
    int rc = init(fp, stream, own_stream, hash, profile);
    if (rc) return rc;
    if (nrc < 1 || nrc > PCS_MAX_RANDOM_CODEWORDS)
        return fail(ERR_BAD_ARG, "pcs: num_random_codewords must be in [1, " + std::to_string(PCS_MAX_RANDOM_CODEWORDS) + "]");
    if (fp.log_blowup + 2 > MAX_LOG_DOMAIN_HIDING) return fail(ERR_BAD_ARG, "pcs: log_blowup too large");
    s.hiding = true; s.nrc = nrc;
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&s.rngs), 3 * sizeof(DevRng)));
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&s.rootbuf), 9 * 4 + 64));
    P3_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.host_root), 9 * 4 + 64));
    // stark_hiding.c:102-103: the input MMCS's stream and its clone's start alike
    if ((rc = rng_seed(s.stream, s.rngs, mmcs_seed, 2))) return rc;
    return rng_seed(s.stream, s.rngs + 2, pcs_seed, 1);
}

// what the three commits share once data->lde holds the LDEs: the salts (per matrix, in input order, big x 4 draws of `mmcs`), the tree
// over (matrix, salt) pairs, and the commit's one synchronisation: the root and the streams' shortage flag in one copy
int Pcs::hiding_finish(PcsData* data, uint32_t root_out[8]) {
    Impl& s = *im;
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    const size_t n = data->lde.size(), big = (size_t)1 << data->log_big;
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&data->salt_base), n * big * PCS_SALT * 4 + 64));
    if ((rc = s.fill(*cxp, s.rngs, data->salt_base, (uint64_t)n * big * PCS_SALT, s.rootbuf + 8))) return rc;
    const uint32_t* mp[2 * PCS_HIDING_MAX_MATS];
    size_t hh[2 * PCS_HIDING_MAX_MATS], ww[2 * PCS_HIDING_MAX_MATS];
    for (size_t m = 0; m < n; m++) {
        data->salts.push_back(data->salt_base + m * big * PCS_SALT);
        mp[2 * m] = data->lde[m]; hh[2 * m] = big; ww[2 * m] = data->widths[m];
        mp[2 * m + 1] = data->salts[m]; hh[2 * m + 1] = big; ww[2 * m + 1] = PCS_SALT;
    }
    if ((rc = mmcs_commit(s.stream, mp, hh, ww, 2 * n, &data->tree, nullptr, nullptr, s.hash, nullptr, s.profile))) return rc;
    P3_HIP(hipMemcpyAsync(s.rootbuf, data->tree->layers + data->tree->layer_off.back(), 32, hipMemcpyDeviceToDevice, s.stream));
    P3_HIP(hipMemcpyAsync(s.host_root, s.rootbuf, 9 * 4, hipMemcpyDeviceToHost, s.stream));
    P3_HIP(hipStreamSynchronize(s.stream));  // the one synchronisation of a commit
    if (s.host_root[8] != 0) return fail(ERR_INTERNAL, "pcs commit: a random stream ran out of raw draws");
    memcpy(root_out, s.host_root, 32);
    return OK;
}

// the gates of a hiding commitment's height, shared by its three forms; *log_h = log2 h
static int pcs_hiding_height(const std::string& who, size_t h, const FriParams& fp, uint32_t* log_h) {
    if (!is_pow2(h) || h < 2) return fail(ERR_BAD_ARG, who + ": height must be a power of two >= 2");
    *log_h = log2u(h);
    if (*log_h + 1 + fp.log_blowup > MAX_LOG_DOMAIN_HIDING)
        return fail(ERR_BAD_ARG, who + ": LDE domain above 2^" + std::to_string(MAX_LOG_DOMAIN_HIDING) + " points (log_h + 1 + log_blowup)");
    return OK;
}

int Pcs::commit_hiding(const uint32_t* const* d_evals, const size_t* heights, const size_t* widths, const uint32_t* shifts, size_t n_mats,
                       uint32_t root_out[8], PcsData** out) {
    Impl& s = *im;
    if (!d_evals || !heights || !widths || !root_out || !out) return fail(ERR_BAD_ARG, "pcs commit: null argument");
    if (n_mats == 0) return fail(ERR_BAD_ARG, "pcs commit: zero matrices");
    if (n_mats > PCS_HIDING_MAX_MATS)
        return fail(ERR_BAD_ARG, "pcs commit: " + std::to_string(n_mats) + " matrices, a hiding commitment holds at most " + std::to_string(PCS_HIDING_MAX_MATS));
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device) return fail(ERR_BAD_ARG, "pcs commit: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cx.device));
    const size_t h = heights[0], wmax = PCS_MAX_COLS - s.nrc;
    uint32_t log_h = 0;
    for (size_t m = 0; m < n_mats; m++) {
        const std::string who = "pcs commit: matrix " + std::to_string(m);
        if (!d_evals[m]) return fail(ERR_BAD_ARG, who + " is null");
        if ((rc = pcs_hiding_height(who, heights[m], s.fp, &log_h))) return rc;
        if (heights[m] != h)
            return fail(ERR_BAD_ARG, who + " has height " + std::to_string(heights[m]) + ", matrix 0 has " + std::to_string(h) + ": mixed heights are not supported");
        if (widths[m] < 1 || widths[m] > wmax)
            return fail(ERR_BAD_ARG, who + ": width must be in [1, " + std::to_string(wmax) + "] (" + std::to_string(PCS_MAX_COLS) + " with the random columns)");
        if (shifts && (shifts[m] == 0 || shifts[m] >= bb::P)) return fail(ERR_BAD_ARG, who + ": domain shift must be a nonzero field element (Montgomery word)");
    }
    const size_t h2 = 2 * h, big = h2 << s.fp.log_blowup;
    std::unique_ptr<PcsData> data(new PcsData());
    data->log_h = log_h + 1; data->log_big = log_h + 1 + s.fp.log_blowup; data->hash = s.hash; data->device = s.device;
    data->hiding = true; data->nrc = s.nrc;
    const uint32_t gen = bb::to_monty(bb::GEN);
    hipStream_t st = s.stream;
    P3_HIP(hipMemsetAsync(s.rootbuf + 8, 0, 4, st));
    for (size_t m = 0; m < n_mats; m++) {
        const size_t w = widths[m], cw = w + s.nrc, dw = w + 2 * s.nrc;
        uint32_t* p = nullptr;
        P3_HIP(hipMalloc(reinterpret_cast<void**>(&p), big * cw * 4 + 64));
        data->lde.push_back(p);
        data->widths.push_back(cw);
        if ((rc = s.draws.reserve(h * dw))) return rc;
        if ((rc = s.rt.reserve(h2 * cw))) return rc;
        if ((rc = s.fill(cx, s.rngs + 2, s.draws.p, (uint64_t)h * dw, s.rootbuf + 8))) return rc;  // stark_hiding.c:111-112
        PcsRandomizeArgs ra{};
        ra.evals = d_evals[m]; ra.draws = s.draws.p; ra.out = s.rt.p;
        ra.w = (uint32_t)w; ra.dw = (uint32_t)dw; ra.len = (uint32_t)(2 * cw); ra.magic = pcs_div_magic(ra.len);
        ra.total = (uint64_t)h * ra.len;
        hipLaunchKernelGGL(pcs_randomize_kernel, dim3((uint32_t)((ra.total + PCS_RND_TILE - 1) / PCS_RND_TILE)), dim3(256), 0, st, ra);
        P3_HIP(hipGetLastError());
        // stark_hiding.c:121 with the caller's shift: the LDE's shift is GENERATOR / (the domain's shift), rows bit-reversed
        const uint32_t shift = shifts ? bb::mul(gen, bb::inv(shifts[m])) : gen;
        if ((rc = ntt_coset_lde(cx, st, s.rt.p, p, h2, (uint32_t)cw, s.fp.log_blowup, shift, true))) return rc;
    }
    if ((rc = hiding_finish(data.get(), root_out))) return rc;
    *out = data.release();
    return OK;
}

int Pcs::commit_quotient(const uint32_t* const* d_chunks, size_t h, size_t width, size_t n_chunks, uint32_t root_out[8], PcsData** out) {
    Impl& s = *im;
    if (!s.hiding) return fail(ERR_BAD_ARG, "pcs commit_quotient: this PCS is not hiding (commit the chunks with commit)");
    if (!d_chunks || !root_out || !out) return fail(ERR_BAD_ARG, "pcs commit_quotient: null argument");
    if (n_chunks < 2 || !is_pow2(n_chunks))
        return fail(ERR_BAD_ARG, "pcs commit_quotient: " + std::to_string(n_chunks) + " chunks: the blinding needs a power of two >= 2");
    if (n_chunks > PCS_HIDING_MAX_MATS)
        return fail(ERR_BAD_ARG, "pcs commit_quotient: " + std::to_string(n_chunks) + " chunks, a hiding commitment holds at most " + std::to_string(PCS_HIDING_MAX_MATS));
    if (width < 1 || width > PCS_MAX_QUOTIENT_WIDTH)
        return fail(ERR_BAD_ARG, "pcs commit_quotient: width must be in [1, " + std::to_string(PCS_MAX_QUOTIENT_WIDTH) + "]");
    uint32_t log_h = 0;
    int rc = pcs_hiding_height("pcs commit_quotient", h, s.fp, &log_h);
    if (rc) return rc;
    for (size_t c = 0; c < n_chunks; c++) if (!d_chunks[c]) return fail(ERR_BAD_ARG, "pcs commit_quotient: chunk " + std::to_string(c) + " is null");
    Context* cxp;
    if ((rc = get_context(&cxp))) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device) return fail(ERR_BAD_ARG, "pcs commit_quotient: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cx.device));
    const size_t C = n_chunks, h2 = 2 * h, big = h2 << s.fp.log_blowup, n = h * width;
    const uint32_t wq = (uint32_t)width, gen = bb::to_monty(bb::GEN);
    std::unique_ptr<PcsData> data(new PcsData());
    data->log_h = log_h + 1; data->log_big = log_h + 1 + s.fp.log_blowup; data->hash = s.hash; data->device = s.device;
    data->hiding = true; data->nrc = s.nrc;
    hipStream_t st = s.stream;
    for (size_t c = 0; c < C; c++) {
        uint32_t* p = nullptr;
        P3_HIP(hipMalloc(reinterpret_cast<void**>(&p), big * width * 4 + 64));
        data->lde.push_back(p);
        data->widths.push_back(width);
    }
    if ((rc = s.draws.reserve((C - 1) * n))) return rc;
    if ((rc = s.co.reserve(C * n))) return rc;
    if ((rc = s.ext.reserve(C * 2 * n))) return rc;
    if ((rc = s.lde_scratch.reserve(2 * n))) return rc;
    P3_HIP(hipMemsetAsync(s.rootbuf + 8, 0, 4, st));
    if ((rc = s.fill(cx, s.rngs + 2, s.draws.p, (uint64_t)(C - 1) * n, s.rootbuf + 8))) return rc;  // stark_hiding.c:156
    for (size_t c = 0; c < C; c++)  // stark_hiding.c:168: coefficients of q_c(s_c X)
        if ((rc = ntt_dft(cx, st, d_chunks[c], s.co.p + c * n, h, wq, true))) return rc;
    {
        // stark_hiding.c:81-92 for C chunks: sh_c = GENERATOR^h w_C^c, k_c = prod_{j != c} (sh_c - sh_j)
        const uint32_t log_c = log2u(C), gh = bb::pow(gen, h), wc = bb::two_adic_generator(log_c), gq = bb::two_adic_generator(log_h + log_c);
        uint32_t sh[PCS_HIDING_MAX_MATS], kc[PCS_HIDING_MAX_MATS], p = bb::ONE;
        for (size_t c = 0; c < C; c++) { sh[c] = bb::mul(gh, p); p = bb::mul(p, wc); }
        for (size_t c = 0; c < C; c++) {
            uint32_t k = bb::ONE;
            for (size_t j = 0; j < C; j++) if (j != c) k = bb::mul(k, bb::sub(sh[c], sh[j]));
            kc[c] = k;
        }
        if ((rc = cx.reserve_scale_slots(C))) return rc;  // the tables below stay valid until the kernel is enqueued
        auto launch = [&](auto args) -> int {
            constexpr int NC = (int)(sizeof(args.co) / sizeof(args.co[0]));
            for (int c = 0; c < NC; c++) {
                args.co[c] = s.co.p + (size_t)c * n; args.ext[c] = s.ext.p + (size_t)c * 2 * n;
                args.sh[c] = sh[c]; args.kinv[c] = bb::inv(kc[c]);
                int r = cx.get_scale_table(st, bb::inv(bb::mul(gen, bb::pow(gq, (uint64_t)c))), log_h, bb::ONE, &args.sp[c]);
                if (r) return r;
            }
            args.t = s.draws.p; args.n = n; args.wq = wq; args.magic = pcs_div_magic(wq); args.k_last = kc[NC - 1];
            const bool v4 = wq % 4 == 0;
            const uint64_t tile = 256ull * PCS_BLIND_PER * (v4 ? 4 : 1);
            const dim3 grid((uint32_t)((n + tile - 1) / tile)), blk(256);
            if (v4) hipLaunchKernelGGL((pcs_blind_kernel<NC, 4>), grid, blk, 0, st, args);
            else hipLaunchKernelGGL((pcs_blind_kernel<NC, 1>), grid, blk, 0, st, args);
            P3_HIP(hipGetLastError());
            return OK;
        };
        if ((rc = C == 2 ? launch(PcsBlindArgs<2>{}) : launch(PcsBlindArgs<4>{}))) return rc;
    }
    // stark_hiding.c:181-183: the blinded chunk polynomials on GENERATOR <g_big>, straight from their coefficients, rows bit-reversed
    for (size_t c = 0; c < C; c++)
        if ((rc = ntt_coset_lde_from_coeffs(cx, st, s.ext.p + c * 2 * n, data->lde[c], s.lde_scratch.p, h2, wq, s.fp.log_blowup, gen))) return rc;
    if ((rc = hiding_finish(data.get(), root_out))) return rc;
    *out = data.release();
    return OK;
}

int Pcs::commit_randomization(uint32_t log_h, uint32_t root_out[8], PcsData** out) {
    Impl& s = *im;
    if (!s.hiding) return fail(ERR_BAD_ARG, "pcs commit_randomization: this PCS is not hiding (it has no randomization polynomial)");
    if (!root_out || !out) return fail(ERR_BAD_ARG, "pcs commit_randomization: null argument");
    if (log_h < 1 || log_h > 31) return fail(ERR_BAD_ARG, "pcs commit_randomization: height must be a power of two >= 2");
    uint32_t lh = 0;
    int rc = pcs_hiding_height("pcs commit_randomization", (size_t)1 << log_h, s.fp, &lh);
    if (rc) return rc;
    Context* cxp;
    if ((rc = get_context(&cxp))) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device) return fail(ERR_BAD_ARG, "pcs commit_randomization: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cx.device));
    const size_t h2 = (size_t)2 << log_h, big = h2 << s.fp.log_blowup, w = s.nrc + 4;  // stark_hiding.c:36 HID_RW
    std::unique_ptr<PcsData> data(new PcsData());
    data->log_h = log_h + 1; data->log_big = log_h + 1 + s.fp.log_blowup; data->hash = s.hash; data->device = s.device;
    data->hiding = true; data->nrc = s.nrc;
    uint32_t* p = nullptr;
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&p), big * w * 4 + 64));
    data->lde.push_back(p);
    data->widths.push_back(w);
    if ((rc = s.rt.reserve(h2 * w))) return rc;
    P3_HIP(hipMemsetAsync(s.rootbuf + 8, 0, 4, s.stream));
    if ((rc = s.fill(cx, s.rngs + 2, s.rt.p, (uint64_t)h2 * w, s.rootbuf + 8))) return rc;  // stark_hiding.c:191
    if ((rc = ntt_coset_lde(cx, s.stream, s.rt.p, p, h2, (uint32_t)w, s.fp.log_blowup, bb::to_monty(bb::GEN), true))) return rc;
    if ((rc = hiding_finish(data.get(), root_out))) return rc;
    *out = data.release();
    return OK;
}

}  // namespace p3
