// TwoAdicFriPcs<BabyBear, GpuDft, MerkleTreeMmcs, ExtensionMmcs> over CALLER-SUPPLIED matrices: commit, open (prover.h Pcs).
// Included by prover.hip (same namespace: ProverCore, QTree, the transcript kernels, the grind and query kernels are shared; the
// fib kernels above are left as they are).  Every matrix of one open has the same height h, unless the object admits MIXED heights
// (init's mixed_heights; include/p3hip.h p3hip_pcs_create_mixed states the protocol): then a CLASS is the set of matrices that share
// log_big_m, each class has its own alpha counter and reduced-opening vector, and the fold that reaches a class's length adds beta^2 ro_c
// (fri_fold_rollin_kernel, prover.hip).  One run of pcs_inv_denoms_kernel over the tallest domain serves every class: in bit-reversed order
// the first big_c rows of GENERATOR * <g_big> are GENERATOR * <g_big_c>.  On a hiding object (pcs_hiding.hip.inc, included at
// the end: HidingFriPcs) commit randomizes and salts, and open runs here over the committed matrices with salts in every opening.
//
// Conventions are the test oracle's restatement of upstream (stark.c, cited by line):
//   commit   LDE = coset_lde_batch(evals, log_blowup, GENERATOR / s), bit-reversed by row (stark.c:33,64), one mmcs_commit per call
//   open     opened value of M at z = barycentric interpolation over the first h rows (stark.c:73-75, interpolate_low_coset);
//            observed round -> matrix -> point -> column (stark.c:76-78); alpha sampled (stark.c:79); each (matrix, point) pair
//            consumes `width` consecutive powers of alpha (stark.c:93-98, verifier stark.c:263-268):
//              ro[j] += alpha^off (Y - sum_c alpha^c v_c[j]) / (z - x_j),  Y = sum_c alpha^c M(z)_c,  x_j = GENERATOR g_big^bitrev(j)
//            then the FRI commit phase, final polynomial, grind and queries of ProverCore (stark.c:102-154)
//   bytes    the FriProof section of the wire format: from the count of commit-phase roots (stark.c:135) through the witness (:154)
//
// Kernels (all streaming or single-wave):
//   pcs_inv_denoms_kernel   1/(z_k - x_j) for K <= 4 points over the LDE domain (norm trick + chunked batched inversion of
//                           inv_denoms_kernel), and x_j/(z_k - x_j) over the low coset
//   pcs_bary_kernel         per matrix: sum_j x_j/(z_k - x_j) M[j][c] for all of the matrix's points at once; lanes run along the
//                           words of a row (64/w rows per wave step when w < 64), workgroup partials through LDS
//   pcs_partial_sum_kernel  adds the workgroup partials
//   pcs_ts_open_kernel      one wavefront: the (z^h - s^h)/(h s^h) factor, observe, sample alpha, the alpha-power table in HBM
//   pcs_y_kernel            per (matrix, point) pair: alpha^off and alpha^off Y
//   pcs_reduced_*_kernel    per matrix: S[j] = sum_c alpha^c v_c[j] ONCE, then every point's alpha^off (Y - S) / (z - x); one lane
//                           per row for w <= 16, 64 x 64 tiles turned through LDS above that
//   pcs_export_kernel       the challenger state behind the staging buffer, so that one copy brings both to the host

namespace p3 {

constexpr uint32_t PCS_STATE_WORDS = (uint32_t)(offsetof(DevState, pis) / 4);  // st, inb, outb, n_in, n_out, kc

struct PcsDenArgs {
    DenConsts k[PCS_MAX_POINTS];
    uint32_t* d;   // [K][big] extension elements
    uint32_t* xd;  // [K][h]
    uint32_t big, log_big, h, gen;
    const DenConsts* dk;  // DEV: the K points' constants in device memory, written earlier on the stream (AirProver); k is not read
};
template <int K, bool DEV = false>
__global__ void __launch_bounds__(256) pcs_inv_denoms_kernel(TwoLevelTable roots, PcsDenArgs a) {
    const uint32_t big = a.big;
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t j0 = t * DEN_CHUNK;
    if (j0 >= big) return;
    uint32_t a0[K * DEN_CHUNK], e0[K * DEN_CHUNK], e1[K * DEN_CHUNK], nrm[K * DEN_CHUNK], pre[K * DEN_CHUNK], xs[DEN_CHUNK];
#pragma unroll
    for (int k = 0; k < DEN_CHUNK; k++) {
        const uint32_t x = bb::mul(a.gen, tl(roots, brev((j0 + k) & (big - 1), a.log_big)));
        xs[k] = x;
#pragma unroll
        for (int z = 0; z < K; z++) {
            const DenConsts& c = DEV ? a.dk[z] : a.k[z];
            const uint32_t v = bb::sub(c.z0, x);
            const uint32_t dd0 = bb::add(bb::sqr(v), c.k0), dd1 = bb::sub(bb::mul(c.k1, v), c.c1);
            a0[K * k + z] = v; e0[K * k + z] = dd0; e1[K * k + z] = dd1;
            nrm[K * k + z] = bb::sub(bb::sqr(dd0), bb::mul(bb::W_MONTY, bb::sqr(dd1)));
        }
    }
    uint32_t acc = bb::ONE;
#pragma unroll
    for (int k = 0; k < K * DEN_CHUNK; k++) { pre[k] = acc; acc = bb::mul(acc, nrm[k]); }
    uint32_t inv = bb::inv(acc);
#pragma unroll
    for (int k = K * DEN_CHUNK - 1; k >= 0; k--) {
        const uint32_t r = bb::mul(inv, pre[k]);
        inv = bb::mul(inv, nrm[k]);
        nrm[k] = r;  // 1 / norm
    }
#pragma unroll
    for (int k = 0; k < DEN_CHUNK; k++) {
        const uint32_t j = j0 + k;
        if (j >= big) break;
#pragma unroll
        for (int z = 0; z < K; z++) {
            const DenConsts& c = DEV ? a.dk[z] : a.k[z];
            const uint32_t i = K * k + z;
            const uint32_t f0 = bb::mul(e0[i], nrm[i]), f1 = bb::neg(bb::mul(e1[i], nrm[i]));  // 1/D = f0 + f1 Y
            Ext r;
            r.c[0] = bb::add(bb::mul(a0[i], f0), bb::mul(c.z2w, f1));
            r.c[2] = bb::add(bb::mul(a0[i], f1), bb::mul(c.z2, f0));
            r.c[1] = bb::neg(bb::add(bb::mul(c.z1, f0), bb::mul(c.z3w, f1)));
            r.c[3] = bb::neg(bb::add(bb::mul(c.z1, f1), bb::mul(c.z3, f0)));
            st_ext(a.d + 4 * ((size_t)z * big + j), r);
            if (j < a.h) st_ext(a.xd + 4 * ((size_t)z * a.h + j), bb::scale(r, xs[k]));
        }
    }
}

// One matrix, all of its NP points: partial[blk][p][c] = sum over the block's rows of xd_p[j] M[j][c].  Lane layout: a wave step
// covers `rps` = 64 / tw rows of a tile of tw = min(w, 64) columns (lane = row offset * tw + column), so a wave's loads are the
// contiguous words rows r .. r + rps of the tile; a matrix wider than 64 takes one tile per blockIdx.y.
struct PcsBaryArgs {
    const uint32_t* lde;
    const uint32_t* xd;  // [K][xstride], the matrix reads the first h of each
    uint32_t* partials;  // [nblk][NP][w] extension elements
    uint32_t w, h, xstride, pidx[PCS_MAX_POINTS];
};
template <int NP>
__global__ void __launch_bounds__(256) pcs_bary_kernel(PcsBaryArgs a) {
    const uint32_t w = a.w, h = a.h;
    const uint32_t tw = w < 64u ? w : 64u, rps = w < 64u ? 64u / w : 1u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t roff = lane / tw, cin = lane - roff * tw, col = blockIdx.y * 64u + cin;
    const bool active = roff < rps && col < w;
    const uint32_t per_blk = (h + gridDim.x - 1) / gridDim.x;
    const uint32_t r_lo = blockIdx.x * per_blk, r_hi = min(h, r_lo + per_blk);
    Ext acc[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) acc[p] = bb::ext_zero();
    // two rows per step under one Montgomery reduction per coefficient (bb::dot2); a lane whose second row lies past the end pairs
    // its row with a zero value
    const uint32_t step = 4u * rps;
    if (active)
        for (uint32_t r = r_lo + wave * rps + roff; r < r_hi; r += 2 * step) {
            const bool two = r + step < r_hi;
            const uint32_t r2 = two ? r + step : r;
            const uint32_t va = a.lde[(size_t)r * w + col], vb = two ? a.lde[(size_t)r2 * w + col] : 0u;
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const uint32_t* xd = a.xd + 4 * (size_t)a.pidx[p] * a.xstride;
                const Ext ea = ld_ext(xd + 4 * (size_t)r), eb = ld_ext(xd + 4 * (size_t)r2);
#pragma unroll
                for (int c = 0; c < 4; c++) acc[p].c[c] = bb::add(acc[p].c[c], bb::dot2(ea.c[c], va, eb.c[c], vb));
            }
        }
    __shared__ uint32_t red[4][64][NP * 4];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int c = 0; c < 4; c++) red[wave][lane][4 * p + c] = active ? acc[p].c[c] : 0u;
    __syncthreads();
    const uint32_t tcols = min(tw, w - blockIdx.y * 64u);  // columns of this tile
    for (uint32_t i = threadIdx.x; i < tcols * NP * 4; i += blockDim.x) {
        const uint32_t k = i & 3u, c = (i >> 2) % tcols, p = (i >> 2) / tcols;
        uint32_t v = 0;
        for (uint32_t wv = 0; wv < 4; wv++)
            for (uint32_t ro = 0; ro < rps; ro++) v = bb::add(v, red[wv][ro * tw + c][4 * p + k]);
        a.partials[(((size_t)blockIdx.x * NP + p) * w + blockIdx.y * 64u + c) * 4 + k] = v;
    }
}
// sums[i] = sum over the matrix's workgroups of partials[blk][i], i over the words of its NP x w opened values: a workgroup takes
// eight words, 32 lanes per word run over the blocks (a lone lane per word would wait for up to 1024 loads one after another)
__global__ void __launch_bounds__(256) pcs_partial_sum_kernel(const uint32_t* partials, uint32_t nblk, uint32_t words, uint32_t* sums) {
    __shared__ uint32_t red[32][8];
    const uint32_t o = threadIdx.x & 7u, part = threadIdx.x >> 3, i = blockIdx.x * 8u + o;
    uint32_t v = 0;
    if (i < words)
        for (uint32_t b = part; b < nblk; b += 32) v = bb::add(v, partials[(size_t)b * words + i]);
    red[part][o] = v;
    __syncthreads();
    if (threadIdx.x < 8 && i < words) {
        uint32_t t = 0;
        for (uint32_t q = 0; q < 32; q++) t = bb::add(t, red[q][threadIdx.x]);
        sums[i] = t;
    }
}

// A (matrix, point) pair in observation order: its first column's index among all opened values, its width, its point, the exponent of
// its first alpha power (its class's counter: ooff when every matrix has one height), and its matrix's height: log_h, GENERATOR^h and
// 1 / (h GENERATOR^h)
struct PcsPair {
    uint32_t ooff, width, point, aoff, log_h, sn, denom, pad;
};
struct PcsOpenArgs {
    TsArgs ts;
    const uint32_t* sums;  // [total] extension elements: the barycentric sums
    const PcsPair* pairs;
    uint32_t* alp;         // [total] extension elements: alpha^i
    Ext z[PCS_MAX_POINTS];
    uint32_t n_points, n_pairs, total, log_h, sn, denom;  // total: the length of the alpha table; log_h, sn, denom: the tallest height's
    const Ext* dz;  // null, or the n_points points in device memory, written earlier on the stream (AirProver): z is not read
};
__device__ __forceinline__ Ext pcs_pick(const Ext* f, uint32_t k) { return k == 0 ? f[0] : k == 1 ? f[1] : k == 2 ? f[2] : f[3]; }
// finish the opened values (interpolate_coset's factor (z^h - s^h) / (h s^h), h the pair's own height), put them into the staging
// buffer, observe them in order, sample the batching challenge and fill its power table (lane l: alpha^l, alpha^(l + 64), ...)
__device__ __forceinline__ void pcs_bary_factors(const PcsOpenArgs& a, uint32_t log_h, uint32_t sn, uint32_t denom, Ext* f) {
#pragma unroll
    for (uint32_t k = 0; k < PCS_MAX_POINTS; k++) {
        Ext z = a.dz ? a.dz[k < a.n_points ? k : 0] : a.z[k < a.n_points ? k : 0];
        for (uint32_t i = 0; i < log_h; i++) z = bb::sqr(z);
        f[k] = bb::scale(bb::sub(z, bb::ext_from_base(sn)), denom);
    }
}
__global__ void __launch_bounds__(64) pcs_ts_open_kernel(PcsOpenArgs a) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    DevChal ch;
    ch.begin(a.ts.kind, a.ts.ds, &ks, false);
    Ext f[PCS_MAX_POINTS];
    uint32_t f_log_h = a.log_h;  // the factors in f are this height's: recomputed when a pair of another height comes (mixed heights)
    pcs_bary_factors(a, a.log_h, a.sn, a.denom, f);
    for (uint32_t p = 0; p < a.n_pairs; p++) {
        const PcsPair pr = a.pairs[p];
        if (pr.log_h != f_log_h) { pcs_bary_factors(a, pr.log_h, pr.sn, pr.denom, f); f_log_h = pr.log_h; }
        const Ext fp = pcs_pick(f, pr.point);
        for (uint32_t c = 0; c < pr.width; c++) {
            const uint32_t i = pr.ooff + c;
            const Ext v = bb::mul(ld_ext(a.sums + 4 * (size_t)i), fp);
            if (threadIdx.x == 0) st_ext(a.ts.ps + a.ts.lay.opened + 4 * (size_t)i, v);
            ch.observe_ext(v);
        }
    }
    const Ext al = ch.sample_ext();
    Ext cur = bb::ext_one(), step = al;
    for (uint32_t i = 0; i < threadIdx.x; i++) cur = bb::mul(cur, al);
    for (int i = 0; i < 6; i++) step = bb::sqr(step);  // alpha^64
    for (uint32_t i = threadIdx.x; i < a.total; i += 64) { st_ext(a.alp + 4 * (size_t)i, cur); cur = bb::mul(cur, step); }
    if (threadIdx.x == 0) { a.ts.ds->status = 0; a.ts.ps[a.ts.lay.status] = 0; }
    ch.end();
}
// ay[pair] = (alpha^off, alpha^off Y), Y = sum_c alpha^c opened[off + c]: one workgroup per pair, lanes along the columns
__global__ void __launch_bounds__(256) pcs_y_kernel(const PcsPair* pairs, uint32_t n_pairs, const uint32_t* alp, const uint32_t* opened,
                                                    uint32_t* ay) {
    __shared__ uint32_t red[4][4];
    const PcsPair pr = pairs[blockIdx.x];
    Ext y = bb::ext_zero();
    for (uint32_t c = threadIdx.x; c < pr.width; c += blockDim.x)
        y = bb::add(y, bb::mul(ld_ext(alp + 4 * (size_t)c), ld_ext(opened + 4 * (size_t)(pr.ooff + c))));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t v = y.c[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = bb::add(v, (uint32_t)__shfl_down((int)v, off, 64));
        if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; k++) y.c[k] = bb::add(bb::add(red[0][k], red[1][k]), bb::add(red[2][k], red[3][k]));
        const Ext ao = ld_ext(alp + 4 * (size_t)pr.aoff);
        st_ext(ay + 8 * (size_t)blockIdx.x, ao);
        st_ext(ay + 8 * (size_t)blockIdx.x + 4, bb::mul(ao, y));
    }
}

// Reduced openings of ONE matrix over the whole LDE domain: S[j] once, then every point of the matrix.  ro is stored by the first
// matrix of an open and added to by the others.
struct PcsReducedArgs {
    const uint32_t* lde;
    const uint32_t* alp;
    const uint32_t* d;   // [K][dstride], the matrix reads the first big of each
    const uint32_t* ay;  // [n_pairs][2]
    uint32_t* ro;
    uint32_t w, big, dstride, np, first, pidx[PCS_MAX_POINTS], pair[PCS_MAX_POINTS];
};
__device__ __forceinline__ void pcs_reduced_tail(const PcsReducedArgs& a, uint32_t j, const Ext& s) {
    Ext r = a.first ? bb::ext_zero() : ld_ext(a.ro + 4 * (size_t)j);
    for (uint32_t p = 0; p < a.np; p++) {
        const Ext ao = ld_ext(a.ay + 8 * (size_t)a.pair[p]), aoy = ld_ext(a.ay + 8 * (size_t)a.pair[p] + 4);
        const Ext e = ld_ext(a.d + 4 * ((size_t)a.pidx[p] * a.dstride + j));
        r = bb::add(r, bb::mul(bb::sub(aoy, bb::mul(ao, s)), e));
    }
    st_ext(a.ro + 4 * (size_t)j, r);
}
// w <= 16: one lane per row, two columns per Montgomery reduction
__global__ void __launch_bounds__(256) pcs_reduced_narrow_kernel(PcsReducedArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.big) return;
    const uint32_t* __restrict__ row = a.lde + (size_t)j * a.w;
    const uint32_t* __restrict__ alp = a.alp;
    Ext s = bb::ext_zero();
    uint32_t c = 0;
    for (; c + 1 < a.w; c += 2) {
        const uint32_t v0 = row[c], v1 = row[c + 1];
#pragma unroll
        for (int k = 0; k < 4; k++) s.c[k] = bb::add(s.c[k], bb::dot2(alp[4 * c + k], v0, alp[4 * c + 4 + k], v1));
    }
    if (c < a.w) {
        const uint32_t v0 = row[c];
#pragma unroll
        for (int k = 0; k < 4; k++) s.c[k] = bb::add(s.c[k], bb::mul(alp[4 * c + k], v0));
    }
    pcs_reduced_tail(a, j, s);
}
// w > 16: one wave per 64 rows.  The wave loads a tile of 64 rows x 64 columns with lanes along the columns (every load of the wave
// is 256 contiguous bytes), turns it through LDS (row stride 65 words: no bank conflicts either way), and lane r then runs along ROW r
// of the tile: its S accumulates in registers, two columns per Montgomery reduction, the alpha powers are wave-uniform (scalar loads),
// and the per-point tail runs one lane per row.  No cross-lane reduction at all: a butterfly per row costs ~100 instructions a row and
// made the first form of this kernel VALU-bound at 0.4 of a copy's rate (DESIGN.md section 5.2).
constexpr uint32_t PCS_TILE = 64, PCS_TILE_STRIDE = PCS_TILE + 1;
__global__ void __launch_bounds__(64) pcs_reduced_tile_kernel(PcsReducedArgs a) {
    __shared__ uint32_t tile[PCS_TILE * PCS_TILE_STRIDE];
    const uint32_t lane = threadIdx.x, r0 = blockIdx.x * PCS_TILE, w = a.w;
    const uint32_t rows = min(PCS_TILE, a.big - r0);  // uniform
    const uint32_t* __restrict__ alp = a.alp;
    Ext s = bb::ext_zero();
    for (uint32_t c0 = 0; c0 < w; c0 += PCS_TILE) {
        const uint32_t cw = min(PCS_TILE, w - c0);
        const uint32_t* __restrict__ src = a.lde + (size_t)r0 * w + c0 + lane;
        if (lane < cw)  // sixteen loads in flight per lane, then their sixteen LDS stores
            for (uint32_t rb = 0; rb < rows; rb += 16) {
                uint32_t v[16];
#pragma unroll
                for (uint32_t i = 0; i < 16; i++) v[i] = rb + i < rows ? src[(size_t)(rb + i) * w] : 0u;
#pragma unroll
                for (uint32_t i = 0; i < 16; i++) tile[(rb + i) * PCS_TILE_STRIDE + lane] = v[i];
            }
        lds_wave_sync();
        const uint32_t* __restrict__ mine = tile + lane * PCS_TILE_STRIDE;
        uint32_t c = 0;
        if (cw == PCS_TILE) {  // a full chunk: a fixed trip count, so that the alpha powers' scalar loads run ahead of their use
#pragma unroll 8
            for (uint32_t cc = 0; cc < PCS_TILE; cc += 2) {
                const uint32_t v0 = mine[cc], v1 = mine[cc + 1];
                const uint32_t* __restrict__ ap = alp + 4 * (size_t)(c0 + cc);
#pragma unroll
                for (int k = 0; k < 4; k++) s.c[k] = bb::add(s.c[k], bb::dot2(ap[k], v0, ap[4 + k], v1));
            }
            c = PCS_TILE;
        }
        for (; c + 1 < cw; c += 2) {
            const uint32_t v0 = mine[c], v1 = mine[c + 1];
            const uint32_t* __restrict__ ap = alp + 4 * (size_t)(c0 + c);
#pragma unroll
            for (int k = 0; k < 4; k++) s.c[k] = bb::add(s.c[k], bb::dot2(ap[k], v0, ap[4 + k], v1));
        }
        if (c < cw) {
            const uint32_t v0 = mine[c];
            const uint32_t* __restrict__ ap = alp + 4 * (size_t)(c0 + c);
#pragma unroll
            for (int k = 0; k < 4; k++) s.c[k] = bb::add(s.c[k], bb::mul(ap[k], v0));
        }
        lds_wave_sync();
    }
    if (lane < rows) pcs_reduced_tail(a, r0 + lane, s);
}

__global__ void __launch_bounds__(64) pcs_export_kernel(const DevState* ds, uint32_t* out) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(ds);
    for (uint32_t i = threadIdx.x; i < PCS_STATE_WORDS; i += 64) out[i] = s[i];
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
PcsData::~PcsData() {
    for (uint32_t* p : lde) (void)hipFree(p);
    if (salt_base) (void)hipFree(salt_base);
    delete tree;
}

// host challenger <-> device transcript state.  The Keccak HashChallenger becomes the streaming sponge: the complete blocks of
// its input are absorbed here, the rest is the pending block; coming back, the sponge state is the challenger's `kst`.
static void chal_to_dev(const Challenger& c, DevState* d) {
    memset(d, 0, sizeof(DevState));
    if (c.kind == HASH_POSEIDON2) {
        memcpy(d->st, c.state, 64); memcpy(d->inb, c.in, 32); memcpy(d->outb, c.out, 32);
        d->n_in = (uint32_t)c.n_in; d->n_out = (uint32_t)c.n_out;
        return;
    }
    memcpy(d->kc.st, c.kst, sizeof c.kst);
    const size_t off = keccak256_absorb_full(d->kc.st, c.ibuf.data(), c.ibuf.size());
    d->kc.blen = (uint32_t)(c.ibuf.size() - off);
    memcpy(d->kc.blk, c.ibuf.data() + off, d->kc.blen);
    memcpy(d->kc.obuf, c.obuf, 32);
    d->kc.n_obuf = (uint32_t)c.n_obuf;
}
static void chal_from_dev(const uint32_t* words, Challenger* c) {
    DevState d;
    memcpy(&d, words, (size_t)PCS_STATE_WORDS * 4);
    if (c->kind == HASH_POSEIDON2) {
        memcpy(c->state, d.st, 64); memcpy(c->in, d.inb, 32); memcpy(c->out, d.outb, 32);
        c->n_in = (int)d.n_in; c->n_out = (int)d.n_out;
        return;
    }
    memcpy(c->kst, d.kc.st, sizeof c->kst);
    c->ibuf.assign(d.kc.blk, d.kc.blk + d.kc.blen);
    memcpy(c->obuf, d.kc.obuf, 32);
    c->n_obuf = (int)d.kc.n_obuf;
}

// the same two conversions for callers that hold transcripts in device memory (include/p3hip.h p3hip_challenger_export / _import)
static_assert(CHALLENGER_STATE_WORDS == PCS_STATE_WORDS, "P3HIP_CHALLENGER_STATE_WORDS is the transcript part of DevState");
void challenger_export(const Challenger& c, uint32_t* words) {
    DevState d;
    chal_to_dev(c, &d);
    memcpy(words, &d, (size_t)PCS_STATE_WORDS * 4);
}
int challenger_import(const uint32_t* words, Challenger* c) {
    DevState d;
    memcpy(&d, words, (size_t)PCS_STATE_WORDS * 4);
    if (c->kind == HASH_POSEIDON2) {
        if (d.n_in >= 8) return fail(ERR_BAD_ARG, "challenger_import: " + std::to_string(d.n_in) + " pending inputs, a duplex challenger holds at most 7");
        if (d.n_out > 8) return fail(ERR_BAD_ARG, "challenger_import: " + std::to_string(d.n_out) + " outputs left, a duplex challenger holds at most 8");
    } else {
        if (d.kc.blen >= 136) return fail(ERR_BAD_ARG, "challenger_import: a pending block of " + std::to_string(d.kc.blen) + " bytes, below the rate of 136 expected");
        if (d.kc.n_obuf > 32) return fail(ERR_BAD_ARG, "challenger_import: " + std::to_string(d.kc.n_obuf) + " output bytes left, a digest has 32");
    }
    chal_from_dev(words, c);
    return OK;
}

// a base-field point with (z / GENERATOR)^big = 1 lies on the LDE coset: 1/(z - x) has no value there (upstream panics)
bool pcs_point_on_lde_coset(const uint32_t z[4], uint32_t log_big) {
    if (z[1] || z[2] || z[3]) return false;
    const uint32_t q = bb::mul(z[0], bb::inv(bb::to_monty(bb::GEN)));
    return bb::pow(q, 1ull << log_big) == bb::ONE;
}

// workgroups of pcs_bary_kernel along a matrix's rows: up to 4096 per matrix (at most 1024 blocks of rows), at least 8 wave steps each
static uint32_t pcs_bary_blocks(uint32_t w, uint32_t log_h) {
    const uint32_t tiles = (w + 63) / 64, rps = w < 64 ? 64 / w : 1, mh = 1u << log_h;
    return std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(1024, 4096 / tiles), mh / std::min<uint32_t>(mh, 32 * rps)));
}

struct Pcs::Impl {
    int hash = HASH_POSEIDON2, profile = PROFILE_LATENCY, device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool mixed = false;  // matrices of mixed heights are admitted (init's mixed_heights)
    FriParams fp{};
    DevState* ds = nullptr;
    // open scratch: allocated at first use, grown when a larger shape arrives
    struct Buf {
        uint32_t* p = nullptr;
        size_t words = 0;
        int reserve(size_t need) {
            if (need <= words) return OK;
            if (p) { (void)hipFree(p); p = nullptr; words = 0; }
            P3_HIP(hipMalloc(reinterpret_cast<void**>(&p), need * 4 + 64));
            words = need;
            return OK;
        }
        ~Buf() { if (p) (void)hipFree(p); }
    } d, xd, partials, sums, alp, ay, pairs;
    // HidingFriPcs (pcs_hiding.hip.inc): the three streams ([0] input mmcs, [1] fri mmcs, [2] pcs), the scratch of a hiding commit
    // (grown like the open scratch) and the nine words a hiding commit reads back: its root and the streams' shortage flag
    bool hiding = false;
    uint32_t nrc = 0;
    DevRng* rngs = nullptr;
    Buf rng_ws, draws, rt, co, ext, lde_scratch;
    uint32_t *rootbuf = nullptr, *host_root = nullptr;
    // the next n field elements of stream r (rng_fill_field, piece by piece beyond what one fill's workspace should take: 2^26 elements;
    // P3HIP_PCS_FILL_PIECE_LOG (tests): log2 of the piece, to enter the multi-piece path on small shapes)
    int fill(Context& cx, DevRng* r, uint32_t* out, uint64_t n, uint32_t* err) {
        uint64_t PIECE = 1ull << 26;
        if (const char* e = getenv("P3HIP_PCS_FILL_PIECE_LOG")) PIECE = 1ull << std::min(std::max(atoi(e), 4), 26);
        size_t w = 0;
        int rc;
        if (!n) return OK;
        if ((rc = rng_workspace_words(std::min<uint64_t>(n, PIECE), &w))) return rc;
        if ((rc = rng_ws.reserve(w))) return rc;
        for (uint64_t o = 0; o < n; o += PIECE)
            if ((rc = rng_fill_field(cx, stream, r, out + o, std::min<uint64_t>(PIECE, n - o), rng_ws.p, err))) return rc;
        return OK;
    }
    // the FRI arena, the staging layout and the pinned landing buffer of ONE shape (log_h, widths, points per matrix): kept while
    // opens of that shape follow one another, rebuilt when another shape arrives
    std::vector<uint32_t> shape;
    std::unique_ptr<ProverCore> core;
    uint32_t* host_stage = nullptr;
    DevState host_ds;
    std::vector<PcsPair> host_pairs;
    std::vector<uint32_t*> class_ro;  // by log_h: the reduced-opening vector of a class below the tallest (in the arena), or null
    ~Impl() {
        core.reset();
        if (host_stage) (void)hipHostFree(host_stage);
        if (host_root) (void)hipHostFree(host_root);
        if (rootbuf) (void)hipFree(rootbuf);
        if (rngs) (void)hipFree(rngs);
        if (ds) (void)hipFree(ds);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

Pcs::Pcs() : im(new Impl()) {}
Pcs::~Pcs() { delete im; }
hipStream_t Pcs::stream() const { return im->stream; }

int Pcs::init(const FriParams& fp, hipStream_t stream, bool own_stream, int hash, int profile, bool mixed_heights) {
    Impl& s = *im;
    s.stream = stream; s.own_stream = own_stream;  // recorded first: an owned stream is destroyed with the object even when init fails
    if (profile != PROFILE_THROUGHPUT && profile != PROFILE_LATENCY) return fail(ERR_BAD_ARG, "pcs: unknown profile");
    if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return fail(ERR_BAD_ARG, "pcs: unknown hash configuration");
    if (fp.log_blowup < 1) return fail(ERR_BAD_ARG, "pcs: log_blowup must be >= 1");
    if (fp.log_blowup + 1 > MAX_LOG_DOMAIN) return fail(ERR_BAD_ARG, "pcs: log_blowup too large");
    if (fp.proof_of_work_bits > 30) return fail(ERR_BAD_ARG, "pcs: proof_of_work_bits too large");
    s.hash = hash; s.profile = profile; s.fp = fp; s.mixed = mixed_heights;
    P3_HIP(hipGetDevice(&s.device));
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&s.ds), sizeof(DevState)));
    return OK;
}

int Pcs::commit(const uint32_t* const* d_evals, const size_t* heights, const size_t* widths, const uint32_t* shifts, size_t n_mats,
                uint32_t root_out[8], PcsData** out) {
    Impl& s = *im;
    if (s.hiding) return commit_hiding(d_evals, heights, widths, shifts, n_mats, root_out, out);
    if (!d_evals || !heights || !widths || !root_out || !out) return fail(ERR_BAD_ARG, "pcs commit: null argument");
    if (n_mats == 0) return fail(ERR_BAD_ARG, "pcs commit: zero matrices");
    if (n_mats > PCS_MAX_MATS)
        return fail(ERR_BAD_ARG, "pcs commit: " + std::to_string(n_mats) + " matrices, a commitment holds at most " + std::to_string(PCS_MAX_MATS));
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    if (cxp->device != s.device) return fail(ERR_BAD_ARG, "pcs commit: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cxp->device));
    size_t h = heights[0];  // the tallest
    for (size_t m = 0; m < n_mats; m++) {
        const std::string who = "pcs commit: matrix " + std::to_string(m);
        if (!d_evals[m]) return fail(ERR_BAD_ARG, who + " is null");
        if (!is_pow2(heights[m]) || heights[m] < 2) return fail(ERR_BAD_ARG, who + ": height must be a power of two >= 2");
        if (heights[m] != h && !s.mixed)
            return fail(ERR_BAD_ARG, who + " has height " + std::to_string(heights[m]) + ", matrix 0 has " + std::to_string(h) + ": mixed heights are not supported");
        h = std::max(h, heights[m]);
        if (widths[m] < 1 || widths[m] > PCS_MAX_COLS) return fail(ERR_BAD_ARG, who + ": width must be in [1, " + std::to_string(PCS_MAX_COLS) + "]");
        if (shifts && (shifts[m] == 0 || shifts[m] >= bb::P)) return fail(ERR_BAD_ARG, who + ": domain shift must be a nonzero field element (Montgomery word)");
    }
    const uint32_t log_h = log2u(h);
    if (log_h + s.fp.log_blowup > MAX_LOG_DOMAIN)
        return fail(ERR_BAD_ARG, "pcs commit: LDE domain above 2^" + std::to_string(MAX_LOG_DOMAIN) + " points (log_h + log_blowup)");
    std::unique_ptr<PcsData> data(new PcsData());
    data->log_h = log_h; data->log_big = log_h + s.fp.log_blowup; data->hash = s.hash; data->device = s.device;
    const uint32_t gen = bb::to_monty(bb::GEN);
    std::vector<size_t> hh(n_mats);  // the LDEs' heights: one tree over them, the shorter ones injected (mmcs_commit)
    for (size_t m = 0; m < n_mats; m++) {
        const size_t h = heights[m], big = h << s.fp.log_blowup;
        hh[m] = big;
        if (s.mixed) data->log_hs.push_back(log2u(h));
        uint32_t* p = nullptr;
        P3_HIP(hipMalloc(reinterpret_cast<void**>(&p), big * widths[m] * 4 + 64));
        data->lde.push_back(p);
        data->widths.push_back(widths[m]);
        // stark.c:33,64: the LDE's shift is GENERATOR / (the domain's shift), rows bit-reversed
        const uint32_t shift = shifts ? bb::mul(gen, bb::inv(shifts[m])) : gen;
        if ((rc = ntt_coset_lde(*cxp, s.stream, d_evals[m], p, h, (uint32_t)widths[m], s.fp.log_blowup, shift, true))) return rc;
    }
    if ((rc = mmcs_commit(s.stream, data->lde.data(), hh.data(), widths, n_mats, &data->tree, nullptr, nullptr, s.hash, nullptr, s.profile))) return rc;
    if ((rc = mmcs_root(s.stream, *data->tree, root_out))) return rc;  // the one synchronisation of a commit
    *out = data.release();
    return OK;
}

int Pcs::open(const PcsData* const* rounds, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, Challenger* chal,
              std::vector<uint32_t>* opened, std::vector<uint8_t>* proof) {
    Impl& s = *im;
    if (!rounds || !points_per_mat || !points || !chal || !opened || !proof) return fail(ERR_BAD_ARG, "pcs open: null argument");
    if (chal->kind != s.hash) return fail(ERR_BAD_ARG, "pcs open: the challenger belongs to another hash configuration");
    if (n_rounds == 0) return fail(ERR_BAD_ARG, "pcs open: zero rounds");
    if (n_rounds > PCS_MAX_ROUNDS)
        return fail(ERR_BAD_ARG, "pcs open: " + std::to_string(n_rounds) + " rounds, an open takes at most " + std::to_string(PCS_MAX_ROUNDS));
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device) return fail(ERR_BAD_ARG, "pcs open: created on device " + std::to_string(s.device) + ", current device is " + std::to_string(cx.device));
    // ---- the shape, the distinct points, the pairs in observation order (round -> matrix -> point) ----
    // A class: the matrices whose LDEs share log_big_m (one, the tallest, unless the object admits mixed heights); it keeps its own
    // count of alpha powers (cnt) and its height's interpolation constants; with a point it has its own reduced-opening vector (the
    // tallest class's is the FRI input core.fri_vec, a shorter class's is Impl::class_ro, in the shape's arena)
    struct Mat { const uint32_t* lde; uint32_t w, np, ooff, log_h, pidx[PCS_MAX_POINTS], pair[PCS_MAX_POINTS]; };
    struct Class { uint32_t cnt = 0, sn = 0, denom = 0; bool started = false; };
    std::vector<Mat> mats;
    std::vector<uint32_t> shape;
    Class cls[MAX_LOG_DOMAIN + 1];  // by log_h
    Ext zs[PCS_MAX_POINTS];
    uint32_t n_points = 0, total = 0;
    s.host_pairs.clear();
    if (!rounds[0]) return fail(ERR_BAD_ARG, "pcs open: round 0 is null");
    uint32_t log_h = rounds[0]->log_h;  // the tallest
    if (s.mixed)
        for (size_t r = 0; r < n_rounds; r++) {
            if (!rounds[r]) return fail(ERR_BAD_ARG, "pcs open: round " + std::to_string(r) + " is null");
            log_h = std::max(log_h, rounds[r]->log_h);
        }
    const uint32_t log_big = log_h + s.fp.log_blowup, gen = bb::to_monty(bb::GEN);
    shape.push_back(log_h);
    size_t mi = 0, pi = 0;
    for (size_t r = 0; r < n_rounds; r++) {
        const PcsData* dt = rounds[r];
        if (!dt) return fail(ERR_BAD_ARG, "pcs open: round " + std::to_string(r) + " is null");
        if (dt->hiding != s.hiding)
            return fail(ERR_BAD_ARG, "pcs open: round " + std::to_string(r) + (s.hiding ? " holds plain prover data, this PCS is hiding" : " holds hiding prover data, this PCS is not hiding"));
        if (dt->hash != s.hash || dt->device != s.device || dt->log_big - dt->log_h != s.fp.log_blowup || dt->nrc != s.nrc)
            return fail(ERR_BAD_ARG, "pcs open: round " + std::to_string(r) + " was committed by another PCS configuration");
        shape.push_back((uint32_t)dt->lde.size());
        for (size_t m = 0; m < dt->lde.size(); m++, mi++) {
            const std::string who = "pcs open: round " + std::to_string(r) + " matrix " + std::to_string(m);
            const uint32_t mlh = dt->mat_log_h(m);
            if (mlh != log_h && !s.mixed)
                return fail(ERR_BAD_ARG, who + " has height 2^" + std::to_string(mlh) + ", round 0 has 2^" + std::to_string(log_h) + ": mixed heights are not supported");
            if (s.mixed && mlh < s.fp.log_final_poly_len)
                return fail(ERR_BAD_ARG, who + " has height 2^" + std::to_string(mlh) + ", below the final polynomial's 2^" + std::to_string(s.fp.log_final_poly_len));
            const size_t np = points_per_mat[mi];
            if (np > PCS_MAX_POINTS) return fail(ERR_BAD_ARG, who + ": more than " + std::to_string(PCS_MAX_POINTS) + " opening points");
            Mat mt{dt->lde[m], (uint32_t)dt->widths[m], (uint32_t)np, total, mlh, {0}, {0}};
            shape.push_back(mt.w); shape.push_back(mt.np); shape.push_back(mlh);
            Class& cl = cls[mlh];
            if (np && !cl.sn) {  // interpolate_coset's constants of this height
                cl.sn = bb::pow(gen, 1ull << mlh);
                cl.denom = bb::inv(bb::mul(bb::to_monty(1u << mlh), cl.sn));
            }
            for (size_t p = 0; p < np; p++, pi++) {
                const uint32_t* z = points + 4 * pi;
                const std::string pw = who + " point " + std::to_string(p);
                for (int c = 0; c < 4; c++) if (z[c] >= bb::P) return fail(ERR_BAD_ARG, pw + " is not a canonical field element");
                if (pcs_point_on_lde_coset(z, log_big)) return fail(ERR_BAD_ARG, pw + " lies on the LDE coset GENERATOR * <g_big>");
                uint32_t k = 0;
                while (k < n_points && memcmp(zs[k].c, z, 16)) k++;
                if (k == n_points) {
                    if (n_points == PCS_MAX_POINTS) return fail(ERR_BAD_ARG, pw + ": more than " + std::to_string(PCS_MAX_POINTS) + " distinct opening points in one open");
                    memcpy(zs[n_points++].c, z, 16);
                }
                mt.pidx[p] = k; mt.pair[p] = (uint32_t)s.host_pairs.size();
                s.host_pairs.push_back(PcsPair{total, mt.w, k, cl.cnt, mlh, cl.sn, cl.denom, 0});
                total += mt.w; cl.cnt += mt.w;
                if (total > PCS_MAX_COLS)
                    return fail(ERR_BAD_ARG, pw + ": more than " + std::to_string(PCS_MAX_COLS) + " batched columns (sum of width over every (matrix, point) pair)");
            }
            mats.push_back(mt);
        }
    }
    if (total == 0) return fail(ERR_BAD_ARG, "pcs open: no opening point");
    if (!cls[log_h].cnt)
        return fail(ERR_BAD_ARG, "pcs open: no matrix of the tallest height 2^" + std::to_string(log_h) + " has an opening point: the FRI input would be missing");
    const uint32_t h = 1u << log_h, big = 1u << log_big, n_pairs = (uint32_t)s.host_pairs.size();
    uint32_t alp_len = 0;  // the alpha table: as long as the largest class counter (total when there is one class)
    for (const Class& c : cls) alp_len = std::max(alp_len, c.cnt);
    hipStream_t st = s.stream;

    // ---- arena of this shape ----
    if (!s.core || s.shape != shape) {
        P3_HIP(hipStreamSynchronize(st));
        s.core.reset();
        if (s.host_stage) { (void)hipHostFree(s.host_stage); s.host_stage = nullptr; }
        s.shape.clear();
        std::unique_ptr<ProverCore> c(new ProverCore());
        if ((rc = c->begin("pcs open", st, false, s.hash, s.profile))) return rc;
        c->salt_words = s.hiding ? PCS_SALT : 0;  // stark_hiding.c:230-247: every commit-phase layer with a salt
        if ((rc = c->set_fri("pcs open", s.fp, log_h))) return rc;
        if ((rc = c->alloc_fri())) return rc;
        for (size_t r = 0; r < n_rounds; r++) {
            QTree t{};
            t.n_mats = (uint32_t)rounds[r]->lde.size();
            // a round's tree is as deep as its own tallest LDE: opened at index >> (log_big - that), a shorter matrix's row that shifted again
            const uint32_t round_log_big = rounds[r]->log_big;
            for (uint32_t m = 0; m < t.n_mats; m++) {
                t.mat[m] = rounds[r]->lde[m]; t.width[m] = t.stride[m] = (uint32_t)rounds[r]->widths[m];
                t.mshift[m] = rounds[r]->log_h - rounds[r]->mat_log_h(m);
            }
            if (s.hiding) {  // stark_hiding.c:70-73: the values of every matrix, then one salt per matrix
                for (uint32_t m = 0; m < t.n_mats; m++) { t.mat[t.n_mats + m] = rounds[r]->salts[m]; t.width[t.n_mats + m] = t.stride[t.n_mats + m] = PCS_SALT; }
                t.n_mats *= 2;
            }
            t.layers = rounds[r]->tree->layers; t.log_height = round_log_big; t.shift = log_big - round_log_big;
            c->trees.push_back(t);
        }
        // the reduced-opening vectors of the shorter classes: 2^log_big_c extension elements each, rolled in while folding
        s.class_ro.assign(MAX_LOG_DOMAIN + 1, nullptr);
        for (uint32_t lh = 0; lh < log_h; lh++)
            if (cls[lh].cnt && (rc = c->alloc(&s.class_ro[lh], (size_t)4 << (lh + s.fp.log_blowup)))) return rc;

        c->lay.root_t = c->lay.root_q = c->lay.opened = 0;  // the staging buffer starts with the opened values
        c->lay.froots = 4 * total;
        if ((rc = c->layout("pcs open", PCS_STATE_WORDS + 1))) return rc;  // + the random streams' shortage flag
        P3_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.host_stage), ((size_t)c->lay.words + PCS_STATE_WORDS + 1) * 4 + 64));
        s.core = std::move(c);
        s.shape = shape;
    }
    ProverCore& core = *s.core;
    const StageLayout& L = core.lay;
    // partial sums: up to 4096 workgroups per matrix (at most 1024 blocks of rows), at least 8 wave steps of rows each
    std::vector<uint32_t> nblk(mats.size());
    std::vector<size_t> part_off(mats.size());
    size_t part_words = 0;
    for (size_t m = 0; m < mats.size(); m++) {
        nblk[m] = pcs_bary_blocks(mats[m].w, mats[m].log_h);
        part_off[m] = part_words;
        part_words += (size_t)nblk[m] * mats[m].np * mats[m].w * 4;
    }
    if ((rc = s.d.reserve((size_t)n_points * big * 4))) return rc;
    if ((rc = s.xd.reserve((size_t)n_points * h * 4))) return rc;
    if ((rc = s.partials.reserve(part_words))) return rc;
    if ((rc = s.sums.reserve((size_t)total * 4))) return rc;
    if ((rc = s.alp.reserve((size_t)alp_len * 4))) return rc;
    if ((rc = s.ay.reserve((size_t)n_pairs * 8))) return rc;
    if ((rc = s.pairs.reserve((size_t)n_pairs * (sizeof(PcsPair) / 4)))) return rc;

    // ---- upload: the challenger's state, the pairs, the trees of this open's commitments ----
    chal_to_dev(*chal, &s.host_ds);
    P3_HIP(hipMemcpyAsync(s.ds, &s.host_ds, sizeof(DevState), hipMemcpyHostToDevice, st));
    P3_HIP(hipMemcpyAsync(s.pairs.p, s.host_pairs.data(), (size_t)n_pairs * sizeof(PcsPair), hipMemcpyHostToDevice, st));
    for (size_t r = 0; r < n_rounds; r++) {
        QTree& t = core.trees[r];
        const uint32_t nm = (uint32_t)rounds[r]->lde.size();
        for (uint32_t m = 0; m < nm; m++) t.mat[m] = rounds[r]->lde[m];
        if (s.hiding) for (uint32_t m = 0; m < nm; m++) t.mat[nm + m] = rounds[r]->salts[m];
        t.layers = rounds[r]->tree->layers;
    }
    P3_HIP(hipMemcpyAsync(core.qtrees, core.trees.data(), n_rounds * sizeof(QTree), hipMemcpyHostToDevice, st));
    const TsArgs ts{s.ds, core.pstage, s.hash, L};

    // ---- inverse denominators ----
    TwoLevelTable roots_big;
    if ((rc = cx.get_root_table(st, log_big, false, &roots_big))) return rc;
    {
        PcsDenArgs da{};
        for (uint32_t k = 0; k < n_points; k++) da.k[k] = den_consts(zs[k]);
        da.d = s.d.p; da.xd = s.xd.p; da.big = big; da.log_big = log_big; da.h = h; da.gen = gen;
        const uint32_t threads = (big + DEN_CHUNK - 1) / DEN_CHUNK;
        const dim3 grid((threads + 255) / 256), blk(256);
        switch (n_points) {
            case 1: hipLaunchKernelGGL(pcs_inv_denoms_kernel<1>, grid, blk, 0, st, roots_big, da); break;
            case 2: hipLaunchKernelGGL(pcs_inv_denoms_kernel<2>, grid, blk, 0, st, roots_big, da); break;
            case 3: hipLaunchKernelGGL(pcs_inv_denoms_kernel<3>, grid, blk, 0, st, roots_big, da); break;
            default: hipLaunchKernelGGL(pcs_inv_denoms_kernel<4>, grid, blk, 0, st, roots_big, da); break;
        }
        P3_HIP(hipGetLastError());
    }
    // ---- opened values: the first h rows of every matrix, read once for all of its points ----
    for (size_t m = 0; m < mats.size(); m++) {
        const Mat& mt = mats[m];
        if (!mt.np) continue;
        PcsBaryArgs ba{};
        ba.lde = mt.lde; ba.xd = s.xd.p; ba.partials = s.partials.p + part_off[m]; ba.w = mt.w; ba.h = 1u << mt.log_h; ba.xstride = h;
        for (uint32_t p = 0; p < mt.np; p++) ba.pidx[p] = mt.pidx[p];
        const dim3 grid(nblk[m], (mt.w + 63) / 64), blk(256);
        switch (mt.np) {
            case 1: hipLaunchKernelGGL(pcs_bary_kernel<1>, grid, blk, 0, st, ba); break;
            case 2: hipLaunchKernelGGL(pcs_bary_kernel<2>, grid, blk, 0, st, ba); break;
            case 3: hipLaunchKernelGGL(pcs_bary_kernel<3>, grid, blk, 0, st, ba); break;
            default: hipLaunchKernelGGL(pcs_bary_kernel<4>, grid, blk, 0, st, ba); break;
        }
        P3_HIP(hipGetLastError());
        const uint32_t words = mt.np * mt.w * 4;
        hipLaunchKernelGGL(pcs_partial_sum_kernel, dim3((words + 7) / 8), dim3(256), 0, st, s.partials.p + part_off[m], nblk[m], words,
                           s.sums.p + 4 * (size_t)mt.ooff);
        P3_HIP(hipGetLastError());
    }
    {
        PcsOpenArgs oa{};
        oa.ts = ts; oa.sums = s.sums.p; oa.pairs = reinterpret_cast<const PcsPair*>(s.pairs.p); oa.alp = s.alp.p;
        for (uint32_t k = 0; k < n_points; k++) oa.z[k] = zs[k];
        oa.n_points = n_points; oa.n_pairs = n_pairs; oa.total = alp_len; oa.log_h = log_h;
        oa.sn = cls[log_h].sn; oa.denom = cls[log_h].denom;
        hipLaunchKernelGGL(pcs_ts_open_kernel, dim3(1), dim3(64), 0, st, oa);
        P3_HIP(hipGetLastError());
        hipLaunchKernelGGL(pcs_y_kernel, dim3(n_pairs), dim3(256), 0, st, oa.pairs, n_pairs, s.alp.p, core.pstage + L.opened, s.ay.p);
        P3_HIP(hipGetLastError());
    }
    // ---- reduced openings -> FRI input: every LDE word read once ----
    // one vector per class: the tallest class's is the FRI input, a shorter class's waits in the arena for its fold.  The first
    // big_c rows of the tallest domain are the class's own domain (bit-reversed order), so it reads the first big_c entries of d's rows.
    std::vector<const uint32_t*> rollin(core.n_rounds, nullptr);
    {
        for (const Mat& mt : mats) {
            if (!mt.np) continue;
            Class& cl = cls[mt.log_h];
            const uint32_t mbig = 1u << (mt.log_h + s.fp.log_blowup);
            PcsReducedArgs ra{};
            ra.lde = mt.lde; ra.alp = s.alp.p; ra.d = s.d.p; ra.ay = s.ay.p;
            ra.ro = mt.log_h == log_h ? core.fri_vec + core.fri_vec_off[0] : s.class_ro[mt.log_h];
            ra.w = mt.w; ra.big = mbig; ra.dstride = big; ra.np = mt.np; ra.first = cl.started ? 0u : 1u;
            for (uint32_t p = 0; p < mt.np; p++) { ra.pidx[p] = mt.pidx[p]; ra.pair[p] = mt.pair[p]; }
            if (mt.w <= 16) hipLaunchKernelGGL(pcs_reduced_narrow_kernel, dim3((mbig + 255) / 256), dim3(256), 0, st, ra);
            else hipLaunchKernelGGL(pcs_reduced_tile_kernel, dim3((mbig + PCS_TILE - 1) / PCS_TILE), dim3(64), 0, st, ra);
            P3_HIP(hipGetLastError());
            cl.started = true;
        }
        // the fold of round r leaves 2^(log_big - 1 - r) elements: the class of that length goes in there
        for (uint32_t lh = 0; lh < log_h; lh++)
            if (cls[lh].cnt) rollin[log_h - 1 - lh] = s.class_ro[lh];
    }
    // ---- FRI commit phase, final polynomial, grind, queries: ProverCore, as a fib proof runs them ----
    // hiding: the salts of every layer first, (big >> (r + 1)) x 4 draws of the `fri` stream in round order (stark_hiding.c:241); the
    // shortage flag sits behind the exported state and travels with the open's one copy
    uint32_t* const err = core.pstage + L.words + PCS_STATE_WORDS;
    if (s.hiding) {
        P3_HIP(hipMemsetAsync(err, 0, 4, st));
        if ((rc = s.fill(cx, s.rngs + 1, core.fri_salts, core.fri_salt_words, err))) return rc;
    }
    if ((rc = core.fri_rounds(cx, ts, core.n_rounds, rollin.data()))) return rc;
    if ((rc = core.fri_final(cx, ts))) return rc;
    if ((rc = core.grind_start(ts))) return rc;
    const uint32_t nq = s.fp.num_queries;
    hipLaunchKernelGGL(ts_queries_kernel, dim3(1), dim3(64), 0, st, ts, nq, log_big, s.fp.proof_of_work_bits, core.qidx);
    P3_HIP(hipGetLastError());
    if (nq) {
        hipLaunchKernelGGL(query_gather_kernel, dim3(nq, (uint32_t)core.trees.size()), dim3(64), 0, st, core.qtrees, core.qidx,
                           (uint32_t)core.slot_words, core.pstage + L.slots);
        P3_HIP(hipGetLastError());
    }
    const size_t words = (size_t)L.words + PCS_STATE_WORDS + (s.hiding ? 1 : 0);
    hipLaunchKernelGGL(pcs_export_kernel, dim3(1), dim3(64), 0, st, s.ds, core.pstage + L.words);
    P3_HIP(hipGetLastError());
    P3_HIP(hipMemcpyAsync(s.host_stage, core.pstage, words * 4, hipMemcpyDeviceToHost, st));
    P3_HIP(hipStreamSynchronize(st));  // the one synchronisation of an open
    const uint32_t* hp = s.host_stage;
    if (hp[L.status] == ST_GRIND_MISS) {  // the first search range held no witness: continue, redo the queries, fetch the state again
        if ((rc = core.continue_grind(ts, s.host_stage, L.words))) return rc;
        hipLaunchKernelGGL(pcs_export_kernel, dim3(1), dim3(64), 0, st, s.ds, core.pstage + L.words);
        P3_HIP(hipGetLastError());
        P3_HIP(hipMemcpyAsync(s.host_stage + L.words, core.pstage + L.words, (size_t)PCS_STATE_WORDS * 4, hipMemcpyDeviceToHost, st));
        P3_HIP(hipStreamSynchronize(st));
    }
    if (hp[L.status] != 0) return fail(ERR_INTERNAL, "pcs open: witness rejected by the device transcript");
    if (s.hiding && hp[L.words + PCS_STATE_WORDS] != 0) return fail(ERR_INTERNAL, "pcs open: a random stream ran out of raw draws");
    opened->assign(hp + L.opened, hp + L.opened + 4 * (size_t)total);
    proof->clear();
    proof->reserve(64 + (size_t)nq * core.slot_words * 4 + 4096);
    core.put_fri(*proof, hp);
    chal_from_dev(hp + L.words, chal);
    return OK;
}

}  // namespace p3

#include "pcs_hiding.hip.inc"
#include "air_prover.hip.inc"
