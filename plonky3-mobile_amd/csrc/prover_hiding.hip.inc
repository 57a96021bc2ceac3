// fib_air prover for the HIDING half of the reference's configuration (native/src/fib_air.rs:40-65):
//   MerkleTreeHidingMmcs<.., SmallRng, .., SALT_ELEMS 4> + HidingFriPcs::new(dft, mmcs, fri_params, 4, SmallRng::seed_from_u64(1)),
// for either hash configuration.  Included by prover.hip (same translation unit: it reuses that file's kernels).
// The protocol — randomized trace of height 2h with 4 random codeword columns, four blinded quotient chunks, the
// randomization-polynomial commitment, salted leaves everywhere, three SmallRng streams — is stated in the test
// restatement this prover must reproduce byte for byte (wire format version 2); it is [UPSTREAM-RECALL] in
// structure and PARITY UNPINNED against the absent p3-fri / p3-merkle-tree / p3-uni-stark 0.4.2.  Everything is
// device-resident: the random streams too (rng.hip), and the transcript, as in the non-hiding prover.

namespace p3 {

constexpr uint32_t HW = 2, HNRC = 4, HSALT = 4, HD = 4, HTW = HW + HNRC, HRW = HNRC + HD, HCH = 4;
constexpr uint32_t HOPEN = HRW + 2 * HTW + HCH * HD;  // 36 opened extension values / batch powers
constexpr uint32_t HQS = HCH * HD;  // the four chunk matrices are the column groups of ONE 16-word-wide matrix: row stride

struct DevStateH {
    DevState base;          // challenger + what the shared kernels read (k0/k1, half_beta, grind state ...)
    Ext alp[HOPEN];         // batch challenge powers
    Ext y0, y1;             // sum alpha^k y_k over the columns opened at zeta / at zeta g
    uint32_t err;           // rng shortage flag
};

// per trace row: w + 2 NRC draws; the row keeps its values + the first NRC draws, the next row is the other w + NRC
__global__ void randomize_trace_kernel(const uint2* trace, const uint32_t* rnd, uint32_t h, uint32_t* out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h) return;
    const uint2 t = trace[i];
    const uint32_t* d = rnd + (size_t)i * (HW + 2 * HNRC);
    uint32_t* even = out + (size_t)(2 * i) * HTW;
    even[0] = t.x; even[1] = t.y;
#pragma unroll
    for (uint32_t k = 0; k < HNRC; k++) even[HW + k] = d[k];
#pragma unroll
    for (uint32_t k = 0; k < HTW; k++) even[HTW + k] = d[HNRC + k];
}

// Selectors of the ORIGINAL trace domain <g_h> on the quotient coset GENERATOR <g_4h>, cached per prover (they depend on log_n
// only) in the order the quotient kernel walks the coset: entry 4 j + c belongs to x = GENERATOR w_4h^(4 t + c), t = bitrev(j).
//   fl = (Z(x) / (x - 1), Z(x) / (x - g_h^-1)) with Z(x) = x^h - 1 (one of four values, by c), tr = x - g_h^-1.
// One lane inverts its eight denominators with Montgomery's trick.  (Until round 4 the quotient kernel took two field inversions
// per point: 1290 of its 1330 VALU instructions.)
struct Zh4 { uint32_t v[4]; };
__global__ void __launch_bounds__(256) selectors_h_kernel(TwoLevelTable roots, uint32_t h, uint32_t log_h, uint32_t gen, uint32_t ginv, Zh4 zh,
                                                          uint2* fl, uint32_t* tr) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= h) return;
    const uint32_t t = brev(j, log_h);
    uint32_t v[8], pre[8], acc = bb::ONE;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t x = bb::mul(gen, tl(roots, 4u * t + c));
        v[2 * c] = bb::sub(x, bb::ONE);
        v[2 * c + 1] = bb::sub(x, ginv);
        tr[4 * (size_t)j + c] = v[2 * c + 1];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) { pre[k] = acc; acc = bb::mul(acc, v[k]); }
    uint32_t inv = bb::inv(acc);
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        const uint32_t r = bb::mul(inv, pre[k]);
        inv = bb::mul(inv, v[k]);
        v[k] = r;
    }
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) fl[4 * (size_t)j + c] = make_uint2(bb::mul(zh.v[c], v[2 * c]), bb::mul(zh.v[c], v[2 * c + 1]));
}

// quotient values on GENERATOR <g_4h> (first 4h rows of the bit-reversed LDE); constraints vanish on the ORIGINAL
// domain of size h.  Chunk c = i & 3 (split_evals), row t = i >> 2; the four chunks are the column groups of one h x 16 matrix.
// Lane j takes the four points i = 4 t + c of row t = bitrev(j): their LDE rows are (bitrev2(c) h + j), so a wave reads whole
// runs of consecutive 24-byte rows (and the rows of t + 1 likewise, wherever the carry stays above the wave's six bits) instead
// of eight scattered rows per lane; the one scattered access left is the 64-byte output row.
struct QuotHArgs {
    const uint32_t* lde;  // randomized trace LDE, big x HTW, bit-reversed rows
    uint32_t* chunks;     // h x HQS
    const DevState* ds;
    const uint2* sel_fl;
    const uint32_t* sel_tr;
    uint32_t h, log_h;
    uint32_t zh_inv[4];   // 1 / (x^h - 1) by i & 3
};
__global__ void __launch_bounds__(256) fib_quotient_h_kernel(QuotHArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.h) return;
    const DevState* __restrict__ ds = a.ds;
    const uint32_t t = brev(j, a.log_h), jn = brev((t + 1u) & (a.h - 1u), a.log_h);
    const uint4 fl01 = reinterpret_cast<const uint4*>(a.sel_fl)[2 * (size_t)j], fl23 = reinterpret_cast<const uint4*>(a.sel_fl)[2 * (size_t)j + 1];
    const uint4 tr4 = reinterpret_cast<const uint4*>(a.sel_tr)[j];
    const uint32_t first[4] = {fl01.x, fl01.z, fl23.x, fl23.z}, last[4] = {fl01.y, fl01.w, fl23.y, fl23.w}, trans[4] = {tr4.x, tr4.y, tr4.z, tr4.w};
    const uint32_t p0 = ds->pis[0], p1 = ds->pis[1], p2 = ds->pis[2];
    const Ext ap0 = ds->apow[0], ap1 = ds->apow[1], ap2 = ds->apow[2], ap3 = ds->apow[3], ap4 = ds->apow[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const size_t base = (size_t)(((c & 1u) << 1) | (c >> 1)) << a.log_h;  // bitrev2(c) * h
        const uint2 loc = *reinterpret_cast<const uint2*>(a.lde + (base + j) * HTW);
        const uint2 nxt = *reinterpret_cast<const uint2*>(a.lde + (base + jn) * HTW);
        const uint32_t c0 = bb::mul(first[c], bb::sub(loc.x, p0));
        const uint32_t c1 = bb::mul(first[c], bb::sub(loc.y, p1));
        const uint32_t c2 = bb::mul(trans[c], bb::sub(loc.y, nxt.x));
        const uint32_t c3 = bb::mul(trans[c], bb::sub(bb::add(loc.x, loc.y), nxt.y));
        const uint32_t c4 = bb::mul(last[c], bb::sub(loc.y, p2));
        Ext acc;
#pragma unroll
        for (int k = 0; k < 4; k++)  // sum of five products per coefficient: two dot2 and one product
            acc.c[k] = bb::add(bb::add(bb::dot2(ap4.c[k], c0, ap3.c[k], c1), bb::dot2(ap2.c[k], c2, ap1.c[k], c3)), bb::mul(ap0.c[k], c4));
        st_ext(a.chunks + (size_t)t * HQS + c * HD, bb::scale(acc, a.zh_inv[c]));
    }
}

// blinded chunk polynomials as coefficient vectors of length 2h: q_c + (X^h - s_c^h) t_c, with
//   co[c]  coefficients of q_c(s_c X) (inverse DFT of the chunk's values), so q_c's k-th coefficient is co[c][k] s_c^-k
//          (s_c^-k from a two-level table: two loads and a product instead of a 20-step square-and-multiply ladder)
//   t_c    random coefficients for c < 3, t_3 = -k_3 sum_{c<3} t_c / k_c
// co and ext hold the four chunks as the column groups of one 16-word-wide matrix (h resp. 2h rows).
struct BlindArgs {
    const uint32_t* co;   // h x HQS
    const uint32_t* t012; // (HCH - 1) x (h x HD) draws
    uint32_t* ext;        // 2h x HQS
    uint32_t h;
    TwoLevelTable sp[HCH];  // s_c^-k
    uint32_t sh[HCH], kinv[HCH], k_last;
};
__global__ void __launch_bounds__(256) blind_chunks_kernel(BlindArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.h) return;
    uint32_t t[HCH][HD];
#pragma unroll
    for (uint32_t c = 0; c + 1 < HCH; c++) {
        const uint4 d = *reinterpret_cast<const uint4*>(a.t012 + ((size_t)c * a.h + k) * HD);
        t[c][0] = d.x; t[c][1] = d.y; t[c][2] = d.z; t[c][3] = d.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < HD; j++)
        t[HCH - 1][j] = bb::neg(bb::mul(a.k_last, bb::add(bb::dot2(t[0][j], a.kinv[0], t[1][j], a.kinv[1]), bb::mul(t[2][j], a.kinv[2]))));
#pragma unroll
    for (uint32_t c = 0; c < HCH; c++) {
        const uint32_t p = tl(a.sp[c], k);
        const uint4 q = *reinterpret_cast<const uint4*>(a.co + (size_t)k * HQS + c * HD);
        const uint32_t cw[HD] = {q.x, q.y, q.z, q.w};
        uint32_t lo[HD];
#pragma unroll
        for (uint32_t j = 0; j < HD; j++) lo[j] = bb::sub(bb::mul(cw[j], p), bb::mul(a.sh[c], t[c][j]));
        *reinterpret_cast<uint4*>(a.ext + (size_t)k * HQS + c * HD) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *reinterpret_cast<uint4*>(a.ext + ((size_t)a.h + k) * HQS + c * HD) = make_uint4(t[c][0], t[c][1], t[c][2], t[c][3]);
    }
}

// The seven barycentric sums of the opening phase in ONE sweep over the low coset: the random matrix at zeta, the trace at zeta
// and at zeta*g, the four chunk matrices at zeta.  Each row's point and its two inverse denominators are read and multiplied once
// instead of seven times (den: 2 x 32 MB instead of 7 x 32 MB at 2^20).  partials: seven sets of 32 words per block (the form of seven
// one-matrix launches it replaced, +1.3 % on the hiding bench, was retired in round 5).
struct BaryAllArgs {
    TwoLevelTable roots;
    uint32_t n2, log_big, gen;
    const uint32_t *lde_r, *lde_t, *lde_q[HCH], *d0, *d1;
    uint32_t* partials;
    uint32_t set_stride;  // words between the partial sums of two sets
};
__global__ void __launch_bounds__(BARY_BLOCK) bary_all_kernel(BaryAllArgs a) {
    constexpr uint32_t NACC = HRW + 2 * HTW + HCH * HD;  // 8 + 6 + 6 + 16 extension accumulators
    Ext acc[NACC];
#pragma unroll
    for (uint32_t k = 0; k < NACC; k++) acc[k] = bb::ext_zero();
    // two rows per step: acc += e_j v_j + e_j' v_j' is ONE Montgomery reduction per coefficient (bb::dot2: 6 + 3 instructions for two
    // terms instead of 2 x (5 + 3)); a lane whose second row lies past the end pairs its row with a zero weight
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < a.n2; j += 2 * step) {
        const bool two = j + step < a.n2;
        const uint32_t j2 = two ? j + step : j;
        const uint32_t xa = bb::mul(a.gen, tl(a.roots, brev(j, a.log_big))), xb = two ? bb::mul(a.gen, tl(a.roots, brev(j2, a.log_big))) : 0u;
        const Ext e0a = bb::scale(ld_ext(a.d0 + 4 * (size_t)j), xa), e1a = bb::scale(ld_ext(a.d1 + 4 * (size_t)j), xa);
        const Ext e0b = bb::scale(ld_ext(a.d0 + 4 * (size_t)j2), xb), e1b = bb::scale(ld_ext(a.d1 + 4 * (size_t)j2), xb);
        auto fma2 = [](Ext& s, const Ext& ea, uint32_t va, const Ext& eb, uint32_t vb) {
#pragma unroll
            for (int c = 0; c < 4; c++) s.c[c] = bb::add(s.c[c], bb::dot2(ea.c[c], va, eb.c[c], vb));
        };
        const uint32_t *ra = a.lde_r + (size_t)j * HRW, *rb = a.lde_r + (size_t)j2 * HRW;
#pragma unroll
        for (uint32_t k = 0; k < HRW; k++) fma2(acc[k], e0a, ra[k], e0b, rb[k]);
        const uint32_t *ta = a.lde_t + (size_t)j * HTW, *tb = a.lde_t + (size_t)j2 * HTW;
#pragma unroll
        for (uint32_t k = 0; k < HTW; k++) {
            const uint32_t va = ta[k], vb = tb[k];
            fma2(acc[HRW + k], e0a, va, e0b, vb);
            fma2(acc[HRW + HTW + k], e1a, va, e1b, vb);
        }
#pragma unroll
        for (uint32_t c = 0; c < HCH; c++) {
            const uint32_t *qa = a.lde_q[c] + (size_t)j * HQS, *qb = a.lde_q[c] + (size_t)j2 * HQS;
#pragma unroll
            for (uint32_t k = 0; k < HD; k++) fma2(acc[HRW + 2 * HTW + c * HD + k], e0a, qa[k], e0b, qb[k]);
        }
    }
    __shared__ uint32_t red[BARY_BLOCK / 64][4 * NACC];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < NACC; k++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t v = acc[k].c[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = bb::add(v, (uint32_t)__shfl_down((int)v, off, 64));
            if (lane == 0) red[wave][4 * k + c] = v;
        }
    __syncthreads();
    if (threadIdx.x < 4 * NACC) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < BARY_BLOCK / 64; w++) v = bb::add(v, red[w][threadIdx.x]);
        // accumulator k of the sweep -> (set, element) of the seven-launch layout: 32 words per block and set
        const uint32_t k = threadIdx.x >> 2, c = threadIdx.x & 3u;
        uint32_t set, idx;
        if (k < HRW) { set = 0; idx = k; }
        else if (k < HRW + HTW) { set = 1; idx = k - HRW; }
        else if (k < HRW + 2 * HTW) { set = 2; idx = k - HRW - HTW; }
        else { set = 3 + (k - HRW - 2 * HTW) / HD; idx = (k - HRW - 2 * HTW) % HD; }
        a.partials[(size_t)set * a.set_stride + blockIdx.x * 32 + 4 * idx + c] = v;
    }
}

// reduced openings over the whole LDE domain: every column of every round enters the batch
struct ReducedHArgs {
    const uint32_t *lde_r, *lde_t, *lde_q[HCH], *d0, *d1;
    uint32_t* ro;
    const DevStateH* hs;
    uint32_t big;
};
__global__ void __launch_bounds__(256) reduced_openings_h_kernel(ReducedHArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.big) return;
    const DevStateH* __restrict__ hs = a.hs;
    // the row's 30 columns opened at zeta (random 8, trace 6, chunks 16) and its 6 trace columns again for zeta g
    uint32_t v[HRW + HTW + HCH * HD];
    {
        const uint4* r = reinterpret_cast<const uint4*>(a.lde_r + (size_t)i * HRW);
        const uint4 r0 = r[0], r1 = r[1];
        v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w; v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
        const uint2* t = reinterpret_cast<const uint2*>(a.lde_t + (size_t)i * HTW);
        const uint2 t0 = t[0], t1 = t[1], t2 = t[2];
        v[8] = t0.x; v[9] = t0.y; v[10] = t1.x; v[11] = t1.y; v[12] = t2.x; v[13] = t2.y;
#pragma unroll
        for (uint32_t c = 0; c < HCH; c++) {
            const uint4 q = *reinterpret_cast<const uint4*>(a.lde_q[c] + (size_t)i * HQS);
            v[14 + 4 * c] = q.x; v[15 + 4 * c] = q.y; v[16 + 4 * c] = q.z; v[17 + 4 * c] = q.w;
        }
    }
    // s0 = y0 - sum alp[k] v_k over the columns opened at zeta, s1 = y1 - the same over the trace columns at zeta g: sums of
    // extension-by-base products, taken two products per Montgomery reduction (bb::dot2).  Batch power index of column n of v:
    // n for n < 14 (random, trace @ zeta), n + 6 for the chunks (the six powers in between belong to trace @ zeta g).
    auto pw = [](uint32_t n) { return n < HRW + HTW ? n : n + HTW; };
    Ext d0 = bb::ext_zero(), d1 = bb::ext_zero();
#pragma unroll
    for (uint32_t n = 0; n < HRW + HTW + HCH * HD; n += 2)
#pragma unroll
        for (int c = 0; c < 4; c++) d0.c[c] = bb::add(d0.c[c], bb::dot2(hs->alp[pw(n)].c[c], v[n], hs->alp[pw(n + 1)].c[c], v[n + 1]));
#pragma unroll
    for (uint32_t n = 0; n < HTW; n += 2)
#pragma unroll
        for (int c = 0; c < 4; c++)
            d1.c[c] = bb::add(d1.c[c], bb::dot2(hs->alp[HRW + HTW + n].c[c], v[HRW + n], hs->alp[HRW + HTW + n + 1].c[c], v[HRW + n + 1]));
    const Ext s0 = bb::sub(hs->y0, d0), s1 = bb::sub(hs->y1, d1);
    const Ext e0 = ld_ext(a.d0 + 4 * (size_t)i), e1 = ld_ext(a.d1 + 4 * (size_t)i);
    st_ext(a.ro + 4 * (size_t)i, bb::add(bb::mul(s0, e0), bb::mul(s1, e1)));
}

// ---- transcript kernels of the hiding protocol (the FRI rounds, the final polynomial and the queries are the
// non-hiding prover's kernels, launched by the host code both provers share: ProverCore in prover.hip) ----
struct StageLayoutH {  // extends StageLayout: three roots, 36 opened values
    StageLayout s;
    uint32_t root_r;
};
__global__ void __launch_bounds__(64) ts_begin_h_kernel(TsArgs a, const uint32_t* trace, uint32_t h, uint32_t log_n, TsPis given) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    DevChal ch;
    ch.begin(a.kind, a.ds, &ks, true);
    uint32_t pis[3];
    if (given.given) {
        for (int k = 0; k < 3; k++) pis[k] = given.w[k];
    } else {
        pis[0] = trace[0]; pis[1] = trace[1]; pis[2] = trace[2 * (size_t)(h - 1) + 1];
    }
    ch.observe(bb::to_monty(log_n + 1));  // log_ext_degree = log_degree + is_zk
    ch.observe(bb::to_monty(log_n));      // log_degree
    ch.observe_n(a.ps + a.lay.root_t, 8);
    ch.observe_n(pis, 3);
    const Ext alpha = ch.sample_ext();
    Ext ap[5];
    ap[0] = bb::ext_one();
#pragma unroll
    for (int k = 1; k < 5; k++) ap[k] = bb::mul(ap[k - 1], alpha);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; k++) a.ds->pis[k] = pis[k];
        for (int k = 0; k < 5; k++) a.ds->apow[k] = ap[k];
        a.ds->status = 0;
        a.ps[a.lay.status] = 0;
    }
    ch.end();
}
__global__ void __launch_bounds__(64) ts_zeta_h_kernel(TsArgs a, uint32_t root_r, uint32_t g_h) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    DevChal ch;
    ch.begin(a.kind, a.ds, &ks, false);
    ch.observe_n(a.ps + a.lay.root_q, 8);
    ch.observe_n(a.ps + root_r, 8);
    const Ext zeta = ch.sample_ext();
    const Ext zeta_next = bb::scale(zeta, g_h);
    if (threadIdx.x == 0) {
        a.ds->zeta = zeta;
        a.ds->zeta_next = zeta_next;
        a.ds->k0 = den_consts(zeta);
        a.ds->k1 = den_consts(zeta_next);
    }
    ch.end();
}
// partial sums of the seven barycentric launches -> the 36 opened values (order: random, trace @ zeta, trace @ zeta g,
// chunks), observed; batch challenge powers; the two constant sums of the reduced openings
constexpr int TS_OPEN_H_THREADS = 1024;
__global__ void __launch_bounds__(TS_OPEN_H_THREADS) ts_open_h_kernel(TsArgs a, DevStateH* hs, const uint32_t* partials,
                                                                      uint32_t n_blocks, uint32_t log_ext, uint32_t sn, uint32_t denom) {
    P3_LATENCY_BOUND_KERNEL();
    __shared__ KState ks;
    __shared__ uint32_t red[4][7][32];
    __shared__ uint32_t tot[7][32];
    __shared__ uint32_t opened[HOPEN][4];
    {   // all seven sets at once: thread = (quarter of the blocks, set, column), four independent loads in flight
        const uint32_t col = threadIdx.x & 31u, set = (threadIdx.x >> 5) & 7u, part = threadIdx.x >> 8;
        if (set < 7u) {
            const uint32_t* p = partials + (size_t)set * n_blocks * 32 + col;
            uint32_t v = 0, b = part;
            for (; b + 12 < n_blocks; b += 16) {
                const uint32_t p0 = p[(size_t)b * 32], p1 = p[(size_t)(b + 4) * 32], p2 = p[(size_t)(b + 8) * 32], p3 = p[(size_t)(b + 12) * 32];
                v = bb::add(bb::add(v, bb::add(p0, p1)), bb::add(p2, p3));
            }
            for (; b < n_blocks; b += 4) v = bb::add(v, p[(size_t)b * 32]);
            red[part][set][col] = v;
        }
        __syncthreads();
        if (part == 0 && set < 7u) tot[set][col] = bb::add(bb::add(red[0][set][col], red[1][set][col]), bb::add(red[2][set][col], red[3][set][col]));
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    DevChal ch;
    ch.begin(a.kind, a.ds, &ks, false);
    Ext z0 = a.ds->zeta, z1 = a.ds->zeta_next;
    for (uint32_t i = 0; i < log_ext; i++) { z0 = bb::sqr(z0); z1 = bb::sqr(z1); }
    const Ext f0 = bb::scale(bb::sub(z0, bb::ext_from_base(sn)), denom);
    const Ext f1 = bb::scale(bb::sub(z1, bb::ext_from_base(sn)), denom);
    // sets: 0 random (8) @ zeta, 1 trace (6) @ zeta, 2 trace (6) @ zeta g, 3..6 chunks (4 each) @ zeta; lane k owns opened value k
    constexpr uint32_t FIRST[8] = {0, HRW, HRW + HTW, HRW + 2 * HTW, HRW + 2 * HTW + HD, HRW + 2 * HTW + 2 * HD, HRW + 2 * HTW + 3 * HD, HOPEN};
    static_assert(FIRST[7] == HRW + 2 * HTW + 4 * HD, "opened values: 8 + 6 + 6 + 4 x 4");
    if (threadIdx.x < HOPEN) {
        uint32_t set = 0;
#pragma unroll
        for (uint32_t t = 1; t < 7; t++) set += threadIdx.x >= FIRST[t] ? 1u : 0u;
        uint32_t first = 0;
#pragma unroll
        for (uint32_t t = 1; t < 7; t++) first = set == t ? FIRST[t] : first;
        const uint32_t j = threadIdx.x - first;
        Ext v;
        for (int c = 0; c < 4; c++) v.c[c] = tot[set][4 * j + c];
        v = bb::mul(v, set == 2 ? f1 : f0);
        for (int c = 0; c < 4; c++) { opened[threadIdx.x][c] = v.c[c]; a.ps[a.lay.opened + 4 * threadIdx.x + c] = v.c[c]; }
    }
    lds_wave_sync();
    for (uint32_t k = 0; k < HOPEN; k++) {
        Ext v;
        for (int c = 0; c < 4; c++) v.c[c] = opened[k][c];
        ch.observe_ext(v);
    }
    const Ext al = ch.sample_ext();
    Ext al_pow = bb::ext_one(), y0 = bb::ext_zero(), y1 = bb::ext_zero();
    for (uint32_t k = 0; k < HOPEN; k++) {
        Ext v;
        for (int c = 0; c < 4; c++) v.c[c] = opened[k][c];
        if (threadIdx.x == 0) hs->alp[k] = al_pow;
        const Ext term = bb::mul(al_pow, v);
        if (k >= FIRST[2] && k < FIRST[3]) y1 = bb::add(y1, term); else y0 = bb::add(y0, term);
        al_pow = bb::mul(al_pow, al);
    }
    if (threadIdx.x == 0) { hs->y0 = y0; hs->y1 = y1; }
    ch.end();
}

#include "prover_tiny.hip.inc"

// ------------------------------------------------------------------------------------------------
struct FibHidingProver::Impl : ProverCore {
    uint32_t log_n = 0, log_ext = 0;
    uint64_t seed = 1;
    // the three stream fills depend on nothing but the seed: they run on a side stream from the start of a proof, under the
    // trace generation, its LDE and (the FRI salts) everything up to the commit phase; each consumer waits for its fill's event
    hipStream_t side = nullptr;
    hipEvent_t ev_start = nullptr, ev_pcs = nullptr, ev_mmcs = nullptr, ev_fri = nullptr;
    // The randomization-polynomial commitment (LDE of the 2h x 8 random matrix + its salted tree: a fifth of a proof's work) depends on
    // nothing but two fills, so it CAN run on a second side stream under the trace and quotient commitments and join before zeta is
    // sampled.  Part of the LATENCY profile (round 4: an environment switch): a single 2^19-row proof 5.5-5.6 -> 5.3-5.4 ms, but four provers
    // gain nothing (186.1 / 187.2 / 188.9 / 186.4 without, 186.1 / 165.3 / 185.6 / 184.7 with: twelve streams on eight hardware queues
    // now and then put one prover's side work in front of another's main chain).  The fills' side stream, in contrast, is worth
    // +7 % to the four-prover bench (176-180 -> 188-194) and stays on.
    hipStream_t side2 = nullptr;
    hipEvent_t ev_r = nullptr;
    // arena
    uint32_t *trace = nullptr, *rnd_t = nullptr, *rt = nullptr, *lde_t = nullptr, *salt_t = nullptr, *layers_t = nullptr;
    uint32_t *qchunks = nullptr, *t012 = nullptr, *co = nullptr, *ext = nullptr, *ev2 = nullptr;
    uint32_t *lde_qb = nullptr, *lde_q[HCH] = {nullptr}, *salt_q[HCH] = {nullptr}, *layers_q = nullptr;  // lde_q[c] = lde_qb + c HD, row stride HQS
    uint2* sel_fl = nullptr;     // cached selectors on the quotient coset (selectors_h_kernel)
    uint32_t* sel_tr = nullptr;
    uint32_t *rm = nullptr, *lde_r = nullptr, *salt_r = nullptr, *layers_r = nullptr;
    uint32_t *d0 = nullptr, *d1 = nullptr, *partials = nullptr;
    uint32_t *pcs_draws = nullptr, *mmcs_draws = nullptr;
    size_t pcs_words = 0, mmcs_words = 0;
    bool one_fill = false;
    bool tiny = false;  // the whole proof in one launch of one workgroup (prover_tiny.hip.inc): latency profile, instances that fit
    uint32_t* rng_ws = nullptr;
    DevStateH* hs = nullptr;
    DevRng* rngs = nullptr;  // [0] input mmcs, [1] fri mmcs, [2] pcs
    uint32_t* host_stage = nullptr;
    uint32_t root_r_off = 0;
    uint32_t bary_blocks = 0;
    ~Impl() {
        if (host_stage) (void)hipHostFree(host_stage);
        for (hipEvent_t e : {ev_start, ev_pcs, ev_mmcs, ev_fri, ev_r}) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        if (side2) (void)hipStreamDestroy(side2);
    }
};

FibHidingProver::FibHidingProver() : im(new Impl()) {}
FibHidingProver::~FibHidingProver() { delete im; }

int FibHidingProver::init(uint32_t log_n, const FriParams& fp, hipStream_t stream, bool own_stream, int hash, uint64_t seed, int profile) {
    Impl& s = *im;
    int rc;
    if ((rc = s.begin("hiding prover", stream, own_stream, hash, profile))) return rc;
    s.seed = seed; s.salt_words = HSALT;
    if (log_n < 1 || fp.log_blowup < 1) return fail(ERR_BAD_ARG, "hiding prover: log_n and log_blowup must be >= 1");
    s.log_n = log_n; s.log_ext = log_n + 1;
    if (s.log_ext + fp.log_blowup > MAX_LOG_DOMAIN_HIDING)
        return fail(ERR_BAD_ARG, "hiding prover: LDE domain above 2^" + std::to_string(MAX_LOG_DOMAIN_HIDING) + " points (log_n + 1 + log_blowup)");
    if ((rc = s.set_fri("hiding prover", fp, s.log_ext))) return rc;
    const size_t h = (size_t)1 << log_n, h2 = 2 * h, big = (size_t)1 << s.log_big;
#define HA(ptr, words) if ((rc = s.alloc(&(ptr), (words)))) return rc
    // every draw of a proof has a known place in its stream, so each stream is ONE region filled by one launch set:
    //   pcs  : trace randomization | chunk blinding polynomials | randomization matrix
    //   mmcs : salts of the trace commitment | of the four chunks | of the randomization commitment
    //   fri  : salts of every commit-phase round, in round order (ProverCore::fri_salts)
    s.pcs_words = h * (HW + 2 * HNRC) + (HCH - 1) * h * HD + h2 * HRW;
    s.mmcs_words = (HCH + 2) * big * HSALT;
    HA(s.pcs_draws, s.pcs_words); HA(s.mmcs_draws, s.mmcs_words);
    s.rnd_t = s.pcs_draws; s.t012 = s.rnd_t + h * (HW + 2 * HNRC); s.rm = s.t012 + (HCH - 1) * h * HD;
    s.salt_t = s.mmcs_draws;
    for (uint32_t c = 0; c < HCH; c++) s.salt_q[c] = s.salt_t + (1 + c) * big * HSALT;
    s.salt_r = s.salt_t + (1 + HCH) * big * HSALT;
    HA(s.trace, h * 2); HA(s.rt, h2 * HTW); HA(s.lde_t, big * HTW);
    HA(s.layers_t, mmcs_layer_words(big));
    HA(s.qchunks, HCH * h * HD); HA(s.co, HCH * h * HD); HA(s.ext, HCH * h2 * HD); HA(s.ev2, HCH * h2 * HD);
    HA(s.lde_qb, big * HQS);
    for (uint32_t c = 0; c < HCH; c++) s.lde_q[c] = s.lde_qb + c * HD;
    { uint32_t* p = nullptr; HA(p, 4 * h * 2); s.sel_fl = reinterpret_cast<uint2*>(p); }
    HA(s.sel_tr, 4 * h);
    HA(s.layers_q, mmcs_layer_words(big));
    HA(s.lde_r, big * HRW); HA(s.layers_r, mmcs_layer_words(big));
    HA(s.d0, big * 4); HA(s.d1, big * 4);
    s.bary_blocks = (uint32_t)std::min<size_t>(256, (h2 + BARY_BLOCK - 1) / BARY_BLOCK);
    HA(s.partials, (size_t)7 * s.bary_blocks * 32);
    if ((rc = s.alloc_fri())) return rc;
    { uint32_t* p = nullptr; HA(p, (sizeof(DevStateH) + 3) / 4); s.hs = reinterpret_cast<DevStateH*>(p); P3_HIP(hipMemset(s.hs, 0, sizeof(DevStateH))); }
    { uint32_t* p = nullptr; HA(p, 3 * sizeof(DevRng) / 4); s.rngs = reinterpret_cast<DevRng*>(p); }
    {
        // one fill per stream when the jump tables reach that far (up to 2^30 raw draws), else piece by piece
        s.one_fill = rng_fill_supported(s.pcs_words) && rng_fill_supported(s.mmcs_words) && rng_fill_supported(s.fri_salt_words);
        if (const char* e = getenv("P3HIP_HIDING_PIECEWISE")) if (e[0] == '1') s.one_fill = false;  // tests: the large-size path
        const uint64_t n_max = s.one_fill ? std::max<uint64_t>(std::max<uint64_t>(s.pcs_words, s.mmcs_words), s.fri_salt_words)
                                          : std::max<uint64_t>(big * HSALT, h2 * HRW);
        size_t w = 0;
        if ((rc = rng_workspace_words(n_max, &w))) return rc;
        HA(s.rng_ws, w);
    }
#undef HA
    // the trees opened per query: the randomization matrix, the randomized trace, the four chunks (then the FRI rounds'), each
    // matrix with its salt
    const uint32_t lb = s.log_big, nq = fp.num_queries;
    s.trees.push_back(QTree{{s.lde_r, s.salt_r}, {HRW, HSALT}, {HRW, HSALT}, 2, s.layers_r, lb});
    s.trees.push_back(QTree{{s.lde_t, s.salt_t}, {HTW, HSALT}, {HTW, HSALT}, 2, s.layers_t, lb});
    {
        QTree t{};
        for (uint32_t c = 0; c < HCH; c++) {
            t.mat[c] = s.lde_q[c]; t.width[c] = HD; t.stride[c] = HQS;
            t.mat[HCH + c] = s.salt_q[c]; t.width[HCH + c] = t.stride[HCH + c] = HSALT;
        }
        t.n_mats = 2 * HCH; t.layers = s.layers_q; t.log_height = lb;
        s.trees.push_back(t);
    }
    StageLayout& L = s.lay;
    s.root_r_off = 16; L.opened = 24; L.froots = L.opened + 4 * HOPEN;
    if ((rc = s.layout("hiding prover", 1))) return rc;  // + the random streams' shortage flag
    P3_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.host_stage), (size_t)L.words * 4 + 64));
    {   // selectors of the trace domain on the quotient coset: fixed by log_n, computed once
        Context* cxp;
        if ((rc = get_context(&cxp))) return rc;
        TwoLevelTable roots;
        if ((rc = cxp->get_root_table(stream, log_n + 2, false, &roots))) return rc;
        const uint32_t gen = bb::to_monty(bb::GEN), gh = bb::pow(gen, h), w4 = bb::two_adic_generator(2);
        Zh4 zh;
        uint32_t p = bb::ONE;
        for (int c = 0; c < 4; c++) { zh.v[c] = bb::sub(bb::mul(gh, p), bb::ONE); p = bb::mul(p, w4); }
        hipLaunchKernelGGL(selectors_h_kernel, dim3((uint32_t)((h + 255) / 256)), dim3(256), 0, stream, roots, (uint32_t)h, log_n, gen,
                           bb::inv(bb::two_adic_generator(log_n)), zh, s.sel_fl, s.sel_tr);
        P3_HIP(hipGetLastError());
    }
    // The whole proof in ONE launch (prover_tiny.hip.inc) — latency profile, instances that fit a workgroup: an LDE domain of at most
    // 2^8 points, every random stream within one wave's small fill, a proof-of-work search short enough to run candidate by candidate
    // on one wave.  The reference's own instance (n = 8, fib_air.rs:56-72) is one of them.
    s.tiny = profile == PROFILE_LATENCY && s.log_big <= TINY_MAX_LOG_BIG && s.n_rounds <= TINY_MAX_ROUNDS && fp.proof_of_work_bits <= 4 &&
             nq <= 64 && rng_small_chunks(s.pcs_words) && rng_small_chunks(s.mmcs_words) && (s.fri_salt_words == 0 || rng_small_chunks(s.fri_salt_words)) &&
             s.fri_vec_words <= 0xffffffffull && s.fri_layer_words <= 0xffffffffull;
    // fills on a side stream under both profiles (+7 % with four provers, profiles/r04_latency_ab.txt); the randomization commitment
    // on a SECOND side stream under the latency profile only (a lone 2^19-row proof 5.5 -> 5.3 ms; four provers gain nothing and now
    // and then lose: twelve streams on eight hardware queues)
    if (s.one_fill && !s.tiny) {
        P3_HIP(hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking));
        for (hipEvent_t* e : {&s.ev_start, &s.ev_pcs, &s.ev_mmcs, &s.ev_fri}) P3_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        if (profile == PROFILE_LATENCY) {
            P3_HIP(hipStreamCreateWithFlags(&s.side2, hipStreamNonBlocking));
            P3_HIP(hipEventCreateWithFlags(&s.ev_r, hipEventDisableTiming));
        }
    }
    return OK;
}

int FibHidingProver::prove(uint64_t a, uint64_t b, std::vector<uint8_t>* proof) { return prove_any(a, b, nullptr, nullptr, proof); }
int FibHidingProver::prove_trace(const uint32_t* d_trace, const uint32_t pis[3], std::vector<uint8_t>* proof) {
    if (!d_trace || !pis) return fail(ERR_BAD_ARG, "hiding prover: null trace or public values");
    return prove_any(0, 0, d_trace, pis, proof);
}
uint32_t* FibHidingProver::arena_trace() const { return im->trace; }
hipStream_t FibHidingProver::stream() const { return im->stream; }
uint32_t FibHidingProver::log_n() const { return im->log_n; }
int FibHidingProver::device() const { return im->device; }
// d_trace == nullptr: (a, b)'s trace is generated (in the arena, or inside the one-launch kernel) and the public values are read from it
int FibHidingProver::prove_any(uint64_t a, uint64_t b, const uint32_t* d_trace, const uint32_t* pis, std::vector<uint8_t>* proof) {
    Impl& s = *im;
    const TsPis given = pis ? TsPis{{pis[0], pis[1], pis[2]}, 1} : TsPis{{0, 0, 0}, 0};
    Context* cxp;
    int rc = get_context(&cxp);
    if (rc) return rc;
    Context& cx = *cxp;
    if (cx.device != s.device) return fail(ERR_BAD_ARG, "hiding prover: created on another device");
    hipStream_t st = s.stream;
    const uint32_t log_n = s.log_n, log_ext = s.log_ext, log_big = s.log_big;
    const uint32_t h = 1u << log_n, h2 = 2 * h, big = 1u << log_big, log_q = log_n + 2;
    const uint32_t gen = bb::to_monty(bb::GEN);
    const uint32_t g_h = bb::two_adic_generator(log_n);
    const StageLayout& L = s.lay;
    DevState* ds = &s.hs->base;
    const TsArgs ts{ds, s.pstage, s.hash, L};
    DevRng *rng_mmcs = s.rngs, *rng_fri = s.rngs + 1, *rng_pcs = s.rngs + 2;
    // the streams' shortage flag is the word right behind the staging buffer: it travels with the proof's one device-to-host copy and is
    // cleared by the launch that seeds the three streams (no memset, no second copy: at the reference's n = 8 a proof IS its launches)
    uint32_t* err = s.pstage + L.words;
    const uint32_t nq = s.fp.num_queries;
    const uint32_t* const hp = s.host_stage;
    if (s.tiny) {
        // ---- one launch: prover_tiny.hip.inc ----
        TinyArgs ta{};
        ta.hash = (uint32_t)s.hash; ta.log_n = log_n; ta.log_blowup = s.fp.log_blowup; ta.log_fpl = s.fp.log_final_poly_len;
        ta.nq = nq; ta.pow_bits = s.fp.proof_of_work_bits;
        ta.a_monty = bb::to_monty((uint32_t)(a % bb::P)); ta.b_monty = bb::to_monty((uint32_t)(b % bb::P));
        rng_seed_from_u64(ta.seed, s.seed);
        if ((rc = rng_jump_table(cx, &ta.jump))) return rc;
        ta.n_pcs = (uint32_t)s.pcs_words; ta.n_mmcs = (uint32_t)s.mmcs_words; ta.n_fri = (uint32_t)s.fri_salt_words;
        // short chunks (64 raw draws per lane instead of 256) when every stream fits 64 of them: the reference's n = 8 instance does
        const bool short_chunks = rng_tiny_chunks(s.pcs_words) && rng_tiny_chunks(s.mmcs_words) && (!s.fri_salt_words || rng_tiny_chunks(s.fri_salt_words));
        ta.chunk_log = short_chunks ? RNG_TINY_CHUNK_LOG : RNG_CHUNK_LOG;
        if (short_chunks) {
            ta.jump += (size_t)RNG_MAX_JUMP * 256 * 4;  // slot RNG_MAX_JUMP of the table: T^64
            ta.ch_pcs = rng_tiny_chunks(s.pcs_words); ta.ch_mmcs = rng_tiny_chunks(s.mmcs_words);
            ta.ch_fri = s.fri_salt_words ? rng_tiny_chunks(s.fri_salt_words) : 0;
        } else {
            ta.ch_pcs = rng_small_chunks(s.pcs_words); ta.ch_mmcs = rng_small_chunks(s.mmcs_words);
            ta.ch_fri = s.fri_salt_words ? rng_small_chunks(s.fri_salt_words) : 0;
        }
        ta.pcs_draws = s.pcs_draws; ta.mmcs_draws = s.mmcs_draws; ta.fri_salts = s.fri_salts;
        ta.trace = s.trace; ta.in_trace = d_trace; ta.pis = given; ta.rt = s.rt; ta.lde_t = s.lde_t; ta.salt_t = s.salt_t; ta.layers_t = s.layers_t;
        ta.qchunks = s.qchunks; ta.co = s.co; ta.ext = s.ext; ta.lde_qb = s.lde_qb; ta.layers_q = s.layers_q; ta.t012 = s.t012;
        for (uint32_t c = 0; c < HCH; c++) ta.salt_q[c] = s.salt_q[c];
        ta.rm = s.rm; ta.lde_r = s.lde_r; ta.salt_r = s.salt_r; ta.layers_r = s.layers_r;
        ta.d0 = s.d0; ta.d1 = s.d1; ta.fri_vec = s.fri_vec; ta.fri_layers = s.fri_layers; ta.fp_ev = s.fp_ev;
        ta.n_rounds = s.n_rounds;
        for (uint32_t r = 0; r <= s.n_rounds; r++) ta.fri_vec_off[r] = (uint32_t)s.fri_vec_off[r];
        for (uint32_t r = 0; r < s.n_rounds; r++) { ta.fri_salt_off[r] = (uint32_t)s.fri_salt_off[r]; ta.fri_layer_off[r] = (uint32_t)s.fri_layer_off[r]; }
        ta.hs = s.hs; ta.pstage = s.pstage; ta.lay = L; ta.root_r_off = s.root_r_off; ta.slot_words = (uint32_t)s.slot_words;
        ta.qtrees = s.qtrees; ta.n_trees = (uint32_t)s.trees.size(); ta.qidx = s.qidx; ta.err = err;
        // three waves' raw candidates + the domain tables behind them (at most 2^8 + 2^7 + 2^6 + 4 x 2^6 words)
        const size_t lds = (size_t)3 * RNG_SMALL_CHUNKS * RNG_SMALL_STRIDE * 4 + 4096;
        if ((rc = cx.ensure_dynamic_lds(reinterpret_cast<const void*>(tiny_hiding_prover_kernel), (int)lds))) return rc;
        hipLaunchKernelGGL(tiny_hiding_prover_kernel, dim3(1), dim3(TINY_THREADS), lds, st, ta);
        P3_HIP(hipGetLastError());
        P3_HIP(hipMemcpyAsync(s.host_stage, s.pstage, ((size_t)L.words + 1) * 4, hipMemcpyDeviceToHost, st));
        P3_HIP(hipStreamSynchronize(st));
    } else {
        // A proof that FAILED between enqueuing its side-stream work and joining it (an error return from a transform, a commitment, a
        // table reservation) leaves fills or the randomization commitment in flight: they write s.rngs, the shortage flag and the draw
        // buffers.  The seeding launch below must not overtake them, so the main stream first joins whatever the side streams were last
        // given (waiting for an event that was never recorded, or has completed, costs nothing).
        if (s.side) P3_HIP(hipStreamWaitEvent(st, s.ev_fri, 0));
        if (s.side2) P3_HIP(hipStreamWaitEvent(st, s.ev_r, 0));
        if ((rc = rng_seed(st, s.rngs, s.seed, 3, err))) return rc;
        auto fill = [&](DevRng* r, uint32_t* out, uint64_t n) {
            return s.one_fill ? OK : rng_fill_field(cx, st, r, out, n, s.rng_ws, err);  // piecewise only when the whole stream does not fit one fill
        };
        if (s.one_fill) {
            // on the side stream when there is one: it starts after everything the main stream holds so far (the previous proof's
            // readers of these buffers, this proof's seeds), and the main stream waits for each fill where its first consumer is
            hipStream_t fs = s.side ? s.side : st;
            if (s.side) { P3_HIP(hipEventRecord(s.ev_start, st)); P3_HIP(hipStreamWaitEvent(s.side, s.ev_start, 0)); }
            if ((rc = rng_fill_field(cx, fs, rng_pcs, s.pcs_draws, s.pcs_words, s.rng_ws, err))) return rc;
            if (s.side) P3_HIP(hipEventRecord(s.ev_pcs, s.side));
            if ((rc = rng_fill_field(cx, fs, rng_mmcs, s.mmcs_draws, s.mmcs_words, s.rng_ws, err))) return rc;
            if (s.side) P3_HIP(hipEventRecord(s.ev_mmcs, s.side));
            if ((rc = rng_fill_field(cx, fs, rng_fri, s.fri_salts, s.fri_salt_words, s.rng_ws, err))) return rc;
            if (s.side) P3_HIP(hipEventRecord(s.ev_fri, s.side));
        }
        auto wait_fill = [&](hipEvent_t e) -> int { if (s.side) P3_HIP(hipStreamWaitEvent(st, e, 0)); return OK; };
        // hiding commitments (ProverCore::commit): leaf row = m0 || s0 || m1 || s1 ...
        const size_t w_r = HRW, w_t = HTW, w_q[HCH] = {HD, HD, HD, HD};
        // the randomization polynomial's commitment, early and on its own stream when there is one
        auto commit_random = [&](hipStream_t on) -> int {
            int r = ntt_coset_lde(cx, on, s.rm, s.lde_r, h2, HRW, s.fp.log_blowup, gen, true);
            if (r) return r;
            return s.commit(1, &s.lde_r, &w_r, &s.salt_r, big, s.layers_r, s.root_r_off, 0, on);
        };
        if (s.side2) {
            P3_HIP(hipStreamWaitEvent(s.side2, s.ev_start, 0));  // the previous proof's readers of lde_r / layers_r / the root slot
            P3_HIP(hipStreamWaitEvent(s.side2, s.ev_pcs, 0));    // rm
            P3_HIP(hipStreamWaitEvent(s.side2, s.ev_mmcs, 0));   // salt_r
            if ((rc = commit_random(s.side2))) return rc;
            P3_HIP(hipEventRecord(s.ev_r, s.side2));
        }

        // ---- randomized trace + commit ----
        const uint32_t* trace = d_trace ? d_trace : s.trace;  // a caller's trace is randomized where it lies
        if (!d_trace && (rc = fib_trace(st, a, b, h, s.trace))) return rc;
        if ((rc = fill(rng_pcs, s.rnd_t, (uint64_t)h * (HW + 2 * HNRC)))) return rc;
        if ((rc = wait_fill(s.ev_pcs))) return rc;
        hipLaunchKernelGGL(randomize_trace_kernel, dim3((h + 255) / 256), dim3(256), 0, st, reinterpret_cast<const uint2*>(trace), s.rnd_t, h, s.rt);
        P3_HIP(hipGetLastError());
        if ((rc = ntt_coset_lde(cx, st, s.rt, s.lde_t, h2, HTW, s.fp.log_blowup, gen, true))) return rc;
        if ((rc = fill(rng_mmcs, s.salt_t, (uint64_t)big * HSALT))) return rc;
        if ((rc = wait_fill(s.ev_mmcs))) return rc;
        if ((rc = s.commit(1, &s.lde_t, &w_t, &s.salt_t, big, s.layers_t, L.root_t))) return rc;
        hipLaunchKernelGGL(ts_begin_h_kernel, dim3(1), dim3(64), 0, st, ts, trace, h, log_n, given);
        P3_HIP(hipGetLastError());

        // ---- quotient on GENERATOR <g_4h>, four blinded chunks, commit ----
        // The four chunks travel as ONE 16-word-wide matrix from here to their commitment: one inverse transform, one blinding pass,
        // one coset LDE (until round 4: four of each on 4-word-wide matrices, twelve general-plan launches for the inverse alone).
        {
            QuotHArgs qa{};
            qa.lde = s.lde_t; qa.chunks = s.qchunks; qa.ds = ds; qa.sel_fl = s.sel_fl; qa.sel_tr = s.sel_tr;
            qa.h = h; qa.log_h = log_n;
            const uint32_t gh = bb::pow(gen, h), w4 = bb::two_adic_generator(2);
            uint32_t p = bb::ONE;
            for (int c = 0; c < 4; c++) { qa.zh_inv[c] = bb::inv(bb::sub(bb::mul(gh, p), bb::ONE)); p = bb::mul(p, w4); }
            hipLaunchKernelGGL(fib_quotient_h_kernel, dim3((h + 255) / 256), dim3(256), 0, st, qa);
            P3_HIP(hipGetLastError());
        }
        if ((rc = fill(rng_pcs, s.t012, (uint64_t)(HCH - 1) * h * HD))) return rc;
        if ((rc = ntt_dft(cx, st, s.qchunks, s.co, h, HQS, true))) return rc;
        {
            BlindArgs ba{};
            ba.co = s.co; ba.t012 = s.t012; ba.ext = s.ext; ba.h = h;
            const uint32_t gh = bb::pow(gen, h), w4 = bb::two_adic_generator(2), g4 = bb::two_adic_generator(log_q);
            uint32_t sh[HCH], kc[HCH], p = bb::ONE;
            for (uint32_t c = 0; c < HCH; c++) { sh[c] = bb::mul(gh, p); p = bb::mul(p, w4); }
            if ((rc = cx.reserve_scale_slots(HCH))) return rc;  // the four tables below stay valid until the kernel is enqueued
            for (uint32_t c = 0; c < HCH; c++) {
                uint32_t k = bb::ONE;
                for (uint32_t j = 0; j < HCH; j++) if (j != c) k = bb::mul(k, bb::sub(sh[c], sh[j]));
                kc[c] = k;
                ba.sh[c] = sh[c]; ba.kinv[c] = bb::inv(k);
                if ((rc = cx.get_scale_table(st, bb::inv(bb::mul(gen, bb::pow(g4, c))), log_n, bb::ONE, &ba.sp[c]))) return rc;
            }
            ba.k_last = kc[HCH - 1];
            hipLaunchKernelGGL(blind_chunks_kernel, dim3((h + 255) / 256), dim3(256), 0, st, ba);
            P3_HIP(hipGetLastError());
        }
        // values of the blinded chunk polynomials on GENERATOR <g_big>: the same coset LDE as every other committed matrix, straight
        // from the coefficients where the narrow plan covers the shape (no forward transform to <g_2h> and back)
        if ((rc = ntt_coset_lde_from_coeffs(cx, st, s.ext, s.lde_qb, s.ev2, h2, HQS, s.fp.log_blowup, gen))) return rc;
        for (uint32_t c = 0; c < HCH; c++) if ((rc = fill(rng_mmcs, s.salt_q[c], (uint64_t)big * HSALT))) return rc;
        if ((rc = s.commit(HCH, s.lde_q, w_q, s.salt_q, big, s.layers_q, L.root_q, HQS))) return rc;

        // ---- randomization polynomial commitment ----
        if (s.side2) {
            P3_HIP(hipStreamWaitEvent(st, s.ev_r, 0));  // committed on the second side stream since the proof's start
        } else {
            if ((rc = fill(rng_pcs, s.rm, (uint64_t)h2 * HRW))) return rc;
            if ((rc = fill(rng_mmcs, s.salt_r, (uint64_t)big * HSALT))) return rc;
            if ((rc = commit_random(st))) return rc;
        }
        hipLaunchKernelGGL(ts_zeta_h_kernel, dim3(1), dim3(64), 0, st, ts, s.root_r_off, g_h);
        P3_HIP(hipGetLastError());

        // ---- opened values: every committed column is a polynomial of degree < 2h ----
        TwoLevelTable roots_big;
        if ((rc = cx.get_root_table(st, log_big, false, &roots_big))) return rc;
        {
            uint32_t threads = (big + DEN_CHUNK - 1) / DEN_CHUNK;
            hipLaunchKernelGGL(inv_denoms_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, roots_big, big, log_big, gen, ds, s.d0, s.d1);
            P3_HIP(hipGetLastError());
            const size_t ps = (size_t)s.bary_blocks * 32;
            {
                // (the sweep leaves the unused words of a set's 32 untouched: ts_open_h_kernel adds them up and never uses those sums)
                BaryAllArgs ba{};
                ba.roots = roots_big; ba.n2 = h2; ba.log_big = log_big; ba.gen = gen;
                ba.lde_r = s.lde_r; ba.lde_t = s.lde_t;
                for (uint32_t c = 0; c < HCH; c++) ba.lde_q[c] = s.lde_q[c];
                ba.d0 = s.d0; ba.d1 = s.d1; ba.partials = s.partials; ba.set_stride = (uint32_t)ps;
                hipLaunchKernelGGL(bary_all_kernel, dim3(s.bary_blocks), dim3(BARY_BLOCK), 0, st, ba);
                P3_HIP(hipGetLastError());
            }
            const uint32_t sn = bb::pow(gen, h2);
            const uint32_t denom = bb::inv(bb::mul(bb::to_monty(h2), sn));
            hipLaunchKernelGGL(ts_open_h_kernel, dim3(1), dim3(TS_OPEN_H_THREADS), 0, st, ts, s.hs, s.partials, s.bary_blocks, log_ext, sn, denom);
            P3_HIP(hipGetLastError());
        }
        {
            ReducedHArgs ra{};
            ra.lde_r = s.lde_r; ra.lde_t = s.lde_t;
            for (uint32_t c = 0; c < HCH; c++) ra.lde_q[c] = s.lde_q[c];
            ra.d0 = s.d0; ra.d1 = s.d1; ra.ro = s.fri_vec + s.fri_vec_off[0]; ra.hs = s.hs; ra.big = big;
            hipLaunchKernelGGL(reduced_openings_h_kernel, dim3((big + 255) / 256), dim3(256), 0, st, ra);
            P3_HIP(hipGetLastError());
        }

        // ---- FRI commit phase: ExtensionMmcs over the hiding MMCS, salts from the `fri` stream; proof of work; query phase ----
        if ((rc = wait_fill(s.ev_fri))) return rc;
        for (uint32_t r = 0; r < s.n_rounds; r++)
            if ((rc = fill(rng_fri, s.fri_salts + s.fri_salt_off[r], (uint64_t)(big >> (r + 1)) * HSALT))) return rc;
        if ((rc = s.fri_rounds(cx, ts, s.n_rounds))) return rc;
        if ((rc = s.fri_final(cx, ts))) return rc;
        if ((rc = s.grind_start(ts))) return rc;
        const size_t words = (size_t)L.words + 1;  // + the shortage flag
        if ((rc = s.queries(ts, s.host_stage, words))) return rc;
        P3_HIP(hipStreamSynchronize(st));
        if (hp[L.status] == ST_GRIND_MISS && (rc = s.continue_grind(ts, s.host_stage, words))) return rc;
    }
    if (hp[L.status] != 0) return fail(ERR_INTERNAL, "grind: witness rejected by the device transcript");
    if (hp[L.words] != 0) return fail(ERR_INTERNAL, "rng: a random stream ran out of raw draws");

    // ---- serialise: wire format version 2 ----
    std::vector<uint8_t>& pf = *proof;
    pf.clear();
    pf.reserve(64 + (size_t)nq * (s.slot_words + 64) * 4 + 4096);
    put_u32(pf, PROOF_MAGIC); put_u32(pf, 2); put_u32(pf, log_n);
    put_words(pf, hp + L.root_t, 8); put_words(pf, hp + L.root_q, 8); put_words(pf, hp + s.root_r_off, 8);
    const uint32_t* op = hp + L.opened;
    put_u32(pf, HRW); put_words(pf, op, 4 * HRW); op += 4 * HRW;
    put_u32(pf, HTW); put_words(pf, op, 4 * HTW); op += 4 * HTW;
    put_u32(pf, HTW); put_words(pf, op, 4 * HTW); op += 4 * HTW;
    put_u32(pf, HCH);
    for (uint32_t c = 0; c < HCH; c++) { put_u32(pf, HD); put_words(pf, op, 4 * HD); op += 4 * HD; }
    s.put_fri(pf, hp);
    return OK;
}

}  // namespace p3
