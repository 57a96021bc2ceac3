// Mmcs::verify_batch (MerkleTreeMmcs / MerkleTreeHidingMmcs as the reference passes them into its PCS, native/src/fib_air.rs:40-51):
// the fourth method of the contract, for both hash configurations.
//   host    mmcs_verify_batch       one opening; what the proof verifiers (verifier.hip) and p3hip_mmcs_verify_batch run
//   device  mmcs_verify_many        n openings of ONE commitment in one launch, in the layout mmcs_open_many (mmcs.hip) writes
// Mixed heights as MerkleTree::new injects them: the matrices of the tallest height form the leaf row; after the compression at
// each level the rows of the matrices whose height equals that level's length are hashed and compressed in; matrix m contributes
// row index >> (log_max - log_h_m).  A hiding tree is verified with its salts listed as width-4 matrices (m0, s0, m1, s1 ...).
//
// Device forms.  All openings of a call share the dimensions, so the level loop, the injection levels and the absorb schedule are
// wave-uniform: the schedule (VerifySched) is computed on the host and passed by value; the left / right placement of the sibling
// is the only per-lane difference and is a select.
//   per lane     one opening per lane: Poseidon2 in exact-integer fp64 (poseidon2_f64.hip.h, what the large layers run), Keccak as
//                kk::permute / permute_digest.  Opened values are read from global memory as they are absorbed; a non-canonical
//                word or an index outside the tree decides the status whatever the hashes give, so the checks ride on those loads.
//   cooperative  (reached through the explicit form argument only until a same-run A/B has fixed the crossover: mmcs.h)
//                small n (one proof's 100 queries are two waves of the per-lane form, each lane walking depth + 1 dependent
//                permutations): one opening per 16-lane DPP row (poseidon2_coop.hip.h) / per wave (kk::f_coop), the forms of the
//                tree tops.
#include <algorithm>

#include "challenger.h"
#include "common.h"
#include "keccak.hip.h"
#include "lane_walk.hip.h"
#include "mmcs.h"
#include "poseidon2.hip.h"
#include "poseidon2_coop.hip.h"
#include "poseidon2_f64.hip.h"

namespace p3 {

// ------------------------------------------------------------------------------------------------
// host: one opening
// ------------------------------------------------------------------------------------------------
namespace {
void hash_row_host(int hash, const uint32_t* items, size_t n, uint32_t out[8]) {
    if (hash == HASH_KECCAK) { keccak_hash_row_host(items, n, out); return; }
    uint32_t st[16] = {0};  // PaddingFreeSponge<_, 16, 8, 8>
    for (size_t i = 0; i < n; i += 8) { size_t take = n - i < 8 ? n - i : 8; memcpy(st, items + i, take * 4); p2::permute(st); }
    memcpy(out, st, 32);
}
void compress_host(int hash, const uint32_t* l, const uint32_t* r, uint32_t out[8]) {
    if (hash == HASH_KECCAK) { keccak_compress_host(l, r, out); return; }
    uint32_t st[16];  // TruncatedPermutation<_, 2, 8, 16>
    memcpy(st, l, 32); memcpy(st + 8, r, 32); p2::permute(st); memcpy(out, st, 32);
}
int bad_arg(std::string* why, const char* msg) { if (why) *why = msg; return ERR_BAD_ARG; }
int reject(std::string* why, int code, const char* msg) { if (why) *why = msg; return code; }

// the checks every form shares; *log_max = log2 of the tallest height
int check_dims(int hash, const size_t* heights, const size_t* widths, size_t n_mats, uint32_t* log_max, size_t* row_words, std::string* why) {
    if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return bad_arg(why, "mmcs_verify_batch: unknown hash configuration");
    if (!heights || !widths) return bad_arg(why, "mmcs_verify_batch: null argument");
    if (!n_mats) return bad_arg(why, "mmcs_verify_batch: no matrices");
    if (n_mats > 64) return bad_arg(why, "mmcs_verify_batch: at most 64 matrices per commitment");
    uint64_t maxh = 0;
    size_t tot = 0;
    for (size_t m = 0; m < n_mats; m++) {
        if (!is_pow2(heights[m])) return bad_arg(why, "mmcs_verify_batch: heights must be powers of two");
        if (widths[m] > 0xffffffffull || tot + widths[m] > 0xffffffffull) return bad_arg(why, "mmcs_verify_batch: width too large");
        tot += widths[m];
        maxh = std::max<uint64_t>(maxh, heights[m]);
    }
    *log_max = log2u(maxh);
    *row_words = tot;
    return OK;
}
}  // namespace

int mmcs_verify_batch(int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats, size_t index,
                      const uint32_t* rows, const uint32_t* path, size_t path_len, std::string* why, bool check_canonical) {
    uint32_t log_max = 0;
    size_t row_words = 0;
    if (int rc = check_dims(hash, heights, widths, n_mats, &log_max, &row_words, why)) return rc;
    if (!root || (row_words && !rows) || (path_len && !path)) return bad_arg(why, "mmcs_verify_batch: null argument");
    if (path_len != log_max) return reject(why, MMCS_WRONG_HEIGHT, "mmcs_verify_batch: WrongHeight: the path length is not log2 of the tallest height");
    if ((uint64_t)index >> log_max) return reject(why, MMCS_BAD_INDEX, "mmcs_verify_batch: index outside the tallest matrix");
    for (size_t i = 0; check_canonical && i < row_words; i++)
        if (rows[i] >= bb::P) return reject(why, MMCS_NOT_CANONICAL, "mmcs_verify_batch: an opened value is not a canonical field element");
    if (check_canonical && hash == HASH_POSEIDON2)
        for (size_t i = 0; i < path_len * 8; i++)
            if (path[i] >= bb::P) return reject(why, MMCS_NOT_CANONICAL, "mmcs_verify_batch: a digest word is not a canonical field element");
    uint32_t small[64];  // the rows of one height class, concatenated: the proof verifiers' leaves (<= 32 words) never allocate
    std::vector<uint32_t> large;
    if (row_words > 64) large.resize(row_words);
    uint32_t* const buf = row_words > 64 ? large.data() : small;
    uint32_t cur[8], rh[8], nxt[8];
    for (uint32_t level = 0;; level++) {
        const uint64_t h = 1ull << (log_max - level);
        size_t k = 0, off = 0;
        bool any = false;
        for (size_t m = 0; m < n_mats; off += widths[m], m++)
            if (heights[m] == h) { if (widths[m]) memcpy(buf + k, rows + off, widths[m] * 4); k += widths[m]; any = true; }
        if (level == 0) hash_row_host(hash, buf, k, cur);
        else if (any) { hash_row_host(hash, buf, k, rh); compress_host(hash, cur, rh, nxt); memcpy(cur, nxt, 32); }
        if (level == log_max) break;
        const uint32_t* sib = path + 8 * (size_t)level;
        if ((index >> level) & 1) compress_host(hash, sib, cur, nxt); else compress_host(hash, cur, sib, nxt);
        memcpy(cur, nxt, 32);
    }
    if (memcmp(cur, root, 32) != 0) return reject(why, MMCS_ROOT_MISMATCH, "mmcs_verify_batch: RootMismatch");
    if (why) why->clear();
    return OK;
}

// ------------------------------------------------------------------------------------------------
// device: n openings of one commitment
// ------------------------------------------------------------------------------------------------
// The absorb schedule of one call.  Class c = the matrices of height 2^(depth - level[c]), tallest first (level[0] = 0); its
// concatenated row is the segments [seg_begin[c], seg_begin[c + 1]) of an opening's row words, in matrix order.
struct VerifySched {
    uint32_t root[8];
    uint32_t depth, row_words, n_classes;
    uint32_t level[MMCS_MAX_MATS];
    uint32_t total[MMCS_MAX_MATS];  // words of the class row
    uint32_t seg_begin[MMCS_MAX_MATS + 1];
    uint32_t seg_off[MMCS_MAX_MATS], seg_w[MMCS_MAX_MATS];
};
static_assert(sizeof(VerifySched) <= 2048, "passed by value in the kernel arguments");

// status of one opening from what its lanes saw
__device__ __forceinline__ uint32_t verdict(bool bad_index, bool not_canonical, bool mismatch) {
    return bad_index ? (uint32_t)MMCS_BAD_INDEX : not_canonical ? (uint32_t)MMCS_NOT_CANONICAL : mismatch ? (uint32_t)MMCS_ROOT_MISMATCH : 0u;
}

// ---- per lane: lane_walk.hip.h's injecting walk over the schedule ----
// The word source: a cursor over one opening's row words, class by class as the walk reaches their levels, segment by segment within a class.
struct SchedCursor {
    const VerifySched& a;
    const uint32_t* row;
    uint32_t c = 0, seg = 0, off = 0;  // next class; the segment and the offset in it of the next word
    __device__ __forceinline__ bool has(uint32_t l) const { return c < a.n_classes && a.level[c] == l; }
    __device__ __forceinline__ uint32_t len(uint32_t) {
        seg = a.seg_begin[c];
        off = 0;
        return a.total[c++];
    }
    __device__ __forceinline__ uint32_t word(uint32_t, uint32_t) {
        while (off >= a.seg_w[seg]) { seg++; off = 0; }
        return row[a.seg_off[seg] + off++];
    }
};
// sibling loader: the path arrays are 16-byte aligned (mmcs_verify_many checks), a digest is two 16-byte loads
struct PathDigests {
    const uint32_t* path;
    __device__ __forceinline__ void operator()(uint32_t l, uint32_t (&sw)[8]) const {
        const uint4* q = reinterpret_cast<const uint4*>(path + l * 8);
        const uint4 x = q[0], y = q[1];
        sw[0] = x.x; sw[1] = x.y; sw[2] = x.z; sw[3] = x.w;
        sw[4] = y.x; sw[5] = y.y; sw[6] = y.z; sw[7] = y.w;
    }
};
template <int HASH>
__device__ __forceinline__ void verify_lane(const VerifySched& a, const uint32_t* indices, uint64_t n, const uint32_t* rows, const uint32_t* paths,
                                            uint32_t* status, uint32_t* d_rejected) {
    if (gridDim.x <= 512u) P3_LATENCY_BOUND_KERNEL();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t index = indices[i];
    SchedCursor src{a, rows + i * a.row_words};
    uint32_t hi = 0;  // the largest opened value (Poseidon2: or digest word) seen: >= P decides the status
    const bool mismatch = lane_walk::walk<HASH, true>(src, PathDigests{paths + i * a.depth * 8}, a.depth, index, a.root, hi);
    const uint32_t st = verdict((index >> a.depth) != 0u, hi >= bb::P, mismatch);
    status[i] = st;
    count_rejected(st != 0u, d_rejected);
}
// (two kernels by name, not one template: the profiler output and the tools that read it know them as verify_lane_*_kernel)
__global__ void __launch_bounds__(256) verify_lane_p2_kernel(VerifySched a, const uint32_t* indices, uint64_t n, const uint32_t* rows,
                                                             const uint32_t* paths, uint32_t* status, uint32_t* d_rejected) {
    verify_lane<HASH_POSEIDON2>(a, indices, n, rows, paths, status, d_rejected);
}
__global__ void __launch_bounds__(256) verify_lane_keccak_kernel(VerifySched a, const uint32_t* indices, uint64_t n, const uint32_t* rows,
                                                                 const uint32_t* paths, uint32_t* status, uint32_t* d_rejected) {
    verify_lane<HASH_KECCAK>(a, indices, n, rows, paths, status, d_rejected);
}

// element e of class c's row: its position in an opening's row words (e < total[c]; a short walk over the class's segments)
__device__ __forceinline__ uint32_t class_word_pos(const VerifySched& a, uint32_t c, uint32_t e) {
    uint32_t seg = a.seg_begin[c];
    while (e >= a.seg_w[seg]) { e -= a.seg_w[seg]; seg++; }
    return a.seg_off[seg] + e;
}

// ---- cooperative, Poseidon2: one opening per 16-lane DPP row, one state element per lane (int32 Montgomery, poseidon2_coop.hip.h) ----
__global__ void __launch_bounds__(256) verify_coop_p2_kernel(VerifySched a, const uint32_t* indices, uint32_t n, const uint32_t* rows,
                                                             const uint32_t* paths, uint32_t* status, uint32_t* d_rejected) {
    P3_LATENCY_BOUND_KERNEL();
    const uint32_t lane16 = threadIdx.x & 15u;
    const p2c::LaneConst lc = p2c::lane_constants(lane16);
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool act = i < n;  // idle rows run the permutations on zeros: every lane of a wave takes part in the exchanges
    const uint32_t index = act ? indices[i] : 0u;
    const uint32_t* row = rows + (size_t)(act ? i : 0u) * a.row_words;
    const uint32_t* path = paths + (size_t)(act ? i : 0u) * a.depth * 8;
    const bool low = lane16 < 8u;
    uint32_t hi = 0, v = 0, cur = 0;  // lanes 0..7 of the row hold the running digest
    uint32_t c = 0;
    for (uint32_t l = 0; l <= a.depth; l++) {
        const bool has = c < a.n_classes && a.level[c] == l;
        if (has) {
            cur = v;
            v = 0;
            const uint32_t total = a.total[c];
            for (uint32_t k = 0; k < total; k += 8) {
                if (act && low && k + lane16 < total) {
                    v = row[class_word_pos(a, c, k + lane16)];
                    hi = max(hi, v);
                }
                v = p2c::permute(v, lc);
            }
            if (!total) v = 0;
            if (l > 0) {  // compress(cur, row digest): the digest moves to lanes 8..15
                const uint32_t rot = p2c::dpp<p2c::ROW_ROR(8)>(v);
                v = p2c::permute(low ? cur : rot, lc);
            }
            c++;
        }
        if (l == a.depth) break;
        const uint32_t sw = act ? path[l * 8 + (lane16 & 7u)] : 0u;
        hi = max(hi, sw);
        const bool right = (index >> l) & 1u;
        const uint32_t rot = p2c::dpp<p2c::ROW_ROR(8)>(v);
        v = p2c::permute(low != right ? (low ? v : rot) : sw, lc);
    }
    const uint64_t grp = 0xffffull << (threadIdx.x & 48u);
    const bool mismatch = (__builtin_amdgcn_ballot_w64(low && v != a.root[lane16 & 7u]) & grp) != 0;
    const bool noncanon = (__builtin_amdgcn_ballot_w64(hi >= bb::P) & grp) != 0;
    const uint32_t st = verdict((index >> a.depth) != 0u, noncanon, mismatch);
    const bool writer = act && lane16 == 0u;
    if (writer) status[i] = st;
    count_rejected(writer && st != 0u, d_rejected);
}

// ---- cooperative, Keccak: one opening per wave, state word x + 5y in lane x + 8y (kk::f_coop) ----
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src_lane) {
    const int addr = (int)(4u * src_lane);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__global__ void __launch_bounds__(256) verify_coop_keccak_kernel(VerifySched a, const uint32_t* indices, uint32_t n, const uint32_t* rows,
                                                                 const uint32_t* paths, uint32_t* status, uint32_t* d_rejected) {
    P3_LATENCY_BOUND_KERNEL();
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= n) return;  // uniform over the wave
    const uint32_t idx = kk::coop_index();  // the state word this lane holds; words 0..3 (lanes 0..3) are a digest
    const uint32_t index = indices[i];
    const uint32_t* row = rows + (size_t)i * a.row_words;
    const uint64_t* path = reinterpret_cast<const uint64_t*>(paths + (size_t)i * a.depth * 8);
    uint32_t hi = 0;
    uint64_t v = 0, cur = 0;
    uint32_t c = 0;
    for (uint32_t l = 0; l <= a.depth; l++) {
        const bool has = c < a.n_classes && a.level[c] == l;
        if (has) {
            cur = v;
            v = 0;
            const uint32_t total = a.total[c], n64 = (total + 1) / 2;
            for (uint32_t b = 0; b < n64; b += 17) {
                const uint32_t e = 2 * (b + idx);
                if (idx < 17u && e < total) {
                    const uint32_t lo = row[class_word_pos(a, c, e)];
                    const uint32_t hw = e + 1 < total ? row[class_word_pos(a, c, e + 1)] : 0u;
                    hi = max(hi, max(lo, hw));
                    v = (uint64_t)lo | ((uint64_t)hw << 32);
                }
                v = kk::f_coop(v);
            }
            if (l > 0) {  // compress(cur, row digest)
                const uint64_t rd = shfl64(v, idx & 3u);
                v = kk::f_coop(idx < 4u ? cur : idx < 8u ? rd : 0ull);
            }
            c++;
        }
        if (l == a.depth) break;
        const uint64_t sw = path[l * 4 + (idx & 3u)];
        const bool right = (index >> l) & 1u;
        const uint64_t cv = shfl64(v, idx & 3u);
        v = kk::f_coop(idx < 8u ? ((idx < 4u) != right ? cv : sw) : 0ull);
    }
    const uint64_t want = (uint64_t)a.root[2 * (idx & 3u)] | ((uint64_t)a.root[2 * (idx & 3u) + 1] << 32);
    const bool mismatch = __builtin_amdgcn_ballot_w64(idx < 4u && v != want) != 0;
    const bool noncanon = __builtin_amdgcn_ballot_w64(hi >= bb::P) != 0;
    const uint32_t st = verdict((index >> a.depth) != 0u, noncanon, mismatch);
    const bool writer = (threadIdx.x & 63u) == 0u;
    if (writer) status[i] = st;
    count_rejected(writer && st != 0u, d_rejected);
}

int mmcs_verify_many(hipStream_t stream, int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats,
                     const uint32_t* d_indices, size_t n, const uint32_t* d_rows, const uint32_t* d_paths, uint32_t* d_status,
                     uint32_t* d_rejected, int form, int profile) {
    std::string why;
    uint32_t log_max = 0;
    size_t row_words = 0;
    if (check_dims(hash, heights, widths, n_mats, &log_max, &row_words, &why)) return fail(ERR_BAD_ARG, why);
    if (!root) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: null root");
    if (form != MMCS_FORM_AUTO && form != MMCS_FORM_LANE && form != MMCS_FORM_COOP) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: unknown form");
    if (n > 0xffffffffull) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: more than 2^32 - 1 openings");
    if (log_max > 31) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: indices are 32-bit words: heights up to 2^31");
    if (n && (!d_indices || !d_status || (row_words && !d_rows) || (log_max && !d_paths))) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: null argument");
    if ((reinterpret_cast<uintptr_t>(d_paths) & 15u)) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: d_paths must be 16-byte aligned");
    if (d_rejected) P3_HIP(hipMemsetAsync(d_rejected, 0, 4, stream));
    if (!n) return OK;
    VerifySched a{};
    memcpy(a.root, root, 32);
    a.depth = log_max;
    a.row_words = (uint32_t)row_words;
    uint32_t nseg = 0;
    for (uint32_t level = 0; level <= log_max; level++) {
        const uint64_t h = 1ull << (log_max - level);
        size_t off = 0;
        bool any = false;
        for (size_t m = 0; m < n_mats; off += widths[m], m++) {
            if (heights[m] != h) continue;
            if (!any) { a.level[a.n_classes] = level; a.seg_begin[a.n_classes] = nseg; any = true; }
            a.seg_off[nseg] = (uint32_t)off; a.seg_w[nseg] = (uint32_t)widths[m]; nseg++;
            a.total[a.n_classes] += (uint32_t)widths[m];
        }
        if (any) a.n_classes++;
    }
    a.seg_begin[a.n_classes] = nseg;
    // Crossover between the forms (mmcs.h).  Under the THROUGHPUT profile the chip is shared and lane-instructions are what is
    // short: the cooperative forms cost ~2.5x (Poseidon2) / ~13x (Keccak) the lane-instructions, so they take a quarter of the range.
    const size_t coop_max = mmcs_verify_coop_max(hash, profile);
    const bool coop = form == MMCS_FORM_COOP || (form == MMCS_FORM_AUTO && n <= coop_max);
    if (coop && hash == HASH_KECCAK) {
        if (n > (1u << 24)) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: the cooperative form takes at most 2^24 openings");
        hipLaunchKernelGGL(verify_coop_keccak_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, stream, a, d_indices, (uint32_t)n, d_rows, d_paths,
                           d_status, d_rejected);
    } else if (coop) {
        if (n > (1u << 24)) return fail(ERR_BAD_ARG, "mmcs_verify_batch_many: the cooperative form takes at most 2^24 openings");
        hipLaunchKernelGGL(verify_coop_p2_kernel, dim3((uint32_t)((n + 15) / 16)), dim3(256), 0, stream, a, d_indices, (uint32_t)n, d_rows, d_paths,
                           d_status, d_rejected);
    } else if (hash == HASH_KECCAK) {
        hipLaunchKernelGGL(verify_lane_keccak_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, a, d_indices, (uint64_t)n, d_rows,
                           d_paths, d_status, d_rejected);
    } else {
        hipLaunchKernelGGL(verify_lane_p2_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, a, d_indices, (uint64_t)n, d_rows, d_paths,
                           d_status, d_rejected);
    }
    P3_HIP(hipGetLastError());
    return OK;
}

}  // namespace p3
