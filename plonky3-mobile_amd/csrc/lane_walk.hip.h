// The per-lane Merkle opening walk of every device verifier: one lane hashes a leaf row and compresses up a path to the root, for both
// hash configurations.  mmcs_verify.hip (verify_lane_*_kernel) and pcs_verifier_dev.hip (pv_open_kernel, which the fib_air and the AIR
// batch verifiers run through their owned PCS verifier) supply where the words come from and decide what a mismatch means; the absorb, the reduce after each permutation,
// the last-block digest form, the left / right select and the canonicity fold into `hi` are here and nowhere else.
//
//   SRC   the word source.  len(l): the words of the row hashed at level l (level 0 = the leaf row); word(l, e): word e of that row,
//         asked for once each with e = 0, 1 .. len - 1 (so a source may be a cursor); has(l): whether a row is hashed at level l,
//         has(0) is true.  len(l) is called once, before the words of level l and after has(l).
//   SIB   sib(l, sw): the 8 words of the sibling digest at level l.
//   INJECT  whether a level above the leaves may have a row (mixed heights as MerkleTree::new injects them: after the compression
//         that reaches level l the row of that level is hashed and compressed in as the right operand, then the sibling follows).
// Two compile-time forms, because they cost different registers:
//   INJECT = false  the leaf, then `depth` compressions.  has() is never called.
//   INJECT = true   one sponge site, then up to two compressions per level through ONE compression site (the loop over `sub` is kept
//                   rolled): with a second sponge or compression site inside the level loop this compiler keeps the Keccak state in
//                   scratch.  A kernel that never injects must not take this form: the schedule costs it registers (pv_open_kernel's
//                   Keccak form takes 104 VGPRs without it and 116 with it).
// Every word absorbed, and under Poseidon2 every sibling word, is folded into `hi` (the largest seen: >= P means not canonical, which
// the caller reports whatever the hashes give; Keccak digest words are raw u64 halves, any value is hashed).  The walk returns whether
// the digest it arrives at differs from `root`.
#pragma once
#include <stdint.h>

#include "keccak.hip.h"
#include "mmcs.h"
#include "poseidon2_f64.hip.h"

namespace p3 {
namespace lane_walk {

// sibling loader over a path read word by word (4-byte aligned: a path inside proof bytes)
struct PathWords {
    const uint32_t* path;
    __device__ __forceinline__ void operator()(uint32_t l, uint32_t (&sw)[8]) const {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = path[8 * l + k];
    }
};

// ---- Poseidon2 in exact-integer fp64 (poseidon2_f64.hip.h) ----
// PaddingFreeSponge<Poseidon2-16, 16, 8, 8> over word(0) .. word(len - 1), digest left in s[0..8)
template <typename F>
__device__ __forceinline__ void p2_sponge(double (&s)[16], uint32_t len, uint32_t& hi, F word) {
#pragma unroll
    for (int k = 0; k < 16; k++) s[k] = 0.0;
    for (uint32_t k = 0; k < len; k += 8) {
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (k + e < len) {
                const uint32_t v = word(k + e);
                hi = max(hi, v);
                s[e] = p2f::load_elem(v);
            }
        p2f::permute(s);
#pragma unroll
        for (int e = 0; e < 16; e++) s[e] = p2f::reduce(s[e]);  // the next permutation assumes |s| <= 2^33
    }
}
// the operands of TruncatedPermutation<_, 2, 8, 16> at level l: cur and the sibling, placed by the index bit
template <typename SIB>
__device__ __forceinline__ void p2_sibling_operands(double (&s)[16], const double (&cur)[8], uint32_t l, uint32_t index, SIB sib, uint32_t& hi) {
    uint32_t sw[8];
    sib(l, sw);
    const bool right = (index >> l) & 1u;  // this opening's node is the right child: the sibling goes left
#pragma unroll
    for (int k = 0; k < 8; k++) {
        hi = max(hi, sw[k]);
        const double sd = p2f::load_elem(sw[k]);
        s[k] = right ? sd : cur[k];
        s[8 + k] = right ? cur[k] : sd;
    }
}
__device__ __forceinline__ void p2_compress(double (&s)[16], double (&cur)[8]) {
    p2f::permute(s);
#pragma unroll
    for (int k = 0; k < 8; k++) cur[k] = p2f::reduce(s[k]);
}

template <bool INJECT, typename SRC, typename SIB>
__device__ __forceinline__ bool p2_walk(SRC& src, SIB sib, uint32_t depth, uint32_t index, const uint32_t* root, uint32_t& hi) {
    const p2f::MagicRegs smk = p2f::magic_regs();
    double s[16], cur[8];
    if constexpr (!INJECT) {
        p2_sponge(s, src.len(0), hi, [&](uint32_t e) { return src.word(0, e); });
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = s[k];
        for (uint32_t l = 0; l < depth; l++) {
            p2_sibling_operands(s, cur, l, index, sib, hi);
            p2_compress(s, cur);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = 0.0;
        for (uint32_t l = 0; l <= depth; l++) {
            const bool has = src.has(l);
            if (has) p2_sponge(s, src.len(l), hi, [&](uint32_t e) { return src.word(l, e); });
            // up to two compressions through ONE call site: the injected row digest (right operand, never swapped), then the sibling
            _Pragma("clang loop unroll(disable)")
            for (uint32_t sub = 0; sub < 2; sub++) {
                if (sub == 0) {
                    if (l == 0) {
#pragma unroll
                        for (int k = 0; k < 8; k++) cur[k] = s[k];
                    }
                    if (!has || l == 0) continue;
#pragma unroll
                    for (int k = 0; k < 8; k++) { s[8 + k] = s[k]; s[k] = cur[k]; }
                } else {
                    if (l == depth) continue;
                    p2_sibling_operands(s, cur, l, index, sib, hi);
                }
                p2_compress(s, cur);
            }
        }
    }
    bool mismatch = false;
#pragma unroll
    for (int k = 0; k < 8; k++) mismatch |= p2f::store_elem(cur[k], smk) != root[k];
    return mismatch;
}

// ---- Keccak ----
// SerializingHasher + PaddingFreeSponge<KeccakF, 25, 17, 4> over word(0) .. word(len - 1), digest left in st[0..4)
template <typename F>
__device__ __forceinline__ void kk_sponge(uint64_t (&st)[25], uint32_t len, uint32_t& hi, F word) {
#pragma unroll
    for (int k = 0; k < 25; k++) st[k] = 0;
    const uint32_t n64 = (len + 1) / 2;
    for (uint32_t b = 0; b < n64; b += 17) {
#pragma unroll
        for (int k = 0; k < 17; k++) {
            const uint32_t e = 2 * (b + k);
            if (e < len) {
                const uint32_t lo = word(e);
                const uint32_t hw = e + 1 < len ? word(e + 1) : 0u;
                hi = max(hi, max(lo, hw));
                st[k] = (uint64_t)lo | ((uint64_t)hw << 32);
            }
        }
        if (b + 17 >= n64) kk::permute_digest(st);  // the last block: only the digest words are read
        else kk::permute(st);
    }
}
template <typename SIB>
__device__ __forceinline__ void kk_load_sibling(uint64_t (&r4)[4], uint32_t l, SIB sib) {
    uint32_t sw[8];
    sib(l, sw);
#pragma unroll
    for (int k = 0; k < 4; k++) r4[k] = (uint64_t)sw[2 * k] | ((uint64_t)sw[2 * k + 1] << 32);
}
// CompressionFunctionFromHasher<U64Hash, 2, 4>: one block of the two digests, r4 on the left when `right`
__device__ __forceinline__ void kk_compress(uint64_t (&st)[25], uint64_t (&cur)[4], const uint64_t (&r4)[4], bool right) {
#pragma unroll
    for (int k = 0; k < 4; k++) { st[k] = right ? r4[k] : cur[k]; st[4 + k] = right ? cur[k] : r4[k]; }
#pragma unroll
    for (int k = 8; k < 25; k++) st[k] = 0;
    kk::permute_digest(st);
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = st[k];
}

template <bool INJECT, typename SRC, typename SIB>
__device__ __forceinline__ bool kk_walk(SRC& src, SIB sib, uint32_t depth, uint32_t index, const uint32_t* root, uint32_t& hi) {
    uint64_t st[25], cur[4] = {0, 0, 0, 0};
    if constexpr (!INJECT) {
        kk_sponge(st, src.len(0), hi, [&](uint32_t e) { return src.word(0, e); });
#pragma unroll
        for (int k = 0; k < 4; k++) cur[k] = st[k];
        for (uint32_t l = 0; l < depth; l++) {
            uint64_t r4[4];
            kk_load_sibling(r4, l, sib);
            kk_compress(st, cur, r4, (index >> l) & 1u);
        }
    } else {
        for (uint32_t l = 0; l <= depth; l++) {
            const bool has = src.has(l);
            if (has) kk_sponge(st, src.len(l), hi, [&](uint32_t e) { return src.word(l, e); });
            // as p2_walk: the injected row digest, then the sibling, through ONE compression site
            _Pragma("clang loop unroll(disable)")
            for (uint32_t sub = 0; sub < 2; sub++) {
                uint64_t r4[4];
                bool right = false;
                if (sub == 0) {
                    if (l == 0) {
#pragma unroll
                        for (int k = 0; k < 4; k++) cur[k] = st[k];
                    }
                    if (!has || l == 0) continue;
#pragma unroll
                    for (int k = 0; k < 4; k++) r4[k] = st[k];
                } else {
                    if (l == depth) continue;
                    kk_load_sibling(r4, l, sib);
                    right = (index >> l) & 1u;
                }
                kk_compress(st, cur, r4, right);
            }
        }
    }
    bool mismatch = false;
#pragma unroll
    for (int k = 0; k < 4; k++) mismatch |= cur[k] != ((uint64_t)root[2 * k] | ((uint64_t)root[2 * k + 1] << 32));
    return mismatch;
}

template <int HASH, bool INJECT, typename SRC, typename SIB>
__device__ __forceinline__ bool walk(SRC& src, SIB sib, uint32_t depth, uint32_t index, const uint32_t* root, uint32_t& hi) {
    if constexpr (HASH == HASH_KECCAK) return kk_walk<INJECT>(src, sib, depth, index, root, hi);
    else return p2_walk<INJECT>(src, sib, depth, index, root, hi);
}

}  // namespace lane_walk

// rejected openings / proofs counted per wave: a ballot popcount and one vector atomic from the wave's first lane (lane 0 is active
// whenever a lane of the wave is: lanes past n are the highest ones)
__device__ __forceinline__ void count_rejected(bool rejected, uint32_t* d_rejected) {
    const uint64_t b = __builtin_amdgcn_ballot_w64(rejected);
    if (d_rejected && b && (threadIdx.x & 63u) == 0u) atomicAdd(d_rejected, (uint32_t)__builtin_popcountll(b));
}

}  // namespace p3
