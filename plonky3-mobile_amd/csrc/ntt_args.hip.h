// What the transform headers (ntt_fast.hip.h, ntt_narrow.hip.h, ntt_narrow_f64.hip.h) need from their includer: the pass
// arguments of the general plans and the two device helpers every kernel family shares.  Lived at the top of ntt.hip until a
// second translation unit (field_probe.hip) had to include ntt_narrow_f64.hip.h; moved here unchanged.
#pragma once
#include "bb31.hip.h"

namespace p3 {

enum SideKind : uint32_t {
    SIDE_INPLACE = 0,   // word = ((hi << (s0+b)) + (pt << s0)) * W + f          (s0 > 0)
    SIDE_GROUP = 1,     // word = (((h0+t) << b) + pt) * W + c                   (contiguous groups)
    SIDE_GROUP_REV = 2, // word = ((rev(h0+t) << b) + pt) * W + c
    SIDE_STRIDED = 3,   // word = ((rev_b(pt) << (n-b)) + h0 + t) * W + c        (bit-reversal gather/scatter)
};

struct PassArgs {
    const uint32_t* src;
    uint32_t* dst;
    uint64_t src_rows;  // natural rows >= src_rows load as zero (zero padding)
    uint32_t W, wshift; // wshift = log2(W) if W is a power of two, else 0xffffffff
    uint32_t n, b, s0;
    uint32_t dif;       // 0: DIT tile (bit-reversed in, natural out); 1: DIF tile (natural in, bit-reversed out)
    uint32_t load_kind, store_kind;
    uint32_t G;         // groups per tile when W < RUN (group modes)
    uint32_t n_inner;   // inner tile count (column chunks / flattened runs)
    const uint32_t* tile_tw;
    uint32_t has_tw;    // pre (DIT) / post (DIF) twiddle w_{2^(s0+b)}^(rev_b(pt) * lo)
    const uint32_t* tw_lo;
    const uint32_t* tw_hi;
    uint32_t tw_T;
    uint32_t has_sc;    // multiply loaded value by sc(row)
    const uint32_t* sc_lo;
    const uint32_t* sc_hi;
    uint32_t sc_T;
    uint32_t has_us;    // multiply stored value by uscale
    uint32_t uscale;
    uint32_t sc_step;   // fast DIF kernel: shift^(rows between a lane's consecutive loads)
    uint32_t sc_base;   // the scale table's base (shift), host side only
    // fused middle kernel only: forward-direction tables and shift^(16 * 2^s0)
    const uint32_t* tile_tw2;
    const uint32_t* tw2_lo;
    const uint32_t* tw2_hi;
    uint32_t tw2_T;
    uint32_t sc_step16;
};

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, uint32_t bits) {
    return bits ? (__brev(v) >> (32 - bits)) : 0u;
}

__device__ __forceinline__ uint32_t two_level(const uint32_t* lo, const uint32_t* hi, uint32_t T, uint64_t e) {
    uint32_t l = lo[(uint32_t)e & ((1u << T) - 1u)];
    uint32_t h = hi[(uint32_t)(e >> T)];
    return bb::mul(l, h);
}

}  // namespace p3
