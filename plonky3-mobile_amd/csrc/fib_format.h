// The two wire formats of a fib_air proof as ONE table, read by the host verifier (verifier.hip verify_fib) and by the device batch
// verifier (verifier_dev.hip): a fib_air proof is a PCS proof of a fixed shape behind a header -- magic, version, log_n, the roots, the
// opened values.  What the formats do not share is here; pcs_layout (pcs_layout.h) lays out the FRI section behind the header.
#pragma once
#include <cstdint>

#include "pcs_layout.h"
#include "prover.h"

namespace p3 {

// What the three callers of the host's pcs_walk answer differently for the same bytes.  Nobody chose these differences; the recordings
// under tests/golden pin them (fib_verify_codes.json, verifier_noncanonical_codes.json, pcs_verify_codes.json), so they are kept, in one place.
struct Dialect {
    const char* round_name[PCS_MAX_ROUNDS];  // the message that names an input round, in proof order
    uint32_t named;                          // bit c: code c (of 9, 12, 13 at an input opening) carries round_name, not the general message
    bool stop_on_flag;  // a reader flagged (truncated, or a word >= P) right after an input opening rejects with 9 before the path is hashed
    enum { LAYOUT_CHECKED, LAYOUT, COUNTS } final_at;  // the final polynomial lies where the layout says, a shorter proof being a 9
                                                       // (CHECKED) or final_poly's own 7; or where skip_queries_by_counts ends
};
constexpr Dialect DIALECT_FIB1{{"trace opening", "quotient opening"}, 1u << 13, false, Dialect::COUNTS};
constexpr Dialect DIALECT_FIB2{{"randomization opening", "trace opening", "quotient opening"}, 1u << 9 | 1u << 12 | 1u << 13, true, Dialect::LAYOUT};

constexpr uint32_t FIB_MAX_ROUNDS = 3, FIB_MAX_MATS = 6, FIB_MAX_OPENED = 36, FIB_MAX_CHUNKS = 4, FIB_MAX_GROUPS = 8;
struct FibFormat {
    uint32_t version;
    bool hiding;        // the salted MMCS, the trace committed at twice its height: the transcript opens with log_n + 1, then log_n
    uint32_t n_rounds;  // the header's roots: trace, quotient[, randomization], observed in that order: the first, the public values,
                        // alpha, then the others, zeta
    // the commitment rounds in PROOF order as a PcsShape: each round's root among the header's, its matrices, their widths, each
    // matrix's points and each (matrix, point) pair's slot (0: zeta, 1: zeta g)
    uint32_t root_of[FIB_MAX_ROUNDS];
    size_t mats[FIB_MAX_ROUNDS], widths[FIB_MAX_MATS], points[FIB_MAX_MATS];
    uint32_t slots[FIB_MAX_MATS + 1];
    // the header's opened values, in the proof's (and the transcript's) order: n > 0 is the count word n and n extension elements behind
    // it, n < 0 the bare count word -n; 0 ends
    int grammar[FIB_MAX_GROUPS + 1];
    uint32_t t_loc, t_nxt, chunks, log_chunks;  // among the opened values: the trace at zeta and at zeta g, the 2^log_chunks quotient chunks
    Dialect dialect;
};
// format 1: trace (2 columns) at zeta and zeta g, the quotient (one chunk, 4 columns: an extension element's coordinates) at zeta
constexpr FibFormat FIB_PLAIN{1, false, 2, {0, 1}, {1, 1}, {2, 4}, {2, 1}, {0, 1, 0}, {2, 2, -1, 4}, 0, 2, 4, 0, DIALECT_FIB1};
// format 2, 4 random codewords: the randomization round (4 + 4 columns) first, the trace with its 4 random columns, 4 blinded chunks
constexpr FibFormat FIB_HIDING{2, true, 3, {2, 0, 1}, {1, 1, 4}, {8, 6, 4, 4, 4, 4}, {1, 2, 1, 1, 1, 1}, {0, 0, 1, 0, 0, 0, 0},
                               {8, 6, 6, -4, 4, 4, 4, 4}, 8, 14, 20, 2, DIALECT_FIB2};
constexpr uint32_t opened_of(const FibFormat& f) { uint32_t n = 0; for (int g : f.grammar) if (g > 0) n += (uint32_t)g; return n; }
// the header's length in words: magic, version, log_n; the roots; the grammar's count words and values
constexpr uint32_t head_words_of(const FibFormat& f) {
    uint32_t n = 3 + 8 * f.n_rounds;
    for (int g : f.grammar) n += g > 0 ? 1 + 4 * (uint32_t)g : g < 0 ? 1 : 0;
    return n;
}
static_assert(opened_of(FIB_PLAIN) == 8 && opened_of(FIB_HIDING) == FIB_MAX_OPENED && (1u << FIB_HIDING.log_chunks) <= FIB_MAX_CHUNKS &&
              FIB_MAX_ROUNDS <= PCS_MAX_ROUNDS && head_words_of(FIB_PLAIN) == 55 && head_words_of(FIB_HIDING) == 179,
              "what a grammar reads fits the verifiers' arrays");

// the PCS shape behind the header (the table's arrays are the shape's: f must outlive it)
inline PcsShape fib_pcs_shape(const FibFormat& f, uint32_t log_n) {
    return PcsShape{log_n, f.n_rounds, f.mats, f.widths, f.points, 2, f.slots, nullptr, f.dialect.final_at == Dialect::COUNTS};
}

}  // namespace p3
