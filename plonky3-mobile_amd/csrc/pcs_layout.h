// pcs_layout.hip: the layout of one PCS shape (host only).  A SHAPE fixes where every word of a TwoAdicFriPcs / HidingFriPcs proof is: the
// FRI parameters, the rounds, per matrix its width, height and opening points, the salts.  pcs_layout derives it ONCE, for the host
// verifier (verifier.hip pcs_verify_any) and for the device batch verifier (pcs_verifier_dev.hip, whose kernels take PLayout by value),
// and holds the only copy of the shape gates and their messages.
// Pcs::open is not a caller: its shape comes from PcsData, and its refusals have their own wording ("an open takes at most", "in one
// open", "mixed heights are not supported"), pinned by its tests.
#pragma once
#include <string>

#include "prover.h"

namespace p3 {

constexpr size_t PCS_MAX_SLOTS = 4;  // point slots of a shape: what PCS_MAX_POINTS distinct values are to the host verifier

// What every proof of one configuration shares.  (Not the C ABI's p3hip_pcs_shape_t, which has no log_heights: c_api.hip fills this.)
// widths: the committed widths (random columns included when hiding); slots: one slot < n_slots per pair, round -> matrix -> point.
struct PcsShape {
    uint32_t log_h = 0;  // the caller's height, as for the host verifiers
    size_t n_rounds = 0;
    const size_t* mats_per_round = nullptr;
    const size_t* widths = nullptr;
    const size_t* points_per_mat = nullptr;
    size_t n_slots = 0;
    const uint32_t* slots = nullptr;  // null: the caller has points, not slots (the host verifier), and fills PLayout::pair_slot itself
    const unsigned* log_heights = nullptr;  // mixed heights: one log height per matrix, round -> matrix; log_h is then ignored
    // wire format 1's dialect (verifier.hip Dialect::COUNTS): its host verifier FOLLOWS the queries' count words to the final polynomial,
    // so a mismatch among them is met before the proof of work.  The device verifier follows nothing; the flag only says where in the
    // order such a word reports (PLayout::counts)
    bool counts = false;
};

constexpr uint32_t PV_MAX_IN = (uint32_t)PCS_MAX_ROUNDS, PV_MAX_ALLMATS = (uint32_t)(PCS_MAX_ROUNDS * PCS_MAX_MATS);
constexpr uint32_t PV_MAX_PAIRS = PV_MAX_ALLMATS * (uint32_t)PCS_MAX_POINTS, PV_MAX_FRI = 28;
static_assert(PCS_HIDING_MAX_MATS <= PCS_MAX_MATS && PV_MAX_ALLMATS <= 256 && PCS_MAX_SLOTS <= 256 && PCS_MAX_POINTS <= 256 && PCS_MAX_COLS <= 65535,
              "the per-matrix and per-pair arrays hold either configuration; matrix and slot numbers fit a byte, column offsets 16 bits");

struct PLayout {
    int hash;
    uint32_t salt, log_big, lfinal, n_fri, nq, fpl, pow_bits;
    // words of the proof.  proof_words and the last three hold the low 32 bits: pcs_layout reports the length in 64 bits
    uint32_t proof_words, nq_off, q_base, q_len, fpl_off, fpoly_off, witness_off;
    uint32_t n_in, n_slots, n_pairs, total, wmax, row_words;
    // mixed heights.  mixed: the matrices are not all of one height (which kernels run); class_mask: bit log_big_c of every class with a
    // point; per round its tree's depth and a bit per log_big_m among its matrices
    uint32_t mixed, class_mask, log_big_r[PV_MAX_IN], round_mask[PV_MAX_IN];
    uint32_t counts;  // PcsShape::counts
    // input rounds; offsets are relative to a query's first word
    uint32_t nm[PV_MAX_IN], mat0[PV_MAX_IN], open_off[PV_MAX_IN], depth_off[PV_MAX_IN], leaf_len[PV_MAX_IN];
    // matrices, round -> matrix: width word at val_off - 1, salt length word at salt_off - 1; leaf_start: where the matrix begins in its leaf
    // (mixed: in the row of its class, the matrices of its round and height in input order)
    uint32_t width[PV_MAX_ALLMATS], val_off[PV_MAX_ALLMATS], salt_off[PV_MAX_ALLMATS], leaf_start[PV_MAX_ALLMATS], np[PV_MAX_ALLMATS];
    uint8_t log_big_m[PV_MAX_ALLMATS];
    // (matrix, point) pairs, round -> matrix -> point: where the pair's opened values begin, the first power of alpha it consumes (its
    // class's counter; with one class the same number), its slot, its matrix
    uint16_t pair_off[PV_MAX_PAIRS], pair_aoff[PV_MAX_PAIRS];
    uint8_t pair_slot[PV_MAX_PAIRS], pair_mat[PV_MAX_PAIRS];
    uint32_t nr_off, fri_off[PV_MAX_FRI];
    // constants of the field
    uint32_t gen, gen_inv, neg_half, gens[PV_MAX_FRI], gens_inv[PV_MAX_FRI];
};

// The layout of (hash, hiding, fp, sh), or ERR_BAD_ARG with the refused argument named in *why.  hiding: sh.log_h is the CALLER's log height
// (the committed one is one more), every opening carries salts of PCS_SALT words, a round has at most PCS_HIDING_MAX_MATS matrices.
// sh.log_heights: mixed heights, the round and matrix counts gated first since log_heights is read by them; with all heights equal the
// layout is the one-class layout.  sh.slots null: no gate on n_slots or a slot, pair_slot is left zero.  *proof_words (may be null): the
// length of a proof in words, whether or not it fits PLayout's 32 bits.
int pcs_layout(int hash, bool hiding, const FriParams& fp, const PcsShape& sh, PLayout* out, uint64_t* proof_words, std::string* why);

}  // namespace p3
