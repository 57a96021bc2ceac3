// Merkle-tree prover data kept in HBM (Plonky3 MerkleTree<..>: leaves + digest_layers).
#pragma once
#include <memory>
#include <cstring>
#include "../../include/p3hip.h"  // p3hip_mmcs_kernel, p3hip_mmcs_step: the plan is exported as it is
#include "common.h"

namespace p3 {

enum HashKind : int { HASH_POSEIDON2 = 0, HASH_KECCAK = 1 };

struct Tree {
    int kind = HASH_POSEIDON2;
    std::vector<const uint32_t*> mats;  // borrowed device pointers (or entries of `owned`)
    std::vector<size_t> heights, widths, strides;  // strides: words between rows (= widths for dense matrices)
    std::vector<void*> owned;           // device copies made by the host-pointer commit
    uint32_t* layers = nullptr;         // all digest layers, leaf layer first, 8 words per digest
    bool root_copied = false;           // the top kernel also wrote the root to the caller's host-mapped buffer
    bool owns_layers = true;            // false: caller-provided arena (prover), nothing to free
    std::vector<size_t> layer_off, layer_len;  // offsets in words / lengths in digests
    uint32_t log_max_height = 0;
    uint32_t* staging = nullptr;        // open_batch gather buffer
    size_t staging_words = 0;
    ~Tree();
};

// ext_layers: optional caller-owned storage of (2*max_height - 1) * 8 words for the digest layers.
// strides: optional words between two rows per matrix (a matrix may be a column group of a wider one); default = widths.
// profile (common.h): how layers of 2^10 .. 2^15 digests are hashed — the latency forms (a lone tree / proof) or the per-lane
// forms (several provers sharing the chip).  Digests are the same either way.
int mmcs_commit(hipStream_t stream, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths,
                size_t n_mats, Tree** out, uint32_t* ext_layers = nullptr, uint32_t* root_copy = nullptr,
                int kind = HASH_POSEIDON2, const size_t* strides = nullptr, int profile = PROFILE_LATENCY);
// The shape checks of mmcs_commit alone (host only: nothing is launched, allocated or drawn): power-of-two heights, at most 64 matrices,
// at most 16 of one height.  The hiding commit asks before it draws a salt, so that a refused shape leaves its rng where it was.
int mmcs_check_shape(const size_t* heights, const size_t* widths, size_t n_mats);
// The launch list of mmcs_commit for one commitment: step[0] hashes the tallest class into layer 0 (levels = 0), every further step
// is one launch that reads digest layer `layer` and writes the `levels` layers above it.  ALL of the launch policy is here (which
// kernel by hash, profile, class shape, layer length, row stride and address alignment); mmcs_commit only executes the list.
// Pure host code, no allocation: d_mats (or any entry of it), strides and layers may be null (= dense, aligned) and are never
// dereferenced.  The caller has run mmcs_check_shape.
struct MmcsPlan {
    p3hip_mmcs_step step[P3HIP_MMCS_MAX_STEPS];
    uint32_t n = 0;
};
int mmcs_plan(int kind, int profile, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths, const size_t* strides,
              size_t n_mats, const uint32_t* layers, MmcsPlan* plan);
const char* mmcs_kernel_name(int kernel);  // "leaf_coop" .. "keccak_compress"; null for an unknown enumerator
inline size_t mmcs_layer_words(uint64_t max_height) { return (size_t)(2 * max_height - 1) * 8; }
int mmcs_root(hipStream_t stream, const Tree& t, uint32_t root_out[8]);
int mmcs_open(hipStream_t stream, const Tree& t, uint64_t index, uint32_t* rows_out, uint32_t* path_out);
// Mmcs::open_batch for n indices in one launch, device to device: opening i = rows of every matrix in matrix order (d_rows + i *
// mmcs_row_words) and the sibling path (d_paths + i * log_max_height * 8).  An index is masked into the tree.  Enqueues only.
size_t mmcs_row_words(const Tree& t);
int mmcs_open_many(hipStream_t stream, const Tree& t, const uint32_t* d_indices, size_t n, uint32_t* d_rows, uint32_t* d_paths);

// ---- Mmcs::verify_batch (mmcs_verify.hip) ----
constexpr size_t MMCS_MAX_MATS = 64;
enum MmcsReject : int { MMCS_ROOT_MISMATCH = 1, MMCS_WRONG_HEIGHT = 2, MMCS_NOT_CANONICAL = 3, MMCS_BAD_INDEX = 4 };
// Host, one opening: 0 = accept, an MmcsReject code, or ERR_BAD_ARG for a malformed call; the reason in *why (never the mailbox).
// check_canonical = false hashes the words as they are (the proof verifiers: their reader has already flagged a word >= P, and
// their own reject codes decide).  rows: the opened rows in matrix order (a hiding tree's salts listed as width-4 matrices, m0 s0 m1 s1 ...); path: path_len x 8.
int mmcs_verify_batch(int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats, size_t index,
                      const uint32_t* rows, const uint32_t* path, size_t path_len, std::string* why, bool check_canonical = true);
// Device, n openings of one commitment in the layout of mmcs_open_many; d_status[i] = 0 or an MmcsReject code, *d_rejected (may be
// null) = how many are nonzero.  Enqueues only.  form: which kernel (AUTO: by n, the crossover constants below and the profile).
enum MmcsVerifyForm : int { MMCS_FORM_AUTO = 0, MMCS_FORM_LANE = 1, MMCS_FORM_COOP = 2 };
// The largest n that MMCS_FORM_AUTO sends to the cooperative form under the LATENCY profile (a quarter of it under THROUGHPUT).
// 0 = never: the cooperative kernels have not yet been timed against the per-lane ones in a same-run A/B (tools/mmcs_verify_bench.py
// latency prints the table that fixes these), and this project does not enable a form on an estimate.  Until then they are reachable
// through the explicit form argument only (MMCS_FORM_COOP: the tests and the bench tool).
constexpr size_t MMCS_VERIFY_COOP_MAX_P2 = 0, MMCS_VERIFY_COOP_MAX_KECCAK = 0;
inline size_t mmcs_verify_coop_max(int hash, int profile) {
    return (hash == HASH_KECCAK ? MMCS_VERIFY_COOP_MAX_KECCAK : MMCS_VERIFY_COOP_MAX_P2) / (profile == PROFILE_LATENCY ? 1 : 4);
}
int mmcs_verify_many(hipStream_t stream, int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats,
                     const uint32_t* d_indices, size_t n, const uint32_t* d_rows, const uint32_t* d_paths, uint32_t* d_status,
                     uint32_t* d_rejected, int form, int profile);
int poseidon2_permute_states(hipStream_t stream, uint32_t* d_states, uint64_t n);
int poseidon2_f64_probe(hipStream_t stream, const double* d_in, uint32_t* d_out, uint64_t n, int mode);
int poseidon2_permute_states_variant(hipStream_t stream, uint32_t* d_states, uint64_t n, int variant);
int keccak_f_states(hipStream_t stream, uint64_t* d_states, uint64_t n);
int keccak_f_states_variant(hipStream_t stream, uint64_t* d_states, uint64_t n, int variant);
// one compression layer through the production kernel of a named form (test entry, mmcs.hip)
int compress_layer_variant_check(int kind, int variant, const uint32_t* d_in, const uint32_t* d_out, uint64_t n_out);  // arguments only: no GPU call
int compress_layer_variant(hipStream_t stream, int kind, int variant, const uint32_t* d_in, uint32_t* d_out, uint64_t n_out);

}  // namespace p3
