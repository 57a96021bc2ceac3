// fib_air prover object: one instance owns its HBM arena and stream, reusable across proofs.
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "common.h"

namespace p3 {

struct Tree;        // mmcs.h
struct Challenger;  // challenger.h

// p3_fri::FriParameters (the mmcs field is implied: ExtensionMmcs over the Poseidon2 tree)
struct FriParams {
    uint32_t log_blowup, log_final_poly_len, num_queries, proof_of_work_bits;
};

// Largest LDE domain (log2 of its points) a prover object admits: BASELINE configs[2] (2^24 rows at blowup 4) — the largest
// size any test or bench has run; the field's two-adicity (27) would admit twice that, which nothing has ever exercised.
constexpr uint32_t MAX_LOG_DOMAIN = 26;
// the hiding prover's (log_n + 1 + log_blowup): 2^22 trace rows at blowup 2, exercised by tests/test_gpu_hiding.py
constexpr uint32_t MAX_LOG_DOMAIN_HIDING = 24;

struct StageTimes {  // host wall clock per stage, accumulated over `proofs`
    double trace_commit_ms = 0, quotient_commit_ms = 0, open_ms = 0, fri_commit_ms = 0, grind_ms = 0, query_ms = 0;
    uint64_t proofs = 0;
};

class FibProver {
  public:
    FibProver();
    ~FibProver();
    FibProver(const FibProver&) = delete;
    // hash: mmcs.h HashKind; profile: common.h Profile (a lone prover: latency; provers sharing the chip: throughput)
    int init(uint32_t log_n, const FriParams& fp, hipStream_t stream, bool own_stream, int hash = 0, int profile = PROFILE_LATENCY);
    // proves the FibonacciAir instance with first row (a, b); public values [a, b, last right value]
    int prove(uint64_t a, uint64_t b, std::vector<uint8_t>* proof);
    // the same in two halves: enqueue returns once the proof's launches are queued (at most two proofs in flight, the second
    // behind the first on the prover's stream); finish waits for the oldest one and serialises it
    int enqueue(uint64_t a, uint64_t b);
    int finish(std::vector<uint8_t>* proof);
    // the same for a CALLER's trace: d_trace = 2^log_n rows x 2 Montgomery words in device memory of the prover's device, read in
    // place (no copy, no generation) and left unchanged by the caller until the proof is returned; pis = the public values
    // (Montgomery words) the transcript observes and the quotient uses, whether or not the trace satisfies them
    int prove_trace(const uint32_t* d_trace, const uint32_t pis[3], std::vector<uint8_t>* proof);
    int enqueue_trace(const uint32_t* d_trace, const uint32_t pis[3]);
    uint32_t* arena_trace() const;  // the arena's trace slot (2^log_n x 2 words): what a host trace is uploaded into
    bool has_pending() const;       // proofs enqueued and not finished
    hipStream_t stream() const;
    uint32_t log_n() const;
    int device() const;
    const StageTimes& times() const;
    void reset_times();
    // proofs so far whose first proof-of-work range held no witness; last_indices = the device's query-index buffer right
    // after the last such miss, before the search was continued (all zero by construction, tests/test_gpu_prover.py)
    uint64_t grind_misses(std::vector<uint32_t>* last_indices) const;

  private:
    struct Impl;
    Impl* im;
    int run(uint64_t a, uint64_t b, int slot, int phase, std::vector<uint8_t>* proof, void* pending_rec);
    int enqueue_any(uint64_t a, uint64_t b, const uint32_t* d_trace, const uint32_t* pis);
};

// The same prover for the HIDING half of the reference's configuration (native/src/fib_air.rs:40-65:
// MerkleTreeHidingMmcs + HidingFriPcs, SmallRng::seed_from_u64(seed)); wire format version 2 (prover_hiding.hip.inc).
class FibHidingProver {
  public:
    FibHidingProver();
    ~FibHidingProver();
    FibHidingProver(const FibHidingProver&) = delete;
    int init(uint32_t log_n, const FriParams& fp, hipStream_t stream, bool own_stream, int hash, uint64_t seed, int profile = PROFILE_LATENCY);
    int prove(uint64_t a, uint64_t b, std::vector<uint8_t>* proof);
    // a caller's trace and public values, as FibProver::prove_trace (the randomization reads the trace in place)
    int prove_trace(const uint32_t* d_trace, const uint32_t pis[3], std::vector<uint8_t>* proof);
    uint32_t* arena_trace() const;
    hipStream_t stream() const;
    uint32_t log_n() const;
    int device() const;

  private:
    struct Impl;
    Impl* im;
    int prove_any(uint64_t a, uint64_t b, const uint32_t* d_trace, const uint32_t* pis, std::vector<uint8_t>* proof);
};

// the first word of every proof's header (fib_air, plain and hiding, and a caller-defined AIR's): "P3FB", little endian
constexpr uint32_t PROOF_MAGIC = 0x42463350u;

// verifier.hip: p3_uni_stark::verify for FibonacciAir on the host (0 = accept, else the failed check's code)
int verify_fib_air(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n,
                   const FriParams& fp, std::string* why, int hash = 0);
// the verifier of hiding proofs (wire format version 2)
int verify_fib_air_hiding(const uint8_t* proof, size_t len, uint64_t a_pub, uint64_t b_pub, uint64_t x_pub, uint32_t log_n,
                          const FriParams& fp, std::string* why, int hash);
// the parameter gates of the two verifiers above (0, or ERR_BAD_ARG with the format's message in *why)
int verify_check_parameters(int hash, bool hiding, uint32_t log_n, const FriParams& fp, std::string* why);


// ---- TwoAdicFriPcs<BabyBear, GpuDft, MerkleTreeMmcs, ExtensionMmcs> over caller-supplied matrices (pcs.hip.inc), non-hiding ----
// Every matrix of one open / verify has the same height h = 2^log_h (what p3_uni_stark produces for any AIR: trace, preprocessed
// trace and quotient chunks); mixed heights are refused by name — unless the object was created for them (Pcs::init's mixed_heights;
// verify: pcs_verify_mixed), see pcs.hip.inc.  Capacities, refused by name when exceeded:
constexpr size_t PCS_MAX_MATS = 8;      // matrices per commitment (QTREE_MAX_MATS)
constexpr size_t PCS_MAX_ROUNDS = 4;    // commitments per open
constexpr size_t PCS_MAX_POINTS = 4;    // distinct opening points per open
constexpr size_t PCS_MAX_COLS = 8192;   // batched columns: sum of width over every (matrix, point) pair; also the widest matrix

// HidingFriPcs (pcs_hiding.hip.inc): a commitment lists every matrix and its salt in one QTree (QTREE_MAX_MATS entries)
constexpr size_t PCS_HIDING_MAX_MATS = 4;
constexpr uint32_t PCS_SALT = 4;               // MerkleTreeHidingMmcs SALT_ELEMS
constexpr uint32_t PCS_MAX_RANDOM_CODEWORDS = 8;
constexpr size_t PCS_MAX_QUOTIENT_WIDTH = 2048;

// prover data of one commitment: the bit-reversed LDEs (owned, in HBM) and their tree.  Of a hiding commitment: log_h is the
// COMMITTED log height (the caller's + 1), widths the committed widths (the caller's + the random columns), salts[m] the
// 2^log_big x PCS_SALT salt matrix of matrix m (pieces of salt_base)
struct PcsData {
    std::vector<uint32_t*> lde;
    std::vector<size_t> widths;
    uint32_t log_h = 0, log_big = 0;
    std::vector<uint32_t> log_hs;  // per matrix, of a commitment of mixed heights (log_h is then the tallest); empty: all log_h
    uint32_t mat_log_h(size_t m) const { return log_hs.empty() ? log_h : log_hs[m]; }
    int hash = 0, device = -1;
    Tree* tree = nullptr;
    bool hiding = false;
    uint32_t nrc = 0;
    uint32_t* salt_base = nullptr;
    std::vector<uint32_t*> salts;
    PcsData() = default;
    PcsData(const PcsData&) = delete;
    ~PcsData();
};

class Pcs {
  public:
    Pcs();
    ~Pcs();
    Pcs(const Pcs&) = delete;
    // mixed_heights: commit and open take matrices of any power-of-two heights >= 2 (one class per height: pcs.hip.inc); false: they
    // refuse them by name, as every object did before the option existed
    int init(const FriParams& fp, hipStream_t stream, bool own_stream, int hash, int profile, bool mixed_heights = false);
    // HidingFriPcs::new(dft, mmcs, fri_params, num_random_codewords, SmallRng::seed_from_u64(pcs_seed)) over a MerkleTreeHidingMmcs
    // seeded with mmcs_seed (the FRI MMCS a clone of it): the object owns the three streams, which advance over its lifetime
    int init_hiding(const FriParams& fp, hipStream_t stream, bool own_stream, int hash, int profile, uint32_t num_random_codewords,
                    uint64_t mmcs_seed, uint64_t pcs_seed);
    bool hiding() const;
    // Pcs::commit: d_evals[m] = heights[m] x widths[m] evaluations over shifts[m] * <g_h> in natural row order (device memory; shifts
    // null: all 1); one synchronisation (the root)
    int commit(const uint32_t* const* d_evals, const size_t* heights, const size_t* widths, const uint32_t* shifts, size_t n_mats,
               uint32_t root_out[8], PcsData** out);
    // hiding objects only.  HidingFriPcs::commit_quotient: n_chunks matrices of h x width, chunk c the evaluations (natural order)
    // on GENERATOR g_(n_chunks h)^c <g_h>; get_opt_randomization_poly_commitment for matrices of 2^log_h rows
    int commit_quotient(const uint32_t* const* d_chunks, size_t h, size_t width, size_t n_chunks, uint32_t root_out[8], PcsData** out);
    int commit_randomization(uint32_t log_h, uint32_t root_out[8], PcsData** out);
    // Pcs::open: points_per_mat per matrix in round -> matrix order, points 4 words each in round -> matrix -> point order; chal: the
    // transcript before the open, on return the transcript after the last query index; opened: extension elements in observation
    // order; proof: the FriProof section of the wire format.  One synchronisation.
    int open(const PcsData* const* rounds, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, Challenger* chal,
             std::vector<uint32_t>* opened, std::vector<uint8_t>* proof);
    hipStream_t stream() const;

  private:
    struct Impl;
    Impl* im;
    int commit_hiding(const uint32_t* const* d_evals, const size_t* heights, const size_t* widths, const uint32_t* shifts, size_t n_mats,
                      uint32_t root_out[8], PcsData** out);
    int hiding_finish(PcsData* data, uint32_t root_out[8]);
};

// p3_uni_stark::prove for a caller-defined AIR (air.h) over the non-hiding PCS, device-resident (air_prover.hip.inc; include/p3hip.h
// p3hip_air_prover_*): one object owns the arena of one (AIR, log_n, FRI parameters, hash, profile); a proof is one launch chain on
// the object's stream with the transcript on the device, one copy-back and one synchronisation.  The bytes are prove_air's.
struct Air;
class AirProver {
  public:
    AirProver();
    ~AirProver();
    AirProver(const AirProver&) = delete;
    // copies the program; every gate is refused by name before anything is allocated
    int init(const Air& air, int profile, int hash, uint32_t log_n, const FriParams& fp, hipStream_t stream, bool own_stream);
    // d_trace: 2^log_n x width Montgomery words in device memory, read in place; pis: n_public host words, each < P.  One proof in
    // flight: enqueue returns once the launches and the copy-back are queued, finish synchronises and serialises
    int enqueue(const uint32_t* d_trace, const uint32_t* pis);
    int finish(std::vector<uint8_t>* proof);
    // check_constraints on the prover's stream (synchronises): *row < 0 when every constraint holds on every row
    int check_trace(const uint32_t* d_trace, const uint32_t* pis, long long* row, int* constraint);
    uint32_t* arena_trace();  // 2^log_n x width words: what a host trace is uploaded into (allocated by the first call)
    bool pending() const;
    hipStream_t stream() const;
    uint32_t log_n() const;
    uint32_t width() const;
    uint32_t n_public() const;
    int device() const;

  private:
    struct Impl;
    Impl* im;
};

bool pcs_point_on_lde_coset(const uint32_t z[4], uint32_t log_big);
// A challenger as the words a device transcript imports and exports (transcript.hip.h DevState up to `pis`): the duplex state,
// buffers and counters, then the Keccak streaming sponge.  import refuses counters no challenger can hold (pending inputs >= 8,
// outputs > 8; pending block >= 136 bytes, output bytes > 32) and leaves *c as it was.
constexpr uint32_t CHALLENGER_STATE_WORDS = 128;
void challenger_export(const Challenger& c, uint32_t* words);
int challenger_import(const uint32_t* words, Challenger* c);
// verifier.hip: Pcs::verify on the host.  0 = accept; ERR_BAD_ARG for a refused argument; a positive code names the failed check
// (the numbering of verify_fib_air's FRI half: 5 commit phase length, 6 query count, 7 final polynomial length, 8 trailing or missing
// bytes, 9 truncated, 11 InvalidPowWitness, 12 query shape, 13 input opening, 14 FRI layer opening, 15 FinalPolyMismatch)
int pcs_verify(int hash, const FriParams& fp, uint32_t log_h, const uint32_t* roots, const size_t* mats_per_round, const size_t* widths,
               size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened, const uint8_t* proof,
               size_t len, Challenger* chal, std::string* why);
// the same for matrices of mixed heights: log_heights one per matrix, round -> matrix, in place of log_h.  With all heights equal it
// returns what pcs_verify returns for the same bytes (the same code; of several refused arguments it may name another one).  The same holds
// for all three between builds: the shape's gates (pcs_layout.h) run before the checks of the points' values, so of a refused point and a
// refused shape the shape is named, wherever the point stands.
int pcs_verify_mixed(int hash, const FriParams& fp, const unsigned* log_heights, const uint32_t* roots, const size_t* mats_per_round,
                     const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened,
                     const uint8_t* proof, size_t len, Challenger* chal, std::string* why);
// HidingFriPcs::verify: log_h the CALLER's log height (the committed polynomials have degree < 2^(log_h + 1)), widths the committed
// widths, every input opening and FRI layer opening with a salt of PCS_SALT words; at most PCS_HIDING_MAX_MATS matrices a round
int pcs_verify_hiding(int hash, const FriParams& fp, uint32_t log_h, const uint32_t* roots, const size_t* mats_per_round,
                      const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened,
                      const uint8_t* proof, size_t len, Challenger* chal, std::string* why);

}  // namespace p3
