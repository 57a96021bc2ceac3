// C++ host-side mirror of the reference's Rust interfaces for the hip backend, header-only over the C ABI
// (include/p3hip.h).  Names, argument meaning and error behaviour follow the reference:
//   BackendKind / set_backend_kind[_from_str] / get_backend_kind / take_last_error   native/src/gpu_dft.rs:14-68
//   GpuDft::{default, with_backend, dft_batch} + Plonky3's provided idft/coset methods     native/src/gpu_dft.rs:70-115
//   RowMajorMatrix (p3_matrix::dense): row-major values + width
//   benchmark_input / percentile_ms / generate_trace_rows                                   native/src/fib_air.rs:77-96,266-284
//   MerkleTreeMmcs (Mmcs::commit / open_batch / verify_batch) and FibAirProver (prove)       native/src/fib_air.rs:40-70
// Rust's `Result<_, String>` becomes p3hip::Error (thrown); there is NO CPU fallback here — the reference's
// GpuDft falls back to Radix2DitParallel on Err (gpu_dft.rs:100-112); a C++ caller catches and decides.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "p3hip.h"

namespace p3hip {

constexpr uint32_t P = 0x78000001u;
constexpr uint32_t MONTY_ONE = 0x0ffffffeu;
constexpr uint32_t GENERATOR_MONTY = (uint32_t)((31ull << 32) % P);  // Val::GENERATOR

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline std::string take_last_error() {  // gpu_dft.rs:65-68
    const char* m = p3hip_take_last_error();
    return m ? std::string(m) : std::string();
}
inline void check(int rc) {
    if (rc != 0) throw Error(rc, take_last_error());
}

enum class BackendKind : int { Cpu = 0, Vulkan = 1, Metal = 2, WebGpu = 3, Hip = 4 };  // gpu_dft.rs:14-40
inline void set_backend_kind_from_str(const std::string& v) {                             // gpu_dft.rs:53-63
    if (p3hip_set_backend(v.c_str()) != 0) throw Error(P3HIP_ERR_BACKEND, take_last_error());
}
inline BackendKind get_backend_kind() { return (BackendKind)p3hip_get_backend(); }       // gpu_dft.rs:49-51
inline std::pair<bool, std::string> is_available() {                                      // lib.rs:167-179
    char buf[256];
    int rc = p3hip_is_available(buf, sizeof buf);
    if (rc != 0) (void)p3hip_take_last_error();
    return {rc == 0, std::string(buf)};
}
inline uint32_t to_monty(uint64_t canon) { return (uint32_t)(((canon % P) << 32) % P); }

struct RowMajorMatrix {  // p3_matrix::dense::RowMajorMatrix<BabyBear>, values are Montgomery words
    std::vector<uint32_t> values;
    size_t width = 0;
    RowMajorMatrix() = default;
    RowMajorMatrix(std::vector<uint32_t> v, size_t w) : values(std::move(v)), width(w) {}
    size_t height() const { return width ? values.size() / width : 0; }
};

class GpuDft {  // gpu_dft.rs:70-115
  public:
    GpuDft() : backend_(get_backend_kind()) {}  // Default (gpu_dft.rs:76-83)
    static GpuDft with_backend(BackendKind b) { GpuDft d; d.backend_ = b; return d; }  // gpu_dft.rs:86-92
    BackendKind backend() const { return backend_; }
    RowMajorMatrix dft_batch(const RowMajorMatrix& m) const {
        require_hip();
        RowMajorMatrix out(std::vector<uint32_t>(m.values.size()), m.width);
        check(p3hip_dft_batch_bb31(m.values.data(), out.values.data(), m.height(), m.width));
        return out;
    }
    RowMajorMatrix idft_batch(const RowMajorMatrix& m) const {
        require_hip();
        RowMajorMatrix out(std::vector<uint32_t>(m.values.size()), m.width);
        check(p3hip_idft_batch_bb31(m.values.data(), out.values.data(), m.height(), m.width));
        return out;
    }
    RowMajorMatrix coset_dft_batch(const RowMajorMatrix& m, uint32_t shift_monty) const {
        require_hip();
        RowMajorMatrix out(std::vector<uint32_t>(m.values.size()), m.width);
        check(p3hip_coset_dft_batch_bb31(m.values.data(), out.values.data(), m.height(), m.width, shift_monty));
        return out;
    }
    RowMajorMatrix coset_lde_batch(const RowMajorMatrix& m, unsigned added_bits, uint32_t shift_monty,
                                   bool bit_reversed_out = false) const {
        require_hip();
        RowMajorMatrix out(std::vector<uint32_t>(m.values.size() << added_bits), m.width);
        check(p3hip_coset_lde_batch_bb31(m.values.data(), out.values.data(), m.height(), m.width, added_bits,
                                         shift_monty, bit_reversed_out ? 1 : 0));
        return out;
    }

  private:
    void require_hip() const {
        if (backend_ != BackendKind::Hip)
            throw Error(P3HIP_ERR_BACKEND, "only the hip backend runs here (the CPU path is the caller's Radix2DitParallel)");
    }
    BackendKind backend_;
};

// fib_air.rs:77-86
inline RowMajorMatrix benchmark_input(size_t height, size_t width) {
    std::vector<uint32_t> v(height * width);
    for (size_t i = 0; i < v.size(); i++) v[i] = to_monty(((uint64_t)i * 17 + 3) % P);
    return RowMajorMatrix(std::move(v), width);
}
// fib_air.rs:88-96 (nearest rank)
inline double percentile_ms(std::vector<double> s, double q) {
    if (s.empty()) return 0.0;
    std::sort(s.begin(), s.end());
    size_t idx = (size_t)std::ceil(q * (double)s.size());
    idx = idx ? idx - 1 : 0;
    return s[std::min(idx, s.size() - 1)];
}

class MerkleTree {  // prover data: device matrices + digest layers owned by the library
  public:
    MerkleTree() = default;
    MerkleTree(const MerkleTree&) = delete;
    MerkleTree(MerkleTree&& o) noexcept : h_(o.h_), widths_(std::move(o.widths_)) { o.h_ = nullptr; }
    ~MerkleTree() { if (h_) p3hip_mmcs_free(h_); }
    size_t log_max_height() const { return p3hip_mmcs_log_max_height(h_); }
    p3hip_tree_t* h_ = nullptr;
    std::vector<size_t> widths_;
};
class MerkleTreeMmcs {  // Mmcs<BabyBear>: Poseidon2 hashes (north_star) or the Keccak ones fib_air.rs:28-51 wires
  public:
    explicit MerkleTreeMmcs(int hash = P3HIP_HASH_POSEIDON2) : hash_(hash) {}
    std::pair<std::vector<uint32_t>, MerkleTree> commit(const std::vector<RowMajorMatrix>& mats) const {
        std::vector<const uint32_t*> ptrs;
        std::vector<size_t> hs, ws;
        for (auto& m : mats) { ptrs.push_back(m.values.data()); hs.push_back(m.height()); ws.push_back(m.width); }
        std::vector<uint32_t> root(8);
        MerkleTree t;
        check(p3hip_mmcs_commit_hash(hash_, ptrs.data(), hs.data(), ws.data(), mats.size(), root.data(), &t.h_));
        t.widths_ = ws;
        return {std::move(root), std::move(t)};
    }
    // -> (opened rows per matrix, sibling digests)
    std::pair<std::vector<std::vector<uint32_t>>, std::vector<uint32_t>> open_batch(size_t index, const MerkleTree& t) const {
        size_t tot = 0;
        for (size_t w : t.widths_) tot += w;
        std::vector<uint32_t> rows(tot ? tot : 1), path(t.log_max_height() * 8 + 8);
        check(p3hip_mmcs_open_batch(t.h_, index, rows.data(), path.data(), nullptr));
        std::vector<std::vector<uint32_t>> out;
        size_t off = 0;
        for (size_t w : t.widths_) { out.emplace_back(rows.begin() + off, rows.begin() + off + w); off += w; }
        path.resize(t.log_max_height() * 8);
        return {std::move(out), std::move(path)};
    }
    // Mmcs::verify_batch (host code): dims = (height, width) per matrix, rows = the opened rows in matrix order, path = the sibling
    // digests.  true / false for accept / RootMismatch; every other reject throws Error with the library's message.
    bool verify_batch(const std::vector<uint32_t>& root, const std::vector<std::pair<size_t, size_t>>& dims, size_t index,
                      const std::vector<std::vector<uint32_t>>& opened_values, const std::vector<uint32_t>& path) const {
        std::vector<size_t> hs, ws;
        for (auto& d : dims) { hs.push_back(d.first); ws.push_back(d.second); }
        std::vector<uint32_t> rows;
        for (auto& v : opened_values) rows.insert(rows.end(), v.begin(), v.end());
        if (root.size() != 8 || path.size() % 8) throw Error(P3HIP_ERR_BAD_ARG, "verify_batch: digests have 8 words");
        rows.push_back(0);  // never a null pointer
        const int rc = p3hip_mmcs_verify_batch(hash_, root.data(), hs.data(), ws.data(), dims.size(), index, rows.data(),
                                               path.empty() ? rows.data() : path.data(), path.size() / 8);
        if (rc == P3HIP_MMCS_ROOT_MISMATCH) { (void)p3hip_take_last_error(); return false; }
        check(rc);
        return true;
    }
    // the bulk, device-resident forms (thin wrappers: device pointers in and out, enqueue only)
    size_t row_words(const MerkleTree& t) const { return p3hip_mmcs_row_words(t.h_); }
    void open_batch_many_dev(const MerkleTree& t, const uint32_t* d_indices, size_t n, uint32_t* d_rows, uint32_t* d_paths,
                             void* stream = nullptr) const {
        check(p3hip_mmcs_open_batch_many_dev(t.h_, d_indices, n, d_rows, d_paths, stream));
    }
    void verify_batch_many_dev(const std::vector<uint32_t>& root, const std::vector<std::pair<size_t, size_t>>& dims, const uint32_t* d_indices,
                               size_t n, const uint32_t* d_rows, const uint32_t* d_paths, uint32_t* d_status, uint32_t* d_rejected = nullptr,
                               void* stream = nullptr) const {
        std::vector<size_t> hs, ws;
        for (auto& d : dims) { hs.push_back(d.first); ws.push_back(d.second); }
        if (root.size() != 8) throw Error(P3HIP_ERR_BAD_ARG, "verify_batch_many: the root has 8 words");
        check(p3hip_mmcs_verify_batch_many_dev(hash_, root.data(), hs.data(), ws.data(), dims.size(), d_indices, n, d_rows, d_paths, d_status,
                                               d_rejected, stream));
    }

  private:
    int hash_;
};

struct FriParameters {  // p3_fri::FriParameters; defaults = create_benchmark_fri_params
    uint32_t log_blowup = 1, log_final_poly_len = 0, num_queries = 100, proof_of_work_bits = 16;
};
class FibAirProver {  // prove(&config, &FibonacciAir{}, generate_trace_rows(a, b, n), &pis), fib_air.rs:61-70
  public:
    // hash: P3HIP_HASH_POSEIDON2 (north_star) or P3HIP_HASH_KECCAK (the reference's own hashes, fib_air.rs:28-53)
    // profile (include/p3hip.h PROFILES): fixed at creation, like the reference's backend (native/src/gpu_dft.rs:85-92).  A prover made on its
    // own proves one proof at a time: the latency profile; provers that share the chip take P3HIP_PROFILE_THROUGHPUT.
    FibAirProver(unsigned log_n, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2, int profile = P3HIP_PROFILE_LATENCY,
                 bool hiding = false, uint64_t seed = 1) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_fib_prover_create_profile(profile, hash, hiding ? 1 : 0, hiding ? seed : 0, log_n, &c, nullptr, 1, &h_));
    }
    FibAirProver(const FibAirProver&) = delete;
    ~FibAirProver() { if (h_) p3hip_fib_prover_destroy(h_); }
    std::vector<uint8_t> prove(uint64_t a, uint64_t b) {
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_fib_prover_prove(h_, a, b, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }
    // prove(&config, &FibonacciAir{}, trace, &pis) for a caller's trace (fib_air.rs:61,68-70): trace = 2^log_n rows x 2 Montgomery
    // words, pis = canonical public values (reduced mod P).  check = upstream's debug-build check_constraints first: a bad row
    // throws Error("constraints had nonzero value on row <i> ...") instead of proving.
    std::vector<uint8_t> prove_trace(const RowMajorMatrix& trace, const uint64_t pis[3], bool check_trace = false) {
        if (trace.width != 2) throw Error(P3HIP_ERR_BAD_ARG, "prove_trace: FibonacciAir traces have two columns");
        const uint32_t pm[3] = {to_monty(pis[0]), to_monty(pis[1]), to_monty(pis[2])};
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_fib_prover_prove_trace(h_, trace.values.data(), trace.height(), pm, check_trace ? P3HIP_PROVE_CHECK_TRACE : 0u, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }
    // the same for a trace in device memory of the prover's device (include/p3hip.h: buffer contract)
    std::vector<uint8_t> prove_trace_dev(const uint32_t* d_trace, const uint64_t pis[3], bool check_trace = false) {
        const uint32_t pm[3] = {to_monty(pis[0]), to_monty(pis[1]), to_monty(pis[2])};
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_fib_prover_prove_trace_dev(h_, d_trace, pm, check_trace ? P3HIP_PROVE_CHECK_TRACE : 0u, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }

  private:
    p3hip_fib_prover_t* h_ = nullptr;
};

// A pool of provers (one host thread + stream each) for batches of independent instances (BASELINE configs[3]).
class FibAirBatchProver {
  public:
    FibAirBatchProver(unsigned log_n, unsigned n_provers = 8, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_fib_batch_create_hash(hash, log_n, &c, n_provers, &h_));
    }
    FibAirBatchProver(const FibAirBatchProver&) = delete;
    ~FibAirBatchProver() { if (h_) p3hip_fib_batch_destroy(h_); }
    std::vector<std::vector<uint8_t>> prove(const std::vector<std::pair<uint64_t, uint64_t>>& instances) {
        size_t n = instances.size();
        std::vector<uint64_t> a(n), b(n);
        for (size_t i = 0; i < n; i++) { a[i] = instances[i].first; b[i] = instances[i].second; }
        std::vector<const uint8_t*> ptrs(n);
        std::vector<size_t> lens(n);
        check(p3hip_fib_batch_prove(h_, n, a.data(), b.data(), ptrs.data(), lens.data()));
        std::vector<std::vector<uint8_t>> out(n);
        for (size_t i = 0; i < n; i++) out[i].assign(ptrs[i], ptrs[i] + lens[i]);
        return out;
    }

  private:
    p3hip_fib_batch_t* h_ = nullptr;
};

// generate_trace_rows' last right value = the public value x (fib_air.rs:57,68)
inline uint64_t fib_public_x(uint64_t a, uint64_t b, uint64_t n) {
    uint64_t l = a % P, r = b % P;
    for (uint64_t i = 1; i < n; i++) { uint64_t t = (l + r) % P; l = r; r = t; }
    return r;
}
// verify(&config, &FibonacciAir{}, &proof, &pis) (fib_air.rs:71-72); throws Error("fib_air verification failed: ...")
inline void verify_fib_air(const std::vector<uint8_t>& proof, uint64_t a, uint64_t b, uint64_t x, unsigned log_n,
                           FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2) {
    p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
    check(p3hip_verify_fib_air_hash(hash, proof.data(), proof.size(), a, b, x, log_n, &c));
}
// verify(&config, &FibonacciAir{}, &proof, &pis) (fib_air.rs:71-72) for batches of proofs of one configuration, on the device
// (p3hip.h "batches of proofs verified ON THE DEVICE": statuses 0, the host verifier's 10 / 11 / 13 / 14 / 15, or P3HIP_VERIFY_MALFORMED)
inline size_t fib_proof_len(unsigned log_n, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2, bool hiding = false) {
    p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
    size_t len = 0;
    check(p3hip_fib_proof_len(hash, hiding ? 1 : 0, log_n, &c, &len));
    return len;
}
class FibVerifier {
  public:
    FibVerifier(unsigned log_n, FriParameters fp, int hash, bool hiding, size_t max_proofs) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_fib_verifier_create(hash, hiding ? 1 : 0, log_n, &c, max_proofs, &h_));
    }
    FibVerifier(const FibVerifier&) = delete;
    FibVerifier& operator=(const FibVerifier&) = delete;
    ~FibVerifier() { p3hip_fib_verifier_destroy(h_); }
    // proofs with their (a, b, x); one status per proof
    std::vector<uint32_t> verify(const std::vector<std::vector<uint8_t>>& proofs, const std::vector<uint64_t>& a,
                                 const std::vector<uint64_t>& b, const std::vector<uint64_t>& x) {
        const size_t n = proofs.size();
        if (a.size() != n || b.size() != n || x.size() != n) throw Error(P3HIP_ERR_BAD_ARG, "FibVerifier: one (a, b, x) per proof");
        std::vector<const uint8_t*> ptrs(n);
        std::vector<size_t> lens(n);
        for (size_t i = 0; i < n; i++) { ptrs[i] = proofs[i].data(); lens[i] = proofs[i].size(); }
        std::vector<uint32_t> status(n);
        check(p3hip_fib_verifier_verify(h_, n, ptrs.data(), lens.data(), a.data(), b.data(), x.data(), status.data()));
        return status;
    }
    // device-resident proofs: enqueues on `stream`, nothing is waited for
    void verify_dev(const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens, const uint32_t* d_pis, size_t n,
                    uint32_t* d_status, uint32_t* d_rejected, void* stream) {
        check(p3hip_fib_verifier_verify_dev(h_, d_proofs, stride_bytes, d_lens, d_pis, n, d_status, d_rejected, stream));
    }

  private:
    p3hip_fib_verifier_t* h_ = nullptr;
};
// The challengers a PCS caller drives (p3hip.h "Fiat-Shamir on the host"): DuplexChallenger (Poseidon2) or SerializingChallenger32 over a
// Keccak-256 HashChallenger.  Field elements are Montgomery words.
class Challenger {
  public:
    explicit Challenger(int hash = P3HIP_HASH_POSEIDON2) { check(p3hip_challenger_create(hash, &h_)); }
    Challenger(const Challenger& o) { check(p3hip_challenger_clone(o.h_, &h_)); }
    Challenger& operator=(const Challenger&) = delete;
    ~Challenger() { p3hip_challenger_destroy(h_); }
    void observe(const std::vector<uint32_t>& words) { check(p3hip_challenger_observe(h_, words.data(), words.size())); }
    void observe_digest(const uint32_t digest[8]) { check(p3hip_challenger_observe_digest(h_, digest)); }
    std::array<uint32_t, 4> sample_ext() { std::array<uint32_t, 4> e{}; check(p3hip_challenger_sample_ext(h_, e.data())); return e; }
    uint32_t sample_bits(unsigned bits) { uint32_t v = 0; check(p3hip_challenger_sample_bits(h_, bits, &v)); return v; }
    p3hip_challenger_t* handle() const { return h_; }
    // the transcript as the words a device verifier imports, and back (p3hip.h p3hip_challenger_export / _import)
    std::array<uint32_t, P3HIP_CHALLENGER_STATE_WORDS> export_state() const {
        std::array<uint32_t, P3HIP_CHALLENGER_STATE_WORDS> w{};
        check(p3hip_challenger_export(h_, w.data()));
        return w;
    }
    void import_state(const std::array<uint32_t, P3HIP_CHALLENGER_STATE_WORDS>& w) { check(p3hip_challenger_import(h_, w.data())); }

  private:
    p3hip_challenger_t* h_ = nullptr;
};
// TwoAdicFriPcs<BabyBear, GpuDft, MerkleTreeMmcs, ExtensionMmcs> over caller matrices in device memory (p3hip.h; non-hiding, one
// height per open).  Points are 4 Montgomery words each, round -> matrix -> point; opened values come back in observation order.
class TwoAdicFriPcs {
  public:
    struct ProverData {  // Pcs::ProverData: the LDEs in HBM and their tree
        p3hip_pcs_data_t* h = nullptr;
        std::array<uint32_t, 8> root{};
        ProverData() = default;
        ProverData(ProverData&& o) noexcept : h(o.h), root(o.root) { o.h = nullptr; }
        ProverData(const ProverData&) = delete;
        ProverData& operator=(const ProverData&) = delete;
        ~ProverData() { p3hip_pcs_data_free(h); }
    };
    struct Opening {
        std::vector<uint32_t> opened;  // 4 words per value
        std::vector<uint8_t> proof;    // the FriProof section of the wire format
    };
    // mixed_heights: commit and open take matrices of any power-of-two heights (p3hip_pcs_create_mixed); false: refused by name
    explicit TwoAdicFriPcs(FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2, int profile = P3HIP_PROFILE_LATENCY,
                           void* stream = nullptr, bool own_stream = true, bool mixed_heights = false)
        : fp_(fp), hash_(hash) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check((mixed_heights ? p3hip_pcs_create_mixed : p3hip_pcs_create)(profile, hash, &c, stream, own_stream ? 1 : 0, &h_));
    }
    TwoAdicFriPcs(const TwoAdicFriPcs&) = delete;
    TwoAdicFriPcs& operator=(const TwoAdicFriPcs&) = delete;
    ~TwoAdicFriPcs() { p3hip_pcs_destroy(h_); }
    // Pcs::commit: evaluations over shifts[m] * <g_h>, natural row order (shifts empty: all 1)
    ProverData commit(const std::vector<const uint32_t*>& d_evals, const std::vector<size_t>& heights, const std::vector<size_t>& widths,
                      const std::vector<uint32_t>& shifts = {}) {
        if (heights.size() != d_evals.size() || widths.size() != d_evals.size() || (!shifts.empty() && shifts.size() != d_evals.size()))
            throw Error(P3HIP_ERR_BAD_ARG, "TwoAdicFriPcs::commit: one height, width and shift per matrix");
        ProverData d;
        check(p3hip_pcs_commit_dev(h_, d_evals.data(), heights.data(), widths.data(), shifts.empty() ? nullptr : shifts.data(), d_evals.size(),
                                   d.root.data(), &d.h));
        return d;
    }
    // Pcs::get_evaluations_on_domain: the stored LDE (a pointer into HBM); the coset GENERATOR * <g_m> is its first m rows, bit-reversed
    const uint32_t* lde(const ProverData& d, size_t mat, size_t* height, size_t* width) const {
        const uint32_t* p = nullptr;
        check(p3hip_pcs_lde_dev(d.h, mat, &p, height, width));
        return p;
    }
    // Pcs::open; opened_words = 4 x the batched columns (sum of width over every (matrix, point) pair)
    Opening open(const std::vector<const ProverData*>& rounds, const std::vector<size_t>& points_per_mat, const std::vector<uint32_t>& points,
                 Challenger& challenger, size_t opened_words) {
        std::vector<const p3hip_pcs_data_t*> hs;
        for (const ProverData* r : rounds) hs.push_back(r ? r->h : nullptr);
        Opening o;
        o.opened.resize(opened_words);
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_pcs_open(h_, hs.data(), hs.size(), points_per_mat.data(), points.data(), challenger.handle(), o.opened.data(), o.opened.size(),
                             &p, &n));
        o.proof.assign(p, p + n);
        return o;
    }
    // Pcs::verify (host): 0 = accept, otherwise the failed check's code (message via take_last_error); throws on a refused argument
    int verify(unsigned log_h, const std::vector<uint32_t>& roots, const std::vector<size_t>& mats_per_round, const std::vector<size_t>& widths,
               const std::vector<size_t>& points_per_mat, const std::vector<uint32_t>& points, const std::vector<uint32_t>& opened,
               const std::vector<uint8_t>& proof, Challenger& challenger) const {
        p3hip_fri_params_t c{fp_.log_blowup, fp_.log_final_poly_len, fp_.num_queries, fp_.proof_of_work_bits};
        int code = 0;
        check(p3hip_pcs_verify(hash_, &c, log_h, roots.data(), mats_per_round.data(), widths.data(), mats_per_round.size(), points_per_mat.data(),
                               points.data(), opened.data(), proof.data(), proof.size(), challenger.handle(), &code));
        return code;
    }
    // the same for matrices of mixed heights: one log height per matrix, round -> matrix (p3hip_pcs_verify_mixed)
    int verify(const std::vector<unsigned>& log_heights, const std::vector<uint32_t>& roots, const std::vector<size_t>& mats_per_round,
               const std::vector<size_t>& widths, const std::vector<size_t>& points_per_mat, const std::vector<uint32_t>& points,
               const std::vector<uint32_t>& opened, const std::vector<uint8_t>& proof, Challenger& challenger) const {
        if (log_heights.size() != widths.size()) throw Error(P3HIP_ERR_BAD_ARG, "TwoAdicFriPcs::verify: one log height per matrix");
        p3hip_fri_params_t c{fp_.log_blowup, fp_.log_final_poly_len, fp_.num_queries, fp_.proof_of_work_bits};
        int code = 0;
        check(p3hip_pcs_verify_mixed(hash_, &c, log_heights.data(), roots.data(), mats_per_round.data(), widths.data(), mats_per_round.size(),
                                     points_per_mat.data(), points.data(), opened.data(), proof.data(), proof.size(), challenger.handle(), &code));
        return code;
    }

  protected:
    struct Adopt {};  // HidingFriPcs creates the object itself
    TwoAdicFriPcs(Adopt, FriParameters fp, int hash) : fp_(fp), hash_(hash) {}
    p3hip_pcs_t* h_ = nullptr;
    FriParameters fp_;
    int hash_;
};
// HidingFriPcs<BabyBear, GpuDft, MerkleTreeHidingMmcs, ExtensionMmcs over it, SmallRng> over caller matrices (p3hip.h "HidingFriPcs over
// CALLER-SUPPLIED matrices": what the reference builds, fib_air.rs:63-65).  commit, lde and open are the base class's on a hiding object:
// commit randomizes (the stored LDE has 2h << log_blowup rows of width w + num_random_codewords, the caller's columns first), open opens
// every committed column.  The three random streams live in the object and advance from call to call.
class HidingFriPcs : public TwoAdicFriPcs {
  public:
    explicit HidingFriPcs(FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2, int profile = P3HIP_PROFILE_LATENCY,
                          unsigned num_random_codewords = 4, uint64_t mmcs_seed = 1, uint64_t pcs_seed = 1, void* stream = nullptr,
                          bool own_stream = true)
        : TwoAdicFriPcs(Adopt{}, fp, hash) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_pcs_create_hiding(profile, hash, &c, num_random_codewords, mmcs_seed, pcs_seed, stream, own_stream ? 1 : 0, &h_));
    }
    // HidingFriPcs::commit_quotient: 2 or 4 chunk matrices of h x width, chunk c on GENERATOR g_(C h)^c <g_h>, natural row order
    ProverData commit_quotient(const std::vector<const uint32_t*>& d_chunks, size_t h, size_t width) {
        ProverData d;
        check(p3hip_pcs_commit_quotient_dev(h_, d_chunks.data(), h, width, d_chunks.size(), d.root.data(), &d.h));
        return d;
    }
    // HidingFriPcs::get_opt_randomization_poly_commitment for traces of 2^log_h rows
    ProverData get_opt_randomization_poly_commitment(unsigned log_h) {
        ProverData d;
        check(p3hip_pcs_commit_randomization(h_, log_h, d.root.data(), &d.h));
        return d;
    }
    // HidingFriPcs::verify (host): log_h the caller's log height, widths the committed ones; codes as TwoAdicFriPcs::verify
    int verify(unsigned log_h, const std::vector<uint32_t>& roots, const std::vector<size_t>& mats_per_round, const std::vector<size_t>& widths,
               const std::vector<size_t>& points_per_mat, const std::vector<uint32_t>& points, const std::vector<uint32_t>& opened,
               const std::vector<uint8_t>& proof, Challenger& challenger) const {
        p3hip_fri_params_t c{fp_.log_blowup, fp_.log_final_poly_len, fp_.num_queries, fp_.proof_of_work_bits};
        int code = 0;
        check(p3hip_pcs_verify_hiding(hash_, &c, log_h, roots.data(), mats_per_round.data(), widths.data(), mats_per_round.size(),
                                      points_per_mat.data(), points.data(), opened.data(), proof.data(), proof.size(), challenger.handle(), &code));
        return code;
    }
};

// Pcs::verify of TwoAdicFriPcs / HidingFriPcs for batches of members of ONE shape, on the device (p3hip.h "batches of PCS proofs verified
// ON THE DEVICE").  widths: the committed widths, round -> matrix; slots: one per (matrix, point) pair, round -> matrix -> point.
class PcsVerifier {
  public:
    PcsVerifier(int hash, bool hiding, FriParameters fp, unsigned log_h, const std::vector<size_t>& mats_per_round, const std::vector<size_t>& widths,
                const std::vector<size_t>& points_per_mat, size_t n_slots, const std::vector<uint32_t>& slots, size_t max_proofs)
        : n_rounds_(mats_per_round.size()), n_slots_(n_slots) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        p3hip_pcs_shape_t s{log_h, mats_per_round.size(), mats_per_round.data(), widths.data(), points_per_mat.data(), n_slots, slots.data()};
        if (widths.size() != points_per_mat.size()) throw Error(P3HIP_ERR_BAD_ARG, "PcsVerifier: one point count per matrix");
        for (size_t m = 0; m < widths.size(); m++) total_ += widths[m] * points_per_mat[m];
        check(p3hip_pcs_proof_len(hash, hiding ? 1 : 0, &c, &s, &proof_len_));
        check(p3hip_pcs_verifier_create(hash, hiding ? 1 : 0, &c, &s, max_proofs, &h_));
    }
    // mixed heights: log_heights, one log height per matrix (round -> matrix), in place of log_h (p3hip_pcs_verifier_create_mixed);
    // hiding is refused by the library
    PcsVerifier(int hash, bool hiding, FriParameters fp, const std::vector<unsigned>& log_heights, const std::vector<size_t>& mats_per_round,
                const std::vector<size_t>& widths, const std::vector<size_t>& points_per_mat, size_t n_slots, const std::vector<uint32_t>& slots,
                size_t max_proofs)
        : n_rounds_(mats_per_round.size()), n_slots_(n_slots) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        p3hip_pcs_shape_t s{0, mats_per_round.size(), mats_per_round.data(), widths.data(), points_per_mat.data(), n_slots, slots.data()};
        if (widths.size() != points_per_mat.size()) throw Error(P3HIP_ERR_BAD_ARG, "PcsVerifier: one point count per matrix");
        if (widths.size() != log_heights.size()) throw Error(P3HIP_ERR_BAD_ARG, "PcsVerifier: one log height per matrix");
        for (size_t m = 0; m < widths.size(); m++) total_ += widths[m] * points_per_mat[m];
        check(p3hip_pcs_proof_len_mixed(hash, hiding ? 1 : 0, &c, &s, log_heights.data(), &proof_len_));
        check(p3hip_pcs_verifier_create_mixed(hash, hiding ? 1 : 0, &c, &s, log_heights.data(), max_proofs, &h_));
    }
    PcsVerifier(const PcsVerifier&) = delete;
    PcsVerifier& operator=(const PcsVerifier&) = delete;
    ~PcsVerifier() { p3hip_pcs_verifier_destroy(h_); }
    size_t proof_len() const { return proof_len_; }
    // per member: n_rounds x 8 root words, n_slots x 4 point words, total x 4 opened words and its challenger (advanced when the
    // member is accepted, left alone otherwise); one status per member
    std::vector<uint32_t> verify_many(const std::vector<std::vector<uint8_t>>& proofs, const std::vector<uint32_t>& roots,
                                      const std::vector<uint32_t>& points, const std::vector<uint32_t>& opened,
                                      const std::vector<Challenger*>& challengers) {
        const size_t n = proofs.size();
        if (challengers.size() != n || roots.size() != n * n_rounds_ * 8 || points.size() != n * n_slots_ * 4 || opened.size() != n * total_ * 4)
            throw Error(P3HIP_ERR_BAD_ARG, "PcsVerifier: one challenger, n_rounds roots, n_slots points and `total` opened values per proof");
        std::vector<const uint8_t*> ptrs(n);
        std::vector<size_t> lens(n);
        std::vector<p3hip_challenger_t*> ch(n);
        for (size_t i = 0; i < n; i++) { ptrs[i] = proofs[i].data(); lens[i] = proofs[i].size(); ch[i] = challengers[i]->handle(); }
        std::vector<uint32_t> status(n);
        check(p3hip_pcs_verifier_verify(h_, n, ptrs.data(), lens.data(), roots.data(), points.data(), opened.data(), ch.data(), status.data()));
        return status;
    }
    // device-resident members: enqueues on `stream`, nothing is waited for
    void verify_many_dev(const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens, const uint32_t* d_roots, const uint32_t* d_points,
                         const uint32_t* d_opened, const uint32_t* d_chal_in, size_t n, uint32_t* d_status, uint32_t* d_rejected,
                         uint32_t* d_chal_out, void* stream) {
        check(p3hip_pcs_verifier_verify_dev(h_, d_proofs, stride_bytes, d_lens, d_roots, d_points, d_opened, d_chal_in, n, d_status, d_rejected,
                                            d_chal_out, stream));
    }

  private:
    p3hip_pcs_verifier_t* h_ = nullptr;
    size_t n_rounds_ = 0, n_slots_ = 0, total_ = 0, proof_len_ = 0;
};

// A caller-defined AIR as a validated program (p3hip.h "caller-defined AIRs"): the quotient kernel, the trace check and the verifier's
// evaluation.  code: 4 words per instruction {op, dst, a, b}; operands are air_operand(kind, index).
inline uint32_t air_operand(uint32_t kind, uint32_t index) { return (kind << P3HIP_AIR_KIND_SHIFT) | index; }
class Air {
  public:
    Air(size_t width, size_t n_public, const std::vector<uint32_t>& code, const std::vector<uint32_t>& consts) {
        if (code.size() % 4) throw Error(P3HIP_ERR_BAD_ARG, "Air: four words per instruction");
        check(p3hip_air_create(width, n_public, code.data(), code.size() / 4, consts.data(), consts.size(), &h_));
        if (p3hip_air_info(h_, &info_) != 0) {
            p3hip_air_destroy(h_);
            throw Error(P3HIP_ERR_BAD_ARG, take_last_error());
        }
    }
    Air(const Air&) = delete;
    Air& operator=(const Air&) = delete;
    ~Air() { p3hip_air_destroy(h_); }
    const p3hip_air_info_t& info() const { return info_; }
    size_t n_chunks() const { return (size_t)1 << info_.log_quotient_degree; }
    p3hip_air_t* handle() const { return h_; }
    // quotient_values: d_lde as p3hip_pcs_lde_dev hands it out; d_chunks: n_chunks() device matrices of 2^log_n x 4 words.  Enqueues only.
    void quotient_dev(void* stream, const uint32_t* d_lde, unsigned log_n, unsigned log_blowup, const std::vector<uint32_t>& pis,
                      const std::array<uint32_t, 4>& alpha, const std::vector<uint32_t*>& d_chunks) {
        if (d_chunks.size() != n_chunks() || pis.size() != info_.n_public) throw Error(P3HIP_ERR_BAD_ARG, "Air: n_chunks chunk pointers, n_public public values");
        check(p3hip_air_quotient_dev(h_, stream, d_lde, log_n, log_blowup, pis.data(), alpha.data(), d_chunks.data()));
    }
    // check_constraints over a device trace: {-1, -1} when every constraint holds, else the smallest failing {row, constraint}
    std::pair<long long, int> check_trace_dev(void* stream, const uint32_t* d_trace, unsigned log_n, const std::vector<uint32_t>& pis) {
        if (pis.size() != info_.n_public) throw Error(P3HIP_ERR_BAD_ARG, "Air: n_public public values");
        long long row = -1;
        int k = -1;
        check(p3hip_air_check_trace_dev(h_, stream, d_trace, log_n, pis.data(), &row, &k));
        return {row, k};
    }
    // the constraints over extension operands folded by Horner's rule (host): local, next width x 4 words; sels 3 x 4 words
    std::array<uint32_t, 4> eval_ext(const std::vector<uint32_t>& local, const std::vector<uint32_t>& next, const std::vector<uint32_t>& pis,
                                     const std::array<uint32_t, 12>& sels, const std::array<uint32_t, 4>& alpha) const {
        if (local.size() != 4 * (size_t)info_.width || next.size() != local.size() || pis.size() != info_.n_public)
            throw Error(P3HIP_ERR_BAD_ARG, "Air: width x 4 words per row, n_public public values");
        std::array<uint32_t, 4> out{};
        check(p3hip_air_eval_ext(h_, local.data(), next.data(), pis.data(), sels.data(), alpha.data(), out.data()));
        return out;
    }

    // eval_ext at n points in one launch (device buffers; enqueues only)
    void eval_ext_dev(void* stream, const uint32_t* d_local, const uint32_t* d_next, const uint32_t* d_pis, const uint32_t* d_sels,
                      const uint32_t* d_alpha, size_t n, uint32_t* d_out) {
        check(p3hip_air_eval_ext_dev(h_, stream, d_local, d_next, d_pis, d_sels, d_alpha, n, d_out));
    }

  private:
    p3hip_air_t* h_ = nullptr;
    p3hip_air_info_t info_{};
};

// p3_uni_stark::verify for proofs of a caller-defined AIR (p3hip.h p3hip_air_proof_len / p3hip_air_verify / p3hip_air_verifier_*).
// The byte length every proof of (air, log_n, fp, hash) has; host only.
inline size_t air_proof_len(const Air& air, unsigned log_n, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2) {
    p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
    size_t len = 0;
    check(p3hip_air_proof_len(air.handle(), hash, log_n, &c, &len));
    return len;
}
// One proof on the host: 0 = accept, else the failed check's code (1-4 header, 10 OodEvaluationMismatch, the PCS verifier's otherwise)
inline int air_verify(const Air& air, const std::vector<uint8_t>& proof, const std::vector<uint32_t>& pis, unsigned log_n,
                      FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2) {
    if (pis.size() != air.info().n_public) throw Error(P3HIP_ERR_BAD_ARG, "air_verify: n_public public values");
    p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
    int code = 0;
    check(p3hip_air_verify(air.handle(), hash, log_n, &c, proof.data(), proof.size(), pis.data(), &code));
    return code;
}
// Batches of such proofs on the device.  The Air may be destroyed once the verifier exists.
class AirVerifier {
  public:
    AirVerifier(const Air& air, unsigned log_n, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2, size_t max_proofs = 64)
        : n_public_(air.info().n_public), proof_len_(air_proof_len(air, log_n, fp, hash)) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_air_verifier_create(air.handle(), hash, log_n, &c, max_proofs, &h_));
    }
    AirVerifier(const AirVerifier&) = delete;
    AirVerifier& operator=(const AirVerifier&) = delete;
    ~AirVerifier() { p3hip_air_verifier_destroy(h_); }
    size_t proof_len() const { return proof_len_; }
    // pis: n_public Montgomery words per proof; one status per proof (0, 10, 11, 13, 14, 15 or P3HIP_VERIFY_MALFORMED)
    std::vector<uint32_t> verify_many(const std::vector<std::vector<uint8_t>>& proofs, const std::vector<uint32_t>& pis) {
        const size_t n = proofs.size();
        if (pis.size() != n * n_public_) throw Error(P3HIP_ERR_BAD_ARG, "AirVerifier: n_public public values per proof");
        std::vector<const uint8_t*> ptrs(n);
        std::vector<size_t> lens(n);
        for (size_t i = 0; i < n; i++) { ptrs[i] = proofs[i].data(); lens[i] = proofs[i].size(); }
        std::vector<uint32_t> status(n);
        check(p3hip_air_verifier_verify(h_, n, ptrs.data(), lens.data(), pis.data(), status.data()));
        return status;
    }
    // device-resident members: enqueues on `stream`, nothing is waited for
    void verify_many_dev(const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens, const uint32_t* d_pis, size_t n, uint32_t* d_status,
                         uint32_t* d_rejected, void* stream) {
        check(p3hip_air_verifier_verify_dev(h_, d_proofs, stride_bytes, d_lens, d_pis, n, d_status, d_rejected, stream));
    }

  private:
    p3hip_air_verifier_t* h_ = nullptr;
    size_t n_public_ = 0, proof_len_ = 0;
};

// p3_uni_stark::prove for a caller-defined AIR in one device-resident launch chain (p3hip.h p3hip_air_prover_*): the arena of one (air,
// log_n, fp, hash, profile); a proof allocates nothing and synchronises once.  The Air may be destroyed once the prover exists.
class AirProver {
  public:
    AirProver(const Air& air, unsigned log_n, FriParameters fp = FriParameters(), int hash = P3HIP_HASH_POSEIDON2,
              int profile = P3HIP_PROFILE_LATENCY, void* stream = nullptr, bool own_stream = true)
        : log_n_(log_n), width_(air.info().width), n_public_(air.info().n_public) {
        p3hip_fri_params_t c{fp.log_blowup, fp.log_final_poly_len, fp.num_queries, fp.proof_of_work_bits};
        check(p3hip_air_prover_create(air.handle(), profile, hash, log_n, &c, stream, own_stream ? 1 : 0, &h_));
    }
    AirProver(const AirProver&) = delete;
    AirProver& operator=(const AirProver&) = delete;
    ~AirProver() { p3hip_air_prover_destroy(h_); }
    // d_trace: 2^log_n x width Montgomery words of device memory, read in place; check: P3HIP_PROVE_CHECK_TRACE first
    std::vector<uint8_t> prove_dev(const uint32_t* d_trace, const std::vector<uint32_t>& pis, bool check_constraints = false) {
        need_pis(pis);
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_air_prover_prove_dev(h_, d_trace, pis.data(), check_constraints ? P3HIP_PROVE_CHECK_TRACE : 0u, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }
    // the same for a trace in host memory (row-major, 2^log_n x width words), uploaded
    std::vector<uint8_t> prove(const std::vector<uint32_t>& trace, const std::vector<uint32_t>& pis, bool check_constraints = false) {
        need_pis(pis);
        if (trace.size() != ((size_t)width_ << log_n_)) throw Error(P3HIP_ERR_BAD_ARG, "AirProver: a trace of 2^log_n x width words");
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_air_prover_prove(h_, trace.data(), pis.data(), check_constraints ? P3HIP_PROVE_CHECK_TRACE : 0u, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }
    // the two halves: one proof in flight; the trace stays unchanged until finish returns
    void enqueue_dev(const uint32_t* d_trace, const std::vector<uint32_t>& pis) {
        need_pis(pis);
        check(p3hip_air_prover_enqueue_dev(h_, d_trace, pis.data()));
    }
    std::vector<uint8_t> finish() {
        const uint8_t* p = nullptr;
        size_t n = 0;
        check(p3hip_air_prover_finish(h_, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }

  private:
    void need_pis(const std::vector<uint32_t>& pis) const {
        if (pis.size() != n_public_) throw Error(P3HIP_ERR_BAD_ARG, "AirProver: n_public public values");
    }
    p3hip_air_prover_t* h_ = nullptr;
    unsigned log_n_ = 0;
    size_t width_ = 0, n_public_ = 0;
};

// run_fib_air_zk (fib_air.rs:27-75) on the hip backend (non-hiding; either hash configuration): "fib_air ok (n=8, x=21)"
inline std::string run_fib_air(unsigned log_n = 3, uint64_t a = 0, uint64_t b = 1, FriParameters fp = FriParameters(),
                               int hash = P3HIP_HASH_POSEIDON2) {
    uint64_t n = 1ull << log_n, x = fib_public_x(a, b, n);
    FibAirProver prover(log_n, fp, hash);
    verify_fib_air(prover.prove(a, b), a, b, x, log_n, fp, hash);
    return "fib_air ok (n=" + std::to_string(n) + ", x=" + std::to_string(x) + ")";
}

// The String of the reference's runFibAirZk() (lib.rs:37-83) from the library: its own instance and configuration
// (n = 8, x = 21, Keccak hashes, hiding MMCS + PCS, seed 1) on the backend the selector names.  Never throws: failures are text.
inline std::string run_fib_air_zk_report() {
    std::string buf(1024, '\0');
    p3hip_run_fib_air_zk(&buf[0], buf.size());
    return std::string(buf.c_str());
}
// The String of runDftBenchmark() (lib.rs:86-131); cpu_dft supplies the CPU column (Radix2DitParallel in the Rust shim).
inline std::string run_dft_benchmark_report(p3hip_cpu_dft_fn cpu_dft = nullptr, void* user = nullptr) {
    std::string buf(1 << 14, '\0');
    p3hip_run_dft_benchmark(cpu_dft, user, &buf[0], buf.size());
    return std::string(buf.c_str());
}

}  // namespace p3hip
