// air_verifier_dev.hip: p3_uni_stark::verify for a caller-defined AIR (air.h) — one proof on the host, batches of proofs of ONE
// (AIR, log_n, FRI parameters, hash) on the device (include/p3hip.h p3hip_air_proof_len, p3hip_air_verify, p3hip_air_verifier_*,
// p3hip_air_eval_ext_dev).
#pragma once
#include "air.h"
#include "prover.h"
#include "verifier_dev.h"

namespace p3 {

// host only: the byte length every prove_air proof of (air, log_n, fp) has; the gates are the PCS verifier's plus the AIR's two
int air_proof_len(const Air& air, int hash, uint32_t log_n, const FriParams& fp, size_t* len_out);
// host only, one proof: 0 = accept, ERR_BAD_ARG for a refused argument, else the failed check's code (1..4 the header, 10
// OodEvaluationMismatch, the PCS verifier's otherwise)
int air_verify(const Air& air, int hash, uint32_t log_n, const FriParams& fp, const uint8_t* proof, size_t len, const uint32_t* pis, std::string* why);
// the program over extension operands at n points, one lane per point (the interpreter core of av_eval_kernel); enqueue only
int air_eval_ext_dev(Air& air, hipStream_t stream, const uint32_t* d_local, const uint32_t* d_next, const uint32_t* d_pis, const uint32_t* d_sels,
                     const uint32_t* d_alpha, size_t n, uint32_t* d_out);

class AirVerifierDev {
  public:
    AirVerifierDev();
    ~AirVerifierDev();
    AirVerifierDev(const AirVerifierDev&) = delete;
    // copies the program to the calling thread's current device and allocates every scratch buffer of the device entry (the owned
    // PCS verifier's included) for max_proofs members; `air` is not referred to afterwards
    int init(const Air& air, int hash, uint32_t log_n, const FriParams& fp, size_t max_proofs);
    // enqueue only: no allocation, no host copy, no synchronise
    int verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_pis, size_t n, uint32_t* d_status,
                   uint32_t* d_rejected, hipStream_t stream);
    // uploads (its staging is allocated by the first call), verifies in rounds of max_proofs, downloads; synchronises
    int verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* pis, uint32_t* status_out);
    size_t proof_len() const;
    size_t max_proofs() const;
    int device() const;

  private:
    struct Impl;
    Impl* im;
};

}  // namespace p3
