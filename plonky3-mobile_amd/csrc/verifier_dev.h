// verifier_dev.hip: batches of fib_air proofs of ONE configuration verified on the device (include/p3hip.h p3hip_fib_verifier_*).
#pragma once
#include "prover.h"

namespace p3 {

// d_status code of a proof whose length, a count / width / length word, or a field word (>= P) is not what the configuration
// dictates; the other codes are the host verifier's (verifier.hip)
constexpr uint32_t VERIFY_MALFORMED = 16;

// The object's device for the duration of a call (HIP's current device is per thread): both batch verifiers enter their device
// this way, so a call from a thread whose current device is another one is redirected, not refused.
struct DeviceScope {
    int prev = -1, want;
    bool switched = false;
    explicit DeviceScope(int dev) : want(dev) {}
    int enter() {
        P3_HIP(hipGetDevice(&prev));
        if (prev != want) { P3_HIP(hipSetDevice(want)); switched = true; }
        return OK;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

// host only: the byte length every proof of the configuration has
int fib_proof_len(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t* len_out);

class FibVerifierDev {
  public:
    FibVerifierDev();
    ~FibVerifierDev();
    FibVerifierDev(const FibVerifierDev&) = delete;
    // allocates every scratch buffer of the device entry for max_proofs proofs on the calling thread's current device
    int init(int hash, bool hiding, uint32_t log_n, const FriParams& fp, size_t max_proofs);
    // enqueue only: no allocation, no host copy, no synchronise
    int verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_pis, size_t n, uint32_t* d_status,
                   uint32_t* d_rejected, hipStream_t stream);
    // uploads (its staging is allocated by the first call), verifies in rounds of max_proofs, downloads; synchronises
    int verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint64_t* a, const uint64_t* b, const uint64_t* x,
                    uint32_t* status_out);
    size_t proof_len() const;
    size_t max_proofs() const;
    int device() const;

  private:
    struct Impl;
    Impl* im;
};

}  // namespace p3
