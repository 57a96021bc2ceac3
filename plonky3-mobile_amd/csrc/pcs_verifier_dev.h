// pcs_verifier_dev.hip: batches of TwoAdicFriPcs / HidingFriPcs proofs of ONE shape verified on the device (include/p3hip.h
// p3hip_pcs_verifier_*).
#pragma once
#include "pcs_layout.h"  // PcsShape, PCS_MAX_SLOTS
#include "prover.h"
#include "verifier_dev.h"

namespace p3 {

// host only: the byte length every proof of the shape has
int pcs_proof_len(int hash, bool hiding, const FriParams& fp, const PcsShape& shape, size_t* len_out);

class PcsVerifierDev {
  public:
    PcsVerifierDev();
    ~PcsVerifierDev();
    PcsVerifierDev(const PcsVerifierDev&) = delete;
    // allocates every scratch buffer of the device entry for max_proofs members on the calling thread's current device
    int init(int hash, bool hiding, const FriParams& fp, const PcsShape& shape, size_t max_proofs);
    // enqueue only: no allocation, no host copy, no synchronise.  d_owner_key (an owning verifier's; not in the C ABI): per member the
    // order key (verifier_dev_common.hip.h) its owner's checks left it at, KEY_NONE when they passed.  A member at KEY_HEADER is skipped
    // unread; any other starts from that key, so d_status and d_rejected are final for the owner's caller.
    int verify_dev(const uint8_t* d_proofs, size_t stride, const uint32_t* d_lens, const uint32_t* d_roots, const uint32_t* d_points,
                   const uint32_t* d_opened, const uint32_t* d_chal_in, size_t n, uint32_t* d_status, uint32_t* d_rejected,
                   uint32_t* d_chal_out, hipStream_t stream, const unsigned long long* d_owner_key = nullptr);
    // uploads (its staging is allocated by the first call), verifies in rounds of max_proofs, downloads; synchronises.  An accepted
    // member's challenger comes out as the host verifier leaves it, a rejected member's is unchanged.
    int verify_host(size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* roots, const uint32_t* points,
                    const uint32_t* opened, Challenger* const* chals, uint32_t* status_out);
    size_t proof_len() const;
    size_t max_proofs() const;
    size_t total_columns() const;  // opened values of one member
    bool wave_form() const;        // the reduced opening runs one wavefront per query
    int hash() const;
    int device() const;

  private:
    struct Impl;
    Impl* im;
};

}  // namespace p3
