// Host side of the device batch verifiers (pcs_verifier_dev.hip: PCS proofs; verifier_dev.hip: fib_air proofs; air_verifier_dev.hip: a
// caller-defined AIR's), what their Impls share: the object's device and its buffers, freed together; the host entry's staging (a
// non-blocking stream, d_proofs, d_lens, d_status and the verifier's own extras), made by the first call that needs it; a chunk's upload,
// with the rule that a proof of the wrong length is rejected unread; the status download; the argument checks of verify_dev and the
// alignment test they use.  Device code is in verifier_dev_common.hip.h.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "common.h"
#include "verifier_dev.h"

namespace p3 {

inline bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

struct VerifierDevHost {
    int device = -1;  // none until init has a context
    size_t max_proofs = 0;
    std::vector<void*> bufs;  // every device buffer of the object, in allocation order
    // the host entry's staging: allocated by its first call (the device entry never needs it)
    uint8_t* d_proofs = nullptr;
    uint32_t *d_lens = nullptr, *d_status = nullptr;
    hipStream_t stream = nullptr;
    bool staging_ready = false;
    std::vector<uint32_t> hl;  // a chunk's lengths as the kernels see them

    struct Buf { void** p; size_t bytes; };
    template <typename T> static Buf buf(T** p, size_t bytes) { return Buf{reinterpret_cast<void**>(p), bytes}; }

    ~VerifierDevHost() {
        if (device < 0) return;  // init refused before anything was allocated: no device to visit
        DeviceScope ds(device);
        (void)ds.enter();
        for (void* p : bufs) if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // Each buffer and the stream are made once and the flag is set last: a call that failed half way is resumed by the next.
    int alloc(std::initializer_list<Buf> list) {
        for (const Buf& b : list) {
            if (*b.p) continue;
            bufs.push_back(nullptr);
            P3_HIP(hipMalloc(b.p, b.bytes));
            bufs.back() = *b.p;
        }
        return OK;
    }
    int stage(size_t plen, std::initializer_list<Buf> extras) {
        if (staging_ready) return OK;
        if (!stream) P3_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (int rc = alloc({buf(&d_proofs, max_proofs * plen), buf(&d_lens, max_proofs * 4)})) return rc;
        if (int rc = alloc(extras)) return rc;
        if (int rc = alloc({buf(&d_status, max_proofs * 4)})) return rc;
        hl.resize(max_proofs);
        staging_ready = true;
        return OK;
    }
    // one chunk of m <= max_proofs members: the proofs, then d_lens.  `entry` names the caller in a refusal.
    int upload(const char* entry, size_t m, const uint8_t* const* proofs, const size_t* lens, size_t plen) {
        for (size_t k = 0; k < m; k++) {
            if (lens[k] == plen) {
                if (!proofs[k]) return fail(ERR_BAD_ARG, std::string(entry) + ": null proof");
                P3_HIP(hipMemcpyAsync(d_proofs + k * plen, proofs[k], plen, hipMemcpyHostToDevice, stream));
                hl[k] = (uint32_t)plen;
            } else hl[k] = lens[k] > 0xfffffffeull ? 0xffffffffu : (uint32_t)lens[k];  // a wrong length is rejected unread: nothing is uploaded
        }
        P3_HIP(hipMemcpyAsync(d_lens, hl.data(), m * 4, hipMemcpyHostToDevice, stream));
        return OK;
    }
    int download_status(uint32_t* status_out, size_t m) { P3_HIP(hipMemcpyAsync(status_out, d_status, m * 4, hipMemcpyDeviceToHost, stream)); return OK; }
    // what the two verify_dev check alike, in their order
    int check_batch(const char* entry, size_t n, bool null_arg, size_t stride, size_t plen) const {
        if (n > max_proofs) return fail(ERR_BAD_ARG, std::string(entry) + ": more proofs than the verifier was created for");
        if (n && null_arg) return fail(ERR_BAD_ARG, std::string(entry) + ": null argument");
        if (n && ((stride & 3u) || stride < plen)) return fail(ERR_BAD_ARG, std::string(entry) + ": the stride must be a multiple of 4 and at least the proof length");
        return OK;
    }
};

}  // namespace p3
