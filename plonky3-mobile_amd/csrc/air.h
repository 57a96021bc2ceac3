// A caller-defined AIR as a small program (include/p3hip.h "caller-defined AIRs"): the validated program, its figures and the
// device copies the two kernels of air.hip read.  Everything a kernel indexes with comes from here, checked once by air_create.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/p3hip.h"

namespace p3 {

constexpr uint32_t AIR_BLOCK = 256;  // lanes per workgroup: a value slot costs AIR_BLOCK * 4 = 1 KiB of LDS
// 64 slots = 64 KiB per workgroup: two workgroups fit a CU's 160 KiB
static_assert(P3HIP_AIR_MAX_SLOTS * AIR_BLOCK * 4 * 2 <= 160 * 1024, "two workgroups per CU");
constexpr uint32_t AIR_MAX_CHUNKS = 1u << P3HIP_AIR_MAX_LOG_QUOTIENT_DEGREE;
constexpr uint32_t AIR_DEGREE_SATURATED = 1u << 20;  // degrees of intermediate values are tracked up to here

struct Air {
    uint32_t width = 0, n_public = 0, n_constraints = 0, n_slots = 0, max_degree = 0, log_quotient_degree = 0;
    std::vector<uint32_t> code;    // 4 words per instruction
    std::vector<uint32_t> consts;  // Montgomery words
    int device = -1;
    uint32_t* d_code = nullptr;    // one allocation: code | consts | per-call table | found
    uint32_t* d_consts = nullptr;
    uint32_t* d_tab = nullptr;     // per call: publics | alpha powers | Z_H | 1 / Z_H | chunk pointers
    unsigned long long* d_found = nullptr;
    size_t tab_words = 0;
    std::vector<uint32_t> h_tab;   // the table of the call being prepared
    uint32_t* h_pin = nullptr;     // pinned staging of tab_words words: the source of the upload
    void* up_done = nullptr;       // hipEvent_t recorded behind the upload: the staging is rewritten only after it
    void* run_done = nullptr;      // hipEvent_t recorded behind the kernel (check: behind the memset too) on last_stream: a call on
    void* last_stream = nullptr;   // ANOTHER stream waits for it before it touches d_tab / d_found
    bool ran = false;
    ~Air();
};

// makes the device copies of the program on the calling thread's current device (what the first device call of an Air does)
int air_ensure_device(Air& a);

// What an owner of a table of its own needs (AirProver, prover.hip): the table of a quotient over 2^log_n rows is
// publics | K alpha powers, entry k = alpha^(K-1-k), at `ap` | Z_H, 1 / Z_H at `zh` | (8-byte aligned) chunk pointers, `words` in all
// (at most Air::tab_words).  air_table_tail fills words [zh, words) into `tail`: they depend on log_n and the chunks alone.
struct AirTable {
    uint32_t ap, zh, words;
};
AirTable air_table(const Air& a, uint32_t log_n);
void air_table_tail(const Air& a, uint32_t log_n, uint32_t* const* d_chunks, uint32_t* tail);
// air_kernel<0> alone on table d_tab, which the caller has filled in stream order: no upload, no event, nothing checked
int air_quotient_launch(Air& a, hipStream_t st, const uint32_t* d_tab, const uint32_t* d_lde, uint32_t log_n);
// p3hip_air_check_trace_dev behind its argument checks
int air_check_trace(Air& a, hipStream_t st, const uint32_t* d_trace, uint32_t log_n, const uint32_t* pis, long long* row_out, int* constraint_out);

}  // namespace p3

struct p3hip_air {
    p3::Air a;
};
