// extern "C" surface of libp3hip (include/p3hip.h).  Thin: argument checks, context lookup, host<->device
// staging for the host-pointer entry points.  Never throws across the boundary (JNI wrappers in the
// reference catch panics, native/src/lib.rs:45-59; here every path returns a status code).
#include "../../include/p3hip.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <deque>
#include <thread>
#include <cctype>
#include <cstdio>
#include <cstring>

#include "air_verifier_dev.h"
#include "bb31.hip.h"
#include "challenger.h"
#include "common.h"
#include "mmcs.h"
#include "prover.h"
#include "pcs_verifier_dev.h"
#include "verifier_dev.h"
#include "rng.h"

namespace p3 {
bool take_error(std::string* out);
}
using namespace p3;

// gpu_dft.rs:41: `static BACKEND_KIND: AtomicU8` — default is the GPU backend.
static std::atomic<uint8_t> g_backend{P3HIP_BACKEND_HIP};

template <class F>
static int guarded(F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        return fail(ERR_INTERNAL, std::string("exception: ") + e.what());
    } catch (...) {
        return fail(ERR_INTERNAL, "unknown exception");
    }
}

extern "C" {

int p3hip_set_backend(const char* name) {
    if (!name) return fail(ERR_BACKEND, "unknown backend '<null>'");
    std::string v;
    for (const char* p = name; *p; ++p) v.push_back((char)std::tolower((unsigned char)*p));
    uint8_t kind;
    if (v == "cpu") kind = P3HIP_BACKEND_CPU;
    else if (v == "vulkan") kind = P3HIP_BACKEND_VULKAN;
    else if (v == "metal") kind = P3HIP_BACKEND_METAL;
    else if (v == "webgpu") kind = P3HIP_BACKEND_WEBGPU;
    else if (v == "hip") kind = P3HIP_BACKEND_HIP;
    else return fail(ERR_BACKEND, "unknown backend '" + v + "'");
    g_backend.store(kind, std::memory_order_relaxed);
    return OK;
}

int p3hip_get_backend(void) { return g_backend.load(std::memory_order_relaxed); }

int p3hip_is_available(char* msg, size_t cap) {
    return guarded([&]() -> int {
        Context* cx = nullptr;
        int rc = get_context(&cx);
        std::string text;
        if (rc == OK) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, cx->device) == hipSuccess)
                text = std::string("HIP available: ") + prop.name + " (" + prop.gcnArchName + ")";
            else
                text = "HIP available";
        } else {
            std::string err;
            take_error(&err);
            text = "HIP unavailable: " + err;
            set_error(err);
        }
        if (msg && cap) snprintf(msg, cap, "%s", text.c_str());
        return rc;
    });
}

const char* p3hip_take_last_error(void) {
    static thread_local std::string held;
    if (!take_error(&held)) return nullptr;
    return held.c_str();
}

int p3hip_malloc(void** dev_ptr, size_t bytes) {
    if (!dev_ptr) return fail(ERR_BAD_ARG, "p3hip_malloc: null out pointer");
    Context* cx;
    int rc = get_context(&cx);
    if (rc) return rc;
    P3_HIP(hipMalloc(dev_ptr, bytes ? bytes : 4));
    return OK;
}
int p3hip_free(void* dev_ptr) {
    if (dev_ptr) P3_HIP(hipFree(dev_ptr));
    return OK;
}
int p3hip_upload(void* dev_dst, const void* host_src, size_t bytes) {
    if (bytes && (!dev_dst || !host_src)) return fail(ERR_BAD_ARG, "p3hip_upload: null pointer");
    if (bytes) P3_HIP(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return OK;
}
int p3hip_download(void* host_dst, const void* dev_src, size_t bytes) {
    if (bytes && (!host_dst || !dev_src)) return fail(ERR_BAD_ARG, "p3hip_download: null pointer");
    if (bytes) P3_HIP(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return OK;
}
int p3hip_sync(void* stream) {
    P3_HIP(hipStreamSynchronize((hipStream_t)stream));
    return OK;
}
void p3hip_release_thread_context(void) { release_thread_contexts(); }

}  // extern "C"

// ---- TwoAdicSubgroupDft ------------------------------------------------------------------------
enum DftOp { OP_DFT, OP_IDFT, OP_COSET_DFT, OP_COSET_LDE };

// BUFFER CONTRACT (include/p3hip.h): an input and an output either coincide or are disjoint.  True when the two ranges share a word
// without starting at the same one: no kernel defines what it reads then, so the entries refuse it before any launch.
static bool partial_overlap(const uint32_t* in, size_t in_words, const uint32_t* out, size_t out_words) {
    if (in == out) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    return a < b + out_words * 4 && b < a + in_words * 4;
}
static bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

static int dft_dev(DftOp op, const uint32_t* d_in, uint32_t* d_out, size_t h, size_t w, unsigned added_bits,
                   uint32_t shift, int br_out, hipStream_t stream) {
    return guarded([&]() -> int {
        if (h == 0 || w == 0) return OK;
        if (!d_in || !d_out) return fail(ERR_BAD_ARG, "null matrix pointer");
        if (w > 0xffffffffull) return fail(ERR_BAD_ARG, "width too large");
        if (shift >= bb::P) return fail(ERR_BAD_ARG, "shift is not a reduced Montgomery word");
        if (partial_overlap(d_in, h * w, d_out, (op == OP_COSET_LDE ? h << added_bits : h) * w))
            return fail(ERR_BAD_ARG, "d_in and d_out overlap without being identical");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        switch (op) {
            case OP_DFT: return ntt_dft(*cx, stream, d_in, d_out, h, (uint32_t)w, false);
            case OP_IDFT: return ntt_dft(*cx, stream, d_in, d_out, h, (uint32_t)w, true);
            case OP_COSET_DFT: return ntt_coset_dft(*cx, stream, d_in, d_out, h, (uint32_t)w, shift);
            default: return ntt_coset_lde(*cx, stream, d_in, d_out, h, (uint32_t)w, added_bits, shift, br_out != 0);
        }
    });
}

// Per-call timing line of the reference's backend (backend_vulkan.rs:1385-1423, log_vulkan_timing :23-39):
//   "vulkan dft: h=.. w=.. stages=.. upload=..ms stages=..ms readback=..ms total=..ms gpu(stage=.. copy_back=.. total=..)"
// Here: "hip dft: ..." with the gpu(...) part from HIP events on the stream.  Written to stderr when
// P3HIP_LOG_TIMING=1 (the reference always logs; a library should not) and always kept as the thread's last line
// (p3hip_last_timing_line), so a host can surface it like the reference's logcat line.
static thread_local std::string g_last_timing;
static bool log_timing_enabled() {
    static const bool on = [] { const char* e = getenv("P3HIP_LOG_TIMING"); return e && atoi(e) != 0; }();
    return on;
}

// host-pointer path: H2D, kernels, D2H, sync (the reference's e2e shape, backend_vulkan.rs:1107-1394)
static int dft_host(DftOp op, const uint32_t* in, uint32_t* out, size_t h, size_t w, unsigned added_bits,
                    uint32_t shift, int br_out) {
    return guarded([&]() -> int {
        if (h == 0 || w == 0) return OK;
        if (!in || !out) return fail(ERR_BAD_ARG, "null matrix pointer");
        if (!is_pow2(h)) return fail(ERR_BAD_ARG, "hip backend requires power-of-two height, got " + std::to_string(h));
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        using clk = std::chrono::steady_clock;
        auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
        const auto t_total = clk::now();
        size_t in_bytes = h * w * 4;
        size_t out_rows = op == OP_COSET_LDE ? (h << added_bits) : h;
        size_t out_bytes = out_rows * w * 4;
        hipStream_t stream = nullptr;
        rc = cx->ws(stream, 2).reserve(in_bytes);
        if (rc) return rc;
        rc = cx->ws(stream, 3).reserve(out_bytes);
        if (rc) return rc;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        for (auto& e : ev) P3_HIP(hipEventCreate(&e));
        auto drop_events = [&] { for (auto& e : ev) if (e) (void)hipEventDestroy(e); };
        const auto t_upload = clk::now();
        if (hipMemcpyAsync(cx->ws(stream, 2).ptr, in, in_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) { drop_events(); return fail(ERR_HIP, "upload failed"); }
        (void)hipEventRecord(ev[0], stream);
        const double upload_ms = ms_since(t_upload);
        const auto t_stages = clk::now();
        rc = dft_dev(op, cx->ws(stream, 2).as<uint32_t>(), cx->ws(stream, 3).as<uint32_t>(), h, w, added_bits, shift, br_out, stream);
        if (rc) { drop_events(); return rc; }
        (void)hipEventRecord(ev[1], stream);
        const double stages_ms = ms_since(t_stages);
        const auto t_read = clk::now();
        if (hipMemcpyAsync(out, cx->ws(stream, 3).ptr, out_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) { drop_events(); return fail(ERR_HIP, "readback failed"); }
        (void)hipEventRecord(ev[2], stream);
        if (hipStreamSynchronize(stream) != hipSuccess) { drop_events(); return fail(ERR_HIP, "synchronise failed"); }
        const double readback_ms = ms_since(t_read), total_ms = ms_since(t_total);
        float g_stage = 0, g_copy = 0, g_total = 0;
        (void)hipEventElapsedTime(&g_stage, ev[0], ev[1]);
        (void)hipEventElapsedTime(&g_copy, ev[1], ev[2]);
        (void)hipEventElapsedTime(&g_total, ev[0], ev[2]);
        drop_events();
        char line[320];
        snprintf(line, sizeof line,
                 "hip dft: op=%s h=%zu w=%zu stages=%u upload=%.3fms stages=%.3fms readback=%.3fms total=%.3fms gpu(stage=%.3fms copy_back=%.3fms total=%.3fms)",
                 op == OP_DFT ? "dft" : op == OP_IDFT ? "idft" : op == OP_COSET_DFT ? "coset_dft" : "coset_lde", h, w,
                 log2u(out_rows), upload_ms, stages_ms, readback_ms, total_ms, g_stage, g_copy, g_total);
        g_last_timing = line;
        if (log_timing_enabled()) fprintf(stderr, "%s\n", line);
        return OK;
    });
}

extern "C" {

const char* p3hip_last_timing_line(void) { return g_last_timing.empty() ? nullptr : g_last_timing.c_str(); }

int p3hip_dft_batch_bb31(const uint32_t* in, uint32_t* out, size_t h, size_t w) {
    return dft_host(OP_DFT, in, out, h, w, 0, bb::ONE, 0);
}
int p3hip_idft_batch_bb31(const uint32_t* in, uint32_t* out, size_t h, size_t w) {
    return dft_host(OP_IDFT, in, out, h, w, 0, bb::ONE, 0);
}
int p3hip_coset_dft_batch_bb31(const uint32_t* in, uint32_t* out, size_t h, size_t w, uint32_t shift) {
    return dft_host(OP_COSET_DFT, in, out, h, w, 0, shift, 0);
}
int p3hip_coset_lde_batch_bb31(const uint32_t* in, uint32_t* out, size_t h, size_t w, unsigned added_bits,
                               uint32_t shift, int br_out) {
    return dft_host(OP_COSET_LDE, in, out, h, w, added_bits, shift, br_out);
}
int p3hip_dft_batch_bb31_dev(const uint32_t* in, uint32_t* out, size_t h, size_t w, void* stream) {
    return dft_dev(OP_DFT, in, out, h, w, 0, bb::ONE, 0, (hipStream_t)stream);
}
int p3hip_idft_batch_bb31_dev(const uint32_t* in, uint32_t* out, size_t h, size_t w, void* stream) {
    return dft_dev(OP_IDFT, in, out, h, w, 0, bb::ONE, 0, (hipStream_t)stream);
}
int p3hip_coset_dft_batch_bb31_dev(const uint32_t* in, uint32_t* out, size_t h, size_t w, uint32_t shift, void* stream) {
    return dft_dev(OP_COSET_DFT, in, out, h, w, 0, shift, 0, (hipStream_t)stream);
}
int p3hip_coset_lde_batch_bb31_dev(const uint32_t* in, uint32_t* out, size_t h, size_t w, unsigned added_bits,
                                   uint32_t shift, int br_out, void* stream) {
    return dft_dev(OP_COSET_LDE, in, out, h, w, added_bits, shift, br_out, (hipStream_t)stream);
}
int p3hip_coset_lde_from_coeffs_bb31_dev(const uint32_t* coeffs, uint32_t* out, size_t h, size_t w, unsigned added_bits,
                                         uint32_t shift, void* stream) {
    return guarded([&]() -> int {
        if (h == 0 || w == 0) return OK;
        if (!coeffs || !out || coeffs == out) return fail(ERR_BAD_ARG, "coset_lde_from_coeffs: null or aliased pointers");
        if (partial_overlap(coeffs, h * w, out, (h << added_bits) * w))
            return fail(ERR_BAD_ARG, "coset_lde_from_coeffs: d_coeffs and d_out overlap without being identical");
        if (w > 0xffffffffull) return fail(ERR_BAD_ARG, "width too large");
        if (shift >= bb::P) return fail(ERR_BAD_ARG, "shift is not a reduced Montgomery word");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        if ((rc = cx->ws(st, 2).reserve(h * w * 4))) return rc;
        return ntt_coset_lde_from_coeffs(*cx, st, coeffs, out, cx->ws(st, 2).as<uint32_t>(), h, (uint32_t)w, added_bits, shift);
    });
}
int p3hip_dft_plan_bb31(size_t height, size_t width, uint32_t* stages_per_pass, size_t cap, size_t* n_passes) {
    return guarded([&]() -> int {
        if (!n_passes) return fail(ERR_BAD_ARG, "dft_plan: null argument");
        *n_passes = 0;
        if (height == 0 || width == 0) return OK;
        if (!is_pow2(height)) return fail(ERR_BAD_ARG, "hip backend requires power-of-two height, got " + std::to_string(height));
        const uint32_t n = log2u(height);
        if (n > bb::TWO_ADICITY) return fail(ERR_BAD_ARG, "height exceeds BabyBear two-adicity");
        const std::vector<uint32_t> d = ntt_dft_plan(n);
        *n_passes = d.size();
        for (size_t i = 0; i < d.size() && i < cap; i++) if (stages_per_pass) stages_per_pass[i] = d[i];
        return OK;
    });
}

int p3hip_mmcs_commit_plan(int hash, int profile, const uint32_t* const* mats, const size_t* heights, const size_t* widths, const size_t* strides,
                           size_t n_mats, const uint32_t* layers, p3hip_mmcs_step* steps, size_t cap, size_t* n_steps) {
    return guarded([&]() -> int {
        if (!n_steps || (cap && !steps)) return fail(ERR_BAD_ARG, "mmcs_commit_plan: null argument");
        *n_steps = 0;
        if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return fail(ERR_BAD_ARG, "mmcs_commit: unknown hash configuration");
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "mmcs_commit_plan: unknown profile");
        if (int rc = mmcs_check_shape(heights, widths, n_mats)) return rc;
        for (size_t i = 0; strides && i < n_mats; i++)
            if (strides[i] < widths[i] || strides[i] > 0xffffffffull) return fail(ERR_BAD_ARG, "mmcs_commit: row stride below the width");
        MmcsPlan plan;
        if (int rc = mmcs_plan(hash, profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY, mats, heights, widths, strides,
                               n_mats, layers, &plan)) return rc;
        *n_steps = plan.n;
        for (size_t i = 0; i < plan.n && i < cap; i++) steps[i] = plan.step[i];
        return OK;
    });
}
const char* p3hip_mmcs_kernel_name(int kernel) { return mmcs_kernel_name(kernel); }

int p3hip_bit_reverse_rows_dev(const uint32_t* in, uint32_t* out, size_t h, size_t w, void* stream) {
    return guarded([&]() -> int {
        if (h == 0 || w == 0) return OK;
        if (!in || !out || in == out) return fail(ERR_BAD_ARG, "bit_reverse_rows: null or aliased pointers");
        if (partial_overlap(in, h * w, out, h * w)) return fail(ERR_BAD_ARG, "bit_reverse_rows: d_in and d_out overlap without being identical");
        return bit_reverse_rows((hipStream_t)stream, in, out, h, (uint32_t)w);
    });
}

// ---- FibonacciAir workload ----------------------------------------------------------------------
int p3hip_fib_trace_dev(uint64_t a, uint64_t b, size_t n, uint32_t* d_out, void* stream) {
    return guarded([&]() -> int {
        if (!n) return OK;
        if (!d_out) return fail(ERR_BAD_ARG, "fib_trace: null output");
        if (misaligned(d_out, 8)) return fail(ERR_BAD_ARG, "fib_trace: d_out must be 8-byte aligned (rows of two words)");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return fib_trace((hipStream_t)stream, a, b, n, d_out);
    });
}

// ---- Poseidon2 ----------------------------------------------------------------------------------
int p3hip_poseidon2_permute_dev(uint32_t* d_states, size_t n, void* stream) {
    return guarded([&]() -> int {
        if (n && !d_states) return fail(ERR_BAD_ARG, "null state pointer");
        if (misaligned(d_states, 4)) return fail(ERR_BAD_ARG, "poseidon2_permute: d_states must be 4-byte aligned");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        // the per-lane forms move a state as four 16-byte pieces: states that are not 16-byte aligned take the 16-lane form, which moves
        // single words (the same words out: tests/test_gpu_permutation_forms.py)
        if (misaligned(d_states, 16)) return poseidon2_permute_states_variant((hipStream_t)stream, d_states, n, 3);
        return poseidon2_permute_states((hipStream_t)stream, d_states, n);
    });
}
int p3hip_poseidon2_permute(uint32_t* states, size_t n) {
    return guarded([&]() -> int {
        if (!n) return OK;
        if (!states) return fail(ERR_BAD_ARG, "null state pointer");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t stream = nullptr;
        rc = cx->ws(stream, 2).reserve(n * 64);
        if (rc) return rc;
        P3_HIP(hipMemcpy(cx->ws(stream, 2).ptr, states, n * 64, hipMemcpyHostToDevice));
        rc = poseidon2_permute_states(stream, cx->ws(stream, 2).as<uint32_t>(), n);
        if (rc) return rc;
        P3_HIP(hipMemcpy(states, cx->ws(stream, 2).ptr, n * 64, hipMemcpyDeviceToHost));
        return OK;
    });
}

// test / diagnostics entries of the two arithmetic forms of the permutation
int p3hip_poseidon2_permute_variant_dev(uint32_t* d_states, size_t n, int variant, void* stream) {
    return guarded([&]() -> int {
        if (n && !d_states) return fail(ERR_BAD_ARG, "null state pointer");
        if (variant < 0 || variant > 3)
            return fail(ERR_BAD_ARG, "poseidon2 variant: 0 = int32, 1 = fp64, 2 = fp64 one state per quad, 3 = int32 one state per 16 lanes");
        if (n > ((size_t)1 << 26)) return fail(ERR_BAD_ARG, "poseidon2 variant: at most 2^26 states per call");
        if (!n) return OK;
        if (misaligned(d_states, variant == 3 ? 4 : 16))
            return fail(ERR_BAD_ARG, "poseidon2 variant: d_states must be 16-byte aligned (4-byte for variant 3)");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return poseidon2_permute_states_variant((hipStream_t)stream, d_states, n, variant);
    });
}
int p3hip_poseidon2_f64_probe_dev(const double* d_in, uint32_t* d_out, size_t n, int mode, void* stream) {
    return guarded([&]() -> int {
        if (n && (!d_in || !d_out)) return fail(ERR_BAD_ARG, "null pointer");
        if (mode < 0 || mode > 3)
            return fail(ERR_BAD_ARG, "probe mode: 0 = permutation, 1 = internal rounds, 2 = reduce, 3 = permutation, one state per quad");
        if (n > ((size_t)1 << 26)) return fail(ERR_BAD_ARG, "probe: at most 2^26 states per call");
        if (!n) return OK;
        if (misaligned(d_in, 8)) return fail(ERR_BAD_ARG, "probe: d_in holds doubles and must be 8-byte aligned");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return poseidon2_f64_probe((hipStream_t)stream, d_in, d_out, n, mode);
    });
}
// test / diagnostics entries of the field primitives, one op per call (field_probe.hip)
int p3hip_field_probe_dev(int op, const void* d_in, void* d_out, size_t n, void* stream) {
    return guarded([&]() -> int { return field_probe((hipStream_t)stream, op, d_in, d_out, n); });
}
int p3hip_field_probe_host(int op, const void* in, void* out, size_t n) {
    return guarded([&]() -> int { return field_probe_host(op, in, out, n); });
}

// ---- Mmcs ---------------------------------------------------------------------------------------
}  // extern "C"
struct p3hip_tree {
    Tree* t;
};
extern "C" {

static int commit_async_kind(int kind, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths,
                             size_t n_mats, p3hip_tree_t** tree_out, void* stream) {
    return guarded([&]() -> int {
        if (!tree_out) return fail(ERR_BAD_ARG, "mmcs_commit: null tree_out");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        Tree* t = nullptr;
        rc = mmcs_commit((hipStream_t)stream, d_mats, heights, widths, n_mats, &t, nullptr, nullptr, kind, nullptr, cx->profile);
        if (rc) return rc;
        *tree_out = new p3hip_tree{t};
        return OK;
    });
}
int p3hip_mmcs_commit_async_dev(const uint32_t* const* d_mats, const size_t* heights, const size_t* widths,
                                size_t n_mats, p3hip_tree_t** tree_out, void* stream) {
    return commit_async_kind(HASH_POSEIDON2, d_mats, heights, widths, n_mats, tree_out, stream);
}
int p3hip_mmcs_commit_hash_dev(int hash, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths,
                               size_t n_mats, uint32_t root_out[8], p3hip_tree_t** tree_out, void* stream) {
    if (!root_out) return fail(ERR_BAD_ARG, "mmcs_commit: null root_out");
    int rc = commit_async_kind(hash, d_mats, heights, widths, n_mats, tree_out, stream);
    if (rc) return rc;
    rc = p3hip_mmcs_root(*tree_out, root_out, stream);
    if (rc) { p3hip_mmcs_free(*tree_out); *tree_out = nullptr; }
    return rc;
}
// commit with CALLER-PROVIDED digest-layer storage (p3hip_mmcs_layer_words(max height) words): nothing is allocated, so
// the call only enqueues (the fib_air prover commits this way into its arena)
size_t p3hip_mmcs_layer_words(size_t max_height) { return mmcs_layer_words(max_height); }
int p3hip_mmcs_commit_into_dev(int hash, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths, size_t n_mats,
                               uint32_t* d_layers, p3hip_tree_t** tree_out, void* stream) {
    return guarded([&]() -> int {
        if (!tree_out || !d_layers) return fail(ERR_BAD_ARG, "mmcs_commit_into: null argument");
        if (misaligned(d_layers, 16)) return fail(ERR_BAD_ARG, "mmcs_commit_into: d_layers must be 16-byte aligned (digests move as 16-byte pieces)");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        Tree* t = nullptr;
        rc = mmcs_commit((hipStream_t)stream, d_mats, heights, widths, n_mats, &t, d_layers, nullptr, hash, nullptr, cx->profile);
        if (rc) return rc;
        *tree_out = new p3hip_tree{t};
        return OK;
    });
}
int p3hip_keccak_f_dev(uint64_t* d_states, size_t n, void* stream) {
    return guarded([&]() -> int {
        if (!d_states && n) return fail(ERR_BAD_ARG, "keccak_f: null states");
        if (misaligned(d_states, 8)) return fail(ERR_BAD_ARG, "keccak_f: d_states must be 8-byte aligned (u64 lanes)");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return keccak_f_states((hipStream_t)stream, d_states, n);
    });
}
// test / diagnostics entries of the three formulations of Keccak-f and of the compression layers' production kernels
int p3hip_keccak_f_variant_dev(uint64_t* d_states, size_t n, int variant, void* stream) {
    return guarded([&]() -> int {
        if (!d_states && n) return fail(ERR_BAD_ARG, "keccak_f variant: null states");
        if (misaligned(d_states, 8)) return fail(ERR_BAD_ARG, "keccak_f variant: d_states must be 8-byte aligned (u64 lanes)");
        if (variant < 0 || variant > 2) return fail(ERR_BAD_ARG, "keccak_f variant: 0 = permute, 1 = permute_digest, 2 = f_coop");
        if (n > ((size_t)1 << 24)) return fail(ERR_BAD_ARG, "keccak_f variant: at most 2^24 states per call");
        if (!n) return OK;
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return keccak_f_states_variant((hipStream_t)stream, d_states, n, variant);
    });
}
int p3hip_compress_layer_variant_dev(int hash, int variant, const uint32_t* d_in, uint32_t* d_out, size_t n_out, void* stream) {
    return guarded([&]() -> int {
        int rc = compress_layer_variant_check(hash, variant, d_in, d_out, n_out);  // refused before the thread's device context is looked up
        if (rc || !n_out) return rc;
        Context* cx;
        rc = get_context(&cx);
        if (rc) return rc;
        return compress_layer_variant((hipStream_t)stream, hash, variant, d_in, d_out, n_out);
    });
}
int p3hip_mmcs_root(const p3hip_tree_t* tree, uint32_t root_out[8], void* stream) {
    return guarded([&]() -> int {
        if (!tree || !root_out) return fail(ERR_BAD_ARG, "mmcs_root: null argument");
        return mmcs_root((hipStream_t)stream, *tree->t, root_out);
    });
}
int p3hip_mmcs_commit_dev(const uint32_t* const* d_mats, const size_t* heights, const size_t* widths,
                          size_t n_mats, uint32_t root_out[8], p3hip_tree_t** tree_out, void* stream) {
    if (!root_out) return fail(ERR_BAD_ARG, "mmcs_commit: null root_out");
    int rc = p3hip_mmcs_commit_async_dev(d_mats, heights, widths, n_mats, tree_out, stream);
    if (rc) return rc;
    rc = p3hip_mmcs_root(*tree_out, root_out, stream);
    if (rc) { p3hip_mmcs_free(*tree_out); *tree_out = nullptr; }
    return rc;
}
size_t p3hip_mmcs_log_max_height(const p3hip_tree_t* tree) { return tree ? tree->t->log_max_height : 0; }
size_t p3hip_mmcs_num_layers(const p3hip_tree_t* tree) { return tree ? tree->t->layer_len.size() : 0; }
const uint32_t* p3hip_mmcs_layer_dev(const p3hip_tree_t* tree, size_t layer, size_t* len_out) {
    if (!tree || layer >= tree->t->layer_len.size()) return nullptr;
    if (len_out) *len_out = tree->t->layer_len[layer];
    return tree->t->layers + tree->t->layer_off[layer];
}
int p3hip_mmcs_open_batch(const p3hip_tree_t* tree, size_t index, uint32_t* rows_out, uint32_t* path_out,
                          void* stream) {
    return guarded([&]() -> int {
        if (!tree) return fail(ERR_BAD_ARG, "mmcs_open_batch: null tree");
        size_t row_words = 0;
        for (size_t w : tree->t->widths) row_words += w;
        if ((row_words && !rows_out) || (tree->t->log_max_height && !path_out))
            return fail(ERR_BAD_ARG, "mmcs_open_batch: null output buffer");
        return mmcs_open((hipStream_t)stream, *tree->t, index, rows_out, path_out);
    });
}
// Mmcs::verify_batch, host code (mmcs_verify.hip): no device context is touched
int p3hip_mmcs_verify_batch(int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats, size_t index,
                            const uint32_t* rows, const uint32_t* path, size_t path_len) {
    return guarded([&]() -> int {
        std::string why;
        int rc = mmcs_verify_batch(hash, root, heights, widths, n_mats, index, rows, path, path_len, &why);
        if (rc != 0) set_error(why);
        return rc;
    });
}
size_t p3hip_mmcs_row_words(const p3hip_tree_t* tree) { return tree ? mmcs_row_words(*tree->t) : 0; }
int p3hip_mmcs_open_batch_many_dev(const p3hip_tree_t* tree, const uint32_t* d_indices, size_t n, uint32_t* d_rows, uint32_t* d_paths,
                                   void* stream) {
    return guarded([&]() -> int {
        if (!tree) return fail(ERR_BAD_ARG, "mmcs_open_batch_many: null tree");
        return mmcs_open_many((hipStream_t)stream, *tree->t, d_indices, n, d_rows, d_paths);
    });
}
int p3hip_mmcs_verify_batch_many_form_dev(int form, int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats,
                                          const uint32_t* d_indices, size_t n, const uint32_t* d_rows, const uint32_t* d_paths,
                                          uint32_t* d_status, uint32_t* d_rejected, void* stream) {
    return guarded([&]() -> int {
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        return mmcs_verify_many((hipStream_t)stream, hash, root, heights, widths, n_mats, d_indices, n, d_rows, d_paths, d_status, d_rejected,
                                form, cx->profile);
    });
}
int p3hip_mmcs_verify_batch_many_dev(int hash, const uint32_t root[8], const size_t* heights, const size_t* widths, size_t n_mats,
                                     const uint32_t* d_indices, size_t n, const uint32_t* d_rows, const uint32_t* d_paths,
                                     uint32_t* d_status, uint32_t* d_rejected, void* stream) {
    return p3hip_mmcs_verify_batch_many_form_dev(MMCS_FORM_AUTO, hash, root, heights, widths, n_mats, d_indices, n, d_rows, d_paths, d_status,
                                                 d_rejected, stream);
}
size_t p3hip_mmcs_verify_coop_max(int hash, int profile) {
    if ((hash != HASH_POSEIDON2 && hash != HASH_KECCAK) || (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY)) return 0;
    return mmcs_verify_coop_max(hash, profile == P3HIP_PROFILE_LATENCY ? PROFILE_LATENCY : PROFILE_THROUGHPUT);
}
void p3hip_mmcs_free(p3hip_tree_t* tree) {
    if (!tree) return;
    delete tree->t;
    delete tree;
}
int p3hip_mmcs_commit(const uint32_t* const* mats, const size_t* heights, const size_t* widths, size_t n_mats,
                      uint32_t root_out[8], p3hip_tree_t** tree_out) {
    return p3hip_mmcs_commit_hash(HASH_POSEIDON2, mats, heights, widths, n_mats, root_out, tree_out);
}
int p3hip_mmcs_commit_hash(int hash, const uint32_t* const* mats, const size_t* heights, const size_t* widths, size_t n_mats,
                           uint32_t root_out[8], p3hip_tree_t** tree_out) {
    return guarded([&]() -> int {
        if (!mats || !heights || !widths || !n_mats || !root_out || !tree_out)
            return fail(ERR_BAD_ARG, "mmcs_commit: null/empty argument");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        std::vector<void*> owned;
        std::vector<const uint32_t*> dptr;
        auto cleanup = [&]() { for (void* p : owned) (void)hipFree(p); };
        for (size_t i = 0; i < n_mats; i++) {
            size_t bytes = heights[i] * widths[i] * 4;
            void* d = nullptr;
            if (hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) { cleanup(); return fail(ERR_HIP, "hipMalloc failed"); }
            owned.push_back(d);
            if (bytes && hipMemcpy(d, mats[i], bytes, hipMemcpyHostToDevice) != hipSuccess) { cleanup(); return fail(ERR_HIP, "hipMemcpy failed"); }
            dptr.push_back((const uint32_t*)d);
        }
        rc = p3hip_mmcs_commit_hash_dev(hash, dptr.data(), heights, widths, n_mats, root_out, tree_out, nullptr);
        if (rc) { cleanup(); return rc; }
        (*tree_out)->t->owned = owned;
        return OK;
    });
}

}  // extern "C"

// ---- fib_air prover (p3_uni_stark::prove as driven by native/src/fib_air.rs:60-70) ---------------
// ---- a caller's trace (prove(&config, &FibonacciAir{}, trace, &pis), fib_air.rs:61,68-70): the checks every entry makes before
// anything is launched, and the optional check_constraints pass ----
// d_trace must be device memory of `device` (hipPointerGetAttributes) holding `rows` rows of two words from d_trace on
static int check_device_trace(const uint32_t* d_trace, uint64_t rows, int device, const std::string& who) {
    if (!d_trace) return fail(ERR_BAD_ARG, who + ": null trace");
    if (misaligned(d_trace, 8)) return fail(ERR_BAD_ARG, who + ": the trace must be 8-byte aligned (rows of two words)");
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, d_trace) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ERR_BAD_ARG, who + ": the trace is not device memory");
    }
    if (attr.type != hipMemoryTypeDevice) return fail(ERR_BAD_ARG, who + ": the trace is not device memory");
    if (attr.device != device)
        return fail(ERR_BAD_ARG, who + ": the trace is on device " + std::to_string(attr.device) + ", the work on device " + std::to_string(device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_trace) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ERR_BAD_ARG, who + ": the trace's allocation is unknown");
    }
    const uint64_t off = (uint64_t)((const char*)d_trace - (const char*)base);
    if (off > size || (size - off) / 8 < rows)
        return fail(ERR_BAD_ARG, who + ": the trace's allocation holds fewer than " + std::to_string(rows) + " rows");
    return OK;
}
static int check_pis_flags(const uint32_t* pis, unsigned flags, const std::string& who) {
    if (!pis) return fail(ERR_BAD_ARG, who + ": null public values");
    for (int k = 0; k < 3; k++)
        if (pis[k] >= bb::P) return fail(ERR_BAD_ARG, who + ": public value " + std::to_string(k) + " is not a field element (>= P)");
    if (flags & ~P3HIP_PROVE_CHECK_TRACE) return fail(ERR_BAD_ARG, who + ": unknown flag bits");
    return OK;
}
// P3HIP_PROVE_CHECK_TRACE: check_constraints on the prover's stream first (upstream's debug builds, p3_uni_stark::prove);
// then the proof.  A trace that breaks a rule is refused with upstream's panic text.
template <class Prover>
static int prove_trace_with(Prover& pr, const uint32_t* d_trace, const uint32_t* pis, unsigned flags, std::vector<uint8_t>* out) {
    if (flags & P3HIP_PROVE_CHECK_TRACE) {
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        if (cx->device != pr.device())
            return fail(ERR_BAD_ARG, "fib prover: created on device " + std::to_string(pr.device()) + ", current device is " + std::to_string(cx->device));
        TraceCheck c;
        if ((rc = fib_check_trace(*cx, pr.stream(), d_trace, 1ull << pr.log_n(), pis, &c))) return rc;
        if (c.first_bad_row >= 0) {
            char tail[96];
            snprintf(tail, sizeof tail, " (rules broken: mask 0x%x; %llu bad rows)", c.mask, (unsigned long long)c.bad_rows);
            return fail(ERR_BAD_ARG, "constraints had nonzero value on row " + std::to_string(c.first_bad_row) + tail);
        }
    }
    return pr.prove_trace(d_trace, pis, out);
}

struct p3hip_fib_prover {
    std::unique_ptr<FibProver> plain;         // TwoAdicFriPcs + MerkleTreeMmcs
    std::unique_ptr<FibHidingProver> hiding;  // HidingFriPcs + MerkleTreeHidingMmcs (fib_air.rs:40-65)
    std::vector<uint8_t> last;
    size_t proof_len = 0;  // length of this prover's proofs, known once one has SUCCEEDED (0 before); never read from `last`
    int prove(uint64_t a, uint64_t b) {
        int rc = hiding ? hiding->prove(a, b, &last) : plain->prove(a, b, &last);
        if (rc) last.clear();  // a failed proof leaves nothing behind that could be mistaken for one
        else proof_len = last.size();
        return rc;
    }
    int prove_trace(const uint32_t* d_trace, const uint32_t* pis, unsigned flags) {
        int rc = hiding ? prove_trace_with(*hiding, d_trace, pis, flags, &last) : prove_trace_with(*plain, d_trace, pis, flags, &last);
        if (rc) last.clear();
        else proof_len = last.size();
        return rc;
    }
    int device() const { return hiding ? hiding->device() : plain->device(); }
    uint32_t log_n() const { return hiding ? hiding->log_n() : plain->log_n(); }
    hipStream_t stream() const { return hiding ? hiding->stream() : plain->stream(); }
    uint32_t* arena_trace() const { return hiding ? hiding->arena_trace() : plain->arena_trace(); }
};

extern "C" {

int p3hip_set_thread_profile(int profile) {
    return guarded([&]() -> int {
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "set_thread_profile: unknown profile");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        cx->profile = profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY;
        return OK;
    });
}
int p3hip_get_thread_profile(void) {
    Context* cx;
    if (get_context(&cx)) return -1;
    return cx->profile == PROFILE_THROUGHPUT ? P3HIP_PROFILE_THROUGHPUT : P3HIP_PROFILE_LATENCY;
}

int p3hip_fib_prover_create_profile(int profile, int hash, int hiding, uint64_t seed, unsigned log_n, const p3hip_fri_params_t* params,
                                    void* stream, int own_stream, p3hip_fib_prover_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "fib_prover_create: null argument");
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "fib_prover_create: unknown profile");
        const int prof = profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY;
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        bool own = false;
        if (own_stream) {
            P3_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            own = true;
        }
        std::unique_ptr<p3hip_fib_prover> p(new p3hip_fib_prover());
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        // on failure the prover's destructor destroys the owned stream
        if (hiding) {
            p->hiding.reset(new FibHidingProver());
            rc = p->hiding->init(log_n, fp, st, own, hash, seed, prof);
        } else {
            p->plain.reset(new FibProver());
            rc = p->plain->init(log_n, fp, st, own, hash, prof);
        }
        if (rc) return rc;
        *out = p.release();
        return OK;
    });
}
// a prover created on its own proves one proof at a time (what the reference does, fib_air.rs:56-72): the latency profile
int p3hip_fib_prover_create(unsigned log_n, const p3hip_fri_params_t* params, void* stream, int own_stream,
                            p3hip_fib_prover_t** out) {
    return p3hip_fib_prover_create_profile(P3HIP_PROFILE_LATENCY, HASH_POSEIDON2, 0, 0, log_n, params, stream, own_stream, out);
}
int p3hip_fib_prover_create_hash(int hash, unsigned log_n, const p3hip_fri_params_t* params, void* stream, int own_stream,
                                 p3hip_fib_prover_t** out) {
    return p3hip_fib_prover_create_profile(P3HIP_PROFILE_LATENCY, hash, 0, 0, log_n, params, stream, own_stream, out);
}

int p3hip_fib_prover_prove(p3hip_fib_prover_t* prover, uint64_t a, uint64_t b, const uint8_t** proof_out,
                           size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "fib_prover_prove: null argument");
        int rc = prover->prove(a, b);
        if (rc) return rc;
        *proof_out = prover->last.data();
        *proof_len = prover->last.size();
        return OK;
    });
}

int p3hip_fib_prover_prove_into(p3hip_fib_prover_t* prover, uint64_t a, uint64_t b, uint8_t* out, size_t cap, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !out || !proof_len) return fail(ERR_BAD_ARG, "fib_prover_prove_into: null argument");
        // proofs of one prover have one length: once it is known, a buffer that cannot hold it fails BEFORE any work is queued
        // (the length is a field of its own, set by a proof that succeeded: `last` may be empty or stale after a failure)
        if (prover->proof_len && prover->proof_len > cap) {
            *proof_len = prover->proof_len;
            return fail(ERR_BAD_ARG, "fib_prover_prove_into: the proof needs " + std::to_string(prover->proof_len) + " bytes");
        }
        int rc = prover->prove(a, b);
        if (rc) return rc;
        *proof_len = prover->last.size();
        if (prover->last.size() > cap) return fail(ERR_BAD_ARG, "fib_prover_prove_into: the proof needs " + std::to_string(prover->last.size()) + " bytes");
        memcpy(out, prover->last.data(), prover->last.size());
        return OK;
    });
}

int p3hip_fib_prover_enqueue(p3hip_fib_prover_t* prover, uint64_t a, uint64_t b) {
    return guarded([&]() -> int {
        if (!prover) return fail(ERR_BAD_ARG, "fib_prover_enqueue: null argument");
        if (!prover->plain) return fail(ERR_BAD_ARG, "fib_prover_enqueue: the hiding prover proves one proof at a time");
        return prover->plain->enqueue(a, b);
    });
}
int p3hip_fib_prover_finish(p3hip_fib_prover_t* prover, const uint8_t** proof_out, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "fib_prover_finish: null argument");
        if (!prover->plain) return fail(ERR_BAD_ARG, "fib_prover_finish: the hiding prover proves one proof at a time");
        int rc = prover->plain->finish(&prover->last);
        if (rc) { prover->last.clear(); return rc; }
        prover->proof_len = prover->last.size();
        *proof_out = prover->last.data();
        *proof_len = prover->last.size();
        return OK;
    });
}

int p3hip_fib_check_trace_dev(const uint32_t* d_trace, size_t n, const uint32_t pis[3], p3hip_trace_check_t* out, void* stream) {
    return guarded([&]() -> int {
        if (!out || !pis) return fail(ERR_BAD_ARG, "fib_check_trace: null argument");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        if (!n) { *out = p3hip_trace_check_t{-1, 0, 0}; return OK; }
        if ((rc = check_device_trace(d_trace, n, cx->device, "fib_check_trace"))) return rc;
        if ((rc = check_pis_flags(pis, 0, "fib_check_trace"))) return rc;
        TraceCheck c;
        if ((rc = fib_check_trace(*cx, (hipStream_t)stream, d_trace, n, pis, &c))) return rc;
        *out = p3hip_trace_check_t{c.first_bad_row, c.mask, c.bad_rows};
        return OK;
    });
}

int p3hip_fib_prover_prove_trace_dev(p3hip_fib_prover_t* prover, const uint32_t* d_trace, const uint32_t pis[3], unsigned flags,
                                     const uint8_t** proof_out, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "fib_prover_prove_trace_dev: null argument");
        int rc = check_pis_flags(pis, flags, "fib_prover_prove_trace_dev");
        if (rc) return rc;
        if ((rc = check_device_trace(d_trace, 1ull << prover->log_n(), prover->device(), "fib_prover_prove_trace_dev"))) return rc;
        if ((rc = prover->prove_trace(d_trace, pis, flags))) return rc;
        *proof_out = prover->last.data();
        *proof_len = prover->last.size();
        return OK;
    });
}
int p3hip_fib_prover_prove_trace(p3hip_fib_prover_t* prover, const uint32_t* host_trace, size_t n, const uint32_t pis[3], unsigned flags,
                                 const uint8_t** proof_out, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !host_trace || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "fib_prover_prove_trace: null argument");
        int rc = check_pis_flags(pis, flags, "fib_prover_prove_trace");
        if (rc) return rc;
        if (n != (1ull << prover->log_n()))
            return fail(ERR_BAD_ARG, "fib_prover_prove_trace: n = " + std::to_string(n) + " rows, the prover proves 2^" + std::to_string(prover->log_n()));
        if (prover->plain && prover->plain->has_pending())
            return fail(ERR_BAD_ARG, "fib prover: finish the enqueued proofs before a synchronous prove");
        Context* cx;
        if ((rc = get_context(&cx))) return rc;
        if (cx->device != prover->device())
            return fail(ERR_BAD_ARG, "fib prover: created on device " + std::to_string(prover->device()) + ", current device is " + std::to_string(cx->device));
        // into the arena's trace slot, on the prover's stream: ordered before everything of the proof that reads it
        P3_HIP(hipMemcpyAsync(prover->arena_trace(), host_trace, (size_t)n * 8, hipMemcpyHostToDevice, prover->stream()));
        if ((rc = prover->prove_trace(prover->arena_trace(), pis, flags))) return rc;
        *proof_out = prover->last.data();
        *proof_len = prover->last.size();
        return OK;
    });
}
int p3hip_fib_prover_enqueue_trace_dev(p3hip_fib_prover_t* prover, const uint32_t* d_trace, const uint32_t pis[3]) {
    return guarded([&]() -> int {
        if (!prover) return fail(ERR_BAD_ARG, "fib_prover_enqueue_trace_dev: null argument");
        if (!prover->plain) return fail(ERR_BAD_ARG, "fib_prover_enqueue_trace_dev: the hiding prover proves one proof at a time");
        int rc = check_pis_flags(pis, 0, "fib_prover_enqueue_trace_dev");
        if (rc) return rc;
        if ((rc = check_device_trace(d_trace, 1ull << prover->log_n(), prover->device(), "fib_prover_enqueue_trace_dev"))) return rc;
        return prover->plain->enqueue_trace(d_trace, pis);
    });
}

int p3hip_fib_prover_stage_times(p3hip_fib_prover_t* prover, double out_ms[6], uint64_t* proofs, int reset) {
    if (!prover || !out_ms) return fail(ERR_BAD_ARG, "fib_prover_stage_times: null argument");
    if (!prover->plain) return fail(ERR_BAD_ARG, "fib_prover_stage_times: not kept by the hiding prover");
    const StageTimes& t = prover->plain->times();
    out_ms[0] = t.trace_commit_ms; out_ms[1] = t.quotient_commit_ms; out_ms[2] = t.open_ms;
    out_ms[3] = t.fri_commit_ms; out_ms[4] = t.grind_ms; out_ms[5] = t.query_ms;
    if (proofs) *proofs = t.proofs;
    if (reset) prover->plain->reset_times();
    return OK;
}

int p3hip_fib_prover_grind_miss_probe(p3hip_fib_prover_t* prover, uint64_t* misses, uint32_t* indices_out, size_t cap, size_t* n_out) {
    if (!prover || !misses) return fail(ERR_BAD_ARG, "fib_prover_grind_miss_probe: null argument");
    if (!prover->plain) return fail(ERR_BAD_ARG, "fib_prover_grind_miss_probe: not kept by the hiding prover");
    std::vector<uint32_t> idx;
    *misses = prover->plain->grind_misses(&idx);
    if (n_out) *n_out = idx.size();
    if (indices_out) for (size_t i = 0; i < idx.size() && i < cap; i++) indices_out[i] = idx[i];
    return OK;
}

void p3hip_fib_prover_destroy(p3hip_fib_prover_t* prover) { delete prover; }

int p3hip_fib_prover_create_hiding(int hash, unsigned log_n, const p3hip_fri_params_t* params, uint64_t seed, void* stream,
                                   int own_stream, p3hip_fib_prover_t** out) {
    return p3hip_fib_prover_create_profile(P3HIP_PROFILE_LATENCY, hash, 1, seed, log_n, params, stream, own_stream, out);
}
int p3hip_verify_fib_air_hiding(int hash, const uint8_t* proof, size_t len, uint64_t a, uint64_t b, uint64_t x, unsigned log_n,
                                const p3hip_fri_params_t* params) {
    return guarded([&]() -> int {
        if (!proof || !params) return fail(ERR_BAD_ARG, "verify_fib_air_hiding: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        int rc = verify_fib_air_hiding(proof, len, a, b, x, log_n, fp, &why, hash);
        if (rc != 0) set_error("fib_air verification failed: " + why);
        return rc;
    });
}

// ---- SmallRng::seed_from_u64 streams on the device (rng.hip) ----
}  // extern "C"
struct p3hip_rng {
    DevRng* d = nullptr;
    uint32_t* err = nullptr;
    DevBuf ws;
    ~p3hip_rng() { if (d) (void)hipFree(d); }
};
extern "C" {
int p3hip_rng_create(uint64_t seed, p3hip_rng_t** out) {
    return guarded([&]() -> int {
        if (!out) return fail(ERR_BAD_ARG, "rng_create: null argument");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        std::unique_ptr<p3hip_rng> r(new p3hip_rng());
        P3_HIP(hipMalloc(reinterpret_cast<void**>(&r->d), sizeof(DevRng) + 16));
        r->err = reinterpret_cast<uint32_t*>(r->d + 1);
        uint64_t s[6] = {0, 0, 0, 0, 0, 0};
        rng_seed_from_u64(s, seed);
        P3_HIP(hipMemcpy(r->d, s, sizeof(DevRng) + 16, hipMemcpyHostToDevice));
        *out = r.release();
        return OK;
    });
}
int p3hip_rng_fill_field_dev(p3hip_rng_t* rng, uint32_t* d_out, size_t n, void* stream) {
    return guarded([&]() -> int {
        if (!rng || (n && !d_out)) return fail(ERR_BAD_ARG, "rng_fill_field: null argument");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        size_t words = 0;
        if ((rc = rng_workspace_words(n, &words))) return rc;
        if ((rc = rng->ws.reserve(words * 4))) return rc;
        return rng_fill_field(*cx, (hipStream_t)stream, rng->d, d_out, n, rng->ws.as<uint32_t>(), rng->err);
    });
}
int p3hip_rng_state(p3hip_rng_t* rng, uint64_t state_out[4], void* stream) {
    return guarded([&]() -> int {
        if (!rng || !state_out) return fail(ERR_BAD_ARG, "rng_state: null argument");
        uint64_t s[6];
        P3_HIP(hipMemcpyAsync(s, rng->d, sizeof(DevRng) + 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
        P3_HIP(hipStreamSynchronize((hipStream_t)stream));
        memcpy(state_out, s, 32);
        if ((uint32_t)s[4] != 0) return fail(ERR_INTERNAL, "rng: a fill ran out of raw draws");
        return OK;
    });
}
void p3hip_rng_destroy(p3hip_rng_t* rng) { delete rng; }

// MerkleTreeHidingMmcs::commit (fib_air.rs:40-51): every matrix is paired with a height x SALT_ELEMS matrix of draws
// from the MMCS's rng; leaf rows are m0 || s0 || m1 || s1 ...  The salt matrices live in HBM and belong to the tree.
int p3hip_mmcs_commit_hiding_dev(int hash, const uint32_t* const* d_mats, const size_t* heights, const size_t* widths, size_t n_mats,
                                 p3hip_rng_t* rng, uint32_t root_out[8], p3hip_tree_t** tree_out, void* stream) {
    return guarded([&]() -> int {
        if (!d_mats || !heights || !widths || !n_mats || !rng || !root_out || !tree_out) return fail(ERR_BAD_ARG, "mmcs_commit_hiding: null/empty argument");
        if (n_mats > 32) return fail(ERR_BAD_ARG, "mmcs_commit_hiding: at most 32 matrices per commitment");
        constexpr size_t SALT = 4;
        std::vector<void*> owned;
        auto cleanup = [&]() { for (void* p : owned) (void)hipFree(p); };
        std::vector<const uint32_t*> mp;
        std::vector<size_t> hh, ww;
        // the salted shape is refused here, before a salt is drawn: a refused commit leaves the rng's stream where it was
        for (size_t i = 0; i < n_mats; i++) { hh.insert(hh.end(), {heights[i], heights[i]}); ww.insert(ww.end(), {widths[i], SALT}); }
        if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return fail(ERR_BAD_ARG, "mmcs_commit: unknown hash configuration");
        if (int rc = mmcs_check_shape(hh.data(), ww.data(), hh.size())) return rc;
        hh.clear(); ww.clear();
        for (size_t i = 0; i < n_mats; i++) {
            void* salt = nullptr;
            if (hipMalloc(&salt, heights[i] * SALT * 4 + 16) != hipSuccess) { cleanup(); return fail(ERR_HIP, "hipMalloc failed"); }
            owned.push_back(salt);
            int rc = p3hip_rng_fill_field_dev(rng, (uint32_t*)salt, heights[i] * SALT, stream);
            if (rc) { cleanup(); return rc; }
            mp.push_back(d_mats[i]); hh.push_back(heights[i]); ww.push_back(widths[i]);
            mp.push_back((const uint32_t*)salt); hh.push_back(heights[i]); ww.push_back(SALT);
        }
        int rc = p3hip_mmcs_commit_hash_dev(hash, mp.data(), hh.data(), ww.data(), mp.size(), root_out, tree_out, stream);
        if (rc) { cleanup(); return rc; }
        (*tree_out)->t->owned = owned;
        return OK;
    });
}

int p3hip_verify_fib_air(const uint8_t* proof, size_t len, uint64_t a, uint64_t b, uint64_t x, unsigned log_n,
                         const p3hip_fri_params_t* params) {
    return p3hip_verify_fib_air_hash(HASH_POSEIDON2, proof, len, a, b, x, log_n, params);
}
int p3hip_verify_fib_air_hash(int hash, const uint8_t* proof, size_t len, uint64_t a, uint64_t b, uint64_t x, unsigned log_n,
                              const p3hip_fri_params_t* params) {
    return guarded([&]() -> int {
        if (!proof || !params) return fail(ERR_BAD_ARG, "verify_fib_air: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        int rc = verify_fib_air(proof, len, a, b, x, log_n, fp, &why, hash);
        if (rc != 0) set_error("fib_air verification failed: " + why);
        return rc;
    });
}

}  // extern "C"

// ---- batches of independent proofs (BASELINE configs[3]): a pool of provers, one host thread + stream each ----
struct p3hip_fib_batch {
    unsigned log_n = 0;
    int hash = HASH_POSEIDON2;
    int device = 0;  // the creator's current device: HIP's current device is per thread and defaults to 0
    FriParams fp{};
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    // Batches in submit order.  A worker takes the next unproved instance of the OLDEST batch that still has one, so a
    // prover that has finished its share of one batch starts on the next at once (no join between batches).
    struct Job {
        uint64_t ticket = 0;
        std::vector<uint64_t> a, b;           // instances (a[i], b[i]); a.size() is the batch's size
        std::vector<const uint32_t*> traces;  // or callers' device traces (prove_traces): then a, b are unused zeros
        std::vector<uint32_t> pis;            // 3 per trace
        unsigned flags = 0;
        size_t next = 0, done = 0;
        std::vector<std::vector<uint8_t>> proofs;
        int first_error = 0;
        std::string error_text;
    };
    std::deque<std::shared_ptr<Job>> jobs;   // submitted, not yet collected
    std::shared_ptr<Job> collected;          // the proofs handed out by the last collect stay alive until the next one
    uint64_t next_ticket = 1;
    bool stop = false;
    size_t ready = 0;
    int first_error = 0;  // of the workers' start-up
    std::string error_text;
    static constexpr size_t MAX_INFLIGHT = 8;

    bool hiding = false;  // provers of the reference's hiding configuration (every one seeded with `seed`, as a fresh
    uint64_t seed = 1;    // config per proof would be: fib_air.rs:50,65)
    int profile = PROFILE_THROUGHPUT;  // several provers share the chip; a pool of ONE prover is a lone prover: latency
    void worker_main() {
        if (hiding) {
            FibHidingProver prover;
            worker_loop(prover, [&](hipStream_t st) { return prover.init(log_n, fp, st, true, hash, seed, profile); });
        } else {
            FibProver prover;
            worker_loop(prover, [&](hipStream_t st) { return prover.init(log_n, fp, st, true, hash, profile); });
        }  // the prover (arena, stream) is gone before the thread's tables and scratch are freed
        release_thread_contexts();
    }
    // a std::thread whose function throws calls std::terminate: every failure becomes first_error instead
    template <class F>
    static int no_throw(F&& f) {
        try { return f(); }
        catch (const std::exception& e) { return fail(ERR_INTERNAL, std::string("exception: ") + e.what()); }
        catch (...) { return fail(ERR_INTERNAL, "unknown exception"); }
    }
    std::shared_ptr<Job> pick(size_t* index) {  // under mu
        for (auto& j : jobs)
            if (j->next < j->a.size()) { *index = j->next++; return j; }
        return nullptr;
    }
    template <class Prover, class Init>
    void worker_loop(Prover& prover, Init&& init) {
        int rc = no_throw([&]() -> int {
            if (hipSetDevice(device) != hipSuccess) return fail(ERR_HIP, "hipSetDevice failed in a batch worker");
            int r = get_context_status();
            if (r) return r;
            hipStream_t st = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(ERR_HIP, "hipStreamCreateWithFlags failed");
            return init(st);
        });
        std::string start_text;
        if (rc != OK) take_error(&start_text);
        {
            std::unique_lock<std::mutex> lk(mu);
            if (rc != OK && first_error == 0) { first_error = rc; error_text = start_text; }
            ready++;
            cv_done.notify_all();
        }
        for (;;) {
            std::shared_ptr<Job> job;
            size_t i = 0;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || (job = pick(&i)) != nullptr; });
                if (!job) return;  // stop
            }
            int prc = rc;
            std::string text = start_text;
            if (prc == OK) {
                prc = no_throw([&]() -> int {
                    if (!job->traces.empty()) return prove_trace_with(prover, job->traces[i], &job->pis[3 * i], job->flags, &job->proofs[i]);
                    return prover.prove(job->a[i], job->b[i], &job->proofs[i]);
                });
                if (prc != OK) take_error(&text);
            }
            {
                std::unique_lock<std::mutex> lk(mu);
                if (prc != OK && job->first_error == 0) { job->first_error = prc; job->error_text = text; }
                if (++job->done == job->a.size()) cv_done.notify_all();
            }
        }
    }
    static int get_context_status() { Context* cx; return get_context(&cx); }
};

extern "C" {

int p3hip_fib_batch_create(unsigned log_n, const p3hip_fri_params_t* params, unsigned n_provers, p3hip_fib_batch_t** out) {
    return p3hip_fib_batch_create_hash(HASH_POSEIDON2, log_n, params, n_provers, out);
}
static int fib_batch_create(int hash, unsigned log_n, const p3hip_fri_params_t* params, unsigned n_provers, bool hiding,
                            uint64_t seed, p3hip_fib_batch_t** out);
int p3hip_fib_batch_create_hash(int hash, unsigned log_n, const p3hip_fri_params_t* params, unsigned n_provers,
                                p3hip_fib_batch_t** out) {
    return fib_batch_create(hash, log_n, params, n_provers, false, 1, out);
}
int p3hip_fib_batch_create_hiding(int hash, unsigned log_n, const p3hip_fri_params_t* params, uint64_t seed, unsigned n_provers,
                                  p3hip_fib_batch_t** out) {
    return fib_batch_create(hash, log_n, params, n_provers, true, seed, out);
}
static int fib_batch_create(int hash, unsigned log_n, const p3hip_fri_params_t* params, unsigned n_provers, bool hiding,
                            uint64_t seed, p3hip_fib_batch_t** out) {
    return guarded([&]() -> int {
        if (!params || !out || n_provers == 0 || n_provers > 64) return fail(ERR_BAD_ARG, "fib_batch_create: bad argument");
        if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return fail(ERR_BAD_ARG, "fib_batch_create: unknown hash configuration");
        std::unique_ptr<p3hip_fib_batch> bt(new p3hip_fib_batch());
        bt->log_n = log_n;
        bt->hash = hash;
        bt->hiding = hiding; bt->seed = seed;
        bt->profile = n_provers > 1 ? PROFILE_THROUGHPUT : PROFILE_LATENCY;
        P3_HIP(hipGetDevice(&bt->device));
        bt->fp = FriParams{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        for (unsigned t = 0; t < n_provers; t++) bt->workers.emplace_back([p = bt.get()] { p->worker_main(); });
        {
            std::unique_lock<std::mutex> lk(bt->mu);
            bt->cv_done.wait(lk, [&] { return bt->ready == n_provers; });
        }
        if (bt->first_error) {
            int rc = bt->first_error;
            std::string text = bt->error_text;
            p3hip_fib_batch_destroy(bt.release());
            return fail(rc, text);
        }
        *out = bt.release();
        return OK;
    });
}

static int fib_batch_submit_job(p3hip_fib_batch_t* bt, std::shared_ptr<p3hip_fib_batch::Job> job, uint64_t* ticket_out);
int p3hip_fib_batch_submit(p3hip_fib_batch_t* bt, size_t n, const uint64_t* a, const uint64_t* b, uint64_t* ticket_out) {
    return guarded([&]() -> int {
        if (!bt || !ticket_out || (n && (!a || !b))) return fail(ERR_BAD_ARG, "fib_batch_submit: null argument");
        auto job = std::make_shared<p3hip_fib_batch::Job>();
        job->a.assign(a, a + n);
        job->b.assign(b, b + n);
        job->proofs.resize(n);
        return fib_batch_submit_job(bt, job, ticket_out);
    });
}
static int fib_batch_submit_job(p3hip_fib_batch_t* bt, std::shared_ptr<p3hip_fib_batch::Job> job, uint64_t* ticket_out) {
    std::unique_lock<std::mutex> lk(bt->mu);
    if (bt->jobs.size() >= p3hip_fib_batch::MAX_INFLIGHT)
        return fail(ERR_BAD_ARG, "fib_batch_submit: too many batches in flight (collect one first)");
    job->ticket = bt->next_ticket++;
    *ticket_out = job->ticket;
    bt->jobs.push_back(job);
    bt->cv_work.notify_all();
    return OK;
}

int p3hip_fib_batch_collect(p3hip_fib_batch_t* bt, uint64_t ticket, const uint8_t** proofs_out, size_t* lens_out) {
    return guarded([&]() -> int {
        if (!bt) return fail(ERR_BAD_ARG, "fib_batch_collect: null argument");
        std::shared_ptr<p3hip_fib_batch::Job> job;
        {
            std::unique_lock<std::mutex> lk(bt->mu);
            auto it = std::find_if(bt->jobs.begin(), bt->jobs.end(), [&](const std::shared_ptr<p3hip_fib_batch::Job>& j) { return j->ticket == ticket; });
            if (it == bt->jobs.end()) return fail(ERR_BAD_ARG, "fib_batch_collect: unknown ticket");
            job = *it;
            if (job->a.size() && (!proofs_out || !lens_out)) return fail(ERR_BAD_ARG, "fib_batch_collect: null argument");
            bt->cv_done.wait(lk, [&] { return job->done == job->a.size(); });
            bt->jobs.erase(std::find(bt->jobs.begin(), bt->jobs.end(), job));
            bt->collected = job;  // keeps the proof bytes alive until the next collect / prove / destroy
        }
        if (job->first_error) return fail(job->first_error, job->error_text);
        for (size_t i = 0; i < job->a.size(); i++) { proofs_out[i] = job->proofs[i].data(); lens_out[i] = job->proofs[i].size(); }
        return OK;
    });
}

int p3hip_fib_batch_prove(p3hip_fib_batch_t* bt, size_t n, const uint64_t* a, const uint64_t* b, const uint8_t** proofs_out,
                          size_t* lens_out) {
    if (!bt || (n && (!a || !b || !proofs_out || !lens_out))) return fail(ERR_BAD_ARG, "fib_batch_prove: null argument");
    if (!n) return OK;
    uint64_t ticket = 0;
    int rc = p3hip_fib_batch_submit(bt, n, a, b, &ticket);
    if (rc) return rc;
    return p3hip_fib_batch_collect(bt, ticket, proofs_out, lens_out);
}

int p3hip_fib_batch_prove_traces_dev(p3hip_fib_batch_t* bt, size_t n, const uint32_t* const* d_traces, const uint32_t* pis, unsigned flags,
                                     const uint8_t** proofs_out, size_t* lens_out) {
    if (!bt || (n && (!d_traces || !pis || !proofs_out || !lens_out))) return fail(ERR_BAD_ARG, "fib_batch_prove_traces_dev: null argument");
    if (!n) return OK;
    int rc = guarded([&]() -> int {
        // every trace and every public value is checked before any prover is given work
        auto job = std::make_shared<p3hip_fib_batch::Job>();
        for (size_t i = 0; i < n; i++) {
            const std::string who = "fib_batch_prove_traces_dev: instance " + std::to_string(i);
            int r = check_pis_flags(pis + 3 * i, flags, who);
            if (r) return r;
            if ((r = check_device_trace(d_traces[i], 1ull << bt->log_n, bt->device, who))) return r;
        }
        job->a.assign(n, 0);
        job->b.assign(n, 0);
        job->traces.assign(d_traces, d_traces + n);
        job->pis.assign(pis, pis + 3 * n);
        job->flags = flags;
        job->proofs.resize(n);
        uint64_t ticket = 0;
        int r = fib_batch_submit_job(bt, job, &ticket);
        if (r) return r;
        return p3hip_fib_batch_collect(bt, ticket, proofs_out, lens_out);
    });
    return rc;
}

void p3hip_fib_batch_destroy(p3hip_fib_batch_t* bt) {
    if (!bt) return;
    {
        std::unique_lock<std::mutex> lk(bt->mu);
        bt->stop = true;
        bt->cv_work.notify_all();
    }
    for (auto& t : bt->workers) t.join();
    delete bt;
}

}  // extern "C"

// ---- batches of proofs verified on the device (verifier_dev.hip) ----
struct p3hip_fib_verifier {
    FibVerifierDev v;
};
extern "C" {
int p3hip_fib_proof_len(int hash, int hiding, unsigned log_n, const p3hip_fri_params_t* params, size_t* len_out) {
    return guarded([&]() -> int {
        if (!params || !len_out) return fail(ERR_BAD_ARG, "fib_proof_len: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        return fib_proof_len(hash, hiding != 0, log_n, fp, len_out);
    });
}
int p3hip_fib_verifier_create(int hash, int hiding, unsigned log_n, const p3hip_fri_params_t* params, size_t max_proofs,
                              p3hip_fib_verifier_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "fib_verifier_create: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::unique_ptr<p3hip_fib_verifier> h(new p3hip_fib_verifier());
        if (int rc = h->v.init(hash, hiding != 0, log_n, fp, max_proofs)) return rc;
        *out = h.release();
        return OK;
    });
}
int p3hip_fib_verifier_verify_dev(p3hip_fib_verifier_t* v, const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens,
                                  const uint32_t* d_pis, size_t n, uint32_t* d_status, uint32_t* d_rejected, void* stream) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "fib_verifier_verify_dev: null verifier");
        return v->v.verify_dev(d_proofs, stride_bytes, d_lens, d_pis, n, d_status, d_rejected, static_cast<hipStream_t>(stream));
    });
}
int p3hip_fib_verifier_verify(p3hip_fib_verifier_t* v, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint64_t* a,
                              const uint64_t* b, const uint64_t* x, uint32_t* status_out) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "fib_verifier_verify: null verifier");
        return v->v.verify_host(n, proofs, lens, a, b, x, status_out);
    });
}
void p3hip_fib_verifier_destroy(p3hip_fib_verifier_t* v) { delete v; }
}  // extern "C"

// ---- TwoAdicFriPcs over caller matrices (pcs.hip.inc, verifier.hip) and the host challengers its callers drive ----
struct p3hip_challenger {
    Challenger c;
};
struct p3hip_pcs_data {
    std::unique_ptr<PcsData> d;
};
struct p3hip_pcs {
    Pcs pcs;
    std::vector<uint32_t> opened;
    std::vector<uint8_t> proof;
};

extern "C" {

int p3hip_challenger_create(int hash, p3hip_challenger_t** out) {
    return guarded([&]() -> int {
        if (!out) return fail(ERR_BAD_ARG, "challenger_create: null argument");
        if (hash != HASH_POSEIDON2 && hash != HASH_KECCAK) return fail(ERR_BAD_ARG, "challenger_create: unknown hash configuration");
        *out = new p3hip_challenger{Challenger(hash)};
        return OK;
    });
}
int p3hip_challenger_observe(p3hip_challenger_t* c, const uint32_t* monty_words, size_t n) {
    return guarded([&]() -> int {
        if (!c || (!monty_words && n)) return fail(ERR_BAD_ARG, "challenger_observe: null argument");
        for (size_t i = 0; i < n; i++)
            if (monty_words[i] >= bb::P) return fail(ERR_BAD_ARG, "challenger_observe: word " + std::to_string(i) + " is not a canonical field element");
        c->c.observe_n(monty_words, n);
        return OK;
    });
}
int p3hip_challenger_observe_digest(p3hip_challenger_t* c, const uint32_t digest[8]) {
    return guarded([&]() -> int {
        if (!c || !digest) return fail(ERR_BAD_ARG, "challenger_observe_digest: null argument");
        if (c->c.kind == HASH_POSEIDON2)
            for (int i = 0; i < 8; i++)
                if (digest[i] >= bb::P) return fail(ERR_BAD_ARG, "challenger_observe_digest: word " + std::to_string(i) + " is not a canonical field element");
        c->c.observe_digest(digest);
        return OK;
    });
}
int p3hip_challenger_sample_ext(p3hip_challenger_t* c, uint32_t out[4]) {
    return guarded([&]() -> int {
        if (!c || !out) return fail(ERR_BAD_ARG, "challenger_sample_ext: null argument");
        const bb::Ext e = c->c.sample_ext();
        memcpy(out, e.c, 16);
        return OK;
    });
}
int p3hip_challenger_sample_bits(p3hip_challenger_t* c, unsigned bits, uint32_t* out) {
    return guarded([&]() -> int {
        if (!c || !out) return fail(ERR_BAD_ARG, "challenger_sample_bits: null argument");
        if (bits > 30) return fail(ERR_BAD_ARG, "challenger_sample_bits: at most 30 bits");
        *out = (uint32_t)c->c.sample_bits(bits);
        return OK;
    });
}
int p3hip_challenger_clone(const p3hip_challenger_t* c, p3hip_challenger_t** out) {
    return guarded([&]() -> int {
        if (!c || !out) return fail(ERR_BAD_ARG, "challenger_clone: null argument");
        *out = new p3hip_challenger{c->c};
        return OK;
    });
}
void p3hip_challenger_destroy(p3hip_challenger_t* c) { delete c; }

static int pcs_create_plain(int profile, int hash, const p3hip_fri_params_t* params, void* stream, int own_stream, bool mixed, p3hip_pcs_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "pcs_create: null argument");
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "pcs_create: unknown profile");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        bool own = false;
        if (own_stream) {
            P3_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            own = true;
        }
        std::unique_ptr<p3hip_pcs> p(new p3hip_pcs());
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        // on failure the object's destructor destroys the owned stream
        if ((rc = p->pcs.init(fp, st, own, hash, profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY, mixed))) return rc;
        *out = p.release();
        return OK;
    });
}
int p3hip_pcs_create(int profile, int hash, const p3hip_fri_params_t* params, void* stream, int own_stream, p3hip_pcs_t** out) {
    return pcs_create_plain(profile, hash, params, stream, own_stream, false, out);
}
int p3hip_pcs_create_mixed(int profile, int hash, const p3hip_fri_params_t* params, void* stream, int own_stream, p3hip_pcs_t** out) {
    return pcs_create_plain(profile, hash, params, stream, own_stream, true, out);
}
int p3hip_pcs_create_hiding(int profile, int hash, const p3hip_fri_params_t* params, unsigned num_random_codewords, uint64_t mmcs_seed,
                            uint64_t pcs_seed, void* stream, int own_stream, p3hip_pcs_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "pcs_create_hiding: null argument");
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "pcs_create_hiding: unknown profile");
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        bool own = false;
        if (own_stream) {
            P3_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            own = true;
        }
        std::unique_ptr<p3hip_pcs> p(new p3hip_pcs());
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        // on failure the object's destructor destroys the owned stream
        if ((rc = p->pcs.init_hiding(fp, st, own, hash, profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY,
                                     num_random_codewords, mmcs_seed, pcs_seed)))
            return rc;
        *out = p.release();
        return OK;
    });
}
int p3hip_pcs_commit_quotient_dev(p3hip_pcs_t* pcs, const uint32_t* const* d_chunks, size_t h, size_t width, size_t n_chunks,
                                  uint32_t root_out[8], p3hip_pcs_data_t** data_out) {
    return guarded([&]() -> int {
        if (!pcs || !data_out) return fail(ERR_BAD_ARG, "pcs_commit_quotient: null argument");
        PcsData* d = nullptr;
        int rc = pcs->pcs.commit_quotient(d_chunks, h, width, n_chunks, root_out, &d);
        if (rc) return rc;
        *data_out = new p3hip_pcs_data{std::unique_ptr<PcsData>(d)};
        return OK;
    });
}
int p3hip_pcs_commit_randomization(p3hip_pcs_t* pcs, unsigned log_h, uint32_t root_out[8], p3hip_pcs_data_t** data_out) {
    return guarded([&]() -> int {
        if (!pcs || !data_out) return fail(ERR_BAD_ARG, "pcs_commit_randomization: null argument");
        PcsData* d = nullptr;
        int rc = pcs->pcs.commit_randomization(log_h, root_out, &d);
        if (rc) return rc;
        *data_out = new p3hip_pcs_data{std::unique_ptr<PcsData>(d)};
        return OK;
    });
}
int p3hip_pcs_commit_dev(p3hip_pcs_t* pcs, const uint32_t* const* d_evals, const size_t* heights, const size_t* widths,
                         const uint32_t* domain_shifts, size_t n_mats, uint32_t root_out[8], p3hip_pcs_data_t** data_out) {
    return guarded([&]() -> int {
        if (!pcs || !data_out) return fail(ERR_BAD_ARG, "pcs_commit: null argument");
        PcsData* d = nullptr;
        int rc = pcs->pcs.commit(d_evals, heights, widths, domain_shifts, n_mats, root_out, &d);
        if (rc) return rc;
        *data_out = new p3hip_pcs_data{std::unique_ptr<PcsData>(d)};
        return OK;
    });
}
int p3hip_pcs_lde_dev(const p3hip_pcs_data_t* data, size_t mat, const uint32_t** d_lde, size_t* height, size_t* width) {
    return guarded([&]() -> int {
        if (!data || !d_lde || !height || !width) return fail(ERR_BAD_ARG, "pcs_lde: null argument");
        if (mat >= data->d->lde.size()) return fail(ERR_BAD_ARG, "pcs_lde: matrix " + std::to_string(mat) + " of a commitment of " + std::to_string(data->d->lde.size()));
        *d_lde = data->d->lde[mat];
        *height = (size_t)1 << (data->d->mat_log_h(mat) + (data->d->log_big - data->d->log_h));  // the matrix's own LDE
        *width = data->d->widths[mat];
        return OK;
    });
}
int p3hip_pcs_open(p3hip_pcs_t* pcs, const p3hip_pcs_data_t* const* rounds, size_t n_rounds, const size_t* points_per_mat,
                   const uint32_t* points, p3hip_challenger_t* challenger, uint32_t* opened_out, size_t opened_cap_words,
                   const uint8_t** proof_out, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!pcs || !rounds || !challenger || !opened_out || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "pcs_open: null argument");
        if (n_rounds > PCS_MAX_ROUNDS) return fail(ERR_BAD_ARG, "pcs open: " + std::to_string(n_rounds) + " rounds, an open takes at most " + std::to_string(PCS_MAX_ROUNDS));
        const PcsData* rr[PCS_MAX_ROUNDS] = {nullptr};
        for (size_t r = 0; r < n_rounds; r++) rr[r] = rounds[r] ? rounds[r]->d.get() : nullptr;
        // the challenger is handed over only when the open succeeds: a failed call leaves the caller's transcript as it was
        Challenger ch = challenger->c;
        int rc = pcs->pcs.open(rr, n_rounds, points_per_mat, points, &ch, &pcs->opened, &pcs->proof);
        if (rc) { pcs->proof.clear(); return rc; }
        if (pcs->opened.size() > opened_cap_words)
            return fail(ERR_BAD_ARG, "pcs_open: the opened values take " + std::to_string(pcs->opened.size()) + " words, the buffer holds " + std::to_string(opened_cap_words));
        memcpy(opened_out, pcs->opened.data(), pcs->opened.size() * 4);
        challenger->c = ch;
        *proof_out = pcs->proof.data();
        *proof_len = pcs->proof.size();
        return OK;
    });
}
int p3hip_pcs_verify(int hash, const p3hip_fri_params_t* params, unsigned log_h, const uint32_t* roots, const size_t* mats_per_round,
                     const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points, const uint32_t* opened,
                     const uint8_t* proof, size_t len, p3hip_challenger_t* challenger, int* reject_code) {
    return guarded([&]() -> int {
        if (!params || !challenger || !reject_code) return fail(ERR_BAD_ARG, "pcs_verify: null argument");
        *reject_code = 0;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        Challenger ch = challenger->c;
        int rc = pcs_verify(hash, fp, log_h, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, &ch, &why);
        if (rc < 0) return fail(rc, why);
        challenger->c = ch;  // accepted or rejected, the transcript is where the verifier left it
        if (rc > 0) { *reject_code = rc; set_error("pcs verification failed: " + why); }
        return OK;
    });
}
int p3hip_pcs_verify_mixed(int hash, const p3hip_fri_params_t* params, const unsigned* log_heights, const uint32_t* roots,
                           const size_t* mats_per_round, const size_t* widths, size_t n_rounds, const size_t* points_per_mat,
                           const uint32_t* points, const uint32_t* opened, const uint8_t* proof, size_t len, p3hip_challenger_t* challenger,
                           int* reject_code) {
    return guarded([&]() -> int {
        if (!params || !challenger || !reject_code) return fail(ERR_BAD_ARG, "pcs_verify_mixed: null argument");
        *reject_code = 0;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        Challenger ch = challenger->c;
        int rc = pcs_verify_mixed(hash, fp, log_heights, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, &ch, &why);
        if (rc < 0) return fail(rc, why);
        challenger->c = ch;  // accepted or rejected, the transcript is where the verifier left it
        if (rc > 0) { *reject_code = rc; set_error("pcs verification failed: " + why); }
        return OK;
    });
}
int p3hip_pcs_verify_hiding(int hash, const p3hip_fri_params_t* params, unsigned log_h, const uint32_t* roots, const size_t* mats_per_round,
                            const size_t* widths, size_t n_rounds, const size_t* points_per_mat, const uint32_t* points,
                            const uint32_t* opened, const uint8_t* proof, size_t len, p3hip_challenger_t* challenger, int* reject_code) {
    return guarded([&]() -> int {
        if (!params || !challenger || !reject_code) return fail(ERR_BAD_ARG, "pcs_verify_hiding: null argument");
        *reject_code = 0;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        Challenger ch = challenger->c;
        int rc = pcs_verify_hiding(hash, fp, log_h, roots, mats_per_round, widths, n_rounds, points_per_mat, points, opened, proof, len, &ch, &why);
        if (rc < 0) return fail(rc, why);
        challenger->c = ch;  // accepted or rejected, the transcript is where the verifier left it
        if (rc > 0) { *reject_code = rc; set_error("pcs verification failed: " + why); }
        return OK;
    });
}
void p3hip_pcs_data_free(p3hip_pcs_data_t* d) { delete d; }
void p3hip_pcs_destroy(p3hip_pcs_t* pcs) { delete pcs; }

}  // extern "C"

// ---- batches of PCS proofs verified on the device (pcs_verifier_dev.hip) ----
struct p3hip_pcs_verifier {
    PcsVerifierDev v;
};
static_assert(P3HIP_CHALLENGER_STATE_WORDS == CHALLENGER_STATE_WORDS, "include/p3hip.h and prover.h agree on the state's size");
static int pcs_shape_of(const p3hip_pcs_shape_t* s, PcsShape* out, const char* who) {
    if (!s) return fail(ERR_BAD_ARG, std::string(who) + ": null argument");
    *out = PcsShape{s->log_h, s->n_rounds, s->mats_per_round, s->widths, s->points_per_mat, s->n_slots, s->slots, nullptr};
    return OK;
}
// the mixed entries: log_heights in place of shape->log_h
static int pcs_shape_mixed_of(const p3hip_pcs_shape_t* s, const unsigned* log_heights, PcsShape* out, const char* who) {
    if (!log_heights) return fail(ERR_BAD_ARG, std::string(who) + ": null argument");
    if (int rc = pcs_shape_of(s, out, who)) return rc;
    out->log_h = 0;
    out->log_heights = log_heights;
    return OK;
}
extern "C" {
int p3hip_challenger_export(const p3hip_challenger_t* c, uint32_t* words) {
    return guarded([&]() -> int {
        if (!c || !words) return fail(ERR_BAD_ARG, "challenger_export: null argument");
        challenger_export(c->c, words);
        return OK;
    });
}
int p3hip_challenger_import(p3hip_challenger_t* c, const uint32_t* words) {
    return guarded([&]() -> int {
        if (!c || !words) return fail(ERR_BAD_ARG, "challenger_import: null argument");
        return challenger_import(words, &c->c);
    });
}
int p3hip_pcs_proof_len(int hash, int hiding, const p3hip_fri_params_t* params, const p3hip_pcs_shape_t* shape, size_t* len_out) {
    return guarded([&]() -> int {
        if (!params || !len_out) return fail(ERR_BAD_ARG, "pcs_proof_len: null argument");
        PcsShape sh;
        if (int rc = pcs_shape_of(shape, &sh, "pcs_proof_len")) return rc;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        return pcs_proof_len(hash, hiding != 0, fp, sh, len_out);
    });
}
int p3hip_pcs_verifier_create(int hash, int hiding, const p3hip_fri_params_t* params, const p3hip_pcs_shape_t* shape, size_t max_proofs,
                              p3hip_pcs_verifier_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "pcs_verifier_create: null argument");
        PcsShape sh;
        if (int rc = pcs_shape_of(shape, &sh, "pcs_verifier_create")) return rc;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::unique_ptr<p3hip_pcs_verifier> h(new p3hip_pcs_verifier());
        if (int rc = h->v.init(hash, hiding != 0, fp, sh, max_proofs)) return rc;
        *out = h.release();
        return OK;
    });
}
int p3hip_pcs_proof_len_mixed(int hash, int hiding, const p3hip_fri_params_t* params, const p3hip_pcs_shape_t* shape, const unsigned* log_heights,
                              size_t* len_out) {
    return guarded([&]() -> int {
        if (!params || !len_out) return fail(ERR_BAD_ARG, "pcs_proof_len_mixed: null argument");
        PcsShape sh;
        if (int rc = pcs_shape_mixed_of(shape, log_heights, &sh, "pcs_proof_len_mixed")) return rc;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        return pcs_proof_len(hash, hiding != 0, fp, sh, len_out);
    });
}
int p3hip_pcs_verifier_create_mixed(int hash, int hiding, const p3hip_fri_params_t* params, const p3hip_pcs_shape_t* shape,
                                    const unsigned* log_heights, size_t max_proofs, p3hip_pcs_verifier_t** out) {
    return guarded([&]() -> int {
        if (!params || !out) return fail(ERR_BAD_ARG, "pcs_verifier_create_mixed: null argument");
        PcsShape sh;
        if (int rc = pcs_shape_mixed_of(shape, log_heights, &sh, "pcs_verifier_create_mixed")) return rc;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::unique_ptr<p3hip_pcs_verifier> h(new p3hip_pcs_verifier());
        if (int rc = h->v.init(hash, hiding != 0, fp, sh, max_proofs)) return rc;
        *out = h.release();
        return OK;
    });
}
int p3hip_pcs_verifier_verify_dev(p3hip_pcs_verifier_t* v, const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens,
                                  const uint32_t* d_roots, const uint32_t* d_points, const uint32_t* d_opened, const uint32_t* d_chal_in,
                                  size_t n, uint32_t* d_status, uint32_t* d_rejected, uint32_t* d_chal_out, void* stream) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "pcs_verifier_verify_dev: null verifier");
        return v->v.verify_dev(d_proofs, stride_bytes, d_lens, d_roots, d_points, d_opened, d_chal_in, n, d_status, d_rejected, d_chal_out,
                               static_cast<hipStream_t>(stream));
    });
}
int p3hip_pcs_verifier_verify(p3hip_pcs_verifier_t* v, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* roots,
                              const uint32_t* points, const uint32_t* opened, p3hip_challenger_t* const* challengers, uint32_t* status_out) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "pcs_verifier_verify: null verifier");
        if (n && !challengers) return fail(ERR_BAD_ARG, "pcs_verifier_verify: null argument");
        std::vector<Challenger*> ch(n);
        for (size_t i = 0; i < n; i++) ch[i] = challengers[i] ? &challengers[i]->c : nullptr;
        return v->v.verify_host(n, proofs, lens, roots, points, opened, ch.data(), status_out);
    });
}
int p3hip_pcs_verifier_wave_form(const p3hip_pcs_verifier_t* v) { return v && v->v.wave_form() ? 1 : 0; }
void p3hip_pcs_verifier_destroy(p3hip_pcs_verifier_t* v) { delete v; }
}  // extern "C"

// ---- proofs of caller-defined AIRs verified on the host and, in batches, on the device (air_verifier_dev.hip) ----
struct p3hip_air_verifier {
    AirVerifierDev v;
};
extern "C" {
int p3hip_air_proof_len(const p3hip_air_t* air, int hash, unsigned log_n, const p3hip_fri_params_t* params, size_t* len_out) {
    return guarded([&]() -> int {
        if (!air || !params || !len_out) return fail(ERR_BAD_ARG, "air_proof_len: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        return air_proof_len(air->a, hash, log_n, fp, len_out);
    });
}
int p3hip_air_verify(const p3hip_air_t* air, int hash, unsigned log_n, const p3hip_fri_params_t* params, const uint8_t* proof, size_t len,
                     const uint32_t* pis, int* reject_code) {
    return guarded([&]() -> int {
        if (!air || !params || (!proof && len) || !reject_code || (!pis && air->a.n_public)) return fail(ERR_BAD_ARG, "air_verify: null argument");
        *reject_code = 0;
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::string why;
        const int rc = air_verify(air->a, hash, log_n, fp, proof, len, pis, &why);
        if (rc < 0) return fail(rc, why);
        if (rc > 0) { *reject_code = rc; set_error("air verification failed: " + why); }
        return OK;
    });
}
int p3hip_air_eval_ext_dev(p3hip_air_t* air, void* stream, const uint32_t* d_local, const uint32_t* d_next, const uint32_t* d_pis,
                           const uint32_t* d_sels, const uint32_t* d_alpha, size_t n, uint32_t* d_out) {
    return guarded([&]() -> int {
        if (!air) return fail(ERR_BAD_ARG, "air_eval_ext_dev: null argument");
        return air_eval_ext_dev(air->a, static_cast<hipStream_t>(stream), d_local, d_next, d_pis, d_sels, d_alpha, n, d_out);
    });
}
int p3hip_air_verifier_create(const p3hip_air_t* air, int hash, unsigned log_n, const p3hip_fri_params_t* params, size_t max_proofs,
                              p3hip_air_verifier_t** out) {
    return guarded([&]() -> int {
        if (!air || !params || !out) return fail(ERR_BAD_ARG, "air_verifier_create: null argument");
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        std::unique_ptr<p3hip_air_verifier> h(new p3hip_air_verifier());
        if (int rc = h->v.init(air->a, hash, log_n, fp, max_proofs)) return rc;
        *out = h.release();
        return OK;
    });
}
int p3hip_air_verifier_verify_dev(p3hip_air_verifier_t* v, const uint8_t* d_proofs, size_t stride_bytes, const uint32_t* d_lens,
                                  const uint32_t* d_pis, size_t n, uint32_t* d_status, uint32_t* d_rejected, void* stream) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "air_verifier_verify_dev: null verifier");
        return v->v.verify_dev(d_proofs, stride_bytes, d_lens, d_pis, n, d_status, d_rejected, static_cast<hipStream_t>(stream));
    });
}
int p3hip_air_verifier_verify(p3hip_air_verifier_t* v, size_t n, const uint8_t* const* proofs, const size_t* lens, const uint32_t* pis,
                              uint32_t* status_out) {
    return guarded([&]() -> int {
        if (!v) return fail(ERR_BAD_ARG, "air_verifier_verify: null verifier");
        return v->v.verify_host(n, proofs, lens, pis, status_out);
    });
}
void p3hip_air_verifier_destroy(p3hip_air_verifier_t* v) { delete v; }
}  // extern "C"

// ---- proofs of caller-defined AIRs made in one device-resident launch chain (air_prover.hip.inc) ----
struct p3hip_air_prover {
    AirProver p;
    std::vector<uint8_t> last;
};
// the public values, the flags and the optional check_constraints pass in front of a proof
static int air_prover_admit(p3hip_air_prover& h, const uint32_t* d_trace, const uint32_t* pis, unsigned flags, const char* who) {
    if (flags & ~P3HIP_PROVE_CHECK_TRACE) return fail(ERR_BAD_ARG, std::string(who) + ": unknown flag bits");
    if (!pis && h.p.n_public()) return fail(ERR_BAD_ARG, std::string(who) + ": null public values");
    for (uint32_t k = 0; k < h.p.n_public(); k++)
        if (pis[k] >= bb::P) return fail(ERR_BAD_ARG, std::string(who) + ": public value " + std::to_string(k) + " is not a canonical field element");
    if (!(flags & P3HIP_PROVE_CHECK_TRACE)) return OK;
    long long row = -1;
    int k = -1;
    if (int rc = h.p.check_trace(d_trace, pis, &row, &k)) return rc;
    if (row >= 0) return fail(ERR_BAD_ARG, "constraints had nonzero value on row " + std::to_string(row) + " (constraint " + std::to_string(k) + ")");
    return OK;
}
static int air_prover_device(const p3hip_air_prover& h) {
    Context* cx;
    if (int rc = get_context(&cx)) return rc;
    if (cx->device != h.p.device())
        return fail(ERR_BAD_ARG, "air prover: created on device " + std::to_string(h.p.device()) + ", current device is " + std::to_string(cx->device));
    return OK;
}
extern "C" {
int p3hip_air_prover_create(const p3hip_air_t* air, int profile, int hash, unsigned log_n, const p3hip_fri_params_t* params, void* stream,
                            int own_stream, p3hip_air_prover_t** out) {
    return guarded([&]() -> int {
        if (!air || !params || !out) return fail(ERR_BAD_ARG, "air_prover_create: null argument");
        if (profile != P3HIP_PROFILE_THROUGHPUT && profile != P3HIP_PROFILE_LATENCY) return fail(ERR_BAD_ARG, "air_prover_create: unknown profile");
        const int prof = profile == P3HIP_PROFILE_THROUGHPUT ? PROFILE_THROUGHPUT : PROFILE_LATENCY;
        Context* cx;
        int rc = get_context(&cx);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        bool own = false;
        if (own_stream) {
            P3_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            own = true;
        }
        std::unique_ptr<p3hip_air_prover> h(new p3hip_air_prover());
        FriParams fp{params->log_blowup, params->log_final_poly_len, params->num_queries, params->proof_of_work_bits};
        if ((rc = h->p.init(air->a, prof, hash, log_n, fp, st, own))) return rc;  // on failure the destructor destroys the owned stream
        *out = h.release();
        return OK;
    });
}
int p3hip_air_prover_enqueue_dev(p3hip_air_prover_t* prover, const uint32_t* d_trace, const uint32_t* pis) {
    return guarded([&]() -> int {
        if (!prover) return fail(ERR_BAD_ARG, "air_prover_enqueue_dev: null argument");
        if (int rc = air_prover_device(*prover)) return rc;
        if (int rc = air_prover_admit(*prover, d_trace, pis, 0, "air_prover_enqueue_dev")) return rc;
        return prover->p.enqueue(d_trace, pis);
    });
}
int p3hip_air_prover_finish(p3hip_air_prover_t* prover, const uint8_t** proof_out, size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "air_prover_finish: null argument");
        int rc = prover->p.finish(&prover->last);
        if (rc) { prover->last.clear(); return rc; }  // a failed proof leaves nothing behind that could be mistaken for one
        *proof_out = prover->last.data();
        *proof_len = prover->last.size();
        return OK;
    });
}
int p3hip_air_prover_prove_dev(p3hip_air_prover_t* prover, const uint32_t* d_trace, const uint32_t* pis, unsigned flags, const uint8_t** proof_out,
                               size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "air_prover_prove_dev: null argument");
        if (prover->p.pending()) return fail(ERR_BAD_ARG, "air prover: finish the enqueued proof before a synchronous prove");
        if (int rc = air_prover_device(*prover)) return rc;
        if (!d_trace) return fail(ERR_BAD_ARG, "air_prover_prove_dev: null trace");
        if (int rc = air_prover_admit(*prover, d_trace, pis, flags, "air_prover_prove_dev")) return rc;
        if (int rc = prover->p.enqueue(d_trace, pis)) return rc;
        return p3hip_air_prover_finish(prover, proof_out, proof_len);
    });
}
int p3hip_air_prover_prove(p3hip_air_prover_t* prover, const uint32_t* host_trace, const uint32_t* pis, unsigned flags, const uint8_t** proof_out,
                           size_t* proof_len) {
    return guarded([&]() -> int {
        if (!prover || !host_trace || !proof_out || !proof_len) return fail(ERR_BAD_ARG, "air_prover_prove: null argument");
        if (prover->p.pending()) return fail(ERR_BAD_ARG, "air prover: finish the enqueued proof before a synchronous prove");
        if (int rc = air_prover_device(*prover)) return rc;
        if (flags & ~P3HIP_PROVE_CHECK_TRACE) return fail(ERR_BAD_ARG, "air_prover_prove: unknown flag bits");
        // into the arena's trace slot, on the prover's stream: ordered before everything of the proof that reads it
        uint32_t* slot = prover->p.arena_trace();
        if (!slot) return ERR_HIP;
        P3_HIP(hipMemcpyAsync(slot, host_trace, ((size_t)4 << prover->p.log_n()) * prover->p.width(), hipMemcpyHostToDevice, prover->p.stream()));
        if (int rc = air_prover_admit(*prover, slot, pis, flags, "air_prover_prove")) return rc;
        if (int rc = prover->p.enqueue(slot, pis)) return rc;
        return p3hip_air_prover_finish(prover, proof_out, proof_len);
    });
}
void p3hip_air_prover_destroy(p3hip_air_prover_t* prover) { delete prover; }
}  // extern "C"
