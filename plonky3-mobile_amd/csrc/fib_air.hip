// FibonacciAir workload pieces on the device (reference native/src/fib_air.rs:224-306).
//   generate_trace_rows (fib_air.rs:266-284): row 0 = (a, b), row i = (right_{i-1}, left_{i-1} + right_{i-1}).
// The recurrence is serial on the CPU; here each lane jumps to its chunk with a 2x2 matrix power
// (fast doubling over BabyBear) and then walks CHUNK rows, storing 8-byte rows coalesced per lane.
//   check_constraints (p3_uni_stark's debug-build check before proving): one streaming pass over a caller's trace.
#include "bb31.hip.h"
#include "common.h"

#include <algorithm>

namespace p3 {

constexpr uint32_t FIB_CHUNK = 16;

struct M2 { uint32_t a, b, c, d; };  // [[a b],[c d]]
__device__ __forceinline__ M2 m2mul(const M2& x, const M2& y) {
    return M2{bb::add(bb::mul(x.a, y.a), bb::mul(x.b, y.c)), bb::add(bb::mul(x.a, y.b), bb::mul(x.b, y.d)),
              bb::add(bb::mul(x.c, y.a), bb::mul(x.d, y.c)), bb::add(bb::mul(x.c, y.b), bb::mul(x.d, y.d))};
}

__global__ void fib_trace_kernel(uint32_t a0, uint32_t b0, uint64_t n, uint32_t* out) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t start = t * FIB_CHUNK;
    if (start >= n) return;
    // (left, right)_i = M^i (a0, b0),  M = [[0,1],[1,1]]
    M2 acc{bb::ONE, 0, 0, bb::ONE}, base{0, bb::ONE, bb::ONE, bb::ONE};
    for (uint64_t e = start; e; e >>= 1) {
        if (e & 1) acc = m2mul(acc, base);
        base = m2mul(base, base);
    }
    uint32_t l = bb::add(bb::mul(acc.a, a0), bb::mul(acc.b, b0));
    uint32_t r = bb::add(bb::mul(acc.c, a0), bb::mul(acc.d, b0));
    uint2* rows = reinterpret_cast<uint2*>(out);
    for (uint32_t i = 0; i < FIB_CHUNK && start + i < n; i++) {
        rows[start + i] = make_uint2(l, r);
        uint32_t nr = bb::add(l, r);
        l = r;
        r = nr;
    }
}

int fib_trace(hipStream_t stream, uint64_t a, uint64_t b, uint64_t n, uint32_t* d_out) {
    if (!n) return OK;
    if (!is_pow2(n)) return fail(ERR_BAD_ARG, "generate_trace_rows: n must be a power of two");  // fib_air.rs:267
    uint64_t threads = (n + FIB_CHUNK - 1) / FIB_CHUNK;
    uint32_t a0 = bb::to_monty((uint32_t)(a % bb::P)), b0 = bb::to_monty((uint32_t)(b % bb::P));
    hipLaunchKernelGGL(fib_trace_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, a0, b0, n, d_out);
    P3_HIP(hipGetLastError());
    return OK;
}

// ---- check_constraints for FibonacciAir (fib_air.rs:236-260 eval) over a device trace of n rows x 2 Montgomery words ----
// Row i gets a mask of the rules it breaks (TRACE_BAD_* in common.h); is_transition is false on row n - 1, no wrap-around.
// A streaming read: every lane loads two rows with one 16-byte load, takes the row after them from the neighbouring lane by a
// shuffle (lane 63: from lane 0 of the next tile, or one 8-byte load behind the wave's last tile), keeps the smallest
// (row << 6 | mask) and a count in registers, and a wave that saw a bad row does one atomicMax on ~key and one atomicAdd.
constexpr uint32_t CHECK_BLOCK = 256, CHECK_UNROLL = 4, CHECK_MAX_BLOCKS = 256 * 8;  // 8 workgroups (32 waves) per CU

struct CheckPis { uint32_t p0, p1, p2; };

__device__ __forceinline__ uint32_t check_row(uint64_t i, uint64_t n, uint32_t l, uint32_t r, uint32_t nl, uint32_t nr, const CheckPis& p) {
    uint32_t m = (l >= bb::P || r >= bb::P) ? TRACE_BAD_RANGE : 0u;
    if (i == 0) m |= (l != p.p0 ? TRACE_BAD_FIRST_LEFT : 0u) | (r != p.p1 ? TRACE_BAD_FIRST_RIGHT : 0u);
    if (i + 1 < n) {
        m |= nl != r ? TRACE_BAD_NEXT_LEFT : 0u;
        m |= nr != (uint32_t)(((uint64_t)l + r) % bb::P) ? TRACE_BAD_NEXT_RIGHT : 0u;  // left + right, defined for any words
    } else {
        m |= r != p.p2 ? TRACE_BAD_LAST_RIGHT : 0u;
    }
    return m;
}

template <bool WIDE>  // WIDE: the trace is 16-byte aligned (one dwordx4 per lane); else two 8-byte loads per lane
__global__ void __launch_bounds__(CHECK_BLOCK) fib_check_trace_kernel(const uint32_t* trace, uint64_t n, CheckPis pis,
                                                                     unsigned long long* res /* [~min key, count] */) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pairs = (n + 1) / 2;
    const uint64_t wave = ((uint64_t)blockIdx.x * CHECK_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * CHECK_BLOCK) >> 6;
    const uint2* rows = reinterpret_cast<const uint2*>(trace);
    unsigned long long best = ~0ull;
    uint32_t bad = 0;
    for (uint64_t base = wave * 64 * CHECK_UNROLL; base < pairs; base += n_waves * 64 * CHECK_UNROLL) {
        uint4 v[CHECK_UNROLL];
#pragma unroll
        for (uint32_t k = 0; k < CHECK_UNROLL; k++) {
            const uint64_t q = base + k * 64 + lane;
            v[k] = make_uint4(0, 0, 0, 0);
            if (2 * q + 2 <= n) {
                if (WIDE) {
                    v[k] = reinterpret_cast<const uint4*>(trace)[q];
                } else {
                    const uint2 x = rows[2 * q], y = rows[2 * q + 1];
                    v[k] = make_uint4(x.x, x.y, y.x, y.y);
                }
            } else if (2 * q < n) {
                const uint2 x = rows[2 * q];
                v[k].x = x.x; v[k].y = x.y;
            }
        }
        // the row behind the wave's last pair of the last tile: the next tile's first row
        uint2 tail = make_uint2(0, 0);
        const uint64_t tail_row = 2 * (base + CHECK_UNROLL * 64);
        if (lane == 63 && tail_row < n) tail = rows[tail_row];
#pragma unroll
        for (uint32_t k = 0; k < CHECK_UNROLL; k++) {
            const uint64_t q = base + k * 64 + lane;
            uint32_t nl = __shfl_down(v[k].x, 1), nr = __shfl_down(v[k].y, 1);
            if (k + 1 < CHECK_UNROLL) {
                const uint32_t fl = __shfl(v[k + 1].x, 0), fr = __shfl(v[k + 1].y, 0);
                if (lane == 63) { nl = fl; nr = fr; }
            } else if (lane == 63) {
                nl = tail.x; nr = tail.y;
            }
            if (2 * q < n) {
                const uint32_t m0 = check_row(2 * q, n, v[k].x, v[k].y, v[k].z, v[k].w, pis);
                if (m0) { best = min(best, ((unsigned long long)(2 * q) << 6) | m0); bad++; }
                if (2 * q + 1 < n) {
                    const uint32_t m1 = check_row(2 * q + 1, n, v[k].z, v[k].w, nl, nr, pis);
                    if (m1) { best = min(best, ((unsigned long long)(2 * q + 1) << 6) | m1); bad++; }
                }
            }
        }
    }
    if (__ballot(bad != 0) == 0) return;  // wave-uniform: a clean wave does no atomic
    unsigned long long total = bad;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        best = min(best, __shfl_xor(best, off));
        total += __shfl_xor(total, off);
    }
    if (lane == 0) {
        atomicMax(&res[0], ~best);
        atomicAdd(&res[1], total);
    }
}

int fib_check_trace(Context& cx, hipStream_t stream, const uint32_t* d_trace, uint64_t n, const uint32_t pis[3], TraceCheck* out) {
    *out = TraceCheck{-1, 0, 0};
    if (!n) return OK;
    if (reinterpret_cast<uintptr_t>(d_trace) % 8) return fail(ERR_BAD_ARG, "check_trace: the trace must be 8-byte aligned (rows of two words)");
    if (n > (1ull << 57)) return fail(ERR_BAD_ARG, "check_trace: too many rows");
    DevBuf& buf = cx.ws(stream, 4);
    int rc = buf.reserve(16);
    if (rc) return rc;
    unsigned long long* res = buf.as<unsigned long long>();
    P3_HIP(hipMemsetAsync(res, 0, 16, stream));
    const uint64_t pairs = (n + 1) / 2, per_block = (uint64_t)CHECK_BLOCK * CHECK_UNROLL;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((pairs + per_block - 1) / per_block, CHECK_MAX_BLOCKS);
    const CheckPis p{pis[0], pis[1], pis[2]};
    if (reinterpret_cast<uintptr_t>(d_trace) % 16 == 0)
        hipLaunchKernelGGL(fib_check_trace_kernel<true>, dim3(blocks), dim3(CHECK_BLOCK), 0, stream, d_trace, n, p, res);
    else
        hipLaunchKernelGGL(fib_check_trace_kernel<false>, dim3(blocks), dim3(CHECK_BLOCK), 0, stream, d_trace, n, p, res);
    P3_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    P3_HIP(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, stream));
    P3_HIP(hipStreamSynchronize(stream));
    if (h[1]) {
        const unsigned long long key = ~h[0];
        out->first_bad_row = (int64_t)(key >> 6);
        out->mask = (uint32_t)(key & 63);
        out->bad_rows = h[1];
    }
    return OK;
}

}  // namespace p3
