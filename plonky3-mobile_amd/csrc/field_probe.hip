// Test probe of the field arithmetic, primitive by primitive (include/p3hip.h, "field probe"): lane i reads its operands, calls the
// HEADER function itself and writes what it returns.  Nothing of bb31.hip.h, poseidon2_f64.hip.h or ntt_narrow_f64.hip.h is repeated
// here, and this unit is compiled by the Makefile's one rule, so a function inlined here is the instruction sequence (and the
// fp-contraction setting) the kernels get.  The integer and extension ops are BB_HD: probe_words is compiled for both sides, the
// kernel runs the device branches, p3hip_field_probe_host the host branches.  The fp64 functions are __device__ only.
// No address and no loop bound comes from an operand: a lane's offsets are i * (words per lane of the op), the only data-dependent
// loops are pow's (at most 64 bits of exponent) and two_adic_generator's (at most 27 squarings for any 32-bit `bits`).
#include "../../include/p3hip.h"

#include "bb31.hip.h"
#include "common.h"
#include "ntt_args.hip.h"
#include "ntt_fast.hip.h"
#include "ntt_narrow.hip.h"
#include "ntt_narrow_f64.hip.h"

namespace p3 {
namespace {

struct OpInfo { int op; const char* name; int k, m; bool f64; };  // k operands in, m results out, per lane
constexpr OpInfo OPS[] = {
    {P3HIP_FP_ADD, "add", 2, 1, false}, {P3HIP_FP_SUB, "sub", 2, 1, false}, {P3HIP_FP_NEG, "neg", 1, 1, false},
    {P3HIP_FP_DBL, "dbl", 1, 1, false}, {P3HIP_FP_MUL, "mul", 2, 1, false}, {P3HIP_FP_SQR, "sqr", 1, 1, false},
    {P3HIP_FP_DOT2, "dot2", 4, 1, false}, {P3HIP_FP_TO_MONTY, "to_monty", 1, 1, false},
    {P3HIP_FP_FROM_MONTY, "from_monty", 1, 1, false}, {P3HIP_FP_POW7, "pow7", 1, 1, false}, {P3HIP_FP_POW, "pow", 3, 1, false},
    {P3HIP_FP_INV, "inv", 1, 1, false}, {P3HIP_FP_TWO_ADIC_GENERATOR, "two_adic_generator", 1, 1, false},
    {P3HIP_FP_SMUL, "smul", 2, 1, false}, {P3HIP_FP_SBOX7_ADD, "sbox7_add", 2, 1, false},
    {P3HIP_FP_EXT_MUL, "ext mul", 8, 4, false}, {P3HIP_FP_EXT_SQR, "ext sqr", 4, 4, false}, {P3HIP_FP_EXT_INV, "ext inv", 4, 4, false},
    {P3HIP_FP_EXT_POW, "ext pow", 6, 4, false}, {P3HIP_FP_EXT_SCALE, "ext scale", 5, 4, false},
    {P3HIP_FP_MULMOD, "mulmod", 2, 1, true}, {P3HIP_FP_MULMOD_P, "mulmod_p", 3, 1, true},
    {P3HIP_FP_MULMOD_P_DEV, "mulmod_p (aP on device)", 2, 1, true}, {P3HIP_FP_MULMOD_M, "mulmod_m", 3, 1, true},
    {P3HIP_FP_MULMOD_M_DEV, "mulmod_m (aP on device)", 2, 1, true}, {P3HIP_FP_ADD_SCALED_POW2, "add_scaled_pow2", 3, 1, true},
    {P3HIP_FP_SBOX7, "sbox7", 1, 1, true}, {P3HIP_FP_STORE_ELEM, "store_elem", 1, 1, true}, {P3HIP_FP_MULM, "mulm", 3, 1, true},
    {P3HIP_FP_MULM_DEV, "mulm (aP on device)", 2, 1, true}, {P3HIP_FP_WORD_CENTERED, "word_centered", 1, 1, true},
    {P3HIP_FP_WORD_ANY, "word_any", 1, 1, true}, {P3HIP_FP_ADD_SCALED_INT, "add_scaled_pow2 (integer multiplier)", 3, 1, true},
    {P3HIP_FP_SBOX7_WIDE, "sbox7 (first-round inputs)", 1, 1, true},
};
const OpInfo* find_op(int op) {
    for (const OpInfo& o : OPS)
        if (o.op == op) return &o;
    return nullptr;
}

BB_HD bb::Ext ext_at(const uint32_t* p) { return bb::Ext{{p[0], p[1], p[2], p[3]}}; }
BB_HD void ext_to(uint32_t* p, const bb::Ext& e) { p[0] = e.c[0]; p[1] = e.c[1]; p[2] = e.c[2]; p[3] = e.c[3]; }
BB_HD uint64_t u64_at(const uint32_t* p) { return (uint64_t)p[0] | ((uint64_t)p[1] << 32); }

// one lane of an integer or extension op: `a` = its k operand words, `o` = its m result words
BB_HD void probe_words(int op, const uint32_t* a, uint32_t* o) {
    switch (op) {
    case P3HIP_FP_ADD: o[0] = bb::add(a[0], a[1]); break;
    case P3HIP_FP_SUB: o[0] = bb::sub(a[0], a[1]); break;
    case P3HIP_FP_NEG: o[0] = bb::neg(a[0]); break;
    case P3HIP_FP_DBL: o[0] = bb::dbl(a[0]); break;
    case P3HIP_FP_MUL: o[0] = bb::mul(a[0], a[1]); break;
    case P3HIP_FP_SQR: o[0] = bb::sqr(a[0]); break;
    case P3HIP_FP_DOT2: o[0] = bb::dot2(a[0], a[1], a[2], a[3]); break;
    case P3HIP_FP_TO_MONTY: o[0] = bb::to_monty(a[0]); break;
    case P3HIP_FP_FROM_MONTY: o[0] = bb::from_monty(a[0]); break;
    case P3HIP_FP_POW7: o[0] = bb::pow7(a[0]); break;
    case P3HIP_FP_POW: o[0] = bb::pow(a[0], u64_at(a + 1)); break;
    case P3HIP_FP_INV: o[0] = bb::inv(a[0]); break;
    case P3HIP_FP_TWO_ADIC_GENERATOR: o[0] = bb::two_adic_generator(a[0]); break;
    case P3HIP_FP_SMUL: o[0] = (uint32_t)bb::smul((int32_t)a[0], (int32_t)a[1]); break;
    case P3HIP_FP_SBOX7_ADD: o[0] = bb::sbox7_add(a[0], a[1]); break;
    case P3HIP_FP_EXT_MUL: ext_to(o, bb::mul(ext_at(a), ext_at(a + 4))); break;
    case P3HIP_FP_EXT_SQR: ext_to(o, bb::sqr(ext_at(a))); break;
    case P3HIP_FP_EXT_INV: ext_to(o, bb::inv(ext_at(a))); break;
    case P3HIP_FP_EXT_POW: ext_to(o, bb::pow(ext_at(a), u64_at(a + 4))); break;
    case P3HIP_FP_EXT_SCALE: ext_to(o, bb::scale(ext_at(a), a[4])); break;
    default: break;
    }
}

// one lane of an fp64 op; the uniform operands arrive as the kernels get them: -(P - 1) and 1 / P of the Poseidon2 functions from
// p2f::d_c, those of the transform's functions from the kernel arguments (narrow64::Uni), the magic pair pinned once per kernel
__device__ __forceinline__ double probe_f64(int op, const double* a, const p2f::MagicRegs& mk, const narrow64::Magic& nk,
                                            const narrow64::Uni& un) {
    const double npm1 = p2f::d_c.neg_pm1, pinv = p2f::d_c.pinv;
    switch (op) {
    case P3HIP_FP_MULMOD: return p2f::mulmod(a[0], a[1]);
    case P3HIP_FP_MULMOD_P: return p2f::mulmod_p(a[0], a[1], a[2]);
    case P3HIP_FP_MULMOD_P_DEV: return p2f::mulmod_p(a[0], a[1], a[0] * pinv);
    case P3HIP_FP_MULMOD_M: return p2f::mulmod_m(a[0], a[1], a[2], mk, npm1);
    case P3HIP_FP_MULMOD_M_DEV: return p2f::mulmod_m(a[0], a[1], a[0] * pinv, mk, npm1);
    case P3HIP_FP_ADD_SCALED_POW2: return p2f::add_scaled_pow2(a[0], a[1], a[2]);
    case P3HIP_FP_SBOX7: return p2f::sbox7(a[0], mk, npm1, pinv);
    case P3HIP_FP_STORE_ELEM: return (double)p2f::store_elem(a[0], mk);
    case P3HIP_FP_MULM: return narrow64::mulm(a[0], a[1], a[2], nk, un.npm1);
    case P3HIP_FP_MULM_DEV: return narrow64::mulm(a[0], a[0] * un.pinv, a[1], nk, un.npm1);
    case P3HIP_FP_WORD_CENTERED: return (double)narrow64::word_centered(a[0]);
    case P3HIP_FP_WORD_ANY: return (double)narrow64::word_any(a[0], un);
    case P3HIP_FP_ADD_SCALED_INT: return p2f::add_scaled_pow2(a[0], a[1], a[2]);  // the same functions, at the operands p2q gives them
    case P3HIP_FP_SBOX7_WIDE: return p2f::sbox7(a[0], mk, npm1, pinv);
    default: return 0.0;
    }
}

// K_MAX / M_MAX: the widest op (extension product: 8 words in, 4 out)
constexpr int K_MAX = 8, M_MAX = 4;

}  // namespace

__global__ void __launch_bounds__(256) field_probe_kernel(int op, int k, int m, int f64, const void* in, void* out, uint64_t n,
                                                           narrow64::Uni un) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (f64) {
        const p2f::MagicRegs mk = p2f::magic_regs();
        const narrow64::Magic nk = narrow64::pin_magic();
        double a[3] = {0.0, 0.0, 0.0};
        const double* src = static_cast<const double*>(in) + i * (uint64_t)k;
        for (int j = 0; j < 3; j++)
            if (j < k) a[j] = src[j];
        static_cast<double*>(out)[i] = probe_f64(op, a, mk, nk, un);
    } else {
        uint32_t a[K_MAX] = {0, 0, 0, 0, 0, 0, 0, 0}, o[M_MAX] = {0, 0, 0, 0};
        const uint32_t* src = static_cast<const uint32_t*>(in) + i * (uint64_t)k;
        for (int j = 0; j < K_MAX; j++)
            if (j < k) a[j] = src[j];
        probe_words(op, a, o);
        uint32_t* dst = static_cast<uint32_t*>(out) + i * (uint64_t)m;
        for (int j = 0; j < M_MAX; j++)
            if (j < m) dst[j] = o[j];
    }
}

constexpr size_t FIELD_PROBE_MAX_LANES = (size_t)1 << 22;

static int check_probe_args(const char* who, int op, const void* in, const void* out, size_t n, const OpInfo** info) {
    *info = find_op(op);
    if (!*info) return fail(ERR_BAD_ARG, std::string(who) + ": unknown op " + std::to_string(op));
    if (n > FIELD_PROBE_MAX_LANES) return fail(ERR_BAD_ARG, std::string(who) + ": at most 2^22 lanes per call, got " + std::to_string(n));
    if (n && (!in || !out)) return fail(ERR_BAD_ARG, std::string(who) + ": null pointer");
    return OK;
}

int field_probe(hipStream_t stream, int op, const void* d_in, void* d_out, size_t n) {
    const OpInfo* o;
    int rc = check_probe_args("field_probe_dev", op, d_in, d_out, n, &o);
    if (rc || !n) return rc;  // a bad argument is refused before the thread's device context is looked up
    if (o->f64 && ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 7u))
        return fail(ERR_BAD_ARG, "field_probe_dev: d_in and d_out of an fp64 op hold doubles and must be 8-byte aligned");
    Context* cx;
    rc = get_context(&cx);
    if (rc) return rc;
    // the uniform operands of the transform's fp64 functions, as ntt.hip passes them to its kernels
    const narrow64::Uni un{-2013265920.0, 1.0 / 2013265921.0, -0.5 + 1.0 / 8589934592.0};
    hipLaunchKernelGGL(field_probe_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, op, o->k, o->m, (int)o->f64, d_in, d_out,
                       (uint64_t)n, un);
    P3_HIP(hipGetLastError());
    return OK;
}

int field_probe_host(int op, const void* in, void* out, size_t n) {
    const OpInfo* o;
    int rc = check_probe_args("field_probe_host", op, in, out, n, &o);
    if (rc) return rc;
    if (o->f64)
        return fail(ERR_BAD_ARG, std::string("field_probe_host: op ") + std::to_string(op) + " (" + o->name +
                                     ") is an fp64 function, __device__ only: no host branch exists");
    const uint32_t* src = static_cast<const uint32_t*>(in);
    uint32_t* dst = static_cast<uint32_t*>(out);
    for (size_t i = 0; i < n; i++) probe_words(op, src + i * o->k, dst + i * o->m);
    return OK;
}

}  // namespace p3
