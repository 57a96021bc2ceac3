// Caller-defined AIRs on gfx950 (include/p3hip.h "caller-defined AIRs"): the step of p3_uni_stark::prove between commit(trace) and
// commit(quotient) — quotient_values — for an AIR the caller describes as a small program, and check_constraints over the trace itself.
//
// The program is a flat list of three-address instructions over per-row value slots; air_create validates ALL of it (every index,
// every read-before-write, every capacity), so the kernels below take no address and no loop bound from the caller unchecked.
// One interpreter serves both kernels: one lane per row, every lane of a wave runs the same instruction, so the program, the
// constants, the public values and the alpha powers are fetched with wave-uniform loads and the operand kind is a scalar branch.
// The value slots are per lane and indexed at run time: they live in LDS, slot-major (slot * AIR_BLOCK + lane: consecutive lanes on
// consecutive banks), never in a per-thread array, which would be placed in scratch.
#include <cstring>
#include <memory>
#include <string>

#include "air.h"
#include "bb31.hip.h"
#include "common.h"

namespace p3 {

using bb::Ext;

namespace {

constexpr uint32_t OPND_INDEX_MASK = (1u << P3HIP_AIR_KIND_SHIFT) - 1u;

__device__ __forceinline__ uint32_t air_tl(const TwoLevelTable& t, uint32_t e) { return bb::mul(t.lo[e & ((1u << t.T) - 1u)], t.hi[e >> t.T]); }
__device__ __forceinline__ uint32_t air_brev(uint32_t v, uint32_t bits) { return bits ? (__brev(v) >> (32 - bits)) : 0u; }

__device__ __forceinline__ uint32_t air_fetch(uint32_t o, const uint32_t* my, const uint32_t* pl, const uint32_t* pn, const uint32_t* __restrict__ tab,
                                              const uint32_t* __restrict__ consts, uint32_t s_first, uint32_t s_last, uint32_t s_trans) {
    const uint32_t idx = o & OPND_INDEX_MASK;
    switch (o >> P3HIP_AIR_KIND_SHIFT) {
        case P3HIP_AIR_KIND_SLOT: return my[idx * AIR_BLOCK];
        case P3HIP_AIR_KIND_LOCAL: return pl[idx];
        case P3HIP_AIR_KIND_NEXT: return pn[idx];
        case P3HIP_AIR_KIND_PUBLIC: return tab[idx];
        case P3HIP_AIR_KIND_CONST: return consts[idx];
        default: return idx == 0 ? s_first : idx == 1 ? s_last : s_trans;
    }
}

struct AirLaunch {
    TwoLevelTable roots;  // g_rows^i (quotient only)
    unsigned long long* found;  // check only: min over failing rows of (row << 32 | constraint)
    uint32_t n_instr, width, rows_n, log_rows, log_qd, gen, ginv;
    uint32_t ap_off, zh_off, ptr_off;  // word offsets into the per-call table
};

// MODE 0: quotient_values over the quotient domain GENERATOR * <g_qn> (rows = the committed LDE, bit-reversed);
// MODE 1: check_constraints over the trace domain (rows = the trace, natural order), no fold.
template <int MODE>
__global__ void __launch_bounds__(AIR_BLOCK) air_kernel(const uint4* __restrict__ code, const uint32_t* __restrict__ consts,
                                                        const uint32_t* __restrict__ tab, const uint32_t* __restrict__ rows, AirLaunch a) {
    extern __shared__ uint32_t air_slots[];
    const uint32_t i = blockIdx.x * AIR_BLOCK + threadIdx.x;
    if (i >= a.rows_n) return;  // no barrier below: a lane's slots are its own
    uint32_t* const my = air_slots + threadIdx.x;
    const uint32_t *pl, *pn;
    uint32_t s_first, s_last, s_trans, zh_inv = 0;
    if (MODE == 0) {
        const uint32_t C = 1u << a.log_qd;
        pl = rows + (size_t)air_brev(i, a.log_rows) * a.width;
        pn = rows + (size_t)air_brev((i + C) & (a.rows_n - 1), a.log_rows) * a.width;
        // selectors_on_coset: x = GENERATOR g_qn^i is in no subgroup of two-power order, so neither denominator vanishes; both are
        // inverted in the lane with ONE field inversion (Montgomery's trick over the pair)
        const uint32_t x = bb::mul(a.gen, air_tl(a.roots, i));
        const uint32_t d0 = bb::sub(x, bb::ONE), d1 = bb::sub(x, a.ginv);
        const uint32_t inv01 = bb::inv(bb::mul(d0, d1));
        const uint32_t c = i & (C - 1);  // Z_H(x_i) = GENERATOR^n w_C^(i mod C) - 1 takes C values: a table of the call
        const uint32_t zh = tab[a.zh_off + c];
        zh_inv = tab[a.zh_off + C + c];
        s_first = bb::mul(zh, bb::mul(inv01, d1));
        s_last = bb::mul(zh, bb::mul(inv01, d0));
        s_trans = d1;
    } else {
        const uint32_t last = a.rows_n - 1;
        pl = rows + (size_t)i * a.width;
        pn = rows + (size_t)((i + 1) & last) * a.width;
        s_first = i == 0 ? bb::ONE : 0u;
        s_last = i == last ? bb::ONE : 0u;
        s_trans = i == last ? 0u : bb::ONE;
    }
    // operands are read where they live; the kind is wave-uniform
#define AIR_FETCH(o) air_fetch(o, my, pl, pn, tab, consts, s_first, s_last, s_trans)
    Ext acc = bb::ext_zero();
    uint32_t pend = 0, k = 0, bad = ~0u;  // k: constraints closed so far (wave-uniform)
    for (uint32_t pc = 0; pc < a.n_instr; pc++) {
        const uint4 ins = code[pc];  // {op, dst, a, b}
        const uint32_t va = AIR_FETCH(ins.z);
        if (ins.x == P3HIP_AIR_OP_ASSERT_ZERO) {
            if (MODE == 0) {
                // the table holds alpha^(K-1-k) at entry k; two constraints share one Montgomery reduction per coefficient
                if (k & 1u) {
                    const uint32_t* ap = tab + a.ap_off + 4 * (k - 1);
#pragma unroll
                    for (int j = 0; j < 4; j++) acc.c[j] = bb::add(acc.c[j], bb::dot2(ap[j], pend, ap[4 + j], va));
                } else {
                    pend = va;
                }
            } else if (va != 0 && bad == ~0u) {
                bad = k;
            }
            k++;
            continue;
        }
        const uint32_t vb = AIR_FETCH(ins.w);
        uint32_t r;
        if (ins.x == P3HIP_AIR_OP_MUL) r = bb::mul(va, vb);
        else if (ins.x == P3HIP_AIR_OP_ADD) r = bb::add(va, vb);
        else r = bb::sub(va, vb);
        my[ins.y * AIR_BLOCK] = r;
    }
    if (MODE == 0) {
        if (k & 1u) {
            const uint32_t* ap = tab + a.ap_off + 4 * (k - 1);
#pragma unroll
            for (int j = 0; j < 4; j++) acc.c[j] = bb::add(acc.c[j], bb::mul(ap[j], pend));
        }
        // chunk c, row r = the quotient at natural row r C + c
        uint32_t* const* chunks = reinterpret_cast<uint32_t* const*>(tab + a.ptr_off);
        uint32_t* out = chunks[i & ((1u << a.log_qd) - 1u)] + 4 * (size_t)(i >> a.log_qd);
        const Ext q = bb::scale(acc, zh_inv);
        *reinterpret_cast<uint4*>(out) = make_uint4(q.c[0], q.c[1], q.c[2], q.c[3]);
    } else if (bad != ~0u) {
        atomicMin(a.found, ((unsigned long long)i << 32) | bad);
    }
#undef AIR_FETCH
}

std::string at(size_t pc) { return "air_create: instruction " + std::to_string(pc) + ": "; }

uint32_t log2_ceil(uint32_t v) {
    uint32_t l = 0;
    while ((1u << l) < v) l++;
    return l;
}

// one operand of instruction pc: its index against the AIR's own sizes, a slot against what has been written; *deg = its degree
int check_operand(const Air& a, size_t pc, const char* which, uint32_t o, const std::vector<uint32_t>& slot_deg, uint32_t* deg) {
    const uint32_t kind = o >> P3HIP_AIR_KIND_SHIFT, idx = o & OPND_INDEX_MASK;
    const std::string w = at(pc) + "operand " + which + ": ";
    switch (kind) {
        case P3HIP_AIR_KIND_SLOT:
            if (idx >= P3HIP_AIR_MAX_SLOTS) return fail(ERR_BAD_ARG, w + "slot " + std::to_string(idx) + " out of range (capacity exceeded: at most " + std::to_string(P3HIP_AIR_MAX_SLOTS) + " slots)");
            if (idx >= slot_deg.size() || slot_deg[idx] == ~0u) return fail(ERR_BAD_ARG, w + "slot " + std::to_string(idx) + " is read before any instruction wrote it");
            *deg = slot_deg[idx];
            return OK;
        case P3HIP_AIR_KIND_LOCAL:
        case P3HIP_AIR_KIND_NEXT:
            if (idx >= a.width) return fail(ERR_BAD_ARG, w + "column " + std::to_string(idx) + " out of range (width " + std::to_string(a.width) + ")");
            *deg = 1;
            return OK;
        case P3HIP_AIR_KIND_PUBLIC:
            if (idx >= a.n_public) return fail(ERR_BAD_ARG, w + "public value " + std::to_string(idx) + " out of range (" + std::to_string(a.n_public) + " public values)");
            *deg = 0;
            return OK;
        case P3HIP_AIR_KIND_CONST:
            if (idx >= a.consts.size()) return fail(ERR_BAD_ARG, w + "constant " + std::to_string(idx) + " out of range (" + std::to_string(a.consts.size()) + " constants)");
            *deg = 0;
            return OK;
        case P3HIP_AIR_KIND_SELECTOR:
            if (idx > P3HIP_AIR_SEL_TRANSITION) return fail(ERR_BAD_ARG, w + "selector " + std::to_string(idx) + " out of range (0 is_first_row, 1 is_last_row, 2 is_transition)");
            *deg = 1;
            return OK;
        default: return fail(ERR_BAD_ARG, w + "unknown kind " + std::to_string(kind));
    }
}

int validate(Air& a) {
    const size_t n_instr = a.code.size() / 4;
    std::vector<uint32_t> slot_deg;  // ~0u: not written yet
    uint32_t n_constraints = 0, max_degree = 0;
    for (size_t pc = 0; pc < n_instr; pc++) {
        const uint32_t op = a.code[4 * pc], dst = a.code[4 * pc + 1], oa = a.code[4 * pc + 2], ob = a.code[4 * pc + 3];
        if (op > P3HIP_AIR_OP_ASSERT_ZERO) return fail(ERR_BAD_ARG, at(pc) + "unknown opcode " + std::to_string(op));
        uint32_t da = 0, db = 0;
        int rc = check_operand(a, pc, "a", oa, slot_deg, &da);
        if (rc) return rc;
        if (op == P3HIP_AIR_OP_ASSERT_ZERO) {
            if (dst || ob) return fail(ERR_BAD_ARG, at(pc) + "assert_zero takes one operand: the dst and b words must be 0");
            if (n_constraints == P3HIP_AIR_MAX_CONSTRAINTS) return fail(ERR_BAD_ARG, at(pc) + "capacity exceeded: at most " + std::to_string(P3HIP_AIR_MAX_CONSTRAINTS) + " constraints");
            if (da > P3HIP_AIR_MAX_DEGREE)
                return fail(ERR_BAD_ARG, at(pc) + "capacity exceeded: constraint " + std::to_string(n_constraints) + " has degree " + (da >= AIR_DEGREE_SATURATED ? ">= " : "") +
                                             std::to_string(da) + ", at most " + std::to_string(P3HIP_AIR_MAX_DEGREE) + " (a commitment holds at most " + std::to_string(AIR_MAX_CHUNKS) + " quotient chunks)");
            n_constraints++;
            if (da > max_degree) max_degree = da;
            continue;
        }
        if ((rc = check_operand(a, pc, "b", ob, slot_deg, &db))) return rc;
        if (dst >= P3HIP_AIR_MAX_SLOTS) return fail(ERR_BAD_ARG, at(pc) + "slot " + std::to_string(dst) + " out of range (capacity exceeded: at most " + std::to_string(P3HIP_AIR_MAX_SLOTS) + " slots)");
        if (dst >= slot_deg.size()) slot_deg.resize(dst + 1, ~0u);
        const uint32_t d = op == P3HIP_AIR_OP_MUL ? da + db : (da > db ? da : db);
        slot_deg[dst] = d < AIR_DEGREE_SATURATED ? d : AIR_DEGREE_SATURATED;
    }
    if (!n_constraints) return fail(ERR_BAD_ARG, "air_create: zero constraints: the program asserts nothing");
    a.n_constraints = n_constraints;
    a.n_slots = (uint32_t)slot_deg.size();
    a.max_degree = max_degree;
    a.log_quotient_degree = log2_ceil((max_degree > 2 ? max_degree : 2) - 1);
    return OK;
}

int check_words(const uint32_t* w, size_t n, const std::string& what) {
    for (size_t i = 0; i < n; i++)
        if (w[i] >= bb::P) return fail(ERR_BAD_ARG, what + " " + std::to_string(i) + " is not a canonical field element");
    return OK;
}

// makes the AIR's device current for the call
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    int enter(int dev) {
        P3_HIP(hipGetDevice(&prev));
        if (prev != dev) {
            P3_HIP(hipSetDevice(dev));
            switched = true;
        }
        return OK;
    }
    ~DeviceScope() {
        if (switched) (void)hipSetDevice(prev);
    }
};

template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        return fail(ERR_INTERNAL, std::string("exception: ") + e.what());
    } catch (...) {
        return fail(ERR_INTERNAL, "unknown exception");
    }
}

// the device copies are made by the first device call: creation, info and eval_ext are host code and need no GPU
int ensure_device(Air& a) {
    if (a.d_code) return OK;
    P3_HIP(hipGetDevice(&a.device));
    const size_t code_w = a.code.size(), const_w = (a.consts.size() + 3) & ~(size_t)3;
    // per-call table: publics | K alpha powers | Z_H, 1 / Z_H | (8-byte aligned) chunk pointers
    a.tab_words = ((a.n_public + 4 * (size_t)a.n_constraints + 2 * AIR_MAX_CHUNKS + 3) & ~(size_t)3) + 2 * AIR_MAX_CHUNKS;
    uint32_t* block = nullptr;
    P3_HIP(hipMalloc(reinterpret_cast<void**>(&block), (code_w + const_w + a.tab_words + 4) * 4));
    hipError_t e = hipMemcpy(block, a.code.data(), code_w * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !a.consts.empty()) e = hipMemcpy(block + code_w, a.consts.data(), a.consts.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(block);
        return fail(ERR_HIP, std::string("air: upload of the program: ") + hipGetErrorString(e));
    }
    hipEvent_t done = nullptr, ran = nullptr;
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&a.h_pin), a.tab_words * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ran, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(block);
        if (a.h_pin) (void)hipHostFree(a.h_pin);
        if (done) (void)hipEventDestroy(done);
        a.h_pin = nullptr;
        return fail(ERR_HIP, std::string("air: staging of the per-call table: ") + hipGetErrorString(e));
    }
    a.up_done = done;
    a.run_done = ran;
    a.d_code = block;
    a.d_consts = block + code_w;
    a.d_tab = a.d_consts + const_w;
    a.d_found = reinterpret_cast<unsigned long long*>(a.d_tab + a.tab_words);
    return OK;
}

// d_tab and d_found are the object's, reused in stream order: a call on another stream than the last one's is ordered behind that
// call's kernel before it writes either.  On one stream this is no operation.
int order_behind_last_call(Air& a, hipStream_t st) {
    if (a.ran && a.last_stream != (void*)st) P3_HIP(hipStreamWaitEvent(st, (hipEvent_t)a.run_done, 0));
    return OK;
}

// the kernel alone, on table `tab` (the object's own d_tab, or a table its owner keeps and has filled in stream order: AirProver)
int launch_kernel(Air& a, int mode, hipStream_t st, const uint32_t* tab, const uint32_t* rows, AirLaunch& la) {
    Context* cx;
    int rc = get_context(&cx);
    if (rc) return rc;
    if (mode == 0 && (rc = cx->get_root_table(st, la.log_rows, false, &la.roots))) return rc;
    const void* kernel = mode == 0 ? reinterpret_cast<const void*>(&air_kernel<0>) : reinterpret_cast<const void*>(&air_kernel<1>);
    if ((rc = cx->ensure_dynamic_lds(kernel, P3HIP_AIR_MAX_SLOTS * AIR_BLOCK * 4))) return rc;
    const uint32_t lds = a.n_slots * AIR_BLOCK * 4;
    const dim3 grid((la.rows_n + AIR_BLOCK - 1) / AIR_BLOCK), block(AIR_BLOCK);
    const uint4* code = reinterpret_cast<const uint4*>(a.d_code);
    if (mode == 0) hipLaunchKernelGGL(air_kernel<0>, grid, block, lds, st, code, a.d_consts, tab, rows, la);
    else hipLaunchKernelGGL(air_kernel<1>, grid, block, lds, st, code, a.d_consts, tab, rows, la);
    P3_HIP(hipGetLastError());
    return OK;
}

int launch(Air& a, int mode, hipStream_t st, const uint32_t* rows, AirLaunch& la) {
    int rc;
    if ((rc = order_behind_last_call(a, st))) return rc;
    // the upload reads pinned staging of the object's; the event behind it says when the staging may be written again (a wait that
    // ends at once unless the previous call's upload has not run yet).  d_tab itself is reused in stream order.
    if (a.h_tab.size() > a.tab_words) return fail(ERR_INTERNAL, "air: the per-call table outgrew its buffer");
    hipEvent_t done = (hipEvent_t)a.up_done;
    P3_HIP(hipEventSynchronize(done));
    memcpy(a.h_pin, a.h_tab.data(), a.h_tab.size() * 4);
    P3_HIP(hipMemcpyAsync(a.d_tab, a.h_pin, a.h_tab.size() * 4, hipMemcpyHostToDevice, st));
    P3_HIP(hipEventRecord(done, st));
    if ((rc = launch_kernel(a, mode, st, a.d_tab, rows, la))) return rc;
    P3_HIP(hipEventRecord((hipEvent_t)a.run_done, st));
    a.last_stream = (void*)st;
    a.ran = true;
    return OK;
}

// the quotient launch's figures and the table's offsets for 2^log_n rows (roots: set by launch_kernel)
AirLaunch quotient_launch(const Air& a, uint32_t log_n) {
    const uint32_t lqd = a.log_quotient_degree, C = 1u << lqd, log_qn = log_n + lqd;
    AirLaunch la{};
    la.n_instr = (uint32_t)(a.code.size() / 4);
    la.width = a.width;
    la.rows_n = 1u << log_qn;
    la.log_rows = log_qn;
    la.log_qd = lqd;
    la.gen = bb::to_monty(bb::GEN);
    la.ginv = bb::inv(bb::two_adic_generator(log_n));
    la.ap_off = a.n_public;
    la.zh_off = la.ap_off + 4 * a.n_constraints;
    la.ptr_off = (la.zh_off + 2 * C + 3) & ~3u;
    return la;
}

}  // namespace

int air_ensure_device(Air& a) { return ensure_device(a); }

AirTable air_table(const Air& a, uint32_t log_n) {
    const AirLaunch la = quotient_launch(a, log_n);
    return AirTable{la.ap_off, la.zh_off, la.ptr_off + 2u * (1u << a.log_quotient_degree)};
}

void air_table_tail(const Air& a, uint32_t log_n, uint32_t* const* d_chunks, uint32_t* tail) {
    const AirLaunch la = quotient_launch(a, log_n);
    const uint32_t C = 1u << a.log_quotient_degree;
    memset(tail, 0, (la.ptr_off + 2 * C - la.zh_off) * 4);
    const uint32_t gn = bb::pow(la.gen, 1u << log_n), wc = bb::two_adic_generator(a.log_quotient_degree);
    uint32_t w = bb::ONE;
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t zh = bb::sub(bb::mul(gn, w), bb::ONE);  // nonzero: GENERATOR^n w is no two-power root of unity
        tail[c] = zh;
        tail[C + c] = bb::inv(zh);
        w = bb::mul(w, wc);
    }
    memcpy(tail + (la.ptr_off - la.zh_off), d_chunks, C * sizeof(uint32_t*));
    static_assert(sizeof(uint32_t*) == 8, "chunk pointers take two words");
}

int air_quotient_launch(Air& a, hipStream_t st, const uint32_t* d_tab, const uint32_t* d_lde, uint32_t log_n) {
    AirLaunch la = quotient_launch(a, log_n);
    return launch_kernel(a, 0, st, d_tab, d_lde, la);
}

int air_check_trace(Air& a, hipStream_t st, const uint32_t* d_trace, uint32_t log_n, const uint32_t* pis, long long* row_out, int* constraint_out) {
    int rc;
    if ((rc = ensure_device(a))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(a.device))) return rc;
    AirLaunch la{};
    la.n_instr = (uint32_t)(a.code.size() / 4);
    la.width = a.width;
    la.rows_n = 1u << log_n;
    la.log_rows = log_n;
    la.found = a.d_found;
    std::vector<uint32_t>& tab = a.h_tab;
    tab.assign(a.n_public ? a.n_public : 1, 0);
    if (a.n_public) memcpy(tab.data(), pis, a.n_public * 4);
    if ((rc = order_behind_last_call(a, st))) return rc;
    P3_HIP(hipMemsetAsync(a.d_found, 0xff, 8, st));
    if ((rc = launch(a, 1, st, d_trace, la))) return rc;
    unsigned long long found = 0;
    P3_HIP(hipMemcpyAsync(&found, a.d_found, 8, hipMemcpyDeviceToHost, st));
    P3_HIP(hipStreamSynchronize(st));
    *row_out = found == ~0ull ? -1 : (long long)(found >> 32);
    *constraint_out = found == ~0ull ? -1 : (int)(found & 0xffffffffu);
    return OK;
}

Air::~Air() {
    if (d_code) (void)hipFree(d_code);  // waits for the device: an enqueued upload or kernel of this object has run when it returns
    if (h_pin) (void)hipHostFree(h_pin);
    if (up_done) (void)hipEventDestroy((hipEvent_t)up_done);
    if (run_done) (void)hipEventDestroy((hipEvent_t)run_done);
}

}  // namespace p3

using namespace p3;

extern "C" {

int p3hip_air_create(size_t width, size_t n_public, const uint32_t* code, size_t n_instr, const uint32_t* consts, size_t n_consts,
                     p3hip_air_t** out) {
    return guarded([&]() -> int {
        if (!out || (!code && n_instr) || (!consts && n_consts)) return fail(ERR_BAD_ARG, "air_create: null argument");
        if (width < 1 || width > P3HIP_AIR_MAX_WIDTH) return fail(ERR_BAD_ARG, "air_create: width " + std::to_string(width) + ": a trace has 1 to " + std::to_string(P3HIP_AIR_MAX_WIDTH) + " columns");
        if (n_public > P3HIP_AIR_MAX_PUBLIC) return fail(ERR_BAD_ARG, "air_create: capacity exceeded: " + std::to_string(n_public) + " public values, at most " + std::to_string(P3HIP_AIR_MAX_PUBLIC));
        if (n_consts > P3HIP_AIR_MAX_CONSTS) return fail(ERR_BAD_ARG, "air_create: capacity exceeded: " + std::to_string(n_consts) + " constants, at most " + std::to_string(P3HIP_AIR_MAX_CONSTS));
        if (n_instr > P3HIP_AIR_MAX_INSTRUCTIONS) return fail(ERR_BAD_ARG, "air_create: capacity exceeded: " + std::to_string(n_instr) + " instructions, at most " + std::to_string(P3HIP_AIR_MAX_INSTRUCTIONS));
        int rc = check_words(consts, n_consts, "air_create: constant");
        if (rc) return rc;
        std::unique_ptr<p3hip_air> p(new p3hip_air());
        Air& a = p->a;
        a.width = (uint32_t)width;
        a.n_public = (uint32_t)n_public;
        a.code.assign(code, code + 4 * n_instr);
        a.consts.assign(consts, consts + n_consts);
        if ((rc = validate(a))) return rc;
        *out = p.release();
        return OK;
    });
}

void p3hip_air_destroy(p3hip_air_t* air) { delete air; }

int p3hip_air_info(const p3hip_air_t* air, p3hip_air_info_t* out) {
    return guarded([&]() -> int {
        if (!air || !out) return fail(ERR_BAD_ARG, "air_info: null argument");
        const Air& a = air->a;
        *out = p3hip_air_info_t{a.width, a.n_public, (uint32_t)(a.code.size() / 4), a.n_constraints, a.n_slots, a.max_degree, a.log_quotient_degree};
        return OK;
    });
}

int p3hip_air_quotient_dev(p3hip_air_t* air, void* stream, const uint32_t* d_lde, unsigned log_n, unsigned log_blowup, const uint32_t* pis,
                           const uint32_t alpha[4], uint32_t* const* d_chunks_out) {
    return guarded([&]() -> int {
        if (!air || !d_lde || !alpha || !d_chunks_out || (!pis && air->a.n_public)) return fail(ERR_BAD_ARG, "air_quotient: null argument");
        Air& a = air->a;
        const uint32_t lqd = a.log_quotient_degree, C = 1u << lqd, K = a.n_constraints;
        if (log_n < 1) return fail(ERR_BAD_ARG, "air_quotient: log_n must be >= 1");
        if (log_blowup < lqd)
            return fail(ERR_BAD_ARG, "air_quotient: log_blowup " + std::to_string(log_blowup) + " is below log_quotient_degree " + std::to_string(lqd) +
                                         ": the committed LDE does not cover the quotient domain");
        if (log_n + log_blowup > bb::TWO_ADICITY) return fail(ERR_BAD_ARG, "air_quotient: log_n + log_blowup exceeds the two-adicity 27");
        if ((uintptr_t)d_lde & 3) return fail(ERR_BAD_ARG, "air_quotient: the LDE must be 4-byte aligned");
        int rc;
        if ((rc = check_words(pis, a.n_public, "air_quotient: public value"))) return rc;
        if ((rc = check_words(alpha, 4, "air_quotient: alpha word"))) return rc;
        for (uint32_t c = 0; c < C; c++)
            if (!d_chunks_out[c] || ((uintptr_t)d_chunks_out[c] & 15)) return fail(ERR_BAD_ARG, "air_quotient: chunk " + std::to_string(c) + " must be a 16-byte aligned device pointer");
        if ((rc = ensure_device(a))) return rc;
        DeviceScope scope;
        if ((rc = scope.enter(a.device))) return rc;
        AirLaunch la = quotient_launch(a, log_n);
        std::vector<uint32_t>& tab = a.h_tab;
        tab.assign(la.ptr_off + 2 * C, 0);
        if (a.n_public) memcpy(tab.data(), pis, a.n_public * 4);
        Ext al, p = bb::ext_one();
        memcpy(al.c, alpha, 16);
        for (uint32_t k = K; k-- > 0;) {  // entry k = alpha^(K-1-k): the first constraint takes the highest power
            memcpy(&tab[la.ap_off + 4 * k], p.c, 16);
            p = bb::mul(p, al);
        }
        air_table_tail(a, log_n, d_chunks_out, &tab[la.zh_off]);
        return launch(a, 0, (hipStream_t)stream, d_lde, la);
    });
}

int p3hip_air_check_trace_dev(p3hip_air_t* air, void* stream, const uint32_t* d_trace, unsigned log_n, const uint32_t* pis,
                              long long* row_out, int* constraint_out) {
    return guarded([&]() -> int {
        if (!air || !d_trace || !row_out || !constraint_out || (!pis && air->a.n_public)) return fail(ERR_BAD_ARG, "air_check_trace: null argument");
        Air& a = air->a;
        if (log_n < 1 || log_n > bb::TWO_ADICITY) return fail(ERR_BAD_ARG, "air_check_trace: log_n must lie in 1..27");
        if ((uintptr_t)d_trace & 3) return fail(ERR_BAD_ARG, "air_check_trace: the trace must be 4-byte aligned");
        int rc;
        if ((rc = check_words(pis, a.n_public, "air_check_trace: public value"))) return rc;
        return air_check_trace(a, (hipStream_t)stream, d_trace, log_n, pis, row_out, constraint_out);
    });
}

int p3hip_air_eval_ext(const p3hip_air_t* air, const uint32_t* local, const uint32_t* next, const uint32_t* pis, const uint32_t* sels,
                       const uint32_t alpha[4], uint32_t out[4]) {
    return guarded([&]() -> int {
        if (!air || !local || !next || !sels || !alpha || !out || (!pis && air->a.n_public)) return fail(ERR_BAD_ARG, "air_eval_ext: null argument");
        const Air& a = air->a;
        int rc;
        if ((rc = check_words(local, 4 * (size_t)a.width, "air_eval_ext: local word"))) return rc;
        if ((rc = check_words(next, 4 * (size_t)a.width, "air_eval_ext: next word"))) return rc;
        if ((rc = check_words(pis, a.n_public, "air_eval_ext: public value"))) return rc;
        if ((rc = check_words(sels, 12, "air_eval_ext: selector word"))) return rc;
        if ((rc = check_words(alpha, 4, "air_eval_ext: alpha word"))) return rc;
        auto ld = [](const uint32_t* p) { return Ext{{p[0], p[1], p[2], p[3]}}; };
        std::vector<Ext> slots(a.n_slots, bb::ext_zero());
        auto fetch = [&](uint32_t o) -> Ext {
            const uint32_t idx = o & OPND_INDEX_MASK;
            switch (o >> P3HIP_AIR_KIND_SHIFT) {
                case P3HIP_AIR_KIND_SLOT: return slots[idx];
                case P3HIP_AIR_KIND_LOCAL: return ld(local + 4 * idx);
                case P3HIP_AIR_KIND_NEXT: return ld(next + 4 * idx);
                case P3HIP_AIR_KIND_PUBLIC: return bb::ext_from_base(pis[idx]);
                case P3HIP_AIR_KIND_CONST: return bb::ext_from_base(a.consts[idx]);
                default: return ld(sels + 4 * idx);
            }
        };
        const Ext al = ld(alpha);
        Ext acc = bb::ext_zero();
        for (size_t pc = 0; pc < a.code.size() / 4; pc++) {
            const uint32_t* ins = &a.code[4 * pc];
            const Ext va = fetch(ins[2]);
            if (ins[0] == P3HIP_AIR_OP_ASSERT_ZERO) {
                acc = bb::add(bb::mul(acc, al), va);  // VerifierConstraintFolder: Horner
                continue;
            }
            const Ext vb = fetch(ins[3]);
            slots[ins[1]] = ins[0] == P3HIP_AIR_OP_MUL ? bb::mul(va, vb) : ins[0] == P3HIP_AIR_OP_ADD ? bb::add(va, vb) : bb::sub(va, vb);
        }
        memcpy(out, acc.c, 16);
        return OK;
    });
}

}  // extern "C"
