/* libp3hip — C ABI of the MI355X (gfx950) backend for the fib_air NTT/LDE + Poseidon2-MMCS path.
 *
 * The reference (miha-stopar/Plonky3-mobile) has no C ABI: its plug points are Rust traits and five
 * JNI exports.  Every entry point below names the reference interface it stands in
 * for, so a Rust `backend_hip.rs` (same shape as native/src/backend_metal.rs:5-10) and a
 * `HipMmcs: Mmcs<BabyBear>` can bind them with `extern "C"`; INTEGRATION.md shows those stubs.
 *
 * Conventions (carried over from the reference):
 *   - values are u32 BabyBear Montgomery words in [0, P), P = 0x78000001 — `to_unique_u32`
 *     (native/src/backend_vulkan.rs:2002-2005); matrices are row-major height x width;
 *   - every function returns 0 on success or a negative P3HIP_ERR_* code and NEVER aborts; the message
 *     goes to a per-thread take-and-clear mailbox (native/src/gpu_dft.rs:42,65-68);
 *   - device state (cached tables, scratch) belongs to the (calling thread, current device) pair and is created on
 *     first use (native/src/backend_vulkan.rs:100-124: the reference's runtime is thread-local too).  A thread that
 *     switches device (hipSetDevice) simply gets that device's own context; objects that own HBM (trees, provers)
 *     remember their device and return P3HIP_ERR_BAD_ARG when used with another one current;
 *   - there is NO CPU fallback inside this library: on error the caller decides (the Rust GpuDft keeps
 *     its own Radix2DitParallel fallback, native/src/gpu_dft.rs:100-112).
 *   - `*_dev` variants take HBM pointers (hipMalloc / p3hip_malloc / a torch tensor's data_ptr) and a
 *     hipStream_t passed as void*; they enqueue and return without synchronising.  STREAM CONTRACT: any number of
 *     streams may be used from one thread, also interleaved — intermediates live in scratch keyed by (thread, stream),
 *     tables built at first use are filled by a kernel on the calling stream and guarded by an event for the others.
 *     The exceptions to "enqueue only": the very first call of a thread on a device builds its context (blocking),
 *     a scratch slab that has to GROW is reallocated after a device synchronise, and so is the bounded table cache
 *     once a thread has used more than 256 distinct (shift, height) pairs.  A given stream must not be used from two
 *     threads at once with buffers that alias.
 *   - BUFFER CONTRACT of the `*_dev` entries (the Rust side hands in pointers into the middle of allocations,
 *     integration/native/src/hip_matrix.rs; tests/test_gpu_buffer_contract.py pins every line of it, DESIGN.md "Test strategy" has
 *     the table pointer by pointer).  Unless an entry says otherwise:
 *       ALIGNMENT  every device pointer needs the 4 bytes of its words and no more.  Where a kernel moves wider pieces it either
 *                  checks the address and takes a word-wise kernel otherwise (any 4-byte alignment is in the contract, both sides
 *                  are tested), or the entry STATES the alignment and refuses a pointer that lacks it with P3HIP_ERR_BAD_ARG and a
 *                  message naming the argument, on the host, before anything is launched or drawn.
 *       READ-ONLY  a `const` pointer is read in place: no copy is made and no word of it is written; the caller keeps it unchanged
 *                  until the work that reads it has completed on the stream.
 *       EXTENT     an output is written exactly over the words its comment gives (rows x width, n statuses, ...): not a word before
 *                  the pointer and not a word past the last one, whatever the launch geometry rounds up to.
 *       ALIASING   an input and an output must not share a word, with one exception: p3hip_dft_batch_bb31_dev and
 *                  p3hip_idft_batch_bb31_dev accept d_out == d_in (the input is staged in the stream's scratch).  The six transform
 *                  entries and p3hip_bit_reverse_rows_dev refuse two ranges that overlap without being identical, and all but dft /
 *                  idft refuse identical ones (heights above one row), with P3HIP_ERR_BAD_ARG and nothing written.  For every other
 *                  entry overlapping arguments are undefined.
 *     Stated alignments (everything else: 4 bytes): p3hip_fib_trace_dev d_out 8; p3hip_fib_check_trace_dev,
 *     p3hip_fib_prover_prove_trace_dev, p3hip_fib_prover_enqueue_trace_dev, p3hip_fib_batch_prove_traces_dev d_trace 8;
 *     p3hip_keccak_f_dev, p3hip_keccak_f_variant_dev d_states 8; p3hip_poseidon2_permute_variant_dev d_states 16 (variant 3: 4);
 *     p3hip_mmcs_commit_into_dev d_layers 16; p3hip_mmcs_verify_batch_many*_dev d_paths 16; p3hip_air_quotient_dev d_chunks_out[c]
 *     16; p3hip_pcs_verifier_verify_dev d_chal_in, d_chal_out 8; the buffers of doubles of the diagnostic probes 8
 *     (p3hip_poseidon2_f64_probe_dev d_in; p3hip_field_probe_dev d_in and d_out of the fp64 ops).
 */
#ifndef P3HIP_H
#define P3HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3HIP_OK 0
#define P3HIP_ERR_BAD_ARG (-1)  /* null pointer, non power-of-two height (backend_vulkan.rs:1992-1995), ... */
#define P3HIP_ERR_HIP (-2)      /* HIP runtime failure; text via p3hip_take_last_error */
#define P3HIP_ERR_BACKEND (-3)  /* unknown backend name (gpu_dft.rs:59) */
#define P3HIP_ERR_INTERNAL (-4)

/* BackendKind codes: gpu_dft.rs:14-40 (Cpu=0, Vulkan=1, Metal=2, WebGpu=3) plus the new Hip=4. */
#define P3HIP_BACKEND_CPU 0
#define P3HIP_BACKEND_VULKAN 1
#define P3HIP_BACKEND_METAL 2
#define P3HIP_BACKEND_WEBGPU 3
#define P3HIP_BACKEND_HIP 4

/* ---- selector + diagnostics -------------------------------------------------------------------- */
/* set_backend_kind_from_str (gpu_dft.rs:53-63) behind JNI setBackend (lib.rs:133-146): case-insensitive
 * "cpu" | "vulkan" | "metal" | "webgpu" | "hip"; unknown -> P3HIP_ERR_BACKEND, message "unknown backend '<x>'".
 * Process-global relaxed atomic, default P3HIP_BACKEND_HIP. */
int p3hip_set_backend(const char *name);
/* get_backend_kind (gpu_dft.rs:49-51) */
int p3hip_get_backend(void);
/* is_vulkan_available (backend_vulkan.rs:726-731) behind JNI isVulkanAvailable (lib.rs:167-179): creates
 * the context; writes "HIP available: <device>" or "HIP unavailable: <error>" into msg. Returns 0 if usable. */
int p3hip_is_available(char *msg, size_t cap);
/* take_last_vulkan_error (gpu_dft.rs:65-68): returns the calling thread's pending message and clears it;
 * NULL when there is none.  The pointer stays valid until the next call on the same thread. */
const char *p3hip_take_last_error(void);

/* ---- device memory helpers for FFI callers that do not link HIP themselves ---------------------- */
int p3hip_malloc(void **dev_ptr, size_t bytes);
int p3hip_free(void *dev_ptr);
int p3hip_upload(void *dev_dst, const void *host_src, size_t bytes);
int p3hip_download(void *host_dst, const void *dev_src, size_t bytes);
int p3hip_sync(void *stream);
/* Frees the calling thread's device state (tables, scratch) on every device it used, after synchronising them.
 * Optional: worker threads that are about to exit call it so that nothing is left behind in HBM. */
void p3hip_release_thread_context(void);

/* ---- TwoAdicSubgroupDft<BabyBear> --------------------------------------------------------------- */
/* backend_vulkan::dft_batch (backend_vulkan.rs:1988-2063) / setup_vulkan_pipeline_plan (:1028-1031):
 * natural row order in, natural row order out, out[k][c] = sum_i in[i][c] w^(ik).  Host pointers:
 * upload, kernels, download, synchronise — the reference's "e2e" view (fib_air.rs:148-157). */
int p3hip_dft_batch_bb31(const uint32_t *in, uint32_t *out, size_t height, size_t width);
/* TwoAdicSubgroupDft::idft_batch [upstream provided method; SURVEY.md §8a R9] */
int p3hip_idft_batch_bb31(const uint32_t *in, uint32_t *out, size_t height, size_t width);
/* TwoAdicSubgroupDft::coset_dft_batch: coefficients -> evaluations over shift*<g>, natural order */
int p3hip_coset_dft_batch_bb31(const uint32_t *in, uint32_t *out, size_t height, size_t width,
                               uint32_t shift_monty);
/* TwoAdicSubgroupDft::coset_lde_batch (+ the `.bit_reverse_rows()` TwoAdicFriPcs::commit applies when
 * bit_reversed_out != 0).  out has (height << added_bits) rows. */
int p3hip_coset_lde_batch_bb31(const uint32_t *in, uint32_t *out, size_t height, size_t width,
                               unsigned added_bits, uint32_t shift_monty, int bit_reversed_out);
/* The reference logs one line per DFT call (backend_vulkan.rs:1385-1423: upload / stages / readback / total, plus the GPU
 * timestamps).  The host-pointer entry points above keep the same line — "hip dft: op=.. h=.. w=.. stages=..
 * upload=..ms stages=..ms readback=..ms total=..ms gpu(stage=..ms copy_back=..ms total=..ms)" — for the calling thread's
 * last call (NULL before the first); with P3HIP_LOG_TIMING=1 it is also written to stderr like the reference's. */
const char *p3hip_last_timing_line(void);
/* device-resident forms — the reference's "kernel-only" view (backend_vulkan.rs:1428-1693).
 * BUFFER CONTRACT (all six, and p3hip_bit_reverse_rows_dev): d_in / d_coeffs height x width words, read-only, any 4-byte alignment;
 * d_out exactly (height, or height << added_bits) x width words, any 4-byte alignment (the three-launch plan of narrow LDEs moves
 * 8-byte pieces and is taken only when both pointers are 8-byte aligned: the general plans serve the same shape otherwise).  dft and
 * idft accept d_out == d_in; every other overlap of the two ranges is refused (conventions above). */
int p3hip_dft_batch_bb31_dev(const uint32_t *d_in, uint32_t *d_out, size_t height, size_t width, void *stream);
int p3hip_idft_batch_bb31_dev(const uint32_t *d_in, uint32_t *d_out, size_t height, size_t width, void *stream);
int p3hip_coset_dft_batch_bb31_dev(const uint32_t *d_in, uint32_t *d_out, size_t height, size_t width,
                                   uint32_t shift_monty, void *stream);
int p3hip_coset_lde_batch_bb31_dev(const uint32_t *d_in, uint32_t *d_out, size_t height, size_t width,
                                   unsigned added_bits, uint32_t shift_monty, int bit_reversed_out,
                                   void *stream);
/* The same extension when the caller already holds COEFFICIENTS (natural order, `height` rows = the degree bound) instead of
 * evaluations: rows of d_out = evaluations over shift*<g_{height << added_bits}> in bit-reversed order, i.e.
 * TwoAdicSubgroupDft::coset_dft_batch of the zero-padded coefficient matrix followed by bit_reverse_rows, without transforming
 * to the subgroup and back (HidingFriPcs commits its blinded quotient chunks from coefficients, fib_air.rs:64-65). */
int p3hip_coset_lde_from_coeffs_bb31_dev(const uint32_t *d_coeffs, uint32_t *d_out, size_t height, size_t width,
                                         unsigned added_bits, uint32_t shift_monty, void *stream);
/* prepare_compute_plan (backend_vulkan.rs:959-975): the reference's VulkanComputePlan carries, next to the stage parameters, the
 * LAUNCH GEOMETRY of its plan (`dispatch`: workgroup counts of one stage; the host then loops log2(height) such dispatches,
 * :1182-1294).  The hip backend's plan for dft_batch / idft_batch of a height x width matrix is a handful of LDS-tiled passes:
 * *n_passes = kernel launches, stages_per_pass[i] = radix-2 stages pass i performs (their sum is log2 height; at most `cap` entries
 * are written).  Host-only: no GPU is touched. */
int p3hip_dft_plan_bb31(size_t height, size_t width, uint32_t *stages_per_pass, size_t cap, size_t *n_passes);
/* The LAUNCH LIST of p3hip_mmcs_commit* for a commitment under a hash (P3HIP_HASH_*) and a profile (P3HIP_PROFILE_*): steps[0] is
 * the kernel that hashes the tallest matrices into the leaf layer (layer = levels = 0), every further step one launch that reads
 * digest layer `layer` (0 = leaves) and writes the `levels` layers above it; makes_root: the last of them is the root.  The choice
 * depends on addresses only through their alignment: mats (or an entry of it) and layers are never dereferenced, NULL = aligned;
 * strides (words between two rows) NULL = dense.  At most `cap` steps are written, *n_steps is their number (<=
 * P3HIP_MMCS_MAX_STEPS).  A shape the commit refuses is refused here with the same message.  Host-only: no GPU is touched. */
enum p3hip_mmcs_kernel {
    P3HIP_MK_LEAF_COOP, P3HIP_MK_LEAF_HASH_Q4, P3HIP_MK_LEAF_HASH_F64_WIDE, P3HIP_MK_LEAF_HASH_F64, P3HIP_MK_LEAF_HASH_F64_ROWSET,
    P3HIP_MK_LEAF_HASH, P3HIP_MK_TREE_LEVELS_COOP, P3HIP_MK_COMPRESS_LAYER_Q4, P3HIP_MK_COMPRESS_LAYER_F64, P3HIP_MK_COMPRESS_LAYER,
    P3HIP_MK_KECCAK_LEAF_WIDE, P3HIP_MK_KECCAK_LEAF_SALTED_4_1, P3HIP_MK_KECCAK_LEAF_SALTED_6_1, P3HIP_MK_KECCAK_LEAF_SALTED_8_1,
    P3HIP_MK_KECCAK_LEAF_SALTED_4_4, P3HIP_MK_KECCAK_LEAF, P3HIP_MK_KECCAK_TREE_LEVELS_COOP, P3HIP_MK_KECCAK_TREE_LEVELS,
    P3HIP_MK_KECCAK_COMPRESS, P3HIP_MK_COUNT
};
typedef struct p3hip_mmcs_step {
    int kernel; /* enum p3hip_mmcs_kernel */
    uint32_t layer, levels, makes_root;
} p3hip_mmcs_step;
#define P3HIP_MMCS_MAX_STEPS 64 /* the leaf step and one per layer above the leaves, whatever power of two a size_t height is */
int p3hip_mmcs_commit_plan(int hash, int profile, const uint32_t *const *mats, const size_t *heights, const size_t *widths,
                           const size_t *strides, size_t n_mats, const uint32_t *layers, p3hip_mmcs_step *steps, size_t cap,
                           size_t *n_steps);
const char *p3hip_mmcs_kernel_name(int kernel); /* "leaf_coop" .. "keccak_leaf_salted<4,4>" .. "keccak_compress"; NULL if unknown */
/* write_bit_reversed_rows_u32 (backend_vulkan.rs:1005-1026) on device; out of place only (any overlap of the ranges is refused) */
int p3hip_bit_reverse_rows_dev(const uint32_t *d_in, uint32_t *d_out, size_t height, size_t width, void *stream);

/* ---- FibonacciAir workload (native/src/fib_air.rs:224-306) --------------------------------------- */
/* generate_trace_rows (fib_air.rs:266-284): n x 2 trace, row 0 = (a, b), row i = (right, left + right);
 * n must be a power of two (fib_air.rs:267).  d_out: exactly 2 n words, 8-byte aligned (rows are stored as pairs; refused otherwise). */
int p3hip_fib_trace_dev(uint64_t a, uint64_t b, size_t n, uint32_t *d_out, void *stream);

/* ---- Poseidon2-BabyBear-16 (default_babybear_poseidon2_16, native/src/poseidon_cpu.rs:17-18) ----- */
/* n independent width-16 states, in place: exactly 16 n words are read and written.  d_states: any 4-byte alignment (16-byte-aligned
 * states run the per-lane fp64 form, which moves 16-byte pieces; any other alignment the 16-lane form, which moves words). */
int p3hip_poseidon2_permute_dev(uint32_t *d_states, size_t n, void *stream);
int p3hip_poseidon2_permute(uint32_t *states, size_t n);
/* The permutation exists in four forms that must agree word for word: int32 Montgomery, one state per lane (variant 0); exact
 * integer arithmetic in fp64, one state per lane (variant 1: what the large tree layers run); the fp64 arithmetic with one state
 * per DPP quad (variant 2: layers of 2^12 .. 2^15 digests under the latency profile); int32 with one state per 16-lane row (variant
 * 3: layers below 2^12, tree tops, the transcript).  Diagnostics / tests:
 *   _variant_dev  the chosen form on n <= 2^26 states in place, all sixteen words of each; the idle quads / rows of the last
 *                 workgroup run the permutation on zeros, as the tree kernels do;
 *   _f64_probe    the fp64 forms on integer-valued DOUBLES (16 per state) of any magnitude the contract allows, canonical
 *                 Montgomery words out — mode 0: whole permutation (|v| <= 2^33), 1: the 13 internal rounds (|v| <= 2^37),
 *                 2: the modular reduction alone, 3: whole permutation, one state per quad (the contract of mode 0).
 * Both refuse an unknown variant / mode with P3HIP_ERR_BAD_ARG; n = 0 is a no-op. */
int p3hip_poseidon2_permute_variant_dev(uint32_t *d_states, size_t n, int variant, void *stream);
int p3hip_poseidon2_f64_probe_dev(const double *d_in, uint32_t *d_out, size_t n, int mode, void *stream);

/* ---- diagnostics / tests: the field probe ------------------------------------------------------------
 * ONE primitive of the field arithmetic per call, lane by lane: lane i reads its k operands at in[i * k ..], calls the function of
 * csrc/bb31.hip.h, csrc/poseidon2_f64.hip.h or csrc/ntt_narrow_f64.hip.h itself, and writes its m results at out[i * m ..].
 * Integer and extension ops move uint32_t words (Montgomery words x * 2^32 mod P unless said otherwise); fp64 ops move doubles and
 * return the function's RAW double (the word, as a double, for the three functions that produce a word), so that a test can assert a
 * bound and not only a congruence.  _dev runs the DEVICE branch of each function (d_in / d_out device memory, enqueued on `stream`);
 * _host runs the HOST branch of the integer and extension ops on host memory, needs no GPU, and refuses the fp64 ops by name (they are
 * __device__ only).  Both refuse an unknown op and n > 2^22 with P3HIP_ERR_BAD_ARG and a message.  Operands outside an op's stated
 * domain give an unspecified value, never an address: no load, store or loop bound depends on an operand, except the at most 64
 * iterations of pow's exponent and the at most 27 squarings of two_adic_generator.
 *
 *  op  function                     in (k)                      out (m)  stated domain
 *   1  add(a, b)                    a, b                        1        a, b in [0, P)
 *   2  sub(a, b)                    a, b                        1        a, b in [0, P)
 *   3  neg(a)                       a                           1        a in [0, P)
 *   4  dbl(a)                       a                           1        a in [0, P)
 *   5  mul(a, b)                    a, b                        1        a, b in [0, P)
 *   6  sqr(a)                       a                           1        a in [0, P)
 *   7  dot2(a0, b0, a1, b1)         a0, b0, a1, b1              1        all in [0, P); = (a0 b0 + a1 b1) 2^-32
 *   8  to_monty(c)                  c (canonical)               1        c in [0, P)
 *   9  from_monty(m)                m                           1 canon. any 32-bit word; = m 2^-32 mod P
 *  10  pow7(x)                      x                           1        x in [0, P)
 *  11  pow(base, e)                 base, e_lo, e_hi            1        base in [0, P), any 64-bit e; pow(., 0) = ONE
 *  12  inv(a)                       a                           1        a in [0, P); inv(0) = 0
 *  13  two_adic_generator(bits)     bits (a plain integer)      1        bits <= 27
 *  14  smul(a, b)                   a, b as int32 bit patterns  1 int32  a, b in (-P, P); result in (-P, P), = a b 2^-32 mod P
 *  15  sbox7_add(s, rc)             s, rc                       1        s, rc in [0, P); = (s + rc)^7 in Montgomery form
 *  16  ext mul(a, b)                a[4], b[4]                  4        coefficients in [0, P); F[x] / (x^4 - 11)
 *  17  ext sqr(a)                   a[4]                        4        "
 *  18  ext inv(a)                   a[4]                        4        "; inv(0) = 0
 *  19  ext pow(a, e)                a[4], e_lo, e_hi            4        ", any 64-bit e
 *  20  ext scale(a, s)              a[4], s                     4        ", s in [0, P)
 *  32  mulmod(a, b)                 a, b                        1        integers, |ab| < 2^76; |result| < 1.1 P
 *  33  mulmod_p(a, b, aP)           a, b, aP                    1        integers a, b, |a| <= P/2 + 2 or a in [0, P), |ab| < 2^76,
 *                                                                        aP = a / P or a * (1/P) correctly rounded
 *  34  mulmod_p(a, b, a * pinv)     a, b                        1        as 33, aP formed on the device
 *  35  mulmod_m(a, b, aP, ..)       a, b, aP                    1        as 33 and |b aP| < 2^51; also |a|, |b| <= 35 (P/2 + 1)
 *  36  mulmod_m(a, b, a * pinv, ..) a, b                        1        as 35, aP formed on the device
 *  37  add_scaled_pow2(tot, x, inv) tot, x, inv                 1        integers |tot| < 2^40, |x| < 2^44, inv = +-2^-K, 1 <= K <= 8
 *  38  sbox7(x, ..)                 x                           1        integer |x| <= 35 (P/2 + 1) + P < 2^37; |result| <= P/2 + 2^9
 *  39  store_elem(v)                v                           1 word   integer |v| < 2^37; = v 2^32 mod P in [0, P)
 *  40  mulm(a, aP, b, ..)           a, aP, b                    1        integers, a in [0, P) or |a| <= P/2 + 2, |b aP| < 2^51
 *  41  mulm(a, a * pinv, b, ..)     a, b                        1        as 40, aP formed on the device
 *  42  word_centered(r)             r                           1 word   integer |r| <= P/2 + 2^22; = r mod P in [0, P)
 *  43  word_any(x, ..)              x                           1 word   integer |x| < 2^43; = x mod P in [0, P)
 *  48  add_scaled_pow2(tot, x, m)   tot, x, m                   1        the integer multipliers of the quad form's diagonal: m in
 *                                                                        {-2, 1, 2, 3, 4, -3, -4, -15, 15}, integers |tot| <= P/2 + 1,
 *                                                                        |x| <= 15^3 35 (P/2 + 2^9) + 241 (P/2 + 1) < 2^47; = tot + m x
 *  49  sbox7(x, ..)                 x                           1        integer |x| <= 35 (P - 1) + P < 2^37 (the first round's
 *                                                                        inputs on canonical states); |result| <= P/2 + 2^9
 * The uniform operands the fp64 functions take besides (".." above: the magic-number pair, -(P - 1), 1 / P, -1/2 + 2^-33) are formed
 * as the kernels form them.  tests/field_ref.py holds the reference of every op and the exact model of every fp64 one. */
#define P3HIP_FP_ADD 1
#define P3HIP_FP_SUB 2
#define P3HIP_FP_NEG 3
#define P3HIP_FP_DBL 4
#define P3HIP_FP_MUL 5
#define P3HIP_FP_SQR 6
#define P3HIP_FP_DOT2 7
#define P3HIP_FP_TO_MONTY 8
#define P3HIP_FP_FROM_MONTY 9
#define P3HIP_FP_POW7 10
#define P3HIP_FP_POW 11
#define P3HIP_FP_INV 12
#define P3HIP_FP_TWO_ADIC_GENERATOR 13
#define P3HIP_FP_SMUL 14
#define P3HIP_FP_SBOX7_ADD 15
#define P3HIP_FP_EXT_MUL 16
#define P3HIP_FP_EXT_SQR 17
#define P3HIP_FP_EXT_INV 18
#define P3HIP_FP_EXT_POW 19
#define P3HIP_FP_EXT_SCALE 20
#define P3HIP_FP_MULMOD 32
#define P3HIP_FP_MULMOD_P 33
#define P3HIP_FP_MULMOD_P_DEV 34
#define P3HIP_FP_MULMOD_M 35
#define P3HIP_FP_MULMOD_M_DEV 36
#define P3HIP_FP_ADD_SCALED_POW2 37
#define P3HIP_FP_SBOX7 38
#define P3HIP_FP_STORE_ELEM 39
#define P3HIP_FP_MULM 40
#define P3HIP_FP_MULM_DEV 41
#define P3HIP_FP_WORD_CENTERED 42
#define P3HIP_FP_WORD_ANY 43
#define P3HIP_FP_ADD_SCALED_INT 48
#define P3HIP_FP_SBOX7_WIDE 49
int p3hip_field_probe_dev(int op, const void *d_in, void *d_out, size_t n, void *stream);
int p3hip_field_probe_host(int op, const void *in, void *out, size_t n);

/* ---- Mmcs<BabyBear>: MerkleTreeMmcs<Poseidon2 sponge 16/8/8, TruncatedPermutation 2/8/16, digest 8>
 *      (the Poseidon2 analogue of the Keccak MMCS wired at native/src/fib_air.rs:31-51) ------------ */
typedef struct p3hip_tree p3hip_tree_t;
/* Mmcs::commit: matrices are device pointers (row-major, power-of-two heights); the tree keeps every
 * digest layer in HBM and BORROWS the matrices (they must outlive the tree).  root_out is a host buffer;
 * the call synchronises the stream before returning the root.  d_mats[m]: heights[m] x widths[m] words, read-only, any 4-byte
 * alignment (of every p3hip_mmcs_commit*_dev entry; the salted Keccak leaf kernel of the hiding commit moves 16-byte rows and is
 * taken only when the rows allow it).  A matrix of width 0 is accepted, alone, inside a class and as an injected class: it adds
 * nothing to its class's row, and an empty row hashes to the all-zero digest, as upstream's sponges do (its pointer is never
 * read).  At most 64 matrices, at most 16 of one height: more are refused by name before anything is launched (the hiding commit:
 * 32 and 8, before a salt is drawn). */
int p3hip_mmcs_commit_dev(const uint32_t *const *d_mats, const size_t *heights, const size_t *widths,
                          size_t n_mats, uint32_t root_out[8], p3hip_tree_t **tree_out, void *stream);
/* as above without the root download/synchronise (root readable later via p3hip_mmcs_root) */
int p3hip_mmcs_commit_async_dev(const uint32_t *const *d_mats, const size_t *heights, const size_t *widths,
                                size_t n_mats, p3hip_tree_t **tree_out, void *stream);
int p3hip_mmcs_root(const p3hip_tree_t *tree, uint32_t root_out[8], void *stream);
size_t p3hip_mmcs_log_max_height(const p3hip_tree_t *tree);
size_t p3hip_mmcs_num_layers(const p3hip_tree_t *tree);
/* device pointer to digest layer `layer` (layer 0 = leaf digests), 8 words per digest */
const uint32_t *p3hip_mmcs_layer_dev(const p3hip_tree_t *tree, size_t layer, size_t *len_out);
/* Mmcs::open_batch: opened rows of every matrix (concatenated, host buffer of sum(widths) words) and the
 * sibling path (host buffer of log_max_height*8 words). */
int p3hip_mmcs_open_batch(const p3hip_tree_t *tree, size_t index, uint32_t *rows_out, uint32_t *path_out,
                          void *stream);
void p3hip_mmcs_free(p3hip_tree_t *tree);
/* Mmcs::verify_batch (upstream p3_commit::Mmcs::verify_batch; the fourth method of the MMCS the reference passes into its PCS,
 * native/src/fib_air.rs:40-51), either hash configuration (P3HIP_HASH_*).  HOST code, no GPU needed, like p3hip_verify_fib_air: the
 * proof verifiers check their openings with it.  Returns 0 to accept, one of the positive codes below to reject (message via
 * p3hip_take_last_error), P3HIP_ERR_BAD_ARG for a malformed call (a null pointer, n_mats 0 or above 64, a height that is no power
 * of two, an unknown hash).  Mixed heights as MerkleTree::new injects them: the matrices of the tallest height form the leaf row,
 * and after the compression at each level the rows of the matrices whose height equals that level's length are hashed and
 * compressed in; matrix m contributes row index >> (log_max - log_h_m).  rows: the opened rows, sum(widths) words in matrix order;
 * path: path_len x 8 words.  A HIDING tree is verified by listing every salt as a width-4 matrix of its matrix's height,
 * interleaved m0, s0, m1, s1 ... — the order p3hip_mmcs_open_batch returns on such a tree. */
#define P3HIP_MMCS_ROOT_MISMATCH 1   /* upstream MerkleTreeError::RootMismatch */
#define P3HIP_MMCS_WRONG_HEIGHT  2   /* path_len != log2(tallest matrix) */
#define P3HIP_MMCS_NOT_CANONICAL 3   /* an opened value >= P, or (Poseidon2 only) a digest word >= P */
#define P3HIP_MMCS_BAD_INDEX     4   /* index >= tallest height */
int p3hip_mmcs_verify_batch(int hash, const uint32_t root[8], const size_t *heights, const size_t *widths, size_t n_mats,
                            size_t index, const uint32_t *rows, const uint32_t *path, size_t path_len);
/* Mmcs::open_batch (fib_air.rs:40-51) for n indices in ONE launch, device to device: opening i is row_words words at d_rows + i *
 * row_words (the rows of every matrix in matrix order, salts included on a hiding tree) and log_max_height x 8 words at d_paths +
 * i * log_max_height * 8.  d_indices: n 32-bit words in device memory; an index is MASKED into the tree (index mod the tallest
 * height), so whatever the buffer holds the gather stays inside the tree.  Enqueues only: no allocation, no copy to the host, no
 * synchronise (it can be captured).  d_indices (read-only), d_rows, d_paths: any 4-byte alignment; exactly n x row_words and n x
 * log_max_height x 8 words are written.  d_paths must be 16-byte aligned for p3hip_mmcs_verify_batch_many_dev. */
size_t p3hip_mmcs_row_words(const p3hip_tree_t *tree);   /* sum of the widths, salts included on a hiding tree */
int p3hip_mmcs_open_batch_many_dev(const p3hip_tree_t *tree, const uint32_t *d_indices, size_t n,
                                   uint32_t *d_rows /* n x row_words */, uint32_t *d_paths /* n x log_max_height x 8 */, void *stream);
/* Mmcs::verify_batch (upstream; fib_air.rs:40-51) for n openings of ONE commitment in one launch, in exactly the layout
 * p3hip_mmcs_open_batch_many_dev writes: commit, open and verify chain on one stream with no host touch.  root, heights and widths
 * are host memory, read before the call returns; d_status[i] = 0 or P3HIP_MMCS_ROOT_MISMATCH / _NOT_CANONICAL / _BAD_INDEX (the
 * path length is given by the dimensions); *d_rejected (device word, may be null) = how many are nonzero.  Enqueues only, allocates
 * nothing.  One opening per lane.  (A lane-cooperative form for small n exists — one opening per 16 lanes under Poseidon2, per wave
 * under Keccak — but this entry does not take it until it has been timed against the per-lane form: DESIGN.md section 4.2, and the
 * diagnostics below.)  Heights up to 2^31.  d_indices, d_rows: read-only, any 4-byte alignment; d_paths: read-only, 16-byte aligned
 * (refused otherwise); exactly n words of d_status and one of d_rejected are written. */
int p3hip_mmcs_verify_batch_many_dev(int hash, const uint32_t root[8] /* host, passed by value */,
                                     const size_t *heights, const size_t *widths, size_t n_mats,
                                     const uint32_t *d_indices, size_t n, const uint32_t *d_rows, const uint32_t *d_paths,
                                     uint32_t *d_status /* n codes: 0 or P3HIP_MMCS_* */, uint32_t *d_rejected /* one word, may be null */,
                                     void *stream);
/* Diagnostics of the two kernel forms (no reference counterpart; tests and tools/mmcs_verify_bench.py time one form against the
 * other, as p3hip_poseidon2_permute_variant_dev does for the two arithmetic forms).  The statuses never differ between forms.
 *   _form_dev   p3hip_mmcs_verify_batch_many_dev with the form chosen by the caller: 0 = by n, as that entry does; 1 = one opening
 *               per lane; 2 = cooperative (at most 2^24 openings);
 *   _coop_max   the largest n that form 0 sends to the cooperative form, by hash and profile (P3HIP_PROFILE_*); 0 = the per-lane
 *               form always (or an unknown hash / profile). */
int p3hip_mmcs_verify_batch_many_form_dev(int form, int hash, const uint32_t root[8], const size_t *heights, const size_t *widths,
                                          size_t n_mats, const uint32_t *d_indices, size_t n, const uint32_t *d_rows,
                                          const uint32_t *d_paths, uint32_t *d_status, uint32_t *d_rejected, void *stream);
size_t p3hip_mmcs_verify_coop_max(int hash, int profile);
/* host-pointer convenience: uploads the matrices, commits, keeps its own device copies inside the tree */
int p3hip_mmcs_commit(const uint32_t *const *mats, const size_t *heights, const size_t *widths,
                      size_t n_mats, uint32_t root_out[8], p3hip_tree_t **tree_out);

/* ---- the reference's own hash configuration (native/src/fib_air.rs:28-38): U64Hash = PaddingFreeSponge<KeccakF, 25,
 *      17, 4>, FieldHash = SerializingHasher<U64Hash>, MyCompress = CompressionFunctionFromHasher<U64Hash, 2, 4>.
 *      Digests are [u64; 4], stored as 8 little-endian u32 words, so trees of both configurations share
 *      p3hip_mmcs_root / open_batch / layer_dev / free.  Non-hiding (MerkleTreeMmcs, not MerkleTreeHidingMmcs). ---- */
#define P3HIP_HASH_POSEIDON2 0
#define P3HIP_HASH_KECCAK 1
int p3hip_mmcs_commit_hash_dev(int hash, const uint32_t *const *d_mats, const size_t *heights, const size_t *widths,
                               size_t n_mats, uint32_t root_out[8], p3hip_tree_t **tree_out, void *stream);
/* host-pointer convenience, as p3hip_mmcs_commit */
int p3hip_mmcs_commit_hash(int hash, const uint32_t *const *mats, const size_t *heights, const size_t *widths,
                           size_t n_mats, uint32_t root_out[8], p3hip_tree_t **tree_out);
/* Mmcs::commit into CALLER-PROVIDED digest-layer storage of p3hip_mmcs_layer_words(max height) 32-bit words (leaf layer
 * first, 8 words per digest): nothing is allocated and nothing synchronises — the call only enqueues.  The tree borrows the
 * storage and the matrices; read the root with p3hip_mmcs_root.  d_layers: 16-byte aligned (every compression kernel moves digests as
 * 16-byte pieces; refused otherwise), written exactly over those words. */
size_t p3hip_mmcs_layer_words(size_t max_height);
int p3hip_mmcs_commit_into_dev(int hash, const uint32_t *const *d_mats, const size_t *heights, const size_t *widths,
                               size_t n_mats, uint32_t *d_layers, p3hip_tree_t **tree_out, void *stream);
/* KeccakF::permute_mut on n independent [u64; 25] states in device memory (p3-keccak's KeccakF, fib_air.rs:32), in place: exactly
 * 25 n u64 words; d_states 8-byte aligned (refused otherwise; also by the variant entry below) */
int p3hip_keccak_f_dev(uint64_t *d_states, size_t n, void *stream);
/* Diagnostics / tests: the three formulations of Keccak-f on n <= 2^24 states of 25 words, in place.  variant 0: one state per lane,
 * all 25 words (what p3hip_keccak_f_dev runs); 1: the digest form every leaf and compression runs (first round peeled, the last
 * computes row 0 only) — words 0..3 of each state are written, words 4..24 of the buffer stay as they were; 2: the lane-cooperative
 * form, one state per wave, all 25 words.  An unknown variant is refused with P3HIP_ERR_BAD_ARG; n = 0 is a no-op. */
int p3hip_keccak_f_variant_dev(uint64_t *d_states, size_t n, int variant, void *stream);
/* Diagnostics / tests: ONE 2-to-1 compression layer through the PRODUCTION kernel of a named form, launched unchanged with the
 * geometry a commitment gives it: d_in = 2 n_out digests of 8 words, d_out = n_out digests.  hash 0 (Poseidon2): variant 0 = int32 per
 * lane (the injected layers' kernel, without injection), 1 = fp64 per lane, 2 = fp64 per quad, 3 = one level of the 16-lane levels
 * kernel.  hash 1 (Keccak): 0 = per lane (no injection), 1 = one level of the per-lane levels kernel, 2 = one level of the per-wave
 * levels kernel.  The entry stages the two layers back to back in a 16-byte-aligned buffer of its own and synchronises `stream`.
 * Refused with P3HIP_ERR_BAD_ARG: an unknown hash or variant, a null pointer, n_out > 2^24, and for the levels kernels an n_out that is
 * not a power of two or exceeds 2^15 (nothing is padded).  n_out = 0 is a no-op. */
int p3hip_compress_layer_variant_dev(int hash, int variant, const uint32_t *d_in, uint32_t *d_out, size_t n_out, void *stream);

/* ---- fib_air prover: p3_uni_stark::prove(&config, &FibonacciAir{}, trace, &pis) as called at
 *      native/src/fib_air.rs:70, for StarkConfig<TwoAdicFriPcs<BabyBear, Dft, Poseidon2 Mmcs, ExtensionMmcs>,
 *      BinomialExtensionField<BabyBear,4>, DuplexChallenger<BabyBear, Poseidon2-16, 16, 8>> ---------------- */
typedef struct {
    uint32_t log_blowup;          /* p3_fri::FriParameters::log_blowup */
    uint32_t log_final_poly_len;  /* ::log_final_poly_len (create_test_fri_params(mmcs, 2) in fib_air.rs:62) */
    uint32_t num_queries;
    uint32_t proof_of_work_bits;
} p3hip_fri_params_t;
typedef struct p3hip_fib_prover p3hip_fib_prover_t;
/* PROFILES — chosen when an object is created, as the reference chooses its backend when GpuDft is constructed
 * (native/src/gpu_dft.rs:85-92 `with_backend`); nothing is read from the environment.  LATENCY: one proof at a time, which is what
 * the reference does (app/src/main/java/com/plonky3/android/MainActivity.kt:29-33, native/src/fib_air.rs:56-72): layers of
 * 2^10..2^15 digests use the forms that shorten a lone proof's chain of dependent launches (one Poseidon2 state per DPP quad,
 * cooperative Keccak up to 2^12 digests), the hiding prover commits its randomization polynomial on a second side stream, the FRI
 * rounds of at most 2^7 rows run in one single-workgroup launch, and a hiding proof whose LDE domain has at most 2^8 points — the
 * reference's own instance, n = 8 (fib_air.rs:56-57) — is ONE kernel launch of one workgroup.  THROUGHPUT: several provers share the chip and VALU issue is what
 * is short: the per-lane forms.  Proof bytes, digests and every intermediate are the same under both.
 * Defaults: p3hip_fib_prover_create* and p3hip_run_fib_air_zk = LATENCY; p3hip_fib_batch_create* with more than one prover =
 * THROUGHPUT; free functions (p3hip_mmcs_commit*) = the calling thread's profile (LATENCY until p3hip_set_thread_profile). */
#define P3HIP_PROFILE_THROUGHPUT 1
#define P3HIP_PROFILE_LATENCY 2
int p3hip_set_thread_profile(int profile);
int p3hip_get_thread_profile(void);  /* -1 when the thread has no device context (no HIP device) */
/* The general creation entry: any hash (P3HIP_HASH_*), hiding != 0 for the reference's MerkleTreeHidingMmcs + HidingFriPcs
 * (then `seed` seeds its SmallRng streams), any profile.  The create functions below are this one with P3HIP_PROFILE_LATENCY. */
int p3hip_fib_prover_create_profile(int profile, int hash, int hiding, uint64_t seed, unsigned log_n, const p3hip_fri_params_t *params,
                                    void *stream, int own_stream, p3hip_fib_prover_t **out);
/* Allocates the prover's HBM arena for 2^log_n-row traces.  stream: hipStream_t to enqueue on, or pass
 * own_stream != 0 to let the prover create (and own) a non-blocking stream — one prover per host thread. */
int p3hip_fib_prover_create(unsigned log_n, const p3hip_fri_params_t *params, void *stream, int own_stream,
                            p3hip_fib_prover_t **out);
/* Proves the instance whose first trace row is (a, b) (generate_trace_rows(a, b, 2^log_n), public values
 * [a, b, last right value], fib_air.rs:61,68).  The returned bytes stay valid until the next prove/destroy.
 * Wire format: DESIGN.md "proof bytes". */
int p3hip_fib_prover_prove(p3hip_fib_prover_t *prover, uint64_t a, uint64_t b, const uint8_t **proof_out,
                           size_t *proof_len);
/* The same with the proof handed over in the CALLER's buffer (e.g. the pinned staging row of a gather): the prover serialises
 * into its own buffer and copies ONCE into `out` (what is saved are the caller-side copies — a Python bytes object and its copy
 * into the staging row).  Returns ERR_BAD_ARG when cap is too small, the needed size in *proof_len: checked BEFORE proving once
 * the prover has produced a proof (proofs of one prover have one length); on a first call that fails this way the proof has been
 * computed and discarded.  A retry returns the same bytes (the hiding prover restarts its streams from the seed for every proof).
 * `out` is HOST memory of any alignment: on success exactly *proof_len bytes are written, on any failure none. */
int p3hip_fib_prover_prove_into(p3hip_fib_prover_t *prover, uint64_t a, uint64_t b, uint8_t *out, size_t cap, size_t *proof_len);
/* The same in two halves, to keep the prover's stream busy across proofs: enqueue returns as soon as the proof's launches
 * are queued (nothing is waited for), finish waits for the OLDEST enqueued proof and returns its bytes (valid until the next
 * prove / finish / destroy).  At most two proofs may be in flight; the second one's kernels queue behind the first on the
 * prover's stream (the arena is reused in stream order, the results land in two pinned buffers), so the host's turnaround
 * between proofs — wake-up, serialisation, the next enqueue: 0.2-0.3 ms at 2^20 — no longer leaves the stream empty.
 * Not available for the hiding prover. */
int p3hip_fib_prover_enqueue(p3hip_fib_prover_t *prover, uint64_t a, uint64_t b);
int p3hip_fib_prover_finish(p3hip_fib_prover_t *prover, const uint8_t **proof_out, size_t *proof_len);
/* host wall-clock per stage [trace commit, quotient commit, open, FRI commit phase, grind, queries] in ms,
 * accumulated over *proofs proofs */
int p3hip_fib_prover_stage_times(p3hip_fib_prover_t *prover, double out_ms[6], uint64_t *proofs, int reset);
/* Diagnostics of the proof-of-work continuation path (no reference counterpart: p3_fri grinds on the host).  *misses = proofs
 * of this prover whose first device search range held no witness; indices_out[0..min(cap, *n_out)) = the device's query-index
 * buffer as it stood when the host learnt of the LAST miss, before the search continued: all zero by construction, because
 * the gather kernel queued behind the query kernel reads that buffer whatever the search returned. */
int p3hip_fib_prover_grind_miss_probe(p3hip_fib_prover_t *prover, uint64_t *misses, uint32_t *indices_out, size_t cap,
                                      size_t *n_out);
void p3hip_fib_prover_destroy(p3hip_fib_prover_t *prover);
/* verify(&config, &FibonacciAir{}, &proof, &pis) (native/src/fib_air.rs:71-72) with pis = [a, b, x]: host-side, a few
 * thousand permutations.  Returns 0 to accept, a positive code naming the failed check otherwise (message via
 * p3hip_take_last_error, e.g. "fib_air verification failed: OodEvaluationMismatch"). */
int p3hip_verify_fib_air(const uint8_t *proof, size_t len, uint64_t a, uint64_t b, uint64_t x, unsigned log_n,
                         const p3hip_fri_params_t *params);

/* The same prover / verifier under the reference's own hashes (hash = P3HIP_HASH_KECCAK; native/src/fib_air.rs:28-53):
 * Keccak MMCS + SerializingChallenger32<BabyBear, HashChallenger<u8, Keccak256Hash, 32>>, non-hiding.  Same wire
 * format; digests are [u64; 4] as 8 little-endian u32 words. */
int p3hip_fib_prover_create_hash(int hash, unsigned log_n, const p3hip_fri_params_t *params, void *stream, int own_stream,
                                 p3hip_fib_prover_t **out);
int p3hip_verify_fib_air_hash(int hash, const uint8_t *proof, size_t len, uint64_t a, uint64_t b, uint64_t x,
                              unsigned log_n, const p3hip_fri_params_t *params);

/* ---- the HIDING half of the reference's configuration (native/src/fib_air.rs:40-65):
 *      MerkleTreeHidingMmcs<.., SmallRng, .., SALT_ELEMS 4> (rng = SmallRng::seed_from_u64(1)) and
 *      HidingFriPcs::new(dft, val_mmcs, fri_params, num_random_codewords 4, SmallRng::seed_from_u64(1)), p3_uni_stark with
 *      SC::Pcs::ZK.  Randomized trace, blinded quotient chunks, randomization polynomial, salted leaves; the random
 *      streams are generated on the device.  Wire format version 2.  The protocol details are recalled from
 *      the absent upstream crates: parity unpinned. ---- */
int p3hip_fib_prover_create_hiding(int hash, unsigned log_n, const p3hip_fri_params_t *params, uint64_t seed, void *stream,
                                   int own_stream, p3hip_fib_prover_t **out);
int p3hip_verify_fib_air_hiding(int hash, const uint8_t *proof, size_t len, uint64_t a, uint64_t b, uint64_t x,
                                unsigned log_n, const p3hip_fri_params_t *params);
/* rand 0.9.2 `SmallRng::seed_from_u64(seed)` (xoshiro256++ behind SplitMix64) as a device-resident stream of BabyBear
 * elements (Montgomery words), exactly the sequence a host loop over `rng.random::<BabyBear>()` yields.  One stream is
 * used from one HIP stream at a time.  p3hip_rng_fill_field_dev: d_out any 4-byte alignment, exactly n words written. */
typedef struct p3hip_rng p3hip_rng_t;
int p3hip_rng_create(uint64_t seed, p3hip_rng_t **out);
int p3hip_rng_fill_field_dev(p3hip_rng_t *rng, uint32_t *d_out, size_t n, void *stream);
/* synchronises `stream` and returns the generator state (s[0..4)) after everything enqueued so far */
int p3hip_rng_state(p3hip_rng_t *rng, uint64_t state_out[4], void *stream);
void p3hip_rng_destroy(p3hip_rng_t *rng);
/* MerkleTreeHidingMmcs::commit (native/src/fib_air.rs:40-51, SALT_ELEMS = 4): every matrix is paired with a
 * height x 4 matrix of draws from `rng` (in input order), leaf rows are m0 || s0 || m1 || s1 ...; the tree owns the salt
 * matrices.  p3hip_mmcs_open_batch on such a tree returns the rows in that interleaved order (2 n_mats entries: the
 * caller splits values from salts, as MerkleTreeHidingMmcs::open_batch does); root / layers / free are shared. */
int p3hip_mmcs_commit_hiding_dev(int hash, const uint32_t *const *d_mats, const size_t *heights, const size_t *widths,
                                 size_t n_mats, p3hip_rng_t *rng, uint32_t root_out[8], p3hip_tree_t **tree_out, void *stream);

/* ---- batches of independent proofs (BASELINE configs[3]; SURVEY.md §8e: instance i is self-contained) ------
 * A pool of n_provers provers, each on its own host thread (thread-local context, as the reference's runtime,
 * backend_vulkan.rs:100-102) and its own stream, so the transcript round trips of one proof hide behind the
 * kernels of the others.  p3hip_fib_batch_prove proves instances (a[i], b[i]) and returns pointers to the proof
 * bytes, valid until the next call on the same batch. */
typedef struct p3hip_fib_batch p3hip_fib_batch_t;
/* Profile of the pool's provers: THROUGHPUT when n_provers > 1, LATENCY for a pool of one. */
int p3hip_fib_batch_create(unsigned log_n, const p3hip_fri_params_t *params, unsigned n_provers,
                           p3hip_fib_batch_t **out);
/* the pool under either hash configuration (P3HIP_HASH_POSEIDON2 / P3HIP_HASH_KECCAK) */
int p3hip_fib_batch_create_hash(int hash, unsigned log_n, const p3hip_fri_params_t *params, unsigned n_provers,
                                p3hip_fib_batch_t **out);
/* the pool in the reference's hiding configuration (fib_air.rs:40-65): every prover's SmallRng streams start from `seed`
 * for every proof, as a freshly built config would */
int p3hip_fib_batch_create_hiding(int hash, unsigned log_n, const p3hip_fri_params_t *params, uint64_t seed, unsigned n_provers,
                                  p3hip_fib_batch_t **out);
int p3hip_fib_batch_prove(p3hip_fib_batch_t *batch, size_t n, const uint64_t *a, const uint64_t *b,
                          const uint8_t **proofs_out, size_t *lens_out);
/* The same in two halves, for callers that keep the pool busy: submit copies the instance list, queues the batch behind
 * the ones already submitted and returns a ticket at once; collect waits for that batch (any order) and hands out the
 * proof pointers, valid until the next collect / prove / destroy on this pool.  A prover that has finished its share of
 * one batch starts on the next without waiting for the batch to complete — joining the provers after every batch costs
 * ~10 % at 64 proofs per batch (464 against ~520 proofs/s at 2^20).  At most 8 batches may be in flight.  A failed proof
 * fails its own batch's collect, not the others. */
int p3hip_fib_batch_submit(p3hip_fib_batch_t *batch, size_t n, const uint64_t *a, const uint64_t *b, uint64_t *ticket_out);
int p3hip_fib_batch_collect(p3hip_fib_batch_t *batch, uint64_t ticket, const uint8_t **proofs_out, size_t *lens_out);
void p3hip_fib_batch_destroy(p3hip_fib_batch_t *batch);

/* ---- a CALLER's trace and public values: prove(&config, &FibonacciAir {}, trace, &pis) (native/src/fib_air.rs:61,68-70) ----
 * The trace is 2^log_n rows x 2 Montgomery words, row-major (what p3hip_fib_trace_dev writes); pis = [left of row 0, right of row 0,
 * right of the last row] as Montgomery words, each < P (else ERR_BAD_ARG).  The proof commits to THIS trace and its transcript
 * observes THESE pis, whether or not they agree: as in upstream's release builds, a trace that is no Fibonacci trace, or pis it does
 * not satisfy, still yields a proof, and the verifiers reject it for those pis.  For a Fibonacci trace with its own pis the bytes are
 * those of p3hip_fib_prover_prove(a, b).  Every prover and pool of the create functions above takes these entries (the hiding ones
 * too; the enqueue form, as p3hip_fib_prover_enqueue, the non-hiding prover only).
 * BUFFER CONTRACT of the _dev entries: d_trace is 8-byte aligned (rows are read as pairs; refused otherwise) and read in place (no copy, no
 * word written).  The caller's writes to it must be complete, or ordered
 * on the prover's stream, before the call; the buffer must stay unchanged until the prove call returns, or, after an enqueue, until
 * finish has returned that proof.  A d_trace that hipPointerGetAttributes does not report as device memory of the prover's device,
 * or whose allocation ends before 2^log_n rows, is refused before anything is launched.
 * flags: P3HIP_PROVE_CHECK_TRACE runs p3hip_fib_check_trace_dev on the prover's stream first (upstream's debug-build
 * check_constraints) and returns ERR_BAD_ARG without proving when a row breaks a rule ("constraints had nonzero value on row <i>");
 * other bits are refused. */
#define P3HIP_PROVE_CHECK_TRACE 1u
/* p3hip_trace_check_t.mask bits: the rules of FibonacciAir (fib_air.rs:236-260) a row breaks.  is_transition is false on the
 * last row and there is no wrap-around; with one row, row 0 is first and last. */
#define P3HIP_TRACE_BAD_FIRST_LEFT 1u   /* first row: left != pis[0] */
#define P3HIP_TRACE_BAD_FIRST_RIGHT 2u  /* first row: right != pis[1] */
#define P3HIP_TRACE_BAD_NEXT_LEFT 4u    /* transition: next.left != right */
#define P3HIP_TRACE_BAD_NEXT_RIGHT 8u   /* transition: next.right != left + right (mod P, of the words as integers) */
#define P3HIP_TRACE_BAD_LAST_RIGHT 16u  /* last row: right != pis[2] */
#define P3HIP_TRACE_BAD_RANGE 32u       /* a word of the row is >= P */
typedef struct {
    int64_t first_bad_row;  /* -1: every row holds */
    uint32_t mask;          /* bits of first_bad_row */
    uint64_t bad_rows;      /* rows with a nonzero mask */
} p3hip_trace_check_t;
/* check_constraints over a device trace of n rows (any n; d_trace 8-byte aligned, device memory of the current device): one
 * streaming pass on `stream`, which the call synchronises. */
int p3hip_fib_check_trace_dev(const uint32_t *d_trace, size_t n, const uint32_t pis[3], p3hip_trace_check_t *out, void *stream);
/* the proof of a device trace; the bytes stay valid until the next prove / finish / destroy */
int p3hip_fib_prover_prove_trace_dev(p3hip_fib_prover_t *prover, const uint32_t *d_trace, const uint32_t pis[3], unsigned flags,
                                     const uint8_t **proof_out, size_t *proof_len);
/* the same from host memory: n must equal 2^log_n; the rows are uploaded into the prover's own trace buffer on its stream */
int p3hip_fib_prover_prove_trace(p3hip_fib_prover_t *prover, const uint32_t *host_trace, size_t n, const uint32_t pis[3], unsigned flags,
                                 const uint8_t **proof_out, size_t *proof_len);
/* p3hip_fib_prover_enqueue for a device trace (non-hiding provers); the proof comes back from p3hip_fib_prover_finish */
int p3hip_fib_prover_enqueue_trace_dev(p3hip_fib_prover_t *prover, const uint32_t *d_trace, const uint32_t pis[3]);
/* p3hip_fib_batch_prove for n device traces (device memory of the device the pool was created on, each complete before the call:
 * the pool's provers run on streams of their own); pis holds 3 words per trace.  Every trace and pis word is checked before any
 * prover starts. */
int p3hip_fib_batch_prove_traces_dev(p3hip_fib_batch_t *batch, size_t n, const uint32_t *const *d_traces, const uint32_t *pis,
                                     unsigned flags, const uint8_t **proofs_out, size_t *lens_out);

/* ---- batches of proofs verified ON THE DEVICE: verify(&config, &FibonacciAir{}, &proof, &pis) (native/src/fib_air.rs:70-72,
 * upstream p3_uni_stark::verify) for many proofs of ONE configuration at once — a pool's caller, a rank that gathers proofs, an
 * aggregator.  p3hip_verify_fib_air_hash / _hiding (host, one proof) are the specification; DESIGN.md "device verifier".
 * REJECT CODES.  status 0 = accept, exactly when the host verifier accepts the same bytes and public values.  Otherwise status is the
 * host verifier's code H whenever H is 10 (OodEvaluationMismatch), 11 (InvalidPowWitness), 13 (commitment opening), 14 (FRI layer
 * opening) or 15 (FinalPolyMismatch) and every field word of the proof is canonical: the first failure in the host's order.  In every
 * other case — a wrong length, a count / width / length word that is not what the parameters dictate (the host's 1..9 and 12), a field
 * word >= P anywhere in the proof, a public value >= P — status is P3HIP_VERIFY_MALFORMED: the device never follows a length word, so
 * it does not tell these apart. ---- */
typedef struct p3hip_fib_verifier p3hip_fib_verifier_t;
#define P3HIP_VERIFY_MALFORMED 16
/* fib_air.rs:70-72, p3_uni_stark::verify: the byte length every proof of this configuration has (DESIGN.md "proof bytes"); host only,
 * no GPU touched.  Refuses the parameters the host verifiers refuse, with their messages. */
int p3hip_fib_proof_len(int hash, int hiding, unsigned log_n, const p3hip_fri_params_t *params, size_t *len_out);
/* fib_air.rs:70-72, p3_uni_stark::verify: a verifier of up to max_proofs proofs per call on the calling thread's current device, which
 * it remembers (as trees and provers do).  Owns all scratch of the device entry, allocated here. */
int p3hip_fib_verifier_create(int hash, int hiding, unsigned log_n, const p3hip_fri_params_t *params, size_t max_proofs,
                              p3hip_fib_verifier_t **out);
/* fib_air.rs:70-72, p3_uni_stark::verify: n <= max_proofs proofs in device memory, proof i at d_proofs + i * stride_bytes (d_proofs
 * 4-byte aligned, stride a multiple of 4, >= p3hip_fib_proof_len); d_lens: n u32 byte lengths, or NULL = every proof has
 * p3hip_fib_proof_len bytes (a proof of another length is rejected without being read); d_pis: n x 3 Montgomery words [a, b, x] (the
 * convention of p3hip_fib_prover_prove_trace_dev); d_status: n codes; *d_rejected (may be NULL) = count of nonzero codes.  Enqueues
 * only (five launches and one 4-byte memset on `stream`): no allocation, no host copy, no synchronise; can be captured.  One call at
 * a time per verifier: the scratch is reused in stream order.  Every input is read-only; exactly n words of d_status and one of
 * d_rejected are written, whatever max_proofs is. */
int p3hip_fib_verifier_verify_dev(p3hip_fib_verifier_t *v, const uint8_t *d_proofs, size_t stride_bytes, const uint32_t *d_lens,
                                  const uint32_t *d_pis, size_t n, uint32_t *d_status, uint32_t *d_rejected, void *stream);
/* fib_air.rs:70-72, p3_uni_stark::verify: host convenience.  proofs[i] / lens[i]: host pointers (what p3hip_fib_batch_prove hands
 * out), a / b / x as p3hip_verify_fib_air takes them (reduced mod P); uploads on a stream of the verifier's own (staging allocated by
 * the first call), verifies, downloads status_out[n]; synchronises.  Splits n > max_proofs into several rounds itself. */
int p3hip_fib_verifier_verify(p3hip_fib_verifier_t *v, size_t n, const uint8_t *const *proofs, const size_t *lens,
                              const uint64_t *a, const uint64_t *b, const uint64_t *x, uint32_t *status_out);
void p3hip_fib_verifier_destroy(p3hip_fib_verifier_t *v);

/* ---- The reference's report-returning entry points (native/src/lib.rs:37-131 call fib_air::run_fib_air_zk /
 * fib_air::run_dft_benchmark and hand the returned String to Java).  Both write a NUL-terminated text of at most cap - 1 bytes
 * to out and return the length of the WHOLE text (snprintf convention); they never fail by status: a failure is text that
 * contains "failed", as in the JNI wrappers (lib.rs:48,104), and a message waiting in the error mailbox is appended as
 * "\nHIP error: ..." (lib.rs:62-65 appends "\nVulkan error: ..."). ---- */
/* run_fib_air_zk (native/src/fib_air.rs:27-75): the reference's own instance and configuration — n = 8, x = 21, Keccak hashes,
 * MerkleTreeHidingMmcs + HidingFriPcs seeded with 1, create_test_fri_params(_, 2) — proved on the device and verified on the
 * host: "fib_air zk ok (n=8, x=21)" (fib_air.rs:74) or "fib_air zk failed: <check>".  Honours the selector: with a backend other
 * than "hip" selected nothing is run and the text says so (fib_air.rs:60 hard-codes Vulkan; see integration/native/src/fib_air.rs.patch). */
int p3hip_run_fib_air_zk(char *out, size_t cap);

/* ---- Fiat-Shamir on the host: the challengers a caller drives between PCS calls.  hash = P3HIP_HASH_POSEIDON2:
 *      DuplexChallenger<BabyBear, Poseidon2-16, 16, 8>; P3HIP_HASH_KECCAK: SerializingChallenger32<BabyBear, HashChallenger<u8,
 *      Keccak256Hash, 32>> (native/src/fib_air.rs:53).  Words are Montgomery words below P. ---- */
typedef struct p3hip_challenger p3hip_challenger_t;
int p3hip_challenger_create(int hash, p3hip_challenger_t **out);                                     /* ::new */
int p3hip_challenger_observe(p3hip_challenger_t *c, const uint32_t *monty_words, size_t n);          /* CanObserve<F>::observe_slice */
int p3hip_challenger_observe_digest(p3hip_challenger_t *c, const uint32_t digest[8]);                /* CanObserve<Hash<..>>::observe */
int p3hip_challenger_sample_ext(p3hip_challenger_t *c, uint32_t out[4]);                             /* sample_algebra_element */
int p3hip_challenger_sample_bits(p3hip_challenger_t *c, unsigned bits, uint32_t *out);               /* CanSampleBits::sample_bits, bits <= 30 */
int p3hip_challenger_clone(const p3hip_challenger_t *c, p3hip_challenger_t **out);                   /* Clone */
void p3hip_challenger_destroy(p3hip_challenger_t *c);
/* A challenger as the words a device transcript reads and writes (p3hip_pcs_verifier_verify_dev's d_chal_in / d_chal_out): the duplex
 * state [16], input buffer [8], output buffer [8], pending inputs, outputs left, then the Keccak-256 hash challenger as a streaming
 * sponge (state [25 x u64], pending bytes, output bytes left, pending block [136 bytes], output [32 bytes]).  export writes the half
 * of the challenger's own configuration and zeroes the other; import reads that half, refuses (P3HIP_ERR_BAD_ARG, challenger
 * unchanged) a counter no challenger can hold — 8 or more pending inputs, more than 8 outputs left; a pending block of 136 bytes or
 * more, more than 32 output bytes left — and is otherwise the inverse of export: the next samples are the same. */
#define P3HIP_CHALLENGER_STATE_WORDS 128
int p3hip_challenger_export(const p3hip_challenger_t *c, uint32_t words[P3HIP_CHALLENGER_STATE_WORDS]);
int p3hip_challenger_import(p3hip_challenger_t *c, const uint32_t words[P3HIP_CHALLENGER_STATE_WORDS]);

/* ---- TwoAdicFriPcs<BabyBear, GpuDft, MerkleTreeMmcs, ExtensionMmcs> over CALLER-SUPPLIED matrices: the Pcs contract the reference
 *      hands to prove (HidingFriPcs::new(dft, val_mmcs, fri_params, ..), native/src/fib_air.rs:62-65), NON-HIDING, for either hash
 *      configuration and either profile.  DESIGN.md section 5.2.
 *      Scope: every matrix that takes part in one open / verify has the same height h = 2^log_h, 1 <= log_h and log_h + log_blowup
 *      <= 26 — what p3_uni_stark produces for any AIR (trace, preprocessed trace, quotient chunks).  Mixed heights are refused with
 *      P3HIP_ERR_BAD_ARG and a message naming the matrix.  Capacities (larger inputs are refused by name, never truncated): 8 matrices
 *      per commitment, 4 commitments ("rounds") per open, 4 distinct opening points per open, 8192 batched columns (the sum of width
 *      over every (matrix, point) pair; also the widest single matrix).  The FRI parameter gates are the fib prover's with log_h for
 *      the trace's log height.  An opening point on the LDE coset GENERATOR * <g_big> (a base-field z with (z / GENERATOR)^big = 1:
 *      upstream panics on the zero denominator) is refused on the host before anything is launched, naming round, matrix and point.
 *      Batches of proofs of one shape are verified on the device by p3hip_pcs_verifier_* (the section after the hiding PCS).
 *      MIXED HEIGHTS are opt-in at creation (p3hip_pcs_create_mixed, verified by p3hip_pcs_verify_mixed; below): an object from
 *      p3hip_pcs_create refuses them as stated above.  HidingFriPcs: the section after this one. ---- */
typedef struct p3hip_pcs p3hip_pcs_t;
typedef struct p3hip_pcs_data p3hip_pcs_data_t;
/* TwoAdicFriPcs::new(dft, mmcs, fri_params); stream / own_stream as p3hip_fib_prover_create */
int p3hip_pcs_create(int profile, int hash, const p3hip_fri_params_t *params, void *stream, int own_stream, p3hip_pcs_t **out);
/* Pcs::commit: d_evals[m] = heights[m] x widths[m] evaluations (device memory, read in place) over domain_shifts[m] * <g_h> in
 * natural row order.  The LDE is coset_lde_batch(evals, log_blowup, GENERATOR / shift), bit-reversed by row; one Merkle tree covers
 * the LDEs of the call, in input order.  The prover data owns the LDEs.  One synchronisation: the root read-back.  d_evals[m]: any
 * 4-byte alignment, read-only (plain, mixed and hiding objects alike), unchanged by commit and by every later open. */
int p3hip_pcs_commit_dev(p3hip_pcs_t *pcs, const uint32_t *const *d_evals, const size_t *heights, const size_t *widths,
                         const uint32_t *domain_shifts /* Montgomery, NULL = all 1 */, size_t n_mats,
                         uint32_t root_out[8], p3hip_pcs_data_t **data_out);
/* Pcs::get_evaluations_on_domain: the stored LDE of matrix `mat` (*height = h << log_blowup rows in HBM, no copy, no launch).  The
 * evaluations over the disjoint coset GENERATOR * <g_m>, h <= m <= *height, are its first m rows: natural index i at row bitrev(i, log m). */
int p3hip_pcs_lde_dev(const p3hip_pcs_data_t *data, size_t mat, const uint32_t **d_lde, size_t *height, size_t *width);
/* Pcs::open.  points_per_mat: one count per matrix, round -> matrix; points: 4 Montgomery words each, round -> matrix -> point.
 * opened_out: every opened value (4 words) in the order they are observed, round -> matrix -> point -> column.  *proof_out: the
 * FriProof section of the wire format (DESIGN.md "proof bytes": from the count of commit-phase roots through the witness; each
 * query's input_proof carries one BatchOpening per round, in round order), valid until the next open / destroy.  challenger: in, the
 * transcript before the open; out, the transcript after the last query index (unchanged when the call fails).  One synchronisation. */
int p3hip_pcs_open(p3hip_pcs_t *pcs, const p3hip_pcs_data_t *const *rounds, size_t n_rounds,
                   const size_t *points_per_mat, const uint32_t *points /* 4 words each, round -> matrix -> point */,
                   p3hip_challenger_t *challenger /* in: state before the open; out: state after the last query */,
                   uint32_t *opened_out, size_t opened_cap_words, const uint8_t **proof_out, size_t *proof_len);
/* Pcs::verify, host code.  roots: 8 words per round; mats_per_round / widths / points_per_mat / points / opened as for open.
 * Returns P3HIP_OK with *reject_code = 0 to accept, or = the failed check (the numbering of p3hip_verify_fib_air's FRI half: 5 commit
 * phase length, 6 query count, 7 final polynomial length, 8 trailing or missing bytes, 9 truncated, 11 InvalidPowWitness, 12 query
 * shape, 13 input opening, 14 FRI layer opening, 15 FinalPolyMismatch; message via p3hip_take_last_error) with the challenger where
 * the verifier stopped; P3HIP_ERR_BAD_ARG for a refused argument (challenger unchanged). */
int p3hip_pcs_verify(int hash, const p3hip_fri_params_t *params, unsigned log_h, const uint32_t *roots /* 8 per round */,
                     const size_t *mats_per_round, const size_t *widths, size_t n_rounds, const size_t *points_per_mat,
                     const uint32_t *points, const uint32_t *opened, const uint8_t *proof, size_t len,
                     p3hip_challenger_t *challenger, int *reject_code);
/* The same object with matrices of MIXED heights admitted (upstream TwoAdicFriPcs's general case; from recall, parity unpinned: DESIGN.md
 * section 3).  p3hip_pcs_commit_dev, p3hip_pcs_lde_dev (the height is the matrix's own) and p3hip_pcs_open serve it with the signatures
 * above; a same-height open on it is the open of a p3hip_pcs_create object, launch for launch.  A CLASS is the set of matrices of one
 * open that share log_big_m = log_h_m + log_blowup; log_big is the tallest class's.  One commitment is one tree over LDEs of their own
 * heights (MerkleTreeMmcs injects the shorter ones), in input order.  Opened values are observed round -> matrix -> point -> column.
 * Every class keeps its own count of alpha powers: a (matrix, point) pair of width w takes alpha^c .. alpha^(c + w - 1), c its class's
 * count so far.  Every class with a point has one reduced-opening vector ro_c over GENERATOR * <g_big_c>; the commit phase starts from
 * the tallest class's and adds beta^2 ro_c to the folded vector right after the fold that reaches 2^log_big_c elements, beta that
 * round's challenge (a class with log_h_c == log_final_poly_len goes into the final vector).  A query index has log_big bits; round r's
 * BatchOpening is opened at index >> (log_big - log_big_r), log_big_r the round's tallest LDE, which is its depth word and path length.
 * Refused by name before any launch or draw (P3HIP_ERR_BAD_ARG, challenger unchanged): no matrix of the tallest height has an opening
 * point (the FRI input would be missing); a matrix with log_h_m < log_final_poly_len; a point on the TALLEST LDE coset (it contains
 * every smaller one); the capacities above, with log_h the tallest log height.  Batches of mixed-height proofs of one shape are verified
 * on the device by a verifier from p3hip_pcs_verifier_create_mixed.  Not covered: a hiding object (p3hip_pcs_create_hiding) stays
 * same-height. */
int p3hip_pcs_create_mixed(int profile, int hash, const p3hip_fri_params_t *params, void *stream, int own_stream, p3hip_pcs_t **out);
/* Pcs::verify for mixed heights, host code: p3hip_pcs_verify with log_heights (one per matrix, round -> matrix) in place of log_h.  With
 * all heights equal it returns what p3hip_pcs_verify returns for the same bytes: the same return code and the same *reject_code.  (Of
 * an argument set with SEVERAL faults the two may name different ones in the message: this entry looks at the round and matrix counts
 * first, since it needs them to read log_heights.)  Reject codes as p3hip_pcs_verify. */
int p3hip_pcs_verify_mixed(int hash, const p3hip_fri_params_t *params, const unsigned *log_heights, const uint32_t *roots /* 8 per round */,
                           const size_t *mats_per_round, const size_t *widths, size_t n_rounds, const size_t *points_per_mat,
                           const uint32_t *points, const uint32_t *opened, const uint8_t *proof, size_t len,
                           p3hip_challenger_t *challenger, int *reject_code);
void p3hip_pcs_data_free(p3hip_pcs_data_t *d);
void p3hip_pcs_destroy(p3hip_pcs_t *pcs);

/* ---- HidingFriPcs<BabyBear, GpuDft, MerkleTreeHidingMmcs, ExtensionMmcs over it, SmallRng> over CALLER-SUPPLIED matrices: the PCS the
 *      reference builds (native/src/fib_air.rs:63-65), for either hash configuration and either profile.  DESIGN.md section 5.2.
 *      A hiding object is a p3hip_pcs_t; p3hip_pcs_commit_dev, p3hip_pcs_lde_dev, p3hip_pcs_open, p3hip_pcs_data_free and
 *      p3hip_pcs_destroy serve it.  It owns three SmallRng streams in HBM — `mmcs` (salts of the input commitments), `fri` (salts of
 *      the commit-phase layers; the FRI MMCS is a clone of the input MMCS taken at construction, so it starts from the same seed) and
 *      `pcs` — which advance from call to call for the object's lifetime; a call refused for its arguments draws nothing.
 *      With h = 2^log_h the caller's height, every committed matrix is a polynomial of degree < 2h: log_h >= 1 and log_h + 1 +
 *      log_blowup <= 24, log_final_poly_len < log_h + 1.  Capacities as above except 4 matrices per hiding commitment (a query lists
 *      every matrix and its salt); the 8192 batched columns count the random columns.  The rounds of one open are all hiding and of
 *      one configuration (hash, blowup, number of random codewords).  Opened values include the random columns.
 *      Batches of hiding proofs of one shape are verified on the device by p3hip_pcs_verifier_* (the next section).
 *      Not covered: mixed heights (a hiding object never accepts them), more than 4 matrices per hiding commitment. ---- */
/* HidingFriPcs::new(dft, mmcs, fri_params, num_random_codewords, SmallRng::seed_from_u64(pcs_seed)) over MerkleTreeHidingMmcs::new(..,
 * SmallRng::seed_from_u64(mmcs_seed)) (fib_air.rs:40-65: 4, 1, 1); num_random_codewords in 1..8 */
int p3hip_pcs_create_hiding(int profile, int hash, const p3hip_fri_params_t *params, unsigned num_random_codewords, uint64_t mmcs_seed,
                            uint64_t pcs_seed, void *stream, int own_stream, p3hip_pcs_t **out);
/* HidingFriPcs::commit is p3hip_pcs_commit_dev on a hiding object: matrix m (h x w, at most 4 of them, w <= 8192 - num_random_codewords)
 * takes h (w + 2 NRC) draws of `pcs` row by row, in input order, and becomes the 2h x (w + NRC) matrix with rows 2i = evals[i] ||
 * d[0..NRC) and 2i+1 = d[NRC..w+2NRC) over the size-2h domain with the caller's shift; then every matrix, in input order, takes a
 * (2h << log_blowup) x 4 salt matrix of `mmcs` draws; leaf rows m0 || s0 || m1 || s1 ...  p3hip_pcs_lde_dev returns the stored LDE:
 * 2h << log_blowup rows of width w + NRC, the caller's own columns first.  One synchronisation. */
/* HidingFriPcs::commit_quotient: d_chunks[c], c < n_chunks in {2, 4}: h x width (<= 2048) evaluations in natural order on the coset
 * GENERATOR g_(n_chunks h)^c <g_h>.  Chunk c is blinded to q_c + (X^h - s_c^h) t_c with t_c (c < n_chunks - 1) h x width draws of
 * `pcs`, in chunk order, and the last t cancelling them in the verifier's recomposition; the n_chunks matrices of degree < 2h go
 * into one salted tree.  One synchronisation. */
int p3hip_pcs_commit_quotient_dev(p3hip_pcs_t *pcs, const uint32_t *const *d_chunks, size_t h, size_t width, size_t n_chunks,
                                  uint32_t root_out[8], p3hip_pcs_data_t **data_out);
/* HidingFriPcs::get_opt_randomization_poly_commitment for traces of 2^log_h rows: a 2h x (NRC + 4) matrix of `pcs` draws over the
 * size-2h domain (shift 1), committed like a trace.  One synchronisation. */
int p3hip_pcs_commit_randomization(p3hip_pcs_t *pcs, unsigned log_h, uint32_t root_out[8], p3hip_pcs_data_t **data_out);
/* HidingFriPcs::open is p3hip_pcs_open: hiding prover data on a hiding object (plain data on a hiding object and hiding data on a
 * plain object are refused by name).  Every committed column is opened, the random ones included; every commit-phase layer takes a
 * salt of `fri` draws; each BatchOpening carries the values per matrix, then one salt per matrix, then the path; each commit-phase
 * opening the sibling, the salt, the path. */
/* HidingFriPcs::verify, host code: p3hip_pcs_verify over salted openings.  log_h is the CALLER's log height; widths are the committed
 * widths (the caller's + NRC; NRC + 4 for the randomization matrix); at most 4 matrices per round.  Reject codes as p3hip_pcs_verify. */
int p3hip_pcs_verify_hiding(int hash, const p3hip_fri_params_t *params, unsigned log_h, const uint32_t *roots /* 8 per round */,
                            const size_t *mats_per_round, const size_t *widths, size_t n_rounds, const size_t *points_per_mat,
                            const uint32_t *points, const uint32_t *opened, const uint8_t *proof, size_t len,
                            p3hip_challenger_t *challenger, int *reject_code);

/* ---- batches of PCS proofs verified ON THE DEVICE: Pcs::verify of TwoAdicFriPcs (hiding = 0) or HidingFriPcs (hiding = 1) for many
 *      MEMBERS of ONE SHAPE at once — the proofs of any AIR a pool's caller, a rank that gathers proofs or an aggregator holds.
 *      p3hip_pcs_verify / p3hip_pcs_verify_hiding (host, one proof) are the specification; DESIGN.md section 5.2.
 *      A shape fixes the layout of every proof: log_h, the caller's log height as for the host verifiers; n_rounds <= 4; per round
 *      mats_per_round <= 8 (<= 4 when hiding); per matrix its committed width (random columns included when hiding) and
 *      points_per_mat <= 4 (zero allowed); n_slots <= 4 point slots; per (matrix, point) pair, round -> matrix -> point, one slot <
 *      n_slots.  A member supplies n_slots points; the host verifier's form is those points expanded pair by pair.  Slots take the
 *      place of the host's "at most 4 distinct values" rule: a slot may repeat and two slots may hold equal values.  Every other gate
 *      (8192 batched columns included) and its message are the host verifiers', refused when the verifier is created.
 *      REJECT CODES.  With H the host verifier's result for the member's expanded arguments: status 0 = accept, exactly when H
 *      accepts.  status = H whenever H is 11 (InvalidPowWitness), 13 (input opening), 14 (FRI layer opening) or 15
 *      (FinalPolyMismatch) and every field word of the proof, the opened values and the points is canonical: the first failure in the
 *      host's order.  Everything else is P3HIP_VERIFY_MALFORMED: the host's 5..9 and 12, a wrong length, a field word >= P, and a
 *      member whose VALUES the host refuses with P3HIP_ERR_BAD_ARG (an opened value or point >= P, a point on the LDE coset, a state
 *      counter out of range).  The field words OUTSIDE the queries, the opened values, the points, the roots and the state counters are
 *      checked before any arithmetic; the field words INSIDE the queries (rows, salts, siblings, Poseidon2 path words) are checked by
 *      the opening kernel, after the fold arithmetic has consumed them — they never reach an address or a loop bound, and the
 *      malformed status wins over whatever that arithmetic reported.  Batch-level arguments (n > max_proofs on the device entry, a misaligned pointer, a stride below the
 *      proof length) are refused with P3HIP_ERR_BAD_ARG before anything is launched. ---- */
typedef struct p3hip_pcs_verifier p3hip_pcs_verifier_t;
typedef struct {
    unsigned log_h;
    size_t n_rounds;
    const size_t *mats_per_round; /* n_rounds */
    const size_t *widths;         /* one per matrix, round -> matrix */
    const size_t *points_per_mat; /* one per matrix */
    size_t n_slots;
    const uint32_t *slots;        /* one per (matrix, point) pair, round -> matrix -> point */
} p3hip_pcs_shape_t;
/* Pcs::verify: the byte length every proof of the shape has (the FriProof section p3hip_pcs_open returns); host only, no GPU touched */
int p3hip_pcs_proof_len(int hash, int hiding, const p3hip_fri_params_t *params, const p3hip_pcs_shape_t *shape, size_t *len_out);
/* Pcs::verify: a verifier of up to max_proofs members per call on the calling thread's current device, which it remembers: a later
 * call from a thread whose current device is another one is NOT refused, it is redirected — the call makes the verifier's device
 * current for its duration and restores the caller's (the pointers must belong to the verifier's device).  p3hip_fib_verifier_* does
 * the same.  Owns all scratch of the device entry, allocated here; the HOST entry's staging (eight buffers and a stream) is allocated
 * by the first p3hip_pcs_verifier_verify call, which can therefore fail for lack of memory after creation succeeded. */
int p3hip_pcs_verifier_create(int hash, int hiding, const p3hip_fri_params_t *params, const p3hip_pcs_shape_t *shape, size_t max_proofs,
                              p3hip_pcs_verifier_t **out);
/* Pcs::verify: n <= max_proofs members in device memory.  Proof i at d_proofs + i * stride_bytes (stride a multiple of 4, >=
 * p3hip_pcs_proof_len); d_lens: n u32 byte lengths, or NULL = every proof has p3hip_pcs_proof_len bytes (a proof of another length
 * is rejected without being read); d_roots: n x n_rounds x 8 words; d_points: n x n_slots x 4 Montgomery words; d_opened: n x total
 * x 4 words in observation order (total = sum of width over the pairs); d_chal_in: n x P3HIP_CHALLENGER_STATE_WORDS, each member's
 * transcript before verification (8-byte aligned, as d_chal_out; everything else 4-byte aligned); d_status: n codes; *d_rejected (may
 * be NULL) = count of nonzero codes; d_chal_out (may be NULL): of an ACCEPTED member the transcript as the host verifier leaves it
 * (of any other member undefined).  Enqueues only (four launches and one 4-byte memset on `stream`): no allocation, no host copy,
 * no synchronise; can be captured.  One call at a time per verifier: the scratch is reused in stream order.  Every input is read-only;
 * exactly n words of d_status, one of d_rejected and n x P3HIP_CHALLENGER_STATE_WORDS of d_chal_out are written. */
int p3hip_pcs_verifier_verify_dev(p3hip_pcs_verifier_t *v, const uint8_t *d_proofs, size_t stride_bytes, const uint32_t *d_lens,
                                  const uint32_t *d_roots, const uint32_t *d_points, const uint32_t *d_opened, const uint32_t *d_chal_in,
                                  size_t n, uint32_t *d_status, uint32_t *d_rejected, uint32_t *d_chal_out, void *stream);
/* Pcs::verify: host convenience.  proofs[i] / lens[i], roots, points, opened: host memory, laid out as above; challengers[i]: in, the
 * member's transcript before verification; out, of an accepted member the transcript as the host verifier leaves it, of a rejected
 * member unchanged.  Uploads on a stream of the verifier's own (staging allocated by the first call), verifies, downloads
 * status_out[n]; synchronises.  Splits n > max_proofs into several rounds itself. */
int p3hip_pcs_verifier_verify(p3hip_pcs_verifier_t *v, size_t n, const uint8_t *const *proofs, const size_t *lens, const uint32_t *roots,
                              const uint32_t *points, const uint32_t *opened, p3hip_challenger_t *const *challengers, uint32_t *status_out);
/* MIXED HEIGHTS: the two entries above with log_heights (one log height per matrix, round -> matrix) in place of shape->log_h, which is
 * ignored — p3hip_pcs_shape_t keeps its layout.  The proofs are those of a p3hip_pcs_create_mixed object; a member brings what a member
 * of any shape brings (proof, n_rounds roots, n_slots points, the opened values in observation order, the state words) and is verified
 * through p3hip_pcs_verifier_verify_dev / p3hip_pcs_verifier_verify; the reject-code contract above holds with p3hip_pcs_verify_mixed as
 * H.  The gates and their messages are p3hip_pcs_verify_mixed's, in its order: the round and matrix counts first, a height below 2^1,
 * the LDE height of the tallest matrix, a matrix below 2^log_final_poly_len, "no matrix of the tallest height ... has an opening point";
 * widths, points per matrix, slots and the 8192 batched columns as above.  A point on the TALLEST LDE coset makes its member malformed.
 * hiding = 1 is refused by name (P3HIP_ERR_BAD_ARG): no HidingFriPcs over mixed heights exists; the flag is there so that one needs no
 * new entry.  With all heights equal both return what the same-height entries return: the same length, and a verifier that runs the
 * same kernels.  No capacity beyond those of the same-height entries. */
int p3hip_pcs_proof_len_mixed(int hash, int hiding, const p3hip_fri_params_t *params, const p3hip_pcs_shape_t *shape,
                              const unsigned *log_heights, size_t *len_out);
int p3hip_pcs_verifier_create_mixed(int hash, int hiding, const p3hip_fri_params_t *params, const p3hip_pcs_shape_t *shape,
                                    const unsigned *log_heights, size_t max_proofs, p3hip_pcs_verifier_t **out);
/* DIAGNOSTIC, not part of the stable ABI: 1 when the shape's reduced opening runs one wavefront per query, 0: one lane per query.  Which
 * form a shape gets is a tuning detail (today: 256 or more row words per query) and will move with measurements; the tests use this
 * entry to show that they run both forms.  Results never depend on the form. */
int p3hip_pcs_verifier_wave_form(const p3hip_pcs_verifier_t *v);
void p3hip_pcs_verifier_destroy(p3hip_pcs_verifier_t *v);

/* ---- caller-defined AIRs: the step of p3_uni_stark::prove between commit(trace) and commit(quotient) — quotient_values — and
 *      check_constraints, for an AIR the caller describes as a small PROGRAM; with the PCS and the challenger above this is every piece
 *      of prove(&config, &air, trace, &pis) / verify for an `air` of the caller's (plonky3-mobile_amd/air.py prove_air / verify_air
 *      compose them).  DESIGN.md section 5.3.
 *      The trace is a base-field matrix of `width` columns with `n_public` public values.  A program is a flat list of instructions
 *      of FOUR uint32_t each, {op, dst, a, b}:
 *        op  P3HIP_AIR_OP_ADD / _SUB / _MUL: slot[dst] = a op b;  P3HIP_AIR_OP_ASSERT_ZERO: constraint number k (k counts the
 *            assertions in program order) is `a`; its dst and b words are 0
 *        dst a value slot, < P3HIP_AIR_MAX_SLOTS
 *        a, b operands: kind << P3HIP_AIR_KIND_SHIFT | index, kind one of P3HIP_AIR_KIND_SLOT (index: a slot some EARLIER instruction
 *            wrote), _LOCAL / _NEXT (a column of the row / of the next row), _PUBLIC (a public value), _CONST (an entry of `consts`,
 *            Montgomery words), _SELECTOR (P3HIP_AIR_SEL_FIRST_ROW / _LAST_ROW / _TRANSITION)
 *      Degrees as upstream's SymbolicExpression: columns and selectors 1, publics and constants 0, add / sub the maximum, mul the
 *      sum; log_quotient_degree = log2_ceil(max(d, 2) - 1) with d the largest constraint degree.
 *      p3hip_air_create validates the WHOLE program and refuses, with P3HIP_ERR_BAD_ARG and a message naming the instruction: a column,
 *      public, constant, selector or slot index out of range, a slot read before any instruction wrote it, an unknown opcode or kind,
 *      zero constraints, a capacity exceeded.  After creation no index of the caller's is checked again: the kernels take no load
 *      address and no loop bound that creation has not validated.  CAPACITIES: ---- */
#define P3HIP_AIR_MAX_INSTRUCTIONS 65536
#define P3HIP_AIR_MAX_CONSTRAINTS 4096
#define P3HIP_AIR_MAX_SLOTS 64 /* 1 KiB of LDS each per workgroup of 256 rows: two workgroups fit a CU's 160 KiB */
#define P3HIP_AIR_MAX_WIDTH 8192
#define P3HIP_AIR_MAX_PUBLIC 4096
#define P3HIP_AIR_MAX_CONSTS 65536
#define P3HIP_AIR_MAX_DEGREE 9 /* of a constraint: at most 8 quotient chunks, what one commitment holds */
#define P3HIP_AIR_MAX_LOG_QUOTIENT_DEGREE 3
#define P3HIP_AIR_OP_ADD 0u
#define P3HIP_AIR_OP_SUB 1u
#define P3HIP_AIR_OP_MUL 2u
#define P3HIP_AIR_OP_ASSERT_ZERO 3u
#define P3HIP_AIR_KIND_SHIFT 24
#define P3HIP_AIR_KIND_SLOT 0u
#define P3HIP_AIR_KIND_LOCAL 1u
#define P3HIP_AIR_KIND_NEXT 2u
#define P3HIP_AIR_KIND_PUBLIC 3u
#define P3HIP_AIR_KIND_CONST 4u
#define P3HIP_AIR_KIND_SELECTOR 5u
#define P3HIP_AIR_SEL_FIRST_ROW 0u
#define P3HIP_AIR_SEL_LAST_ROW 1u
#define P3HIP_AIR_SEL_TRANSITION 2u
typedef struct p3hip_air p3hip_air_t;
typedef struct {
    uint32_t width, n_public, n_instructions;
    uint32_t n_constraints, n_slots /* highest slot written + 1 */, max_degree, log_quotient_degree;
} p3hip_air_info_t;
/* an Air (p3_air::Air::eval recorded as a program); host code, no GPU touched: the device copy is made by the first device call, on
 * that call's current device, which the object then belongs to: a later call makes that device current for its duration */
int p3hip_air_create(size_t width, size_t n_public, const uint32_t *code /* 4 words per instruction */, size_t n_instr,
                     const uint32_t *consts /* Montgomery */, size_t n_consts, p3hip_air_t **out);
void p3hip_air_destroy(p3hip_air_t *air);
int p3hip_air_info(const p3hip_air_t *air, p3hip_air_info_t *out);
/* p3_uni_stark::quotient_values.  d_lde: the committed trace LDE as p3hip_pcs_lde_dev hands it out ((2^log_n << log_blowup) rows of
 * `width` words on GENERATOR * <g_big>, bit-reversed; read in place).  With C = 2^log_quotient_degree and qn = 2^log_n * C the quotient
 * domain GENERATOR * <g_qn> is the LDE's first qn rows: natural row i is LDE row bitrev(i, log qn), its next row is natural row (i + C)
 * mod qn, x_i = GENERATOR g_qn^i; selectors are selectors_on_coset (Z_H = x^n - 1, is_first_row = Z_H / (x - 1), is_last_row = Z_H / (x -
 * g_n^-1), is_transition = x - g_n^-1).  The quotient (sum_k alpha^(K-1-k) c_k(i)) / Z_H(x_i), four words, goes to C dense n x 4
 * matrices: d_chunks_out[c] row r = natural row r C + c (16-byte aligned device pointers in a HOST array, refused otherwise, exactly
 * n x 4 words written each; d_lde any 4-byte alignment, read-only; chunk c is committed with domain shift GENERATOR g_qn^c).  pis: n_public Montgomery words, host memory.  log_blowup < log_quotient_degree is refused by name.
 * Enqueues on `stream` (one small upload and one launch; the first call at a log qn also builds that domain's root table) and does
 * not synchronise.  The per-call table (publics, alpha powers, chunk pointers) is the object's and is reused in stream order: calls on
 * ONE Air may follow each other without a synchronisation (the upload reads pinned staging that a later call rewrites only after an
 * event behind the earlier upload), also on different streams of one thread — a call on another stream than the one before it is
 * ordered behind that call's kernel by an event, so two streams SERIALISE on one Air; they never overlap.  Not from two threads. */
int p3hip_air_quotient_dev(p3hip_air_t *air, void *stream, const uint32_t *d_lde, unsigned log_n, unsigned log_blowup, const uint32_t *pis,
                           const uint32_t alpha[4], uint32_t *const *d_chunks_out);
/* p3_uni_stark::check_constraints (debug builds of prove): the same program over the trace itself, d_trace 2^log_n rows of `width`
 * words in natural order (any 4-byte alignment, read-only); selectors i == 0, i == n - 1, i != n - 1; next is row i + 1 mod n.  *row_out, *constraint_out: the smallest
 * (row, constraint) whose value is nonzero, or -1, -1.  One pass, one synchronisation. */
int p3hip_air_check_trace_dev(p3hip_air_t *air, void *stream, const uint32_t *d_trace, unsigned log_n, const uint32_t *pis,
                              long long *row_out, int *constraint_out);
/* VerifierConstraintFolder: the program over extension operands, host code.  local, next: width x 4 words; sels: is_first_row,
 * is_last_row, is_transition at the point, 4 words each; out = sum_k alpha^(K-1-k) c_k by Horner's rule. */
int p3hip_air_eval_ext(const p3hip_air_t *air, const uint32_t *local, const uint32_t *next, const uint32_t *pis, const uint32_t *sels,
                       const uint32_t alpha[4], uint32_t out[4]);
/* DIAGNOSTIC: p3hip_air_eval_ext at n points in one launch, one lane per point (the interpreter core of the batch verifier's
 * av_eval_kernel).  Device buffers, 4-byte aligned, read-only; per point width x 4 (d_local), width x 4 (d_next), n_public (d_pis; may be
 * NULL when n_public == 0), 12 (d_sels) and 4 (d_alpha) Montgomery words, which the caller keeps canonical; exactly 4 n words of d_out
 * are written.  Enqueues only; n = 0 is no operation; n > 2^20 is refused. */
int p3hip_air_eval_ext_dev(p3hip_air_t *air, void *stream, const uint32_t *d_local, const uint32_t *d_next, const uint32_t *d_pis,
                           const uint32_t *d_sels, const uint32_t *d_alpha, size_t n, uint32_t *d_out);
/* p3_uni_stark::verify for a proof of an `air` of the caller's (the bytes plonky3-mobile_amd/air.py prove_air returns: the header —
 * magic, 1, log_n, the trace and quotient roots, width and the local values, width and the next values, the chunk count C =
 * 2^log_quotient_degree and per chunk 4 and its 16 words — then the PCS's FriProof section).  DESIGN.md section 5.4.
 * p3hip_air_proof_len: the byte length every such proof has, 4 (3 + 16 + 2 (1 + 4 width) + 1 + 17 C) + p3hip_pcs_proof_len of the PCS
 * shape log_h = log_n, two rounds of [1, C] matrices of widths [width, 4, .., 4], the trace opened at [zeta, zeta g_n], every chunk at
 * [zeta].  Host only.  The gates and their messages are the PCS verifier's, plus 1 <= log_n <= 27 - log_quotient_degree and log_blowup >=
 * log_quotient_degree, each named when it fails. */
int p3hip_air_proof_len(const p3hip_air_t *air, int hash, unsigned log_n, const p3hip_fri_params_t *params, size_t *len_out);
/* One proof on the host.  *reject_code = 0: accepted; 1 magic or version, 2 log_n, 3 a count that is not the AIR's, 4 a truncated header
 * or a header field word >= P (the roots under Poseidon2 only), 10 OodEvaluationMismatch (the constraints at zeta, folded by Horner's
 * rule, against quotient(zeta) Z_H(zeta)), else p3hip_pcs_verify's code for the shape above with the opened values in the order local,
 * next, chunk 0 .. C - 1.  The transcript observes log_n twice, the trace root and the publics, samples alpha, observes the quotient root
 * and samples zeta.  pis: n_public Montgomery words; one >= P is P3HIP_ERR_BAD_ARG, as is log_n outside 1 .. 27 - log_quotient_degree. */
int p3hip_air_verify(const p3hip_air_t *air, int hash, unsigned log_n, const p3hip_fri_params_t *params, const uint8_t *proof, size_t len,
                     const uint32_t *pis, int *reject_code);
/* BATCHES of such proofs of ONE (air, hash, log_n, params) verified ON THE DEVICE; p3hip_air_verify is the specification and the
 * contract is p3hip_fib_verifier_*'s.  create copies what it needs of the program (the air may be destroyed afterwards), owns all device
 * scratch (a p3hip_pcs_verifier of the shape above included) and remembers the calling thread's current device: later calls are
 * redirected to it.  REJECT CODES, with H = p3hip_air_verify's result for the member: status 0 exactly when H accepts; status = H when H
 * is 10, 11, 13, 14 or 15 AND the proof has p3hip_air_proof_len bytes AND every count / width / depth word is the one the shape
 * dictates, the FRI section's included, AND every field word of the proof and every public value is canonical.  Everything else is
 * P3HIP_VERIFY_MALFORMED: H in 1..9 or 12, a wrong length, a word >= P, or what the host refuses for the member's values.  A member whose
 * header values fail the OOD check AND whose FRI section is malformed is MALFORMED: the host stops at 10 there and never looks at the
 * FRI section.
 * verify_dev: n <= max_proofs members in device memory, proof i at d_proofs + i * stride_bytes (4-byte aligned; the stride a multiple
 * of 4 and >= p3hip_air_proof_len); d_lens: n u32 byte lengths or NULL (a proof of another length is rejected unread); d_pis: n x
 * n_public Montgomery words, may be NULL when n_public == 0.  Enqueues only (seven launches and one 4-byte memset on `stream`): no
 * allocation, no host copy, no synchronise.  Every input is read-only; exactly n words of d_status and one of d_rejected (may be NULL)
 * are written.  Batch-level faults are refused with P3HIP_ERR_BAD_ARG before any launch.  One call at a time per verifier.
 * verify: host convenience; stages on a stream of its own (staging allocated by the first call), splits n > max_proofs into rounds,
 * synchronises.  pis: n x n_public words of host memory. */
typedef struct p3hip_air_verifier p3hip_air_verifier_t;
int p3hip_air_verifier_create(const p3hip_air_t *air, int hash, unsigned log_n, const p3hip_fri_params_t *params, size_t max_proofs,
                              p3hip_air_verifier_t **out);
int p3hip_air_verifier_verify_dev(p3hip_air_verifier_t *v, const uint8_t *d_proofs, size_t stride_bytes, const uint32_t *d_lens,
                                  const uint32_t *d_pis, size_t n, uint32_t *d_status, uint32_t *d_rejected, void *stream);
int p3hip_air_verifier_verify(p3hip_air_verifier_t *v, size_t n, const uint8_t *const *proofs, const size_t *lens, const uint32_t *pis,
                              uint32_t *status_out);
void p3hip_air_verifier_destroy(p3hip_air_verifier_t *v);

/* ---- p3_uni_stark::prove for an `air` of the caller's in ONE device-resident launch chain.  The proof is the one
 * p3hip_air_verify takes, byte for byte what plonky3-mobile_amd/air.py prove_air returns over a non-hiding TwoAdicFriPcs; the contract
 * follows p3hip_fib_prover_* and p3hip_air_verifier_create.
 * create copies the program (the air may be destroyed at once), remembers the calling thread's current device — every later call with
 * another one current is refused — and allocates everything a proof needs: the trace LDE, the C = 2^log_quotient_degree chunk matrices
 * and their LDEs, the two trees' digest layers, the open's scratch, the FRI arena, the proof staging buffer and its pinned landing
 * buffer.  A failed allocation is reported with the arena's size.  profile / hash: P3HIP_PROFILE_*, 0 Poseidon2 / 1 Keccak; stream:
 * the caller's (own_stream = 0; NULL is the null stream) or one the prover creates and owns.
 * LIMITS, each refused by name before anything is allocated:  1 <= log_n <= 27 - log_quotient_degree;  log_blowup >= 1 and >=
 * log_quotient_degree (the committed LDE must cover the quotient domain);  log_n + log_blowup <= 26;  log_final_poly_len < log_n;
 * 2 width + 4 C <= 8192 batched columns;  proof_of_work_bits <= 30;  and whatever p3hip_air_proof_len refuses for the shape.  The
 * hiding PCS and preprocessed columns are not covered.
 * prove_dev: d_trace = 2^log_n x width Montgomery words of device memory on the prover's device, natural row order, ANY 4-byte
 * alignment, READ IN PLACE: never written, never copied; the caller leaves it unchanged until the proof is returned.  pis: n_public
 * Montgomery words of HOST memory (may be NULL when n_public == 0); one >= P is P3HIP_ERR_BAD_ARG.  The prover does not judge the trace:
 * a broken one yields a proof the verifiers reject with code 10.  flags: P3HIP_PROVE_CHECK_TRACE runs p3hip_air_check_trace_dev on the
 * prover's stream first and refuses a broken trace with "constraints had nonzero value on row R (constraint K)", R and K the ones that
 * entry names; this costs one more synchronisation.  *proof_out stays valid until the prover's next proof or its destruction.
 * Between the first launch and the copy-back there is no allocation and no host synchronisation: the transcript runs on the device.
 * One synchronisation per proof, plus one per continued search range when the first proof-of-work range held no witness.
 * prove: the same for a trace in host memory, uploaded into a slot the first such call allocates.
 * enqueue_dev / finish: the same in two halves.  enqueue_dev returns once the launches and the copy-back are queued on the prover's
 * stream; finish synchronises and serialises.  ONE proof in flight: a second enqueue, or a prove, before finish is refused, as is
 * finish without enqueue.  Calls of one prover come from one thread at a time; two provers on two streams overlap freely. */
typedef struct p3hip_air_prover p3hip_air_prover_t;
int p3hip_air_prover_create(const p3hip_air_t *air, int profile, int hash, unsigned log_n, const p3hip_fri_params_t *params, void *stream,
                            int own_stream, p3hip_air_prover_t **out);
int p3hip_air_prover_prove_dev(p3hip_air_prover_t *prover, const uint32_t *d_trace, const uint32_t *pis, unsigned flags,
                               const uint8_t **proof_out, size_t *proof_len);
int p3hip_air_prover_prove(p3hip_air_prover_t *prover, const uint32_t *host_trace, const uint32_t *pis, unsigned flags,
                           const uint8_t **proof_out, size_t *proof_len);
int p3hip_air_prover_enqueue_dev(p3hip_air_prover_t *prover, const uint32_t *d_trace, const uint32_t *pis);
int p3hip_air_prover_finish(p3hip_air_prover_t *prover, const uint8_t **proof_out, size_t *proof_len);
void p3hip_air_prover_destroy(p3hip_air_prover_t *prover);

/* The CPU column of the benchmark is the caller's: the reference times Plonky3's Radix2DitParallel (fib_air.rs:101,137-141),
 * which libp3hip does not contain (no CPU path in the product).  Returns 0 on success; Montgomery words, natural row order. */
typedef int (*p3hip_cpu_dft_fn)(void *user, const uint32_t *in, uint32_t *out, size_t height, size_t width);
/* run_dft_benchmark (native/src/fib_air.rs:98-222): the reference's 11 shapes, warmup 1, repeats 10, batches of 4; per shape
 * avg/median/p95 of hip_e2e (host matrix in and out), hip_e2e_batched (4 transforms per synchronisation) and hip_kernel (device
 * resident, HIP events), the speedups over the caller's CPU transform and the reference's equality check (fib_air.rs:193-196:
 * "dft benchmark failed: dft benchmark mismatch at h=.., w=.."); cpu_dft == NULL leaves the CPU column and the check out. */
int p3hip_run_dft_benchmark(p3hip_cpu_dft_fn cpu_dft, void *user, char *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* P3HIP_H */
