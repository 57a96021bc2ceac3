// NEVER COMPILED HERE (no Rust toolchain in the build image; p3-* 0.4.2 path dependencies absent).
//
// native/src/hip_front_end.rs — what native/src/fib_air.rs calls when the selector says "hip" (fib_air.rs.patch):
// run_fib_air_zk and run_dft_benchmark as ONE call each into libp3hip, returning the same Result<String, String> the
// reference's functions return (fib_air.rs:27,98), so lib.rs:37-131 needs no change.
use core::ffi::{c_char, c_void};

use p3_baby_bear::BabyBear;
use p3_dft::TwoAdicSubgroupDft;
use p3_matrix::dense::RowMajorMatrix;

use crate::gpu_dft::{BackendKind, GpuDft};

type Val = BabyBear;

/// include/p3hip.h `p3hip_cpu_dft_fn`
type CpuDftFn = unsafe extern "C" fn(*mut c_void, *const u32, *mut u32, usize, usize) -> i32;

/// include/p3hip.h `p3hip_fri_params_t`
#[repr(C)]
struct FriParamsC {
    log_blowup: u32,
    log_final_poly_len: u32,
    num_queries: u32,
    proof_of_work_bits: u32,
}
#[repr(C)]
struct FibProverC {
    _opaque: [u8; 0],
}
#[repr(C)]
struct FibVerifierC {
    _opaque: [u8; 0],
}
const P3HIP_HASH_KECCAK: i32 = 1;

// include/p3hip.h, "report-returning entry points" and "a CALLER's trace"
extern "C" {
    fn p3hip_run_fib_air_zk(out: *mut c_char, cap: usize) -> i32;
    fn p3hip_run_dft_benchmark(cpu_dft: Option<CpuDftFn>, user: *mut c_void, out: *mut c_char, cap: usize) -> i32;
    fn p3hip_fib_prover_create_hiding(hash: i32, log_n: u32, params: *const FriParamsC, seed: u64, stream: *mut c_void,
                                      own_stream: i32, out: *mut *mut FibProverC) -> i32;
    fn p3hip_fib_prover_prove_trace(prover: *mut FibProverC, host_trace: *const u32, n: usize, pis: *const u32, flags: u32,
                                    proof_out: *mut *const u8, proof_len: *mut usize) -> i32;
    fn p3hip_fib_prover_destroy(prover: *mut FibProverC);
    fn p3hip_take_last_error() -> *const c_char;
    // "batches of proofs verified ON THE DEVICE": verify(&config, &FibonacciAir {}, &proof, pis) (fib_air.rs:71-72) for many proofs
    fn p3hip_fib_proof_len(hash: i32, hiding: i32, log_n: u32, params: *const FriParamsC, len_out: *mut usize) -> i32;
    fn p3hip_fib_verifier_create(hash: i32, hiding: i32, log_n: u32, params: *const FriParamsC, max_proofs: usize,
                                 out: *mut *mut FibVerifierC) -> i32;
    fn p3hip_fib_verifier_verify_dev(v: *mut FibVerifierC, d_proofs: *const u8, stride_bytes: usize, d_lens: *const u32,
                                     d_pis: *const u32, n: usize, d_status: *mut u32, d_rejected: *mut u32, stream: *mut c_void) -> i32;
    fn p3hip_fib_verifier_verify(v: *mut FibVerifierC, n: usize, proofs: *const *const u8, lens: *const usize, a: *const u64,
                                 b: *const u64, x: *const u64, status_out: *mut u32) -> i32;
    fn p3hip_fib_verifier_destroy(v: *mut FibVerifierC);
}

fn last_error() -> String {
    let p = unsafe { p3hip_take_last_error() };
    if p.is_null() {
        return String::from("unknown libp3hip error");
    }
    unsafe { std::ffi::CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

/// `prove(&config, &FibonacciAir {}, trace, pis)` (fib_air.rs:61,68-70) in the reference's configuration (Keccak hashes,
/// MerkleTreeHidingMmcs + HidingFriPcs seeded with 1, create_test_fri_params(_, 2)) for a trace the CALLER built, with the public
/// values the caller chose: the proof bytes (wire format version 2), or the library's error text.  BabyBear is
/// `#[repr(transparent)]` over its Montgomery `u32` (backend_hip.rs), so the trace and the public values are handed over as they
/// lie in memory.  As upstream's release builds, a trace that is no Fibonacci trace, or pis it does not satisfy, is proven all
/// the same and `verify` rejects the proof; debug builds check the constraints first (P3HIP_PROVE_CHECK_TRACE), as upstream's do.
pub fn prove_fib_air_hip(trace: &RowMajorMatrix<Val>, pis: &[Val]) -> Result<Vec<u8>, String> {
    let (h, w) = (trace.height(), trace.width());
    if w != 2 || pis.len() != 3 || !h.is_power_of_two() {
        return Err(format!("fib_air: expected a 2^k x 2 trace and 3 public values, got {h} x {w} and {}", pis.len()));
    }
    let params = FriParamsC { log_blowup: 2, log_final_poly_len: 2, num_queries: 2, proof_of_work_bits: 1 };
    let flags: u32 = if cfg!(debug_assertions) { 1 } else { 0 }; // P3HIP_PROVE_CHECK_TRACE
    let mut prover: *mut FibProverC = core::ptr::null_mut();
    let log_n = h.trailing_zeros();
    if unsafe { p3hip_fib_prover_create_hiding(P3HIP_HASH_KECCAK, log_n, &params, 1, core::ptr::null_mut(), 1, &mut prover) } != 0 {
        return Err(last_error());
    }
    let mut proof: *const u8 = core::ptr::null();
    let mut len = 0usize;
    let rc = unsafe {
        p3hip_fib_prover_prove_trace(prover, trace.values.as_ptr() as *const u32, h, pis.as_ptr() as *const u32, flags,
                                     &mut proof, &mut len)
    };
    let out = if rc == 0 { Ok(unsafe { core::slice::from_raw_parts(proof, len) }.to_vec()) } else { Err(last_error()) };
    unsafe { p3hip_fib_prover_destroy(prover) };
    out
}

fn text_of(buf: &[c_char]) -> String {
    unsafe { std::ffi::CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
}

/// The reference reports failures as `Err(String)` and lib.rs prefixes them ("fib_air zk failed: {err}", lib.rs:48): strip
/// the prefix libp3hip already wrote so the Java side sees the same text either way.
fn into_result(text: String, prefix: &str) -> Result<String, String> {
    match text.strip_prefix(prefix) {
        Some(err) => Err(err.to_string()),
        // an otherwise-ok report may carry a trailing "\nHIP error: .." (a message left in the mailbox by a call that then fell
        // back): it stays part of the Ok text, exactly as lib.rs:60-75 appends "\nVulkan error: .." to a SUCCESSFUL report
        None => Ok(text),
    }
}

pub fn run_fib_air_zk_hip() -> Result<String, String> {
    let mut buf = vec![0 as c_char; 1024];
    unsafe { p3hip_run_fib_air_zk(buf.as_mut_ptr(), buf.len()) };
    into_result(text_of(&buf), "fib_air zk failed: ")
}

/// CPU column of the benchmark: Plonky3's Radix2DitParallel on the words libp3hip hands over (BabyBear is
/// `#[repr(transparent)]` over its Montgomery u32, backend_hip.rs).
unsafe extern "C" fn cpu_dft_cb(user: *mut c_void, input: *const u32, out: *mut u32, height: usize, width: usize) -> i32 {
    let cpu = &*(user as *const GpuDft<Val>);
    let src = core::slice::from_raw_parts(input as *const Val, height * width);
    // GpuDft holds no interior state a panic could leave half-updated; the closure borrows it and a fresh Vec
    let res = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| cpu.dft_batch(RowMajorMatrix::new(src.to_vec(), width)).to_row_major_matrix()));
    match res {
        Ok(m) => {
            core::ptr::copy_nonoverlapping(m.values.as_ptr() as *const u32, out, height * width);
            0
        }
        Err(_) => 1,
    }
}

pub fn run_dft_benchmark_hip() -> Result<String, String> {
    let cpu = GpuDft::<Val>::with_backend(BackendKind::Cpu);
    let mut buf = vec![0 as c_char; 1 << 14];
    unsafe {
        p3hip_run_dft_benchmark(
            Some(cpu_dft_cb),
            &cpu as *const GpuDft<Val> as *mut c_void,
            buf.as_mut_ptr(),
            buf.len(),
        )
    };
    into_result(text_of(&buf), "dft benchmark failed: ")
}
