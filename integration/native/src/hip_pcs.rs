// NEVER COMPILED HERE (no Rust toolchain in the build image; p3-* 0.4.2 path dependencies absent).
//
// native/src/hip_pcs.rs — `HipPcs`: the `Pcs<Challenge, Challenger>` the reference builds at native/src/fib_air.rs:62-65, with
// commit / get_evaluations_on_domain / open on the device (libp3hip's TwoAdicFriPcs over caller matrices: include/p3hip.h
// "TwoAdicFriPcs over CALLER-SUPPLIED matrices" and "HidingFriPcs over CALLER-SUPPLIED matrices") and verify on the host, or for batches of one shape on the device (HipPcsVerifier).  Every matrix
// of one open has the same height, which is what p3_uni_stark hands a PCS (trace, preprocessed trace, quotient chunks).
//
//     let pcs = HipPcs::keccak(fri_params);        // the reference's hashes (fib_air.rs:28-53), non-hiding
//     let pcs = HipPcs::poseidon2(fri_params);     // north_star's configuration, non-hiding
//     let pcs = HipPcs::hiding(P3HIP_HASH_KECCAK, fri_params, 4, 1, 1);   // the PCS the reference builds (fib_air.rs:40-65)
//
// The Fiat-Shamir transcript lives in a `HipChallenger` (p3hip_challenger_*): the library hands it to the device for the open and
// back, so it must be the library's own object; it implements the p3-challenger traits uni-stark uses by forwarding.
// Trait shapes are those of p3-commit / p3-challenger 0.4.2 as recalled (the crates are not in this container) — [UPSTREAM-RECALL].
use core::ffi::c_void;

use p3_baby_bear::BabyBear;
use p3_challenger::{CanObserve, CanSample, CanSampleBits};
use p3_field::coset::TwoAdicMultiplicativeCoset;
use p3_field::extension::BinomialExtensionField;
use p3_field::PrimeField32;
use p3_fri::FriParameters;
use p3_matrix::dense::RowMajorMatrix;
use p3_matrix::Matrix;

pub type Val = BabyBear;
pub type Challenge = BinomialExtensionField<Val, 4>;

pub const P3HIP_HASH_POSEIDON2: i32 = 0;
pub const P3HIP_HASH_KECCAK: i32 = 1;
pub const P3HIP_PROFILE_LATENCY: i32 = 2;

#[repr(C)]
pub struct p3hip_fri_params_t {
    pub log_blowup: u32,
    pub log_final_poly_len: u32,
    pub num_queries: u32,
    pub proof_of_work_bits: u32,
}
#[repr(C)]
pub struct p3hip_challenger_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct p3hip_pcs_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct p3hip_pcs_data_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct p3hip_pcs_verifier_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct p3hip_pcs_shape_t {
    pub log_h: u32,
    pub n_rounds: usize,
    pub mats_per_round: *const usize,
    pub widths: *const usize,
    pub points_per_mat: *const usize,
    pub n_slots: usize,
    pub slots: *const u32,
}
pub const P3HIP_CHALLENGER_STATE_WORDS: usize = 128;
pub const P3HIP_VERIFY_MALFORMED: u32 = 16;

// include/p3hip.h
extern "C" {
    fn p3hip_take_last_error() -> *const core::ffi::c_char;
    fn p3hip_challenger_create(hash: i32, out: *mut *mut p3hip_challenger_t) -> i32;
    fn p3hip_challenger_observe(c: *mut p3hip_challenger_t, monty_words: *const u32, n: usize) -> i32;
    fn p3hip_challenger_observe_digest(c: *mut p3hip_challenger_t, digest: *const u32) -> i32;
    fn p3hip_challenger_sample_ext(c: *mut p3hip_challenger_t, out: *mut u32) -> i32;
    fn p3hip_challenger_sample_bits(c: *mut p3hip_challenger_t, bits: u32, out: *mut u32) -> i32;
    fn p3hip_challenger_clone(c: *const p3hip_challenger_t, out: *mut *mut p3hip_challenger_t) -> i32;
    fn p3hip_challenger_destroy(c: *mut p3hip_challenger_t);
    fn p3hip_pcs_create(
        profile: i32,
        hash: i32,
        params: *const p3hip_fri_params_t,
        stream: *mut c_void,
        own_stream: i32,
        out: *mut *mut p3hip_pcs_t,
    ) -> i32;
    fn p3hip_pcs_commit_dev(
        pcs: *mut p3hip_pcs_t,
        d_evals: *const *const u32,
        heights: *const usize,
        widths: *const usize,
        domain_shifts: *const u32,
        n_mats: usize,
        root_out: *mut u32,
        data_out: *mut *mut p3hip_pcs_data_t,
    ) -> i32;
    fn p3hip_pcs_lde_dev(
        data: *const p3hip_pcs_data_t,
        mat: usize,
        d_lde: *mut *const u32,
        height: *mut usize,
        width: *mut usize,
    ) -> i32;
    fn p3hip_pcs_open(
        pcs: *mut p3hip_pcs_t,
        rounds: *const *const p3hip_pcs_data_t,
        n_rounds: usize,
        points_per_mat: *const usize,
        points: *const u32,
        challenger: *mut p3hip_challenger_t,
        opened_out: *mut u32,
        opened_cap_words: usize,
        proof_out: *mut *const u8,
        proof_len: *mut usize,
    ) -> i32;
    fn p3hip_pcs_verify(
        hash: i32,
        params: *const p3hip_fri_params_t,
        log_h: u32,
        roots: *const u32,
        mats_per_round: *const usize,
        widths: *const usize,
        n_rounds: usize,
        points_per_mat: *const usize,
        points: *const u32,
        opened: *const u32,
        proof: *const u8,
        len: usize,
        challenger: *mut p3hip_challenger_t,
        reject_code: *mut i32,
    ) -> i32;
    fn p3hip_pcs_create_mixed(
        profile: i32,
        hash: i32,
        params: *const p3hip_fri_params_t,
        stream: *mut c_void,
        own_stream: i32,
        out: *mut *mut p3hip_pcs_t,
    ) -> i32;
    fn p3hip_pcs_verify_mixed(
        hash: i32,
        params: *const p3hip_fri_params_t,
        log_heights: *const u32,
        roots: *const u32,
        mats_per_round: *const usize,
        widths: *const usize,
        n_rounds: usize,
        points_per_mat: *const usize,
        points: *const u32,
        opened: *const u32,
        proof: *const u8,
        len: usize,
        challenger: *mut p3hip_challenger_t,
        reject_code: *mut i32,
    ) -> i32;
    fn p3hip_pcs_create_hiding(
        profile: i32,
        hash: i32,
        params: *const p3hip_fri_params_t,
        num_random_codewords: u32,
        mmcs_seed: u64,
        pcs_seed: u64,
        stream: *mut c_void,
        own_stream: i32,
        out: *mut *mut p3hip_pcs_t,
    ) -> i32;
    fn p3hip_pcs_commit_quotient_dev(
        pcs: *mut p3hip_pcs_t,
        d_chunks: *const *const u32,
        h: usize,
        width: usize,
        n_chunks: usize,
        root_out: *mut u32,
        data_out: *mut *mut p3hip_pcs_data_t,
    ) -> i32;
    fn p3hip_pcs_commit_randomization(pcs: *mut p3hip_pcs_t, log_h: u32, root_out: *mut u32, data_out: *mut *mut p3hip_pcs_data_t) -> i32;
    fn p3hip_pcs_verify_hiding(
        hash: i32,
        params: *const p3hip_fri_params_t,
        log_h: u32,
        roots: *const u32,
        mats_per_round: *const usize,
        widths: *const usize,
        n_rounds: usize,
        points_per_mat: *const usize,
        points: *const u32,
        opened: *const u32,
        proof: *const u8,
        len: usize,
        challenger: *mut p3hip_challenger_t,
        reject_code: *mut i32,
    ) -> i32;
    fn p3hip_pcs_data_free(d: *mut p3hip_pcs_data_t);
    fn p3hip_pcs_destroy(pcs: *mut p3hip_pcs_t);
    fn p3hip_challenger_export(c: *const p3hip_challenger_t, words: *mut u32) -> i32;
    fn p3hip_challenger_import(c: *mut p3hip_challenger_t, words: *const u32) -> i32;
    fn p3hip_pcs_proof_len(hash: i32, hiding: i32, params: *const p3hip_fri_params_t, shape: *const p3hip_pcs_shape_t, len_out: *mut usize) -> i32;
    fn p3hip_pcs_verifier_create(
        hash: i32,
        hiding: i32,
        params: *const p3hip_fri_params_t,
        shape: *const p3hip_pcs_shape_t,
        max_proofs: usize,
        out: *mut *mut p3hip_pcs_verifier_t,
    ) -> i32;
    fn p3hip_pcs_proof_len_mixed(
        hash: i32,
        hiding: i32,
        params: *const p3hip_fri_params_t,
        shape: *const p3hip_pcs_shape_t,
        log_heights: *const u32,
        len_out: *mut usize,
    ) -> i32;
    fn p3hip_pcs_verifier_create_mixed(
        hash: i32,
        hiding: i32,
        params: *const p3hip_fri_params_t,
        shape: *const p3hip_pcs_shape_t,
        log_heights: *const u32,
        max_proofs: usize,
        out: *mut *mut p3hip_pcs_verifier_t,
    ) -> i32;
    fn p3hip_pcs_verifier_verify(
        v: *mut p3hip_pcs_verifier_t,
        n: usize,
        proofs: *const *const u8,
        lens: *const usize,
        roots: *const u32,
        points: *const u32,
        opened: *const u32,
        challengers: *const *mut p3hip_challenger_t,
        status_out: *mut u32,
    ) -> i32;
    fn p3hip_pcs_verifier_destroy(v: *mut p3hip_pcs_verifier_t);
    fn p3hip_malloc(dev_ptr: *mut *mut c_void, bytes: usize) -> i32;
    fn p3hip_free(dev_ptr: *mut c_void) -> i32;
    fn p3hip_upload(dev_dst: *mut c_void, host_src: *const c_void, bytes: usize) -> i32;
    fn p3hip_download(host_dst: *mut c_void, dev_src: *const c_void, bytes: usize) -> i32;
}

// include/p3hip.h "caller-defined AIRs": an AIR as a validated program, its proofs verified on the host (one) and on the device (batches).
// Declarations only: what verifies the proofs p3hip_air_quotient_dev helped to make; no Rust type wraps them yet.
#[repr(C)]
pub struct p3hip_air_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct p3hip_air_verifier_t {
    _private: [u8; 0],
}
#[allow(dead_code)]
extern "C" {
    fn p3hip_air_create(
        width: usize, n_public: usize, code: *const u32, n_instr: usize, consts: *const u32, n_consts: usize, out: *mut *mut p3hip_air_t,
    ) -> i32;
    fn p3hip_air_destroy(air: *mut p3hip_air_t);
    fn p3hip_air_proof_len(air: *const p3hip_air_t, hash: i32, log_n: u32, params: *const p3hip_fri_params_t, len_out: *mut usize) -> i32;
    fn p3hip_air_verify(
        air: *const p3hip_air_t, hash: i32, log_n: u32, params: *const p3hip_fri_params_t, proof: *const u8, len: usize, pis: *const u32,
        reject_code: *mut i32,
    ) -> i32;
    fn p3hip_air_eval_ext_dev(
        air: *mut p3hip_air_t, stream: *mut c_void, d_local: *const u32, d_next: *const u32, d_pis: *const u32, d_sels: *const u32,
        d_alpha: *const u32, n: usize, d_out: *mut u32,
    ) -> i32;
    fn p3hip_air_verifier_create(
        air: *const p3hip_air_t, hash: i32, log_n: u32, params: *const p3hip_fri_params_t, max_proofs: usize, out: *mut *mut p3hip_air_verifier_t,
    ) -> i32;
    fn p3hip_air_verifier_verify_dev(
        v: *mut p3hip_air_verifier_t, d_proofs: *const u8, stride_bytes: usize, d_lens: *const u32, d_pis: *const u32, n: usize,
        d_status: *mut u32, d_rejected: *mut u32, stream: *mut c_void,
    ) -> i32;
    fn p3hip_air_verifier_verify(
        v: *mut p3hip_air_verifier_t, n: usize, proofs: *const *const u8, lens: *const usize, pis: *const u32, status_out: *mut u32,
    ) -> i32;
    fn p3hip_air_verifier_destroy(v: *mut p3hip_air_verifier_t);
}
// The prover of the same proofs as one device-resident launch chain (include/p3hip.h p3hip_air_prover_*): declarations only.
#[repr(C)]
pub struct p3hip_air_prover_t {
    _private: [u8; 0],
}
#[allow(dead_code)]
extern "C" {
    fn p3hip_air_prover_create(
        air: *const p3hip_air_t, profile: i32, hash: i32, log_n: u32, params: *const p3hip_fri_params_t, stream: *mut c_void, own_stream: i32,
        out: *mut *mut p3hip_air_prover_t,
    ) -> i32;
    fn p3hip_air_prover_prove_dev(
        prover: *mut p3hip_air_prover_t, d_trace: *const u32, pis: *const u32, flags: u32, proof_out: *mut *const u8, proof_len: *mut usize,
    ) -> i32;
    fn p3hip_air_prover_prove(
        prover: *mut p3hip_air_prover_t, host_trace: *const u32, pis: *const u32, flags: u32, proof_out: *mut *const u8, proof_len: *mut usize,
    ) -> i32;
    fn p3hip_air_prover_enqueue_dev(prover: *mut p3hip_air_prover_t, d_trace: *const u32, pis: *const u32) -> i32;
    fn p3hip_air_prover_finish(prover: *mut p3hip_air_prover_t, proof_out: *mut *const u8, proof_len: *mut usize) -> i32;
    fn p3hip_air_prover_destroy(prover: *mut p3hip_air_prover_t);
}

// BabyBear is a transparent u32 holding the Montgomery word (the same reinterpretation backend_hip.rs makes of `shift`), and
// BinomialExtensionField<Val, 4> is its four coefficients in order [UPSTREAM-RECALL]
fn vals_from_monty_words(words: Vec<u32>) -> Vec<Val> {
    words.into_iter().map(|w| unsafe { *(&w as *const u32 as *const Val) }).collect()
}
fn ext_from_monty_words(w: [u32; 4]) -> Challenge {
    unsafe { *(&w as *const [u32; 4] as *const Challenge) }
}

fn last_error(rc: i32) -> String {
    let p = unsafe { p3hip_take_last_error() };
    let msg = if p.is_null() { String::new() } else { unsafe { core::ffi::CStr::from_ptr(p) }.to_string_lossy().into_owned() };
    format!("libp3hip error {rc}: {msg}")
}

/// DuplexChallenger<Val, Poseidon2-16, 16, 8> or SerializingChallenger32<Val, HashChallenger<u8, Keccak256Hash, 32>>, inside libp3hip.
pub struct HipChallenger {
    h: *mut p3hip_challenger_t,
}
impl HipChallenger {
    pub fn new(hash: i32) -> Result<Self, String> {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { p3hip_challenger_create(hash, &mut h) };
        if rc != 0 { Err(last_error(rc)) } else { Ok(Self { h }) }
    }
}
impl Clone for HipChallenger {
    fn clone(&self) -> Self {
        let mut h = core::ptr::null_mut();
        let rc = unsafe { p3hip_challenger_clone(self.h, &mut h) };
        assert_eq!(rc, 0, "{}", last_error(rc));
        Self { h }
    }
}
impl Drop for HipChallenger {
    fn drop(&mut self) {
        unsafe { p3hip_challenger_destroy(self.h) }
    }
}
impl CanObserve<Val> for HipChallenger {
    fn observe(&mut self, value: Val) {
        let w = value.to_unique_u32(); // the Montgomery word (backend_vulkan.rs:2002-2005)
        let rc = unsafe { p3hip_challenger_observe(self.h, &w, 1) };
        assert_eq!(rc, 0, "{}", last_error(rc));
    }
}
impl CanObserve<[u32; 8]> for HipChallenger {
    // a commitment: Hash<Val, Val, 8> as 8 Montgomery words, or Hash<Val, u64, 4> as the same 32 little-endian bytes
    fn observe(&mut self, digest: [u32; 8]) {
        let rc = unsafe { p3hip_challenger_observe_digest(self.h, digest.as_ptr()) };
        assert_eq!(rc, 0, "{}", last_error(rc));
    }
}
impl CanSample<Challenge> for HipChallenger {
    fn sample(&mut self) -> Challenge {
        let mut w = [0u32; 4];
        let rc = unsafe { p3hip_challenger_sample_ext(self.h, w.as_mut_ptr()) };
        assert_eq!(rc, 0, "{}", last_error(rc));
        ext_from_monty_words(w)
    }
}
impl CanSampleBits<usize> for HipChallenger {
    fn sample_bits(&mut self, bits: usize) -> usize {
        let mut v = 0u32;
        let rc = unsafe { p3hip_challenger_sample_bits(self.h, bits as u32, &mut v) };
        assert_eq!(rc, 0, "{}", last_error(rc));
        v as usize
    }
}

/// Pcs::ProverData: the bit-reversed LDEs in HBM and their Merkle tree, owned by libp3hip.
pub struct HipPcsData {
    h: *mut p3hip_pcs_data_t,
    pub root: [u32; 8],
    pub dims: Vec<(usize, usize)>,
}
impl Drop for HipPcsData {
    fn drop(&mut self) {
        unsafe { p3hip_pcs_data_free(self.h) }
    }
}

/// What `open` returns and `verify` takes beside the opened values: the FriProof section of the wire format (DESIGN.md "proof bytes").
pub type HipFriProof = Vec<u8>;

pub struct HipPcs {
    h: *mut p3hip_pcs_t,
    hash: i32,
    params: p3hip_fri_params_t,
    /// 0: TwoAdicFriPcs; otherwise HidingFriPcs with this many random codewords (Pcs::ZK = true)
    num_random_codewords: usize,
}
impl HipPcs {
    pub fn new<M>(hash: i32, fri: &FriParameters<M>) -> Result<Self, String> {
        let params = p3hip_fri_params_t {
            log_blowup: fri.log_blowup as u32,
            log_final_poly_len: fri.log_final_poly_len as u32,
            num_queries: fri.num_queries as u32,
            proof_of_work_bits: fri.proof_of_work_bits as u32,
        };
        let mut h = core::ptr::null_mut();
        let rc = unsafe { p3hip_pcs_create(P3HIP_PROFILE_LATENCY, hash, &params, core::ptr::null_mut(), 1, &mut h) };
        if rc != 0 { Err(last_error(rc)) } else { Ok(Self { h, hash, params, num_random_codewords: 0 }) }
    }
    /// HidingFriPcs::new(dft, mmcs, fri_params, num_random_codewords, SmallRng::seed_from_u64(pcs_seed)) over a MerkleTreeHidingMmcs
    /// seeded with mmcs_seed (fib_air.rs:40-65: 4, 1, 1).  The three random streams live in the object and advance from call to call.
    pub fn hiding<M>(hash: i32, fri: &FriParameters<M>, num_random_codewords: usize, mmcs_seed: u64, pcs_seed: u64) -> Result<Self, String> {
        let params = p3hip_fri_params_t {
            log_blowup: fri.log_blowup as u32,
            log_final_poly_len: fri.log_final_poly_len as u32,
            num_queries: fri.num_queries as u32,
            proof_of_work_bits: fri.proof_of_work_bits as u32,
        };
        let mut h = core::ptr::null_mut();
        let rc = unsafe {
            p3hip_pcs_create_hiding(P3HIP_PROFILE_LATENCY, hash, &params, num_random_codewords as u32, mmcs_seed, pcs_seed,
                                    core::ptr::null_mut(), 1, &mut h)
        };
        if rc != 0 { Err(last_error(rc)) } else { Ok(Self { h, hash, params, num_random_codewords }) }
    }
    pub fn keccak<M>(fri: &FriParameters<M>) -> Result<Self, String> {
        Self::new(P3HIP_HASH_KECCAK, fri)
    }
    pub fn poseidon2<M>(fri: &FriParameters<M>) -> Result<Self, String> {
        Self::new(P3HIP_HASH_POSEIDON2, fri)
    }

    /// Pcs::commit: uploads each (domain, evaluations) pair (4hw bytes; nothing if the caller already holds them in HBM and uses
    /// commit_dev) and commits; the root is the only thing that comes back.
    pub fn commit_host(&self, evaluations: &[(TwoAdicMultiplicativeCoset<Val>, RowMajorMatrix<Val>)]) -> Result<HipPcsData, String> {
        let mut dev: Vec<*mut c_void> = Vec::new();
        let (mut hs, mut ws, mut shifts, mut dims) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
        for (domain, m) in evaluations {
            let bytes = m.height() * m.width() * 4;
            let mut p = core::ptr::null_mut();
            let rc = unsafe { p3hip_malloc(&mut p, bytes) };
            if rc != 0 { return Err(last_error(rc)); }
            let rc = unsafe { p3hip_upload(p, m.values.as_ptr() as *const c_void, bytes) };
            if rc != 0 { return Err(last_error(rc)); }
            dev.push(p);
            hs.push(m.height());
            ws.push(m.width());
            shifts.push(domain.shift().to_unique_u32());
            // a hiding commitment stores the randomized matrix: twice the rows, the random columns behind the caller's
            let k = self.num_random_codewords;
            dims.push(if k > 0 { (2 * m.height(), m.width() + k) } else { (m.height(), m.width()) });
        }
        let ptrs: Vec<*const u32> = dev.iter().map(|p| *p as *const u32).collect();
        let mut root = [0u32; 8];
        let mut h = core::ptr::null_mut();
        let rc = unsafe {
            p3hip_pcs_commit_dev(self.h, ptrs.as_ptr(), hs.as_ptr(), ws.as_ptr(), shifts.as_ptr(), ptrs.len(), root.as_mut_ptr(), &mut h)
        };
        for p in dev { unsafe { p3hip_free(p) }; } // the prover data owns the LDEs, not the evaluations
        if rc != 0 { Err(last_error(rc)) } else { Ok(HipPcsData { h, root, dims }) }
    }

    /// HidingFriPcs::commit_quotient: the chunk matrices (chunk c on GENERATOR g_(C h)^c <g_h>, C in {2, 4}) are uploaded, blinded on
    /// the device and committed in one salted tree.
    pub fn commit_quotient_host(&self, chunks: &[RowMajorMatrix<Val>]) -> Result<HipPcsData, String> {
        let mut dev: Vec<*mut c_void> = Vec::new();
        let (h, w) = chunks.first().map(|m| (m.height(), m.width())).unwrap_or((0, 0));
        for m in chunks {
            let bytes = m.height() * m.width() * 4;
            let mut p = core::ptr::null_mut();
            let rc = unsafe { p3hip_malloc(&mut p, bytes) };
            if rc != 0 { return Err(last_error(rc)); }
            let rc = unsafe { p3hip_upload(p, m.values.as_ptr() as *const c_void, bytes) };
            if rc != 0 { return Err(last_error(rc)); }
            dev.push(p);
        }
        let ptrs: Vec<*const u32> = dev.iter().map(|p| *p as *const u32).collect();
        let mut root = [0u32; 8];
        let mut d = core::ptr::null_mut();
        let rc = unsafe { p3hip_pcs_commit_quotient_dev(self.h, ptrs.as_ptr(), h, w, ptrs.len(), root.as_mut_ptr(), &mut d) };
        for p in dev { unsafe { p3hip_free(p) }; }
        if rc != 0 { Err(last_error(rc)) } else { Ok(HipPcsData { h: d, root, dims: vec![(2 * h, w); chunks.len()] }) }
    }

    /// HidingFriPcs::get_opt_randomization_poly_commitment for traces of 2^log_h rows.
    pub fn randomization_commitment(&self, log_h: u32) -> Result<HipPcsData, String> {
        let mut root = [0u32; 8];
        let mut d = core::ptr::null_mut();
        let rc = unsafe { p3hip_pcs_commit_randomization(self.h, log_h, root.as_mut_ptr(), &mut d) };
        if rc != 0 { Err(last_error(rc)) } else { Ok(HipPcsData { h: d, root, dims: vec![(2usize << log_h, self.num_random_codewords + 4)] }) }
    }

    /// Pcs::get_evaluations_on_domain for GENERATOR * <g_m>: the first m rows of the stored LDE (natural index i at row bitrev(i)).
    /// A device pointer; `download_rows` brings them to the host for a quotient computed there.
    pub fn evaluations_on_domain_dev(&self, data: &HipPcsData, idx: usize) -> Result<(*const u32, usize, usize), String> {
        let (mut p, mut h, mut w) = (core::ptr::null(), 0usize, 0usize);
        let rc = unsafe { p3hip_pcs_lde_dev(data.h, idx, &mut p, &mut h, &mut w) };
        if rc != 0 { Err(last_error(rc)) } else { Ok((p, h, w)) }
    }
    pub fn download_rows(&self, data: &HipPcsData, idx: usize, rows: usize) -> Result<RowMajorMatrix<Val>, String> {
        let (p, _, w) = self.evaluations_on_domain_dev(data, idx)?;
        let mut words = vec![0u32; rows * w];
        let rc = unsafe { p3hip_download(words.as_mut_ptr() as *mut c_void, p as *const c_void, rows * w * 4) };
        if rc != 0 { return Err(last_error(rc)); }
        Ok(RowMajorMatrix::new(vals_from_monty_words(words), w))
    }

    /// Pcs::open: rounds = (prover data, points per matrix); returns the opened values in observation order (round -> matrix ->
    /// point -> column, 4 Montgomery words each) and the FRI proof bytes; the challenger is advanced on the device.
    pub fn open_words(
        &self,
        rounds: &[(&HipPcsData, Vec<Vec<[u32; 4]>>)],
        challenger: &mut HipChallenger,
    ) -> Result<(Vec<u32>, HipFriProof), String> {
        let handles: Vec<*const p3hip_pcs_data_t> = rounds.iter().map(|(d, _)| d.h as *const _).collect();
        let (mut counts, mut points, mut total) = (Vec::new(), Vec::new(), 0usize);
        for (d, per_mat) in rounds {
            for (m, pts) in per_mat.iter().enumerate() {
                counts.push(pts.len());
                total += pts.len() * d.dims[m].1;
                for z in pts { points.extend_from_slice(z); }
            }
        }
        let mut opened = vec![0u32; 4 * total];
        let (mut proof, mut len) = (core::ptr::null(), 0usize);
        let rc = unsafe {
            p3hip_pcs_open(self.h, handles.as_ptr(), handles.len(), counts.as_ptr(), points.as_ptr(), challenger.h, opened.as_mut_ptr(),
                           opened.len(), &mut proof, &mut len)
        };
        if rc != 0 { return Err(last_error(rc)); }
        Ok((opened, unsafe { core::slice::from_raw_parts(proof, len) }.to_vec()))
    }

    /// Pcs::verify on the host: Ok(()) or the failed check's code and text.
    #[allow(clippy::too_many_arguments)]
    pub fn verify_words(
        &self,
        log_h: u32,
        roots: &[[u32; 8]],
        widths: &[Vec<usize>],
        points: &[Vec<Vec<[u32; 4]>>],
        opened: &[u32],
        proof: &[u8],
        challenger: &mut HipChallenger,
    ) -> Result<(), String> {
        let flat_roots: Vec<u32> = roots.iter().flatten().copied().collect();
        let mats: Vec<usize> = widths.iter().map(|w| w.len()).collect();
        let flat_w: Vec<usize> = widths.iter().flatten().copied().collect();
        let counts: Vec<usize> = points.iter().flatten().map(|p| p.len()).collect();
        let flat_p: Vec<u32> = points.iter().flatten().flatten().flatten().copied().collect();
        let mut code = 0i32;
        // a hiding PCS: log_h is still the caller's log height, the widths are the committed ones
        let verify = if self.num_random_codewords > 0 { p3hip_pcs_verify_hiding } else { p3hip_pcs_verify };
        let rc = unsafe {
            verify(self.hash, &self.params, log_h, flat_roots.as_ptr(), mats.as_ptr(), flat_w.as_ptr(), mats.len(), counts.as_ptr(),
                   flat_p.as_ptr(), opened.as_ptr(), proof.as_ptr(), proof.len(), challenger.h, &mut code)
        };
        if rc != 0 { return Err(last_error(rc)); }
        if code != 0 { return Err(last_error(code)); }
        Ok(())
    }
}
impl Drop for HipPcs {
    fn drop(&mut self) {
        unsafe { p3hip_pcs_destroy(self.h) }
    }
}

impl HipChallenger {
    /// The transcript as the words a device verifier imports (include/p3hip.h p3hip_challenger_export).
    pub fn export_state(&self) -> Result<[u32; P3HIP_CHALLENGER_STATE_WORDS], String> {
        let mut w = [0u32; P3HIP_CHALLENGER_STATE_WORDS];
        let rc = unsafe { p3hip_challenger_export(self.h, w.as_mut_ptr()) };
        if rc != 0 { Err(last_error(rc)) } else { Ok(w) }
    }
    pub fn import_state(&mut self, w: &[u32; P3HIP_CHALLENGER_STATE_WORDS]) -> Result<(), String> {
        let rc = unsafe { p3hip_challenger_import(self.h, w.as_ptr()) };
        if rc != 0 { Err(last_error(rc)) } else { Ok(()) }
    }
}

/// Pcs::verify for batches of members of ONE shape on the device (include/p3hip.h "batches of PCS proofs verified ON THE DEVICE").
/// widths: the committed widths per round; slots: per matrix the slot (< n_slots) of each of its opening points.
pub struct HipPcsVerifier {
    h: *mut p3hip_pcs_verifier_t,
    pub proof_len: usize,
    n_rounds: usize,
    n_slots: usize,
    total: usize,
}
impl HipPcsVerifier {
    pub fn new(pcs: &HipPcs, log_h: u32, widths: &[Vec<usize>], slots: &[Vec<Vec<u32>>], n_slots: usize, max_proofs: usize) -> Result<Self, String> {
        Self::create(pcs, log_h, None, widths, slots, n_slots, max_proofs)
    }

    /// The same for matrices of MIXED heights (p3hip_pcs_verifier_create_mixed): log_heights holds one log height per matrix, laid out
    /// as widths.  Members are verified through verify_many as those of any other shape.  A hiding PCS is refused by the library.
    pub fn new_mixed(
        pcs: &HipPcs,
        log_heights: &[Vec<u32>],
        widths: &[Vec<usize>],
        slots: &[Vec<Vec<u32>>],
        n_slots: usize,
        max_proofs: usize,
    ) -> Result<Self, String> {
        if log_heights.len() != widths.len() || log_heights.iter().zip(widths.iter()).any(|(l, w)| l.len() != w.len()) {
            return Err("new_mixed: one log height per matrix".into());
        }
        let flat_h: Vec<u32> = log_heights.iter().flatten().copied().collect();
        Self::create(pcs, 0, Some(&flat_h), widths, slots, n_slots, max_proofs)
    }

    fn create(
        pcs: &HipPcs,
        log_h: u32,
        log_heights: Option<&[u32]>,
        widths: &[Vec<usize>],
        slots: &[Vec<Vec<u32>>],
        n_slots: usize,
        max_proofs: usize,
    ) -> Result<Self, String> {
        let mats: Vec<usize> = widths.iter().map(|w| w.len()).collect();
        let flat_w: Vec<usize> = widths.iter().flatten().copied().collect();
        let counts: Vec<usize> = slots.iter().flatten().map(|s| s.len()).collect();
        let flat_s: Vec<u32> = slots.iter().flatten().flatten().copied().collect();
        let total = flat_w.iter().zip(counts.iter()).map(|(w, c)| w * c).sum();
        let shape = p3hip_pcs_shape_t {
            log_h,
            n_rounds: mats.len(),
            mats_per_round: mats.as_ptr(),
            widths: flat_w.as_ptr(),
            points_per_mat: counts.as_ptr(),
            n_slots,
            slots: flat_s.as_ptr(),
        };
        let hiding = (pcs.num_random_codewords > 0) as i32;
        let (mut h, mut proof_len) = (core::ptr::null_mut(), 0usize);
        let rc = unsafe {
            match log_heights {
                Some(lh) => p3hip_pcs_proof_len_mixed(pcs.hash, hiding, &pcs.params, &shape, lh.as_ptr(), &mut proof_len),
                None => p3hip_pcs_proof_len(pcs.hash, hiding, &pcs.params, &shape, &mut proof_len),
            }
        };
        if rc != 0 { return Err(last_error(rc)); }
        let rc = unsafe {
            match log_heights {
                Some(lh) => p3hip_pcs_verifier_create_mixed(pcs.hash, hiding, &pcs.params, &shape, lh.as_ptr(), max_proofs, &mut h),
                None => p3hip_pcs_verifier_create(pcs.hash, hiding, &pcs.params, &shape, max_proofs, &mut h),
            }
        };
        if rc != 0 { return Err(last_error(rc)); }
        Ok(Self { h, proof_len, n_rounds: mats.len(), n_slots, total })
    }

    /// One status per member: 0 = accept, 11 / 13 / 14 / 15 the host verifier's code, 16 malformed.  roots: n_rounds x 8 words per
    /// member, points: n_slots x 4, opened: total x 4.  An accepted member's challenger is advanced, a rejected member's is left alone.
    pub fn verify_many(
        &mut self,
        proofs: &[&[u8]],
        roots: &[u32],
        points: &[u32],
        opened: &[u32],
        challengers: &mut [HipChallenger],
    ) -> Result<Vec<u32>, String> {
        let n = proofs.len();
        if challengers.len() != n || roots.len() != n * self.n_rounds * 8 || points.len() != n * self.n_slots * 4 || opened.len() != n * self.total * 4 {
            return Err("verify_many: one challenger, n_rounds roots, n_slots points and `total` opened values per proof".into());
        }
        let ptrs: Vec<*const u8> = proofs.iter().map(|p| p.as_ptr()).collect();
        let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
        let chals: Vec<*mut p3hip_challenger_t> = challengers.iter().map(|c| c.h).collect();
        let mut status = vec![0u32; n];
        let rc = unsafe {
            p3hip_pcs_verifier_verify(self.h, n, ptrs.as_ptr(), lens.as_ptr(), roots.as_ptr(), points.as_ptr(), opened.as_ptr(), chals.as_ptr(),
                                      status.as_mut_ptr())
        };
        if rc != 0 { return Err(last_error(rc)); }
        Ok(status)
    }
}
impl Drop for HipPcsVerifier {
    fn drop(&mut self) {
        unsafe { p3hip_pcs_verifier_destroy(self.h) }
    }
}

// `impl Pcs<Challenge, HipChallenger> for HipPcs` (p3-commit 0.4.2, as recalled): Domain = TwoAdicMultiplicativeCoset<Val>,
// Commitment = [u32; 8] digest words, ProverData = HipPcsData, EvaluationsOnDomain = RowMajorMatrix<Val> (download_rows), Proof =
// HipFriProof, Error = String.  natural_domain_for_degree is TwoAdicFriPcs's own; commit = commit_host; get_evaluations_on_domain =
// download_rows of the first `domain.size()` rows, un-bit-reversed by the caller's `.bit_reverse_rows()`; open = open_words with the
// points' Montgomery words, reshaped into OpenedValues<Challenge> (round -> matrix -> point -> column is already upstream's nesting);
// verify = verify_words over the same flattening.  The trait impl itself is left to the crate that has p3-commit to compile against.
