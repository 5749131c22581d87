//! Rust side of `libtyplonk_hip.so` -- the safe layer a TyPLONK maintainer calls from the `kzg` and `plonk` crates.
//!
//! SOURCE ONLY: this repository's image has no Rust toolchain, so nothing in this crate has been through `rustc`.
//! What IS tested is the C side every function here forwards to (`include/typlonk.h`, exercised through ctypes and
//! through the C++ mirror `typlonk_amd/host/typlonk_host.hpp`, which has the same shape as this file).
//!
//! Seams (file:line under the reference):
//!   * `Backend::msm`            replaces the body of `KzgScheme::evaluate_in_s`      kzg/src/lib.rs:41-54
//!   * `Backend::upload_srs`     once per `Srs` (`Srs::from_secret`)                  kzg/src/srs.rs:30-34
//!   * `Backend::interpolate` / `interpolate_batch` / `evaluate_over_domain`
//!                               replace `Evaluations::interpolate()` / `evaluate_over_domain()`
//!                               plonk/src/proof.rs:50,106,115,125,128  plonk/src/builder.rs:85
//!   * `Backend::load_circuit` + `Backend::prove`
//!                               replace the body of `plonk::proof::prove`           plonk/src/proof.rs:96-194
//!   * `Backend::verify_batch`   replaces `plonk::proof::verify` for a batch          plonk/src/proof.rs:195-281
//!   * `Backend::prove_compact` / `prove_batch_compact` / `verifying_key` / `verify_compact`
//!                               the compact proof shape of include/typlonk.h (batched openings; no counterpart there)
//!   * `proof_to_bytes` / `vk_to_bytes` / `vk_from_bytes` / `Backend::proofs_from_bytes` / `verify_compact_bytes` /
//!     `upload_srs_compressed` / `download_srs_compressed`
//!                               the wire format of include/typlonk.h: compressed points, subgroup-checked on the way in
//!
//! Data crosses the boundary in arkworks' own in-memory form (`Fp256.0 .0`: 4 LE u64 limbs of the Montgomery residue;
//! `Fp384.0 .0`: 6), so nothing is converted -- coordinates are copied limb-wise because `GroupAffine` is `repr(Rust)`.
pub mod ffi;

use ark_bls12_381::{Fq, Fr, G1Affine};
use ark_ff::{BigInteger256, BigInteger384, Zero};
use ark_poly::{univariate::DensePolynomial, UVPolynomial};
use std::ffi::CStr;
use std::os::raw::c_int;
use std::ptr;

pub type G1Point = G1Affine;
pub type Poly = DensePolynomial<Fr>;
/// `TYPLONK_VERIFY_PI_AS_PROVER` of include/typlonk.h (a flag of `typlonk_verify`)
pub const VERIFY_PI_AS_PROVER: u32 = 1;
/// `TYPLONK_CELL_NONE` of include/typlonk.h (`circuit_permutation`: a sigma value that is the id of no cell)
pub const CELL_NONE: u32 = 0xffff_ffff;
/// `TYPLONK_DECODE_SKIP_SUBGROUP` of include/typlonk.h (a flag of the `*_from_bytes` / `*_compressed` calls)
pub const DECODE_SKIP_SUBGROUP: u32 = 1;

/// Why a byte string was refused: the reject class (`TYPLONK_POINT_*` / `TYPLONK_SCALAR_RANGE`) of the first bad field and
/// that field's index in wire order (`TYPLONK_DECODE_CLASS` / `TYPLONK_DECODE_FIELD` of a decode status).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct DecodeError {
    pub class: u32,
    pub field: u32,
}
impl DecodeError {
    fn from_status(status: u32) -> Option<DecodeError> {
        if status == 0 { None } else { Some(DecodeError { class: status & 0xff, field: status >> 8 }) }
    }
}

/// `typlonk_proof_compact_to_bytes` (host-only): the 656-byte wire form.  `None` for a field that is not canonical or a
/// point that is not on the curve.
pub fn proof_to_bytes(proof: &ffi::TyplonkProofCompact) -> Option<[u8; ffi::TYPLONK_PROOF_COMPACT_BYTES]> {
    let mut out = [0u8; ffi::TYPLONK_PROOF_COMPACT_BYTES];
    if unsafe { ffi::typlonk_proof_compact_to_bytes(proof, out.as_mut_ptr()) } == ffi::TYPLONK_OK { Some(out) } else { None }
}
/// `typlonk_vk_to_bytes` (host-only): the 628-byte wire form of a verifying key.
pub fn vk_to_bytes(vk: &ffi::TyplonkVk) -> Option<[u8; ffi::TYPLONK_VK_WIRE_BYTES]> {
    let mut out = [0u8; ffi::TYPLONK_VK_WIRE_BYTES];
    if unsafe { ffi::typlonk_vk_to_bytes(vk, out.as_mut_ptr()) } == ffi::TYPLONK_OK { Some(out) } else { None }
}
/// `typlonk_vk_from_bytes` (host-only; a verifier needs nothing else): every point on the curve and in the subgroup.
/// `Err((code, status))`: the library's error code and, for a rejected field, what was wrong with it.
pub fn vk_from_bytes(bytes: &[u8; ffi::TYPLONK_VK_WIRE_BYTES], flags: u32) -> Result<ffi::TyplonkVk, (c_int, Option<DecodeError>)> {
    let mut vk = std::mem::MaybeUninit::<ffi::TyplonkVk>::zeroed();
    let mut status = 0u32;
    let rc = unsafe { ffi::typlonk_vk_from_bytes(bytes.as_ptr(), flags, vk.as_mut_ptr(), &mut status) };
    if rc == ffi::TYPLONK_OK { Ok(unsafe { vk.assume_init() }) } else { Err((rc, DecodeError::from_status(status))) }
}

/// One HIP device + stream + workspaces (`typlonk_ctx`).  It holds a raw pointer, so it is neither `Send` nor `Sync`
/// -- and therefore neither is anything that embeds it (`kzg::srs::Srs`, `plonk::CompiledCircuit` after the patches):
/// one host thread per context, as typlonk.h requires.  A program that proves on several threads gives each thread its
/// own `Backend::shared` (the registry is thread-local) or wraps the calls in its own lock.
pub struct Backend {
    ctx: *mut ffi::TyplonkCtx,
}

thread_local! {
    // Backend::shared: one context per (thread, device ordinal), created on first use
    static SHARED: std::cell::RefCell<Vec<(i32, std::rc::Rc<Backend>)>> = std::cell::RefCell::new(Vec::new());
}

/// the device this process works on: `TYPLONK_DEVICE` (default 0).  One process per GPU: the launcher sets it per rank.
pub fn device_from_env() -> i32 {
    std::env::var("TYPLONK_DEVICE").ok().and_then(|v| v.parse().ok()).unwrap_or(0)
}
/// fixed-base window tables for an uploaded SRS are opt-in (`TYPLONK_TABLES=1`): they multiply the SRS's footprint in
/// HBM by 13-17 and only pay when many commitments follow (a prover; not a one-off `commit`)
pub fn tables_from_env() -> bool {
    std::env::var("TYPLONK_TABLES").map(|v| v != "0" && !v.is_empty()).unwrap_or(false)
}

/// An SRS resident in HBM (`typlonk_srs_load`), with the fixed-base tables the library chooses for its length.
#[derive(Debug, Clone, Copy)]
pub struct SrsHandle {
    pub id: u32,
    pub len: usize,
}

/// Per-circuit constants of the quotient on the device (`typlonk_circuit_load`): selectors and sigmas on the 4n coset.
#[derive(Debug, Clone, Copy)]
pub struct CircuitHandle {
    pub id: u32,
    pub log_n: u32,
}

/// A device-resident vector of Fr (`typlonk_buf`), freed on drop.
pub struct DeviceVec<'a> {
    backend: &'a Backend,
    buf: *mut ffi::TyplonkBuf,
}

impl std::fmt::Debug for Backend {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "typlonk::Backend({:p})", self.ctx)
    }
}

fn fr_limbs(x: &Fr) -> [u64; 4] {
    (x.0).0
}
fn fr_from_limbs(l: [u64; 4]) -> Fr {
    // the limbs ARE the Montgomery residue: construct without a conversion (ark-ff 0.3: `Fp256::new(BigInteger256)`)
    Fr::new(BigInteger256(l))
}
fn g1_from_abi(xy: &[u64; 12], inf: u8) -> G1Point {
    let mut x = [0u64; 6];
    let mut y = [0u64; 6];
    x.copy_from_slice(&xy[0..6]);
    y.copy_from_slice(&xy[6..12]);
    // identity comes back as (0, 1, inf = 1) = GroupAffine::zero()
    G1Point::new(Fq::new(BigInteger384(x)), Fq::new(BigInteger384(y)), inf != 0)
}

impl Backend {
    /// `typlonk_init`: fails (panics, like the reference's `unwrap()`s) when there is no HIP device -- no CPU fallback.
    pub fn new(device_ordinal: i32) -> Self {
        let mut ctx = ptr::null_mut();
        let rc = unsafe { ffi::typlonk_init(&mut ctx, device_ordinal as c_int) };
        if rc != ffi::TYPLONK_OK {
            panic!("typlonk_init: {}", strerror(rc));
        }
        Backend { ctx }
    }

    /// negative code -> panic with the library's message: the reference panics at the same places
    /// (`TYPLONK_ERR_LENGTH` <=> `assert!(srs.len() > polynomial.degree())`, kzg/src/lib.rs:43)
    fn check(&self, rc: c_int) {
        if rc != ffi::TYPLONK_OK {
            let detail = unsafe { CStr::from_ptr(ffi::typlonk_last_error(self.ctx)) }.to_string_lossy().into_owned();
            panic!("{}: {}", strerror(rc), detail);
        }
    }

    /// The context of this thread for `device_ordinal`, created on first use and shared by every `Srs` /
    /// `CompiledCircuit` of the thread: `Srs::from_secret` must not open a context (streams, workspaces, an SRS upload)
    /// per call.
    pub fn shared(device_ordinal: i32) -> std::rc::Rc<Backend> {
        SHARED.with(|reg| {
            let mut reg = reg.borrow_mut();
            if let Some((_, b)) = reg.iter().find(|(d, _)| *d == device_ordinal) {
                return b.clone();
            }
            let b = std::rc::Rc::new(Backend::new(device_ordinal));
            reg.push((device_ordinal, b.clone()));
            b
        })
    }

    // ---- SRS ------------------------------------------------------------------------------------------------------
    /// once per `Srs` (kzg/src/srs.rs:30-34): copy the G1 powers to HBM; `tables`: also build the fixed-base window
    /// tables (`precompute_tables`)
    pub fn upload_srs(&self, g1: &[G1Point], tables: bool) -> SrsHandle {
        let mut xy = Vec::with_capacity(g1.len() * 12);
        let mut inf = Vec::with_capacity(g1.len());
        for p in g1 {
            xy.extend_from_slice(&(p.x.0).0);
            xy.extend_from_slice(&(p.y.0).0);
            inf.push(p.infinity as u8);
        }
        let mut id = 0u32;
        self.check(unsafe { ffi::typlonk_srs_load(self.ctx, xy.as_ptr(), inf.as_ptr(), g1.len(), &mut id) });
        let h = SrsHandle { id, len: g1.len() };
        if tables {
            self.precompute_tables(h);
        }
        h
    }

    /// `typlonk_srs_free`: the device copy of an SRS and its fixed-base tables (13-17 x the SRS when built).  Called by
    /// `OwnedSrs::drop`; a handle must not be used afterwards.
    pub fn free_srs(&self, srs: SrsHandle) {
        self.check(unsafe { ffi::typlonk_srs_free(self.ctx, srs.id) });
    }
    /// `typlonk_circuit_free`: the per-circuit coset evaluations (9 x 4n + 11 x n Fr).  Called by `OwnedCircuit::drop`.
    pub fn free_circuit(&self, circuit: CircuitHandle) {
        self.check(unsafe { ffi::typlonk_circuit_free(self.ctx, circuit.id) });
    }

    /// `typlonk_srs_precompute`: speed only, results unchanged; the window is chosen by length (nothing at all below
    /// TYPLONK_TABLES_AUTO_MIN_LEN points).  13-17 copies of the SRS in HBM.
    pub fn precompute_tables(&self, srs: SrsHandle) {
        self.check(unsafe { ffi::typlonk_srs_precompute(self.ctx, srs.id, 0) });
    }

    /// `Srs::from_secret` on the device: `[s^(start + i)] G`, i < len (each GPU of a node builds only its shard)
    pub fn generate_srs(&self, secret: &Fr, start: u64, len: usize, tables: bool) -> SrsHandle {
        let s = fr_limbs(secret);
        let mut id = 0u32;
        self.check(unsafe { ffi::typlonk_srs_generate(self.ctx, s.as_ptr(), start, len, &mut id) });
        let h = SrsHandle { id, len };
        if tables {
            self.precompute_tables(h);
        }
        h
    }

    // ---- MSM seam: the body of KzgScheme::evaluate_in_s (kzg/src/lib.rs:41-54) -------------------------------------
    /// sum_i coeffs[i] * srs[i].  `coeffs` are the polynomial's coefficients with ark-poly's trailing-zero trim, so the
    /// MSM length is what the reference's `zip` would have consumed.
    pub fn msm(&self, srs: SrsHandle, coeffs: &[Fr]) -> G1Point {
        let mut scalars = Vec::with_capacity(coeffs.len() * 4);
        for c in coeffs {
            scalars.extend_from_slice(&fr_limbs(c));
        }
        let (mut xy, mut inf) = ([0u64; 12], 0u8);
        self.check(unsafe {
            ffi::typlonk_msm_g1(self.ctx, srs.id, scalars.as_ptr(), coeffs.len(), xy.as_mut_ptr(), &mut inf)
        });
        g1_from_abi(&xy, inf)
    }

    /// the same with the coefficients already in HBM (an iNTT result feeding a commitment: proof.rs:50 -> :109)
    pub fn msm_dev(&self, srs: SrsHandle, v: &DeviceVec, offset: usize, m: usize) -> G1Point {
        let (mut xy, mut inf) = ([0u64; 12], 0u8);
        self.check(unsafe { ffi::typlonk_msm_g1_dev(self.ctx, srs.id, v.buf, offset, m, xy.as_mut_ptr(), &mut inf) });
        g1_from_abi(&xy, inf)
    }

    // ---- NTT seam ---------------------------------------------------------------------------------------------------
    /// `Evaluations::from_vec_and_domain(evals, domain).interpolate()`: ifft, then ark-poly's trailing-zero trim
    /// (`from_coefficients_vec`), which is what sets MSM lengths downstream
    pub fn interpolate(&self, mut evals: Vec<Fr>, log_n: u32) -> Poly {
        assert_eq!(evals.len(), 1usize << log_n);
        let mut limbs: Vec<u64> = evals.iter().flat_map(|e| fr_limbs(e)).collect();
        self.check(unsafe { ffi::typlonk_ntt_fr(self.ctx, limbs.as_mut_ptr(), log_n, 1, ptr::null()) });
        for (e, l) in evals.iter_mut().zip(limbs.chunks_exact(4)) {
            *e = fr_from_limbs([l[0], l[1], l[2], l[3]]);
        }
        Poly::from_coefficients_vec(evals)
    }

    /// A GROUP of interpolations in one call -- the three wire columns (plonk/src/proof.rs:50), the three sigma columns
    /// (:334-338), the five selector columns (plonk/src/builder.rs:84-88): one upload, ONE `typlonk_ntt_fr_batch_devptr`
    /// (every pass of the transform is a single launch carrying all the columns), one download; each result gets ark-poly's
    /// trailing-zero trim like `interpolate`.
    pub fn interpolate_batch(&self, columns: Vec<Vec<Fr>>, log_n: u32) -> Vec<Poly> {
        let n = 1usize << log_n;
        let count = columns.len();
        if count == 0 {
            return Vec::new();
        }
        let mut limbs: Vec<u64> = Vec::with_capacity(4 * n * count);
        for col in &columns {
            assert_eq!(col.len(), n);
            limbs.extend(col.iter().flat_map(|e| fr_limbs(e)));
        }
        let mut buf = ptr::null_mut();
        self.check(unsafe { ffi::typlonk_buf_alloc(self.ctx, n * count, &mut buf) });
        let dev = DeviceVec { backend: self, buf }; // freed on drop, also when a check below panics
        self.check(unsafe { ffi::typlonk_buf_upload(self.ctx, dev.buf, 0, limbs.as_ptr(), n * count) });
        let base = unsafe { ffi::typlonk_buf_devptr(dev.buf) } as *mut u8;
        let ptrs: Vec<*mut std::os::raw::c_void> =
            (0..count).map(|v| unsafe { base.add(32 * n * v) } as *mut std::os::raw::c_void).collect();
        self.check(unsafe { ffi::typlonk_ntt_fr_batch_devptr(self.ctx, ptrs.as_ptr(), count, log_n, 1, ptr::null()) });
        self.check(unsafe { ffi::typlonk_buf_download(self.ctx, dev.buf, 0, limbs.as_mut_ptr(), n * count) });
        limbs
            .chunks_exact(4 * n)
            .map(|col| Poly::from_coefficients_vec(col.chunks_exact(4).map(|l| fr_from_limbs([l[0], l[1], l[2], l[3]])).collect()))
            .collect()
    }

    /// `poly.evaluate_over_domain(domain).evals`: zero-pad to the domain size, fft, natural order
    pub fn evaluate_over_domain(&self, poly: &Poly, log_n: u32) -> Vec<Fr> {
        let n = 1usize << log_n;
        assert!(poly.coeffs.len() <= n);
        let mut limbs = vec![0u64; 4 * n];
        for (c, l) in poly.coeffs.iter().zip(limbs.chunks_exact_mut(4)) {
            l.copy_from_slice(&fr_limbs(c));
        }
        self.check(unsafe { ffi::typlonk_ntt_fr(self.ctx, limbs.as_mut_ptr(), log_n, 0, ptr::null()) });
        limbs.chunks_exact(4).map(|l| fr_from_limbs([l[0], l[1], l[2], l[3]])).collect()
    }

    // ---- device vectors ---------------------------------------------------------------------------------------------
    pub fn upload(&self, v: &[Fr], capacity: usize) -> DeviceVec<'_> {
        let mut buf = ptr::null_mut();
        self.check(unsafe { ffi::typlonk_buf_alloc(self.ctx, capacity.max(v.len()), &mut buf) });
        let d = DeviceVec { backend: self, buf };
        self.check(unsafe { ffi::typlonk_buf_zero(self.ctx, buf, 0, capacity.max(v.len())) });
        let limbs: Vec<u64> = v.iter().flat_map(|e| fr_limbs(e)).collect();
        self.check(unsafe { ffi::typlonk_buf_upload(self.ctx, buf, 0, limbs.as_ptr(), v.len()) });
        d
    }

    // ---- whole prover ---------------------------------------------------------------------------------------------
    /// once per `CompiledCircuit` (plonk/src/lib.rs:19-35): the five selector polynomials (coefficients, zero-padded
    /// to n) and the three sigma polynomials (`interpolate` of `copy_constrains.cols[i]`'s second components)
    pub fn load_circuit(&self, selectors: [&Poly; 5], sigma: [&Poly; 3], log_n: u32) -> CircuitHandle {
        let n = 1usize << log_n;
        let sel: Vec<DeviceVec> = selectors.iter().map(|p| self.upload(&p.coeffs, n)).collect();
        let sig: Vec<DeviceVec> = sigma.iter().map(|p| self.upload(&p.coeffs, n)).collect();
        let selp: Vec<*const ffi::TyplonkBuf> = sel.iter().map(|d| d.buf as *const _).collect();
        let sigp: Vec<*const ffi::TyplonkBuf> = sig.iter().map(|d| d.buf as *const _).collect();
        let mut id = 0u32;
        self.check(unsafe { ffi::typlonk_circuit_load(self.ctx, selp.as_ptr(), sigp.as_ptr(), log_n, &mut id) });
        CircuitHandle { id, log_n }
    }

    /// The same circuit from what the front end holds before `Permutation::compile` (permutation/src/lib.rs:101-128): the five
    /// selector columns as EVALUATIONS over the domain and the permutation itself, `perm` = 3n successors over the flat cells
    /// `col * n + row` (`None`: no copy constraints).  `typlonk_circuit_compile_host` makes the sigma columns and interpolates
    /// all eight on the device, and keeps the permutation with the circuit, so `check_witnesses` never recovers it.
    /// Panics, with the number of defects and the lowest defective cell, when `perm` is no permutation of the cells.
    pub fn compile_circuit(&self, selector_evals: [&[Fr]; 5], perm: Option<&[u32]>, cosets: [Fr; 3], log_n: u32) -> CircuitHandle {
        let n = 1usize << log_n;
        assert!(selector_evals.iter().all(|c| c.len() == n), "selector columns of n evaluations");
        assert!(perm.map_or(true, |p| p.len() == 3 * n), "perm holds 3n successors");
        let cols: Vec<Vec<u64>> = selector_evals.iter().map(|c| c.iter().flat_map(|e| fr_limbs(e)).collect()).collect();
        let colp: Vec<*const u64> = cols.iter().map(|c| c.as_ptr()).collect();
        let ks = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let (mut id, mut defects) = (0u32, 0u64);
        self.check(unsafe {
            ffi::typlonk_circuit_compile_host(self.ctx, colp.as_ptr(), n, perm.map_or(ptr::null(), |p| p.as_ptr()), ks.as_ptr(), log_n,
                                              &mut id, &mut defects)
        });
        CircuitHandle { id, log_n }
    }

    /// The same from what the front end holds before `PermutationBuilder::build` (permutation/src/lib.rs:48-93): the copy
    /// constraints themselves, `pairs` of flat cells `col * n + row` that must carry one value.  The library makes the canonical
    /// permutation of their classes on the device (every class ascending, the same for any order of the pairs and on every
    /// run -- `build` walks a `HashMap`) and compiles from it without the map visiting the host.  Returns the circuit and the
    /// number of classes among the 3n cells.  Panics, with the lowest bad pair named, when a pair names a cell outside the table.
    pub fn compile_circuit_from_pairs(&self, selector_evals: [&[Fr]; 5], pairs: &[[u32; 2]], cosets: [Fr; 3], log_n: u32) -> (CircuitHandle, u64) {
        let n = 1usize << log_n;
        assert!(selector_evals.iter().all(|c| c.len() == n), "selector columns of n evaluations");
        let cols: Vec<Vec<u64>> = selector_evals.iter().map(|c| c.iter().flat_map(|e| fr_limbs(e)).collect()).collect();
        let colp: Vec<*const u64> = cols.iter().map(|c| c.as_ptr()).collect();
        let ks = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let (mut id, mut classes) = (0u32, 0u64);
        let pp = if pairs.is_empty() { ptr::null() } else { pairs.as_ptr() as *const u32 };
        self.check(unsafe {
            ffi::typlonk_circuit_compile_pairs_host(self.ctx, colp.as_ptr(), n, pp, pairs.len(), ks.as_ptr(), log_n, &mut id, &mut classes)
        });
        (CircuitHandle { id, log_n }, classes)
    }

    /// `typlonk_permutation_from_pairs`: the canonical permutation alone, as `(perm, classes)`.
    pub fn permutation_from_pairs(&self, pairs: &[[u32; 2]], log_n: u32) -> (Vec<u32>, u64) {
        assert!((1..=24).contains(&log_n), "1 <= log_n <= 24");
        let mut perm = vec![0u32; 3usize << log_n];
        let mut classes = 0u64;
        let pp = if pairs.is_empty() { ptr::null() } else { pairs.as_ptr() as *const u32 };
        self.check(unsafe { ffi::typlonk_permutation_from_pairs(self.ctx, pp, pairs.len(), log_n, perm.as_mut_ptr(), &mut classes) });
        (perm, classes)
    }

    /// `plonk::proof::prove` (plonk/src/proof.rs:96-194) in one native call: `wire_evals` are the three padded and
    /// blinded witness COLUMNS (what `CompiledCircuit::prove` builds at :43-49, before `.interpolate()`),
    /// `public_inputs` the padded public-input column (:52-53), `cosets` = `copy_constrains.cosets`.
    /// Panics with "r(zeta) != 0" where the reference panics in `vanishes()` (:321, :361).
    pub fn prove(&self, srs: SrsHandle, circuit: CircuitHandle, wire_evals: [&[Fr]; 3], public_inputs: &[Fr],
                 cosets: [Fr; 3]) -> ffi::TyplonkProof {
        // The columns go over as they are, in host memory (`typlonk_prove_host`, round 6): the library uploads each one right
        // before its interpolation and commitment are queued, so column i + 1 crosses PCIe while column i is transformed,
        // sorted and accumulated -- instead of four uploads (128 MiB at 2^20) before the first kernel starts.
        let n = 1usize << circuit.log_n;
        let flat = |c: &[Fr]| -> Vec<u64> {
            assert_eq!(c.len(), n);
            c.iter().flat_map(|e| fr_limbs(e)).collect()
        };
        let w: Vec<Vec<u64>> = wire_evals.iter().map(|c| flat(c)).collect();
        let wp: [*const u64; 3] = [w[0].as_ptr(), w[1].as_ptr(), w[2].as_ptr()];
        let pi = if public_inputs.iter().all(|x| x.is_zero()) { None } else { Some(flat(public_inputs)) };
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut out = std::mem::MaybeUninit::<ffi::TyplonkProof>::zeroed();
        self.check(unsafe {
            ffi::typlonk_prove_host(self.ctx, srs.id, circuit.id, wp.as_ptr(), pi.as_ref().map_or(ptr::null(), |v| v.as_ptr()),
                                    k.as_ptr(), out.as_mut_ptr())
        });
        unsafe { out.assume_init() }
    }

    /// `prove` for many witnesses of one circuit in one call (`typlonk_prove_batch_host`, batched across proofs in waves):
    /// `wire_evals[k]` and `public_inputs[k]` as for `prove` (`public_inputs` empty = every column zero).  Returns each
    /// proof with its status: `TYPLONK_OK`, or `TYPLONK_ERR_UNSATISFIED` for a witness with r(zeta) != 0 (its proof is
    /// filled all the same and will not verify) -- no panic for those.  Proof k equals `prove` on witness k, bit for bit.
    pub fn prove_batch(&self, srs: SrsHandle, circuit: CircuitHandle, wire_evals: &[[&[Fr]; 3]], public_inputs: &[&[Fr]],
                       cosets: [Fr; 3]) -> Vec<(ffi::TyplonkProof, i32)> {
        assert!(public_inputs.is_empty() || public_inputs.len() == wire_evals.len(), "one public-input column per witness");
        let n = 1usize << circuit.log_n;
        let flat = |c: &[Fr]| -> Vec<u64> {
            assert_eq!(c.len(), n);
            c.iter().flat_map(|e| fr_limbs(e)).collect()
        };
        let w: Vec<Vec<u64>> = wire_evals.iter().flat_map(|cols| cols.iter().map(|c| flat(c))).collect();
        let wp: Vec<*const u64> = w.iter().map(|c| c.as_ptr()).collect();
        let pi: Vec<Option<Vec<u64>>> = public_inputs.iter()
            .map(|c| if c.iter().all(|x| x.is_zero()) { None } else { Some(flat(c)) }).collect();
        let pp: Vec<*const u64> = pi.iter().map(|c| c.as_ref().map_or(ptr::null(), |v| v.as_ptr())).collect();
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let count = wire_evals.len();
        let mut out: Vec<ffi::TyplonkProof> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
        let mut status = vec![0i32; count];
        self.check(unsafe {
            ffi::typlonk_prove_batch_host(self.ctx, srs.id, circuit.id, wp.as_ptr(), if pp.is_empty() { ptr::null() } else { pp.as_ptr() },
                                          count, k.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr())
        });
        out.into_iter().zip(status).collect()
    }

    /// `plonk::proof::verify` (plonk/src/proof.rs:195-281) for a batch of `prove` outputs of one circuit
    /// (`typlonk_verify`): one pairing product for a batch that is all valid, bisected down to the bad proofs otherwise.
    /// `g2s` = [s]G2 as x.c0 x.c1 y.c0 y.c1 limbs; `public_inputs` empty or one column per proof (an empty column = all
    /// zero); `pi_as_prover` subtracts PI(zeta) as the prover adds it (the default is the reference's sign, :497-502).
    /// Returns one verdict per proof.
    pub fn verify_batch(&self, srs: SrsHandle, circuit: CircuitHandle, g2s: &[u64; 24], cosets: [Fr; 3],
                        proofs: &[ffi::TyplonkProof], public_inputs: &[Vec<Fr>], pi_as_prover: bool) -> Vec<bool> {
        assert!(public_inputs.is_empty() || public_inputs.len() == proofs.len(), "one public-input column per proof");
        let cols: Vec<Vec<u64>> = public_inputs.iter().map(|c| c.iter().flat_map(|e| fr_limbs(e)).collect()).collect();
        let pis: Vec<*const u64> = cols.iter().map(|c| if c.is_empty() { ptr::null() } else { c.as_ptr() }).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|c| c.len()).collect();
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut ok = vec![0u8; proofs.len().max(1)];
        self.check(unsafe {
            ffi::typlonk_verify(self.ctx, srs.id, circuit.id, g2s.as_ptr(), k.as_ptr(), proofs.as_ptr(), proofs.len(),
                                if pis.is_empty() { ptr::null() } else { pis.as_ptr() },
                                if lens.is_empty() { ptr::null() } else { lens.as_ptr() },
                                if pi_as_prover { VERIFY_PI_AS_PROVER } else { 0 }, ok.as_mut_ptr())
        });
        ok[..proofs.len()].iter().map(|&b| b != 0).collect()
    }

    // ---- the compact proof shape (include/typlonk.h): batched openings, a transcript that binds the statement ----------
    /// The verifying key of a loaded circuit (`typlonk_circuit_vk`): all `verify_compact` needs, on any backend.
    /// After `set_shard` and `comm_init` this is a COLLECTIVE every rank must call: one fold of 9 records (the ranks' partial
    /// sums of the eight circuit commitments and the P0 record); every rank gets the key one GPU with the whole SRS returns.
    pub fn verifying_key(&self, srs: SrsHandle, circuit: CircuitHandle, cosets: [Fr; 3], g2s: &[u64; 24]) -> ffi::TyplonkVk {
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut vk = std::mem::MaybeUninit::<ffi::TyplonkVk>::zeroed();
        self.check(unsafe { ffi::typlonk_circuit_vk(self.ctx, srs.id, circuit.id, k.as_ptr(), g2s.as_ptr(), vk.as_mut_ptr()) });
        unsafe { vk.assume_init() }
    }

    /// A compact proof (`typlonk_prove_compact_host`): `wire_evals` as for `prove`; `public_inputs` = the statement's public
    /// values themselves (at most n, not padded: their number is part of the statement).  Panics on an unsatisfied witness.
    ///
    /// Multi-GPU: after `set_shard` on `srs` and `comm_init` on this backend the call is a COLLECTIVE that every rank makes
    /// with the same witness -- four folds of 12, 1, 3 and 2 records inside the library ([a] [b] [c] + the rank's eight
    /// partial circuit commitments + its P0 record; [Z]; [t_lo] [t_mid] [t_hi]; W_z, W_zw) -- and every rank returns the
    /// proof one GPU holding the whole SRS returns, byte for byte.  A rank whose call is refused (or whose device fails)
    /// panics with its own error, every peer with `TYPLONK_ERR_COMM` naming that rank, all at the same fold; the
    /// communicator stays usable.  A shard without a communicator is refused (`TYPLONK_ERR_INVALID_ARG`);
    /// `prove_batch_compact`, `prove_batch` and `verify_batch` refuse shards always: a batch of small proofs belongs on one GPU
    /// per proof.
    pub fn prove_compact(&self, srs: SrsHandle, circuit: CircuitHandle, wire_evals: [&[Fr]; 3], public_inputs: &[Fr],
                         cosets: [Fr; 3]) -> ffi::TyplonkProofCompact {
        let rows = wire_evals[0].len();   // the library checks it against the circuit's n
        assert!(wire_evals.iter().all(|c| c.len() == rows), "three columns of equal length");
        let flat = |c: &[Fr]| -> Vec<u64> { c.iter().flat_map(|e| fr_limbs(e)).collect() };
        let w: Vec<Vec<u64>> = wire_evals.iter().map(|c| flat(c)).collect();
        let wp: [*const u64; 3] = [w[0].as_ptr(), w[1].as_ptr(), w[2].as_ptr()];
        let pi = flat(public_inputs);
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut out = std::mem::MaybeUninit::<ffi::TyplonkProofCompact>::zeroed();
        self.check(unsafe {
            ffi::typlonk_prove_compact_host(self.ctx, srs.id, circuit.id, wp.as_ptr(), rows,
                                            if pi.is_empty() { ptr::null() } else { pi.as_ptr() }, public_inputs.len(),
                                            k.as_ptr(), out.as_mut_ptr())
        });
        unsafe { out.assume_init() }
    }

    /// `prove_compact` for many witnesses of one circuit in one call (`typlonk_prove_batch_compact_host`, batched across
    /// proofs in waves): `wire_evals[k]` as for `prove_batch`, `public_inputs` empty or one list of public values per witness.
    /// Returns each proof with its status: `TYPLONK_OK`, or `TYPLONK_ERR_UNSATISFIED` for a witness with r(zeta) != 0 (its
    /// proof is filled all the same and will not verify) -- no panic for those.  Proof k equals `prove_compact` on witness
    /// k and statement k, bit for bit.
    pub fn prove_batch_compact(&self, srs: SrsHandle, circuit: CircuitHandle, wire_evals: &[[&[Fr]; 3]], public_inputs: &[&[Fr]],
                               cosets: [Fr; 3]) -> Vec<(ffi::TyplonkProofCompact, i32)> {
        assert!(public_inputs.is_empty() || public_inputs.len() == wire_evals.len(), "one public-input list per witness");
        let count = wire_evals.len();
        let rows = if count == 0 { 0 } else { wire_evals[0][0].len() };   // the library checks it against the circuit's n
        assert!(wire_evals.iter().all(|cols| cols.iter().all(|c| c.len() == rows)), "columns of equal length");
        let flat = |c: &[Fr]| -> Vec<u64> { c.iter().flat_map(|e| fr_limbs(e)).collect() };
        let w: Vec<Vec<u64>> = wire_evals.iter().flat_map(|cols| cols.iter().map(|c| flat(c))).collect();
        let wp: Vec<*const u64> = w.iter().map(|c| c.as_ptr()).collect();
        let pi: Vec<Vec<u64>> = public_inputs.iter().map(|c| flat(c)).collect();
        let pp: Vec<*const u64> = pi.iter().map(|c| if c.is_empty() { ptr::null() } else { c.as_ptr() }).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|c| c.len()).collect();
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut out: Vec<ffi::TyplonkProofCompact> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
        let mut status = vec![0i32; count];
        self.check(unsafe {
            ffi::typlonk_prove_batch_compact_host(self.ctx, srs.id, circuit.id, wp.as_ptr(), rows,
                                                  if pp.is_empty() { ptr::null() } else { pp.as_ptr() },
                                                  if lens.is_empty() { ptr::null() } else { lens.as_ptr() }, count, k.as_ptr(),
                                                  out.as_mut_ptr(), status.as_mut_ptr())
        });
        out.into_iter().zip(status).collect()
    }

    /// `typlonk_circuit_permutation`: the successor map of the 3n cells (flat index col * n + row) recovered from the
    /// circuit's sigma columns -- `CELL_NONE` where a sigma value is the id of no cell -- and the number of
    /// defects; 0 = sigma is a permutation of the cells.  A lint to run once after `load_circuit`; cached with the circuit.
    pub fn circuit_permutation(&self, circuit: CircuitHandle, cosets: [Fr; 3]) -> (Vec<u32>, u64) {
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut perm = vec![0u32; 3usize << circuit.log_n];
        let mut defects = 0u64;
        self.check(unsafe { ffi::typlonk_circuit_permutation(self.ctx, circuit.id, k.as_ptr(), perm.as_mut_ptr(), &mut defects) });
        (perm, defects)
    }

    /// `typlonk_witness_check_host`: which gate rows and which copy constraints each witness fails -- exact, no SRS, a
    /// fraction of a proof's cost; what to call before a prover on witnesses of unknown quality.  `wire_evals` and
    /// `public_inputs` as for `prove_batch_compact`.  Per witness: the two failure counts (totals), the lowest failing rows
    /// and the lowest failing cells as (x, perm[x]) over flat cells col * n + row, at most `cap` of each.  A witness
    /// satisfies the circuit exactly when both counts are 0.  Panics on a malformed circuit (sigma is no permutation).
    pub fn check_witnesses(&self, circuit: CircuitHandle, wire_evals: &[[&[Fr]; 3]], public_inputs: &[&[Fr]], cosets: [Fr; 3],
                           cap: u32) -> Vec<WitnessReport> {
        assert!(public_inputs.is_empty() || public_inputs.len() == wire_evals.len(), "one public-input list per witness");
        let count = wire_evals.len();
        let rows = if count == 0 { 0 } else { wire_evals[0][0].len() };   // the library checks it against the circuit's n
        assert!(wire_evals.iter().all(|cols| cols.iter().all(|c| c.len() == rows)), "columns of equal length");
        let flat = |c: &[Fr]| -> Vec<u64> { c.iter().flat_map(|e| fr_limbs(e)).collect() };
        let w: Vec<Vec<u64>> = wire_evals.iter().flat_map(|cols| cols.iter().map(|c| flat(c))).collect();
        let wp: Vec<*const u64> = w.iter().map(|c| c.as_ptr()).collect();
        let pi: Vec<Vec<u64>> = public_inputs.iter().map(|c| flat(c)).collect();
        let pp: Vec<*const u64> = pi.iter().map(|c| if c.is_empty() { ptr::null() } else { c.as_ptr() }).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|c| c.len()).collect();
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut reports: Vec<ffi::TyplonkWitnessReport> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
        let cap_n = cap as usize;
        let mut gate = vec![0u32; (count * cap_n).max(1)];
        let mut copy = vec![0u32; (2 * count * cap_n).max(1)];
        self.check(unsafe {
            ffi::typlonk_witness_check_host(self.ctx, circuit.id, wp.as_ptr(), rows,
                                            if pp.is_empty() { ptr::null() } else { pp.as_ptr() },
                                            if lens.is_empty() { ptr::null() } else { lens.as_ptr() }, count, k.as_ptr(), cap,
                                            reports.as_mut_ptr(), gate.as_mut_ptr(), copy.as_mut_ptr())
        });
        reports.iter().enumerate().map(|(i, r)| WitnessReport {
            gate_failures: r.gate_failures,
            copy_failures: r.copy_failures,
            gate_rows: gate[i * cap_n..i * cap_n + r.gate_listed as usize].to_vec(),
            copy_cells: (0..r.copy_listed as usize).map(|j| (copy[2 * (i * cap_n + j)], copy[2 * (i * cap_n + j) + 1])).collect(),
        }).collect()
    }

    /// `typlonk_witness_solve_plan`: what a solve of this circuit costs -- driven rows, free classes, levels (`depth`) and
    /// kernel launches per solve.  Built on first use per (circuit, cosets) and cached with the circuit.  A deep, narrow
    /// circuit (depth close to n) is latency-bound on the device: a caller with a single witness of one reads `depth` here
    /// and may fill it on the CPU instead.
    pub fn solve_info(&self, circuit: CircuitHandle, cosets: [Fr; 3]) -> ffi::TyplonkSolveInfo {
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        let mut info: ffi::TyplonkSolveInfo = unsafe { std::mem::zeroed() };
        self.check(unsafe { ffi::typlonk_witness_solve_plan(self.ctx, circuit.id, k.as_ptr(), &mut info) });
        info
    }

    /// `typlonk_circuit_set_hints`: the advice the solve computes itself -- `TYPLONK_HINT_INV0` (dst = 1 / src, 0 for 0) and
    /// `TYPLONK_HINT_BITS` (a window of at most 64 bits of src's integer).  `dst` names a free class, `src` any cell; both
    /// are flat indices col * n + row.  Replaces the circuit's whole set; an empty slice removes it.  Panics for a refused
    /// set (a hint into a driven class, two into one class, a dependency cycle ...), which leaves the installed one in force.
    pub fn set_hints(&self, circuit: CircuitHandle, hints: &[ffi::TyplonkHint], cosets: [Fr; 3]) {
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        self.check(unsafe {
            ffi::typlonk_circuit_set_hints(self.ctx, circuit.id, k.as_ptr(), if hints.is_empty() { ptr::null() } else { hints.as_ptr() },
                                           hints.len())
        });
    }

    /// `typlonk_witness_solve`: the three wire columns of `values.len()` witnesses from the circuit's inputs, computed on
    /// the device (`C::run(ComputeVar..)` of the reference, builder.rs:381-396).  `cells`: the flat indices col * n + row of
    /// the assigned cells -- the inputs and, if wanted, the three blinding rows -- shared by all witnesses; `values[k]`: their
    /// values for witness k; `public_inputs`: empty, or one list of public values per witness.  Every other free class reads
    /// 0; every driven row's c cell is computed.  The columns stay on the device: `[a, b, c]` per witness, ready for the
    /// check and the provers.  Panics for a cell in a driven class, two cells of one class, or an unsolvable circuit.
    pub fn solve_witnesses(&self, circuit: CircuitHandle, cells: &[u32], values: &[&[Fr]], public_inputs: &[&[Fr]],
                           cosets: [Fr; 3]) -> Vec<[DeviceVec<'_>; 3]> {
        let count = values.len();
        assert!(values.iter().all(|v| v.len() == cells.len()), "one value per assigned cell and witness");
        assert!(public_inputs.is_empty() || public_inputs.len() == count, "one public-input list per witness");
        let n = 1usize << circuit.log_n;
        let vals: Vec<u64> = values.iter().flat_map(|v| v.iter().flat_map(|e| fr_limbs(e))).collect();
        let pis: Vec<DeviceVec<'_>> = public_inputs.iter().map(|p| self.upload(p, p.len().max(1))).collect();
        let pp: Vec<*const ffi::TyplonkBuf> = pis.iter().map(|d| d.buf as *const ffi::TyplonkBuf).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|p| p.len()).collect();
        let out: Vec<[DeviceVec<'_>; 3]> = (0..count).map(|_| [self.upload(&[], n), self.upload(&[], n), self.upload(&[], n)]).collect();
        let wp: Vec<*mut ffi::TyplonkBuf> = out.iter().flat_map(|cols| cols.iter().map(|d| d.buf)).collect();
        let k = [fr_limbs(&cosets[0]), fr_limbs(&cosets[1]), fr_limbs(&cosets[2])];
        self.check(unsafe {
            ffi::typlonk_witness_solve(self.ctx, circuit.id, k.as_ptr(), if cells.is_empty() { ptr::null() } else { cells.as_ptr() },
                                       cells.len(), if vals.is_empty() { ptr::null() } else { vals.as_ptr() },
                                       if pp.is_empty() { ptr::null() } else { pp.as_ptr() },
                                       if lens.is_empty() { ptr::null() } else { lens.as_ptr() }, count, wp.as_ptr())
        });
        out
    }

    /// `typlonk_verify_compact`: a batch of compact proofs against a verifying key; needs no SRS and no circuit on this
    /// backend.  `public_inputs`: empty, or one list of public values per proof.
    pub fn verify_compact(&self, vk: &ffi::TyplonkVk, proofs: &[ffi::TyplonkProofCompact], public_inputs: &[Vec<Fr>]) -> Vec<bool> {
        assert!(public_inputs.is_empty() || public_inputs.len() == proofs.len(), "one public-input list per proof");
        let cols: Vec<Vec<u64>> = public_inputs.iter().map(|c| c.iter().flat_map(|e| fr_limbs(e)).collect()).collect();
        let pis: Vec<*const u64> = cols.iter().map(|c| if c.is_empty() { ptr::null() } else { c.as_ptr() }).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|c| c.len()).collect();
        let mut ok = vec![0u8; proofs.len().max(1)];
        self.check(unsafe {
            ffi::typlonk_verify_compact(self.ctx, vk, proofs.as_ptr(), proofs.len(),
                                        if pis.is_empty() { ptr::null() } else { pis.as_ptr() },
                                        if lens.is_empty() { ptr::null() } else { lens.as_ptr() }, ok.as_mut_ptr())
        });
        ok[..proofs.len()].iter().map(|&b| b != 0).collect()
    }

    // ---- the wire format (include/typlonk.h): compressed points, decoded and subgroup-checked on the device --------------
    /// `typlonk_srs_load_compressed`: a ceremony file's G1 powers, 48 bytes per point.  `Err(i)`: point i (the lowest such)
    /// was rejected and no SRS was created.  Panics on any other failure.
    pub fn upload_srs_compressed(&self, bytes: &[u8], flags: u32, tables: bool) -> Result<SrsHandle, usize> {
        let mut id = 0u32;
        let mut first_bad = usize::MAX;
        let rc = unsafe { ffi::typlonk_srs_load_compressed(self.ctx, bytes.as_ptr(), bytes.len(), flags, &mut id, &mut first_bad) };
        if rc == ffi::TYPLONK_ERR_INVALID_ARG && first_bad != usize::MAX {
            return Err(first_bad);
        }
        self.check(rc);
        let h = SrsHandle { id, len: bytes.len() / ffi::TYPLONK_G1_BYTES };
        if tables {
            self.precompute_tables(h);
        }
        Ok(h)
    }
    /// `typlonk_srs_download_compressed`: the whole SRS as 48 bytes per point, compressed on the device
    pub fn download_srs_compressed(&self, srs: SrsHandle) -> Vec<u8> {
        let mut out = vec![0u8; srs.len * ffi::TYPLONK_G1_BYTES];
        self.check(unsafe { ffi::typlonk_srs_download_compressed(self.ctx, srs.id, 0, srs.len, out.as_mut_ptr()) });
        out
    }
    /// `typlonk_srs_check`: is the SRS `[s^i] G` for the s of `g2s`?  `seed`: 32 bytes that whoever produced the points
    /// cannot have known (draw them after the points are fixed).  An invalid SRS is the report's `verdict`
    /// (`TYPLONK_SRS_*`), not a panic; bad arguments panic like everywhere else.
    pub fn check_srs(&self, srs: SrsHandle, g2s: &[u64; 24], seed: &[u8; 32]) -> ffi::TyplonkSrsReport {
        let mut report: ffi::TyplonkSrsReport = unsafe { std::mem::zeroed() };
        self.check(unsafe { ffi::typlonk_srs_check(self.ctx, srs.id, g2s.as_ptr(), seed.as_ptr(), &mut report) });
        report
    }
    /// `typlonk_srs_contribute`: a new SRS `[t^i] P_i` (no tables) and `[t] g2s`; the old SRS is untouched.  Check the
    /// input before, or the output after: the call itself demands neither.  Unlike the other makers of an `SrsHandle`
    /// this one builds NO fixed-base tables, whatever the old SRS had: call `precompute_tables` on the returned handle
    /// if they are wanted.
    pub fn contribute_srs(&self, srs: SrsHandle, t: &Fr, g2s: &[u64; 24]) -> (SrsHandle, [u64; 24]) {
        let tl = fr_limbs(t);
        let mut id = 0u32;
        let mut out = [0u64; 24];
        self.check(unsafe { ffi::typlonk_srs_contribute(self.ctx, srs.id, tl.as_ptr(), g2s.as_ptr(), &mut id, out.as_mut_ptr()) });
        (SrsHandle { id, len: srs.len }, out)
    }
    /// `typlonk_proof_compact_from_bytes`: `bytes` = count x 656; every point through one kernel launch.  Entry k is the
    /// proof (its challenge fields zero) or why it was refused.
    pub fn proofs_from_bytes(&self, bytes: &[u8], flags: u32) -> Vec<Result<ffi::TyplonkProofCompact, DecodeError>> {
        assert!(bytes.len() % ffi::TYPLONK_PROOF_COMPACT_BYTES == 0, "proofs are 656 bytes each");
        let count = bytes.len() / ffi::TYPLONK_PROOF_COMPACT_BYTES;
        let mut out: Vec<ffi::TyplonkProofCompact> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
        let mut status = vec![0u32; count];
        self.check(unsafe {
            ffi::typlonk_proof_compact_from_bytes(self.ctx, bytes.as_ptr(), count, flags, out.as_mut_ptr(), status.as_mut_ptr())
        });
        out.into_iter().zip(status).map(|(p, st)| match DecodeError::from_status(st) { None => Ok(p), Some(e) => Err(e) }).collect()
    }
    /// `typlonk_verify_compact_bytes`: `verify_compact` over the wire form.  A proof that does not decode is `false` and
    /// never reaches the verifier.
    pub fn verify_compact_bytes(&self, vk: &ffi::TyplonkVk, bytes: &[u8], public_inputs: &[Vec<Fr>], flags: u32) -> Vec<bool> {
        assert!(bytes.len() % ffi::TYPLONK_PROOF_COMPACT_BYTES == 0, "proofs are 656 bytes each");
        let count = bytes.len() / ffi::TYPLONK_PROOF_COMPACT_BYTES;
        assert!(public_inputs.is_empty() || public_inputs.len() == count, "one public-input list per proof");
        let cols: Vec<Vec<u64>> = public_inputs.iter().map(|c| c.iter().flat_map(|e| fr_limbs(e)).collect()).collect();
        let pis: Vec<*const u64> = cols.iter().map(|c| if c.is_empty() { ptr::null() } else { c.as_ptr() }).collect();
        let lens: Vec<usize> = public_inputs.iter().map(|c| c.len()).collect();
        let mut ok = vec![0u8; count.max(1)];
        self.check(unsafe {
            ffi::typlonk_verify_compact_bytes(self.ctx, vk, bytes.as_ptr(), count,
                                              if pis.is_empty() { ptr::null() } else { pis.as_ptr() },
                                              if lens.is_empty() { ptr::null() } else { lens.as_ptr() }, flags, ok.as_mut_ptr())
        });
        ok[..count].iter().map(|&b| b != 0).collect()
    }

    // ---- multi-GPU: one process per GPU, RCCL inside the library --------------------------------------------------
    /// this process holds bases [first, first + len) of a `total`-point SRS
    pub fn set_shard(&self, srs: SrsHandle, first: usize, total: usize) {
        self.check(unsafe { ffi::typlonk_srs_set_shard(self.ctx, srs.id, first, total) });
    }
    /// rank 0: the 128-byte rendezvous id, to be handed to the other ranks by any channel the host program has
    pub fn comm_unique_id() -> [u8; ffi::TYPLONK_COMM_ID_BYTES] {
        let mut id = [0u8; ffi::TYPLONK_COMM_ID_BYTES];
        let rc = unsafe { ffi::typlonk_comm_unique_id(id.as_mut_ptr()) };
        if rc != ffi::TYPLONK_OK {
            panic!("typlonk_comm_unique_id: {}", strerror(rc));
        }
        id
    }
    /// every rank (collective).  Call `typlonk_comm_available()` on every rank first and agree on the answer.
    pub fn comm_init(&self, id: &[u8; ffi::TYPLONK_COMM_ID_BYTES], rank: i32, world: i32) {
        self.check(unsafe { ffi::typlonk_comm_init(self.ctx, id.as_ptr(), rank, world) });
    }
    /// `evaluate_in_s` over the whole node: every rank passes the device address of coefficient 0 of the full vector
    /// and gets the FULL sum (local partial MSM + one all-gather + fold in rank order)
    pub fn msm_sharded(&self, srs: SrsHandle, v: &DeviceVec, m: usize) -> G1Point {
        let (mut xy, mut inf) = ([0u64; 12], 0u8);
        let p = unsafe { ffi::typlonk_buf_devptr(v.buf) };
        self.check(unsafe { ffi::typlonk_msm_g1_sharded_devptr(self.ctx, srs.id, p, m, xy.as_mut_ptr(), &mut inf) });
        g1_from_abi(&xy, inf)
    }
}

/// `typlonk_proof` -> the pieces of the reference's `Proof` (plonk/src/proof.rs:65-95)
/// One witness's report from `Backend::check_witnesses`.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct WitnessReport {
    pub gate_failures: u64,
    pub copy_failures: u64,
    pub gate_rows: Vec<u32>,
    pub copy_cells: Vec<(u32, u32)>,
}

impl WitnessReport {
    pub fn satisfied(&self) -> bool { self.gate_failures == 0 && self.copy_failures == 0 }
}

pub struct ProofParts {
    pub commitments: [G1Point; 3],          // [a], [b], [c]
    pub z_commitment: G1Point,               // permutation.commitment
    pub t: [G1Point; 3],                     // quotient slices
    pub witnesses: [G1Point; 6],             // a, b, c at zeta; Z at zeta; Z at zeta*w; r at zeta
    pub evals: [Fr; 6],                      // a(zeta) b(zeta) c(zeta) Z(zeta) Z(zeta w) r(zeta)
    pub evaluation_point: Fr,
}
impl From<&ffi::TyplonkProof> for ProofParts {
    fn from(p: &ffi::TyplonkProof) -> Self {
        let g = |xy: &[u64; 12], inf: u8| g1_from_abi(xy, inf);
        ProofParts {
            commitments: [0, 1, 2].map(|i| g(&p.commit_xy[i], p.commit_inf[i])),
            z_commitment: g(&p.z_xy, p.z_inf),
            t: [0, 1, 2].map(|i| g(&p.tail.t_xy[i], p.tail.t_inf[i])),
            witnesses: [0, 1, 2, 3, 4, 5].map(|i| g(&p.tail.w_xy[i], p.tail.w_inf[i])),
            evals: [0, 1, 2, 3, 4, 5].map(|i| fr_from_limbs(p.tail.evals[i])),
            evaluation_point: fr_from_limbs(p.zeta),
        }
    }
}

/// An SRS resident on the shared context of its thread, freed when dropped: what the patched `kzg::srs::Srs` holds.
/// (`Backend::shared` keeps ONE context per thread and device alive for the thread's lifetime, so the device memory of
/// an `Srs` must be returned when the `Srs` goes -- not when the context does.)
#[derive(Debug)]
pub struct OwnedSrs {
    backend: std::rc::Rc<Backend>,
    handle: SrsHandle,
}
impl OwnedSrs {
    pub fn new(backend: std::rc::Rc<Backend>, handle: SrsHandle) -> Self {
        OwnedSrs { backend, handle }
    }
    pub fn backend(&self) -> &Backend {
        &self.backend
    }
    pub fn backend_rc(&self) -> std::rc::Rc<Backend> {
        self.backend.clone()
    }
    pub fn handle(&self) -> SrsHandle {
        self.handle
    }
    /// `typlonk_srs_g1_ntt`, TO_LAGRANGE: the Lagrange form `[L_i(s)] G`, i < 2^log_n, of this monomial SRS as an SRS of its own
    /// (no tables): the MSM of a column of evaluations over it is the commitment to the column's polynomial.  Check the
    /// monomial SRS first (`Backend::check_srs` tests that form only).
    pub fn lagrange(&self, log_n: u32) -> OwnedSrs {
        let mut id = 0u32;
        self.backend.check(unsafe {
            ffi::typlonk_srs_g1_ntt(self.backend.ctx, self.handle.id, log_n, ffi::TYPLONK_SRS_TO_LAGRANGE as u32, &mut id)
        });
        OwnedSrs { backend: self.backend.clone(), handle: SrsHandle { id, len: 1usize << log_n } }
    }
    /// `typlonk_srs_open_all_table`: the table `open_all` needs for the domain of 2^log_n points over this monomial SRS -- 2^(log_n + 1)
    /// records held like an SRS (freed when dropped) that are no SRS to commit over.
    pub fn open_all_table(&self, log_n: u32) -> OwnedSrs {
        let mut id = 0u32;
        self.backend.check(unsafe { ffi::typlonk_srs_open_all_table(self.backend.ctx, self.handle.id, log_n, &mut id) });
        OwnedSrs { backend: self.backend.clone(), handle: SrsHandle { id, len: 2usize << log_n } }
    }
    /// `typlonk_open_all_host` over `self`, a table made by `open_all_table`: the openings of `coeffs` (1..=n coefficients, 4
    /// Montgomery limbs each) at every point w^k of the table's domain, k < n = len / 2, in natural order -- (12 limbs x || y,
    /// identity flag) per proof and the 4 limbs of f(w^k).  What `KzgScheme::open` gives at each w^k, in one call.
    pub fn open_all(&self, coeffs: &[[u64; 4]]) -> (Vec<[u64; 12]>, Vec<u8>, Vec<[u64; 4]>) {
        let n = self.handle.len / 2;
        let mut xy = vec![[0u64; 12]; n];
        let mut inf = vec![0u8; n];
        let mut evals = vec![[0u64; 4]; n];
        self.backend.check(unsafe {
            ffi::typlonk_open_all_host(self.backend.ctx, self.handle.id, coeffs.as_ptr() as *const u64, coeffs.len(),
                                       xy.as_mut_ptr() as *mut u64, inf.as_mut_ptr(), evals.as_mut_ptr() as *mut u64)
        });
        (xy, inf, evals)
    }
    /// `typlonk_srs_open_chunks_table`: the table `open_chunks` needs for the domain of 2^log_n points cut into cosets of 2^log_l
    /// over this monomial SRS -- 2^(log_n + 1) records held like an SRS (freed when dropped).  log_l = 0 is `open_all_table`.
    pub fn open_chunks_table(&self, log_n: u32, log_l: u32) -> OwnedSrs {
        let mut id = 0u32;
        self.backend.check(unsafe { ffi::typlonk_srs_open_chunks_table(self.backend.ctx, self.handle.id, log_n, log_l, &mut id) });
        OwnedSrs { backend: self.backend.clone(), handle: SrsHandle { id, len: 2usize << log_n } }
    }
    /// `typlonk_open_chunks_host` over `self`, a table made by `open_chunks_table` with this `log_l`: for each polynomial (all of one
    /// length, 1..=n coefficients of 4 Montgomery limbs) the r = n >> log_l multi-proofs, proof k of polynomial p at p r + k, and the
    /// n evaluations chunk-major: evals[p n + k l + t] = f_p(w^(k + r t)).  (The buffers are sized for the table's domain, not for
    /// log_l, so a log_l other than the table's mis-sizes the result and nothing else.)
    pub fn open_chunks(&self, log_l: u32, polys: &[&[[u64; 4]]]) -> (Vec<[u64; 12]>, Vec<u8>, Vec<[u64; 4]>) {
        let n = self.handle.len / 2;
        let count = polys.len();
        let m = polys.first().map_or(0, |p| p.len());
        assert!(polys.iter().all(|p| p.len() == m), "open_chunks: the polynomials of one call have one length");
        let ptrs: Vec<*const u64> = polys.iter().map(|p| p.as_ptr() as *const u64).collect();
        let mut xy = vec![[0u64; 12]; count * n];
        let mut inf = vec![0u8; count * n];
        let mut evals = vec![[0u64; 4]; count * n];
        self.backend.check(unsafe {
            ffi::typlonk_open_chunks_host(self.backend.ctx, self.handle.id, ptrs.as_ptr(), m, count,
                                          xy.as_mut_ptr() as *mut u64, inf.as_mut_ptr(), evals.as_mut_ptr() as *mut u64)
        });
        xy.truncate(count * (n >> log_l));
        inf.truncate(count * (n >> log_l));
        (xy, inf, evals)
    }
}
impl Drop for OwnedSrs {
    fn drop(&mut self) {
        unsafe { ffi::typlonk_srs_free(self.backend.ctx, self.handle.id) }; // (no panic in drop: the status is ignored)
    }
}
/// The per-circuit device constants (`typlonk_circuit_load`), freed when dropped: what the patched `CompiledCircuit` holds.
#[derive(Debug)]
pub struct OwnedCircuit {
    backend: std::rc::Rc<Backend>,
    handle: CircuitHandle,
}
impl OwnedCircuit {
    pub fn new(backend: std::rc::Rc<Backend>, handle: CircuitHandle) -> Self {
        OwnedCircuit { backend, handle }
    }
    /// `Backend::compile_circuit`, owned: from selector evaluations and the permutation (`None`: the identity)
    pub fn compile(backend: std::rc::Rc<Backend>, selector_evals: [&[Fr]; 5], perm: Option<&[u32]>, cosets: [Fr; 3], log_n: u32) -> Self {
        let handle = backend.compile_circuit(selector_evals, perm, cosets, log_n);
        OwnedCircuit { backend, handle }
    }
    pub fn handle(&self) -> CircuitHandle {
        self.handle
    }
}
impl Drop for OwnedCircuit {
    fn drop(&mut self) {
        unsafe { ffi::typlonk_circuit_free(self.backend.ctx, self.handle.id) };
    }
}

impl Drop for Backend {
    fn drop(&mut self) {
        unsafe { ffi::typlonk_destroy(self.ctx) }
    }
}
impl Drop for DeviceVec<'_> {
    fn drop(&mut self) {
        unsafe { ffi::typlonk_buf_free(self.backend.ctx, self.buf) };
    }
}

fn strerror(rc: c_int) -> String {
    unsafe { CStr::from_ptr(ffi::typlonk_strerror(rc)) }.to_string_lossy().into_owned()
}
