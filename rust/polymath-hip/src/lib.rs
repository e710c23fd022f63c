//! Safe wrapper over `polymath-hip-sys` for arkworks types.
//!
//! What crosses the FFI is what arkworks already holds in memory (include/polymath_hip.h, "Data conventions"):
//! `Fp<MontBackend<_, N>, N>` = N little-endian u64 Montgomery limbs; `Affine<P>` = `x, y, infinity: bool`.  Rust does not
//! promise that layout, so it is CHECKED, once per curve and process, against values whose limbs are known
//! ([`layout_check`]): a compiler or arkworks version that lays the types out differently makes every entry point return
//! [`Status::LayoutMismatch`] instead of feeding the GPU garbage.  Inputs are passed by pointer (no copy of a 2^20-element
//! witness), outputs (three points and one scalar per proof) are rebuilt with `Fp::new_unchecked` / `Affine::new_unchecked`.
//!
//! All entry points are generic over `E: Pairing` and dispatch on `TypeId`: the reference's `Polymath<E, T>` is generic
//! (src/lib.rs:44-50) and has no curve-specific trait to hang a GPU backend on; [`supports`] tells whether `E` has one.
//!
//! NEVER COMPILED IN THE BUILD IMAGE (no cargo there) -- `rust/check.sh` is the first thing to run on a machine with one.
use core::any::{Any, TypeId};
use core::ffi::c_void;
use std::collections::HashMap;
use std::ffi::CStr;
use std::sync::{Arc, Mutex, OnceLock};

use ark_ec::pairing::Pairing;
use ark_ff::BigInt;
use polymath_hip_sys as sys;

// ------------------------------------------------------------------------------------------ status
/// `pm_status`, plus the two conditions only this wrapper can detect.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Status {
    InvalidArg,
    /// `assert!(scalars.len() <= g1_elems.len())`, prover.rs:381
    LenMismatch,
    /// `D::new(..)` is `None` / `SynthesisError::PolynomialDegreeTooLarge`, prover.rs:83,317
    DomainTooLarge,
    /// `assert!(rem_poly.is_zero())`, prover.rs:108,221
    RemainderNonzero,
    /// the degree asserts, prover.rs:107,113,222
    DegreeBound,
    Hip,
    NoDevice,
    State,
    Comm,
    /// `E` is not a curve the library implements
    UnsupportedCurve,
    /// this build of arkworks does not lay `Fp` / `Affine` out as the header's conventions assume
    LayoutMismatch,
    Unknown(i32),
}

impl Status {
    fn from_raw(rc: i32) -> Status {
        match rc {
            sys::PM_ERR_INVALID_ARG => Status::InvalidArg,
            sys::PM_ERR_LEN_MISMATCH => Status::LenMismatch,
            sys::PM_ERR_DOMAIN_TOO_LARGE => Status::DomainTooLarge,
            sys::PM_ERR_REMAINDER_NONZERO => Status::RemainderNonzero,
            sys::PM_ERR_DEGREE_BOUND => Status::DegreeBound,
            sys::PM_ERR_HIP => Status::Hip,
            sys::PM_ERR_NO_DEVICE => Status::NoDevice,
            sys::PM_ERR_STATE => Status::State,
            sys::PM_ERR_COMM => Status::Comm,
            other => Status::Unknown(other),
        }
    }
}

#[derive(Clone, Debug)]
pub struct HipError {
    pub status: Status,
    pub message: String,
}

impl core::fmt::Display for HipError {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        write!(f, "libpolymath_hip: {:?}: {}", self.status, self.message)
    }
}
impl std::error::Error for HipError {}

fn err(status: Status, message: &str) -> HipError {
    HipError { status, message: message.to_string() }
}

// ------------------------------------------------------------------------------------------ curves
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Curve {
    Bls12_381,
    Bn254,
}

impl Curve {
    fn id(self) -> i32 {
        match self {
            Curve::Bls12_381 => sys::PM_BLS12_381,
            Curve::Bn254 => sys::PM_BN254,
        }
    }
    /// u64 limbs of a base-field element
    fn fq_limbs(self) -> usize {
        match self {
            Curve::Bls12_381 => 6,
            Curve::Bn254 => 4,
        }
    }
}

/// The library's curve for a pairing engine, by `TypeId` (`Pairing: 'static`).
pub fn curve_of<E: Pairing>() -> Option<Curve> {
    let t = TypeId::of::<E>();
    if t == TypeId::of::<ark_bls12_381::Bls12_381>() {
        return Some(Curve::Bls12_381);
    }
    #[cfg(feature = "bn254")]
    if t == TypeId::of::<ark_bn254::Bn254>() {
        return Some(Curve::Bn254);
    }
    None
}

/// `true` when proofs over `E` can run on the GPU in this process: a known curve, the expected memory layout, a device.
pub fn supports<E: Pairing>() -> bool {
    match curve_of::<E>() {
        Some(c) => layout_check(c) && device_count() > 0,
        None => false,
    }
}

pub fn device_count() -> i32 {
    // SAFETY: no arguments, no preconditions.
    unsafe { sys::pm_device_count() }
}

/// A value of type `A` as a value of type `B` when the two are the same type (safe: `Any` downcast of an `Option`).
fn same_type<A: 'static, B: 'static>(a: A) -> Option<B> {
    let mut slot = Some(a);
    (&mut slot as &mut dyn Any).downcast_mut::<Option<B>>().and_then(Option::take)
}

/// Does this build lay the curve's `Fr` and `G1Affine` out as `x || y || infinity` of Montgomery limbs?  Checked on the
/// generator, on the identity and on `Fr::from(7)`, whose limbs are read through the public fields.  Cached.
pub fn layout_check(curve: Curve) -> bool {
    static BLS: OnceLock<bool> = OnceLock::new();
    #[cfg(feature = "bn254")]
    static BN: OnceLock<bool> = OnceLock::new();
    match curve {
        Curve::Bls12_381 => *BLS.get_or_init(|| {
            use ark_bls12_381::{Fr, G1Affine};
            use ark_ec::AffineRepr;
            let seven = Fr::from(7u64);
            let g = G1Affine::generator();
            let id = G1Affine::identity();
            core::mem::size_of::<Fr>() == 32
                && core::mem::size_of::<G1Affine>() == 104
                && raw_words(&seven, 4) == (seven.0).0.to_vec()
                && raw_words(&g, 6) == (g.x.0).0.to_vec()
                && raw_words(&g, 12)[6..] == (g.y.0).0[..]
                && raw_byte(&g, 96) == 0
                && raw_byte(&id, 96) == 1
        }),
        #[cfg(feature = "bn254")]
        Curve::Bn254 => *BN.get_or_init(|| {
            use ark_bn254::{Fr, G1Affine};
            use ark_ec::AffineRepr;
            let seven = Fr::from(7u64);
            let g = G1Affine::generator();
            let id = G1Affine::identity();
            core::mem::size_of::<Fr>() == 32
                && core::mem::size_of::<G1Affine>() == 72
                && raw_words(&seven, 4) == (seven.0).0.to_vec()
                && raw_words(&g, 4) == (g.x.0).0.to_vec()
                && raw_words(&g, 8)[4..] == (g.y.0).0[..]
                && raw_byte(&g, 64) == 0
                && raw_byte(&id, 64) == 1
        }),
        #[cfg(not(feature = "bn254"))]
        Curve::Bn254 => false,
    }
}

fn raw_words<T>(v: &T, n: usize) -> Vec<u64> {
    assert!(core::mem::size_of::<T>() >= 8 * n && core::mem::align_of::<T>() >= 8);
    // SAFETY: `v` is a live, 8-aligned value of at least 8 n bytes made of plain integers (checked above for size and
    // alignment; the types passed in are Fp / Affine, which hold arrays of u64 and one bool).
    unsafe { core::slice::from_raw_parts(v as *const T as *const u64, n) }.to_vec()
}

fn raw_byte<T>(v: &T, at: usize) -> u8 {
    assert!(core::mem::size_of::<T>() > at);
    // SAFETY: inside the value; the byte read is the `infinity: bool` (0 or 1) or a limb byte, never padding, when the layout
    // is the expected one -- and when it is not, the comparison fails on some other line first or reads an initialised limb byte.
    unsafe { *(v as *const T as *const u8).add(at) }
}

fn curve_checked<E: Pairing>() -> Result<Curve, HipError> {
    let c = curve_of::<E>().ok_or_else(|| err(Status::UnsupportedCurve, "no GPU implementation of this pairing engine"))?;
    if !layout_check(c) {
        return Err(err(Status::LayoutMismatch, "arkworks types are not laid out as x || y || infinity of Montgomery limbs in this build"));
    }
    Ok(c)
}

fn fr_ptr<F>(s: &[F]) -> *const u64 {
    s.as_ptr() as *const u64
}

/// The quotient marker of `PM_ASSIGNMENT_SOLVE` (`PM_UNKNOWN_QUOTIENT_WORDS`): four limbs that are no field element on either curve
/// and say "unknown, and the Euclidean quotient of its division row" (`q * b = a - rem`: circom's `q <-- a \ b`, arkworks' DIV /
/// REM).  The `Option` rows of [`GpuKey::prove_batch_from_partial`] and [`GpuKey::solve`] write the plain marker for `None`; a caller
/// whose circuit has division rows passes limb rows with this constant on the quotients to the `-sys` calls.  The marker is
/// explicit: with `None` on a quotient the row is refused, as it always was.
pub const UNKNOWN_QUOTIENT: [u64; 4] = sys::PM_UNKNOWN_QUOTIENT_WORDS;

/// The indicator marker of `PM_ASSIGNMENT_SOLVE` (`PM_HINT_INDICATOR_WORDS`): four limbs that are no field element on either curve
/// and say "unknown, and the indicator of its guard row" (`out * (inp - i) = 0`: circomlib's `Decoder` / `Multiplexer`,
/// `out[i] <-- (inp == i) ? 1 : 0`).  The value is 1 where the guard's known side is zero and 0 elsewhere.  The marker is explicit:
/// with `None` on such a column the row is an ordinary dividing row, which is stuck where `inp == i`, as it always was.
pub const HINT_INDICATOR: [u64; 4] = sys::PM_HINT_INDICATOR_WORDS;

/// The square-root marker of `PM_ASSIGNMENT_SOLVE` (`PM_HINT_SQRT_MARKER`): four limbs that are no field element on either curve and
/// say "unknown, and the smaller square root of its square-root row" (`u * u = c`: circom's `x <-- sqrt(c); x*x === c`, arkworks'
/// `sqrt` witness in point decompression).  The value is the root whose canonical integer is `<= (r - 1) / 2`; a non-residue leaves
/// that assignment stuck at the row.  The marker is explicit: with `None` on such a column the row is refused, as it always was.  A
/// caller who wants the larger root supplies the value itself.
pub const HINT_SQRT: [u64; 4] = sys::PM_HINT_SQRT_MARKER;

/// Montgomery limbs of a partial assignment appended to `out`: a value's own four words, or the unknown marker (four times
/// `u64::MAX`: not a field element on either curve) for `None`.
fn partial_limbs<F>(vals: &[Option<F>], out: &mut Vec<u64>) {
    for v in vals {
        match v {
            // SAFETY: a scalar is four u64 limbs (`curve_checked` has verified the layout before any caller gets here).
            Some(f) => out.extend_from_slice(unsafe { core::slice::from_raw_parts(fr_ptr(core::slice::from_ref(f)), 4) }),
            None => out.extend_from_slice(&[u64::MAX; 4]),
        }
    }
}

fn fr_from_raw<E: Pairing>(curve: Curve, limbs: [u64; 4]) -> E::ScalarField {
    match curve {
        Curve::Bls12_381 => same_type(ark_bls12_381::Fr::new_unchecked(BigInt::new(limbs))),
        #[cfg(feature = "bn254")]
        Curve::Bn254 => same_type(ark_bn254::Fr::new_unchecked(BigInt::new(limbs))),
        #[cfg(not(feature = "bn254"))]
        Curve::Bn254 => None,
    }
    .expect("curve_of::<E>() named this curve")
}

fn g1_from_raw<E: Pairing>(curve: Curve, xy: &[u64; 12], inf: i32) -> E::G1Affine {
    match curve {
        Curve::Bls12_381 => {
            use ark_bls12_381::{Fq, G1Affine};
            let p = if inf != 0 {
                G1Affine::identity()
            } else {
                let mut x = [0u64; 6];
                let mut y = [0u64; 6];
                x.copy_from_slice(&xy[..6]);
                y.copy_from_slice(&xy[6..12]);
                G1Affine::new_unchecked(Fq::new_unchecked(BigInt::new(x)), Fq::new_unchecked(BigInt::new(y)))
            };
            same_type(p)
        },
        #[cfg(feature = "bn254")]
        Curve::Bn254 => {
            use ark_bn254::{Fq, G1Affine};
            let p = if inf != 0 {
                G1Affine::identity()
            } else {
                let mut x = [0u64; 4];
                let mut y = [0u64; 4];
                x.copy_from_slice(&xy[..4]);
                y.copy_from_slice(&xy[4..8]);
                G1Affine::new_unchecked(Fq::new_unchecked(BigInt::new(x)), Fq::new_unchecked(BigInt::new(y)))
            };
            same_type(p)
        },
        #[cfg(not(feature = "bn254"))]
        Curve::Bn254 => None,
    }
    .expect("curve_of::<E>() named this curve")
}

// ------------------------------------------------------------------------------------------ context
/// `pm_option` (include/polymath_hip.h): what a host may choose, per context; the reference keeps no global state either.
#[derive(Clone, Copy, Debug)]
#[repr(i32)]
pub enum PmOption {
    MsmOverlap = 0,
    NttOverlap = 1,
    Tables = 2,
    MsmMaxPieceLog = 3,
    MaxSegLog = 4,
    InflightContexts = 5,
    MsmTaskLen = 6,
    TableWindowBits = 7,
}

/// One `pm_ctx`: a HIP stream and the per-proof state; one proof in flight per context, one context per thread.
pub struct Context {
    raw: *mut sys::pm_ctx,
    device: i32,
}

/// `pm_verify_verdict`: what [`Context::verify_batch`] says about one proof.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Verdict {
    Rejected,
    Accepted,
    /// the bytes `pm_host_verify` refuses: a point that does not decode into the group, `a_at_x1 >= r`
    Malformed,
}

impl Verdict {
    fn from_raw(v: u8) -> Verdict {
        match v {
            sys::PM_VERIFY_ACCEPTED => Verdict::Accepted,
            sys::PM_VERIFY_MALFORMED => Verdict::Malformed,
            _ => Verdict::Rejected,
        }
    }
}

// SAFETY: a pm_ctx may be driven from any ONE thread at a time (the header's threading rule); `&mut self` on every call
// that touches it enforces that.
unsafe impl Send for Context {}

impl Context {
    pub fn new(device: i32) -> Result<Context, HipError> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: `raw` is a valid out-pointer.
        let rc = unsafe { sys::pm_ctx_create(device, &mut raw) };
        if rc != sys::PM_OK || raw.is_null() {
            return Err(err(Status::from_raw(rc), "pm_ctx_create failed"));
        }
        Ok(Context { raw, device })
    }

    pub fn device(&self) -> i32 {
        self.device
    }

    pub fn raw(&mut self) -> *mut sys::pm_ctx {
        self.raw
    }

    pub fn set_option(&mut self, option: PmOption, value: i64) -> Result<(), HipError> {
        // SAFETY: live context.
        let rc = unsafe { sys::pm_ctx_set_option(self.raw, option as i32, value as core::ffi::c_longlong) };
        self.check(rc)
    }

    pub fn last_error(&self) -> String {
        // SAFETY: live context; the library returns a NUL-terminated string it owns until the context's next call.
        unsafe { CStr::from_ptr(sys::pm_last_error(self.raw)) }.to_string_lossy().into_owned()
    }

    fn check(&self, rc: i32) -> Result<(), HipError> {
        if rc == sys::PM_OK {
            Ok(())
        } else {
            Err(HipError { status: Status::from_raw(rc), message: self.last_error() })
        }
    }

    /// Many proofs against one verifying key (`pm_verify_batch`): the per-proof curve work on the GPU, a handful of pairing
    /// checks on the host.  `public_inputs`: `proofs.len() / proof_len` x `n_inputs` `Fr` as Montgomery limbs, WITHOUT the leading
    /// one; `proofs`: packed `Proof::serialize_compressed` records; `transcript`: a `sys::PM_TRANSCRIPT_*` id; `seed`: mixed
    /// into the weights' key (the weights are bound to the batch either way).  Returns one verdict per proof and the number of
    /// pairing checks made.
    pub fn verify_batch(&mut self, curve: Curve, transcript: i32, vk_bytes: &[u8], public_inputs: &[u64], n_inputs: usize, proofs: &[u8],
                        seed: Option<&[u8; 32]>) -> Result<(Vec<Verdict>, usize), HipError> {
        let proof_len = match curve {
            Curve::Bls12_381 => 176,
            Curve::Bn254 => 128,
        };
        if proofs.len() % proof_len != 0 || public_inputs.len() != proofs.len() / proof_len * n_inputs * sys::PM_FR_LIMBS {
            return Err(err(Status::InvalidArg, "verify_batch: proofs / public_inputs do not have the batch's shape"));
        }
        let count = proofs.len() / proof_len;
        let mut raw = vec![0u8; count];
        let (mut all, mut checks) = (0i32, 0usize);
        // SAFETY: live context; every pointer covers the length passed with it, `raw` holds `count` bytes, the seed is 32 bytes or null.
        let rc = unsafe {
            sys::pm_verify_batch(self.raw, curve.id(), transcript, vk_bytes.as_ptr(), vk_bytes.len(), public_inputs.as_ptr(), n_inputs, proofs.as_ptr(),
                                 proof_len, count, seed.map_or(core::ptr::null(), |s| s.as_ptr()), raw.as_mut_ptr(), &mut all, &mut checks)
        };
        self.check(rc)?;
        Ok((raw.into_iter().map(Verdict::from_raw).collect(), checks))
    }

    /// [`Context::verify_batch`] with the pairing checks on the GPU (`pm_verify_batch2`, `PM_VERIFY_PAIRING_DEVICE`): the root in a launch
    /// of one lane and, if it fails, every well-formed proof's own check in ONE more launch -- no bisection.  Same verdicts; the
    /// number of checks is then 1 + the number of proofs that are not [`Verdict::Malformed`].
    pub fn verify_batch_device_pairing(&mut self, curve: Curve, transcript: i32, vk_bytes: &[u8], public_inputs: &[u64], n_inputs: usize,
                                       proofs: &[u8], seed: Option<&[u8; 32]>) -> Result<(Vec<Verdict>, usize), HipError> {
        self.verify_batch_with(curve, transcript, vk_bytes, public_inputs, n_inputs, proofs, seed, sys::PM_VERIFY_PAIRING_DEVICE,
                               sys::PM_VERIFY_CHALLENGES_HOST)
    }

    /// [`Context::verify_batch_device_pairing`] with every check spread over a group of 36 lanes of one wave (`pm_verify_batch2`,
    /// `PM_VERIFY_PAIRING_DEVICE_WAVE`): the root always, the leaves after a failing root while at most 1024 proofs are live.  Same
    /// verdicts and the same number of checks, byte for byte.
    pub fn verify_batch_wave_pairing(&mut self, curve: Curve, transcript: i32, vk_bytes: &[u8], public_inputs: &[u64], n_inputs: usize,
                                     proofs: &[u8], seed: Option<&[u8; 32]>) -> Result<(Vec<Verdict>, usize), HipError> {
        self.verify_batch_with(curve, transcript, vk_bytes, public_inputs, n_inputs, proofs, seed, sys::PM_VERIFY_PAIRING_DEVICE_WAVE,
                               sys::PM_VERIFY_CHALLENGES_HOST)
    }

    /// [`Context::verify_batch`] with both modes chosen (`pm_verify_batch2`): `pairing` a `sys::PM_VERIFY_PAIRING_*`, `challenges` a
    /// `sys::PM_VERIFY_CHALLENGES_*` value, OR-ed into the call's `pairing` argument.  With `PM_VERIFY_CHALLENGES_DEVICE` the per-proof Fiat-Shamir challenges and scalar glue
    /// run on the GPU too, one lane per proof; the challenges are the same bits, so verdicts and the number of checks do not change.
    #[allow(clippy::too_many_arguments)]
    pub fn verify_batch_with(&mut self, curve: Curve, transcript: i32, vk_bytes: &[u8], public_inputs: &[u64], n_inputs: usize, proofs: &[u8],
                             seed: Option<&[u8; 32]>, pairing: i32, challenges: i32) -> Result<(Vec<Verdict>, usize), HipError> {
        let proof_len = match curve {
            Curve::Bls12_381 => 176,
            Curve::Bn254 => 128,
        };
        if proofs.len() % proof_len != 0 || public_inputs.len() != proofs.len() / proof_len * n_inputs * sys::PM_FR_LIMBS {
            return Err(err(Status::InvalidArg, "verify_batch: proofs / public_inputs do not have the batch's shape"));
        }
        let count = proofs.len() / proof_len;
        let mut raw = vec![0u8; count];
        let (mut all, mut checks) = (0i32, 0usize);
        // SAFETY: live context; every pointer covers the length passed with it, `raw` holds `count` bytes, the seed is 32 bytes or null.
        let rc = unsafe {
            sys::pm_verify_batch2(self.raw, curve.id(), transcript, vk_bytes.as_ptr(), vk_bytes.len(), public_inputs.as_ptr(), n_inputs, proofs.as_ptr(),
                                  proof_len, count, seed.map_or(core::ptr::null(), |s| s.as_ptr()), pairing | challenges, raw.as_mut_ptr(), &mut all,
                                  &mut checks)
        };
        self.check(rc)?;
        Ok((raw.into_iter().map(Verdict::from_raw).collect(), checks))
    }

    /// What the lanes of the last [`Context::verify_batch_with`] call with `PM_VERIFY_CHALLENGES_DEVICE` derived (`pm_prove_tap(8)`):
    /// per proof `x1`, `x2`, `c(x1)` as Montgomery limbs and whether `a_at_x1` was canonical (if not, the three are zero).
    #[allow(clippy::type_complexity)]
    pub fn last_verifier_challenges(&mut self, count: usize) -> Result<Vec<([u64; 4], [u64; 4], [u64; 4], bool)>, HipError> {
        let mut raw = vec![0u64; 16 * count];
        let mut n = 0usize;
        // SAFETY: live context; `raw` holds 4 * count elements of 4 limbs.
        let rc = unsafe { sys::pm_prove_tap(self.raw, 8, raw.as_mut_ptr(), 4 * count, &mut n) };
        self.check(rc)?;
        if n != 4 * count {
            return Err(err(Status::InvalidArg, "last_verifier_challenges: the last batch had another count"));
        }
        let limbs = |i: usize| [raw[i], raw[i + 1], raw[i + 2], raw[i + 3]];
        Ok((0..count).map(|r| (limbs(16 * r), limbs(16 * r + 4), limbs(16 * r + 8), raw[16 * r + 12] != 0)).collect())
    }

    /// `pm_pairing_check_batch`: `g1.len() / (k * 2 * fq_limbs)` checks `prod_j e(g1[i][j], g2[j]) == 1` against `k <= 4` fixed G2
    /// points, one GPU lane each.  `g2`: `k` x (`x.c0 || x.c1 || y.c0 || y.c1`), `g1`: checks x `k` x (`x || y`), Montgomery limbs;
    /// an all-zero G1 point is the point at infinity and contributes 1.
    pub fn pairing_check_batch(&mut self, curve: Curve, g2: &[u64], g1: &[u64]) -> Result<Vec<bool>, HipError> {
        let fq = curve.fq_limbs();
        let k = g2.len() / (4 * fq);
        if k == 0 || g2.len() != k * 4 * fq || g1.len() % (k * 2 * fq) != 0 {
            return Err(err(Status::InvalidArg, "pairing_check_batch: g2 / g1 do not have the checks' shape"));
        }
        let count = g1.len() / (k * 2 * fq);
        let mut raw = vec![0u8; count];
        // SAFETY: live context; `g2` holds k points, `g1` count * k points 16 * fq bytes apart, `raw` count bytes.
        let rc = unsafe {
            sys::pm_pairing_check_batch(self.raw, curve.id(), g2.as_ptr(), k, g1.as_ptr() as *const c_void, 16 * fq, count, raw.as_mut_ptr())
        };
        self.check(rc)?;
        Ok(raw.into_iter().map(|b| b != 0).collect())
    }

    /// Run `f` on this thread's context (created on first use on `device`).
    pub fn with_thread_local<T>(device: i32, f: impl FnOnce(&mut Context) -> Result<T, HipError>) -> Result<T, HipError> {
        use std::cell::RefCell;
        thread_local! { static CTX: RefCell<Option<Context>> = const { RefCell::new(None) }; }
        CTX.with(|slot| {
            let mut slot = slot.borrow_mut();
            if slot.as_ref().map(|c| c.device) != Some(device) {
                *slot = Some(Context::new(device)?);
            }
            f(slot.as_mut().expect("just filled"))
        })
    }

    /// Phase 1 (prover.rs:75-123): witness map, inverse transforms, u^2, h, then `[a]_1` and `[c]_1`.
    /// `instance` INCLUDES the leading one (prover.rs:56); `r_a` = the two `F::rand` draws of prover.rs:110, constant term first.
    ///
    /// The C context keeps a pointer to the key between the phases (`pm_prove_phase3` reads the key's bases), so the phases
    /// that follow live on the returned [`ProofInFlight`], which borrows BOTH the context and the key: safe code cannot drop
    /// the key, start another proof on the context, or free the context while a proof is between its phases.
    pub fn prove_phase1<'c, 'k, E: Pairing>(
        &'c mut self,
        key: &'k GpuKey,
        instance: &[E::ScalarField],
        witness: &[E::ScalarField],
        r_a: &[E::ScalarField; 2],
    ) -> Result<(ProofInFlight<'c, 'k>, E::G1Affine, E::G1Affine), HipError> {
        let curve = curve_checked::<E>()?;
        if curve != key.curve || instance.len() as u64 != key.m0 || witness.len() as u64 != key.mw {
            return Err(err(Status::InvalidArg, "assignment does not fit the key"));
        }
        let (mut a, mut c) = ([0u64; 12], [0u64; 12]);
        let (mut a_inf, mut c_inf) = (0i32, 0i32);
        // SAFETY: the slices hold m0 / mw / 2 field elements of 4 limbs each (layout checked); the outputs have room for
        // 2 * fq_limbs <= 12 words.
        let rc = unsafe {
            sys::pm_prove_phase1(self.raw, key.raw, fr_ptr(instance), fr_ptr(witness), fr_ptr(&r_a[..]), a.as_mut_ptr(), &mut a_inf, c.as_mut_ptr(), &mut c_inf)
        };
        self.check(rc)?;
        let (a_g1, c_g1) = (g1_from_raw::<E>(curve, &a, a_inf), g1_from_raw::<E>(curve, &c, c_inf));
        Ok((ProofInFlight { ctx: self, _key: key, curve }, a_g1, c_g1))
    }

    /// `E::G1::msm_unchecked(bases, scalars)` (prover.rs:380-384) on host slices, zipped to the shorter length like arkworks.
    pub fn msm_g1<E: Pairing>(&mut self, bases: &[E::G1Affine], scalars: &[E::ScalarField]) -> Result<E::G1Affine, HipError> {
        let curve = curve_checked::<E>()?;
        let len = bases.len().min(scalars.len());
        let mut out = [0u64; 12];
        let mut inf = 0i32;
        // SAFETY: `len` points of size_of::<G1Affine>() bytes each and `len` scalars (layout checked).
        let rc = unsafe {
            sys::pm_msm_g1(self.raw, curve.id(), bases.as_ptr() as *const c_void, core::mem::size_of::<E::G1Affine>(), fr_ptr(scalars), len, out.as_mut_ptr(), &mut inf)
        };
        self.check(rc)?;
        Ok(g1_from_raw::<E>(curve, &out, inf))
    }

    /// `Radix2EvaluationDomain::{fft, ifft}_in_place` (prover.rs:241,319,325): natural order in and out, 1/n on the inverse.
    pub fn ntt_in_place<E: Pairing>(&mut self, data: &mut [E::ScalarField], inverse: bool) -> Result<(), HipError> {
        let curve = curve_checked::<E>()?;
        if !data.len().is_power_of_two() {
            return Err(err(Status::InvalidArg, "length is not a power of two"));
        }
        // SAFETY: 2^log_n field elements, read and written in place.
        let rc = unsafe { sys::pm_ntt(self.raw, curve.id(), data.as_mut_ptr() as *mut u64, data.len().trailing_zeros(), inverse as i32) };
        self.check(rc)
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        // SAFETY: created by pm_ctx_create, destroyed once.
        unsafe { sys::pm_ctx_destroy(self.raw) }
    }
}

/// A proof between its phases: phase 1 has run on `ctx` against `key`; phases 2 and 3 are methods of this guard and nothing
/// else can touch the context or drop the key until it is gone (the library's `pm_ctx` holds a raw pointer to the `pm_pk`).
pub struct ProofInFlight<'c, 'k> {
    ctx: &'c mut Context,
    _key: &'k GpuKey,
    curve: Curve,
}

impl ProofInFlight<'_, '_> {
    /// Phase 2 (prover.rs:132): `u_poly.evaluate(&x1)`; the caller adds `r_a(x1) * y1^alpha`.
    pub fn prove_phase2<E: Pairing>(&mut self, x1: &E::ScalarField) -> Result<E::ScalarField, HipError> {
        if curve_checked::<E>()? != self.curve {
            return Err(err(Status::InvalidArg, "phase 2 called with another pairing engine than phase 1"));
        }
        let mut out = [0u64; 4];
        // SAFETY: one field element in, one out; the key of phase 1 is still alive (borrowed by `self`).
        let rc = unsafe { sys::pm_prove_phase2(self.ctx.raw, fr_ptr(core::slice::from_ref(x1)), out.as_mut_ptr()) };
        self.ctx.check(rc)?;
        Ok(fr_from_raw::<E>(self.curve, out))
    }

    /// Phase 3 (prover.rs:142-229): the Y^-gamma-scaled numerator, its division by (X - x1), `[d]_1`.  Consumes the guard.
    pub fn prove_phase3<E: Pairing>(
        self,
        x1: &E::ScalarField,
        x2: &E::ScalarField,
        a_at_x1: &E::ScalarField,
        c_at_x1: &E::ScalarField,
    ) -> Result<E::G1Affine, HipError> {
        if curve_checked::<E>()? != self.curve {
            return Err(err(Status::InvalidArg, "phase 3 called with another pairing engine than phase 1"));
        }
        let mut d = [0u64; 12];
        let mut d_inf = 0i32;
        let one = |v: &E::ScalarField| fr_ptr(core::slice::from_ref(v));
        // SAFETY: four field elements in, 2 * fq_limbs <= 12 words out; the key of phase 1 is still alive (borrowed by `self`).
        let rc = unsafe { sys::pm_prove_phase3(self.ctx.raw, one(x1), one(x2), one(a_at_x1), one(c_at_x1), d.as_mut_ptr(), &mut d_inf) };
        self.ctx.check(rc)?;
        Ok(g1_from_raw::<E>(self.curve, &d, d_inf))
    }
}

// ------------------------------------------------------------------------------------------ proving key
/// The fields of the reference's `ProvingKey<E>` (data_structures.rs:56-73) the GPU needs, borrowed.  The wrapper cannot
/// name that type (the reference depends on this crate, not the other way round).
pub struct KeyParts<'a, E: Pairing> {
    pub n: u64,
    pub sigma: u64,
    /// `SAPMatrices` (common.rs:113-127): num_instance_variables, num_r1cs_witness_variables, num_r1cs_constraints, a, b, c
    pub m0: u64,
    pub mw: u64,
    pub nr: u64,
    pub a: &'a [Vec<(E::ScalarField, usize)>],
    pub b: &'a [Vec<(E::ScalarField, usize)>],
    pub c: &'a [Vec<(E::ScalarField, usize)>],
    pub x_powers_g1: &'a [E::G1Affine],
    pub x_powers_y_alpha_g1: &'a [E::G1Affine],
    pub x_powers_y_gamma_g1: &'a [E::G1Affine],
    pub x_powers_y_gamma_z_g1: &'a [E::G1Affine],
    pub x_powers_zh_by_y_alpha_g1: &'a [E::G1Affine],
    pub uj_wj_lcs_by_y_alpha_g1: &'a [E::G1Affine],
}

/// `pm_base_vec` (include/polymath_hip.h): the six base vectors of `ProvingKey<E>` (data_structures.rs:56-73), in the order
/// of `pm_pk_load`'s array and of `pm_pk_info`'s lengths.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum BaseVec {
    XPowers = 0,
    XPowersYAlpha = 1,
    XPowersYGamma = 2,
    XPowersYGammaZ = 3,
    XPowersZhByYAlpha = 4,
    UjWjLcsByYAlpha = 5,
}

impl BaseVec {
    pub const ALL: [BaseVec; 6] =
        [BaseVec::XPowers, BaseVec::XPowersYAlpha, BaseVec::XPowersYGamma, BaseVec::XPowersYGammaZ, BaseVec::XPowersZhByYAlpha, BaseVec::UjWjLcsByYAlpha];
}

/// What `generate_proving_key` has in hand after synthesis (generator.rs:46-54): the R1CS matrices of `cs.to_matrices()`
/// and their shape.  `m0` counts the leading one (`num_instance_variables`).
pub struct R1csParts<'a, E: Pairing> {
    pub m0: u64,
    pub mw: u64,
    pub nr: u64,
    pub a: &'a [Vec<(E::ScalarField, usize)>],
    pub b: &'a [Vec<(E::ScalarField, usize)>],
    pub c: &'a [Vec<(E::ScalarField, usize)>],
}

/// `pm_pk_info`: the scalars of the verifying key (data_structures.rs:38-52) a resident key was made for, and the lengths of
/// its six base vectors ([`BaseVec`] order).
pub struct KeyInfo<E: Pairing> {
    pub n: u64,
    pub m0: u64,
    pub sigma: u64,
    /// `domain.group_gen()` (generator.rs:156)
    pub omega: E::ScalarField,
    pub base_lens: [u64; 6],
}

/// The six `Vec<E::G1Affine>` of `ProvingKey<E>` (data_structures.rs:60-72), copied back from the device.
pub struct ExportedBases<E: Pairing> {
    pub x_powers_g1: Vec<E::G1Affine>,
    pub x_powers_y_alpha_g1: Vec<E::G1Affine>,
    pub x_powers_y_gamma_g1: Vec<E::G1Affine>,
    pub x_powers_y_gamma_z_g1: Vec<E::G1Affine>,
    pub x_powers_zh_by_y_alpha_g1: Vec<E::G1Affine>,
    pub uj_wj_lcs_by_y_alpha_g1: Vec<E::G1Affine>,
}

struct Csr<F> {
    rowptr: Vec<u64>,
    col: Vec<u32>,
    val: Vec<F>,
}

fn flatten<F: Copy>(rows: &[Vec<(F, usize)>]) -> Result<Csr<F>, HipError> {
    let nnz: usize = rows.iter().map(Vec::len).sum();
    let mut m = Csr { rowptr: Vec::with_capacity(rows.len() + 1), col: Vec::with_capacity(nnz), val: Vec::with_capacity(nnz) };
    m.rowptr.push(0);
    for row in rows {
        for &(v, j) in row {
            m.col.push(u32::try_from(j).map_err(|_| err(Status::InvalidArg, "column index above 2^32"))?);
            m.val.push(v);
        }
        m.rowptr.push(m.col.len() as u64);
    }
    Ok(m)
}

impl<F> Csr<F> {
    fn raw(&self) -> sys::pm_csr {
        sys::pm_csr { nrows: (self.rowptr.len() - 1) as u64, rowptr: self.rowptr.as_ptr(), col: self.col.as_ptr(), val: fr_ptr(self.val.as_slice()) }
    }
}

/// The divisor of a long division or the modulus of a modular division in a [`Hint`]: CSR columns, or literal limbs of four words.
pub enum HintLimbs<'a> {
    Columns(&'a [u64]),
    Literal(&'a [[u64; 4]]),
}

/// One record of the declaration that [`GpuKey::set_hints`] takes, as the header states it.  Columns are CSR columns (0: the
/// constant one, then the instance, then the witness); limbs have `n` bits.
pub enum Hint<'a> {
    /// `PM_HINT_LONGDIV`: `q` and `rem` are the limbs of `floor(D / E)` and `D mod E`.
    LongDiv { n: u64, q: &'a [u64], rem: &'a [u64], dividend: &'a [u64], divisor: HintLimbs<'a> },
    /// `PM_HINT_LONGDIV_WIDE`: the same record under the wide limits (a dividend below 2^8192, a divisor below 2^4096: RSA-2048).
    LongDivWide { n: u64, q: &'a [u64], rem: &'a [u64], dividend: &'a [u64], divisor: HintLimbs<'a> },
    /// `PM_HINT_MODDIV`: `z` are the limbs of the `Z` in `[0, P)` with `Z (D+ - D-) = N+ - N- (mod P)`; both numerator lists empty
    /// mean `N = 1`, the modular inverse.
    ModDiv { n: u64, z: &'a [u64], n_plus: &'a [u64], n_minus: &'a [u64], d_plus: &'a [u64], d_minus: &'a [u64], modulus: HintLimbs<'a> },
}

impl Hint<'_> {
    /// The words of a declaration: the records of `hints` one after the other (what [`GpuKey::set_hints`] takes as `desc`).
    pub fn encode(hints: &[Hint]) -> Vec<u64> {
        let mut words = Vec::new();
        for hint in hints {
            let (lists, last): (Vec<&[u64]>, &HintLimbs) = match hint {
                Hint::LongDiv { n, q, rem, dividend, divisor } => {
                    words.extend_from_slice(&[sys::PM_HINT_LONGDIV, *n, q.len() as u64, rem.len() as u64, dividend.len() as u64]);
                    (vec![*q, *rem, *dividend], divisor)
                }
                Hint::LongDivWide { n, q, rem, dividend, divisor } => {
                    words.extend_from_slice(&[sys::PM_HINT_LONGDIV_WIDE, *n, q.len() as u64, rem.len() as u64, dividend.len() as u64]);
                    (vec![*q, *rem, *dividend], divisor)
                }
                Hint::ModDiv { n, z, n_plus, n_minus, d_plus, d_minus, modulus } => {
                    words.extend_from_slice(&[sys::PM_HINT_MODDIV, *n, z.len() as u64, n_plus.len() as u64, n_minus.len() as u64, d_plus.len() as u64,
                                              d_minus.len() as u64]);
                    (vec![*z, *n_plus, *n_minus, *d_plus, *d_minus], modulus)
                }
            };
            // PM_HINT_DIVISOR_LITERAL and PM_HINT_MODULUS_LITERAL are the same bit of the record's last head word
            match last {
                HintLimbs::Columns(cols) => {
                    words.extend_from_slice(&[cols.len() as u64, 0]);
                    lists.iter().for_each(|l| words.extend_from_slice(l));
                    words.extend_from_slice(cols);
                }
                HintLimbs::Literal(limbs) => {
                    words.extend_from_slice(&[limbs.len() as u64, sys::PM_HINT_MODULUS_LITERAL]);
                    lists.iter().for_each(|l| words.extend_from_slice(l));
                    limbs.iter().for_each(|l| words.extend_from_slice(l));
                }
            }
        }
        words
    }
}

/// A proving key resident in HBM (`pm_pk`): bases in the internal radix, window tables, CSR matrices.  Immutable after
/// creation; contexts on the same device may share it.
pub struct GpuKey {
    raw: *mut sys::pm_pk,
    curve: Curve,
    m0: u64,
    mw: u64,
}

// SAFETY: pm_pk is immutable after creation and may be shared by contexts on the same device (header, "Threading").
unsafe impl Send for GpuKey {}
unsafe impl Sync for GpuKey {}

impl GpuKey {
    /// `pm_pk_load`: upload an existing key.  The library copies everything it needs; nothing is borrowed after the call.
    pub fn upload<E: Pairing>(ctx: &mut Context, k: &KeyParts<'_, E>) -> Result<GpuKey, HipError> {
        let curve = curve_checked::<E>()?;
        let (a, b, c) = (flatten(k.a)?, flatten(k.b)?, flatten(k.c)?);
        let stride = core::mem::size_of::<E::G1Affine>();
        let arr = |s: &[E::G1Affine]| sys::pm_base_array { points: s.as_ptr() as *const c_void, len: s.len(), stride };
        // pm_base_vec order
        let bases = [
            arr(k.x_powers_g1),
            arr(k.x_powers_y_alpha_g1),
            arr(k.x_powers_y_gamma_g1),
            arr(k.x_powers_y_gamma_z_g1),
            arr(k.x_powers_zh_by_y_alpha_g1),
            arr(k.uj_wj_lcs_by_y_alpha_g1),
        ];
        let mut raw = core::ptr::null_mut();
        // SAFETY: the CSR vectors and base slices outlive the call; strides and lengths are the slices' own.
        let rc = unsafe {
            sys::pm_pk_load(ctx.raw, curve.id(), k.n, k.m0, k.mw, k.nr, k.sigma, &a.raw(), &b.raw(), &c.raw(), bases.as_ptr(), 0, 1, &mut raw)
        };
        ctx.check(rc)?;
        Ok(GpuKey { raw, curve, m0: k.m0, mw: k.mw })
    }

    /// `pm_pk_load_bytes`: a key file's bytes (`ProvingKey::serialize_compressed`, e.g. an mmap) straight to the device; the
    /// points are decoded there, with `validate` as ark's `Validate::Yes`.  A refused key names its first bad point in the error.
    pub fn load_bytes<E: Pairing>(ctx: &mut Context, bytes: &[u8], validate: bool) -> Result<GpuKey, HipError> {
        Self::load_bytes_form::<E>(ctx, bytes, validate, WireForm::Compressed)
    }

    /// [`GpuKey::load_bytes`] for either record form: [`WireForm::Uncompressed`] takes `ProvingKey::serialize_uncompressed` bytes
    /// (96 / 64-byte G1 records, vk prefix 728 / 504 bytes).  The curve equation is checked in every mode; `validate` adds the
    /// subgroup check.  Bytes of the other form are refused as a malformed key: the form is never guessed.
    pub fn load_bytes_form<E: Pairing>(ctx: &mut Context, bytes: &[u8], validate: bool, form: WireForm) -> Result<GpuKey, HipError> {
        Self::load_bytes_flags::<E>(ctx, bytes, validate as i32, form)
    }

    /// [`GpuKey::load_bytes_form`] with `PM_KEY_CHECK_RELATIONS`: besides validating every point, the loader decides whether the
    /// bytes are a proving key at all -- what `generate_proving_key` would have produced for some `(x, z)` under the key's own vk and
    /// SAP matrices -- before it builds the window tables.  A key that is not (vectors of another circuit, an `[x]_2` of another
    /// ceremony, one record overwritten by another valid point) is refused like a key with a bad point, the error naming the first
    /// failing relation, e.g. `uj_wj_lcs_by_y_alpha_g1: does not match the SAP matrices`.  Unsharded keys only.
    pub fn load_bytes_checked<E: Pairing>(ctx: &mut Context, bytes: &[u8], form: WireForm) -> Result<GpuKey, HipError> {
        Self::load_bytes_flags::<E>(ctx, bytes, 1 | sys::PM_KEY_CHECK_RELATIONS, form)
    }

    // `validate`: the flag word without the form bit (0, 1, or 1 | PM_KEY_CHECK_RELATIONS)
    fn load_bytes_flags<E: Pairing>(ctx: &mut Context, bytes: &[u8], validate: i32, form: WireForm) -> Result<GpuKey, HipError> {
        let curve = curve_checked::<E>()?;
        let vk_len = match (curve.id() == sys::PM_BLS12_381, form) {
            (true, WireForm::Compressed) => 392,
            (true, WireForm::Uncompressed) => 728,
            (false, WireForm::Compressed) => 280,
            (false, WireForm::Uncompressed) => 504,
        };
        let header = |k: usize| bytes.get(vk_len + 8 * k..vk_len + 8 * k + 8).map(|b| u64::from_le_bytes(b.try_into().unwrap()));
        let (m0, mw) = match (header(0), header(1)) {
            (Some(m0), Some(mw)) => (m0, mw),
            _ => return Err(err(Status::InvalidArg, "truncated key")),
        };
        let mut raw = core::ptr::null_mut();
        let rc = Self::load_bytes_raw(ctx, curve, bytes.as_ptr(), bytes.len(), validate as i32 | form as i32, &mut raw);
        ctx.check(rc)?;
        Ok(GpuKey { raw, curve, m0, mw })
    }

    // THE call of pm_pk_load_bytes, for an unsharded key: the loaders above (`raw` null on entry, the new key on success) and
    // `set_hints` (`flags` = PM_KEY_HINTS, `raw` the existing key, which stays).  `bytes` may be null where `len` is 0.
    fn load_bytes_raw(ctx: &mut Context, curve: Curve, bytes: *const u8, len: usize, flags: i32, raw: &mut *mut sys::pm_pk) -> i32 {
        // SAFETY: the caller's `bytes` hold `len` bytes, outlive the call and are only read; the library keeps no pointer to them.
        unsafe { sys::pm_pk_load_bytes(ctx.raw, curve.id(), bytes, len, flags, 0, 1, sys::PM_SHARD_PAIRS, raw) }
    }

    /// `pm_pk_load_sharded`: this rank's share of a key for ONE proof over `shard_count` GPUs (one process per GPU).  `layout`:
    /// [`ShardLayout::Vector`] shards witness map, transforms, scans and MSM pairs (the context must have been joined to its
    /// rank's [`Comm`] first); [`ShardLayout::Pairs`] shards the MSM pair ranges only and the phases return PARTIAL points
    /// (sum them with [`Comm::combine_points`]).  Every rank then runs exactly the three phases of a single-GPU proof.
    pub fn upload_sharded<E: Pairing>(ctx: &mut Context, k: &KeyParts<'_, E>, shard_rank: i32, shard_count: i32, layout: ShardLayout) -> Result<GpuKey, HipError> {
        let curve = curve_checked::<E>()?;
        let (a, b, c) = (flatten(k.a)?, flatten(k.b)?, flatten(k.c)?);
        let stride = core::mem::size_of::<E::G1Affine>();
        let arr = |s: &[E::G1Affine]| sys::pm_base_array { points: s.as_ptr() as *const c_void, len: s.len(), stride };
        let bases = [
            arr(k.x_powers_g1),
            arr(k.x_powers_y_alpha_g1),
            arr(k.x_powers_y_gamma_g1),
            arr(k.x_powers_y_gamma_z_g1),
            arr(k.x_powers_zh_by_y_alpha_g1),
            arr(k.uj_wj_lcs_by_y_alpha_g1),
        ];
        let mut raw = core::ptr::null_mut();
        // SAFETY: as in `upload`; a collective only in the sense that every rank must make the same call for its own share.
        let rc = unsafe {
            sys::pm_pk_load_sharded(ctx.raw, curve.id(), k.n, k.m0, k.mw, k.nr, k.sigma, &a.raw(), &b.raw(), &c.raw(), bases.as_ptr(), shard_rank, shard_count,
                                    layout as i32, &mut raw)
        };
        ctx.check(rc)?;
        Ok(GpuKey { raw, curve, m0: k.m0, mw: k.mw })
    }

    /// `pm_pk_generate` == `generate_proving_key` (generator.rs:24-167) from the point where it holds the matrices and the two
    /// trapdoor draws: `x` then `z`, both `domain.sample_element_outside_domain(rng)` (generator.rs:72,77) -- the RNG stays with
    /// the caller.  The dense, serial `uj_wj_lcs` loop (generator.rs:112-136: n * (m - m0) calls of `SAPMatrices::u / w`) is
    /// replaced by an O(nnz) pass and the ~14 n scalar multiplications of `Self::generate` (generator.rs:169-177) by a
    /// fixed-base batch on the device; the base vectors are born resident, so the first `prove` uploads nothing.
    /// The library derives `n` and `sigma = n + 3` itself (`SAPMatrices::size`, common.rs:130-134); read them with [`GpuKey::info`].
    pub fn generate<E: Pairing>(ctx: &mut Context, r1cs: &R1csParts<'_, E>, x: &E::ScalarField, z: &E::ScalarField) -> Result<GpuKey, HipError> {
        let curve = curve_checked::<E>()?;
        if r1cs.a.len() as u64 != r1cs.nr || r1cs.b.len() as u64 != r1cs.nr || r1cs.c.len() as u64 != r1cs.nr {
            return Err(err(Status::InvalidArg, "matrices do not have num_constraints rows"));
        }
        let (a, b, c) = (flatten(r1cs.a)?, flatten(r1cs.b)?, flatten(r1cs.c)?);
        let one = |v: &E::ScalarField| fr_ptr(core::slice::from_ref(v));
        let mut raw = core::ptr::null_mut();
        // SAFETY: the CSR vectors outlive the call; `x` and `z` are one field element (4 limbs, layout checked) each.
        let rc = unsafe { sys::pm_pk_generate(ctx.raw, curve.id(), r1cs.m0, r1cs.mw, r1cs.nr, &a.raw(), &b.raw(), &c.raw(), one(x), one(z), 0, 1, &mut raw) };
        ctx.check(rc)?;
        Ok(GpuKey { raw, curve, m0: r1cs.m0, mw: r1cs.mw })
    }

    /// `pm_host_prove_batch`: `rows.len()` runs of `create_proof_with_assignment` against this (unsharded) key in one call, the
    /// library's own transcript (`transcript`: `sys::PM_TRANSCRIPT_*`) included.  Row i = (instance with the leading one, witness,
    /// r_a).  Returns, per row, `Ok(Proof::serialize_compressed bytes)` or the status `pm_host_prove` gives that row (an unsatisfied
    /// assignment: `RemainderNonzero` / `DegreeBound`); a failing row leaves its neighbours alone.  The outer error is the call's.
    pub fn prove_batch<E: Pairing>(
        &self,
        ctx: &mut Context,
        transcript: i32,
        rows: &[(&[E::ScalarField], &[E::ScalarField], [E::ScalarField; 2])],
    ) -> Result<Vec<Result<Vec<u8>, Status>>, HipError> {
        self.prove_batch_with_glue::<E>(ctx, transcript, sys::PM_PROVE_GLUE_HOST, rows)
    }

    /// [`GpuKey::prove_batch`] with `PM_PROVE_GLUE_DEVICE`: the Fiat-Shamir glue between the phases of a group of proofs runs in
    /// kernels with one lane per proof, and a group costs one copy to the host and one stream synchronisation.  Statuses and bytes
    /// are those of `prove_batch`, bit for bit.
    pub fn prove_batch_device_glue<E: Pairing>(
        &self,
        ctx: &mut Context,
        transcript: i32,
        rows: &[(&[E::ScalarField], &[E::ScalarField], [E::ScalarField; 2])],
    ) -> Result<Vec<Result<Vec<u8>, Status>>, HipError> {
        self.prove_batch_with_glue::<E>(ctx, transcript, sys::PM_PROVE_GLUE_DEVICE, rows)
    }

    /// `glue`: a `sys::PM_PROVE_GLUE_*` value, OR-ed into the call's `transcript` argument.
    pub fn prove_batch_with_glue<E: Pairing>(
        &self,
        ctx: &mut Context,
        transcript: i32,
        glue: i32,
        rows: &[(&[E::ScalarField], &[E::ScalarField], [E::ScalarField; 2])],
    ) -> Result<Vec<Result<Vec<u8>, Status>>, HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "key of another curve"));
        }
        let (mut x, mut w, mut ra) = (Vec::new(), Vec::new(), Vec::new());
        for (xi, wi, ri) in rows {
            if xi.len() as u64 != self.m0 || wi.len() as u64 != self.mw {
                return Err(err(Status::LenMismatch, "a row's instance / witness length is not the key's"));
            }
            x.extend_from_slice(xi);
            w.extend_from_slice(wi);
            ra.extend_from_slice(ri);
        }
        let proof_len = 3 * 8 * curve.fq_limbs() + 32;
        let mut bytes = vec![0u8; proof_len * rows.len()];
        let mut status = vec![0i32; rows.len()];
        let w_ptr = if w.is_empty() { core::ptr::null() } else { fr_ptr(&w) };
        // SAFETY: live key and context; x / w / ra hold rows.len() records of m0 / mw / 2 elements (layout checked), `bytes` and
        // `status` have room for rows.len() records.
        let rc = unsafe {
            sys::pm_host_prove_batch(ctx.raw, self.raw, transcript | glue, rows.len(), fr_ptr(&x), fr_ptr(&x), w_ptr, 0, fr_ptr(&ra), bytes.as_mut_ptr(),
                                     proof_len, status.as_mut_ptr())
        };
        ctx.check(rc)?;
        Ok(status
            .iter()
            .zip(bytes.chunks_exact(proof_len))
            .map(|(&s, b)| if s == sys::PM_OK { Ok(b.to_vec()) } else { Err(Status::from_raw(s)) })
            .collect())
    }

    /// `pm_host_prove_batch` with `PM_ASSIGNMENT_SOLVE`: the rows are PARTIAL assignments -- `None` where the library is to compute
    /// the value on the GPU, by forward propagation through the key's constraint rows (bit decompositions included: the bits of
    /// `Boolean::new_witness` variables that one row sums to a known value are computed from it) -- and every row must leave the same
    /// entries open.  Row i = (instance with the leading one, witness, r_a).  Returns, per row, the proof bytes together with the
    /// completed instance (what the verifier needs; `pm_prove_tap(9)`), or the row's status: `InvalidArg` for an assignment that
    /// got stuck on a division by zero or on a value that does not fit its bits, otherwise what [`GpuKey::prove_batch`] gives it.  The outer error is the call's: an
    /// unsolvable structure is `InvalidArg` with the row or column in the message, and nothing has been computed.
    ///
    /// The is-zero pair -- the two rows of every equality test (`FpVar::is_neq`: `(a - b) * mult = neq`, `(a - b) * (1 - neq) = 0`;
    /// circom's `IsZero` alike) with both the multiplier and the flag left `None` -- is completed as one step.  Where the tested
    /// value is zero the multiplier is free and the library writes m = 0; arkworks' own witness generation writes 1 there, and a
    /// caller that needs that value gives the multiplier as `Some(..)` and leaves only the flag open.
    ///
    /// The rows need not come in dependency order: a system whose pass in matrix order is refused is planned by a waiting-row
    /// scheduler (a row waits until the rows that compute its inputs have acted), so an R1CS assembled from parts, booleanity rows
    /// emitted after the recomposition or a row-sorted matrix file complete as well.  An assignment that gets stuck under such a plan
    /// reports the ROOT CAUSE: the stuck row of lowest dependency level, then smallest index.  A pair's opener must still come
    /// before its closer; a system that no order solves keeps the matrix-order error text.
    #[allow(clippy::type_complexity)]
    pub fn prove_batch_from_partial<E: Pairing>(
        &self,
        ctx: &mut Context,
        transcript: i32,
        rows: &[(&[Option<E::ScalarField>], &[Option<E::ScalarField>], [E::ScalarField; 2])],
    ) -> Result<Vec<Result<(Vec<u8>, Vec<E::ScalarField>), Status>>, HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "key of another curve"));
        }
        let (mut x, mut w, mut ra) = (Vec::new(), Vec::new(), Vec::new());
        for (xi, wi, ri) in rows {
            if xi.len() as u64 != self.m0 || wi.len() as u64 != self.mw {
                return Err(err(Status::LenMismatch, "a row's instance / witness length is not the key's"));
            }
            partial_limbs(xi, &mut x);
            partial_limbs(wi, &mut w);
            ra.extend_from_slice(ri);
        }
        let proof_len = 3 * 8 * curve.fq_limbs() + 32;
        let mut bytes = vec![0u8; proof_len * rows.len()];
        let mut status = vec![0i32; rows.len()];
        let w_ptr = if w.is_empty() { core::ptr::null() } else { w.as_ptr() };
        // SAFETY: live key and context; x / w hold rows.len() records of m0 / mw elements of 4 limbs, ra rows.len() records of 2
        // elements (layout checked), `bytes` and `status` have room for rows.len() records.  The arrays are only read.
        let rc = unsafe {
            sys::pm_host_prove_batch(ctx.raw, self.raw, transcript, rows.len(), x.as_ptr(), x.as_ptr(), w_ptr, sys::PM_ASSIGNMENT_SOLVE, fr_ptr(&ra),
                                     bytes.as_mut_ptr(), proof_len, status.as_mut_ptr())
        };
        ctx.check(rc)?;
        let solved = if rows.is_empty() { Vec::new() } else { self.solve_results::<E>(ctx, rows.len())? };
        Ok(status
            .iter()
            .zip(bytes.chunks_exact(proof_len))
            .zip(solved)
            .map(|((&s, b), (_, inst))| if s == sys::PM_OK { Ok((b.to_vec(), inst)) } else { Err(Status::from_raw(s)) })
            .collect())
    }

    /// `pm_r1cs_check_batch` with `PM_ASSIGNMENT_SOLVE` and no rows asked for: complete partial assignments (`None` = to be computed)
    /// without proving.  Returns, per assignment, its stuck row (`Some(row)`: a division by zero there, or a bit decomposition of a
    /// value of 2^k or more; the instance is then all zero) and the completed instance, leading one included.  An is-zero pair never
    /// sticks: with the tested value zero its multiplier is stored as m = 0 (see [`GpuKey::prove_batch_from_partial`]).
    #[allow(clippy::type_complexity)]
    pub fn solve<E: Pairing>(
        &self,
        ctx: &mut Context,
        rows: &[(&[Option<E::ScalarField>], &[Option<E::ScalarField>])],
    ) -> Result<Vec<(Option<u64>, Vec<E::ScalarField>)>, HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "key of another curve"));
        }
        if rows.is_empty() {
            return Ok(Vec::new());
        }
        let (mut x, mut w) = (Vec::new(), Vec::new());
        for (xi, wi) in rows {
            if xi.len() as u64 != self.m0 || wi.len() as u64 != self.mw {
                return Err(err(Status::LenMismatch, "a row's instance / witness length is not the key's"));
            }
            partial_limbs(xi, &mut x);
            partial_limbs(wi, &mut w);
        }
        let mut n_bad = vec![0u64; rows.len()];
        let w_ptr = if w.is_empty() { core::ptr::null() } else { w.as_ptr() };
        // SAFETY: live key and context; x / w hold rows.len() records of m0 / mw elements of 4 limbs; no rows, no residuals.
        let rc = unsafe {
            sys::pm_r1cs_check_batch(ctx.raw, self.raw, rows.len(), x.as_ptr(), w_ptr, sys::PM_ASSIGNMENT_SOLVE, 0, n_bad.as_mut_ptr(), core::ptr::null_mut(),
                                     core::ptr::null_mut())
        };
        ctx.check(rc)?;
        self.solve_results::<E>(ctx, rows.len())
    }

    /// `pm_prove_tap(9)`: stuck row and completed instance of each of the `count` assignments of the last solving call on `ctx`.
    #[allow(clippy::type_complexity)]
    fn solve_results<E: Pairing>(&self, ctx: &mut Context, count: usize) -> Result<Vec<(Option<u64>, Vec<E::ScalarField>)>, HipError> {
        let per = 1 + self.m0 as usize;
        let mut raw = vec![0u64; 4 * per * count];
        let mut n = 0usize;
        // SAFETY: live context; `raw` holds per * count elements of 4 limbs.
        let rc = unsafe { sys::pm_prove_tap(ctx.raw, 9, raw.as_mut_ptr(), per * count, &mut n) };
        ctx.check(rc)?;
        if n != per * count {
            return Err(err(Status::InvalidArg, "solve_results: the last solving call had another count"));
        }
        let limbs = |i: usize| [raw[i], raw[i + 1], raw[i + 2], raw[i + 3]];
        Ok((0..count)
            .map(|r| {
                let at = 4 * per * r;
                let stuck = if raw[at] == u64::MAX { None } else { Some(raw[at]) };
                (stuck, (1..per).map(|j| fr_from_raw::<E>(self.curve, limbs(at + 4 * j))).collect())
            })
            .collect())
    }

    /// `pm_r1cs_check`: which constraints the assignment violates -- what `ConstraintSystem::which_is_unsatisfied` answers on the
    /// host, from the key's resident matrices; the call to make after a `RemainderNonzero`.  `instance` carries the leading one.
    /// Returns the number of rows r with (Az)_r (Bz)_r != (Cz)_r and the `min(n_bad, max_rows)` smallest of them in ascending
    /// order (a row index is the constraint's position in the matrices the key was made from).  The count is zero exactly when
    /// the prover's witness check passes.  A proof in flight on `ctx` is not disturbed.
    pub fn check_assignment<E: Pairing>(
        &self,
        ctx: &mut Context,
        instance: &[E::ScalarField],
        witness: &[E::ScalarField],
        max_rows: usize,
    ) -> Result<(u64, Vec<u64>), HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "key of another curve"));
        }
        if instance.len() as u64 != self.m0 || witness.len() as u64 != self.mw {
            return Err(err(Status::LenMismatch, "the instance / witness length is not the key's"));
        }
        let mut n_bad = 0u64;
        let mut rows = vec![u64::MAX; max_rows];
        let w_ptr = if witness.is_empty() { core::ptr::null() } else { fr_ptr(witness) };
        let rows_ptr = if max_rows == 0 { core::ptr::null_mut() } else { rows.as_mut_ptr() };
        // SAFETY: live key and context; instance / witness hold m0 / mw elements (layout checked), `rows` has max_rows slots,
        // the residuals are not asked for.
        let rc = unsafe { sys::pm_r1cs_check(ctx.raw, self.raw, fr_ptr(instance), w_ptr, 0, max_rows, &mut n_bad, rows_ptr, core::ptr::null_mut()) };
        ctx.check(rc)?;
        rows.truncate((n_bad as usize).min(max_rows));
        Ok((n_bad, rows))
    }

    /// Declare the witness solver's hints of this key (`pm_pk_load_bytes` with `PM_KEY_HINTS`: no key is loaded, this one keeps its
    /// address) -- `desc` is the sequence of records the header states (`PM_HINT_LONGDIV, n, kq, kr, kD, kE, flags`, then the columns
    /// or literal limbs; `PM_HINT_MODDIV, n, kz, kNp, kNm, kDp, kDm, kP, flags` for a modular division; [`Hint::encode`] writes
    /// both, and `PM_HINT_LONGDIV_WIDE`, which has the long division's layout); an empty slice clears the declaration.  Taking `&mut self` keeps safe code from racing the call with calls
    /// that use the key.
    pub fn set_hints(&mut self, ctx: &mut Context, desc: &[u64]) -> Result<(), HipError> {
        let ptr = if desc.is_empty() { core::ptr::null() } else { desc.as_ptr() as *const u8 };
        let mut key = self.raw;
        // `desc` holds `8 * desc.len()` bytes, which the library only reads and copies; under PM_KEY_HINTS `key` is read and left as it is
        let rc = Self::load_bytes_raw(ctx, self.curve, ptr, 8 * desc.len(), sys::PM_KEY_HINTS, &mut key);
        debug_assert!(key == self.raw);
        ctx.check(rc)
    }

    /// `pm_pk_info`: n, m0, sigma, omega and the six base-vector lengths of this key.
    pub fn info<E: Pairing>(&self) -> Result<KeyInfo<E>, HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "key of another curve"));
        }
        let (mut n, mut m0, mut sigma) = (0u64, 0u64, 0u64);
        let mut omega = [0u64; 4];
        let mut base_lens = [0u64; 6];
        // SAFETY: live key; five valid out-pointers (4 limbs for omega, PM_NUM_BASE_VECS = 6 lengths).
        let rc = unsafe { sys::pm_pk_info(self.raw, &mut n, &mut m0, &mut sigma, omega.as_mut_ptr(), base_lens.as_mut_ptr()) };
        if rc != sys::PM_OK {
            return Err(err(Status::from_raw(rc), "pm_pk_info failed"));
        }
        Ok(KeyInfo { n, m0, sigma, omega: fr_from_raw::<E>(curve, omega), base_lens })
    }

    /// `pm_pk_export_bases_compressed`: one base vector as the point records of a key file, encoded on the device -- 48 / 32 bytes
    /// a point in [`WireForm::Compressed`], 96 / 64 in [`WireForm::Uncompressed`] (`which | PM_WIRE_UNCOMPRESSED`).
    pub fn export_bases_bytes<E: Pairing>(&self, ctx: &mut Context, which: BaseVec, form: WireForm) -> Result<Vec<u8>, HipError> {
        let info = self.info::<E>()?;
        let total = info.base_lens[which as usize] as usize;
        let record = 8 * self.curve.fq_limbs() * if form == WireForm::Uncompressed { 2 } else { 1 };
        let mut out = vec![0u8; record * total];
        // SAFETY: `out` holds `total` records of the form's size.
        let rc = unsafe { sys::pm_pk_export_bases_compressed(ctx.raw, self.raw, which as i32 | form as i32, 0, total, out.as_mut_ptr()) };
        ctx.check(rc)?;
        Ok(out)
    }

    /// `pm_pk_export_bases`: one base vector back on the host as `Vec<E::G1Affine>`, ready for a `ProvingKey<E>` field.  The
    /// device hands over `x || y` in Montgomery form (16 * fq_limbs bytes per point, the identity as all-zero x, y); records are
    /// rebuilt with `Affine::new_unchecked` / `Affine::identity()` -- no decompression, no subgroup check (the points were
    /// computed as multiples of the generator).  Copied in chunks of 2^18 points so the staging buffer stays small.
    pub fn export_bases<E: Pairing>(&self, ctx: &mut Context, which: BaseVec) -> Result<Vec<E::G1Affine>, HipError> {
        let info = self.info::<E>()?;
        let curve = self.curve;
        let words = 2 * curve.fq_limbs();
        let total = info.base_lens[which as usize] as usize;
        let mut out = Vec::with_capacity(total);
        const CHUNK: usize = 1 << 18;
        let mut staging = vec![0u64; words * CHUNK.min(total.max(1))];
        let mut offset = 0usize;
        while offset < total {
            let len = CHUNK.min(total - offset);
            // SAFETY: live key and context; `staging` has room for `len` points of `words` u64 each.
            let rc = unsafe { sys::pm_pk_export_bases(ctx.raw, self.raw, which as i32, offset, len, staging.as_mut_ptr()) };
            ctx.check(rc)?;
            for p in staging[..words * len].chunks_exact(words) {
                let mut xy = [0u64; 12];
                xy[..words].copy_from_slice(p);
                let inf = p.iter().all(|&w| w == 0) as i32;
                out.push(g1_from_raw::<E>(curve, &xy, inf));
            }
            offset += len;
        }
        Ok(out)
    }

    /// All six vectors, in the shape of `ProvingKey<E>`'s fields.
    pub fn export_all<E: Pairing>(&self, ctx: &mut Context) -> Result<ExportedBases<E>, HipError> {
        Ok(ExportedBases {
            x_powers_g1: self.export_bases::<E>(ctx, BaseVec::XPowers)?,
            x_powers_y_alpha_g1: self.export_bases::<E>(ctx, BaseVec::XPowersYAlpha)?,
            x_powers_y_gamma_g1: self.export_bases::<E>(ctx, BaseVec::XPowersYGamma)?,
            x_powers_y_gamma_z_g1: self.export_bases::<E>(ctx, BaseVec::XPowersYGammaZ)?,
            x_powers_zh_by_y_alpha_g1: self.export_bases::<E>(ctx, BaseVec::XPowersZhByYAlpha)?,
            uj_wj_lcs_by_y_alpha_g1: self.export_bases::<E>(ctx, BaseVec::UjWjLcsByYAlpha)?,
        })
    }

    pub fn raw(&self) -> *const sys::pm_pk {
        self.raw
    }
}

/// `pm_wire_form`: the record form of a key's points, a flag OR-ed into `validate` / `which`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum WireForm {
    Compressed = sys::PM_WIRE_COMPRESSED,
    Uncompressed = sys::PM_WIRE_UNCOMPRESSED,
}

/// `pm_shard_layout`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum ShardLayout {
    Pairs = 0,
    Vector = 1,
}

impl Drop for GpuKey {
    fn drop(&mut self) {
        // SAFETY: created by pm_pk_load / pm_pk_generate, freed once.
        unsafe { sys::pm_pk_free(self.raw) }
    }
}

/// Keys already uploaded, by an identity the caller chooses (the reference patch uses blake3 of the verifying key's bytes):
/// `ProvingKey<E>` is a plain struct of `Vec`s and cannot carry a device handle itself.
#[derive(Default)]
pub struct GpuKeyCache {
    map: Mutex<HashMap<[u8; 32], Arc<GpuKey>>>,
}

impl GpuKeyCache {
    pub fn get_or_upload(&self, id: [u8; 32], upload: impl FnOnce() -> Result<GpuKey, HipError>) -> Result<Arc<GpuKey>, HipError> {
        if let Some(k) = self.map.lock().expect("key cache poisoned").get(&id) {
            return Ok(k.clone());
        }
        let k = Arc::new(upload()?); // outside the lock: an upload takes seconds (window tables are built on the device)
        Ok(self.map.lock().expect("key cache poisoned").entry(id).or_insert(k).clone())
    }

    /// Register a key that is ALREADY resident (made by [`GpuKey::generate`]) under `id`, so the first proof with the
    /// `ProvingKey<E>` built from its exported vectors neither re-uploads ~3 GB of bases nor rebuilds the window tables.
    /// An entry already present under `id` wins (and `key` is freed).
    pub fn adopt(&self, id: [u8; 32], key: GpuKey) -> Arc<GpuKey> {
        self.map.lock().expect("key cache poisoned").entry(id).or_insert_with(|| Arc::new(key)).clone()
    }

    pub fn forget(&self, id: &[u8; 32]) {
        self.map.lock().expect("key cache poisoned").remove(id);
    }
}

pub fn global_key_cache() -> &'static GpuKeyCache {
    static CACHE: OnceLock<GpuKeyCache> = OnceLock::new();
    CACHE.get_or_init(GpuKeyCache::default)
}

// ------------------------------------------------------------------------------------------ multi-GPU exchange layer
/// One rank's `pm_comm` (include/polymath_hip.h, "multi-GPU exchange layer"): RCCL inside the library, one process per GPU.
/// Rank 0 makes the 128-byte id ([`Comm::rccl_unique_id`]) and ships it to the other ranks over the job's own channel (MPI, a
/// TCP store, a file); every rank then calls [`Comm::rccl`] (collective: ncclCommInitRank) and joins its context with
/// [`Context::set_comm`].  Collectives have a deadline; a failed communicator stays failed ([`Comm::failed`]).
pub struct Comm {
    raw: *mut sys::pm_comm,
}

// SAFETY: a pm_comm is used by the one thread that drives its rank's context (plus the library's own watchdog thread).
unsafe impl Send for Comm {}

impl Comm {
    pub fn rccl_unique_id() -> Result<[u8; 128], HipError> {
        let mut id = [0u8; 128];
        // SAFETY: 128 writable bytes.
        let rc = unsafe { sys::pm_comm_rccl_unique_id(id.as_mut_ptr() as *mut c_void) };
        if rc != sys::PM_OK {
            return Err(err(Status::from_raw(rc), "pm_comm_rccl_unique_id failed (librccl could not be loaded?)"));
        }
        Ok(id)
    }

    pub fn rccl(unique_id: &[u8; 128], rank: i32, world: i32, device: i32) -> Result<Comm, HipError> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: 128 readable bytes, a valid out-pointer.
        let rc = unsafe { sys::pm_comm_rccl_create(unique_id.as_ptr() as *const c_void, rank, world, device, &mut raw) };
        if rc != sys::PM_OK || raw.is_null() {
            return Err(err(Status::from_raw(rc), "pm_comm_rccl_create failed"));
        }
        Ok(Comm { raw })
    }

    pub fn set_timeout_ms(&mut self, ms: i64) -> Result<(), HipError> {
        // SAFETY: live communicator.
        let rc = unsafe { sys::pm_comm_set_timeout_ms(self.raw, ms as core::ffi::c_long) };
        if rc == sys::PM_OK { Ok(()) } else { Err(err(Status::from_raw(rc), "pm_comm_set_timeout_ms")) }
    }

    pub fn failed(&self) -> bool {
        // SAFETY: live communicator.
        unsafe { sys::pm_comm_failed(self.raw) != 0 }
    }

    pub fn last_error(&self) -> String {
        // SAFETY: live communicator; the library returns a NUL-terminated copy it owns.
        unsafe { CStr::from_ptr(sys::pm_comm_last_error(self.raw)) }.to_string_lossy().into_owned()
    }

    /// Sum over the ranks of `points` (a [`ShardLayout::Pairs`] key's partial results), in place: all-gather + `pm_g1_sum`
    /// (RCCL has no elliptic-curve reduction).
    pub fn combine_points<E: Pairing>(&mut self, points: &mut [E::G1Affine]) -> Result<(), HipError> {
        let curve = curve_checked::<E>()?;
        let words = 2 * curve.fq_limbs();
        let mut xy = vec![0u64; words * points.len()];
        let mut inf = vec![0i32; points.len()];
        for (i, p) in points.iter().enumerate() {
            let raw = raw_words(p, words);
            inf[i] = raw_byte(p, 8 * words) as i32;
            if inf[i] == 0 {
                xy[i * words..(i + 1) * words].copy_from_slice(&raw);
            }
        }
        // SAFETY: `count` points of `words` u64 each and as many flags.
        let rc = unsafe { sys::pm_comm_combine_points(self.raw, curve.id(), points.len() as i32, xy.as_mut_ptr(), inf.as_mut_ptr()) };
        if rc != sys::PM_OK {
            return Err(HipError { status: Status::from_raw(rc), message: self.last_error() });
        }
        for (i, p) in points.iter_mut().enumerate() {
            let mut buf = [0u64; 12];
            buf[..words].copy_from_slice(&xy[i * words..(i + 1) * words]);
            *p = g1_from_raw::<E>(curve, &buf, inf[i]);
        }
        Ok(())
    }
}

impl Drop for Comm {
    fn drop(&mut self) {
        // SAFETY: created by pm_comm_rccl_create, destroyed once; detach it from its context first (`Context::set_comm(None)`).
        unsafe { sys::pm_comm_destroy(self.raw) }
    }
}

impl Context {
    /// Join this context to its rank's communicator (required before proving on a [`ShardLayout::Vector`] key), or detach it.
    /// The context does not own the communicator: keep the `Comm` alive for as long as it is attached.
    pub fn set_comm(&mut self, comm: Option<&mut Comm>) -> Result<(), HipError> {
        let raw = comm.map_or(core::ptr::null_mut(), |c| c.raw);
        // SAFETY: live context; a null communicator detaches.
        let rc = unsafe { sys::pm_ctx_set_comm(self.raw, raw) };
        self.check(rc)
    }
}

// ------------------------------------------------------------------------------------------ resident bases
/// One `pm_bases`: a G1 base vector resident in HBM (an SRS that many polynomials are committed against).
pub struct ResidentBases {
    raw: *mut sys::pm_bases,
    curve: Curve,
    len: usize,
}

// SAFETY: the device allocation is immutable after upload; calls take the context by `&mut`.
unsafe impl Send for ResidentBases {}

impl ResidentBases {
    pub fn upload<E: Pairing>(ctx: &mut Context, bases: &[E::G1Affine]) -> Result<ResidentBases, HipError> {
        let curve = curve_checked::<E>()?;
        let mut raw = core::ptr::null_mut();
        // SAFETY: `bases.len()` points of size_of::<G1Affine>() bytes each (layout checked).
        let rc = unsafe { sys::pm_bases_upload(ctx.raw, curve.id(), bases.as_ptr() as *const c_void, core::mem::size_of::<E::G1Affine>(), bases.len(), &mut raw) };
        ctx.check(rc)?;
        Ok(ResidentBases { raw, curve, len: bases.len() })
    }

    pub fn len(&self) -> usize {
        self.len
    }

    pub fn is_empty(&self) -> bool {
        self.len == 0
    }

    /// `pm_msm_g1_resident_batch`: one MSM per row of `rows` (all of one length `len <= self.len() - offset`) against bases
    /// `[offset, offset + len)`, in one call.  Rows are copied into one contiguous host buffer first.
    pub fn msm_batch<E: Pairing>(&self, ctx: &mut Context, offset: usize, rows: &[&[E::ScalarField]]) -> Result<Vec<E::G1Affine>, HipError> {
        let curve = curve_checked::<E>()?;
        if curve != self.curve {
            return Err(err(Status::InvalidArg, "bases were uploaded for another curve"));
        }
        let len = rows.first().map_or(0, |r| r.len());
        if rows.iter().any(|r| r.len() != len) {
            return Err(err(Status::InvalidArg, "rows of a batch must have one length"));
        }
        let flat: Vec<E::ScalarField> = rows.iter().flat_map(|r| r.iter().copied()).collect();
        let mut xy = vec![0u64; rows.len() * 12];
        let mut inf = vec![0i32; rows.len()];
        let nq = 2 * curve.fq_limbs();
        // SAFETY: rows.len() * len scalars in (layout checked); rows.len() points of nq <= 12 words and as many flags out.
        let rc = unsafe { sys::pm_msm_g1_resident_batch(ctx.raw, self.raw, offset, fr_ptr(&flat), 0, len, rows.len(), xy.as_mut_ptr(), inf.as_mut_ptr()) };
        ctx.check(rc)?;
        Ok((0..rows.len())
            .map(|b| {
                let mut p = [0u64; 12];
                p[..nq].copy_from_slice(&xy[b * nq..(b + 1) * nq]);
                g1_from_raw::<E>(curve, &p, inf[b])
            })
            .collect())
    }
}

impl Drop for ResidentBases {
    fn drop(&mut self) {
        // SAFETY: created by pm_bases_upload, freed once.
        unsafe { sys::pm_bases_free(self.raw) }
    }
}

/// The device this process proves on: `POLYMATH_HIP_DEVICE`, else `LOCAL_RANK` (one process per GPU), else 0.
pub fn default_device() -> i32 {
    for var in ["POLYMATH_HIP_DEVICE", "LOCAL_RANK"] {
        if let Some(d) = std::env::var(var).ok().and_then(|v| v.parse().ok()) {
            return d;
        }
    }
    0
}
