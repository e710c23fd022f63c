/*
 * polymath_hip.h -- C ABI of libpolymath_hip.so, the MI355X (gfx950) implementation of
 * the Polymath prover hot path.  This is the drop-in boundary: everything the reference's
 * Rust crate would bind over FFI for `create_proof_with_assignment`
 * (/root/reference/src/prover.rs:66-237) plus the standalone MSM / NTT entry points the
 * headline metric is quoted on.  Plain pointers and sizes only; no C++/torch types.
 *
 * Data conventions (identical to arkworks' in-memory layout):
 *   Fr  : PM_FR_LIMBS  u64 little-endian limbs, MONTGOMERY form (R = 2^256).
 *   Fq  : fq_limbs     u64 little-endian limbs, MONTGOMERY form (R = 2^384 BLS12-381, 2^256 BN254).
 *   G1 affine in : x||y (2*fq_limbs u64) every `stride` bytes.  If stride > 16*fq_limbs the byte
 *                  at offset 16*fq_limbs is arkworks' `infinity: bool`; a point whose x and y are
 *                  both all-zero is also treated as the point at infinity.
 *   G1 affine out: x||y Montgomery into `out_xy` (2*fq_limbs u64) and *out_inf = 1 for infinity
 *                  (then x = y = 0).
 * All functions return PM_OK (0) or a pm_status error; none throws or aborts.  The caller owns
 * every host buffer; the library keeps no host pointer after a call returns.
 *
 * Threading: pm_pk is immutable after creation and may be shared by contexts on the same device;
 * a pm_ctx owns its HIP stream and per-proof state, so one proof in flight per ctx
 * (the reference has no global state: src/lib.rs:44-50).
 */
#ifndef POLYMATH_HIP_H
#define POLYMATH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_FR_LIMBS 4

typedef enum pm_curve {
    PM_BLS12_381 = 0, /* the reference's only instantiated curve (Cargo.toml:35) */
    PM_BN254 = 1      /* BASELINE.json configs[4] */
} pm_curve;

typedef enum pm_status {
    PM_OK = 0,
    PM_ERR_INVALID_ARG = 1,
    PM_ERR_LEN_MISMATCH = 2,       /* == assert!(scalars.len() <= g1_elems.len())  prover.rs:381 */
    PM_ERR_DOMAIN_TOO_LARGE = 3,   /* == D::new(..) None / PolynomialDegreeTooLarge prover.rs:83,317 */
    PM_ERR_REMAINDER_NONZERO = 4,  /* == assert!(rem_poly.is_zero())               prover.rs:108,221 */
    PM_ERR_DEGREE_BOUND = 5,       /* == degree asserts                            prover.rs:107,113,222 */
    PM_ERR_HIP = 6,                /* a HIP runtime call failed; see pm_last_error */
    PM_ERR_NO_DEVICE = 7,
    PM_ERR_STATE = 8,              /* phases called out of order */
    PM_ERR_COMM = 9                /* multi-GPU proofs only (no reference counterpart): a peer rank failed, or a collective
                                      did not complete within the communicator's deadline; the communicator is dead */
} pm_status;

typedef struct pm_ctx pm_ctx;
typedef struct pm_pk pm_pk;
typedef struct pm_bases pm_bases;

/* R1CS matrix in CSR form: what ark-relations `ConstraintMatrices` (generator.rs:46-54) holds as
 * Vec<Vec<(F, usize)>>, flattened.  Column 0 = One, 1..m0-1 instance, then witness. */
typedef struct pm_csr {
    uint64_t nrows;
    const uint64_t *rowptr; /* nrows+1 */
    const uint32_t *col;    /* nnz */
    const uint64_t *val;    /* nnz * PM_FR_LIMBS, Montgomery */
} pm_csr;

/* Base-vector selector, one per ProvingKey field (data_structures.rs:56-73). */
typedef enum pm_base_vec {
    PM_X_POWERS = 0,             /* x_powers_g1                  n+1 points     generator.rs:82  */
    PM_X_POWERS_Y_ALPHA = 1,     /* x_powers_y_alpha_g1          3 points       generator.rs:86  */
    PM_X_POWERS_Y_GAMMA = 2,     /* x_powers_y_gamma_g1          2 points       generator.rs:90  */
    PM_X_POWERS_Y_GAMMA_Z = 3,   /* x_powers_y_gamma_z_g1        10n+23 points  generator.rs:94  */
    PM_X_POWERS_ZH_BY_Y_ALPHA = 4,/* x_powers_zh_by_y_alpha_g1   n-1 points     generator.rs:107 */
    PM_UJ_WJ_LCS_BY_Y_ALPHA = 5, /* uj_wj_lcs_by_y_alpha_g1      M-m0 points    generator.rs:115 */
    PM_NUM_BASE_VECS = 6
} pm_base_vec;

/* How a key is spread over the ranks of a multi-GPU proof.
 *   PM_SHARD_PAIRS : only the MSM pair ranges are sharded (contiguous 1/N slices); witness map, NTTs and scans are
 *                    replicated on every rank (BASELINE.json configs[2]: "MSM buckets sharded").
 *   PM_SHARD_VECTOR: the vector phases are sharded too (configs[3]: "NTT domain + MSM both 8-way partitioned"):
 *                    evaluations cyclic, coefficients blocked (polymath_amd/host/layout.hpp), four-step NTT with one
 *                    all-to-all per transform, scans exchange per-segment values; the ranks' contexts must be joined
 *                    by a pm_comm (pm_ctx_set_comm).  Needs shard_count a power of two with shard_count^2 | n. */
typedef enum pm_shard_layout { PM_SHARD_PAIRS = 0, PM_SHARD_VECTOR = 1 } pm_shard_layout;

typedef struct pm_base_array {
    const void *points; /* host pointer, G1 affine-in convention above */
    size_t len;         /* number of points */
    size_t stride;      /* bytes between points */
} pm_base_array;

/* ---- library / context ------------------------------------------------------------------ */
int pm_device_count(void);
int pm_ctx_create(int device, pm_ctx **out);
void pm_ctx_destroy(pm_ctx *ctx);
const char *pm_last_error(const pm_ctx *ctx);
/* Wall-clock GPU milliseconds of the most recent call's kernels, by stage (hipEvent timers;
 * replaces the reference's start_timer!/end_timer! tracing, prover.rs:32-61).  After pm_host_prove[_sharded] the
 * slots cover the whole proof and the events are read HERE (a few dozen event queries, ~0.1 ms of host time), not
 * between the proof's phases: call it from the thread that proved, before the context's next call.  It MUTATES the
 * context (pending events are read and recycled, the device is made current): not thread-safe against any other call on
 * the same context -- hence no const. */
int pm_last_timings(pm_ctx *ctx, double *ms_out, int n_slots);

/* ---- options -----------------------------------------------------------------------------
 * What a host may choose, per context.  The reference keeps no global state (src/lib.rs:44-50: `Polymath<E, T>` is a
 * PhantomData), so neither does the library: every mode below is a field of the context, set through this call, and
 * contexts with different settings prove side by side.  The environment variables named in the comments only give a
 * new context its DEFAULTS -- they are read once, in pm_ctx_create, never while a proof runs.  Options marked (key) are
 * read when a key or a resident base vector is created on the context (pm_pk_generate / pm_pk_load / pm_bases_precompute)
 * and stay with that key. */
typedef enum pm_option {
    PM_OPT_MSM_OVERLAP = 0,       /* 0 / 1: the [a]_1 and [c]_1 MSMs of phase 1 (prover.rs:118-123,132) run concurrently.
                                   * Default 1 (PM_MSM_OVERLAP). */
    PM_OPT_NTT_OVERLAP = 1,       /* 0 / 1, multi-GPU proofs: w's distributed transform on a second stream beside u's chain
                                   * (prover.rs:93-96: the two are independent).  Default 1 (PM_NTT_OVERLAP). */
    PM_OPT_TABLES = 2,            /* (key) pm_tables_mode.  Default PM_TABLES_AUTO (PM_TABLES = 0 | 1 | wide, PM_WIDE = 0). */
    PM_OPT_MSM_MAX_PIECE_LOG = 3, /* one bucket pipeline covers at most 2^v pairs, 4 <= v <= 27; longer MSMs run in pieces.
                                   * Default 27 (PM_MSM_MAX_PIECE_LOG); lower values exercise the piece split at small sizes. */
    PM_OPT_MAX_SEG_LOG = 4,       /* (key, multi-GPU) sub-segments of the division scan hold at most 2^v indices; 0 = chosen
                                   * from n and the world size.  Default 0 (PM_MAX_SEG_LOG). */
    PM_OPT_INFLIGHT_CONTEXTS = 5, /* (key) how many contexts will prove on the key at once: their per-proof vectors and MSM
                                   * workspaces are left out of the HBM granted to window tables.  Default 1 (PM_INFLIGHT_CONTEXTS). */
    PM_OPT_MSM_TASK_LEN = 6,      /* entries of one bucket-accumulation task; 0 = twice the mean bucket load.  Default 0 (PM_MSM_SEG). */
    PM_OPT_TABLE_WINDOW_BITS = 7, /* (key) developer knob (tuning sweeps, tests) over the MSM window plans; default 0 (PM_TABLE_C).
                                   * Decoded in one place, csrc/msm_plan.h: decode_window_option.  Accepted, 0 ... 532:
                                   *   0          the cost models choose (tables_plan for window tables, wide_plan without them);
                                   *   4 ... 24   the widest window of the power-of-two layout: ceil(256 / v) windows of v bits or one
                                   *              fewer, taken as it is (the MSM is refused if the kernels cannot run it: more than 32
                                   *              windows, i.e. v < 8).  A key's MSMs without tables (wide mode) are held to v as well
                                   *              when 16 <= v <= 23: 16, 18, 19, 20, 22 name 16, 15, 14, 13, 12 windows; 17, 21 and 23
                                   *              name none, and such an MSM then runs the per-window pipeline;
                                   *   100 m + w  the window radix m 2^a on w windows: m = 1 the power-of-two layout, 10 <= w <= 32; m = 5
                                   *              radix 5 2^a, 10 <= w <= 16 (a = the smallest shift that covers the scalar field);
                                   *              w = 0: the cost model's count for that m.  100 restores the power-of-two plans, 511 is
                                   *              11 windows of radix 5 2^21.  Wide mode plans as for 0.  Any other m or w: no tables;
                                   *   1 ... 3, 25 ... 99   name nothing: as 0. */
    PM_OPT_WIRE_CHUNK_LOG = 8,    /* compressed points per staging chunk of pm_pk_load_bytes / pm_g1_decode /
                                   * pm_pk_export_bases_compressed: 2^v, 4 <= v <= 24.  Default 20 (PM_WIRE_CHUNK_LOG); lower values put
                                   * chunk boundaries inside small vectors (tests). */
    PM_NUM_OPTIONS = 9
} pm_option;
typedef enum pm_tables_mode {
    PM_TABLES_OFF = 0,      /* no window tables, no wide mode: every MSM on the per-window pipeline */
    PM_TABLES_AUTO = 1,     /* tables for the MSMs whose tables fit in HBM, the wide mode for the others */
    PM_TABLES_WIDE = 2,     /* the wide mode for every MSM (test / tuning) */
    PM_TABLES_NO_WIDE = 3   /* tables where they fit, the per-window pipeline for the others */
} pm_tables_mode;
/* PM_ERR_INVALID_ARG for an unknown option or a value outside its range.  A change takes effect at the next phase (next MSM,
 * next key) the context starts; call it from the thread that drives the context. */
int pm_ctx_set_option(pm_ctx *ctx, int option, long long value);
int pm_ctx_get_option(const pm_ctx *ctx, int option, long long *value);

/* ---- standalone kernels (unit parity + the "G1 MSM pairs/s" metric) ----------------------- */
/* Radix-2 NTT over Fr, natural order in and out, like ark-poly Radix2EvaluationDomain::fft /
 * ifft (prover.rs:241,319,325); inverse scales by 1/n.  `data` is a HOST buffer of 2^log_n Fr. */
int pm_ntt(pm_ctx *ctx, int curve, uint64_t *data, unsigned log_n, int inverse);
/* Same on a DEVICE buffer (hipMalloc'd by the caller, e.g. a torch tensor's data_ptr).  The transform runs on the context's own
 * non-blocking stream and has finished when the call returns; work of the caller's streams that writes the buffer must be
 * complete before the call. */
int pm_ntt_device(pm_ctx *ctx, int curve, uint64_t *d_data, unsigned log_n, int inverse);
/* `rows` transforms of 2^log_n points each on a DEVICE buffer, row b at d_data + b * row_stride Fr elements; the elements
 * between the end of a row and the start of the next (row_stride > 2^log_n) are neither read nor written.  rows == 0 is
 * PM_OK and touches nothing; PM_ERR_INVALID_ARG for rows > 65535 or row_stride < 2^log_n. */
int pm_ntt_batch_device(pm_ctx *ctx, int curve, uint64_t *d_data, unsigned log_n, int inverse, size_t rows, size_t row_stride);

/* Variable-base MSM == E::G1::msm_unchecked(bases, scalars) (prover.rs:380-384), host buffers. */
int pm_msm_g1(pm_ctx *ctx, int curve, const void *bases, size_t base_stride, const uint64_t *scalars,
              size_t len, uint64_t *out_xy, int *out_inf);
/* Resident form: upload a base vector once (the pk's bases are fixed), then run MSMs against a
 * sub-range of it with scalars already in HBM (`d_scalars` device pointer) or on the host. */
int pm_bases_upload(pm_ctx *ctx, int curve, const void *bases, size_t base_stride, size_t len, pm_bases **out);
/* Synthetic base vector P_i = (i+1)*G built on the device (SURVEY.md §8d MSM micro-inputs). */
int pm_bases_generate_multiples(pm_ctx *ctx, int curve, size_t len, pm_bases **out);
/* Build the window tables 2^(c w) * P_i of a resident base vector (W x its memory): later resident MSMs
 * against it then need ceil(256/c) instead of 16 mixed additions per pair.  Proving keys do this
 * themselves when the tables fit in HBM (PM_TABLES=0 in the environment disables it). */
int pm_bases_precompute(pm_ctx *ctx, pm_bases *b);
int pm_bases_download(pm_ctx *ctx, const pm_bases *b, size_t offset, size_t len, uint64_t *out_xy);
size_t pm_bases_len(const pm_bases *b);
void pm_bases_free(pm_bases *b);
int pm_msm_g1_resident(pm_ctx *ctx, const pm_bases *bases, size_t base_offset, const uint64_t *scalars,
                       int scalars_on_device, size_t len, uint64_t *out_xy, int *out_inf);
/* `batch` MSMs of `len` pairs each against the SAME base range [base_offset, base_offset + len) in one call: row b is
 * scalars[b * len .. (b + 1) * len) (Montgomery Fr, 4 limbs each), its result out_xy[b] (2 fq limb vectors) and out_inf[b], in the
 * form pm_msm_g1_resident gives.  Same argument checks and status codes; batch == 0 writes nothing, len == 0 gives every row the
 * identity, batch == 1 is pm_msm_g1_resident itself.  Runs the per-window pipeline over the plain resident points: window tables
 * (pm_bases_precompute) and wide plans are not used by batches; the results are the same on a precomputed pm_bases. */
int pm_msm_g1_resident_batch(pm_ctx *ctx, const pm_bases *bases, size_t base_offset, const uint64_t *scalars,
                             int scalars_on_device, size_t len, size_t batch, uint64_t *out_xy, int *out_inf);

/* Host-side G1 helpers used to combine per-GPU partial MSM results (RCCL has no
 * elliptic-curve reduction op, so partial points are all-gathered and summed locally). */
int pm_g1_sum(int curve, const uint64_t *points_xy, const int *infs, size_t count, uint64_t *out_xy, int *out_inf);

/* ---- proving key ------------------------------------------------------------------------ */
/* Upload an existing ProvingKey (data_structures.rs:56-73).  `shard_rank/shard_count` keep only
 * the contiguous 1/shard_count slice of every MSM's pair range on this device;
 * pass 0,1 for a whole key. */
int pm_pk_load(pm_ctx *ctx, int curve, uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma,
               const pm_csr *a, const pm_csr *b, const pm_csr *c, const pm_base_array bases[PM_NUM_BASE_VECS],
               int shard_rank, int shard_count, pm_pk **out);
/* Circuit-specific setup on the device == generate_proving_key (generator.rs:24-167) with the two
 * rng draws (x then z, generator.rs:72,77) supplied by the caller so RNG stays on the host side.
 * Sparse O(nnz) replacement of the dense uj_wj_lcs loop; base vectors never leave HBM. */
int pm_pk_generate(pm_ctx *ctx, int curve, uint64_t m0, uint64_t mw, uint64_t nr, const pm_csr *a,
                   const pm_csr *b, const pm_csr *c, const uint64_t *x_trapdoor, const uint64_t *z_trapdoor,
                   int shard_rank, int shard_count, pm_pk **out);
/* The same two with the shard layout chosen (pm_shard_layout); pm_pk_load / pm_pk_generate are layout PM_SHARD_PAIRS. */
int pm_pk_load_sharded(pm_ctx *ctx, int curve, uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma,
                       const pm_csr *a, const pm_csr *b, const pm_csr *c, const pm_base_array bases[PM_NUM_BASE_VECS],
                       int shard_rank, int shard_count, int layout, pm_pk **out);
int pm_pk_generate_sharded(pm_ctx *ctx, int curve, uint64_t m0, uint64_t mw, uint64_t nr, const pm_csr *a,
                           const pm_csr *b, const pm_csr *c, const uint64_t *x_trapdoor, const uint64_t *z_trapdoor,
                           int shard_rank, int shard_count, int layout, pm_pk **out);
/* PM_SHARD_VECTOR index maps (polymath_amd/host/layout.hpp), host arithmetic only: out[p] = the global coefficient index
 * (coefficients != 0) or evaluation row (coefficients == 0) of local position p < n / shard_count of rank shard_rank. */
int pm_layout_indices(uint64_t n, int shard_count, int shard_rank, int coefficients, uint64_t *out);
/* The resident pairs of merged MSM `which` on this key/shard, as ranges [cat_lo, cat_lo + count) of the logical base
 * concatenation [uj_wj_lcs | x_powers_zh | x_powers | y_alpha | y_gamma | y_gamma_z], in device / scalar order. */
int pm_pk_msm_pieces(const pm_pk *pk, int which, uint64_t *cat_lo, uint64_t *count, size_t capacity, size_t *n_pieces);
int pm_pk_info(const pm_pk *pk, uint64_t *n, uint64_t *m0, uint64_t *sigma, uint64_t *omega /*Fr*/,
               uint64_t base_lens[PM_NUM_BASE_VECS]);
/* How merged MSM `which` (0 = [a]_1: prover.rs:118,330-338; 1 = [c]_1: :121,340-357; 2 = [d]_1: :229) runs on
 * this key/shard: resident pairs, bucket additions per pair (windows), widest window in bits, and whether the
 * key holds window tables for it.  Measurement aid (bench.py's VALU roofline); no reference counterpart. */
int pm_pk_msm_plan(const pm_pk *pk, int which, uint64_t *pairs, unsigned *windows, unsigned *window_bits, int *tables);
/* Copy (a range of) one base vector back to the host, x||y Montgomery, 16*fq_limbs bytes apart. */
int pm_pk_export_bases(pm_ctx *ctx, const pm_pk *pk, int which, size_t offset, size_t len, uint64_t *out_xy);
/* The witness solver's DECLARED HINTS (PM_ASSIGNMENT_SOLVE, "Declared hints" below): values that the circuit's witness generator
 * computes and no row determines.  They belong to the key, because they are part of the circuit, like the matrices.  The call is
 *     pm_pk_set_hints(ctx, pk, desc, n_words)  ==  pm_pk_load_bytes(ctx, curve of pk, (const uint8_t *)desc, 8 * n_words, PM_KEY_HINTS, 0, 1, 0, &pk)
 * -- a FLAG of pm_pk_load_bytes' `validate` (below) and no entry point of its own, because the set of entry points is pinned.
 * `pm_pk_set_hints` is ONLY SHORTHAND for that call, here and in the text of pm_last_error: the library exports no function of that
 * name and a C caller calls pm_pk_load_bytes as written above (the Python and Rust wrappers have a set_hints that does).  With
 * the flag no key is loaded and *out is not replaced: `bytes` is the declaration for the existing key *out.  PM_KEY_HINTS stands alone
 * in `validate`, `curve` is the key's and `len` a multiple of 8, else PM_ERR_INVALID_ARG.  `desc` is a sequence of records of n_words
 * 64-bit words (in memory order) in all; the first opcode is limb-wise long division (the second, modular division, follows below):
 *     PM_HINT_LONGDIV, n, kq, kr, kD, kE, flags,
 *       kq quotient columns, kr remainder columns, kD dividend columns, then kE divisor columns
 *       -- or, with PM_HINT_DIVISOR_LITERAL (flags bit 0), kE limb values of four words each (canonical integers, little-endian)
 * Columns are CSR columns: 0 is the constant one, then the instance, then the witness.  The step stores the kq n-bit limbs of
 * floor(D / E) and the kr n-bit limbs of D mod E for D = sum_j int(z_{D_j}) 2^(n j), E alike or the literal.
 * PM_ERR_INVALID_ARG, pm_last_error naming the hint's index and the condition, the key unchanged: an unknown opcode, unknown flags or
 * a truncated record; n outside 1..128; kD > 32, kE > 16, kq > 32, kr > 16, or any of them 0; n (kD - 1) >= 1024 or
 * n (kE - 1) >= 512; a column >= m0 + mw; an output that is column 0; an output named twice, or by two hints, or also an input of
 * its own hint; a literal limb >= r; a sharded key.  The refusals' text begins "pm_pk_set_hints: hint h: ".  A second call replaces
 * the declaration and n_words = 0 clears it; a context's solving plan is rebuilt after either.  The caller must not race the call with
 * calls that use the key, as with pm_pk_free.
 * Out of scope for the long-division record: other opcodes (modular inverse, gcd, sorting), signed limbs, dividends beyond 1024 bits (RSA-2048), hints on sharded
 * keys, per-assignment declarations, inferring a hint from rows.  Of these, modular inverse and modular division have a record of
 * their own in the same stream (opcode 3; opcode 2 stays reserved and is refused as unknown):
 *     PM_HINT_MODDIV, n, kz, kNp, kNm, kDp, kDm, kP, flags,
 *       kz output columns, kNp + kNm numerator columns, kDp + kDm denominator columns, then kP modulus columns
 *       -- or, with PM_HINT_MODULUS_LITERAL (flags bit 0), kP limb values of four words each
 * With each column list the sum of int(z_c_j) 2^(n j) (int: the canonical integer; limbs need not be normalised), N = N+ - N-,
 * D = D+ - D- and P the modulus, the step stores the kz n-bit limbs of the unique Z in [0, P) with Z D = N (mod P): the slope
 * (Y2 - Y1) / (X2 - X1) of an affine point addition, ark-r1cs-std's non-native inverse, circom-ecdsa's BigModInv.  kNp = kNm = 0
 * means N = 1, a plain inverse.  P need not be prime.  Refused like the long-division record, with the same wording for columns,
 * outputs, literal limbs and sharded keys: unknown flags; a truncated record; n outside 1..128; kz outside 1..16 or kP outside 1..16;
 * kDp outside 1..32; kNp, kNm or kDm above 32; n (k - 1) >= 1024 for an operand list; n (kP - 1) >= 512.  Records of both opcodes
 * may be mixed in one declaration; they share the index h, and no output may be named by two hints of either opcode.
 * Still out of scope: even moduli, operands beyond 1024 bits, the slope of a doubling as one hint (its numerator is a product), gcd,
 * sorting.  Of the long-division record's list, dividends beyond 1024 bits (RSA-2048) now have a record of their own in the same stream
 * (opcode 5; opcodes 2 and 4 are refused as unknown):
 *     PM_HINT_LONGDIV_WIDE, n, kq, kr, kD, kE, flags,
 *       kq quotient columns, kr remainder columns, kD dividend columns, then kE divisor columns
 *       -- or, with PM_HINT_DIVISOR_LITERAL (flags bit 0, the literal flag of opcode 1), kE limb values of four words each
 * It has the shape and the meaning of PM_HINT_LONGDIV: the step stores the kq n-bit limbs of floor(D / E) and the kr n-bit limbs of
 * D mod E, limbs need not be normalised.  An RSA-2048 modular multiplication divides a dividend of about 4200 bits by a 2048-bit
 * modulus: 32 limbs of 64 bits, or the 17 limbs of 121 bits of the zk-email circuits.  Refused like the long-division record, with the
 * same wording for columns, outputs, literal limbs and sharded keys: unknown flags; a truncated record; n outside 1..128; kD > 128,
 * kE > 64, kq > 128, kr > 64, or any of them 0; n (kD - 1) >= 8192 or n (kE - 1) >= 4096.  Records of all three opcodes may be mixed
 * in one declaration; they share the index h, and no output may be named by two hints of any opcode.  PM_HINT_LONGDIV itself is not
 * widened: kD = 33 under opcode 1 is refused as before.
 * Still out of scope: modular division at these widths (PM_HINT_MODDIV keeps 1024 / 512 bits), even moduli, linear blocks beyond 64
 * unknowns (RSA-4096 at 64-bit limbs; 3072-bit moduli at 96-bit limbs fit this record), hints on sharded keys, per-assignment
 * declarations, gcd, sorting.  Of the modular record's list, the slope of a doubling now has a record of its own in the same stream
 * (opcode 7; opcodes 2, 4 and 6 are refused as unknown, and so is 8):
 *     PM_HINT_MODMULDIV, n, kz, kA, kB, kNp, kNm, kDp, kDm, kP, flags, cN, cD,
 *       kz output columns, kA + kB factor columns, kNp + kNm addend columns, kDp + kDm denominator columns, then kP modulus columns
 *       -- or, with PM_HINT_MODULUS_LITERAL (flags bit 0, the literal flag of opcode 3), kP limb values of four words each
 * With each column list the sum of int(z_c_j) 2^(n j) (limbs need not be normalised) the step stores the kz n-bit limbs of the unique
 * Z in [0, P) with cD (D+ - D-) Z = cN (A B + N+ - N-) (mod P).  cN and cD are one-word literals in 1 .. 2^32 - 1; because they are
 * small literals the record works with a modulus held in columns as well.  The slope 3 X^2 / (2 Y) of a tangent (circom-ecdsa's
 * Secp256k1Double, every "lamda <-- ..." of a doubling) is A = B = X, D+ = Y, cN = 3, cD = 2: A and B may name the same columns.
 * kDp = kDm = 0 means D = 1, a modular multiply-add (the remainder of A B + C without its quotient); kNp = kNm = 0 means no addend.
 * Refused like the modular record, with the same wording for columns, outputs, literal limbs and sharded keys: unknown flags; a
 * truncated record; n outside 1..128; kz outside 1..16 or kP outside 1..16; kA or kB outside 1..32; kNp, kNm, kDp or kDm above 32;
 * kDm > 0 with kDp = 0; n (k - 1) >= 1024 for any of the six operand lists; n (kP - 1) >= 512; cN or cD outside 1 .. 2^32 - 1.
 * Records of all four opcodes may be mixed in one declaration; they share the index h, and no output may be named by two hints of
 * any opcode.  PM_HINT_MODDIV itself is not touched: its record, its results and its plans are what they were.
 * Still out of scope: curves with a != 0 as a case of their own (the numerator 3 X^2 + a is N+ = a, which this record allows);
 * complete addition formulas; windowed or GLV scalar multiplication; operands beyond 1024 bits; even moduli; hints on sharded keys;
 * per-assignment declarations. */
typedef enum pm_hint_op { PM_HINT_LONGDIV = 1 } pm_hint_op;
typedef enum pm_hint_flags { PM_HINT_DIVISOR_LITERAL = 1 } pm_hint_flags;
typedef enum pm_key_hints { PM_KEY_HINTS = 1024 } pm_key_hints;
typedef enum pm_hint_op_modular { PM_HINT_MODDIV = 3 } pm_hint_op_modular;
typedef enum pm_hint_moddiv_flags { PM_HINT_MODULUS_LITERAL = 1 } pm_hint_moddiv_flags;
typedef enum pm_hint_op_wide { PM_HINT_LONGDIV_WIDE = 5 } pm_hint_op_wide;
typedef enum pm_hint_op_muldiv { PM_HINT_MODMULDIV = 7 } pm_hint_op_muldiv;
void pm_pk_free(pm_pk *pk);

/* ---- proving keys as bytes: ProvingKey::serialize_compressed (data_structures.rs:56-73), decoded on the device ---------
 * Compressed G1 = ark-serialize's compressed form: BLS12-381 48 bytes, the zcash encoding (big-endian x, flags 0x80 compressed /
 * 0x40 infinity / 0x20 y > -y in the FIRST byte); BN254 32 bytes, ark's short-Weierstrass flags (little-endian x, 0x80 y > -y /
 * 0x40 infinity in the LAST byte, both at once is an error).  Infinity must be canonical (every other bit zero).  validate != 0 is
 * ark's Validate::Yes (deserialize_compressed: on the curve AND, on BLS12-381, in the prime-order subgroup, checked as [r]P == O);
 * validate == 0 is deserialize_compressed_unchecked (the curve equation is still enforced by decompression).  BN254's G1 has
 * cofactor 1.  The host mirror polymath_amd/host/wire.hpp (deser_g1 / ser_g1) is the specification, bit for bit. */
typedef enum pm_g1_status {       /* one verdict per point; the text is deser_g1's WireError for the same case */
    PM_G1_OK = 0,
    PM_G1_BAD_FLAGS = 1,          /* "G1: not a compressed point" (BLS12-381) / "G1: both flag bits set" (BN254) */
    PM_G1_COORD_GE_P = 2,         /* "G1: coordinate >= p" */
    PM_G1_NOT_ON_CURVE = 3,       /* "G1: not on the curve" (x^3 + b has no square root) */
    PM_G1_NOT_IN_SUBGROUP = 4,    /* "G1: not in the prime-order subgroup" (validate != 0, BLS12-381 only) */
    PM_G1_NONCANONICAL_INF = 5,   /* "G1: non-canonical encoding of the point at infinity" */
    PM_G1_INF_SIGN = 6            /* "G1: sign bit on the point at infinity" (BLS12-381; on BN254 that is PM_G1_BAD_FLAGS) */
} pm_g1_status;
/* The second record form: ark-serialize's Compress::No (ProvingKey::serialize_uncompressed), both coordinates of every point and no
 * square root on the way in.  PM_WIRE_UNCOMPRESSED is a FLAG, OR-ed into the `validate` argument of pm_g1_decode and
 * pm_pk_load_bytes and into the `which` argument of pm_pk_export_bases_compressed; there is no entry point of its own.
 *   BLS12-381 G1, 96 bytes: x || y, 48 bytes big-endian each, the three flag bits in byte 0 (x is read with them masked, y uses all
 *     384 bits).  0x80 set: PM_G1_BAD_FLAGS, whose text in this form is "G1: not an uncompressed point".  0x20 set: PM_G1_INF_SIGN
 *     next to 0x40, PM_G1_BAD_FLAGS on a finite point.  0x40: infinity, every other bit zero or PM_G1_NONCANONICAL_INF.
 *   BN254 G1, 64 bytes: x || y, 32 bytes little-endian each, the two flag bits in the LAST byte (byte 63; x's top byte carries
 *     none).  Both set: PM_G1_BAD_FLAGS.  0x40: infinity, every other bit zero.  0x80 on a finite point (ark's "y > -y") is written
 *     as the compressed form writes it and IGNORED by the reader, as ark's reader ignores it.
 * Then, in this order: a coordinate >= p is PM_G1_COORD_GE_P; y^2 != x^3 + b is PM_G1_NOT_ON_CURVE -- checked ALWAYS, with
 * validation off too (stricter than ark's deserialize_uncompressed_unchecked, which trusts the pair: a resident key's points are
 * curve points in every mode); with validation on, on BLS12-381, [r]P != O is PM_G1_NOT_IN_SUBGROUP.  pm_g1_status has no new value.
 * A key in this form is field for field the compressed string with every point long: the vk prefix (one G1, three G2 of 192 / 128
 * bytes, n, m0, sigma, omega) is 728 bytes on BLS12-381 and 504 on BN254.  Compressed bytes given with the flag, or uncompressed
 * bytes without it, are a malformed key (PM_ERR_INVALID_ARG): the form is never guessed.  pm_host_verify, pm_verify_batch[2] and
 * pm_host_make_vk keep taking and producing COMPRESSED vk and proof bytes; the host mirror (wire.hpp: read_vk_c / ser_vk_c with a
 * form) and the Python twin convert a vk between the two.
 * In `validate`, bit 8 selects the form and validation is on iff (validate & ~256) != 0, so 0 and 1 mean what they always meant.
 * One thing changes in the letter: a value with bit 8 set used to read as plain "validate"; no caller in this tree passes anything
 * but 0 or 1. */
typedef enum pm_wire_form { PM_WIRE_COMPRESSED = 0, PM_WIRE_UNCOMPRESSED = 256 } pm_wire_form;
/* Point validation says that every point of a key file is a point; it does not say that the points are a proving key.  Vectors of
 * one circuit beside the matrices of another, an [x]_2 of another ceremony, one record overwritten by another valid point: such a
 * file loads, proves at full speed, and no verifier accepts its proofs.  PM_KEY_CHECK_RELATIONS is a FLAG, OR-ed into the `validate`
 * argument of pm_pk_load_bytes only; there is no entry point of its own.  With it the loader decides, after the point verdicts and
 * BEFORE the window tables are built (a refused key does not pay for tables), whether the bytes are what generate_proving_key
 * (generator.rs:66-137) would have produced for SOME (x, z): every base vector is a fixed function of x, z and the key's own SAP
 * matrices, and the key carries [1]_1, [1]_2, [x]_2, [z]_2 as its vk prefix.  With a = 3, g = 5, s = sigma, T = x_powers_y_gamma_z_g1,
 * fresh 128-bit weights rho, and every check of the form e(A, [1]_2) e(B, [x]_2) e(C, [z]_2) = 1, in this order:
 *    0     x_powers_g1[0] == vk.one_g1                                       "x_powers_g1: the first entry is not vk.one_g1"
 *    1-5   per power vector V, in pm_base_vec order (x_powers_g1, x_powers_y_alpha_g1, x_powers_y_gamma_g1, x_powers_y_gamma_z_g1,
 *          x_powers_zh_by_y_alpha_g1):  e(sum rho_i V[i+1], [1]_2) = e(sum rho_i V[i], [x]_2)
 *                                                                            "<vector>: consecutive entries are not in ratio x"
 *    6-9   anchors:  e(T[g s], [1]_2) = e(one_g1, [z]_2);  e(x_powers_y_gamma_g1[0], [z]_2) = e(T[0], [1]_2);
 *          e(x_powers_y_alpha_g1[0], [z]_2) = e(T[(g - a) s], [1]_2);
 *          e(x_powers_zh_by_y_alpha_g1[0], [z]_2) = e(T[n + (a + g) s] - T[(a + g) s], [1]_2)
 *                                   "<vector>: is not anchored to vk.one_g1 and vk.z_g2"  (in the order T, y_gamma, y_alpha, zh)
 *    10    e(sum_j rho_j uj_wj_lcs[j], [z]_2) = e(sum_k U_k T[k + a s] + sum_k W_k T[k + (a + g) s], [1]_2), U = sum_j rho_j u_j,
 *          W = sum_j rho_j w_j over every SAP column j >= m0 (common.rs:138-207, first entry of a repeated column)
 *                                                                            "uj_wj_lcs_by_y_alpha_g1: does not match the SAP matrices"
 * A key that fails a relation is refused exactly as a key with a bad point is refused: PM_ERR_INVALID_ARG, no handle, nothing stays
 * allocated, and pm_last_error is "pm_pk_load_bytes: " and the text of the FIRST failing relation in the order above.  The weights:
 * 32 bytes from the operating system (getrandom(2)) per call, expanded on the device by ChaCha12 (block counter = weight index); the
 * key's bytes are fixed before the draw, so a false key passes with probability about 2^-128.  A load that gets no random bytes is
 * refused with PM_ERR_STATE.  The sums are MSMs over the plain resident points, two inverse transforms and ONE launch of the 36-lane
 * pairing check (polymath_amd/csrc/key_check.hip; polymath_amd/host/key_check.hpp is the same decision on the CPU).
 * The sentence above stays literally true: validation is on iff (validate & ~256) != 0, so the flag implies point validation -- the
 * relations mean nothing on points outside the subgroup, and a caller passing 512 before the flag existed already got plain
 * validation.  It combines with PM_WIRE_UNCOMPRESSED.  pm_g1_decode ignores it, as it always did.  With shard_count > 1 (or
 * PM_SHARD_VECTOR) the flag is PM_ERR_INVALID_ARG: the check needs whole vectors.  Out of scope: sharded keys; checking a key that is
 * already resident from pm_pk_load; a caller-supplied seed; a vk supplied separately from the key. */
typedef enum pm_key_check { PM_KEY_CHECK_NONE = 0, PM_KEY_CHECK_RELATIONS = 512 } pm_key_check;
/* Batch decode, host to host: `count` packed records of 48 (BLS12-381) / 32 (BN254) bytes -- 96 / 64 with PM_WIRE_UNCOMPRESSED
 * in `validate` -- -> out_xy (x||y Montgomery, 2*fq_limbs
 * u64 per point; infinity and every refused point x = y = 0) and one pm_g1_status byte per point.  PM_OK even when points are bad:
 * the verdicts are in `status`. */
int pm_g1_decode(pm_ctx *ctx, int curve, const uint8_t *in, size_t count, int validate, uint64_t *out_xy, uint8_t *status);
/* The whole ProvingKey::serialize_compressed byte string -> a resident key, as pm_pk_load_sharded would make it (shard_rank /
 * shard_count / layout alike; window tables and the wide mode follow the same way).  The host parses the vk, the SAP header and
 * matrices (canonical Fr) and the six length prefixes; the points go to the device compressed, through pinned staging in chunks
 * of 2^PM_OPT_WIRE_CHUNK_LOG, and are decoded straight into the resident base array: no decoded point crosses the bus.  On a
 * sharded key only this rank's resident ranges are copied and checked.  `bytes` may be an mmap of the key file; it is only read.
 * The VerifyingKey is the byte prefix (data_structures.rs:56-58: vk is the first field): 392 bytes on BLS12-381, 280 on BN254 --
 * its points are always validated (host).  PM_ERR_INVALID_ARG, no handle, nothing allocated: truncated or trailing bytes, a vector
 * length that does not fit the key's shape, vk.m0 / n / sigma / omega disagreeing with the SAP matrices, or a refused point --
 * pm_last_error then names the first one in wire order, e.g. "x_powers_g1[17]: G1: not in the prime-order subgroup".
 * validate | PM_WIRE_UNCOMPRESSED: the bytes are ProvingKey::serialize_uncompressed (vk prefix 728 / 504 bytes); staging slots
 * hold 2^PM_OPT_WIRE_CHUNK_LOG records of 96 / 64 bytes -- the option keeps counting points. */
int pm_pk_load_bytes(pm_ctx *ctx, int curve, const uint8_t *bytes, size_t len, int validate, int shard_rank, int shard_count,
                     int layout, pm_pk **out);
/* pm_pk_export_bases, compressed: `len` records of 48 / 32 bytes (ser_g1, the encoding pm_pk_load_bytes reads) into out.
 * Same ranges and restrictions as pm_pk_export_bases.  which | PM_WIRE_UNCOMPRESSED: records of 96 / 64 bytes
 * (ser_g1_uncompressed).  Any other high bit, or (which & 255) >= PM_NUM_BASE_VECS, is PM_ERR_INVALID_ARG. */
int pm_pk_export_bases_compressed(pm_ctx *ctx, const pm_pk *pk, int which, size_t offset, size_t len, uint8_t *out);

/* ---- prove: create_proof_with_assignment split at its two transcript calls ---------------- */
/* Fiat-Shamir choices of the reference (src/transcript/{merlin,keccak256,blake3}.rs) for pm_host_prove. */
typedef enum pm_transcript { PM_TRANSCRIPT_MERLIN = 0, PM_TRANSCRIPT_KECCAK256 = 1, PM_TRANSCRIPT_BLAKE3 = 2 } pm_transcript;
/* Phase 1 (prover.rs:75-123): witness map, iNTTs, u^2, h, then [a]_1 and [c]_1.
 *   x   : m0 Fr, instance assignment INCLUDING the leading one (prover.rs:56)
 *   w   : mw Fr, witness assignment
 *   r_a : 2 Fr, the two F::rand draws of prover.rs:110 (constant term first) -- an input so
 *         the RNG stays with the caller.
 * On a PM_SHARD_PAIRS key the outputs are this shard's PARTIAL sums; combine with pm_g1_sum (pm_comm_combine_points).
 * On a PM_SHARD_VECTOR key they are already the sums over all ranks: each phase ends with ONE small exchange that carries
 * the ranks' status flags, partial points and (phase 1) the block-boundary coefficients the division needs, so every rank
 * returns the same points and the same status.  With HOST x, w a PM_SHARD_VECTOR rank uploads only its 1/shard_count slice
 * of w and the communicator's device all-gather delivers the rest.
 * On a non-zero status the output points are UNDEFINED (the [a]_1 MSM may already have run when the witness check
 * fails: it overlaps the transforms). */
int pm_prove_phase1(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, const uint64_t *r_a,
                    uint64_t *a_g1_xy, int *a_inf, uint64_t *c_g1_xy, int *c_inf);
/* Same with the assignment ALREADY RESIDENT in HBM: d_x (m0 Fr) and d_w (mw Fr) are device pointers (e.g. the
 * output of a GPU witness generator); r_a stays a host pointer (2 Fr). */
int pm_prove_phase1_device(pm_ctx *ctx, const pm_pk *pk, const uint64_t *d_x, const uint64_t *d_w, const uint64_t *r_a,
                           uint64_t *a_g1_xy, int *a_inf, uint64_t *c_g1_xy, int *c_inf);
/* Phase 2 (prover.rs:132): u(x1), the only O(n) part of a_at_x1; the caller adds r_a(x1)*y1^alpha. */
int pm_prove_phase2(pm_ctx *ctx, const uint64_t *x1, uint64_t *u_at_x1);
/* Phase 3 (prover.rs:142-229): assemble the Y^-gamma-scaled numerator, divide by (X - x1),
 * commit the dense quotient: [d]_1.  Returns PM_ERR_REMAINDER_NONZERO like prover.rs:221.
 * On a PM_SHARD_VECTOR key x1 must be the x1 of phase 2 (the x1-dependent sums of the division scan were exchanged there);
 * another value returns PM_ERR_INVALID_ARG. */
int pm_prove_phase3(pm_ctx *ctx, const uint64_t *x1, const uint64_t *x2, const uint64_t *a_at_x1,
                    const uint64_t *c_at_x1, uint64_t *d_g1_xy, int *d_inf);

/* ---- partial assignments: flags of the `assignment_on_device` argument -----------------------------------------------------
 * pm_host_prove, pm_host_prove_batch, pm_r1cs_check and pm_r1cs_check_batch read `assignment_on_device` as a flag word (flags of an
 * existing argument: the set of entry points and the option table are pinned).  0 and 1 mean what they always meant; a bit outside
 * the two below is PM_ERR_INVALID_ARG.  The other entry points with such an argument (pm_host_prove_sharded, the phases) do not solve.
 *   PM_ASSIGNMENT_SOLVE: the caller supplies only the values it chooses; every Fr of x or w whose four words are UINT64_MAX (>= r on
 *     both curves, so never a field element; or the quotient marker, which differs in the lowest bit: "a division row" below; or
 *     the indicator marker, which differs in bit 64: "an indicator row" below; or the square-root marker, which differs in bit 192:
 *     "a square-root row" below) is
 *     UNKNOWN and is computed on the device first, by forward propagation through the key's
 *     resident constraint rows (first-entry rule applied, as the prover and pm_r1cs_check read them; a stored entry with a zero
 *     coefficient names no variable).  The call then runs on the completed assignment and its results are, bit for bit, those of the
 *     same call without the flag on that assignment.  instance_host of the prove calls uses the same marker: unknown public inputs are
 *     replaced by the solved values before they are hashed.  Without the flag nothing looks for markers.  The caller's arrays are
 *     never written, on host or device: the completed assignment lives in memory of the context.
 *   The rule.  Rows are visited once, in matrix order; a system that this pass refuses is then looked at in ANY ROW ORDER (below).
 *   At row r, among the non-zero entries of A_r, B_r, C_r:
 *     no unknown column                       -- a check row, skipped
 *     one unknown u, in exactly one of them   -- z_u = (Az Bz - C_rest) / coef   (u in C)
 *                                                z_u = (Cz / Bz - A_rest) / coef (u in A; u in B alike with Az), and u is known from here on
 *     a booleanity row                        -- the only unknown is u, C_r has no non-zero entry and {A_r, B_r} = {k z_u, k' (1 - z_u)} in
 *                                                either order, k, k' != 0: one side is the single entry (k, u), the other exactly the two
 *                                                entries (k', column 0) and (-k', u).  It marks u BOOLEAN-PENDING and is otherwise a check row
 *     a decomposition row                     -- k >= 2 unknowns, all boolean-pending, all in the same one of A, B, C and in neither of the
 *                                                others, with coefficients c 2^0 ... c 2^(k-1), each exactly once in any stored order, c != 0,
 *                                                k <= bitlength(r) - 1 (254 on BLS12-381's Fr, 253 on BN254's: the solution is then unique).
 *                                                ONE step for all k columns: t = the ordinary formula of that matrix with the k entries left
 *                                                out and coef = c; z_{u_i} = bit i of the canonical integer of t, as field 0 or field 1
 *     a division row                          -- ONE row with two fresh unknowns q (the quotient) and rem (the remainder), each named once,
 *                                                where the caller marks q with PM_UNKNOWN_QUOTIENT_WORDS (below) instead of the plain
 *                                                marker: circom's  q <-- a \ b; rem <-- a % b; q*b + rem === a , arkworks' DIV / REM and
 *                                                reductions by a non-power-of-two modulus.  One of A_r, B_r has (cq, q) as its only non-zero
 *                                                entry, the other is the known divisor side K (no unknown, not zero), C_r names rem with
 *                                                coefficient -cq beside any known rest R.  ONE step for both columns; with d = K z and
 *                                                a = R / cq read as canonical integers below r:
 *                                                  d != 0:  q = floor(a / d),  rem = a mod d   (q d + rem = a in the integers, so the row
 *                                                           holds; a 256-bit integer division per row and assignment)
 *                                                  d == 0:  the assignment is STUCK at row r
 *                                                The marker is explicit, as circom's <-- is: the row has the shape of an is-zero opener and
 *                                                nothing is inferred -- with the plain marker on q it is an opener, as it always was.  The
 *                                                quotient marker has meaning in that position only: a column that carries it and is the
 *                                                single unknown of an ordinary row is solved by that row, and named anywhere else it is a
 *                                                plain unknown.  Such a row is never an opener and waits for no closer.  A row with two or
 *                                                more unknowns whose quotient-marked column is the lone entry of A_r or B_r and which misses
 *                                                a condition is unsolvable; pm_last_error says which after ", and no division row: "
 *                                                (cr != -cq; rem in A or B; rem named twice; the other side not known; the quotient named
 *                                                twice; a third unknown).  The range checks that make the Euclidean pair the row's ONLY
 *                                                solution (rem < d, and q small enough that q d + rem does not wrap) are the circuit's: they
 *                                                are decomposition rows like any other.  Not handled: signed division, cr != -cq, a known
 *                                                rest beside q on its side, a division without the marker
 *     an indicator row                        -- ONE row whose only unknown u the caller marks with PM_HINT_INDICATOR_WORDS (below) and which
 *                                                names u exactly once, as the ONLY non-zero entry (k, u) of A_r or B_r; the other of the
 *                                                two is the known guard side K (no unknown, not zero) and C_r has no non-zero entry:
 *                                                circomlib's Decoder / Multiplexer,  out[i] <-- (inp == i) ? 1 : 0; out[i] * (inp - i) === 0 ,
 *                                                which is how a circuit reads table[idx] with a signal as the index.  ONE step:
 *                                                  z_u = 1 where K z == 0, else 0      (field one or field zero, whatever k is)
 *                                                The step never divides and never leaves an assignment stuck.  The rows do not determine
 *                                                the value at the hit (0 satisfies the guard too, and the sum row with success = 0), so it
 *                                                is a hint and the marker is explicit, as circom's <-- is: nothing is inferred -- with the
 *                                                plain marker on u the row is an ordinary dividing row, as it always was, and the
 *                                                assignment is stuck at it where K z == 0.  The indicator marker has meaning in that
 *                                                position only: a column that carries it and is the single unknown of a row of any other
 *                                                shape (C_r not empty, other non-zero entries beside u on its side, an empty other side)
 *                                                is solved by that row as an ordinary row, and named beside other unknowns it is a plain
 *                                                unknown; no refusal is added.  Not handled: a hit value other than 1, a non-empty C_r,
 *                                                a known rest beside u, inferring indicators without the marker, sharded keys,
 *                                                per-assignment patterns
 *     a square-root row                       -- ONE row whose only unknown u the caller marks with PM_HINT_SQRT_MARKER (below) and which names
 *                                                u exactly twice: as the ONLY non-zero entry (ka, u) of A_r and as the ONLY non-zero entry
 *                                                (kb, u) of B_r.  C_r names no unknown and does not name u; it may be empty.  (Stored zero
 *                                                coefficients name nothing, as everywhere.)  circom's  x <-- sqrt(u); x*x === u  (circomlib's
 *                                                pointbits.circom, Bits2Point_Strict) and arkworks' sqrt witness in point decompression.
 *                                                ONE step; with c = (C z)_r / (ka kb):
 *                                                  c a square, 0 included:  z_u = the root whose canonical integer is the smaller of the
 *                                                                           pair, <= (r - 1) / 2: what circom's sqrt returns
 *                                                  c a non-residue:         the assignment is STUCK at row r (zero is stored)
 *                                                a Tonelli-Shanks of fixed trip count per row and assignment.  The rows do not determine the
 *                                                value (-u satisfies them too), so it is a hint and the marker is explicit, as circom's <--
 *                                                is: nothing is inferred -- with the plain marker on u the row is refused in matrix order
 *                                                and waits, in any order, for a row that determines u, as it always did; no plan, message or
 *                                                word changes and no refusal is added.  The square-root marker has meaning in that position
 *                                                only: a column that carries it and is the single unknown of an ordinary row, named once,
 *                                                is solved by that row, and named beside other unknowns it is a plain unknown.  In any row
 *                                                order such a row waits on the unknowns of C_r like any other row and acts when u is the
 *                                                only one left.  Not handled: a known rest beside u on either side ((u + k)(u + k) = c),
 *                                                u in C_r (a general quadratic), the larger root or arkworks' unspecified choice of root (a
 *                                                caller who wants either supplies u itself), inferring a square root without the marker,
 *                                                sharded keys, per-assignment patterns
 *     an is-zero pair                         -- the two rows every equality test compiles to, with two fresh unknowns m (the multiplier)
 *                                                and b (the flag):  arkworks  (a - b) mult = neq ; (a - b) (1 - neq) = 0
 *                                                                   circom    (-in) inv = out - 1 ; in out = 0
 *                                                The opener r1 has exactly these two unknowns, each once: one of A_r1, B_r1 is the known side
 *                                                K1 (no unknown, not zero), the other has (cm, m) as its only non-zero entry, C_r1 names b with
 *                                                coefficient cb beside any known rest.  The closer r2 is the FIRST later row that names m or b:
 *                                                it names b and not m, b is its only unknown, in exactly one of A_r2, B_r2 (coefficient kb
 *                                                beside any known rest) and not in C_r2, and the other of A_r2, B_r2 is K2 = K1 or -K1: the
 *                                                same non-zero (column, coefficient) entries in any stored order, or every one negated.  Any
 *                                                number of openers may be open at once.  ONE step for both columns, with d = K1 z:
 *                                                  d != 0:  b = ((C_r2 z) / (K2 z) - rest_r2) / kb,  m = ((C_r1 z, with b) / d) / cm
 *                                                  d == 0:  b = -C_r1_rest / cb,  m = 0
 *                                                Where d == 0 every m satisfies both rows; the library fixes m = 0 (circom's convention, and
 *                                                what d^(r-2) gives).  A caller that wants another value (arkworks' witness generation
 *                                                writes 1) supplies m itself: only b is unknown then and r1 is an ordinary row.  The step
 *                                                never leaves an assignment stuck; if d == 0 and C_r2 z != 0 the closer is a failing row like
 *                                                any other (the check reports it, the prover returns PM_ERR_REMAINDER_NONZERO)
 *     anything else                           -- two or more unknowns that are no decomposition and no opener, an opener whose closer is
 *                                                missing or has another shape (the opener's row is named), or one unknown in two of the three in any
 *                                                other shape (u u = ..., a constant other than minus the coefficient, a non-empty C, further
 *                                                entries): unsolvable
 *   A boolean-pending column that is the single unknown of a later ordinary row is solved by that row; its booleanity row is then a
 *   constraint like any other, which the check reports if the value is not 0 or 1.  One that is still pending when the rows end is
 *   unsolvable: its booleanity row (the smallest such row) and column are named.  XOR, AND, rotations and recompositions are ordinary
 *   one-unknown rows, so range checks, comparisons, modular additions and ARX hashes complete, and with the is-zero pair so do
 *   equality tests, selection on equality, table membership and data-dependent branches.  (Table membership in the arkworks form,
 *   one is-zero pair per index.  circomlib's one-hot Decoder / Multiplexer completes through its indicator rows, with the indicator
 *   marker on its outputs.)
 *   Rows in any order.  Where the pass in matrix order refuses, a waiting-row scheduler applies the same rules in DEPENDENCY order: it
 *   examines the rows smallest first, and a row that cannot act yet WAITS on its unknown columns and is examined again when one of
 *   them becomes known or boolean-pending -- a row with two or more unknowns that is no decomposition and no opener, a decomposition
 *   row before its booleanity rows, one unknown named twice in a shape that is no booleanity row (a later row may determine it: this
 *   one is a check row then), and a row that names a pending pair's multiplier or flag beside something else.  A row whose only
 *   unknown is a pending flag is that pair's closer or, in any other shape, a refusal as in matrix order; a row whose only unknown
 *   is a pending multiplier, named once, determines it as an ordinary row (the opener was none and is examined again).  An R1CS
 *   assembled from parts, booleanity rows emitted after the recomposition, a row-sorted matrix file and a system with its assertion
 *   first all complete this way, with the values the rows in dependency order give.  If no order solves the system the error is the
 *   matrix-order pass's -- same row, column and text -- with "; in any row order: ..." and what stays unknown appended.  Not solved,
 *   in any order: a closer examined before its opener (it is an ordinary dividing row then and sticks where the tested value is 0),
 *   K2 = lambda K1 for other lambda, a known rest beside m in the opener, bits spread over two matrices, signed or non-binary digits,
 *   per-assignment patterns, sharded keys.
 *   Linear blocks (the scheduler only).  k >= 2 rows whose unknowns are the SAME k columns, each named in C_r only (A_r and B_r name
 *   no unknown; either may be empty, the product is then 0), none of them boolean- or pair-pending, and which no rule above claims,
 *   are a square linear system in those columns whose matrix is part of the key: the shape of non-native multiplication
 *   (ark-r1cs-std's mul_without_reduce, circom-bigint's BigMultNoCarry), which pins the 2l - 1 limbs of a product by evaluating
 *   (sum a_i c^i)(sum b_i c^i) = sum p_j c^j  at 2l - 1 points c.  No row order propagates through such rows; they WAIT, and when the
 *   k-th row over exactly the same set has been examined, with k <= 64, the k rows are ONE step for all k columns:
 *   z_S = M^-1 (A z B z - C_known z), M[i][j] = the coefficient of column S_j in row r_i.  The rows determine the values, so there is no
 *   marker and no hint (the quotient, indicator and square-root markers on such a column are plain unknowns there).  The library
 *   inverts every distinct M once per plan on the host -- blocks whose k^2 coefficients are equal word for word share one inverse --
 *   so the step never divides and never leaves an assignment stuck.  A column of the set that another row determines first shrinks
 *   the set (a row at the point 0,  a_0 b_0 = p_0 , is an ordinary row and the others a system in 2l - 2 columns); further rows over
 *   the set are check rows.  A singular M is PM_ERR_INVALID_ARG before any assignment is touched: "rows r_1, ..., r_k: the linear
 *   block over columns ... is singular (no pivot in column S_j)", for the block of smallest first row.  More than 64 unknowns wait to
 *   the end, and the refusal then ends ", and no linear block: k unknowns exceed 64"; fewer than k such rows is the refusal it always
 *   was.  Not handled: an unknown in A_r or B_r (the matrix would depend on the assignment), rows over different sets (banded or
 *   triangular systems), k > 64, boolean- or pair-pending columns in the set, an independent subset of dependent rows, sharded keys,
 *   per-assignment patterns.
 *   Declared hints (the scheduler only; pm_pk_set_hints above, beside pm_pk_free, states the declaration).  The quotient and remainder LIMBS of a
 *   non-native reduction -- circom-bigint's BigMod / BigMultModP (div[i] <-- long_div(..)), ark-r1cs-std's non-native reduce -- are
 *   multi-word integers that no row determines: the limb equations are underdetermined, uniqueness comes from the range checks, and
 *   which rows name them differs per compiler, so there is no shape to recognise and no marker that could say "these 8 columns are
 *   divmod of those 11".  The key DECLARES them instead: a hint PM_HINT_LONGDIV with limb width n names kq quotient columns, kr
 *   remainder columns, kD dividend columns and kE divisor columns (or kE literal limbs).  In a call the hint is ACTIVE when all its
 *   outputs carry PM_UNKNOWN_WORDS, INERT when all are given (the caller supplied q and rem; everything is as without the
 *   declaration), and the call is refused, naming the hint, when some are marked and some given or one carries another marker.  An
 *   output of an active hint is solved by no row: rows that name it wait, the hint waits for its inputs like a row, and when the last
 *   is known it is ONE step: with int(v) the canonical integer of a field element, D = sum_j int(z_{D_j}) 2^(n j) and
 *   E = sum_j int(z_{E_j}) 2^(n j) (limbs need not be normalised: the overflowing limbs of a no-carry product are the intended
 *   dividend), it stores the kq n-bit limbs of floor(D / E) and the kr n-bit limbs of D mod E.  The assignment is STUCK, with zero in
 *   every output, where E = 0, D >= 2^1024, E >= 2^512, q >= 2^(n kq) or rem >= 2^(n kr); the stuck word of hint h (its index in the
 *   declaration) is nr + h, a value no row has, and the root-cause rule below applies to it with its dependency level:
 *   pm_r1cs_check reports it in rows[i][0].  A hint that never becomes ready is refused as "hint h: input column c is never
 *   determined", followed by what stays unknown.  With an active hint every refusal of the structure is reported from the scheduler,
 *   as "column j stays unknown" with its reason: the row that the matrix-order pass would have named (a row with two or more
 *   unknowns, an unknown in two matrices) is not named then, because no matrix order is tried.  Without a declaration, or with every hint inert, plans, messages and words are what
 *   they are without this rule.  Not handled by a long division: other opcodes (modular inverse, gcd, sorting), signed limbs, dividends beyond 1024 bits
 *   (RSA-2048), hints on sharded keys, per-assignment declarations, inferring a hint from rows.
 *   Declared hints: modular division.  Modular inverse and division have their own record, PM_HINT_MODDIV (pm_pk_set_hints above states
 *   it): Z = (N+ - N-) (D+ - D-)^-1 mod P is a value that every gadget on non-native arithmetic contains -- the slope of an affine
 *   point addition, a non-native inverse -- and that no row determines: the circuit only checks Z D = N (mod P) afterwards, through
 *   the product and the long division above.  The ACTIVE / INERT / mixed-marker rule is the long-division one, applied to the kz
 *   outputs; the hint waits for its input columns and is ONE step at 1 + the largest level of its inputs, after the long divisions of
 *   that level.  The assignment is STUCK at the word nr + h, with zero in every output, where P is even or P < 3, P >= 2^512, any of
 *   N+, N-, D+, D- is >= 2^1024, gcd(D mod P, P) != 1 (D = 0 mod P included: a missing inverse is detected, not assumed away), or
 *   Z >= 2^(n kz); the root-cause rule applies to that word as to a long division's.  Without an active modular hint every plan,
 *   message and word is what it is without this rule.  Not handled: even moduli, operands beyond 1024 bits, the slope of a doubling
 *   as one hint, gcd, sorting.
 *   Declared hints: wide long division.  Dividends beyond 1024 bits have their own record, PM_HINT_LONGDIV_WIDE (pm_pk_set_hints above
 *   states it): the quotient and remainder limbs of a reduction modulo an RSA-2048 modulus, which range checks fix and no row
 *   determines.  The rules are the long-division rules unchanged -- ACTIVE / INERT / mixed-marker, HINT-OWNED outputs, waiting on
 *   inputs, the never-ready refusal -- and the hint is ONE step at 1 + the largest level of its inputs, after the modular divisions of
 *   that level, computed by one wave.  The assignment is STUCK at the word nr + h, with zero in every output, where E = 0,
 *   D >= 2^8192, E >= 2^4096, q >= 2^(n kq) or rem >= 2^(n kr); the root-cause rule applies to that word as to a long division's.
 *   Without an active wide hint every plan, message and word is what it is without this rule.  Not handled: modular division at these
 *   widths, even moduli, linear blocks beyond 64 unknowns (RSA-4096 at 64-bit limbs), hints on sharded keys, per-assignment
 *   declarations, gcd, sorting.
 *   Declared hints: modular multiply-divide.  The slope of a DOUBLING has its own record, PM_HINT_MODMULDIV (pm_pk_set_hints above
 *   states it): the tangent's slope 3 X^2 / (2 Y) mod p has a product for its numerator, which PM_HINT_MODDIV's column lists cannot
 *   express unless the circuit happens to carry 3 X^2 as columns, and a key's rows are fixed by its verifying key.  With it ECDSA
 *   verification completes: s^-1, h / s and r / s by opcode 3, the scalars' bits by decomposition rows, the conditional additions by
 *   ordinary rows, the reductions by opcode 1 and the linear blocks.  The rules are the modular hint's -- ACTIVE / INERT /
 *   mixed-marker, HINT-OWNED outputs, waiting on inputs, the never-ready refusal -- applied to the kz outputs, and the hint is ONE step
 *   at 1 + the largest level of its inputs, after the wide long divisions of that level.  The assignment is STUCK at the word nr + h,
 *   with zero in every output, where P is even or P < 3, P >= 2^512, any of the six list sums is >= 2^1024,
 *   gcd(cD D mod P, P) != 1 (D = 0 mod P included, and a cD that shares a factor with a composite P), or Z >= 2^(n kz) -- and in no
 *   other case: the literals scale residues, after the reductions.  Without an active multiply-divide hint every plan, message and
 *   word is what it is without this rule.  Not handled: complete addition formulas, windowed or GLV scalar multiplication, operands
 *   beyond 1024 bits, even moduli, hints on sharded keys, per-assignment declarations.
 *   PM_ERR_INVALID_ARG, pm_last_error naming the row or column, nothing computed and no output written: an unsolvable row, a marked
 *   column that no row determines, a marker at column 0, a sharded key, and -- in a batch -- an assignment that does not mark the
 *   columns assignment 0 marks, or marks one with the other marker (any two of the four markers differ; the first differing (assignment, column) is named; a kernel
 *   compares them).
 *   At run time a step that would divide by zero (Bz = 0 with u in A) leaves that assignment STUCK, even where Cz = 0 too (the value
 *   is then undetermined), and so does a decomposition whose t is 2^k or more (no boolean solution; its k values are stored as
 *   zero) and a division row whose divisor is zero (both values are stored as zero) and a square-root row whose value is a non-residue (zero is stored): its other solved values are undefined, its neighbours are not affected, and its smallest stuck row is
 *   reported (a 64-bit atomic minimum: the same word on every run, since everything downstream of a stuck row has a larger index).
 *   Where the rows were reordered that is not so -- a row that reads the stored zero may stick too, at a smaller index -- and the row
 *   reported is the ROOT CAUSE: among the stuck rows the one of lowest dependency level, then smallest index, which read only valid
 *   values:
 *     pm_r1cs_check[_batch]   n_bad[i] = UINT64_MAX, rows[i][0] = the stuck row (max_rows > 0), the other slots UINT64_MAX, abc zero
 *     pm_host_prove_batch     status[i] = PM_ERR_INVALID_ARG, zeroed bytes
 *     pm_host_prove           returns PM_ERR_INVALID_ARG
 *   Assignments are solved in the groups the call runs in anyway; the results are the same words under every grouping.  The solving
 *   plan (steps, dependency levels, launch schedule, inverses of the coefficients) is kept by the context for ONE (key, pattern) and
 *   rebuilt when either differs; it is freed with the context.  pm_prove_tap 9 and 10 read the results back.
 *   pm_last_timings: after a check call slot 1 holds the GPU ms of the solve kernels (slot 0: the check kernels, as without the flag);
 *   in the prove calls they are added to slot 0, which carries the witness map. */
typedef enum pm_assignment_flags {
    PM_ASSIGNMENT_DEVICE = 1,   /* x, w are device pointers (what "non-zero" has meant) */
    PM_ASSIGNMENT_SOLVE = 2     /* entries equal to the unknown marker are solved first */
} pm_assignment_flags;
/* The two markers of PM_ASSIGNMENT_SOLVE, as initialisers of a uint64_t[4] (little-endian words of one Fr).  Both are >= r on both
 * curves, so neither is ever a field element.  PM_UNKNOWN_WORDS: the value is unknown.  PM_UNKNOWN_QUOTIENT_WORDS: the value is
 * unknown, and it is the Euclidean quotient of its division row (the rule above); everywhere else it means what PM_UNKNOWN_WORDS means.
 * A third marker, PM_HINT_INDICATOR_WORDS (2^256 - 1 - 2^64: the top word is all ones, so it is >= r on both curves as well): the
 * value is unknown, and it is the INDICATOR of its guard row ("an indicator row" above), 1 where the guard's known side is zero,
 * else 0; everywhere else it means what PM_UNKNOWN_WORDS means.  A value with both bit 0 and bit 64 clear is no marker.
 * A fourth marker, PM_HINT_SQRT_MARKER (2^256 - 1 - 2^192: the top word is 0xFFFF...FE, so it is >= r on both curves as well): the
 * value is unknown, and it is the SMALLER SQUARE ROOT of its square-root row ("a square-root row" above), the root whose canonical
 * integer is <= (r - 1) / 2; everywhere else it means what PM_UNKNOWN_WORDS means.  Exactly one of the bits 0, 64 and 192 may be
 * clear: a value that clears bit 192 together with bit 0 or bit 64 is no marker. */
#define PM_UNKNOWN_WORDS { UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT64_MAX }
#define PM_UNKNOWN_QUOTIENT_WORDS { UINT64_MAX - 1, UINT64_MAX, UINT64_MAX, UINT64_MAX }
#define PM_HINT_INDICATOR_WORDS { UINT64_MAX, UINT64_MAX - 1, UINT64_MAX, UINT64_MAX }
#define PM_HINT_SQRT_MARKER { UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT64_MAX - 1 }

/* Whole create_proof_with_assignment (prover.rs:66-237) for an UNSHARDED key, transcript included: the three
 * phases above plus the host glue between them (compute_x1 / compute_x2, common.rs:21-71; pi and c at x1,
 * :73-98; transcript = pm_transcript), run by the library's own C++ mirror of that glue.  For hosts without a
 * Transcript implementation of their own; a Rust host keeps calling the phases and owns T.
 * instance_host: the m0 public inputs (leading one included) as host Montgomery limbs -- they are hashed;
 * x, w: the assignment, host pointers or (assignment_on_device != 0) device pointers as in
 * pm_prove_phase1_device.  proof_bytes receives Proof::serialize_compressed (data_structures.rs:10-19):
 * 176 bytes on BLS12-381, 128 on BN254.  Status codes as for the phases.  transcript must be a pm_transcript, 0 .. 2: the
 * pm_prove_glue flag below belongs to pm_host_prove_batch alone -- pm_host_prove, pm_host_prove_sharded and the verify entry points
 * refuse it like any other value (PM_ERR_INVALID_ARG). */
int pm_host_prove(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x,
                  const uint64_t *w, int assignment_on_device, const uint64_t *r_a, uint8_t *proof_bytes, size_t capacity,
                  size_t *proof_len);

/* `count` runs of create_proof_with_assignment (prover.rs:66-237) against ONE unsharded key, transcript included.
 *   instance_host : count x m0 Fr, host, Montgomery, leading one included (hashed), proof after proof
 *   x, w          : count x m0 / count x mw Fr, host pointers or (assignment_on_device != 0) device pointers, row after row
 *   r_a           : count x 2 Fr, host
 *   proofs        : count x proof_len bytes (176 BLS12-381 / 128 BN254), Proof::serialize_compressed of proof i at i * proof_len
 *   status        : count ints, pm_status of proof i
 * The proofs run in GROUPS: every vector of the prover is a [group][len] array on the device, every kernel has the proof as a grid
 * dimension, and the three MSMs of a proof are three batched MSMs per group over the key's plain points (the key's window tables are
 * neither used nor needed).  A group is as many proofs as keep group * (10 n + 22) inside one MSM piece and the group's vectors inside
 * half of the free device memory; the workspace is owned by the context, reused by later calls and KEPT at the size of the largest group
 * seen until pm_ctx_destroy -- after one large batch, device memory that a later pm_pk_generate or key load on the same device could
 * use for window tables stays with this context (use a context of its own for large batches and destroy it to hand the memory
 * back).  A key whose single proof exceeds an MSM piece runs
 * as a loop of pm_host_prove.  For every i with status[i] == PM_OK, proof i is bit for bit what pm_host_prove returns for row i.
 * PM_OK: the batch ran, the per-proof outcomes are in status[] -- a row with an unsatisfied assignment gets the status pm_host_prove
 * returns for it (PM_ERR_REMAINDER_NONZERO / PM_ERR_DEGREE_BOUND) and zeroed bytes, and does not disturb its neighbours.
 * PM_ERR_INVALID_ARG, nothing computed: a sharded key, a key on another device, an unknown transcript, a wrong proof_len, a NULL
 * pointer where one is required.  count == 0 is PM_OK; count == 1 is pm_host_prove.  The context stays usable as before (a proof in
 * flight between pm_prove_phase1 and phase 3 is not disturbed); pm_last_timings reports every slot summed over the batch.
 *
 * transcript = pm_transcript | pm_prove_glue.  transcript & 255 must be a pm_transcript and transcript & ~(255 | 256) zero; anything
 * else is PM_ERR_INVALID_ARG with nothing written.
 *   PM_PROVE_GLUE_HOST (the default): between the three device phases of a group the stream is stopped, the phase's points and
 *     values come to the host and the glue above runs there, proof after proof: about six synchronisations a group.
 *   PM_PROVE_GLUE_DEVICE: the same glue -- both transcript messages, x1, the powers of y1, a(x1), pi(x1), c(x1), x2, the numerator's
 *     constants, the compressed records and the proof's bytes -- runs in three kernels with one lane per proof, and the phases read
 *     their per-proof records from device memory those kernels wrote.  A group goes from its uploads (the assignments, r_a, and
 *     instance_host's rows x m0 x 32 bytes, once) to its proof bytes without the host: ONE device-to-host copy (rows x proof_len
 *     bytes and one status word per proof) and ONE stream synchronisation per group.  (A workspace that has to grow is reallocated
 *     first, which waits for the device: the first call at a shape.)  Under PM_ASSIGNMENT_SOLVE the solver's read-back for tap 9 stays:
 *     one more synchronisation per group, before phase 1.
 *     CONTRACT: for every i the status and the bytes of proof i are bit for bit those of the same call without the flag, refused rows
 *     included (same status, zeroed bytes, neighbours untouched).  The hashed public inputs are instance_host's, as in host mode --
 *     under PM_ASSIGNMENT_SOLVE with their marker entries replaced by the solved values -- not the x row's, should a caller pass
 *     different ones.  With the flag count == 1 runs the group path with one row (it is not forwarded to pm_host_prove).  A key whose
 *     single proof exceeds an MSM piece keeps running as the loop of pm_host_prove, with the host's glue: the bytes are the same, and
 *     such a call leaves no tap 11.  pm_last_timings: the glue kernels' GPU ms are part of slot 2 (poly); the stage timers are read
 *     when pm_last_timings is called, not during the call.  pm_prove_tap(11) returns what the kernels derived. */
typedef enum pm_prove_glue { PM_PROVE_GLUE_HOST = 0, PM_PROVE_GLUE_DEVICE = 256 } pm_prove_glue;
int pm_host_prove_batch(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t count, const uint64_t *instance_host,
                        const uint64_t *x, const uint64_t *w, int assignment_on_device, const uint64_t *r_a,
                        uint8_t *proofs, size_t proof_len, int *status);

/* WHICH constraints an assignment violates: what a caller runs after PM_ERR_REMAINDER_NONZERO (the prover itself only learns that
 * some row fails).  The answer ark-relations' ConstraintSystem::which_is_unsatisfied gives on the host, for `count` assignments
 * against ONE unsharded key, from the key's resident matrices.
 *   x, w      : count x m0 (leading one included) / count x mw Fr, Montgomery, host pointers or (assignment_on_device != 0) device
 *               pointers, row after row, exactly as pm_host_prove_batch takes them; device arrays are read in place
 *   n_bad[i]  : count u64, host: the number of constraint rows r < nr with (A z)_r (B z)_r != (C z)_r for assignment i, under the
 *               first-entry rule the prover applies to a column named twice in a row (common.rs:100-105)
 *   rows      : count x max_rows u64, host: rows[i * max_rows + j], j < min(n_bad[i], max_rows), are the SMALLEST failing row
 *               indices of assignment i in ascending order; the slots after them hold UINT64_MAX.  A row index is the
 *               constraint's position in the matrices the key was made from.  May be NULL only if max_rows == 0 (count only).
 *   abc       : count x max_rows x 12 u64, host, or NULL (then not computed): (A z)_r, (B z)_r, (C z)_r of the row in the same
 *               slot of `rows`, 4 Montgomery limbs each; zero for an unused slot
 * n_bad[i] == 0 exactly when the prover's witness check passes for assignment i: (Az + Bz)^2 = 4 Cz + (Az - Bz)^2 <=> Az Bz = Cz
 * in odd characteristic, and the public-input rows of the square system hold identically.  The outputs are the same words on
 * every run (no atomics), whatever the grouping: assignments run in groups of as many as keep group * (m0 + mw) <=
 * 2^PM_OPT_MSM_MAX_PIECE_LOG (at least one, at most 65 535).
 * count == 0 is PM_OK and writes nothing.  PM_ERR_INVALID_ARG, nothing computed or written: a sharded key, a key on another
 * device, a NULL n_bad, a NULL rows with max_rows > 0, a NULL x, a NULL w with mw > 0.  Device memory is taken per call and
 * returned; the context stays usable and a proof in flight between pm_prove_phase1 and pm_prove_phase3 is not disturbed.
 * pm_last_timings afterwards: slot 0 the GPU ms of the call's kernels, the other slots zero.
 * pm_r1cs_check is pm_r1cs_check_batch with count == 1. */
int pm_r1cs_check(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, int assignment_on_device,
                  size_t max_rows, uint64_t *n_bad, uint64_t *rows, uint64_t *abc);
int pm_r1cs_check_batch(pm_ctx *ctx, const pm_pk *pk, size_t count, const uint64_t *x, const uint64_t *w,
                        int assignment_on_device, size_t max_rows, uint64_t *n_bad, uint64_t *rows, uint64_t *abc);

/* The same on a SHARDED key (one rank of a multi-GPU proof): `combine` is called between the phases with this
 * rank's partial points -- count = 2 ([a]_1, [c]_1) after phase 1, count = 1 ([d]_1) after phase 3 -- and must
 * replace them, in place, by the sums over all ranks (all-gather over RCCL + pm_g1_sum: SURVEY.md §8e; RCCL has
 * no elliptic-curve reduction).  xy: count x (x||y Montgomery, 16*fq_limbs bytes); inf: count flags.  A non-zero
 * return aborts the proof with that status.  Every rank then hashes the same points and returns the same proof.
 * `combine` is for PM_SHARD_PAIRS keys; it is ignored on a PM_SHARD_VECTOR key, whose phases return summed points. */
typedef int (*pm_combine_fn)(void *user, int count, uint64_t *xy, int *inf);
int pm_host_prove_sharded(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x,
                          const uint64_t *w, int assignment_on_device, const uint64_t *r_a, pm_combine_fn combine, void *user,
                          uint8_t *proof_bytes, size_t capacity, size_t *proof_len);

/* Polymath::verify (lib.rs:80-90 -> verify_proof, verifier.rs:19-62) and the VerifyingKey of a key made from the trapdoors
 * (generator.rs:139-157), for hosts without a pairing implementation of their own.  HOST code (the verifier is O(1): two
 * Miller loops and a final exponentiation on the CPU; measured 142.5 ms per proof on BLS12-381, 59.1 ms on BN254, on the MI355X box's
 * host, profiles/verify_batch.txt; many proofs for one key: pm_verify_batch): needs no GPU and no context.  Both pairing engines.
 * vk_bytes: VerifyingKey::serialize_compressed (data_structures.rs:25-52): one_g1, one_g2, x_g2, z_g2, n, m0, sigma, omega --
 * 392 bytes on BLS12-381 (zcash point encoding), 280 on BN254 (ark-serialize's default short-Weierstrass form).
 * public_inputs: n_inputs Fr, Montgomery, WITHOUT the leading one (verifier.rs:26); proof_bytes: Proof::serialize_compressed.
 * Malformed bytes return PM_ERR_INVALID_ARG; otherwise PM_OK with *accepted = 0 / 1. */
int pm_host_make_vk(int curve, uint64_t n, uint64_t m0, uint64_t sigma, const uint64_t *omega, const uint64_t *x_trapdoor,
                    const uint64_t *z_trapdoor, uint8_t *vk_bytes, size_t capacity, size_t *vk_len);
int pm_host_verify(int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                   const uint8_t *proof_bytes, size_t proof_len, int *accepted);

/* ---- batch verification: `count` proofs against ONE verifying key, one verdict each -----------------------------------------
 * The per-proof elliptic-curve work runs on the device (three point decompressions with curve and subgroup checks, four scalar
 * multiplications, a binary tree of sums); the pairings stay on the host, a handful per batch.  With x1_i, x2_i, c_i(x1_i) of
 * proof i as verify_proof computes them (verifier.rs:24-42), s_i = a_at_x1_i + x2_i c_i(x1_i) and weights rho_i,
 *     U_i = rho_i A_i + (rho_i x2_i) C_i      V_i = rho_i D_i      W_i = (rho_i x1_i) D_i      g_i = rho_i s_i,
 * a set S of proofs passes iff   e(U_S - g_S G, [z]_2) e(-V_S, [x]_2) e(W_S, [1]_2) = 1   (sums over S; three Miller loops, one final
 * exponentiation).  For one proof this IS the reference's equation (verifier.rs:44-61, with e(-D, [x]_2 - x1 [1]_2) split so that
 * every G2 argument belongs to the key), so a verdict reached on a single proof is exact.  A set of valid proofs always passes; a
 * set that passes holds only valid proofs except with probability ~2^-128 over the weights -- every point has been put into the
 * prime-order group by the decoder first.  The weights are 128-bit outputs of ChaCha12 keyed with
 *     Keccak256("polymath-verify-batch" || seed32 (32 zero bytes if NULL) || vk || transcript id || all inputs || all proof bytes):
 * they are bound to the batch, so whoever chose the proofs could not choose them to cancel under the weights, whether the seed is
 * secret, public or absent.  A caller who wants verdicts nobody else can predict passes 32 random bytes.
 * The root (all proofs) is checked first: ONE check when everything is valid.  Otherwise, with verdicts != NULL, the call bisects
 * over the device's sum tree; when a node fails and its left child passes, the right child is known to fail without a check.
 * With f proofs REJECTED:  *n_checks <= 1 + 2 f ceil(log2 count);  with verdicts == NULL:  *n_checks <= 1.
 *   public_inputs : count x n_inputs Fr, Montgomery, WITHOUT the leading one (as pm_host_verify), proof after proof
 *   proofs        : count packed Proof::serialize_compressed records of proof_len = 176 (BLS12-381) / 128 (BN254) bytes
 *   verdicts      : count bytes of pm_verify_verdict, or NULL for *all_accepted only
 *   *all_accepted : 1 iff every proof is PM_VERIFY_ACCEPTED (count == 0: 1, with *n_checks = 0)
 * PM_ERR_INVALID_ARG, nothing computed: a malformed vk, another proof_len, an unknown curve or transcript, count > 2^20.
 * Device and host memory are taken per call and returned.  pm_last_timings afterwards: slot 0 the decode kernel, 1 the terms kernel,
 * 2 the tree kernels, 7 the device part as a whole up to the tree (GPU ms); 3 the host's per-proof glue, 4 the pairing checks (wall ms). */
typedef enum pm_verify_verdict {
    PM_VERIFY_REJECTED = 0,
    PM_VERIFY_ACCEPTED = 1,
    PM_VERIFY_MALFORMED = 2   /* the bytes pm_host_verify answers with PM_ERR_INVALID_ARG: a point whose pm_g1_status is not PM_G1_OK, a_at_x1 >= r */
} pm_verify_verdict;
int pm_verify_batch(pm_ctx *ctx, int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                    const uint8_t *proofs, size_t proof_len, size_t count, const uint8_t *seed32, uint8_t *verdicts, int *all_accepted,
                    size_t *n_checks);

/* The same call with the place of the pairing checks chosen.  (An argument, not a pm_option: the option table is part of the ABI that
 * existing hosts compile against.)  pm_verify_batch is pm_verify_batch2 with PM_VERIFY_PAIRING_HOST, bit for bit.
 *   PM_VERIFY_PAIRING_DEVICE: the root is checked by pm_pairing_check_batch's kernel in a launch of ONE lane (the same sums, -g_S G
 *     included: the lane forms it): a valid batch still costs one check.  After a failing root, with verdicts != NULL, ONE launch checks
 *     every live leaf of the sum tree -- U_i - g_i G against [z]_2, -V_i against [x]_2, W_i against [1]_2, the lane forming g_i G, -V_i
 *     and the affine points -- and a leaf's check is exact (above), so there is no bisection:
 *         *n_checks = 1 + the number of proofs that are not PM_VERIFY_MALFORMED;   with verdicts == NULL:  *n_checks <= 1
 *     (host mode: *n_checks <= 1 + 2 f ceil(log2 count)).  Malformed proofs keep PM_VERIFY_MALFORMED and are not checked.
 *   PM_VERIFY_PAIRING_DEVICE_WAVE: PM_VERIFY_PAIRING_DEVICE with each check spread over a group of 36 lanes of one wave instead of one
 *     lane (the same line tables, Miller loop and final exponentiation; -g G summed from a table of G's multiples built once per call).
 *     The root is always checked this way; the leaf launch after a failing root while at most VERIFY_WAVE_LEAF_MAX = 1024 proofs are live
 *     (a wave a leaf), and one lane a leaf above that (a starting value for the threshold, not a tuned one).  Contract: verdicts,
 *     *all_accepted, the weights, the meaning of seed32, *n_checks and every refusal are, byte for byte, PM_VERIFY_PAIRING_DEVICE's.
 * Verdicts, *all_accepted, the weights, the meaning of seed32 and every PM_ERR_INVALID_ARG case are the same in all modes; another
 * `pairing` value (2, 3, 5, .., and 4 with any other low bit) is PM_ERR_INVALID_ARG with nothing written.  pm_last_timings: slot 4 is the pairing checks' wall ms wherever they ran (device mode: line
 * tables, launches and copies), slot 5 the GPU ms of the pairing launches (the device modes only).
 * `pairing` may be OR-ed with a pm_verify_challenges value, the place of the per-proof challenges (a flag of this argument: the set of
 * entry points is pinned like the option table).  PM_VERIFY_CHALLENGES_HOST (0) changes nothing, bit for bit.
 *   PM_VERIFY_CHALLENGES_DEVICE: x1_i, x2_i, c_i(x1_i) (verifier.rs:24-42 with common.rs:21-98: the Fiat-Shamir transcript of
 *     src/transcript/{merlin,keccak256,blake3}.rs, pi(x1) and c(x1)) come from one lane per proof of ONE launch behind the decode, and
 *     the lane goes on to rho_i x2_i, rho_i x1_i and g_i: the proofs and inputs go up once; one byte, g_i and the challenges
 *     (pm_prove_tap, which = 8) come back per proof, and
 *     the host keeps the weights' key and draws, the merge of malformed points, the prefix sums of g_i and the checks.
 * The challenges are the same bits in both modes, hence so are verdicts, *all_accepted, the weights and *n_checks for one seed, under
 * either pairing mode; any other bit in `pairing` is PM_ERR_INVALID_ARG.  pm_last_timings: slot 6 is the GPU ms of the challenge launch
 * (0 with host challenges); slot 3 stays the host's glue (wall ms), which with device challenges is the weights' key, the draws and
 * the uploads. */
typedef enum pm_verify_pairing { PM_VERIFY_PAIRING_HOST = 0, PM_VERIFY_PAIRING_DEVICE = 1, PM_VERIFY_PAIRING_DEVICE_WAVE = 4 } pm_verify_pairing;
typedef enum pm_verify_challenges { PM_VERIFY_CHALLENGES_HOST = 0, PM_VERIFY_CHALLENGES_DEVICE = 256 } pm_verify_challenges;
int pm_verify_batch2(pm_ctx *ctx, int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                     const uint8_t *proofs, size_t proof_len, size_t count, const uint8_t *seed32, int pairing, uint8_t *verdicts,
                     int *all_accepted, size_t *n_checks);

/* count independent checks  prod_{j<k} e(P[i][j], Q[j]) == 1  against k <= 4 FIXED G2 points, one lane of ONE launch per check.
 * g2: k affine points, x.c0 || x.c1 || y.c0 || y.c1, Montgomery, 4 * fq_limbs u64 each (on the twist, else PM_ERR_INVALID_ARG;
 *     the subgroup is the caller's business, as with msm_unchecked).  g1: count * k points, the G1 affine-in convention
 *     (stride, infinity byte / all-zero), check after check; a pair whose G1 point is infinity contributes 1.  is_one: count bytes, 0 / 1.
 * The pairing is the optimal ate pairing of both engines, with the final exponentiation's hard part by an x-chain (on BLS12-381 it
 * yields the cube of the usual value: 3 does not divide r, so "== 1" is unchanged).  count == 0 returns PM_OK; count <= 2^22.
 * Device and host memory are taken per call and returned.  pm_last_timings slot 7: the GPU ms of the launch. */
int pm_pairing_check_batch(pm_ctx *ctx, int curve, const uint64_t *g2, size_t k, const void *g1, size_t g1_stride,
                           size_t count, uint8_t *is_one);

/* Host helper: Keccak-f[1600] on 25 little-endian lanes, shared by the host mirrors' Merlin / Keccak256
 * transcripts (the reference's transcripts are host code too: src/transcript/ *.rs). */
void pm_host_keccak_f1600(uint64_t state[25]);

/* ---- multi-GPU exchange layer (no reference counterpart: the reference is single-process CPU code) ------
 * One pm_comm per rank.  The sharded prover needs two collectives: an all-to-all of equal DEVICE blocks (the transpose of
 * the four-step NTT, prover.rs:239-243 / 315-328 split over ranks) and an all-gather of small HOST payloads (partial
 * points, status flags, scan carries).  RCCL form: rank 0 calls pm_comm_rccl_unique_id and ships the 128 bytes to the
 * other ranks by any means (the Rust host's own channel, torch.distributed's store, MPI ...); every rank then calls
 * pm_comm_rccl_create (collective: ncclCommInitRank).  librccl is loaded at first use (dlopen): no link-time dependency.
 * Contract: collectives are matched by program order on every rank.  The status checks of the prover itself (unsatisfied
 * witness, degree bounds: prover.rs:107,108,221) are exchanged first and fail on ALL ranks together, with the communicator
 * intact.  Any other failure of one rank (HIP error, out of memory, a dead process) ends the proof on every rank with
 * PM_ERR_COMM instead of a hang: no collective waits longer than the communicator's deadline (pm_comm_set_timeout_ms;
 * PM_COMM_TIMEOUT_MS in the environment; 120 s by default), a failing phase aborts its communicator (pm_comm_abort: the local
 * group wakes its peers at once, RCCL calls ncclCommAbort and the peers run into their deadline), and a failed communicator
 * stays failed -- the host tears the job down and starts again, as with any NCCL / MPI program. */
typedef struct pm_comm pm_comm;
int pm_comm_rccl_unique_id(void *out_128_bytes);
int pm_comm_rccl_create(const void *unique_id_128_bytes, int rank, int world, int device, pm_comm **out);
/* `world` ranks as threads of ONE process (one or several devices): rendezvous + device-to-device copies.  out[world]. */
int pm_comm_local_create(int world, pm_comm **out);
/* The host brings its own transport. */
typedef struct pm_comm_ops {
    void *user;
    /* block p of d_send (bytes_per_peer each) goes to rank p; block p of d_recv comes from rank p; device pointers;
     * must be ordered after the work already enqueued on hip_stream and complete (or be enqueued on it) on return */
    int (*all_to_all)(void *user, const void *d_send, void *d_recv, size_t bytes_per_peer, void *hip_stream);
    /* host pointers; recv holds world x bytes, rank r's block at r * bytes */
    int (*all_gather)(void *user, const void *send, void *recv, size_t bytes);
} pm_comm_ops;
int pm_comm_from_callbacks(const pm_comm_ops *ops, int rank, int world, pm_comm **out);
void pm_comm_destroy(pm_comm *c);
int pm_comm_rank(const pm_comm *c);
int pm_comm_world(const pm_comm *c);
const char *pm_comm_last_error(const pm_comm *c);
/* "rccl" | "local" | "callbacks": which transport a communicator runs on (bench.py reports it). */
const char *pm_comm_kind(const pm_comm *c);
/* Deadline of every collective of this communicator, in milliseconds (> 0). */
int pm_comm_set_timeout_ms(pm_comm *c, long timeout_ms);
/* This rank gives up (`why` goes to pm_comm_last_error of whoever notices): the communicator fails for good. */
int pm_comm_abort(pm_comm *c, const char *why);
/* 1 once the communicator has failed (deadline, peer abort, transport error). */
int pm_comm_failed(const pm_comm *c);
/* Local group only (measurement aid; any handle of the group, before its first collective): on = 1 makes the ranks take
 * turns between collectives, so that N ranks emulated on ONE GPU do not time-slice it -- each rank's kernels then take what
 * they would take alone (tools/shard_emulation.py).  PM_ERR_INVALID_ARG for other transports. */
int pm_comm_local_set_serialize(pm_comm *c, int on);
/* Serialised local group: the milliseconds this rank spent running, waits for its peers excluded; 0 for other communicators. */
double pm_comm_busy_ms(pm_comm *c, int reset);
int pm_comm_all_gather(pm_comm *c, const void *send, void *recv, size_t bytes);
int pm_comm_all_to_all(pm_comm *c, const void *d_send, void *d_recv, size_t bytes_per_peer, void *hip_stream);
/* All-gather of equal DEVICE blocks (rank r's `bytes` at d_recv + r * bytes), stream-ordered: how the sharded prover
 * distributes the assignment -- each rank uploads 1/world of the witness over its own PCIe link (prover.rs:75-80 needs all
 * of it on every rank: "broadcast of assignment"). */
int pm_comm_all_gather_device(pm_comm *c, const void *d_send, void *d_recv, size_t bytes, void *hip_stream);
/* Sum over ranks of `count` partial G1 points, in place (all-gather + pm_g1_sum): the native pm_combine_fn. */
int pm_comm_combine_points(pm_comm *c, int curve, int count, uint64_t *xy, int *inf);
/* Join a context to its rank's communicator.  Required before proving on a PM_SHARD_VECTOR key; with it,
 * pm_host_prove_sharded needs no `combine` callback either.  The context does not own the comm. */
int pm_ctx_set_comm(pm_ctx *ctx, pm_comm *comm);

/* Harness workload (no reference counterpart in src/; benches/bench.rs:38-61 is the reference's own): the synthetic
 * "random A*B=C gates" R1CS of BASELINE.json configs[1..4], generated natively with the same splitmix64
 * draws as polymath_amd/circuits.py: synthetic_r1cs.  m0 = 2, mw = nr + 1, one entry per row in A, B and C, so
 * rowptr = 0..nr is implied.  a_val/b_val/c_val: nr x 4 u64 Montgomery; *_col: nr u32; instance: 2 Fr (one, out);
 * witness: (nr + 1) Fr.  Host code: needs no GPU. */
int pm_synth_r1cs(int curve, uint64_t nr, uint64_t seed, uint64_t *a_val, uint32_t *a_col, uint64_t *b_val, uint32_t *b_col,
                  uint64_t *c_val, uint32_t *c_col, uint64_t *instance, uint64_t *witness);

/* Diagnostic: `products_per_field` seeded products a*b and squares a*a per field (plus p-1, 0, 1 operands), computed on the
 * device the way the kernels do -- the dense reduced-radix product of field.cuh and the internal-radix product of fq28.cuh --
 * and compared word for word with the host's 32-bit CIOS.  mismatches[k]: k = 0 BLS12-381 Fr, 1 BN254 Fr, 2 BLS12-381 Fq,
 * 3 BN254 Fq; all zero on a healthy build.  No reference counterpart: ark-ff's `Fp::mul_assign` is the thing restated. */
int pm_selftest_field(pm_ctx *ctx, size_t products_per_field, uint64_t seed, uint64_t mismatches[4]);

/* Debug / parity taps: copy an intermediate vector of the proof in flight back to the host.
 * which: 0 u_evals(n) 1 w_evals(n) 2 u coeffs(n) 3 w coeffs(n) 4 h coeffs(n) 5 witness-u coeffs(n)
 *        6 z_tail(M-m0) 7 quotient (10n+23)
 *        8 (no proof in flight needed) what the last pm_verify_batch2 with PM_VERIFY_CHALLENGES_DEVICE on this context derived, four
 *          elements a proof: x1, x2, c(x1) (Montgomery) and one whose first word is 1 iff a_at_x1 < r (else the other three are
 *          zero); the point records were hashed as given, whether or not they decode.  PM_ERR_STATE when there is none.
 *        9 (no proof in flight needed) the last call with PM_ASSIGNMENT_SOLVE on this context, 1 + m0 elements per assignment, for all
 *          `count` of them: one whose first word is the assignment's stuck row, UINT64_MAX if it completed, then the m0 completed
 *          instance values (Montgomery; zeros if stuck).  Host memory.  PM_ERR_STATE when there was no such call.
 *       10 (no proof in flight needed) the last pm_r1cs_check[_batch] with PM_ASSIGNMENT_SOLVE: count x (m0 + mw) elements, the completed
 *          x || w rows, assignment after assignment (a stuck one's row is undefined).  PM_ERR_STATE if the last call with the flag was a
 *          prove call (its groups reuse the prover's workspace) or there was none.  The rows stay in a device buffer of the context,
 *          count * (m0 + mw) * 32 bytes, KEPT until the next call with the flag reuses it or pm_ctx_destroy frees it: after one large
 *          batch that memory stays with the context (use a context of its own for large batches and destroy it).
 *       11 (no proof in flight needed) what the last pm_host_prove_batch with PM_PROVE_GLUE_DEVICE on this context derived, four
 *          elements a proof (Montgomery), for all `count` proofs: x1, x2, a(x1), c(x1); a refused row holds zeros.  A device buffer of
 *          the context (count * 128 bytes), kept like tap 10's.  PM_ERR_STATE when there was no such call, or the last one failed or
 *          fell back to the per-proof loop. */
int pm_prove_tap(pm_ctx *ctx, int which, uint64_t *out, size_t max_elems, size_t *n_elems);

#ifdef __cplusplus
}
#endif
#endif /* POLYMATH_HIP_H */
