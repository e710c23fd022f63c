"""ctypes binding of libpolymath_hip.so (include/polymath_hip.h).

This is the Python face of the C ABI: thin, typed wrappers on numpy uint64 limb arrays
(Montgomery form, arkworks' in-memory layout).  There is NO CPU fallback: if the library is
missing or no GPU is present, calls raise.
"""
import ctypes as ct
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# POLYMATH_HIP_LIB: another BUILD of the same library (same-box A/B runs load variants from ab/ through this instead of
# copying them over the in-tree file; tools/README.md).  Still the HIP library: there is no CPU fallback behind it.
LIB_PATH = os.environ.get("POLYMATH_HIP_LIB") or os.path.join(HERE, "libpolymath_hip.so")

PM_BLS12_381, PM_BN254 = 0, 1
CURVE_IDS = {"bls12_381": PM_BLS12_381, "bn254": PM_BN254}
FQ_LIMBS64 = {PM_BLS12_381: 6, PM_BN254: 4}

STATUS = {0: "PM_OK", 1: "PM_ERR_INVALID_ARG", 2: "PM_ERR_LEN_MISMATCH", 3: "PM_ERR_DOMAIN_TOO_LARGE",
          4: "PM_ERR_REMAINDER_NONZERO", 5: "PM_ERR_DEGREE_BOUND", 6: "PM_ERR_HIP", 7: "PM_ERR_NO_DEVICE",
          8: "PM_ERR_STATE", 9: "PM_ERR_COMM"}
(X_POWERS, X_POWERS_Y_ALPHA, X_POWERS_Y_GAMMA, X_POWERS_Y_GAMMA_Z, X_POWERS_ZH_BY_Y_ALPHA,
 UJ_WJ_LCS_BY_Y_ALPHA) = range(6)
# pm_g1_status (include/polymath_hip.h): the verdict of one compressed G1 encoding
G1_OK, G1_BAD_FLAGS, G1_COORD_GE_P, G1_NOT_ON_CURVE, G1_NOT_IN_SUBGROUP, G1_NONCANONICAL_INF, G1_INF_SIGN = range(7)
G1_BYTES = {PM_BLS12_381: 48, PM_BN254: 32}                # compressed record of one point
# pm_wire_form: a flag OR-ed into `validate` (pm_g1_decode, pm_pk_load_bytes) and `which` (pm_pk_export_bases_compressed)
PM_WIRE_COMPRESSED, PM_WIRE_UNCOMPRESSED = 0, 256
WIRE_FORMS = {"compressed": PM_WIRE_COMPRESSED, "uncompressed": PM_WIRE_UNCOMPRESSED}
# pm_key_check: a flag OR-ed into pm_pk_load_bytes' `validate` -- the key's relations against its own vk and matrices (implies validation)
PM_KEY_CHECK_NONE, PM_KEY_CHECK_RELATIONS = 0, 512


def g1_record_bytes(curve_id, form="compressed"):
    """Bytes of one G1 record: 48 / 32 compressed, 96 / 64 uncompressed (x || y)."""
    return G1_BYTES[curve_id] * (2 if WIRE_FORMS[form] else 1)
PROOF_BYTES = {PM_BLS12_381: 176, PM_BN254: 128}            # Proof::serialize_compressed
# pm_verify_verdict (include/polymath_hip.h): one per proof of pm_verify_batch
VERIFY_REJECTED, VERIFY_ACCEPTED, VERIFY_MALFORMED = range(3)
# what pm_last_timings' slots hold after pm_verify_batch (ms: GPU time of the kernels, wall time of the two host parts).  host_pairing is
# the pairing checks' wall time wherever they ran; pairing_kernels the GPU time of the device mode's launches (0 in host mode);
# challenge_kernel the GPU time of the challenge launch (device challenges; else 0)
VERIFY_TIMING_SLOTS = {"decode": 0, "terms": 1, "tree": 2, "host_glue": 3, "host_pairing": 4, "pairing_kernels": 5, "challenge_kernel": 6, "device_total": 7}
# pm_verify_pairing (include/polymath_hip.h): where pm_verify_batch2 runs its pairing checks
VERIFY_PAIRING = {"host": 0, "device": 1, "wave": 4}
# wave mode's leaf launch after a failing root: a wave a leaf while at most this many proofs are live, a lane a leaf above (csrc/internal.h:
# VERIFY_WAVE_LEAF_MAX; a starting value, not a tuned one)
VERIFY_WAVE_LEAF_MAX = 1024
# pm_verify_challenges (include/polymath_hip.h): where the per-proof Fiat-Shamir challenges run; OR-ed into pm_verify_batch2's `pairing`
VERIFY_CHALLENGES = {"host": 0, "device": 256}
PROVE_GLUE_HOST, PROVE_GLUE_DEVICE = 0, 256    # pm_prove_glue: OR-ed into the `transcript` argument of pm_host_prove_batch
PROVE_GLUE = {"host": PROVE_GLUE_HOST, "device": PROVE_GLUE_DEVICE}
# pm_assignment_flags (include/polymath_hip.h): the `assignment_on_device` argument of the check and host-prove calls is a flag word
ASSIGNMENT_DEVICE, ASSIGNMENT_SOLVE = 1, 2
UNKNOWN_LIMBS = (0xFFFFFFFFFFFFFFFF,) * 4     # an Fr of x / w / instance_host with these words is unknown under ASSIGNMENT_SOLVE
QUOTIENT_LIMBS = (0xFFFFFFFFFFFFFFFE,) + (0xFFFFFFFFFFFFFFFF,) * 3     # PM_UNKNOWN_QUOTIENT_WORDS: unknown, and the Euclidean quotient of a division row
INDICATOR_LIMBS = (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)     # PM_HINT_INDICATOR_WORDS: unknown, and the indicator of its guard row
SQRT_LIMBS = (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE)     # PM_HINT_SQRT_MARKER: unknown, and the smaller square root of its square-root row
# the declared hints of the witness solver (include/polymath_hip.h): PM_KEY_HINTS, the flag of pm_pk_load_bytes' `validate` under which
# `bytes` declares the hints of an existing key; the one opcode of a hint, its one flag and the limits of a record
PM_KEY_HINTS = 1024
HINT_LONGDIV, HINT_DIVISOR_LITERAL = 1, 1
HINT_LIMITS = {"n": 128, "kq": 32, "kr": 16, "kD": 32, "kE": 16}
# the second opcode, modular division Z = (N+ - N-) / (D+ - D-) mod P (2 is reserved), its one flag and the limits of its record
HINT_MODDIV, HINT_MODULUS_LITERAL = 3, 1
MODDIV_LIMITS = {"n": 128, "kz": 16, "kNp": 32, "kNm": 32, "kDp": 32, "kDm": 32, "kP": 16}
# the third opcode, the wide long division (4 is refused as unknown): opcode 1's record and flag under limits of its own
HINT_LONGDIV_WIDE = 5
WIDE_LIMITS = {"n": 128, "kq": 128, "kr": 64, "kD": 128, "kE": 64}
# the fourth opcode, the modular multiply-divide cD (D+ - D-) Z = cN (A B + N+ - N-) mod P (6 is refused as unknown): opcode 3's flag,
# the limits of its record; cN and cD are one-word literals in 1 .. 2^32 - 1
HINT_MODMULDIV = 7
MODMULDIV_LIMITS = {"n": 128, "kz": 16, "kA": 32, "kB": 32, "kNp": 32, "kNm": 32, "kDp": 32, "kDm": 32, "kP": 16, "c": 2 ** 32 - 1}
NOT_STUCK = 0xFFFFFFFFFFFFFFFF                # first word of a tap-9 record of an assignment that completed
TIMING_SLOTS = ["witness_map", "ntt", "poly", "msm_sort", "msm_accumulate", "msm_reduce", "msm_total", "phase"]

u64p = ct.POINTER(ct.c_uint64)
u32p = ct.POINTER(ct.c_uint32)
intp = ct.POINTER(ct.c_int)


# pm_combine_fn: int (*)(void *user, int count, uint64_t *xy, int *inf)
COMBINE_FN = ct.CFUNCTYPE(ct.c_int, ct.c_void_p, ct.c_int, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_int))


class PmCsr(ct.Structure):
    _fields_ = [("nrows", ct.c_uint64), ("rowptr", u64p), ("col", u32p), ("val", u64p)]


class PmBaseArray(ct.Structure):
    _fields_ = [("points", ct.c_void_p), ("len", ct.c_size_t), ("stride", ct.c_size_t)]


class PolymathError(RuntimeError):
    def __init__(self, status, detail=""):
        super().__init__("%s (%d) %s" % (STATUS.get(status, "?"), status, detail))
        self.status = status


EXPORTS = [
    "pm_device_count", "pm_ctx_create", "pm_ctx_destroy", "pm_last_error", "pm_last_timings", "pm_ntt",
    "pm_ntt_device", "pm_ntt_batch_device", "pm_msm_g1", "pm_bases_upload", "pm_bases_generate_multiples", "pm_bases_download",
    "pm_bases_precompute", "pm_bases_len", "pm_bases_free", "pm_msm_g1_resident", "pm_msm_g1_resident_batch", "pm_g1_sum", "pm_pk_load", "pm_pk_generate",
    "pm_pk_info", "pm_pk_msm_plan", "pm_pk_export_bases", "pm_pk_free", "pm_prove_phase1", "pm_prove_phase1_device", "pm_prove_phase2", "pm_prove_phase3", "pm_host_prove", "pm_host_prove_batch", "pm_host_prove_sharded",
    "pm_prove_tap", "pm_host_keccak_f1600", "pm_synth_r1cs", "pm_selftest_field",
    "pm_pk_load_sharded", "pm_pk_generate_sharded", "pm_layout_indices", "pm_pk_msm_pieces",
    "pm_comm_rccl_unique_id", "pm_comm_rccl_create", "pm_comm_local_create", "pm_comm_from_callbacks", "pm_comm_destroy", "pm_comm_rank",
    "pm_comm_world", "pm_comm_last_error", "pm_comm_kind", "pm_comm_set_timeout_ms", "pm_comm_abort", "pm_comm_failed", "pm_comm_busy_ms", "pm_host_make_vk", "pm_host_verify", "pm_comm_all_gather", "pm_comm_all_to_all", "pm_comm_all_gather_device", "pm_comm_combine_points", "pm_ctx_set_comm",
    "pm_ctx_set_option", "pm_ctx_get_option", "pm_comm_local_set_serialize",
    "pm_g1_decode", "pm_pk_load_bytes", "pm_pk_export_bases_compressed", "pm_verify_batch",
    "pm_verify_batch2", "pm_pairing_check_batch",
    "pm_r1cs_check", "pm_r1cs_check_batch",
]
# pm_option / pm_tables_mode (include/polymath_hip.h)
OPTIONS = {"msm_overlap": 0, "ntt_overlap": 1, "tables": 2, "msm_max_piece_log": 3, "max_seg_log": 4, "inflight_contexts": 5,
           "msm_task_len": 6, "table_window_bits": 7, "wire_chunk_log": 8}
TABLES_MODES = {"off": 0, "auto": 1, "wide": 2, "no_wide": 3}
SHARD_PAIRS, SHARD_VECTOR = 0, 1
LAYOUTS = {"pairs": SHARD_PAIRS, "vector": SHARD_VECTOR, 0: 0, 1: 1}

_lib = None


def load_library():
    """Loads the HIP library or raises -- the product never falls back to a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libpolymath_hip.so not built: run `python -m polymath_amd.build` "
                          "(__graft_entry__.build()).  There is no CPU fallback.")
    L = ct.CDLL(LIB_PATH)
    vp, sz, u64, i = ct.c_void_p, ct.c_size_t, ct.c_uint64, ct.c_int
    L.pm_device_count.restype = i
    L.pm_ctx_create.argtypes = [i, ct.POINTER(vp)]
    L.pm_ctx_destroy.argtypes = [vp]
    L.pm_ctx_destroy.restype = None
    L.pm_last_error.argtypes = [vp]
    L.pm_last_error.restype = ct.c_char_p
    L.pm_last_timings.argtypes = [vp, ct.POINTER(ct.c_double), i]
    L.pm_ntt.argtypes = [vp, i, u64p, ct.c_uint, i]
    L.pm_ntt_device.argtypes = [vp, i, vp, ct.c_uint, i]
    L.pm_ntt_batch_device.argtypes = [vp, i, vp, ct.c_uint, i, sz, sz]
    L.pm_msm_g1.argtypes = [vp, i, vp, sz, u64p, sz, u64p, intp]
    L.pm_bases_upload.argtypes = [vp, i, vp, sz, sz, ct.POINTER(vp)]
    L.pm_bases_generate_multiples.argtypes = [vp, i, sz, ct.POINTER(vp)]
    L.pm_bases_download.argtypes = [vp, vp, sz, sz, u64p]
    L.pm_bases_precompute.argtypes = [vp, vp]
    L.pm_bases_len.argtypes = [vp]
    L.pm_bases_len.restype = sz
    L.pm_bases_free.argtypes = [vp]
    L.pm_bases_free.restype = None
    L.pm_msm_g1_resident.argtypes = [vp, vp, sz, vp, i, sz, u64p, intp]
    L.pm_msm_g1_resident_batch.argtypes = [vp, vp, sz, vp, i, sz, sz, u64p, intp]
    L.pm_g1_sum.argtypes = [i, u64p, intp, sz, u64p, intp]
    L.pm_pk_load.argtypes = [vp, i, u64, u64, u64, u64, u64, ct.POINTER(PmCsr), ct.POINTER(PmCsr), ct.POINTER(PmCsr),
                             ct.POINTER(PmBaseArray), i, i, ct.POINTER(vp)]
    L.pm_pk_generate.argtypes = [vp, i, u64, u64, u64, ct.POINTER(PmCsr), ct.POINTER(PmCsr), ct.POINTER(PmCsr), u64p,
                                 u64p, i, i, ct.POINTER(vp)]
    L.pm_pk_info.argtypes = [vp, u64p, u64p, u64p, u64p, u64p]
    L.pm_host_prove.argtypes = [vp, vp, ct.c_int, u64p, ct.c_void_p, ct.c_void_p, ct.c_int, u64p, ct.c_char_p, ct.c_size_t, ct.POINTER(ct.c_size_t)]
    L.pm_host_prove_batch.argtypes = [vp, vp, ct.c_int, sz, u64p, ct.c_void_p, ct.c_void_p, ct.c_int, u64p, ct.c_char_p, sz, intp]
    L.pm_r1cs_check.argtypes = [vp, vp, ct.c_void_p, ct.c_void_p, ct.c_int, sz, u64p, u64p, u64p]
    L.pm_r1cs_check_batch.argtypes = [vp, vp, sz, ct.c_void_p, ct.c_void_p, ct.c_int, sz, u64p, u64p, u64p]
    L.pm_host_prove_sharded.argtypes = [vp, vp, ct.c_int, u64p, ct.c_void_p, ct.c_void_p, ct.c_int, u64p, COMBINE_FN, ct.c_void_p, ct.c_char_p,
                                        ct.c_size_t, ct.POINTER(ct.c_size_t)]
    L.pm_pk_msm_plan.argtypes = [vp, ct.c_int, u64p, ct.POINTER(ct.c_uint), ct.POINTER(ct.c_uint), intp]
    L.pm_pk_export_bases.argtypes = [vp, vp, i, sz, sz, u64p]
    L.pm_pk_free.argtypes = [vp]
    L.pm_pk_free.restype = None
    L.pm_prove_phase1.argtypes = [vp, vp, u64p, u64p, u64p, u64p, intp, u64p, intp]
    L.pm_prove_phase1_device.argtypes = [vp, vp, vp, vp, u64p, u64p, intp, u64p, intp]
    L.pm_prove_phase2.argtypes = [vp, u64p, u64p]
    L.pm_prove_phase3.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, intp]
    L.pm_prove_tap.argtypes = [vp, i, u64p, sz, ct.POINTER(sz)]
    L.pm_host_keccak_f1600.argtypes = [u64p]
    L.pm_host_keccak_f1600.restype = None
    L.pm_synth_r1cs.argtypes = [i, u64, u64, u64p, u32p, u64p, u32p, u64p, u32p, u64p, u64p]
    L.pm_selftest_field.argtypes = [vp, sz, u64, u64p]
    L.pm_pk_load_sharded.argtypes = [vp, i, u64, u64, u64, u64, u64, ct.POINTER(PmCsr), ct.POINTER(PmCsr), ct.POINTER(PmCsr),
                                     ct.POINTER(PmBaseArray), i, i, i, ct.POINTER(vp)]
    L.pm_pk_generate_sharded.argtypes = [vp, i, u64, u64, u64, ct.POINTER(PmCsr), ct.POINTER(PmCsr), ct.POINTER(PmCsr), u64p,
                                         u64p, i, i, i, ct.POINTER(vp)]
    L.pm_layout_indices.argtypes = [u64, i, i, i, u64p]
    L.pm_pk_msm_pieces.argtypes = [vp, i, u64p, u64p, sz, ct.POINTER(sz)]
    L.pm_comm_rccl_unique_id.argtypes = [vp]
    L.pm_comm_rccl_create.argtypes = [vp, i, i, i, ct.POINTER(vp)]
    L.pm_comm_local_create.argtypes = [i, ct.POINTER(vp)]
    L.pm_comm_from_callbacks.argtypes = [vp, i, i, ct.POINTER(vp)]
    L.pm_comm_destroy.argtypes = [vp]
    L.pm_comm_destroy.restype = None
    L.pm_comm_rank.argtypes = [vp]
    L.pm_comm_world.argtypes = [vp]
    L.pm_comm_last_error.argtypes = [vp]
    L.pm_comm_last_error.restype = ct.c_char_p
    L.pm_comm_kind.argtypes = [vp]
    L.pm_comm_kind.restype = ct.c_char_p
    L.pm_comm_set_timeout_ms.argtypes = [vp, ct.c_long]
    L.pm_comm_abort.argtypes = [vp, ct.c_char_p]
    L.pm_comm_failed.argtypes = [vp]
    L.pm_host_make_vk.argtypes = [i, u64, u64, u64, u64p, u64p, u64p, ct.c_char_p, sz, ct.POINTER(sz)]
    L.pm_host_verify.argtypes = [i, i, ct.c_char_p, sz, u64p, sz, ct.c_char_p, sz, intp]
    L.pm_comm_busy_ms.argtypes = [vp, i]
    L.pm_comm_busy_ms.restype = ct.c_double
    L.pm_comm_all_gather.argtypes = [vp, vp, vp, sz]
    L.pm_comm_all_to_all.argtypes = [vp, vp, vp, sz, vp]
    L.pm_comm_all_gather_device.argtypes = [vp, vp, vp, sz, vp]
    L.pm_comm_combine_points.argtypes = [vp, i, i, u64p, intp]
    L.pm_ctx_set_comm.argtypes = [vp, vp]
    L.pm_ctx_set_option.argtypes = [vp, i, ct.c_longlong]
    L.pm_ctx_get_option.argtypes = [vp, i, ct.POINTER(ct.c_longlong)]
    L.pm_comm_local_set_serialize.argtypes = [vp, i]
    L.pm_g1_decode.argtypes = [vp, i, vp, sz, i, u64p, vp]
    L.pm_pk_load_bytes.argtypes = [vp, i, vp, sz, i, i, i, i, ct.POINTER(vp)]
    L.pm_pk_export_bases_compressed.argtypes = [vp, vp, i, sz, sz, vp]
    L.pm_verify_batch.argtypes = [vp, i, i, ct.c_char_p, sz, u64p, sz, vp, sz, sz, ct.c_char_p, vp, intp, ct.POINTER(sz)]
    L.pm_verify_batch2.argtypes = [vp, i, i, ct.c_char_p, sz, u64p, sz, vp, sz, sz, ct.c_char_p, i, vp, intp, ct.POINTER(sz)]
    L.pm_pairing_check_batch.argtypes = [vp, i, u64p, sz, vp, sz, sz, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(u64p)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def encode_hints(hints):
    """The words of pm_pk_set_hints for a list of hints.  A hint is a dict {"n", "q", "rem", "D", and "E" (divisor columns) or "literal"
    (the divisor's limbs as Python integers)} or a tuple (n, q, rem, D, E) / (n, q, rem, D, None, literal); q, rem, D, E are lists of
    CSR columns (0: the constant one, then the instance, then the witness).  A modular division is a dict with "op": "moddiv":
    {"op", "n", "z", "Dp", "P" (modulus columns) or "literal" (the modulus' limbs), and optionally "Np", "Nm", "Dm"}; without "Np" and
    "Nm" the numerator is 1.  A wide long division is the long division's dict with "op": "longdiv_wide".  A modular multiply-divide
    is a dict with "op": "modmuldiv": {"op", "n", "z", "A", "B", "P" or "literal", and optionally "Np", "Nm", "Dp", "Dm" (no denominator
    lists: D = 1), "cN", "cD" (1 where absent)}.  -> np.uint64[n_words]"""
    words = []
    for hint in hints:
        if isinstance(hint, dict) and hint.get("op") == "modmuldiv":
            P, literal = hint.get("P"), hint.get("literal")
            if (P is None) == (literal is None):
                raise ValueError("a modular hint has modulus columns P or a literal modulus, not both and not neither")
            lists = [list(hint["z"]), list(hint["A"]), list(hint["B"])] + [list(hint.get(key, ())) for key in ("Np", "Nm", "Dp", "Dm")]
            modulus = list(P) if literal is None else list(literal)
            cN, cD = int(hint.get("cN", 1)), int(hint.get("cD", 1))
            if not (1 <= cN < 1 << 32 and 1 <= cD < 1 << 32):
                raise ValueError("cN and cD are one-word literals in 1 .. 2^32 - 1")
            words += [HINT_MODMULDIV, int(hint["n"])] + [len(v) for v in lists] + [len(modulus), 0 if literal is None else HINT_MODULUS_LITERAL, cN, cD]
            words += [int(c) for v in lists for c in v]
            if literal is None:
                words += [int(c) for c in modulus]
            else:
                for limb in modulus:
                    if not 0 <= int(limb) < 1 << 256:
                        raise ValueError("a literal limb is four words")
                    words += [(int(limb) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
            continue
        if isinstance(hint, dict) and hint.get("op", "longdiv") not in ("longdiv", "longdiv_wide"):
            if hint["op"] != "moddiv":
                raise ValueError("unknown hint op %r" % (hint["op"],))
            P, literal = hint.get("P"), hint.get("literal")
            if (P is None) == (literal is None):
                raise ValueError("a modular hint has modulus columns P or a literal modulus, not both and not neither")
            lists = [list(hint["z"])] + [list(hint.get(key, ())) for key in ("Np", "Nm")] + [list(hint["Dp"]), list(hint.get("Dm", ()))]
            modulus = list(P) if literal is None else list(literal)
            words += [HINT_MODDIV, int(hint["n"])] + [len(v) for v in lists] + [len(modulus), 0 if literal is None else HINT_MODULUS_LITERAL]
            words += [int(c) for v in lists for c in v]
            if literal is None:
                words += [int(c) for c in modulus]
            else:
                for limb in modulus:
                    if not 0 <= int(limb) < 1 << 256:
                        raise ValueError("a literal limb is four words")
                    words += [(int(limb) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
            continue
        if isinstance(hint, dict):
            n, q, rem, D, E, literal = hint["n"], hint["q"], hint["rem"], hint["D"], hint.get("E"), hint.get("literal")
        else:
            n, q, rem, D, E, literal = (tuple(hint) + (None,))[:6]
        if (E is None) == (literal is None):
            raise ValueError("a hint has divisor columns E or a literal divisor, not both and not neither")
        divisor = list(E) if literal is None else list(literal)
        wide = isinstance(hint, dict) and hint.get("op") == "longdiv_wide"
        words += [HINT_LONGDIV_WIDE if wide else HINT_LONGDIV, int(n), len(q), len(rem), len(D), len(divisor), 0 if literal is None else HINT_DIVISOR_LITERAL]
        words += [int(c) for c in list(q) + list(rem) + list(D)]
        if literal is None:
            words += [int(c) for c in divisor]
        else:
            for limb in divisor:
                if not 0 <= int(limb) < 1 << 256:
                    raise ValueError("a literal limb is four words")
                words += [(int(limb) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return np.array(words, dtype=np.uint64)


def decode_hints(words):
    """encode_hints backwards: -> a list of dicts (the words are trusted to be well-formed: the library is what refuses).  A modular
    division comes back with "op": "moddiv" and all of "Np", "Nm", "Dp", "Dm" (empty lists where the record has none), a wide long
    division with "op": "longdiv_wide", a modular multiply-divide with "op": "modmuldiv", all six lists, "cN" and "cD" """
    words, out, at = [int(v) for v in words], [], 0
    while at < len(words):
        if words[at] == HINT_MODMULDIV:
            n, kz, kA, kB, kNp, kNm, kDp, kDm, kP, flags, cN, cD = words[at + 1:at + 13]
            at += 13
            hint = {"op": "modmuldiv", "n": n, "cN": cN, "cD": cD}
            for key, k in (("z", kz), ("A", kA), ("B", kB), ("Np", kNp), ("Nm", kNm), ("Dp", kDp), ("Dm", kDm)):
                hint[key] = words[at:at + k]
                at += k
            if flags & HINT_MODULUS_LITERAL:
                hint["literal"] = [sum(words[at + 4 * i + j] << (64 * j) for j in range(4)) for i in range(kP)]
                at += 4 * kP
            else:
                hint["P"] = words[at:at + kP]
                at += kP
            out.append(hint)
            continue
        if words[at] == HINT_MODDIV:
            n, kz, kNp, kNm, kDp, kDm, kP, flags = words[at + 1:at + 9]
            at += 9
            hint = {"op": "moddiv", "n": n}
            for key, k in (("z", kz), ("Np", kNp), ("Nm", kNm), ("Dp", kDp), ("Dm", kDm)):
                hint[key] = words[at:at + k]
                at += k
            if flags & HINT_MODULUS_LITERAL:
                hint["literal"] = [sum(words[at + 4 * i + j] << (64 * j) for j in range(4)) for i in range(kP)]
                at += 4 * kP
            else:
                hint["P"] = words[at:at + kP]
                at += kP
            out.append(hint)
            continue
        op, n, kq, kr, kD, kE, flags = words[at:at + 7]
        if op not in (HINT_LONGDIV, HINT_LONGDIV_WIDE):
            raise ValueError("unknown opcode %d" % op)
        at += 7
        take = lambda k: words[at:at + k]
        hint = {"op": "longdiv_wide", "n": n, "q": take(kq)} if op == HINT_LONGDIV_WIDE else {"n": n, "q": take(kq)}
        at += kq
        hint["rem"] = take(kr)
        at += kr
        hint["D"] = take(kD)
        at += kD
        if flags & HINT_DIVISOR_LITERAL:
            hint["literal"] = [sum(words[at + 4 * i + j] << (64 * j) for j in range(4)) for i in range(kE)]
            at += 4 * kE
        else:
            hint["E"] = take(kE)
            at += kE
        out.append(hint)
    return out


def g1_sum(curve, pts, infs=None):
    """pm_g1_sum: host-side sum of G1 points (combining per-GPU partial MSM results); needs no GPU."""
    L = load_library()
    cid = CURVE_IDS[curve]
    pts = _c(pts).reshape(-1, 2 * FQ_LIMBS64[cid])
    out = np.zeros(2 * FQ_LIMBS64[cid], dtype=np.uint64)
    inf = ct.c_int(0)
    ia = np.ascontiguousarray(infs, dtype=np.int32) if infs is not None else None
    st = L.pm_g1_sum(cid, _p(pts), ia.ctypes.data_as(intp) if ia is not None else None, len(pts), _p(out), ct.byref(inf))
    if st:
        raise PolymathError(st, "pm_g1_sum")
    return out, inf.value


TRANSCRIPT_IDS = {"merlin": 0, "keccak256": 1, "blake3": 2}


def make_vk(curve, n, m0, sigma, omega_limbs, x_trapdoor_limbs, z_trapdoor_limbs):
    """pm_host_make_vk: VerifyingKey::serialize_compressed bytes of the key the two trapdoors define (host code, no GPU)."""
    L = load_library()
    buf = ct.create_string_buffer(512)
    n_out = ct.c_size_t(0)
    st = L.pm_host_make_vk(CURVE_IDS[curve], n, m0, sigma, _p(_c(omega_limbs)), _p(_c(x_trapdoor_limbs)), _p(_c(z_trapdoor_limbs)), buf, len(buf),
                           ct.byref(n_out))
    if st:
        raise PolymathError(st, "pm_host_make_vk")
    return buf.raw[:n_out.value]


def verify(curve, transcript, vk_bytes, public_input_limbs, proof_bytes):
    """pm_host_verify: Polymath::verify (verifier.rs:19-62) on the CPU with the library's own pairing.  public inputs WITHOUT the
    leading one, Montgomery limbs [k, 4].  Malformed bytes raise; -> bool."""
    L = load_library()
    pub = _c(public_input_limbs).reshape(-1, 4) if len(public_input_limbs) else np.zeros((0, 4), dtype=np.uint64)
    acc = ct.c_int(0)
    st = L.pm_host_verify(CURVE_IDS[curve], TRANSCRIPT_IDS[transcript], bytes(vk_bytes), len(vk_bytes), _p(pub) if len(pub) else None, len(pub),
                          bytes(proof_bytes), len(proof_bytes), ct.byref(acc))
    if st:
        raise PolymathError(st, "pm_host_verify")
    return bool(acc.value)


def synth_r1cs(curve, nr, seed):
    """pm_synth_r1cs: the SURVEY §8d synthetic R1CS as limb arrays -> (CsrArrays A, B, C, instance [2,4], witness [nr+1,4])."""
    L = load_library()
    vals = [np.zeros((nr, 4), dtype=np.uint64) for _ in range(3)]
    cols = [np.zeros(nr, dtype=np.uint32) for _ in range(3)]
    inst, wit = np.zeros((2, 4), dtype=np.uint64), np.zeros((nr + 1, 4), dtype=np.uint64)
    st = L.pm_synth_r1cs(CURVE_IDS[curve], nr, seed, _p(vals[0]), cols[0].ctypes.data_as(u32p), _p(vals[1]), cols[1].ctypes.data_as(u32p),
                         _p(vals[2]), cols[2].ctypes.data_as(u32p), _p(inst), _p(wit))
    if st:
        raise PolymathError(st, "pm_synth_r1cs")
    rowptr = np.arange(nr + 1, dtype=np.uint64)
    return [CsrArrays(rowptr, cols[k], vals[k]) for k in range(3)], inst, wit


def _byte_view(data):
    """(buffer keeping the memory alive, address, length) of bytes / bytearray / memoryview / np.memmap, without a copy where the
    object exposes a C-contiguous buffer (bytes objects do: ctypes reads them in place)."""
    if isinstance(data, bytes):
        return data, ct.cast(ct.c_char_p(data), ct.c_void_p).value, len(data)
    arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    if not arr.flags.c_contiguous:
        arr = np.ascontiguousarray(arr)
    return arr, arr.ctypes.data, arr.nbytes


def g1_decode(ctx, curve, data, validate=True, form="compressed"):
    """pm_g1_decode: packed G1 records (compressed: 48 B BLS12-381 / 32 B BN254; form="uncompressed": 96 B / 64 B) -> (xy np.uint64
    [count, 2 fq_limbs] Montgomery, infinity and refused points all-zero; status np.uint8 [count] of G1_* codes)."""
    cid = CURVE_IDS[curve]
    keep, addr, nbytes = _byte_view(data)
    rec = g1_record_bytes(cid, form)
    if nbytes % rec:
        raise ValueError("not a whole number of %d-byte records" % rec)
    count = nbytes // rec
    xy = np.zeros((count, 2 * FQ_LIMBS64[cid]), dtype=np.uint64)
    status = np.zeros(count, dtype=np.uint8)
    ctx.check(ctx.L.pm_g1_decode(ctx.h, cid, ct.c_void_p(addr), count, int(bool(validate)) | WIRE_FORMS[form], _p(xy), status.ctypes.data_as(ct.c_void_p)))
    del keep
    return xy, status


def pairing_check_batch(ctx, curve, g2, g1):
    """pm_pairing_check_batch: count checks prod_j e(g1[i][j], g2[j]) == 1 on the GPU, one lane each.  g2: Montgomery limbs
    [k, 4 fq_limbs] (x.c0 || x.c1 || y.c0 || y.c1), k <= 4; g1: [count, k, 2 fq_limbs] (x || y; all-zero = infinity).
    -> np.uint8[count] of 0 / 1."""
    cid = CURVE_IDS[curve]
    g2 = _c(g2).reshape(-1, 4 * FQ_LIMBS64[cid])
    k = g2.shape[0]
    g1 = _c(g1).reshape(-1, k, 2 * FQ_LIMBS64[cid]) if np.size(g1) else np.zeros((0, k, 2 * FQ_LIMBS64[cid]), dtype=np.uint64)
    out = np.zeros(g1.shape[0], dtype=np.uint8)
    ctx.check(ctx.L.pm_pairing_check_batch(ctx.h, cid, _p(g2), k, g1.ctypes.data_as(ct.c_void_p), 16 * FQ_LIMBS64[cid], g1.shape[0],
                                           out.ctypes.data_as(ct.c_void_p)))
    return out


def verify_batch(ctx, curve, transcript, vk_bytes, public_inputs, proofs, seed=None, verdicts=True, pairing="host", challenges="host"):
    """pm_verify_batch2: many proofs against one verifying key; the per-proof curve work on the GPU, the pairing checks on the host
    (pairing="host": a handful per valid batch, a bisection otherwise; what pm_verify_batch does) or on the GPU (pairing="device":
    the root in a launch of one lane, every live leaf in one more launch if it fails; pairing="wave": the same two launches with every
    check spread over 36 lanes of a wave, the leaves while at most VERIFY_WAVE_LEAF_MAX are live -- same results).  public_inputs: Montgomery limbs [count, n_inputs, 4], WITHOUT the leading one; proofs: a list of
    Proof::serialize_compressed byte strings or one packed buffer; seed: None or 32 bytes mixed into the weights' key.
    challenges="device": the per-proof Fiat-Shamir challenges and scalar glue on the GPU too (one lane per proof; the same bits, so
    nothing in the result changes; PM_VERIFY_CHALLENGES_DEVICE OR-ed into the call's `pairing` argument).
    -> (np.uint8[count] of VERIFY_* codes, or None with verdicts=False; all_accepted: bool; n_checks: int)."""
    cid = CURVE_IDS[curve]
    plen = PROOF_BYTES[cid]
    if isinstance(proofs, (list, tuple)):
        if any(len(p) != plen for p in proofs):
            raise PolymathError(1, "pm_verify_batch: a proof is not %d bytes" % plen)
        proofs = b"".join(bytes(p) for p in proofs)
    keep, addr, nbytes = _byte_view(proofs)
    if nbytes % plen:
        raise PolymathError(1, "pm_verify_batch: not a whole number of %d-byte proofs" % plen)
    count = nbytes // plen
    pub = _c(public_inputs).reshape(count, -1, 4) if count and np.size(public_inputs) else np.zeros((count, 0, 4), dtype=np.uint64)
    n_inputs = pub.shape[1]
    if seed is not None and len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    out = np.zeros(count, dtype=np.uint8) if verdicts else None
    acc, checks = ct.c_int(0), ct.c_size_t(0)
    ctx.check(ctx.L.pm_verify_batch2(ctx.h, cid, TRANSCRIPT_IDS[transcript], bytes(vk_bytes), len(vk_bytes), _p(pub) if pub.size else None, n_inputs,
                                     ct.c_void_p(addr), plen, count, bytes(seed) if seed is not None else None,
                                     VERIFY_PAIRING[pairing] | VERIFY_CHALLENGES[challenges],
                                     out.ctypes.data_as(ct.c_void_p) if verdicts else None, ct.byref(acc), ct.byref(checks)))
    del keep
    return out, bool(acc.value), int(checks.value)


def verifier_challenges_batch(ctx, curve, transcript, vk_bytes, public_inputs, proofs):
    """x1, x2 and c(x1) of every proof as verify_proof derives them (verifier.rs:24-42), computed on the GPU, one lane per proof: a
    verify_batch call with challenges="device", then pm_prove_tap(8), which holds what that call's lanes derived.  Arguments as
    verify_batch; the point records are hashed as given, whether or not they decode.  A diagnostic: the batch is verified as well.
    -> (x1, x2, c_at_x1: np.uint64 [count, 4] Montgomery limbs; ok: np.uint8 [count], 0 where a_at_x1 >= r, that row's outputs zero)."""
    _, _, _ = verify_batch(ctx, curve, transcript, vk_bytes, public_inputs, proofs, verdicts=False, challenges="device")
    count = (len(proofs) if isinstance(proofs, (list, tuple)) else _byte_view(proofs)[2] // PROOF_BYTES[CURVE_IDS[curve]])
    rows = np.zeros((count, 4, 4), dtype=np.uint64)
    if count:
        n = ct.c_size_t(0)
        ctx.check(ctx.L.pm_prove_tap(ctx.h, 8, _p(rows), 4 * count, ct.byref(n)))
        if n.value != 4 * count:
            raise PolymathError(8, "pm_prove_tap(8): %d elements for %d proofs" % (n.value, count))
    return rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy(), rows[:, 3, 0].astype(np.uint8)


def verify_batch_timings(ctx):
    """pm_last_timings after verify_batch, under the names of VERIFY_TIMING_SLOTS (ms)."""
    arr = (ct.c_double * len(TIMING_SLOTS))()
    ctx.L.pm_last_timings(ctx.h, arr, len(TIMING_SLOTS))
    return {k: float(arr[v]) for k, v in VERIFY_TIMING_SLOTS.items()}


def layout_indices(n, shard_count, shard_rank, coefficients=True):
    """pm_layout_indices: global coefficient indices (blocked layout) or evaluation rows (cyclic) of a rank's local positions."""
    L = load_library()
    out = np.zeros(n // shard_count, dtype=np.uint64)
    st = L.pm_layout_indices(n, shard_count, shard_rank, int(coefficients), _p(out))
    if st:
        raise PolymathError(st, "pm_layout_indices")
    return out


class Comm:
    """pm_comm: one rank's end of the exchange layer."""

    def __init__(self, handle, keep=None):
        self.L, self.h, self._keep = load_library(), handle, keep

    @classmethod
    def local_group(cls, world, serialize=False):
        """`world` ranks as threads of this process (tests, emulation, single-process multi-GPU).  serialize: the ranks take turns
        between collectives (pm_comm_local_set_serialize: the per-rank emulation of N GPUs on one)."""
        L = load_library()
        arr = (ct.c_void_p * world)()
        st = L.pm_comm_local_create(world, arr)
        if st:
            raise PolymathError(st, "pm_comm_local_create")
        if serialize:
            st = L.pm_comm_local_set_serialize(ct.c_void_p(arr[0]), 1)
            if st:
                raise PolymathError(st, "pm_comm_local_set_serialize")
        return [cls(ct.c_void_p(arr[r])) for r in range(world)]

    @staticmethod
    def rccl_unique_id():
        L = load_library()
        buf = ct.create_string_buffer(128)
        st = L.pm_comm_rccl_unique_id(buf)
        if st:
            raise PolymathError(st, "pm_comm_rccl_unique_id (librccl not loadable?)")
        return buf.raw

    @classmethod
    def rccl(cls, unique_id, rank, world, device):
        """ncclCommInitRank over the 128-byte id rank 0 made with rccl_unique_id(); collective."""
        L = load_library()
        h = ct.c_void_p()
        st = L.pm_comm_rccl_create(ct.c_char_p(unique_id), rank, world, device, ct.byref(h))
        if st:
            raise PolymathError(st, "pm_comm_rccl_create")
        return cls(h)

    @property
    def rank(self):
        return self.L.pm_comm_rank(self.h)

    @property
    def world(self):
        return self.L.pm_comm_world(self.h)

    def busy_ms(self, reset=True):
        return float(self.L.pm_comm_busy_ms(self.h, int(reset)))

    @property
    def kind(self):
        return self.L.pm_comm_kind(self.h).decode()

    @property
    def failed(self):
        return bool(self.L.pm_comm_failed(self.h))

    def last_error(self):
        return self.L.pm_comm_last_error(self.h).decode()

    def set_timeout_ms(self, ms):
        st = self.L.pm_comm_set_timeout_ms(self.h, int(ms))
        if st:
            raise PolymathError(st, "pm_comm_set_timeout_ms")

    def abort(self, why="aborted by the host"):
        self.L.pm_comm_abort(self.h, why.encode())

    def all_gather(self, arr):
        arr = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + arr.shape, dtype=arr.dtype)
        st = self.L.pm_comm_all_gather(self.h, arr.ctypes.data_as(ct.c_void_p), out.ctypes.data_as(ct.c_void_p), arr.nbytes)
        if st:
            raise PolymathError(st, self.L.pm_comm_last_error(self.h).decode())
        return out

    def all_to_all_device(self, d_send, d_recv, bytes_per_peer, stream=None):
        """pm_comm_all_to_all on device pointers: block p of d_send goes to rank p, block r of d_recv comes from rank r
        (enqueued on `stream`; the caller synchronises)."""
        st = self.L.pm_comm_all_to_all(self.h, ct.c_void_p(d_send), ct.c_void_p(d_recv), bytes_per_peer, ct.c_void_p(stream or 0))
        if st:
            raise PolymathError(st, self.L.pm_comm_last_error(self.h).decode())

    def all_gather_device(self, d_send, d_recv, nbytes, stream=None):
        """pm_comm_all_gather_device on device pointers: rank r's `nbytes` land at d_recv + r * nbytes (the caller synchronises)."""
        st = self.L.pm_comm_all_gather_device(self.h, ct.c_void_p(d_send), ct.c_void_p(d_recv), nbytes, ct.c_void_p(stream or 0))
        if st:
            raise PolymathError(st, self.L.pm_comm_last_error(self.h).decode())

    def close(self):
        """pm_comm_destroy.  Detach it from its contexts first (Context.set_comm(None)): a context does not own its comm."""
        if getattr(self, "h", None):
            self.L.pm_comm_destroy(self.h)
            self.h = None


class Context:
    """pm_ctx: one HIP stream + workspaces on one GPU; one proof in flight."""

    def __init__(self, device=0):
        self.L = load_library()
        h = ct.c_void_p()
        st = self.L.pm_ctx_create(device, ct.byref(h))
        if st:
            raise PolymathError(st, "pm_ctx_create(device=%d)" % device)
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.pm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        """pm_last_error: the message of the context's last failing call (the row or column a solving call refused, ...)."""
        return self.L.pm_last_error(self.h).decode()

    def check(self, st):
        if st:
            raise PolymathError(st, self.last_error())

    def set_comm(self, comm):
        """Join this context to its rank's communicator (needed by PM_SHARD_VECTOR keys)."""
        self.comm = comm
        self.check(self.L.pm_ctx_set_comm(self.h, comm.h if comm is not None else None))

    def set_option(self, name, value):
        """pm_ctx_set_option: name in OPTIONS (or the pm_option number); "tables" also takes a TABLES_MODES name."""
        key = OPTIONS[name] if isinstance(name, str) else int(name)
        if key == OPTIONS["tables"] and isinstance(value, str):
            value = TABLES_MODES[value]
        self.check(self.L.pm_ctx_set_option(self.h, key, int(value)))

    def get_option(self, name):
        key = OPTIONS[name] if isinstance(name, str) else int(name)
        v = ct.c_longlong(0)
        self.check(self.L.pm_ctx_get_option(self.h, key, ct.byref(v)))
        return int(v.value)

    def selftest_field(self, products_per_field=4096, seed=1):
        """pm_selftest_field: the device's field products vs the host's CIOS -> mismatch counts {field: n} (all zero when healthy)."""
        bad = (ct.c_uint64 * 4)()
        self.check(self.L.pm_selftest_field(self.h, products_per_field, seed, bad))
        return dict(zip(("bls12_381_fr", "bn254_fr", "bls12_381_fq", "bn254_fq"), (int(v) for v in bad)))

    def timings(self):
        arr = (ct.c_double * len(TIMING_SLOTS))()
        self.L.pm_last_timings(self.h, arr, len(TIMING_SLOTS))
        return dict(zip(TIMING_SLOTS, list(arr)))

    # ---- standalone kernels
    def ntt(self, curve, data, log_n, inverse=False):
        data = _c(data).copy()
        self.check(self.L.pm_ntt(self.h, CURVE_IDS[curve], _p(data), log_n, int(inverse)))
        return data

    def ntt_device(self, curve, dptr, log_n, inverse=False):
        self.check(self.L.pm_ntt_device(self.h, CURVE_IDS[curve], ct.c_void_p(dptr), log_n, int(inverse)))

    def ntt_batch_device(self, curve, dptr, log_n, inverse, rows, row_stride):
        """pm_ntt_batch_device: `rows` transforms in place on a device buffer, row b at dptr + b * row_stride Fr elements."""
        self.check(self.L.pm_ntt_batch_device(self.h, CURVE_IDS[curve], ct.c_void_p(dptr), log_n, int(inverse), rows, row_stride))

    def msm(self, curve, bases, scalars):
        cid = CURVE_IDS[curve]
        bases, scalars = _c(bases), _c(scalars)
        out = np.zeros(2 * FQ_LIMBS64[cid], dtype=np.uint64)
        inf = ct.c_int(0)
        self.check(self.L.pm_msm_g1(self.h, cid, bases.ctypes.data_as(ct.c_void_p), max(bases.strides[0], 16 * FQ_LIMBS64[cid]) if bases.ndim > 1 else 16 * FQ_LIMBS64[cid],
                                    _p(scalars), scalars.shape[0], _p(out), ct.byref(inf)))
        return out, inf.value

    def g1_sum(self, curve, pts, infs=None):
        return g1_sum(curve, pts, infs)


class Bases:
    """pm_bases: a G1 base vector resident in HBM."""

    def __init__(self, ctx, curve, handle):
        self.ctx, self.curve, self.cid, self.h = ctx, curve, CURVE_IDS[curve], handle

    @classmethod
    def upload(cls, ctx, curve, bases):
        bases = _c(bases)
        h = ct.c_void_p()
        ctx.check(ctx.L.pm_bases_upload(ctx.h, CURVE_IDS[curve], bases.ctypes.data_as(ct.c_void_p), max(bases.strides[0], 16 * FQ_LIMBS64[CURVE_IDS[curve]]),
                                        bases.shape[0], ct.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def multiples(cls, ctx, curve, length):
        h = ct.c_void_p()
        ctx.check(ctx.L.pm_bases_generate_multiples(ctx.h, CURVE_IDS[curve], length, ct.byref(h)))
        return cls(ctx, curve, h)

    def precompute(self):
        """pm_bases_precompute: build the window tables (W x memory) for faster resident MSMs."""
        self.ctx.check(self.ctx.L.pm_bases_precompute(self.ctx.h, self.h))
        return self

    def __len__(self):
        return int(self.ctx.L.pm_bases_len(self.h))

    def download(self, offset=0, length=None):
        if length is None:
            length = len(self) - offset
        out = np.zeros((length, 2 * FQ_LIMBS64[self.cid]), dtype=np.uint64)
        self.ctx.check(self.ctx.L.pm_bases_download(self.ctx.h, self.h, offset, length, _p(out)))
        return out

    def msm(self, scalars, offset=0, length=None, device_ptr=None):
        """scalars: host np.uint64 [len,4], or device_ptr (int) + length for scalars already in HBM."""
        out = np.zeros(2 * FQ_LIMBS64[self.cid], dtype=np.uint64)
        inf = ct.c_int(0)
        if device_ptr is not None:
            st = self.ctx.L.pm_msm_g1_resident(self.ctx.h, self.h, offset, ct.c_void_p(device_ptr), 1, length, _p(out), ct.byref(inf))
        else:
            scalars = _c(scalars)
            length = scalars.shape[0] if length is None else length
            st = self.ctx.L.pm_msm_g1_resident(self.ctx.h, self.h, offset, scalars.ctypes.data_as(ct.c_void_p), 0, length,
                                               _p(out), ct.byref(inf))
        self.ctx.check(st)
        return out, inf.value

    def msm_batch(self, scalars, offset=0, length=None, device_ptr=None, batch=None):
        """pm_msm_g1_resident_batch: `batch` MSMs of `length` pairs against bases [offset, offset + length).  scalars: host np.uint64
        [batch, len, 4], or device_ptr (int) + length + batch for rows already in HBM, row after row.
        -> (np.uint64 [batch, 2 nq], np.int32 [batch])."""
        if device_ptr is not None:
            ptr, on_device = ct.c_void_p(device_ptr), 1
        else:
            scalars = _c(scalars)
            batch = scalars.shape[0] if batch is None else batch
            length = (scalars.shape[1] if scalars.ndim == 3 else 0) if length is None else length
            ptr, on_device = scalars.ctypes.data_as(ct.c_void_p), 0
        out = np.zeros((batch, 2 * FQ_LIMBS64[self.cid]), dtype=np.uint64)
        inf = np.zeros(batch, dtype=np.int32)
        self.ctx.check(self.ctx.L.pm_msm_g1_resident_batch(self.ctx.h, self.h, offset, ptr, on_device, length, batch, _p(out),
                                                           inf.ctypes.data_as(intp)))
        return out, inf

    def free(self):
        if self.h:
            self.ctx.L.pm_bases_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CsrArrays:
    """numpy-backed pm_csr.  rows: list of rows of (value_montgomery_limbs_or_index...)."""

    def __init__(self, rowptr, col, val):
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        self.col = np.ascontiguousarray(col if len(col) else [0], dtype=np.uint32)
        self.val = _c(val) if len(val) else np.zeros((1, 4), dtype=np.uint64)
        self.struct = PmCsr(len(self.rowptr) - 1, _p(self.rowptr), self.col.ctypes.data_as(u32p), _p(self.val))


class ProvingKey:
    """pm_pk: R1CS matrices + the six base vectors resident on one GPU (optionally one shard)."""

    def __init__(self, ctx, curve, handle, csrs):
        self.ctx, self.curve, self.cid, self.h, self._csrs = ctx, curve, CURVE_IDS[curve], handle, csrs
        n, m0, sigma = ct.c_uint64(), ct.c_uint64(), ct.c_uint64()
        omega = np.zeros(4, dtype=np.uint64)
        lens = np.zeros(6, dtype=np.uint64)
        ctx.check(ctx.L.pm_pk_info(self.h, ct.byref(n), ct.byref(m0), ct.byref(sigma), _p(omega), _p(lens)))
        self.n, self.m0, self.sigma, self.omega_limbs = n.value, m0.value, sigma.value, omega
        self.base_lens = [int(v) for v in lens]
        self.nq = FQ_LIMBS64[self.cid]

    @classmethod
    def generate(cls, ctx, curve, m0, mw, nr, a, b, c, x_trapdoor, z_trapdoor, shard_rank=0, shard_count=1, layout="pairs"):
        """a, b, c: CsrArrays; trapdoors: np.uint64[4] Montgomery (generator.rs:72,77 draws).  layout: "pairs" (MSM pair
        ranges sharded, vector phases replicated) or "vector" (everything sharded; the context needs set_comm)."""
        h = ct.c_void_p()
        ctx.check(ctx.L.pm_pk_generate_sharded(ctx.h, CURVE_IDS[curve], m0, mw, nr, ct.byref(a.struct), ct.byref(b.struct),
                                               ct.byref(c.struct), _p(_c(x_trapdoor)), _p(_c(z_trapdoor)), shard_rank, shard_count,
                                               LAYOUTS[layout], ct.byref(h)))
        pk = cls(ctx, curve, h, (a, b, c))
        pk.shard_rank, pk.shard_count, pk.layout = shard_rank, shard_count, LAYOUTS[layout]
        return pk

    @classmethod
    def load(cls, ctx, curve, n, m0, mw, nr, sigma, a, b, c, base_arrays, shard_rank=0, shard_count=1, layout="pairs"):
        """base_arrays: six np.uint64 2-D arrays in pm_base_vec order."""
        arrs = [_c(x) for x in base_arrays]
        BA = (PmBaseArray * 6)()
        for k, x in enumerate(arrs):
            BA[k] = PmBaseArray(x.ctypes.data_as(ct.c_void_p), x.shape[0], x.strides[0])
        h = ct.c_void_p()
        ctx.check(ctx.L.pm_pk_load_sharded(ctx.h, CURVE_IDS[curve], n, m0, mw, nr, sigma, ct.byref(a.struct), ct.byref(b.struct),
                                           ct.byref(c.struct), BA, shard_rank, shard_count, LAYOUTS[layout], ct.byref(h)))
        pk = cls(ctx, curve, h, (a, b, c))
        pk.shard_rank, pk.shard_count, pk.layout = shard_rank, shard_count, LAYOUTS[layout]
        return pk

    @classmethod
    def load_bytes(cls, ctx, curve, data, validate=True, shard_rank=0, shard_count=1, layout="pairs", form="compressed", relations=False):
        """pm_pk_load_bytes: ProvingKey::serialize_compressed (form="uncompressed": serialize_uncompressed) bytes -> resident key;
        the points are decoded (and with `validate` checked as ark's Validate::Yes does) on the device.  data: bytes, memoryview or
        np.memmap of a key file, not copied.  relations: PM_KEY_CHECK_RELATIONS -- the key is also checked against its own vk and
        matrices (validation included) and refused, naming the first relation that fails, if it is not a proving key."""
        keep, addr, nbytes = _byte_view(data)
        h = ct.c_void_p()
        flags = int(bool(validate)) | WIRE_FORMS[form] | (PM_KEY_CHECK_RELATIONS if relations else PM_KEY_CHECK_NONE)
        ctx.check(ctx.L.pm_pk_load_bytes(ctx.h, CURVE_IDS[curve], ct.c_void_p(addr), nbytes, flags, shard_rank, shard_count,
                                         LAYOUTS[layout], ct.byref(h)))
        del keep
        pk = cls(ctx, curve, h, None)
        pk.shard_rank, pk.shard_count, pk.layout = shard_rank, shard_count, LAYOUTS[layout]
        return pk

    def view(self, ctx):
        """The same resident key used from another context (a pm_pk is immutable and shareable; each context runs
        one proof at a time).  The view does not own the handle: free the original."""
        v = ProvingKey.__new__(ProvingKey)
        v.__dict__.update(self.__dict__)
        v.ctx, v._view = ctx, True
        return v

    def msm_plan(self, which):
        """(pairs, windows = bucket additions per pair, window bits, has tables) of merged MSM 0 = a, 1 = c, 2 = d."""
        pairs, win, bits, tb = ct.c_uint64(), ct.c_uint(), ct.c_uint(), ct.c_int()
        self.ctx.check(self.ctx.L.pm_pk_msm_plan(self.h, which, ct.byref(pairs), ct.byref(win), ct.byref(bits), ct.byref(tb)))
        return pairs.value, win.value, bits.value, bool(tb.value)

    def msm_pieces(self, which):
        """[(cat_lo, count), ...]: the resident pairs of merged MSM `which` as ranges of the logical base concatenation."""
        n = ct.c_size_t(0)
        self.ctx.check(self.ctx.L.pm_pk_msm_pieces(self.h, which, None, None, 0, ct.byref(n)))
        lo, cnt = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        self.ctx.check(self.ctx.L.pm_pk_msm_pieces(self.h, which, _p(lo), _p(cnt), n.value, ct.byref(n)))
        return [(int(a), int(b)) for a, b in zip(lo, cnt)]

    def msm_windows(self, which):
        return self.msm_plan(which)[1]

    def export_bases(self, which, offset=0, length=None):
        if length is None:
            length = self.base_lens[which] - offset
        out = np.zeros((length, 2 * self.nq), dtype=np.uint64)
        self.ctx.check(self.ctx.L.pm_pk_export_bases(self.ctx.h, self.h, which, offset, length, _p(out)))
        return out

    def export_bases_compressed(self, which, offset=0, length=None, form="compressed"):
        """pm_pk_export_bases_compressed: (a range of) base vector `which` as its serialize_compressed point records -> bytes;
        form="uncompressed": its serialize_uncompressed records (which | PM_WIRE_UNCOMPRESSED)."""
        if length is None:
            length = self.base_lens[which] - offset
        rec = g1_record_bytes(self.cid, form)
        out = ct.create_string_buffer(max(1, length * rec))
        self.ctx.check(self.ctx.L.pm_pk_export_bases_compressed(self.ctx.h, self.h, which | WIRE_FORMS[form], offset, length, out))
        return out.raw[:length * rec]

    # --- the three prover phases: (status, outputs...) tuples, status codes of pm_status
    def phase1(self, x, w, r_a):
        a = np.zeros(2 * self.nq, dtype=np.uint64)
        c = np.zeros(2 * self.nq, dtype=np.uint64)
        ai, ci = ct.c_int(0), ct.c_int(0)
        w = _c(w) if len(w) else np.zeros((1, 4), dtype=np.uint64)
        rc = self.ctx.L.pm_prove_phase1(self.ctx.h, self.h, _p(_c(x)), _p(w), _p(_c(r_a)), _p(a), ct.byref(ai), _p(c), ct.byref(ci))
        return rc, a, ai.value, c, ci.value

    def phase1_device(self, d_x, d_w, r_a):
        """assignment already in HBM: d_x, d_w are device pointers (ints) to m0 / mw Montgomery Fr."""
        a = np.zeros(2 * self.nq, dtype=np.uint64)
        c = np.zeros(2 * self.nq, dtype=np.uint64)
        ai, ci = ct.c_int(0), ct.c_int(0)
        rc = self.ctx.L.pm_prove_phase1_device(self.ctx.h, self.h, ct.c_void_p(d_x), ct.c_void_p(d_w), _p(_c(r_a)), _p(a), ct.byref(ai),
                                               _p(c), ct.byref(ci))
        return rc, a, ai.value, c, ci.value

    TRANSCRIPT_IDS = {"merlin": 0, "keccak256": 1, "blake3": 2}

    def host_prove(self, transcript, instance_limbs, x, w, r_a, on_device=False, combine_many=None, solve=False):
        """pm_host_prove / pm_host_prove_sharded: all three phases and the Fiat-Shamir glue in one native call.
        x, w: numpy limb arrays, or device pointers (ints) with on_device=True.  combine_many (sharded keys):
        [(xy, inf), ...] -> the same list summed over all ranks (polymath_amd.distributed.PointCombiner.many).
        solve (unsharded keys, pm_host_prove with PM_ASSIGNMENT_SOLVE): entries equal to UNKNOWN_LIMBS are computed on the device first;
        solve_results() then returns the completed public inputs.
        -> (status, proof bytes)."""
        buf = ct.create_string_buffer(256)
        n = ct.c_size_t(0)
        if solve:
            if combine_many is not None:
                raise ValueError("solve needs an unsharded key")
            if on_device:
                px, pw = ct.c_void_p(x), ct.c_void_p(w)
            else:
                x = _c(x)
                w = _c(w) if len(w) else np.zeros((1, 4), dtype=np.uint64)
                px, pw = x.ctypes.data_as(ct.c_void_p), w.ctypes.data_as(ct.c_void_p)
            rc = self.ctx.L.pm_host_prove(self.ctx.h, self.h, self.TRANSCRIPT_IDS[transcript], _p(_c(instance_limbs)), px, pw,
                                          int(bool(on_device)) | ASSIGNMENT_SOLVE, _p(_c(r_a)), buf, len(buf), ct.byref(n))
            return rc, buf.raw[:n.value]
        words = 2 * self.nq
        failure = []

        def _cb(_user, count, xy, inf):
            try:
                pts = [(np.ctypeslib.as_array(xy, shape=(count * words,))[j * words:(j + 1) * words].copy(), int(inf[j])) for j in range(count)]
                for j, (sxy, sinf) in enumerate(combine_many(pts)):
                    for k, v in enumerate(np.asarray(sxy, dtype=np.uint64).tolist()):
                        xy[j * words + k] = v
                    inf[j] = int(sinf)
                return 0
            except Exception as e:          # never unwind through the C frames
                failure.append(e)
                return 8                    # PM_ERR_STATE
        cb = COMBINE_FN(_cb) if combine_many is not None else ct.cast(None, COMBINE_FN)
        if on_device:
            px, pw = ct.c_void_p(x), ct.c_void_p(w)
        else:
            x = _c(x)
            w = _c(w) if len(w) else np.zeros((1, 4), dtype=np.uint64)
            px, pw = x.ctypes.data_as(ct.c_void_p), w.ctypes.data_as(ct.c_void_p)
        rc = self.ctx.L.pm_host_prove_sharded(self.ctx.h, self.h, self.TRANSCRIPT_IDS[transcript], _p(_c(instance_limbs)), px, pw, int(on_device),
                                              _p(_c(r_a)), cb, None, buf, len(buf), ct.byref(n))
        if failure:
            raise failure[0]
        return rc, buf.raw[:n.value]

    def host_prove_batch(self, transcript, instance_limbs, x, w, r_a, on_device=False, solve=False, glue="host"):
        """pm_host_prove_batch: `count` proofs against this (unsharded) key in one native call.  instance_limbs: (count, m0, 4) host
        limbs (hashed); x, w: (count, m0, 4) / (count, mw, 4) host limbs, or device pointers (ints) to the same rows with
        on_device=True; r_a: (count, 2, 4).  solve: PM_ASSIGNMENT_SOLVE, entries equal to UNKNOWN_LIMBS (instance_limbs included) are computed
        on the device first; solve_results() then returns the completed public inputs.
        glue: "host" (the default) or "device" -- PM_PROVE_GLUE_DEVICE: the Fiat-Shamir glue between the phases runs in kernels with
        one lane per proof, one copy to the host and one synchronisation per group; same statuses, same bytes; glue_challenges()
        then returns what the kernels derived.
        -> (status of the call, bytes of count * proof_len, np.int32[count] per-proof statuses)."""
        inst = _c(instance_limbs)
        count = int(inst.shape[0]) if inst.ndim == 3 else 0
        proof_len = 3 * 8 * self.nq + 32
        buf = ct.create_string_buffer(max(1, count * proof_len))
        status = np.zeros(max(1, count), dtype=np.int32)
        r_a = _c(r_a)
        if on_device:
            px, pw = ct.c_void_p(x), ct.c_void_p(w)
        else:
            x = _c(x)
            w = _c(w) if np.size(w) else np.zeros((max(1, count), 1, 4), dtype=np.uint64)
            px, pw = x.ctypes.data_as(ct.c_void_p), w.ctypes.data_as(ct.c_void_p)
        rc = self.ctx.L.pm_host_prove_batch(self.ctx.h, self.h, self.TRANSCRIPT_IDS[transcript] | PROVE_GLUE[glue], count, _p(inst), px, pw, int(bool(on_device)) | (ASSIGNMENT_SOLVE if solve else 0), _p(r_a),
                                            buf, proof_len, status.ctypes.data_as(ct.POINTER(ct.c_int)))
        return rc, buf.raw[:count * proof_len], status[:count]

    def set_hints(self, hints):
        """Declare the key's hints: pm_pk_load_bytes with PM_KEY_HINTS on this key (encode_hints takes the list; an empty one clears the
        declaration) -> status"""
        words = hints if isinstance(hints, np.ndarray) else encode_hints(hints)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        raw = self.h.value if isinstance(self.h, ct.c_void_p) else self.h
        key = ct.c_void_p(raw)
        rc = self.ctx.L.pm_pk_load_bytes(self.ctx.h, self.cid, words.ctypes.data_as(ct.c_void_p) if words.size else None, int(words.size) * 8, PM_KEY_HINTS, 0, 1, 0,
                                         ct.byref(key))
        assert key.value == raw      # the key stays where it is
        return rc

    def r1cs_check_batch(self, x, w, max_rows=16, residuals=False, on_device=False, count=None, solve=False):
        """pm_r1cs_check_batch: which constraint rows each of `count` assignments violates.  x, w: (count, m0, 4) / (count, mw, 4) host
        limbs, or device pointers (ints) to the same rows with on_device=True and `count` given.  -> (status of the call,
        np.uint64[count] n_bad, np.uint64[count, max_rows] smallest failing rows ascending (padding 2^64 - 1),
        np.uint64[count, max_rows, 3, 4] (Az, Bz, Cz) of the listed rows or None).  solve: PM_ASSIGNMENT_SOLVE, entries equal to
        UNKNOWN_LIMBS are computed on the device first (a stuck assignment: n_bad = 2^64 - 1, rows[0] = its stuck row);
        solve_results() / solved_assignments() read the completed values back."""
        if on_device:
            px, pw = ct.c_void_p(x), ct.c_void_p(w)
        else:
            x = _c(x)
            count = int(x.shape[0]) if x.ndim == 3 else 0
            w = _c(w) if np.size(w) else np.zeros((max(1, count), 1, 4), dtype=np.uint64)
            px, pw = x.ctypes.data_as(ct.c_void_p), w.ctypes.data_as(ct.c_void_p)
        count, max_rows = int(count), int(max_rows)
        n_bad = np.zeros(count, dtype=np.uint64)
        rows = np.full((count, max_rows), np.iinfo(np.uint64).max, dtype=np.uint64)
        abc = np.zeros((count, max_rows, 3, 4), dtype=np.uint64) if residuals else None
        rc = self.ctx.L.pm_r1cs_check_batch(self.ctx.h, self.h, count, px, pw, int(bool(on_device)) | (ASSIGNMENT_SOLVE if solve else 0), max_rows, _p(n_bad) if count else None,
                                            _p(rows) if rows.size else None, _p(abc) if residuals and abc.size else None)
        return rc, n_bad, rows, abc

    def r1cs_check(self, x, w, max_rows=16, residuals=False, on_device=False, solve=False):
        """pm_r1cs_check: one assignment, x (m0, 4) / w (mw, 4) host limbs or device pointers; solve as in r1cs_check_batch.
        -> (status, n_bad, rows[max_rows], abc or None)."""
        if on_device:
            px, pw = ct.c_void_p(x), ct.c_void_p(w)
        else:
            x = _c(x)
            w = _c(w) if np.size(w) else np.zeros((1, 4), dtype=np.uint64)
            px, pw = x.ctypes.data_as(ct.c_void_p), w.ctypes.data_as(ct.c_void_p)
        max_rows = int(max_rows)
        n_bad = np.zeros(1, dtype=np.uint64)
        rows = np.full(max_rows, np.iinfo(np.uint64).max, dtype=np.uint64)
        abc = np.zeros((max_rows, 3, 4), dtype=np.uint64) if residuals else None
        rc = self.ctx.L.pm_r1cs_check(self.ctx.h, self.h, px, pw, int(bool(on_device)) | (ASSIGNMENT_SOLVE if solve else 0), max_rows, _p(n_bad), _p(rows) if rows.size else None,
                                      _p(abc) if residuals and abc.size else None)
        return rc, int(n_bad[0]), rows, abc

    def phase2(self, x1):
        out = np.zeros(4, dtype=np.uint64)
        rc = self.ctx.L.pm_prove_phase2(self.ctx.h, _p(_c(x1)), _p(out))
        return rc, out

    def phase3(self, x1, x2, a_at_x1, c_at_x1):
        d = np.zeros(2 * self.nq, dtype=np.uint64)
        di = ct.c_int(0)
        rc = self.ctx.L.pm_prove_phase3(self.ctx.h, _p(_c(x1)), _p(_c(x2)), _p(_c(a_at_x1)), _p(_c(c_at_x1)), _p(d), ct.byref(di))
        return rc, d, di.value

    def tap(self, which, max_elems):
        out = np.zeros((max_elems, 4), dtype=np.uint64)
        n = ct.c_size_t(0)
        self.ctx.check(self.ctx.L.pm_prove_tap(self.ctx.h, which, _p(out), max_elems, ct.byref(n)))
        return out[:min(n.value, max_elems)]

    def solve_results(self, count):
        """pm_prove_tap(9) after a call with solve=True over `count` assignments on this key's context
        -> (np.uint64[count] stuck row or NOT_STUCK, np.uint64[count, m0, 4] completed public inputs, Montgomery limbs, zeros where stuck)."""
        rec = self.tap(9, count * (1 + self.m0)).reshape(count, 1 + self.m0, 4)
        return rec[:, 0, 0].copy(), rec[:, 1:, :].copy()

    def glue_challenges(self, count):
        """pm_prove_tap(11) after host_prove_batch(glue="device") over `count` proofs on this key's context
        -> np.uint64[count, 4, 4]: x1, x2, a(x1), c(x1) of every proof, Montgomery limbs, zeros for a refused row."""
        return self.tap(11, 4 * count).reshape(count, 4, 4)

    def solved_assignments(self, count, mw):
        """pm_prove_tap(10) after r1cs_check[_batch](solve=True) over `count` assignments -> np.uint64[count, m0 + mw, 4], the completed
        x || w rows (a stuck assignment's row is undefined)."""
        return self.tap(10, count * (self.m0 + mw)).reshape(count, self.m0 + mw, 4)

    def free(self):
        if self.h and not getattr(self, "_view", False):
            self.ctx.L.pm_pk_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
