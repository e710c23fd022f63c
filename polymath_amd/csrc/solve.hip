// PM_ASSIGNMENT_SOLVE: complete partial assignments on the device by forward propagation through the key's resident constraint rows
// (include/polymath_hip.h), so that a caller supplies only the values it chooses and the library computes the rest
// before it checks or proves.  The PLAN -- which row determines which column, in which order -- is host work, done once per (key,
// pattern) by host/solve_plan.hpp; the arithmetic is the kernels below, assignment = grid y (or the lane, in the chain kernel):
//   k_solve_pattern   one lane per (column, assignment): the unknown pattern of assignment 0 (a byte per column: 1 the unknown
//                     marker, 2 the quotient marker, 3 the indicator marker); every other assignment is compared with it, byte for byte, and the first
//                     differing (assignment, column) lowers one word
//   k_solve_inv       one lane per step, once per plan: 1 / coefficient of the step's unknown (a division row: 1 / cq); two more
//                     lanes per is-zero pair: 1 / cm and 1 / cb of its opener; an indicator step needs none and its record is left alone
//   k_solve_level     a WIDE dependency level: one lane per (step, assignment); a level is its own launch, so stream order is
//                     the dependency order
//   k_solve_bits      the bit decompositions of a wide level, one lane per (step, assignment) as well: a launch of their own, so
//                     that lanes doing one store do not sit beside lanes doing k
//   k_solve_iszero    the is-zero pairs of a wide level, one lane per (step, assignment) as well: two stores and one inversion each
//   k_solve_divrem    the division rows of a wide level, one lane per (step, assignment) as well: two stores and one 256-bit
//                     integer division each (divrem.cuh: a fixed trip count, so a wave does not diverge on operand size)
//   k_solve_indicator the indicator rows of a wide level, one lane per (step, assignment) as well: one dot product over the guard's
//                     known side, a zero test and one store of field one under a mask; no division
//   k_solve_chain     a run of consecutive NARROW levels: one lane per assignment walks the run's steps in plan order.  A lane
//                     reads back only its own stores: no barriers, no fences.  The MiMC shape (depth 644, width 1) is one such run
//                     and the batch is its parallel dimension.
// The solving kernels exist twice: DIV = false for ranges of kind-C steps only, DIV = true for ranges with kind-A / kind-B steps,
// or is-zero pairs, which call inverse<P> (a Fermat chain) -- the plan sorts a level by kind, so kind-C ranges do not carry its
// registers, and the is-zero step and the division step (a dividing one by the plan's count, for 1 / cq) exist in the DIV = true
// chain only.  The indicator step does not divide: it is a branch of BOTH chain instantiations.
//   k_solve_stuck_row after the launches of a REORDERED plan (build_plan_any_order found a dependency order that is not the matrix
//                     order): one lane per assignment turns the stuck word's (level, row) into the row
// A step that would divide by zero stores zero and lowers the assignment's stuck word to its row (64-bit atomic minimum: the same
// word on every run); so does a decomposition whose value has no k-bit form, in all its k columns, and a division row whose
// divisor is zero, in both its columns.  In matrix order everything
// downstream of a stuck row has a larger row, so the minimum is the root cause.  Under a reordered plan that is false -- a step that
// reads the stored zero may stick too, at a smaller row -- so the word is lowered to (level << 32) | row there: the minimum is the
// stuck step of lowest level, then smallest row, which read only valid values, and k_solve_stuck_row leaves its row in the word.  Every other store has one
// writer.  An is-zero pair never sticks: where the tested value is zero its multiplier is free and is stored as zero.  Plain C++ and
// vector stores only.
#include <cstring>
#include <vector>

#include "internal.h"
#include "prove_common.cuh"
#include "divrem.cuh"

namespace pm {

constexpr uint64_t SOLVE_NONE = ~(uint64_t)0;   // no stuck row / no mismatch / no entry to skip

template <class P>
struct SolveStepDev {
    uint64_t pos;                    // the unknown's entry in its matrix; a decomposition: the entry that holds c
    uint32_t row, col, kind, bits;   // bits != 0: a decomposition into the columns bit_cols[col .. col + bits), exponent order;
                                     // kind == KIND_ISZERO: row = the closer, pos / col = the flag's entry in it, bits = its SolvePairDev
                                     // kind == KIND_DIVREM: pos / col = the quotient's entry, inv = 1 / cq, bits = its SolveDivDev
                                     // kind == KIND_INDICATOR: pos / col = the indicator's entry, bits = 1: it lies in B_r and K = A_r,
                                     //                         0: the other way round; inv is not set
    Fp<P> inv;                       // 1 / coefficient (k_solve_inv)
    uint32_t level, pad;             // a stuck step lowers the stuck word to (level << 32) | row; level is 0 unless the plan is reordered
};

// what an is-zero step needs beside its SolveStepDev: the opener row r1
template <class P>
struct SolvePairDev {
    uint64_t pos_m, pos_c;           // (cm, m) in A_r1 or B_r1; (cb, b) in C_r1
    uint32_t row1, col_m;
    uint32_t m_in_b, b_in_b;         // K1 = A_r1 (the multiplier lies in B_r1) / K2 = A_r2 (the flag lies in B_r2); 0: the B sides
    uint32_t negated, pad;           // K2 = -K1
    Fp<P> inv_cm, inv_cb;            // k_solve_inv
};

// what a division step needs beside its SolveStepDev
struct SolveDivDev {
    uint64_t pos_r;                  // (cr, rem) in C_r
    uint32_t col_r, q_in_b;          // the remainder's column; K = A_r (the quotient lies in B_r), 0: K = B_r
};

// What a stuck step lowers the stuck word to.  The level is read HERE, on the rare path (a volatile load the compiler cannot hoist
// into the registers every step carries): the step bodies keep the registers they had.
template <class P>
__device__ __forceinline__ unsigned long long stuck_key(const SolveStepDev<P> &s) {
    const uint32_t level = *(const volatile uint32_t *)&s.level;
    return (unsigned long long)level << 32 | s.row;
}

// any of the three markers (divrem.cuh: marker_byte)
template <class P>
__device__ __forceinline__ bool is_marker(const Fp<P> &v) {
    return marker_byte<P>(v) != 0;
}

// xw: [g][ncols], the group's rows; g0 = the batch index of row 0.  pattern: one byte per column, written from assignment 0 of the
// batch (a lane per byte) and read by the groups after the first (an earlier launch wrote it); the rows that share assignment 0's
// launch compare with its values directly.
template <class P>
__global__ __launch_bounds__(256) void k_solve_pattern(const Fp<P> *xw, uint64_t ncols, uint64_t g0, uint8_t *pattern, unsigned long long *mismatch) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= ncols) return;
    const uint8_t unknown = marker_byte<P>(xw[b * ncols + j]);
    if (g0 + b == 0) {
        pattern[j] = unknown;
        return;
    }
    const uint8_t expected = g0 == 0 ? marker_byte<P>(xw[j]) : pattern[j];
    if (unknown != expected) atomicMin(mismatch, (unsigned long long)(((g0 + b) << 32) | j));
}

__device__ __forceinline__ const CsrDev &matrix_of(uint32_t kind, const CsrDev &A, const CsrDev &B, const CsrDev &Cm) {
    return kind == pmsolve::KIND_A ? A : kind == pmsolve::KIND_B ? B : Cm;
}

// KIND_BITS_x -> KIND_x
__device__ __forceinline__ uint32_t matrix_kind(uint32_t kind) { return kind >= pmsolve::KIND_BITS_C ? kind - pmsolve::KIND_BITS_C : kind; }

template <class P>
__global__ __launch_bounds__(256) void k_solve_inv(CsrDev A, CsrDev B, CsrDev Cm, SolveStepDev<P> *steps, uint64_t count, SolvePairDev<P> *pairs, uint64_t n_pairs,
                                                   const SolveDivDev *divs) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count + 2 * n_pairs) return;
    if (t < count && steps[t].kind == pmsolve::KIND_INDICATOR) return;      // no inverse: the record stays as the host wrote it
    const Fp<P> *at;
    Fp<P> *out;
    if (t < count) {                 // an is-zero step's own entry is the flag's, in the closer's A or B; a division step's the quotient's
        const uint32_t kind = steps[t].kind;
        const CsrDev &M = kind == pmsolve::KIND_ISZERO ? (pairs[steps[t].bits].b_in_b ? B : A)
                        : kind == pmsolve::KIND_DIVREM ? (divs[steps[t].bits].q_in_b ? B : A) : matrix_of(matrix_kind(kind), A, B, Cm);
        at = (const Fp<P> *)(M.val + 4 * steps[t].pos);
        out = &steps[t].inv;
    } else {
        SolvePairDev<P> &pr = pairs[(t - count) >> 1];
        const bool multiplier = ((t - count) & 1) == 0;
        at = (const Fp<P> *)(multiplier ? (pr.m_in_b ? B : A).val + 4 * pr.pos_m : Cm.val + 4 * pr.pos_c);
        out = multiplier ? &pr.inv_cm : &pr.inv_cb;
    }
    const Fp<P> coef = *at;
    *out = coef.eq(Fp<P>::one()) ? coef : inverse<P>(coef);
}

// (M z)_r without entry `skip` (SOLVE_NONE: the whole row)
template <class P>
__device__ __forceinline__ Fp<P> row_dot_skip(const CsrDev &M, const Fp<P> *z, uint64_t r, uint64_t skip) {
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = M.rowptr[r]; k < M.rowptr[r + 1]; ++k) {
        if (k == skip) continue;
        acc = add<P>(acc, mul<P>(*(const Fp<P> *)(M.val + 4 * k), z[M.col[k]]));
    }
    return acc;
}

// (M z)_r without the entries whose value is still the marker.  In a decomposition row those are exactly its k unknowns: every other
// column the row names was given (never a marker) or was stored by an earlier level or an earlier step of this lane (a field
// element, zero where that step was stuck).
template <class P>
__device__ __forceinline__ Fp<P> row_dot_unmarked(const CsrDev &M, const Fp<P> *z, uint64_t r) {
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = M.rowptr[r]; k < M.rowptr[r + 1]; ++k) {
        const Fp<P> v = z[M.col[k]];
        if (is_marker<P>(v)) continue;
        acc = add<P>(acc, mul<P>(*(const Fp<P> *)(M.val + 4 * k), v));
    }
    return acc;
}

// one step on one assignment (z = its x || w row): the partial dot products of the row, the unknown's entry left out, then
//   kind C: z_u = (Az Bz - C_rest) / coef      kind A: z_u = (Cz / Bz - A_rest) / coef      kind B: z_u = (Cz / Az - B_rest) / coef
template <class P, bool DIV>
__device__ __forceinline__ void solve_step(const CsrDev &A, const CsrDev &B, const CsrDev &Cm, const SolveStepDev<P> &s, Fp<P> *z,
                                           unsigned long long *stuck) {
    const uint64_t r = s.row;
    const uint32_t kind = s.kind;
    const Fp<P> az = row_dot_skip<P>(A, z, r, kind == pmsolve::KIND_A ? s.pos : SOLVE_NONE);
    const Fp<P> bz = row_dot_skip<P>(B, z, r, kind == pmsolve::KIND_B ? s.pos : SOLVE_NONE);
    const Fp<P> cz = row_dot_skip<P>(Cm, z, r, kind == pmsolve::KIND_C ? s.pos : SOLVE_NONE);
    Fp<P> v;
    if (!DIV || kind == pmsolve::KIND_C) {
        v = sub<P>(mul<P>(az, bz), cz);
    } else {
        const Fp<P> den = kind == pmsolve::KIND_A ? bz : az, rest = kind == pmsolve::KIND_A ? az : bz;
        if (den.is_zero()) {        // 0 / 0 included: the value is then undetermined
            atomicMin(stuck, stuck_key<P>(s));
            z[s.col] = Fp<P>::zero();
            return;
        }
        v = sub<P>(mul<P>(cz, inverse<P>(den)), rest);
    }
    z[s.col] = mul<P>(v, s.inv);
}

// one decomposition on one assignment: t = (the unknown part of the row) / c with the k unknown entries left out of the dot
// product -- their columns still hold the marker, and row_dot_unmarked passes over markers -- then z_{cols[i]} = bit i of the
// canonical integer of t, as field 0 or field 1.  t >= 2^k has no such form: stuck, like a zero divisor, with zero in all k columns.
template <class P, bool DIV>
__device__ __forceinline__ void solve_bits(const CsrDev &A, const CsrDev &B, const CsrDev &Cm, const SolveStepDev<P> &s, const uint32_t *__restrict__ bit_cols,
                                           Fp<P> *z, unsigned long long *stuck) {
    const uint64_t r = s.row;
    const uint32_t kind = matrix_kind(s.kind), k = s.bits;
    const uint32_t *cols = bit_cols + s.col;
    const Fp<P> az = kind == pmsolve::KIND_A ? row_dot_unmarked<P>(A, z, r) : row_dot_skip<P>(A, z, r, SOLVE_NONE);
    const Fp<P> bz = kind == pmsolve::KIND_B ? row_dot_unmarked<P>(B, z, r) : row_dot_skip<P>(B, z, r, SOLVE_NONE);
    const Fp<P> cz = kind == pmsolve::KIND_C ? row_dot_unmarked<P>(Cm, z, r) : row_dot_skip<P>(Cm, z, r, SOLVE_NONE);
    Fp<P> v = Fp<P>::zero();
    bool ok = true;
    if (!DIV || kind == pmsolve::KIND_C) {
        v = sub<P>(mul<P>(az, bz), cz);
    } else {
        const Fp<P> den = kind == pmsolve::KIND_A ? bz : az, rest = kind == pmsolve::KIND_A ? az : bz;
        ok = !den.is_zero();
        if (ok) v = sub<P>(mul<P>(cz, inverse<P>(den)), rest);
    }
    Fp<P> t = Fp<P>::zero();
    if (ok) {
        t = from_mont<P>(mul<P>(v, s.inv));
        uint32_t high = 0;           // the bits of t from k upwards; k <= bitlength(r) - 1 < 32 N
#pragma unroll
        for (int i = 0; i < P::N; ++i) high |= 32u * i >= k ? t.l[i] : 32u * (i + 1) > k ? t.l[i] >> (k - 32u * i) : 0u;
        ok = high == 0;
    }
    if (!ok) {
        atomicMin(stuck, stuck_key<P>(s));
        t = Fp<P>::zero();
    }
    for (uint32_t i = 0; i < k; i += 32) {
        uint32_t word = 0;
#pragma unroll
        for (int w = 0; w < P::N; ++w) word = i == 32u * w ? t.l[w] : word;   // t.l[i / 32] without indexing registers
        for (uint32_t j = i; j < k && j < i + 32; ++j) {
            const uint32_t mask = 0u - ((word >> (j - i)) & 1u);              // one & mask: field 1 or field 0, no table to select from
            Fp<P> bit;
#pragma unroll
            for (int w = 0; w < P::N; ++w) bit.l[w] = P::ONE[w] & mask;
            z[cols[j]] = bit;
        }
    }
}

// one is-zero pair on one assignment.  d1 = K1 z is the tested value up to sign, d2 = K2 z = +-d1 by the plan, so ONE inversion
// serves both rows; inverse<P>(0) is 0 (a power of zero), which is the convention for the free multiplier, so m needs no branch and
// only b is a select:
//   d1 != 0:  b = ((C_r2 z) / d2 - rest_r2) / kb,   m = ((C_r1 z, with b) / d1) / cm
//   d1 == 0:  b = -C_r1_rest / cb,                  m = 0
// Both columns still hold the marker; the dot products leave their entries out by position.
template <class P>
__device__ __forceinline__ void solve_iszero(const CsrDev &A, const CsrDev &B, const CsrDev &Cm, const SolveStepDev<P> &s, const SolvePairDev<P> &pr, Fp<P> *z) {
    const uint64_t r1 = pr.row1, r2 = s.row;
    const Fp<P> d1 = row_dot_skip<P>(pr.m_in_b ? A : B, z, r1, SOLVE_NONE);
    const Fp<P> c1_rest = row_dot_skip<P>(Cm, z, r1, pr.pos_c);
    const Fp<P> rest2 = row_dot_skip<P>(pr.b_in_b ? B : A, z, r2, s.pos);
    const Fp<P> c2 = row_dot_skip<P>(Cm, z, r2, SOLVE_NONE);
    const Fp<P> inv1 = inverse<P>(d1);
    const Fp<P> inv2 = pr.negated ? neg<P>(inv1) : inv1;
    const Fp<P> b_unequal = mul<P>(sub<P>(mul<P>(c2, inv2), rest2), s.inv);
    const Fp<P> b_equal = mul<P>(neg<P>(c1_rest), pr.inv_cb);
    const Fp<P> b = d1.is_zero() ? b_equal : b_unequal;
    const Fp<P> c1 = add<P>(c1_rest, mul<P>(*(const Fp<P> *)(Cm.val + 4 * pr.pos_c), b));
    z[s.col] = b;
    z[pr.col_m] = mul<P>(mul<P>(c1, inv1), pr.inv_cm);
}

// one division row on one assignment: cq q (K z) = R - cq rem, so with d = K z and a = R / cq as canonical integers
//   d != 0:  q = floor(a / d),  rem = a mod d      (euclid_divrem: Montgomery -> canonical, 256 / 256 bits, back)
//   d == 0:  stuck at the row, zero in both columns
// The partial dot products as the is-zero step forms them: K's whole row and C's without rem's entry; the quotient's side has no
// other non-zero entry, so its partial dot product is zero and is not formed.  Both columns still hold their markers.
template <class P>
__device__ __forceinline__ void solve_divrem(const CsrDev &A, const CsrDev &B, const CsrDev &Cm, const SolveStepDev<P> &s, const SolveDivDev &dv, Fp<P> *z,
                                             unsigned long long *stuck) {
    const uint64_t r = s.row;
    const Fp<P> d = row_dot_skip<P>(dv.q_in_b ? A : B, z, r, SOLVE_NONE);
    const Fp<P> a = mul<P>(row_dot_skip<P>(Cm, z, r, dv.pos_r), s.inv);
    Fp<P> q = Fp<P>::zero(), rem = Fp<P>::zero();
    if (!euclid_divrem<P>(a, d, &q, &rem)) atomicMin(stuck, stuck_key<P>(s));
    z[s.col] = q;
    z[dv.col_r] = rem;
}

// one indicator row on one assignment: z_u = [K z == 0] as field one or field zero, whatever u's coefficient is.  K's whole row (the
// indicator's side has no other non-zero entry and C_r none at all); the column still holds its marker.  No division, never stuck.
template <class P>
__device__ __forceinline__ void solve_indicator(const CsrDev &A, const CsrDev &B, const SolveStepDev<P> &s, Fp<P> *z) {
    z[s.col] = indicator_of<P>(row_dot_skip<P>(s.bits ? A : B, z, s.row, SOLVE_NONE));
}

template <class P, bool DIV>
__global__ __launch_bounds__(256) void k_solve_level(CsrDev A, CsrDev B, CsrDev Cm, const SolveStepDev<P> *__restrict__ steps, uint32_t lo, uint32_t hi,
                                                     Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_step<P, DIV>(A, B, Cm, steps[t], xw + b * ncols, stuck + b);
}

template <class P, bool DIV>
__global__ __launch_bounds__(256) void k_solve_bits(CsrDev A, CsrDev B, CsrDev Cm, const SolveStepDev<P> *__restrict__ steps, const uint32_t *__restrict__ bit_cols,
                                                    uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_bits<P, DIV>(A, B, Cm, steps[t], bit_cols, xw + b * ncols, stuck + b);
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_iszero(CsrDev A, CsrDev B, CsrDev Cm, const SolveStepDev<P> *__restrict__ steps, const SolvePairDev<P> *__restrict__ pairs,
                                                      uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_iszero<P>(A, B, Cm, steps[t], pairs[steps[t].bits], xw + b * ncols);
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_divrem(CsrDev A, CsrDev B, CsrDev Cm, const SolveStepDev<P> *__restrict__ steps, const SolveDivDev *__restrict__ divs,
                                                      uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_divrem<P>(A, B, Cm, steps[t], divs[steps[t].bits], xw + b * ncols, stuck + b);
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_indicator(CsrDev A, CsrDev B, const SolveStepDev<P> *__restrict__ steps, uint32_t lo, uint32_t hi, Fp<P> *xw,
                                                         uint64_t ncols) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_indicator<P>(A, B, steps[t], xw + b * ncols);
}

// the step index is the same in every lane: the step record, the pair record, the row's CSR metadata and a decomposition's column
// list are uniform loads.  A range with an is-zero pair or a division row is a dividing one (the plan says so): the DIV = false body
// has no such branches.  An indicator row does not divide and is a branch of both.
template <class P, bool DIV>
__global__ __launch_bounds__(64) void k_solve_chain(CsrDev A, CsrDev B, CsrDev Cm, const SolveStepDev<P> *__restrict__ steps, const uint32_t *__restrict__ bit_cols,
                                                    const SolvePairDev<P> *__restrict__ pairs, const SolveDivDev *__restrict__ divs, uint32_t lo, uint32_t hi,
                                                    Fp<P> *xw, uint64_t ncols, unsigned long long *stuck, uint64_t rows) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    Fp<P> *z = xw + b * ncols;
    for (uint32_t t = lo; t < hi; ++t) {
        if (steps[t].kind == pmsolve::KIND_ISZERO) {
            // DIV = false would pass over the pair and leave both markers in place: solve_plan refuses a plan that asks for that
            if constexpr (DIV) solve_iszero<P>(A, B, Cm, steps[t], pairs[steps[t].bits], z);
        } else if (steps[t].kind == pmsolve::KIND_DIVREM) {
            if constexpr (DIV) solve_divrem<P>(A, B, Cm, steps[t], divs[steps[t].bits], z, stuck + b);      // as above
        } else if (steps[t].kind == pmsolve::KIND_INDICATOR) {
            solve_indicator<P>(A, B, steps[t], z);
        } else if (steps[t].bits) solve_bits<P, DIV>(A, B, Cm, steps[t], bit_cols, z, stuck + b);
        else solve_step<P, DIV>(A, B, Cm, steps[t], z, stuck + b);
    }
}

// After the last launch of a REORDERED plan: the stuck word (level << 32) | row of the root cause becomes its row, which is what
// every reader of the word expects.  One lane per assignment.
__global__ __launch_bounds__(256) void k_solve_stuck_row(unsigned long long *stuck, uint64_t rows) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    const unsigned long long w = stuck[b];
    if (w != SOLVE_NONE) stuck[b] = w & 0xffffffffull;
}

namespace {

inline CsrDev csr_dev(const pm_pk *pk, int i) { return CsrDev{pk->d_rowptr[i], pk->d_col[i], pk->d_val[i]}; }

}  // namespace

template <class C>
int solve_begin(pm_ctx *ctx, const pm_pk *pk, size_t count) {
    SolveWs &sv = ctx->sv;
    const uint64_t ncols = pk->m0 + pk->mw;
    sv.tap9.clear();
    sv.tap10_rows = sv.tap10_cols = 0;
    if (count == 0 || count > 0xffffffffull || pk->nr > 0xffffffffull || ncols > 0xffffffffull) {
        ctx->err = "pm solve: more than 2^32 - 1 assignments, rows or columns";
        return PM_ERR_INVALID_ARG;
    }
    PM_HIP(ctx, sv.pattern.reserve(ncols));
    PM_HIP(ctx, sv.mismatch.reserve(sizeof(unsigned long long)));
    PM_HIP(ctx, hipMemsetAsync(sv.mismatch.p, 0xff, sizeof(unsigned long long), ctx->stream));
    sv.tap9.assign(count * 4 * (1 + pk->m0), 0);
    return PM_OK;
}

template <class C>
int solve_load(pm_ctx *ctx, const pm_pk *pk, Fp<typename C::FrP> *d_xw, size_t g, size_t g0, const uint64_t *x, const uint64_t *w, bool on_device) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const uint64_t m0 = pk->m0, mw = pk->mw, ncols = m0 + mw;
    if (g == 0 || g > 65535) return PM_ERR_INVALID_ARG;
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // rows of x (m0) and of w (mw) interleave into rows of x || w; the caller's arrays are only read
    PM_HIP(ctx, hipMemcpy2DAsync(d_xw, ncols * sizeof(Fr), x + 4 * m0 * g0, m0 * sizeof(Fr), m0 * sizeof(Fr), g, kind, st));
    if (mw) PM_HIP(ctx, hipMemcpy2DAsync(d_xw + m0, ncols * sizeof(Fr), w + 4 * mw * g0, mw * sizeof(Fr), mw * sizeof(Fr), g, kind, st));
    PM_LAUNCH(ctx, k_solve_pattern<P>, dim3(nblk(ncols), (unsigned)g), dim3(256), 0, st, d_xw, ncols, (uint64_t)g0, ctx->sv.pattern.as<uint8_t>(),
                   ctx->sv.mismatch.as<unsigned long long>());
    return PM_OK;
}

template <class C>
int solve_plan(pm_ctx *ctx, const pm_pk *pk) {
    typedef typename C::FrP P;
    SolveWs &sv = ctx->sv;
    const uint64_t ncols = pk->m0 + pk->mw, nr = pk->nr;
    hipStream_t st = ctx->stream;
    std::vector<uint8_t> pattern(ncols);
    unsigned long long mismatch = SOLVE_NONE;
    PM_HIP(ctx, hipMemcpyAsync(pattern.data(), sv.pattern.p, ncols, hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipMemcpyAsync(&mismatch, sv.mismatch.p, sizeof mismatch, hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    if (pattern[0]) {
        ctx->err = "pm solve: column 0 (the constant one) is marked unknown";
        return PM_ERR_INVALID_ARG;
    }
    if (mismatch != SOLVE_NONE) {
        ctx->err = "pm solve: assignment " + std::to_string(mismatch >> 32) + " differs from assignment 0 at column " + std::to_string(mismatch & 0xffffffffull) +
                   ": every assignment of a batch must mark the same columns";
        return PM_ERR_INVALID_ARG;
    }
    if (sv.plan_key == pk->serial && sv.plan_pattern == pattern) return PM_OK;
    sv.plan_key = 0;
    // the key's matrices come down once per plan: the key keeps no host copy
    std::vector<uint64_t> rowptr[3], val[3];
    std::vector<uint32_t> col[3];
    pmsolve::Csr m[3];
    for (int i = 0; i < 3; ++i) {
        const uint64_t nnz = pk->nnz[i];
        rowptr[i].resize(nr + 1);
        col[i].resize(nnz ? nnz : 1);
        val[i].resize(nnz ? 4 * nnz : 4);
        PM_HIP(ctx, hipMemcpyAsync(rowptr[i].data(), pk->d_rowptr[i], (nr + 1) * 8, hipMemcpyDeviceToHost, st));
        if (nnz) {
            PM_HIP(ctx, hipMemcpyAsync(col[i].data(), pk->d_col[i], nnz * 4, hipMemcpyDeviceToHost, st));
            PM_HIP(ctx, hipMemcpyAsync(val[i].data(), pk->d_val[i], nnz * 32, hipMemcpyDeviceToHost, st));
        }
        m[i] = pmsolve::Csr{rowptr[i].data(), col[i].data(), val[i].data()};
    }
    PM_HIP(ctx, hipStreamSynchronize(st));
    uint64_t modulus[4];
    for (int i = 0; i < 4; ++i) modulus[i] = (uint64_t)P::MOD[2 * i] | (uint64_t)P::MOD[2 * i + 1] << 32;
    sv.plan = pmsolve::build_plan_any_order(m, nr, pk->m0, pk->mw, pattern.data(), pmsolve::WIDE_STEPS, modulus);
    if (sv.plan.error != pmsolve::OK) {
        ctx->err = "pm solve: " + sv.plan.message;
        return PM_ERR_INVALID_ARG;
    }
    // the DIV = false kernels have no is-zero step and no division step in them: a range with one must be a dividing one
    for (const pmsolve::Launch &l : sv.plan.launches)
        for (uint32_t t = l.lo; t < l.hi && !l.divides; ++t)
            if (sv.plan.steps[t].kind == pmsolve::KIND_ISZERO || sv.plan.steps[t].kind == pmsolve::KIND_DIVREM) {
                ctx->err = std::string("pm solve: the plan puts the ") + (sv.plan.steps[t].kind == pmsolve::KIND_ISZERO ? "is-zero pair" : "division") + " of row " +
                           std::to_string(sv.plan.steps[t].row) + " into a launch that does not divide";
                return PM_ERR_STATE;
            }
    const size_t n_steps = sv.plan.steps.size();
    sv.n_pairs = sv.n_divs = 0;
    if (n_steps) {
        std::vector<SolveStepDev<P>> host(n_steps);
        std::vector<SolvePairDev<P>> host_pairs;
        std::vector<SolveDivDev> host_divs;
        memset((void *)host.data(), 0, n_steps * sizeof(SolveStepDev<P>));
        for (size_t t = 0; t < n_steps; ++t) {
            const pmsolve::Step &s = sv.plan.steps[t];
            host[t].pos = s.pos; host[t].row = s.row; host[t].col = s.bits ? s.cols_off : s.col; host[t].kind = s.kind; host[t].bits = s.bits;
            host[t].level = sv.plan.reordered ? s.level : 0;
            if (s.kind == pmsolve::KIND_INDICATOR) host[t].bits = s.cols_off;
            if (s.kind == pmsolve::KIND_DIVREM) {
                const pmsolve::DivRow &row = sv.plan.divs[s.cols_off];
                host[t].bits = (uint32_t)host_divs.size();
                host_divs.push_back(SolveDivDev{row.pos_r, row.col_r, row.q_in_b});
            }
            if (s.kind != pmsolve::KIND_ISZERO) continue;
            host[t].bits = (uint32_t)host_pairs.size();
            SolvePairDev<P> pr;
            memset((void *)&pr, 0, sizeof pr);
            const pmsolve::PairRows &rows = sv.plan.pairs[s.cols_off];
            pr.pos_m = rows.pos_m; pr.pos_c = rows.pos_c; pr.row1 = rows.row1; pr.col_m = rows.col_m; pr.m_in_b = rows.m_in_b; pr.b_in_b = rows.b_in_b;
            pr.negated = rows.negated;
            host_pairs.push_back(pr);
        }
        sv.n_pairs = host_pairs.size();
        if (sv.n_pairs) {
            PM_HIP(ctx, sv.pairs.reserve(sv.n_pairs * sizeof(SolvePairDev<P>)));
            PM_HIP(ctx, hipMemcpyAsync(sv.pairs.p, host_pairs.data(), sv.n_pairs * sizeof(SolvePairDev<P>), hipMemcpyHostToDevice, st));
        }
        sv.n_divs = host_divs.size();
        if (sv.n_divs) {
            PM_HIP(ctx, sv.divs.reserve(sv.n_divs * sizeof(SolveDivDev)));
            PM_HIP(ctx, hipMemcpyAsync(sv.divs.p, host_divs.data(), sv.n_divs * sizeof(SolveDivDev), hipMemcpyHostToDevice, st));
        }
        const std::vector<uint32_t> &bit_cols = sv.plan.bit_cols;
        if (!bit_cols.empty()) {
            PM_HIP(ctx, sv.bit_cols.reserve(bit_cols.size() * sizeof(uint32_t)));
            PM_HIP(ctx, hipMemcpyAsync(sv.bit_cols.p, bit_cols.data(), bit_cols.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        PM_HIP(ctx, sv.steps.reserve(n_steps * sizeof(SolveStepDev<P>)));
        PM_HIP(ctx, hipMemcpyAsync(sv.steps.p, host.data(), n_steps * sizeof(SolveStepDev<P>), hipMemcpyHostToDevice, st));
        PM_LAUNCH(ctx, k_solve_inv<P>, dim3(nblk(n_steps + 2 * sv.n_pairs)), dim3(256), 0, st, csr_dev(pk, 0), csr_dev(pk, 1), csr_dev(pk, 2),
                       sv.steps.as<SolveStepDev<P>>(), (uint64_t)n_steps, sv.n_pairs ? sv.pairs.as<SolvePairDev<P>>() : nullptr, (uint64_t)sv.n_pairs,
                       sv.n_divs ? sv.divs.as<SolveDivDev>() : nullptr);
        PM_HIP(ctx, hipStreamSynchronize(st));   // `host`, `host_pairs` and `host_divs` go out of scope
    }
    sv.plan_pattern.swap(pattern);
    sv.plan_key = pk->serial;
    return PM_OK;
}

template <class C>
int solve_group(pm_ctx *ctx, const pm_pk *pk, Fp<typename C::FrP> *d_xw, size_t g, size_t g0, int timing_slot) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    SolveWs &sv = ctx->sv;
    const uint64_t m0 = pk->m0, ncols = m0 + pk->mw;
    if (g == 0 || g > 65535 || sv.plan_key != pk->serial || (g0 + g) * 4 * (1 + m0) > sv.tap9.size()) return PM_ERR_STATE;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    PM_HIP(ctx, sv.stuck.reserve(g * sizeof(unsigned long long)));
    unsigned long long *stuck = sv.stuck.as<unsigned long long>();
    PM_HIP(ctx, hipMemsetAsync(stuck, 0xff, g * sizeof(unsigned long long), st));
    const CsrDev A = csr_dev(pk, 0), B = csr_dev(pk, 1), Cm = csr_dev(pk, 2);
    const SolveStepDev<P> *steps = sv.steps.as<SolveStepDev<P>>();
    const uint32_t *bit_cols = sv.plan.bit_cols.empty() ? nullptr : sv.bit_cols.as<uint32_t>();
    const SolvePairDev<P> *pairs = sv.n_pairs ? sv.pairs.as<SolvePairDev<P>>() : nullptr;
    const SolveDivDev *divs = sv.n_divs ? sv.divs.as<SolveDivDev>() : nullptr;
    {
        StageTimer t(ctx, timing_slot);
        for (const pmsolve::Launch &l : sv.plan.launches) {
            if (l.chain) {
                const dim3 grid(nblk(g, 64)), block(64);
                if (l.divides) hipLaunchKernelGGL((k_solve_chain<P, true>), grid, block, 0, st, A, B, Cm, steps, bit_cols, pairs, divs, l.lo, l.hi, d_xw, ncols, stuck, (uint64_t)g);
                else hipLaunchKernelGGL((k_solve_chain<P, false>), grid, block, 0, st, A, B, Cm, steps, bit_cols, pairs, divs, l.lo, l.hi, d_xw, ncols, stuck, (uint64_t)g);
            } else {
                const dim3 grid(nblk(l.hi - l.lo), (unsigned)g), block(256);
                if (l.indicator) hipLaunchKernelGGL((k_solve_indicator<P>), grid, block, 0, st, A, B, steps, l.lo, l.hi, d_xw, ncols);
                else if (l.divrem) hipLaunchKernelGGL((k_solve_divrem<P>), grid, block, 0, st, A, B, Cm, steps, divs, l.lo, l.hi, d_xw, ncols, stuck);
                else if (l.iszero) hipLaunchKernelGGL((k_solve_iszero<P>), grid, block, 0, st, A, B, Cm, steps, pairs, l.lo, l.hi, d_xw, ncols);
                else if (l.bits && l.divides) hipLaunchKernelGGL((k_solve_bits<P, true>), grid, block, 0, st, A, B, Cm, steps, bit_cols, l.lo, l.hi, d_xw, ncols, stuck);
                else if (l.bits) hipLaunchKernelGGL((k_solve_bits<P, false>), grid, block, 0, st, A, B, Cm, steps, bit_cols, l.lo, l.hi, d_xw, ncols, stuck);
                else if (l.divides) hipLaunchKernelGGL((k_solve_level<P, true>), grid, block, 0, st, A, B, Cm, steps, l.lo, l.hi, d_xw, ncols, stuck);
                else hipLaunchKernelGGL((k_solve_level<P, false>), grid, block, 0, st, A, B, Cm, steps, l.lo, l.hi, d_xw, ncols, stuck);
            }
            PM_HIP(ctx, hipGetLastError());
        }
        if (sv.plan.reordered) PM_LAUNCH(ctx, k_solve_stuck_row, dim3(nblk(g)), dim3(256), 0, st, stuck, (uint64_t)g);
    }
    // the small results: per assignment the stuck word and the completed instance -> tap 9
    std::vector<unsigned long long> h_stuck(g);
    uint64_t *tap = sv.tap9.data() + g0 * 4 * (1 + m0);
    PM_HIP(ctx, hipMemcpyAsync(h_stuck.data(), stuck, g * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipMemcpy2DAsync(tap + 4, (1 + m0) * sizeof(Fr), d_xw, ncols * sizeof(Fr), m0 * sizeof(Fr), g, hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    for (size_t b = 0; b < g; ++b) {
        uint64_t *row = tap + b * 4 * (1 + m0);
        row[0] = h_stuck[b];
        row[1] = row[2] = row[3] = 0;
        if (h_stuck[b] != SOLVE_NONE) memset(row + 4, 0, m0 * sizeof(Fr));
    }
    return PM_OK;
}

template <class C>
int solve_all(pm_ctx *ctx, const pm_pk *pk, size_t count, const uint64_t *x, const uint64_t *w, bool on_device, size_t group, int timing_slot) {
    typedef Fp<typename C::FrP> Fr;
    const uint64_t ncols = pk->m0 + pk->mw;
    if (group < 1) group = 1;
    if (group > 65535) group = 65535;
    PM_TRY(solve_begin<C>(ctx, pk, count));
    PM_HIP(ctx, ctx->sv.xw.reserve(count * ncols * sizeof(Fr)));
    Fr *xw = ctx->sv.xw.as<Fr>();
    for (size_t g0 = 0; g0 < count; g0 += group)
        PM_TRY(solve_load<C>(ctx, pk, xw + g0 * ncols, count - g0 < group ? count - g0 : group, g0, x, w, on_device));
    PM_TRY(solve_plan<C>(ctx, pk));
    for (size_t g0 = 0; g0 < count; g0 += group)
        PM_TRY(solve_group<C>(ctx, pk, xw + g0 * ncols, count - g0 < group ? count - g0 : group, g0, timing_slot));
    ctx->sv.tap10_rows = count;
    ctx->sv.tap10_cols = ncols;
    return PM_OK;
}

#define PM_INST(C)                                                                                                             \
    template int solve_begin<C>(pm_ctx *, const pm_pk *, size_t);                                                              \
    template int solve_load<C>(pm_ctx *, const pm_pk *, Fp<typename C::FrP> *, size_t, size_t, const uint64_t *, const uint64_t *, bool); \
    template int solve_plan<C>(pm_ctx *, const pm_pk *);                                                                       \
    template int solve_group<C>(pm_ctx *, const pm_pk *, Fp<typename C::FrP> *, size_t, size_t, int);                         \
    template int solve_all<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, bool, size_t, int);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
