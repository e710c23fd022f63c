// The witness solver's STEP BODIES (solve.hip: the kernels that call them): what one step of a plan does to one
// assignment, the record a step is on the device and how those records are filled from a pmsolve::Plan.  ONE text for device and
// host, like field.cuh and divrem.cuh: the kernels call these bodies per (step, assignment), and the CPU self-tests
// (tests/native/solve_selftest.hpp) walk a plan's launches through the same bodies on the host field type.
//
// The one thing the two sides cannot share is what a stuck step does to the assignment's stuck word (a 64-bit atomic minimum on the
// device, a plain minimum on the host), so the bodies take that action as a SINK: an object called with the step record, at the
// place where the store used to be.  Plain C++ and vector stores only.
#pragma once
#include <cstring>
#include <vector>

#include "../host/solve_plan.hpp"
#include "divrem.cuh"
#include "field.cuh"
#include "sqrt.cuh"

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
                                     // kind == KIND_SQRT: pos / col = the root's entry in A_r, bits = the offset of its entry in B_r from
                                     //                    that row's start, inv = 1 / (ka kb)
    Fp<P> inv;                       // 1 / coefficient (solve_inverse)
    uint32_t level, pad;             // a stuck step lowers the stuck word to (level << 32) | row; level is 0 unless the plan is reordered
};

// what an is-zero step needs beside its SolveStepDev: the opener row r1
template <class P>
struct SolvePairDev {
    uint64_t pos_m, pos_c;           // (cm, m) in A_r1 or B_r1; (cb, b) in C_r1
    uint32_t row1, col_m;
    uint32_t m_in_b, b_in_b;         // K1 = A_r1 (the multiplier lies in B_r1) / K2 = A_r2 (the flag lies in B_r2); 0: the B sides
    uint32_t negated, pad;           // K2 = -K1
    Fp<P> inv_cm, inv_cb;            // solve_inverse
};

// what a division step needs beside its SolveStepDev
struct SolveDivDev {
    uint64_t pos_r;                  // (cr, rem) in C_r
    uint32_t col_r, q_in_b;          // the remainder's column; K = A_r (the quotient lies in B_r), 0: K = B_r
};

// what a block step needs beside its SolveStepDev (whose bits = its SolveBlockDev): k rows and k columns, both ascending, in the index
// pool, and the inverse of its matrix in the inverse pool, k x k elements stored TRANSPOSED (InvT[i][j] = Inv[j][i]: the lanes j of a
// wave read consecutive elements).  Blocks with the same matrix share an inverse.
struct SolveBlockDev {
    uint32_t k, rows_off, cols_off, pad;
    uint64_t inv_off;                // in elements
};

// what a long-division step needs beside its SolveStepDev (whose bits = its SolveHintDev): in the hint pool from `off` the kq quotient
// columns, the kr remainder columns, the kD dividend columns, then the kE divisor columns -- or, literal != 0, the 16 words of the
// divisor's literal limbs accumulated at bit offset n j and one word that is non-zero where they reach 2^512 (solve_records forms both)
struct SolveHintDev {
    uint32_t n, kq, kr, kD, kE, literal, off, pad;
};

// what a modular-division step needs beside its SolveStepDev (whose bits = its SolveModDev): in the hint pool from `off` the kz output
// columns, the kNp, kNm, kDp and kDm operand columns, then the kP modulus columns -- or, literal != 0, the 16 words of the modulus'
// literal limbs accumulated at bit offset n j and one word that is non-zero where they reach 2^512, as for a literal divisor
// A WIDE long-division step (KIND_LONGDIV_WIDE) has a SolveHintDev as well, in the same array; its literal divisor is 128 pool words
// and the word that is non-zero where the limbs reach 2^4096.
struct SolveModDev {
    uint32_t n, kz, k[4], kP, literal, off, pad;
};

// what a modular multiply-divide step needs beside its SolveStepDev (whose bits = its SolveMulDev): in the hint pool from `off` the kz
// output columns, the kA, kB, kNp, kNm, kDp and kDm operand columns, then the kP modulus columns or the 17 words of a literal modulus
// as above; cN and cD, the two one-word literals
struct SolveMulDev {
    uint32_t n, kz, k[6], kP, literal, off, cN, cD, pad;
};

// The record arrays of a plan, as the kernels read them; the inverses are left zero (solve_inverse fills them), the pool of block
// inverses empty (solve_block_inverses fills it).
template <class P>
struct SolveRecords {
    std::vector<SolveStepDev<P>> steps;
    std::vector<SolvePairDev<P>> pairs;
    std::vector<SolveDivDev> divs;
    std::vector<SolveBlockDev> blocks;
    std::vector<uint32_t> block_idx;      // the blocks' rows and columns
    std::vector<uint64_t> mat_off;        // per distinct matrix: where its inverse begins in block_inv; one more entry: the pool's size
    std::vector<Fp<P>> block_inv;         // the inverse pool
    std::vector<SolveHintDev> hints;
    std::vector<uint32_t> hint_idx;       // the hint pool
    std::vector<SolveModDev> mods;        // the modular divisions; their columns and literal moduli are in the hint pool too
    std::vector<SolveMulDev> muls;        // the modular multiply-divides; their columns and literal moduli are in the hint pool as well
};

constexpr int LONGDIV_WD = 32, LONGDIV_WE = 16;   // the long division's registers in 32-bit words: a 1024-bit dividend, a 512-bit divisor
// the WIDE long division's operands in 32-bit words: an 8192-bit dividend and a 4096-bit divisor, and the words their limb sums are
// formed in -- ten more, since kD limbs below 2^256 at bit offsets up to 8191 stay below 2^(8191 + 256 + 7); a sum that reaches into
// those ten is D >= 2^8192 (E >= 2^4096)
constexpr int WIDE_WD = 256, WIDE_WE = 128, WIDE_SUM_D = WIDE_WD + 10, WIDE_SUM_E = WIDE_WE + 10;

// acc += v << off for the 256-bit v (eight words) and the W-word acc, off < 32 W.  -> non-zero where bits were lost above 32 W.  No
// register is indexed by `off`: the word of the shifted value (nine words) that falls on acc[w] is selected by comparison, W x 9 selects.
template <int W>
PM_HD uint32_t add_shifted(uint32_t (&acc)[W], const uint32_t v[8], uint32_t off) {
    const uint32_t wo = off >> 5, down = 32u - (off & 31u);   // down in 1..32: a 64-bit shift
    uint32_t s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const uint64_t pair = (uint64_t)(k < 8 ? v[k] : 0u) << 32 | (k > 0 ? v[k - 1] : 0u);
        s[k] = (uint32_t)(pair >> down);
    }
    uint32_t carry = 0, lost = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t k = (uint32_t)w - wo;
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) t = k == (uint32_t)i ? s[i] : t;
        const uint64_t sum = (uint64_t)acc[w] + t + carry;
        acc[w] = (uint32_t)sum;
        carry = (uint32_t)(sum >> 32);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) lost |= wo + (uint32_t)i >= (uint32_t)W ? s[i] : 0u;
    return lost | carry;
}

// word i of the W-word src, zero where i >= W: selected by comparison, W selects, no register indexed by i
template <int W>
PM_HD uint32_t word_at(const uint32_t (&src)[W], uint32_t i) {
    uint32_t g = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) g = (uint32_t)w == i ? src[w] : g;
    return g;
}

// the low `keep` bits of a word (keep >= 32: all of it)
PM_HD uint32_t low_bits(uint32_t word, uint32_t keep) { return word & (keep >= 32u ? ~0u : (1u << keep) - 1u); }

// The n-bit limb (n <= 128) of the W-word src at bit offset off, as a canonical element: five source words selected by comparison
// (5 W selects, held in five scalars: no private array), a 64-bit shift per output word, a mask.  Bits at and above 32 W read as zero.
template <class P, int W>
PM_HD Fp<P> limb_at(const uint32_t (&src)[W], uint32_t off, uint32_t n) {
    static_assert(P::N == 8, "four 64-bit words");
    const uint32_t wo = off >> 5, bs = off & 31u;
    const uint32_t g0 = word_at<W>(src, wo), g1 = word_at<W>(src, wo + 1), g2 = word_at<W>(src, wo + 2), g3 = word_at<W>(src, wo + 3), g4 = word_at<W>(src, wo + 4);
    Fp<P> out;
    out.l[0] = low_bits((uint32_t)(((uint64_t)g1 << 32 | g0) >> bs), n);
    out.l[1] = low_bits((uint32_t)(((uint64_t)g2 << 32 | g1) >> bs), n > 32u ? n - 32u : 0u);
    out.l[2] = low_bits((uint32_t)(((uint64_t)g3 << 32 | g2) >> bs), n > 64u ? n - 64u : 0u);
    out.l[3] = low_bits((uint32_t)(((uint64_t)g4 << 32 | g3) >> bs), n > 96u ? n - 96u : 0u);
    out.l[4] = out.l[5] = out.l[6] = out.l[7] = 0;
    return out;
}

// the bits of the W-word a from bit `from` upwards, or-ed together: non-zero where a >= 2^from
template <int W>
PM_HD uint32_t bits_from(const uint32_t (&a)[W], uint32_t from) {
    uint32_t high = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) high |= 32u * w >= from ? a[w] : 32u * (w + 1) > from ? a[w] >> (from - 32u * w) : 0u;
    return high;
}

// divrem.cuh's restoring shift-subtract on 32-bit words: num = floor(num / d) and rem = num mod d for a WD-word dividend and a
// WE-word divisor d != 0; rem has WE + 1 words (twice a remainder plus a bit may reach 2^(32 WE + 1) - 1; what is left is below d).
// The quotient is shifted into the dividend's register from the bottom, where the dividend's bits have left.  `rounds` <= 32 WD is the
// trip count, the same in every lane of a launch (the plan's bound: Launch::rounds): the dividend is below 2^rounds and comes
// SHIFTED LEFT by 32 WD - rounds, so that its bits leave the register's top from the first round on; after `rounds` rounds the
// register holds the quotient and nothing else.  Every word loop unrolled, the round loop rolled; no branch and no register index
// depends on an operand.  d == 0 gives a quotient of `rounds` ones: the caller tests for it.
template <int WD, int WE>
PM_HD void longdiv(uint32_t (&num)[WD], const uint32_t (&d)[WE], uint32_t (&rem)[WE + 1], uint32_t rounds) {
#pragma unroll
    for (int j = 0; j <= WE; ++j) rem[j] = 0;
#pragma unroll 1
    for (uint32_t round = 0; round < rounds; ++round) {
#pragma unroll
        for (int j = WE; j > 0; --j) rem[j] = rem[j] << 1 | rem[j - 1] >> 31;
        rem[0] = rem[0] << 1 | num[WD - 1] >> 31;
#pragma unroll
        for (int j = WD - 1; j > 0; --j) num[j] = num[j] << 1 | num[j - 1] >> 31;
        num[0] <<= 1;
        uint32_t t[WE + 1], borrow = 0;
#pragma unroll
        for (int j = 0; j <= WE; ++j) {
            const uint32_t dj = j < WE ? d[j < WE ? j : 0] : 0u;
            const uint32_t x = rem[j] - borrow;
            const uint32_t b1 = rem[j] < borrow;
            t[j] = x - dj;
            borrow = b1 | (uint32_t)(x < dj);
        }
        const uint32_t take = borrow ^ 1u;          // 2 rem + bit >= d
        const uint32_t mask = 0u - take;
#pragma unroll
        for (int j = 0; j <= WE; ++j) rem[j] = (t[j] & mask) | (rem[j] & ~mask);
        num[0] |= take;
    }
}

// acc += v << off for the 256-bit v (eight words) and the W words of acc in memory, off + 288 <= 32 W (nothing is lost): the wide long
// division's accumulation, where it is serial (the host's literal divisor, the CPU rig); the kernel forms the same sum by columns
PM_HD void add_shifted_words(uint32_t *acc, uint32_t W, const uint32_t v[8], uint32_t off) {
    const uint32_t wo = off >> 5, bs = off & 31u;
    uint64_t carry = 0;
    for (uint32_t k = 0; wo + k < W && (k < 9 || carry); ++k) {
        const uint64_t pair = (uint64_t)(k < 8 ? v[k] : 0u) << 32 | (k > 0 && k < 9 ? v[k - 1] : 0u);
        const uint64_t sum = (uint64_t)acc[wo + k] + (k < 9 ? (uint32_t)(pair << bs >> 32) : 0u) + carry;
        acc[wo + k] = (uint32_t)sum;
        carry = sum >> 32;
    }
}

// A literal divisor or modulus, a constant of the key, accumulated once per plan: onto `pool` the W words (16, or the wide division's
// 128) of the sum of the literal's limbs at bit offset n j, then ONE word that is non-zero exactly where the sum reaches 2^(32 W).  The
// sum is formed in WIDE_SUM_E words, which lose nothing at either width: n j + 288 <= 32 WIDE_SUM_E under both records' limits
inline void literal_words(const pmsolve::Hint &h, int W, std::vector<uint32_t> &pool) {
    static_assert(pmsolve::HINT_MAX_N * (pmsolve::HINT_MAX_KE - 1) + 288 <= 32u * WIDE_SUM_E && pmsolve::WIDE_E_BITS - 1 + 288 <= 32u * WIDE_SUM_E, "no bit is lost");
    uint32_t E[WIDE_SUM_E] = {0}, above = 0;
    for (size_t j = 0; j < h.lit.size() / 4; ++j) {
        uint32_t v[8];
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (uint32_t)h.lit[4 * j + i];
            v[2 * i + 1] = (uint32_t)(h.lit[4 * j + i] >> 32);
        }
        add_shifted_words(E, WIDE_SUM_E, v, h.n * (uint32_t)j);
    }
    for (int w = W; w < WIDE_SUM_E; ++w) above |= E[w];
    pool.insert(pool.end(), E, E + W);
    pool.push_back(above);
}

template <class P>
inline SolveRecords<P> solve_records(const pmsolve::Plan &plan) {
    SolveRecords<P> rec;
    rec.mat_off.assign(1, 0);
    for (const pmsolve::BlockMat &mat : plan.block_mats) rec.mat_off.push_back(rec.mat_off.back() + (uint64_t)mat.k * mat.k);
    const size_t n_steps = plan.steps.size();
    rec.steps.resize(n_steps);
    if (n_steps) memset((void *)rec.steps.data(), 0, n_steps * sizeof(SolveStepDev<P>));
    for (size_t t = 0; t < n_steps; ++t) {
        const pmsolve::Step &s = plan.steps[t];
        SolveStepDev<P> &d = rec.steps[t];
        d.pos = s.pos; d.row = s.row; d.col = s.bits ? s.cols_off : s.col; d.kind = s.kind; d.bits = s.bits;
        d.level = plan.reordered ? s.level : 0;
        if (s.kind == pmsolve::KIND_INDICATOR || s.kind == pmsolve::KIND_SQRT) d.bits = s.cols_off;
        if (s.kind == pmsolve::KIND_DIVREM) {
            const pmsolve::DivRow &row = plan.divs[s.cols_off];
            d.bits = (uint32_t)rec.divs.size();
            rec.divs.push_back(SolveDivDev{row.pos_r, row.col_r, row.q_in_b});
        }
        if (s.kind == pmsolve::KIND_BLOCK) {
            const pmsolve::BlockRows &blk = plan.blocks[s.cols_off];
            const uint32_t k = (uint32_t)blk.cols.size(), rows_off = (uint32_t)rec.block_idx.size();
            d.bits = (uint32_t)rec.blocks.size();
            rec.block_idx.insert(rec.block_idx.end(), blk.rows.begin(), blk.rows.end());
            rec.block_idx.insert(rec.block_idx.end(), blk.cols.begin(), blk.cols.end());
            rec.blocks.push_back(SolveBlockDev{k, rows_off, rows_off + k, 0, rec.mat_off[blk.mat]});
        }
        if (s.kind == pmsolve::KIND_LONGDIV || s.kind == pmsolve::KIND_MODDIV || s.kind == pmsolve::KIND_LONGDIV_WIDE || s.kind == pmsolve::KIND_MODMULDIV) {
            const pmsolve::Hint &h = plan.hints[s.cols_off];
            const bool literal = (h.flags & pmsolve::HINT_DIVISOR_LITERAL) != 0;   // HINT_MODULUS_LITERAL is the same bit
            const uint32_t kE = (uint32_t)(literal ? h.lit.size() / 4 : h.E.size()), off = (uint32_t)rec.hint_idx.size();
            if (s.kind == pmsolve::KIND_MODDIV) {
                d.bits = (uint32_t)rec.mods.size();
                rec.mods.push_back(SolveModDev{h.n, (uint32_t)h.q.size(), {h.k[0], h.k[1], h.k[2], h.k[3]}, kE, literal ? 1u : 0u, off, 0});
            } else if (s.kind == pmsolve::KIND_MODMULDIV) {
                d.bits = (uint32_t)rec.muls.size();
                rec.muls.push_back(SolveMulDev{h.n, (uint32_t)h.q.size(), {h.km[0], h.km[1], h.km[2], h.km[3], h.km[4], h.km[5]}, kE, literal ? 1u : 0u, off, h.c[0], h.c[1], 0});
            } else {
                d.bits = (uint32_t)rec.hints.size();
                rec.hints.push_back(SolveHintDev{h.n, (uint32_t)h.q.size(), (uint32_t)h.rem.size(), (uint32_t)h.D.size(), kE, literal ? 1u : 0u, off, 0});
            }
            for (const std::vector<uint32_t> *cols : {&h.q, &h.rem, &h.D, &h.E}) rec.hint_idx.insert(rec.hint_idx.end(), cols->begin(), cols->end());
            if (literal) literal_words(h, s.kind == pmsolve::KIND_LONGDIV_WIDE ? WIDE_WE : LONGDIV_WE, rec.hint_idx);
        }
        if (s.kind != pmsolve::KIND_ISZERO) continue;
        d.bits = (uint32_t)rec.pairs.size();
        SolvePairDev<P> pr;
        memset((void *)&pr, 0, sizeof pr);
        const pmsolve::PairRows &rows = plan.pairs[s.cols_off];
        pr.pos_m = rows.pos_m; pr.pos_c = rows.pos_c; pr.row1 = rows.row1; pr.col_m = rows.col_m; pr.m_in_b = rows.m_in_b; pr.b_in_b = rows.b_in_b;
        pr.negated = rows.negated;
        rec.pairs.push_back(pr);
    }
    return rec;
}

// any of the four markers (divrem.cuh: marker_byte)
template <class P>
PM_HD bool is_marker(const Fp<P> &v) {
    return marker_byte<P>(v) != 0;
}

PM_HD const pmsolve::Csr &matrix_of(uint32_t kind, const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm) {
    return kind == pmsolve::KIND_A ? A : kind == pmsolve::KIND_B ? B : Cm;
}

// KIND_BITS_x -> KIND_x
PM_HD uint32_t matrix_kind(uint32_t kind) { return kind >= pmsolve::KIND_BITS_C ? kind - pmsolve::KIND_BITS_C : kind; }

// Inverse t of a plan's count + 2 n_pairs: 1 / coefficient of step t's unknown (a division row: 1 / cq), and for t >= count 1 / cm
// and 1 / cb of an is-zero pair's opener; an indicator step needs none and its record is left alone.  A square-root step: 1 / (ka kb),
// the product of the root's two coefficients, both found from the step record alone.
template <class P>
PM_HD void solve_inverse(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, SolveStepDev<P> *steps, uint64_t count, SolvePairDev<P> *pairs,
                         const SolveDivDev *divs, uint64_t t) {
    if (t < count && (steps[t].kind == pmsolve::KIND_INDICATOR || steps[t].kind == pmsolve::KIND_BLOCK || steps[t].kind == pmsolve::KIND_LONGDIV || steps[t].kind == pmsolve::KIND_MODDIV || steps[t].kind == pmsolve::KIND_LONGDIV_WIDE || steps[t].kind == pmsolve::KIND_MODMULDIV)) return;   // no inverse of a coefficient: the record stays as the host wrote it
    if (t < count && steps[t].kind == pmsolve::KIND_SQRT) {
        const Fp<P> ka = *(const Fp<P> *)(A.val + 4 * steps[t].pos), kb = *(const Fp<P> *)(B.val + 4 * (B.rowptr[steps[t].row] + steps[t].bits));
        const Fp<P> coef = mul<P>(ka, kb);
        steps[t].inv = coef.eq(Fp<P>::one()) ? coef : inverse<P>(coef);
        return;
    }
    const Fp<P> *at;
    Fp<P> *out;
    if (t < count) {                 // an is-zero step's own entry is the flag's, in the closer's A or B; a division step's the quotient's
        const uint32_t kind = steps[t].kind;
        const pmsolve::Csr &M = kind == pmsolve::KIND_ISZERO ? (pairs[steps[t].bits].b_in_b ? B : A)
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
PM_HD Fp<P> row_dot_skip(const pmsolve::Csr &M, const Fp<P> *z, uint64_t r, uint64_t skip) {
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
PM_HD Fp<P> row_dot_unmarked(const pmsolve::Csr &M, const Fp<P> *z, uint64_t r) {
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
template <class P, bool DIV, class Sink>
PM_HD void solve_step(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveStepDev<P> &s, Fp<P> *z, const Sink &stuck) {
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
            stuck(s);
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
template <class P, bool DIV, class Sink>
PM_HD void solve_bits(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveStepDev<P> &s, const uint32_t *__restrict__ bit_cols, Fp<P> *z,
                      const Sink &stuck) {
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
        stuck(s);
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
PM_HD void solve_iszero(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveStepDev<P> &s, const SolvePairDev<P> &pr, Fp<P> *z) {
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
template <class P, class Sink>
PM_HD void solve_divrem(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveStepDev<P> &s, const SolveDivDev &dv, Fp<P> *z,
                        const Sink &stuck) {
    const uint64_t r = s.row;
    const Fp<P> d = row_dot_skip<P>(dv.q_in_b ? A : B, z, r, SOLVE_NONE);
    const Fp<P> a = mul<P>(row_dot_skip<P>(Cm, z, r, dv.pos_r), s.inv);
    Fp<P> q = Fp<P>::zero(), rem = Fp<P>::zero();
    if (!euclid_divrem<P>(a, d, &q, &rem)) stuck(s);
    z[s.col] = q;
    z[dv.col_r] = rem;
}

// one indicator row on one assignment: z_u = [K z == 0] as field one or field zero, whatever u's coefficient is.  K's whole row (the
// indicator's side has no other non-zero entry and C_r none at all); the column still holds its marker.  No division, never stuck.
template <class P>
PM_HD void solve_indicator(const pmsolve::Csr &A, const pmsolve::Csr &B, const SolveStepDev<P> &s, Fp<P> *z) {
    z[s.col] = indicator_of<P>(row_dot_skip<P>(s.bits ? A : B, z, s.row, SOLVE_NONE));
}

// one square-root row on one assignment: ka kb z_u^2 = (C z)_r, so with c = (C z)_r / (ka kb)
//   c a square, 0 included:  z_u = the root whose canonical integer is <= (r - 1) / 2 (sqrt.cuh: fr_sqrt, a fixed trip count)
//   c a non-residue:         stuck at the row, zero stored
// C's whole row: it does not name u, and u's sides have no other non-zero entry.  The column still holds its marker.
template <class P, class Sink>
PM_HD void solve_sqrt(const pmsolve::Csr &Cm, const SolveStepDev<P> &s, Fp<P> *z, const Sink &stuck) {
    const Fp<P> c = mul<P>(row_dot_skip<P>(Cm, z, s.row, SOLVE_NONE), s.inv);
    Fp<P> root = Fp<P>::zero();
    if (!fr_sqrt<P>(c, &root)) stuck(s);
    z[s.col] = root;
}

constexpr uint32_t SOLVE_NO_COLUMN = ~(uint32_t)0;   // solve_block_invert: every column has a pivot

// out = M^-1 for the k x k matrix M (row-major; M is destroyed): Gauss-Jordan with a row-pivot search (the first row at or below the
// diagonal with a non-zero entry), one inverse<P> per pivot.  The trip counts depend on k only: the search looks at every row, the
// swap is always made (with itself where the diagonal entry serves) and every row is eliminated over its full width.
// -> the first column without a pivot (M is singular; out is not the inverse then), or SOLVE_NO_COLUMN.
template <class P>
PM_HD uint32_t solve_block_invert(Fp<P> *M, uint32_t k, Fp<P> *out) {
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t j = 0; j < k; ++j) out[(size_t)i * k + j] = i == j ? Fp<P>::one() : Fp<P>::zero();
    uint32_t missing = SOLVE_NO_COLUMN;
    for (uint32_t c = 0; c < k; ++c) {
        uint32_t p = k;
        for (uint32_t i = c; i < k; ++i) p = (p == k && !M[(size_t)i * k + c].is_zero()) ? i : p;
        if (p == k) {
            missing = missing == SOLVE_NO_COLUMN ? c : missing;
            p = c;
        }
        for (uint32_t j = 0; j < k; ++j) {
            const Fp<P> m = M[(size_t)p * k + j], o = out[(size_t)p * k + j];
            M[(size_t)p * k + j] = M[(size_t)c * k + j];
            out[(size_t)p * k + j] = out[(size_t)c * k + j];
            M[(size_t)c * k + j] = m;
            out[(size_t)c * k + j] = o;
        }
        const Fp<P> scale = inverse<P>(M[(size_t)c * k + c]);      // inverse(0) = 0: a column without a pivot zeroes its row
        for (uint32_t j = 0; j < k; ++j) {
            M[(size_t)c * k + j] = mul<P>(M[(size_t)c * k + j], scale);
            out[(size_t)c * k + j] = mul<P>(out[(size_t)c * k + j], scale);
        }
        for (uint32_t i = 0; i < k; ++i) {
            const Fp<P> f = i == c ? Fp<P>::zero() : M[(size_t)i * k + c];
            for (uint32_t j = 0; j < k; ++j) {
                M[(size_t)i * k + j] = sub<P>(M[(size_t)i * k + j], mul<P>(f, M[(size_t)c * k + j]));
                out[(size_t)i * k + j] = sub<P>(out[(size_t)i * k + j], mul<P>(f, out[(size_t)c * k + j]));
            }
        }
    }
    return missing;
}

// The inverse pool of a plan's records: every distinct block matrix inverted once and stored transposed at rec.mat_off[mat].
// -> the block of smallest first row whose matrix is singular, with `column` = the index (in the block's columns) of the first column
// without a pivot; or plan.blocks.size().
template <class P>
inline size_t solve_block_inverses(const pmsolve::Plan &plan, SolveRecords<P> &rec, uint32_t *column) {
    const size_t n_mats = plan.block_mats.size();
    std::vector<uint32_t> missing(n_mats, SOLVE_NO_COLUMN);
    rec.block_inv.assign(rec.mat_off.back(), Fp<P>::zero());
    std::vector<Fp<P>> M, inv;
    for (size_t t = 0; t < n_mats; ++t) {
        const uint32_t k = plan.block_mats[t].k;
        M.resize((size_t)k * k);
        inv.resize((size_t)k * k);
        memcpy((void *)M.data(), plan.block_mats[t].words.data(), (size_t)k * k * sizeof(Fp<P>));
        missing[t] = solve_block_invert<P>(M.data(), k, inv.data());
        for (uint32_t i = 0; i < k; ++i)
            for (uint32_t j = 0; j < k; ++j) rec.block_inv[rec.mat_off[t] + (size_t)i * k + j] = inv[(size_t)j * k + i];
    }
    size_t bad = plan.blocks.size();
    for (size_t b = 0; b < plan.blocks.size(); ++b)
        if (missing[plan.blocks[b].mat] != SOLVE_NO_COLUMN && (bad == plan.blocks.size() || plan.blocks[b].rows[0] < plan.blocks[bad].rows[0])) bad = b;
    if (bad != plan.blocks.size()) *column = missing[plan.blocks[bad].mat];
    return bad;
}

// One row of a linear block on one assignment: rhs = (A z)_r (B z)_r - the known entries of (C z)_r.  The block's columns still
// hold their markers (they are unknown until the block's stores, which come after every rhs), and no other column a row names does.
template <class P>
PM_HD Fp<P> solve_block_rhs(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, uint64_t r, const Fp<P> *z) {
    const Fp<P> az = row_dot_skip<P>(A, z, r, SOLVE_NONE), bz = row_dot_skip<P>(B, z, r, SOLVE_NONE);
    return sub<P>(mul<P>(az, bz), row_dot_unmarked<P>(Cm, z, r));
}

// Column j of a linear block from the k right-hand sides: sum_i Inv[j][i] rhs_i, the inverse read transposed
template <class P>
PM_HD Fp<P> solve_block_out(const Fp<P> *__restrict__ inv_t, uint32_t k, uint32_t j, const Fp<P> *rhs) {
    Fp<P> acc = Fp<P>::zero();
    for (uint32_t i = 0; i < k; ++i) acc = add<P>(acc, mul<P>(inv_t[(size_t)i * k + j], rhs[i]));
    return acc;
}

// one linear block on one assignment, serially (the kernel gives a lane to each row, then to each column): every right-hand side
// before any store.  No division, never stuck.
template <class P>
PM_HD void solve_block(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveBlockDev &blk, const uint32_t *__restrict__ block_idx,
                       const Fp<P> *__restrict__ block_inv, Fp<P> *z) {
    Fp<P> rhs[pmsolve::MAX_BLOCK];
    for (uint32_t i = 0; i < blk.k; ++i) rhs[i] = solve_block_rhs<P>(A, B, Cm, block_idx[blk.rows_off + i], z);
    for (uint32_t j = 0; j < blk.k; ++j) z[block_idx[blk.cols_off + j]] = solve_block_out<P>(block_inv + blk.inv_off, blk.k, j, rhs);
}

// one declared long division on one assignment: every input limb from Montgomery form to its canonical integer, accumulated at bit
// offset n j (limbs need not be normalised: they overlap and carry), D = the dividend's sum, E = the divisor's (or the literal that
// solve_records accumulated); D is formed 1024 - rounds bits higher, where longdiv wants it (`rounds`: the launch's trip count, at
// least n (kD - 1) + 256 or 1024, so what add_shifted loses above the register is exactly D >= 2^1024); then longdiv, and the kq n-bit limbs of floor(D / E) and the kr n-bit limbs of D mod E go back to
// Montgomery form and into their columns.  Stuck at the hint's word (nr + h: the step's row), with zero in every output:
//   E = 0;  D >= 2^1024;  E >= 2^512;  q >= 2^(n kq);  rem >= 2^(n kr)
// The conditions are or-ed into one word and the outputs stored under its mask: no branch on an operand but the sink's.
template <class P, class Sink>
PM_HD void solve_longdiv(const SolveStepDev<P> &s, const SolveHintDev &h, const uint32_t *__restrict__ hint_idx, uint32_t rounds, Fp<P> *z, const Sink &stuck) {
    static_assert(P::N == 8, "four 64-bit words");
    const uint32_t *q_cols = hint_idx + h.off, *r_cols = q_cols + h.kq, *d_cols = r_cols + h.kr, *e_words = d_cols + h.kD;
    uint32_t D[LONGDIV_WD], E[LONGDIV_WE], R[LONGDIV_WE + 1], bad = 0;
#pragma unroll
    for (int w = 0; w < LONGDIV_WD; ++w) D[w] = 0;
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) E[w] = 0;
    const uint32_t base = 32u * LONGDIV_WD - rounds;
    for (uint32_t j = 0; j < h.kD; ++j) bad |= add_shifted<LONGDIV_WD>(D, from_mont<P>(z[d_cols[j]]).l, base + h.n * j);
    if (h.literal) {
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) E[w] = e_words[w];
        bad |= e_words[LONGDIV_WE];
    } else {
        for (uint32_t j = 0; j < h.kE; ++j) bad |= add_shifted<LONGDIV_WE>(E, from_mont<P>(z[e_words[j]]).l, h.n * j);
    }
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) any |= E[w];
    bad |= (uint32_t)(any == 0);
    longdiv<LONGDIV_WD, LONGDIV_WE>(D, E, R, rounds);
    bad |= bits_from<LONGDIV_WD>(D, h.n * h.kq) | bits_from<LONGDIV_WE + 1>(R, h.n * h.kr);
    if (bad) stuck(s);
    const uint32_t mask = bad ? 0u : ~0u;
    for (uint32_t i = 0; i < h.kq; ++i) {
        Fp<P> limb = limb_at<P, LONGDIV_WD>(D, h.n * i, h.n);
#pragma unroll
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[q_cols[i]] = to_mont<P>(limb);
    }
    for (uint32_t i = 0; i < h.kr; ++i) {
        Fp<P> limb = limb_at<P, LONGDIV_WE + 1>(R, h.n * i, h.n);
#pragma unroll
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[r_cols[i]] = to_mont<P>(limb);
    }
}

// a -= b & mask on W words -> the borrow (0 or 1)
template <int W>
PM_HD uint32_t sub_masked(uint32_t (&a)[W], const uint32_t (&b)[W], uint32_t mask) {
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const uint32_t bj = b[j] & mask, x = a[j] - borrow, b1 = a[j] < borrow;
        a[j] = x - bj;
        borrow = b1 | (uint32_t)(x < bj);
    }
    return borrow;
}

// a += b & mask on W words -> the carry (0 or 1)
template <int W>
PM_HD uint32_t add_masked(uint32_t (&a)[W], const uint32_t (&b)[W], uint32_t mask) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const uint64_t sum = (uint64_t)a[j] + (b[j] & mask) + carry;
        a[j] = (uint32_t)sum;
        carry = (uint32_t)(sum >> 32);
    }
    return carry;
}

// Binary extended Euclid for an ODD modulus p, every update masked, `rounds` rounds whatever the operands: on entry u in [0, p),
// v = p, x1 = c in [0, p), x2 = 0; where gcd(u, p) = 1 it leaves v = 1 and x2 = c / u mod p (c = 1: the inverse; the caller passes the
// numerator of a modular division and saves the product and the reduction that would follow).  One round:
//     u odd and u < v:  swap (u, v) and (x1, x2)          -- v is odd on entry and stays odd: it only ever takes an odd u's value
//     u odd:            u -= v,  x1 = x1 - x2 mod p       -- u is even now
//     always:           u /= 2,  x1 = x1 / 2 mod p        -- p is odd: x1 or x1 + p is even
// Invariants: x1 d = u c and x2 d = v c (mod p) for the d the caller put into u, and gcd(u, v) = gcd(d, p).
// THE BOUND.  Let p < 2^L and s = bitlength(u) + bitlength(v) <= 2 L.  The swap leaves s alone.  A round with u > 0 lowers s by at
// least one: an even u loses a bit by the halving; an odd u >= v becomes (u - v) / 2 < u / 2, at least one bit shorter.  v >= 1
// always, so u > 0 means s >= 2, and u > 0 can hold for at most 2 L - 1 rounds.  With u = 0 a round changes neither v nor x2 (u is
// even, never swapped; only x1 is halved, which nothing reads).  So after 2 L rounds u = 0 and v = gcd(d, p): the caller tests v = 1.
// Worst cases: u = 2^(L - 1) (L - 1 halvings before the first subtraction), u = p - 1 and u = (p +- 1) / 2 (subtractions that shorten
// by one bit only).  An even p (the caller has marked it stuck) breaks the invariants, not the trip count.  Word loops unrolled, the
// round loop rolled; no branch and no register index depends on an operand.
template <int W>
PM_HD void modinv_odd(uint32_t (&u)[W], uint32_t (&v)[W], uint32_t (&x1)[W], uint32_t (&x2)[W], const uint32_t (&p)[W], uint32_t rounds) {
#pragma unroll 1
    for (uint32_t round = 0; round < rounds; ++round) {
        const uint32_t odd = 0u - (u[0] & 1u);
        uint32_t borrow = 0;         // of u - v: u < v
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t x = u[j] - borrow, b1 = u[j] < borrow;
            borrow = b1 | (uint32_t)(x < v[j]);
        }
        const uint32_t swap = odd & (0u - borrow);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint32_t tu = (u[j] ^ v[j]) & swap, tx = (x1[j] ^ x2[j]) & swap;
            u[j] ^= tu; v[j] ^= tu;
            x1[j] ^= tx; x2[j] ^= tx;
        }
        sub_masked<W>(u, v, odd);
        add_masked<W>(x1, p, 0u - sub_masked<W>(x1, x2, odd));
        const uint32_t top = add_masked<W>(x1, p, 0u - (x1[0] & 1u));
#pragma unroll
        for (int j = 0; j < W - 1; ++j) {
            u[j] = u[j] >> 1 | u[j + 1] << 31;
            x1[j] = x1[j] >> 1 | x1[j + 1] << 31;
        }
        u[W - 1] >>= 1;
        x1[W - 1] = x1[W - 1] >> 1 | top << 31;
    }
}

// one declared modular division on one assignment: Z = (N+ - N-) / (D+ - D-) mod P.  The modulus is accumulated like a divisor (or is
// the literal that solve_records accumulated).  Then the four operand lists in turn, in ONE rolled loop so that the kernel holds one
// copy of longdiv: a list's limbs leave Montgomery form and are accumulated at bit offset n j, 1024 - rounds bits higher (`rounds`:
// the launch's reduction bound, at least n (k - 1) + 256 or 1024 for every list, so what add_shifted loses is exactly a sum >= 2^1024),
// longdiv leaves the sum mod P, and a masked select puts it into N or D (lists 0 and 2) or subtracts it modulo P (lists 1 and 3);
// an empty list is passed over, which is a branch on the record, not on an operand.  kNp = kNm = 0: N = 1.  modinv_odd with u = D,
// x1 = N and `inv_rounds` = 2 L rounds (P < 2^L, or P >= 2^512 and the lane is stuck already) leaves Z = N / D mod P in x2 where v = 1
// -- the product N D^-1 and its reduction are not formed: the Euclid carries the numerator instead of 1 --, and the kz n-bit limbs of
// Z go back to Montgomery form and into their columns.  Stuck at the hint's word (nr + h: the step's row), with zero in every output:
//   P even or P < 3;  P >= 2^512;  N+, N-, D+ or D- >= 2^1024;  gcd(D mod P, P) != 1 (D = 0 mod P included);  Z >= 2^(n kz)
// or-ed into one word, the outputs stored under its mask.  The dividend, remainder and trial difference of the reductions are dead
// when the Euclid's v, x1 and x2 come to life.
template <class P, class Sink>
PM_HD void solve_moddiv(const SolveStepDev<P> &s, const SolveModDev &h, const uint32_t *__restrict__ hint_idx, uint32_t rounds, uint32_t inv_rounds, Fp<P> *z,
                        const Sink &stuck) {
    static_assert(P::N == 8, "four 64-bit words");
    const uint32_t *z_cols = hint_idx + h.off, *cols = z_cols + h.kz, *p_words = cols + h.k[0] + h.k[1] + h.k[2] + h.k[3];
    uint32_t M[LONGDIV_WE], Nr[LONGDIV_WE], Dr[LONGDIV_WE], bad = 0;
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) M[w] = Nr[w] = Dr[w] = 0;
    if (h.literal) {
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) M[w] = p_words[w];
        bad |= p_words[LONGDIV_WE];
    } else {
        for (uint32_t j = 0; j < h.kP; ++j) bad |= add_shifted<LONGDIV_WE>(M, from_mont<P>(z[p_words[j]]).l, h.n * j);
    }
    uint32_t high = 0;
#pragma unroll
    for (int w = 1; w < LONGDIV_WE; ++w) high |= M[w];
    bad |= (uint32_t)((M[0] & 1u) == 0) | (uint32_t)(high == 0 && M[0] == 1u);   // even (0 and 2 included), or 1
    const uint32_t base = 32u * LONGDIV_WD - rounds;
#pragma unroll 1
    for (uint32_t which = 0; which < 4; ++which) {
        const uint32_t k = h.k[which];
        if (k == 0) continue;
        uint32_t S[LONGDIV_WD], R[LONGDIV_WE + 1], T[LONGDIV_WE];
#pragma unroll
        for (int w = 0; w < LONGDIV_WD; ++w) S[w] = 0;
        for (uint32_t j = 0; j < k; ++j) bad |= add_shifted<LONGDIV_WD>(S, from_mont<P>(z[cols[j]]).l, base + h.n * j);
        cols += k;
        longdiv<LONGDIV_WD, LONGDIV_WE>(S, M, R, rounds);
        const uint32_t numerator = which < 2 ? ~0u : 0u, subtract = 0u - (which & 1u);
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) T[w] = ((Nr[w] & numerator) | (Dr[w] & ~numerator)) & subtract;   // 0, or what the list is subtracted from
        // lists 0 and 2: T = R;  lists 1 and 3: T = T - R mod P.  R < P (R[16] = 0) wherever P != 0
        uint32_t Rw[LONGDIV_WE];
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) Rw[w] = R[w];
        add_masked<LONGDIV_WE>(T, Rw, ~subtract);
        add_masked<LONGDIV_WE>(T, M, 0u - sub_masked<LONGDIV_WE>(T, Rw, subtract));
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) {
            Nr[w] = (T[w] & numerator) | (Nr[w] & ~numerator);
            Dr[w] = (T[w] & ~numerator) | (Dr[w] & numerator);
        }
    }
    if ((h.k[0] | h.k[1]) == 0) Nr[0] = 1;       // a plain inverse (P = 1 is stuck)
    uint32_t V[LONGDIV_WE], Z[LONGDIV_WE];
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) {
        V[w] = M[w];
        Z[w] = 0;
    }
    modinv_odd<LONGDIV_WE>(Dr, V, Nr, Z, M, inv_rounds);
    uint32_t rest = V[0] ^ 1u;       // gcd(D mod P, P) - 1
#pragma unroll
    for (int w = 1; w < LONGDIV_WE; ++w) rest |= V[w];
    bad |= rest | bits_from<LONGDIV_WE>(Z, h.n * h.kz);
    if (bad) stuck(s);
    const uint32_t mask = bad ? 0u : ~0u;
    for (uint32_t i = 0; i < h.kz; ++i) {
        Fp<P> limb = limb_at<P, LONGDIV_WE>(Z, h.n * i, h.n);
#pragma unroll
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[z_cols[i]] = to_mont<P>(limb);
    }
}

// acc <<= bits on W words, bits < 32 W: whole words by a rolled loop of `bits / 32` trips (the same in every lane of a launch), the rest
// by one funnel shift; no register is indexed by `bits`
template <int W>
PM_HD void shift_up(uint32_t (&acc)[W], uint32_t bits) {
#pragma unroll 1
    for (uint32_t i = 0; i < (bits >> 5); ++i) {
#pragma unroll
        for (int w = W - 1; w > 0; --w) acc[w] = acc[w - 1];
        acc[0] = 0;
    }
    const uint32_t down = 32u - (bits & 31u);    // in 1..32: a 64-bit shift
#pragma unroll
    for (int w = W - 1; w >= 0; --w) acc[w] = (uint32_t)(((uint64_t)acc[w] << 32 | (w > 0 ? acc[w > 0 ? w - 1 : 0] : 0u)) >> down);
}

// one declared modular multiply-divide on one assignment: Z with cD (D+ - D-) Z = cN (A B + N+ - N-) (mod P).  The modulus is
// accumulated as solve_moddiv does.  Then NINE PHASES in one rolled loop, so that the kernel holds one copy of longdiv and one of the
// schoolbook product; each forms a 1024-bit value in the register S where longdiv wants it (shifted left by 1024 - its trip count),
// reduces it modulo P and folds the remainder into one of two residues, X (the numerator) and Y (the second factor, then the
// denominator):
//   0, 1   the lists A and B: accumulated like a dividend (`rounds`: the launch's bound, so what add_shifted loses is exactly a sum
//          >= 2^1024);  X = A mod P,  Y = B mod P
//   2      S = X Y, a 16 x 16-word schoolbook product, below P^2 < 2^(2 L): `inv_rounds` = 2 L rounds;  X = A B mod P
//   3, 4   the lists N+ and N-:  X = X + N+ mod P,  X = X - N- mod P
//   5, 6   the lists D+ and D-:  Y = D+ mod P,  Y = Y - D- mod P     (no denominator lists: Y = 1 before phase 8)
//   7, 8   S = cN X and S = cD Y, the same product with the literal as its second factor, below 2^32 P < 2^(L + 32): L + 32 rounds
// An empty list is passed over, which is a branch on the record, not on an operand; which phase it is, is the loop counter.  The
// literals scale AFTER the reductions, so nothing is stuck that the five conditions below do not name.  modinv_odd with u = Y, x1 = X
// and `inv_rounds` rounds leaves Z in x2 where v = 1, as in solve_moddiv.  Stuck at the hint's word (nr + h: the step's row), with zero
// in every output:
//   P even or P < 3;  P >= 2^512;  a list sum >= 2^1024;  gcd(cD D mod P, P) != 1 (D = 0 mod P included);  Z >= 2^(n kz)
// or-ed into one word, the outputs stored under its mask.  Word loops unrolled, round loops rolled; no branch and no register index
// depends on an operand.
template <class P, class Sink>
PM_HD void solve_modmuldiv(const SolveStepDev<P> &s, const SolveMulDev &h, const uint32_t *__restrict__ hint_idx, uint32_t rounds, uint32_t inv_rounds, Fp<P> *z,
                           const Sink &stuck) {
    static_assert(P::N == 8, "four 64-bit words");
    const uint32_t *z_cols = hint_idx + h.off, *cols = z_cols + h.kz, *p_words = cols + h.k[0] + h.k[1] + h.k[2] + h.k[3] + h.k[4] + h.k[5];
    uint32_t M[LONGDIV_WE], X[LONGDIV_WE], Y[LONGDIV_WE], bad = 0;
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) M[w] = X[w] = Y[w] = 0;
    if (h.literal) {
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) M[w] = p_words[w];
        bad |= p_words[LONGDIV_WE];
    } else {
        for (uint32_t j = 0; j < h.kP; ++j) bad |= add_shifted<LONGDIV_WE>(M, from_mont<P>(z[p_words[j]]).l, h.n * j);
    }
    uint32_t high = 0;
#pragma unroll
    for (int w = 1; w < LONGDIV_WE; ++w) high |= M[w];
    bad |= (uint32_t)((M[0] & 1u) == 0) | (uint32_t)(high == 0 && M[0] == 1u);   // even (0 and 2 included), or 1
    const uint32_t scale_rounds = (inv_rounds >> 1) + 32u;
#pragma unroll 1
    for (uint32_t phase = 0; phase < 9; ++phase) {
        const bool product = phase == 2 || phase >= 7;
        const uint32_t list = phase < 2 ? phase : phase - 1;      // of a list phase
        if (!product && h.k[list < 6 ? list : 0] == 0) continue;
        const uint32_t into_y = phase == 1 || phase == 5 || phase == 6 || phase == 8 ? ~0u : 0u;      // the residue the phase folds into
        uint32_t S[LONGDIV_WD], R[LONGDIV_WE + 1], T[LONGDIV_WE], trips = rounds;
#pragma unroll
        for (int w = 0; w < LONGDIV_WD; ++w) S[w] = 0;
        if (product) {
            if (phase == 8 && (h.k[4] | h.k[5]) == 0) {      // no denominator lists: D = 1 (P = 1 is stuck)
#pragma unroll
                for (int w = 0; w < LONGDIV_WE; ++w) Y[w] = w == 0 ? 1u : 0u;
            }
            // the factors: X Y, X cN or Y cD
            const uint32_t literal = phase == 2 ? 0u : ~0u, c = phase == 7 ? h.cN : h.cD;
            uint32_t F[LONGDIV_WE], G[LONGDIV_WE];
#pragma unroll
            for (int w = 0; w < LONGDIV_WE; ++w) {
                F[w] = (Y[w] & into_y) | (X[w] & ~into_y);
                G[w] = (Y[w] & ~literal) | ((w == 0 ? c : 0u) & literal);
            }
#pragma unroll
            for (int i = 0; i < LONGDIV_WE; ++i) {
                uint32_t carry = 0;
#pragma unroll
                for (int j = 0; j < LONGDIV_WE; ++j) {
                    const uint64_t t = (uint64_t)F[j] * G[i] + S[i + j] + carry;
                    S[i + j] = (uint32_t)t;
                    carry = (uint32_t)(t >> 32);
                }
                S[i + LONGDIV_WE] = carry;
            }
            trips = phase == 2 ? inv_rounds : scale_rounds;
            shift_up<LONGDIV_WD>(S, 32u * LONGDIV_WD - trips);
        } else {
            const uint32_t k = h.k[list < 6 ? list : 0], base = 32u * LONGDIV_WD - rounds;
            for (uint32_t j = 0; j < k; ++j) bad |= add_shifted<LONGDIV_WD>(S, from_mont<P>(z[cols[j]]).l, base + h.n * j);
            cols += k;
        }
        longdiv<LONGDIV_WD, LONGDIV_WE>(S, M, R, trips);
        // T = what the remainder R is folded into: zero (the phase sets its residue), or the residue (phases 3, 4 and 6 add to it or
        // subtract from it).  R < P (R[16] = 0) wherever P != 0
        const uint32_t keep = phase == 3 || phase == 4 || phase == 6 ? ~0u : 0u, subtract = phase == 4 || phase == 6 ? ~0u : 0u;
        uint32_t Rw[LONGDIV_WE], U[LONGDIV_WE];
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) {
            T[w] = ((Y[w] & into_y) | (X[w] & ~into_y)) & keep;
            Rw[w] = R[w];
        }
        // T + R mod P: the sum, then P taken off where the sum carried or is not below P;  T - R mod P: the difference, then P put back
        const uint32_t carry = add_masked<LONGDIV_WE>(T, Rw, ~subtract);
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) U[w] = T[w];
        const uint32_t below = sub_masked<LONGDIV_WE>(U, M, ~0u);      // 1: T < P
        const uint32_t reduce = ~subtract & (0u - (carry | (below ^ 1u)));
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) T[w] = (U[w] & reduce) | (T[w] & ~reduce);
        add_masked<LONGDIV_WE>(T, M, 0u - sub_masked<LONGDIV_WE>(T, Rw, subtract));
#pragma unroll
        for (int w = 0; w < LONGDIV_WE; ++w) {
            X[w] = (T[w] & ~into_y) | (X[w] & into_y);
            Y[w] = (T[w] & into_y) | (Y[w] & ~into_y);
        }
    }
    uint32_t V[LONGDIV_WE], Z[LONGDIV_WE];
#pragma unroll
    for (int w = 0; w < LONGDIV_WE; ++w) {
        V[w] = M[w];
        Z[w] = 0;
    }
    modinv_odd<LONGDIV_WE>(Y, V, X, Z, M, inv_rounds);
    uint32_t rest = V[0] ^ 1u;       // gcd(cD D mod P, P) - 1
#pragma unroll
    for (int w = 1; w < LONGDIV_WE; ++w) rest |= V[w];
    bad |= rest | bits_from<LONGDIV_WE>(Z, h.n * h.kz);
    if (bad) stuck(s);
    const uint32_t mask = bad ? 0u : ~0u;
    for (uint32_t i = 0; i < h.kz; ++i) {
        Fp<P> limb = limb_at<P, LONGDIV_WE>(Z, h.n * i, h.n);
#pragma unroll
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[z_cols[i]] = to_mont<P>(limb);
    }
}

// ---- the WIDE long division (KIND_LONGDIV_WIDE): schoolbook division in base 2^32 over word arrays in memory

// what the digit recurrence did, for the tests that must know that a family of operands reaches its rare branches
struct WideCounters {
    uint32_t addbacks = 0, saturated = 0;
};

// the significant words of the W-word a: W less its leading zero words
PM_HD uint32_t significant_words(const uint32_t *a, uint32_t W) {
    while (W && a[W - 1] == 0) --W;
    return W;
}

// One quotient digit's ESTIMATE (Knuth 4.3.1 D3): from the window's three leading words u2 u1 u0 and the normalised divisor's two
// leading words v1 v0 (v1 >= 2^31; v0 = u0 = 0 where the divisor has one word).  floor((u2 B + u1) / v1), SATURATED at B - 1 where
// u2 = v1 (u2 > v1 cannot be: the window's remainder is below the divisor), then lowered while qhat v0 > rhat B + u0 and rhat < B:
// at most twice, so the refinement is two tests and no loop.  The result is the digit or one more.
PM_HD uint32_t wide_estimate(uint32_t u2, uint32_t u1, uint32_t u0, uint32_t v1, uint32_t v0, uint32_t *saturated) {
    const uint64_t num = (uint64_t)u2 << 32 | u1;
    const bool sat = u2 >= v1;
    uint64_t qhat = sat ? 0xffffffffull : num / v1;
    uint64_t rhat = num - qhat * v1;
    *saturated = sat ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (rhat <= 0xffffffffull && qhat * v0 > (rhat << 32 | u0)) {
            --qhat;
            rhat += v1;
        }
    return (uint32_t)qhat;
}

// q = floor(D / E) and rem = D mod E for the nD-word D and the nE-word E (little-endian 32-bit words), Knuth's algorithm D:
//   m = the significant words of E (m = 0: E = 0, -> 1 with q and rem zero), t = those of D; s = the leading zeros of E[m - 1]
//   v = E << s (m words), u = D << s (t + 1 words)
//   for j = t - m down to 0 (none where t < m):
//       qhat = wide_estimate(u[j + m], u[j + m - 1], u[j + m - 2], v[m - 1], v[m - 2])
//       u[j .. j + m] -= qhat v;  where that borrows: u[j .. j + m] += v and qhat -= 1      -- the ADD-BACK, about 2 / B of random digits
//       q[j] = qhat
//   rem = u >> s
// A divisor of ONE significant word takes the same path: v[m - 2] and u[j + m - 2] read as zero, the refinement never fires and the
// estimate is exact.  This is the statement of the recurrence that k_solve_longdiv_wide distributes over a wave's lanes: there lane i
// holds word i of qhat v and of the window, and the carries and borrows are resolved by ballot.  q has nD words, rem nE; u (nD + 1
// words) and v (nE words) are working memory.  `counters` (may be null) counts executed add-backs and saturated estimates.
PM_HD uint32_t longdiv_wide_words(const uint32_t *D, uint32_t nD, const uint32_t *E, uint32_t nE, uint32_t *q, uint32_t *rem, uint32_t *u, uint32_t *v,
                                  WideCounters *counters) {
    for (uint32_t i = 0; i < nD; ++i) q[i] = 0;
    for (uint32_t i = 0; i < nE; ++i) rem[i] = 0;
    const uint32_t m = significant_words(E, nE), t = significant_words(D, nD);
    if (m == 0) return 1;
    uint32_t s = 0;
    while (!(E[m - 1] << s & 0x80000000u)) ++s;
    for (uint32_t i = 0; i < m; ++i) v[i] = s ? E[i] << s | (i ? E[i - 1] >> (32 - s) : 0u) : E[i];
    for (uint32_t i = 0; i <= nD; ++i) {
        const uint32_t lo = i && i - 1 < t ? D[i - 1] : 0u, here = i < t ? D[i] : 0u;
        u[i] = s ? here << s | lo >> (32 - s) : here;
    }
    const uint32_t v1 = v[m - 1], v0 = m >= 2 ? v[m - 2] : 0u;
    for (uint32_t j = t >= m ? t - m + 1 : 0; j-- > 0;) {
        uint32_t saturated;
        uint32_t qhat = wide_estimate(u[j + m], u[j + m - 1], m >= 2 ? u[j + m - 2] : 0u, v1, v0, &saturated);
        uint64_t carry = 0, borrow = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const uint64_t prod = (uint64_t)qhat * v[i] + carry;
            carry = prod >> 32;
            const uint64_t diff = (uint64_t)u[j + i] - (uint32_t)prod - borrow;
            u[j + i] = (uint32_t)diff;
            borrow = diff >> 63;
        }
        const uint64_t diff = (uint64_t)u[j + m] - carry - borrow;
        u[j + m] = (uint32_t)diff;
        if (diff >> 63) {
            uint64_t c = 0;
            for (uint32_t i = 0; i < m; ++i) {
                const uint64_t sum = (uint64_t)u[j + i] + v[i] + c;
                u[j + i] = (uint32_t)sum;
                c = sum >> 32;
            }
            u[j + m] += (uint32_t)c;
            --qhat;
            if (counters) ++counters->addbacks;
        }
        if (counters) counters->saturated += saturated;
        q[j] = qhat;
    }
    for (uint32_t i = 0; i < m; ++i) rem[i] = s ? u[i] >> s | u[i + 1] << (32 - s) : u[i];
    return 0;
}

// limb_at for W words in memory (the kernel: in LDS): the n-bit limb (n <= 128) at bit offset off, as a canonical element; words at
// and above W read as zero
template <class P>
PM_HD Fp<P> limb_at_words(const uint32_t *src, uint32_t W, uint32_t off, uint32_t n) {
    static_assert(P::N == 8, "four 64-bit words");
    const uint32_t wo = off >> 5, bs = off & 31u;
    uint32_t g[5];
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) g[i] = wo + i < W ? src[wo + i] : 0u;
    Fp<P> out;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) out.l[i] = low_bits((uint32_t)(((uint64_t)g[i + 1] << 32 | g[i]) >> bs), n > 32u * i ? n - 32u * i : 0u);
    out.l[4] = out.l[5] = out.l[6] = out.l[7] = 0;
    return out;
}

// the bits of word w of an array from bit `from` of the array upwards: non-zero where the array has a bit at or above `from` in that word
PM_HD uint32_t word_bits_from(uint32_t word, uint32_t w, uint32_t from) { return 32u * w >= from ? word : 32u * (w + 1) > from ? word >> (from - 32u * w) : 0u; }

// one declared WIDE long division on one assignment, serially: what the CPU rig's executor runs for KIND_LONGDIV_WIDE, and the
// statement of what k_solve_longdiv_wide computes with a wave.  Limbs leave Montgomery form and are accumulated at bit offset n j
// into WIDE_SUM_D and WIDE_SUM_E words; longdiv_wide_words divides; the kq n-bit limbs of the quotient and the kr of the remainder go
// back to Montgomery form.  Stuck at the hint's word (nr + h), with zero in every output:
//   E = 0;  D >= 2^8192;  E >= 2^4096;  q >= 2^(n kq);  rem >= 2^(n kr)
template <class P, class Sink>
inline void solve_longdiv_wide(const SolveStepDev<P> &s, const SolveHintDev &h, const uint32_t *hint_idx, Fp<P> *z, const Sink &stuck, WideCounters *counters = nullptr) {
    const uint32_t *q_cols = hint_idx + h.off, *r_cols = q_cols + h.kq, *d_cols = r_cols + h.kr, *e_words = d_cols + h.kD;
    std::vector<uint32_t> D(WIDE_SUM_D, 0), E(WIDE_SUM_E, 0), Q(WIDE_WD), R(WIDE_WE), U(WIDE_WD + 1), V(WIDE_WE);
    uint32_t bad = 0;
    for (uint32_t j = 0; j < h.kD; ++j) add_shifted_words(D.data(), WIDE_SUM_D, from_mont<P>(z[d_cols[j]]).l, h.n * j);
    if (h.literal) {
        for (int w = 0; w < WIDE_WE; ++w) E[w] = e_words[w];
        bad |= e_words[WIDE_WE];
    } else {
        for (uint32_t j = 0; j < h.kE; ++j) add_shifted_words(E.data(), WIDE_SUM_E, from_mont<P>(z[e_words[j]]).l, h.n * j);
    }
    for (int w = WIDE_WD; w < WIDE_SUM_D; ++w) bad |= D[w];
    for (int w = WIDE_WE; w < WIDE_SUM_E; ++w) bad |= E[w];
    bad |= longdiv_wide_words(D.data(), WIDE_WD, E.data(), WIDE_WE, Q.data(), R.data(), U.data(), V.data(), counters);
    for (uint32_t w = 0; w < (uint32_t)WIDE_WD; ++w) bad |= word_bits_from(Q[w], w, h.n * h.kq);
    for (uint32_t w = 0; w < (uint32_t)WIDE_WE; ++w) bad |= word_bits_from(R[w], w, h.n * h.kr);
    if (bad) stuck(s);
    const uint32_t mask = bad ? 0u : ~0u;
    for (uint32_t i = 0; i < h.kq + h.kr; ++i) {
        Fp<P> limb = i < h.kq ? limb_at_words<P>(Q.data(), WIDE_WD, h.n * i, h.n) : limb_at_words<P>(R.data(), WIDE_WE, h.n * (i - h.kq), h.n);
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[q_cols[i]] = to_mont<P>(limb);          // the remainder's columns follow the quotient's in the pool
    }
}

// One step of a chain, whatever its kind.  A range with an is-zero pair or a division row is a dividing one (the plan says so): the
// DIV = false body has no such branches.  An indicator row does not divide and is a branch of both.
template <class P, bool DIV, class Sink>
PM_HD void solve_any(const pmsolve::Csr &A, const pmsolve::Csr &B, const pmsolve::Csr &Cm, const SolveStepDev<P> &s, const uint32_t *__restrict__ bit_cols,
                     const SolvePairDev<P> *__restrict__ pairs, const SolveDivDev *__restrict__ divs, Fp<P> *z, const Sink &stuck) {
    if (s.kind == pmsolve::KIND_ISZERO) {
        // DIV = false would pass over the pair and leave both markers in place: solve_plan refuses a plan that asks for that
        if constexpr (DIV) solve_iszero<P>(A, B, Cm, s, pairs[s.bits], z);
    } else if (s.kind == pmsolve::KIND_DIVREM) {
        if constexpr (DIV) solve_divrem<P>(A, B, Cm, s, divs[s.bits], z, stuck);      // as above
    } else if (s.kind == pmsolve::KIND_INDICATOR) {
        solve_indicator<P>(A, B, s, z);
    } else if (s.kind == pmsolve::KIND_SQRT) {
        if constexpr (DIV) solve_sqrt<P>(Cm, s, z, stuck);                            // as above: a dividing range only
    } else if (s.bits) solve_bits<P, DIV>(A, B, Cm, s, bit_cols, z, stuck);
    else solve_step<P, DIV>(A, B, Cm, s, z, stuck);
}

}  // namespace pm
