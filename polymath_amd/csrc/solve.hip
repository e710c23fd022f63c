// PM_ASSIGNMENT_SOLVE: complete partial assignments on the device by forward propagation through the key's resident constraint rows
// (include/polymath_hip.h), so that a caller supplies only the values it chooses and the library computes the rest
// before it checks or proves.  The PLAN -- which row determines which column, in which order -- is host work, done once per (key,
// pattern) by host/solve_plan.hpp; what ONE step does to ONE assignment (solve_step, solve_bits, solve_iszero, solve_divrem,
// solve_indicator, solve_sqrt, solve_block, solve_longdiv, solve_moddiv, solve_modmuldiv, solve_longdiv_wide and its longdiv_wide_words, the dispatch
// solve_any, the inverses' solve_inverse and solve_block_invert, and the records a plan becomes: solve_records) is solve_steps.cuh,
// text that the CPU self-tests run as well; this file is the kernels that call it and the host driver, assignment = grid y (or the
// lane, in the chain kernel).  Before the plan's launches:
//   k_solve_pattern   one lane per (column, assignment): the unknown pattern of assignment 0 (a byte per column: 1 the unknown
//                     marker, 2 the quotient marker, 3 the indicator marker, 4 the square-root marker); every other assignment is
//                     compared with it, byte for byte, and the first differing (assignment, column) lowers one word
//   k_solve_inv       one lane per step, once per plan: 1 / coefficient of the step's unknown (a division row: 1 / cq); two more
//                     lanes per is-zero pair: 1 / cm and 1 / cb of its opener; an indicator step needs none and its record is left alone
// Then the launches, one entry per pmsolve::LaunchKind (solve_group's switch): the kernel, what a lane is, whether a step can stick.
//   LAUNCH_CHAIN      k_solve_chain<DIV>: a run of consecutive NARROW levels: one lane per assignment walks the run's steps in plan
//                     order.  A lane reads back only its own stores: no barriers, no fences.  The MiMC shape (depth 644, width 1) is
//                     one such run and the batch is its parallel dimension.  A step sticks as it would in the launch of its kind
//   LAUNCH_LEVEL      k_solve_level<DIV>: the ordinary steps of a WIDE dependency level: one lane per (step, assignment); a level is
//                     its own launch, so stream order is the dependency order.  Stuck where a kind-A / kind-B step would divide by zero
//   LAUNCH_BITS       k_solve_bits<DIV>: the bit decompositions of a wide level, one lane per (step, assignment) as well: a launch of
//                     their own, so that lanes doing one store do not sit beside lanes doing k.  Stuck, in all its k columns, where
//                     the value has no k-bit form or the divisor is zero
//   LAUNCH_ISZERO     k_solve_iszero: the is-zero pairs of a wide level, one lane per (step, assignment) as well: two stores and one
//                     inversion each.  Never stuck
//   LAUNCH_DIVREM     k_solve_divrem: the division rows of a wide level, one lane per (step, assignment) as well: two stores and one
//                     256-bit integer division each (divrem.cuh: a fixed trip count, so a wave does not diverge on operand size).
//                     Stuck, in both its columns, where the divisor is zero
//   LAUNCH_INDICATOR  k_solve_indicator: the indicator rows of a wide level, one lane per (step, assignment) as well: one dot product
//                     over the guard's known side, a zero test and one store of field one under a mask; no division.  Never stuck
//   LAUNCH_SQRT       k_solve_sqrt: the square-root rows of a wide level, one lane per (step, assignment) as well: one dot product over
//                     C_r, one multiplication by 1 / (ka kb) and one constant-time Tonelli-Shanks (sqrt.cuh: a fixed trip count, so a
//                     wave does not diverge on the operand); a non-residue is stuck at the row
//   LAUNCH_BLOCK      k_solve_block: the linear blocks of a level, whatever its width: one WAVE per (block, assignment), four to a
//                     workgroup.  Lane i < k forms the right-hand side of row i into LDS, lane j < k accumulates column j from the LDS
//                     values and the transposed inverse of the block's matrix, which solve_plan computed on the host once per plan
//                     (distinct matrices only: solve_steps.cuh, solve_block_invert).  No division, no atomic, never stuck
//   LAUNCH_LONGDIV    k_solve_longdiv: the declared long divisions of a level (pm_pk_set_hints), whatever its width: one lane per
//                     (hint, assignment).  The input limbs leave Montgomery form and are accumulated at bit offset n j into a 1024-bit
//                     dividend and a 512-bit divisor, a restoring shift-subtract divides in the launch's trip count (wave-uniform: the
//                     plan's bound, at most 1024; solve_steps.cuh: longdiv), and the n-bit limbs of quotient and remainder are stored.
//                     No register is indexed at run time; stuck at the word nr + h
//   LAUNCH_MODDIV     k_solve_moddiv: the declared modular divisions of a level, Z = (N+ - N-) / (D+ - D-) mod P, whatever its width:
//                     one lane per (hint, assignment).  The modulus and, one after the other, the four operand lists are accumulated
//                     like a dividend; each list is reduced modulo P by longdiv (the launch's reduction bound) and folded into N or D
//                     by masked selects; a binary extended Euclid for odd modulus with masked updates runs the launch's 2 L rounds
//                     with the numerator in place of 1, so that it ends in Z itself (solve_steps.cuh: modinv_odd proves the bound).
//                     No register is indexed at run time; stuck at the word nr + h
//   LAUNCH_LONGDIV_WIDE  k_solve_longdiv_wide: the declared WIDE long divisions of a level (opcode 5: up to 8192 / 4096 bits,
//                     RSA-2048), whatever its width: one WAVE per (hint, assignment), four to a workgroup.  No lane holds an operand:
//                     the 32-bit words of dividend, divisor and quotient live in the wave's slice of LDS, lane i working on words i,
//                     i + 64, ...  Gather: lane j stages limb j out of Montgomery form, the words are column sums of the staged limbs,
//                     one carry resolution by ballot.  Divide: Knuth's algorithm D in base 2^32, a word of quotient per step
//                     (solve_steps.cuh: longdiv_wide_words states the recurrence); lane i multiplies divisor word i, carries and
//                     borrows by ballot.  Scatter: lane i cuts limb i and stores it.  Every trip count is wave-uniform; stuck at the
//                     word nr + h
//   LAUNCH_MODMULDIV  k_solve_modmuldiv: the declared modular multiply-divides of a level (opcode 7: the slope 3 X^2 / (2 Y) of a
//                     tangent), cD (D+ - D-) Z = cN (A B + N+ - N-) mod P, whatever its width: one lane per (hint, assignment).  Nine
//                     phases in one rolled loop share one longdiv and one 16 x 16-word schoolbook product: the two factor lists, their
//                     product (reduced in the launch's 2 L rounds), the addend and denominator lists folded in by masked add and
//                     subtract modulo P, then the two one-word literals, which scale residues below P; the same Euclid ends in Z
//                     (solve_steps.cuh: solve_modmuldiv).  No register is indexed at run time; stuck at the word nr + h
// The chain, level and bits kernels exist twice: DIV = false for ranges of kind-C steps only, DIV = true for ranges with kind-A / kind-B steps,
// or is-zero pairs, which call inverse<P> (a Fermat chain) -- the plan sorts a level by kind, so kind-C ranges do not carry its
// registers, and the is-zero step and the division step (a dividing one by the plan's count, for 1 / cq) exist in the DIV = true
// chain only.  The indicator step does not divide: it is a branch of BOTH chain instantiations.  The square-root step (a dividing one
// by the plan's count, for 1 / (ka kb)) exists in the DIV = true chain only.  solve_plan checks every launch against the plan's table
// (pmsolve::KIND_INFO) before any of this runs.  After the launches:
//   k_solve_stuck_row of a REORDERED plan (build_plan_any_order found a dependency order that is not the matrix order): one lane per
//                     assignment turns the stuck word's (level, row) into the row
// A step that would divide by zero stores zero and lowers the assignment's stuck word to its row (64-bit atomic minimum: the same
// word on every run); so does a decomposition whose value has no k-bit form, in all its k columns, and a division row whose
// divisor is zero, in both its columns, and a square-root row whose value is a non-residue.  In matrix order everything
// downstream of a stuck row has a larger row, so the minimum is the root cause.  Under a reordered plan that is false -- a step that
// reads the stored zero may stick too, at a smaller row -- so the word is lowered to (level << 32) | row there: the minimum is the
// stuck step of lowest level, then smallest row, which read only valid values, and k_solve_stuck_row leaves its row in the word.
// Every other store has one writer.  An is-zero pair never sticks: where the tested value is zero its multiplier is free and is
// stored as zero.  Plain C++ and vector stores only.
#include <cstring>
#include <vector>

#include "internal.h"
#include "prove_common.cuh"
#include "solve_steps.cuh"

namespace pm {

using pmsolve::Csr;   // the kernels' matrices: the three pointers of CsrDev, under the name the step bodies know

// What a stuck step lowers the stuck word to.  The level is read HERE, on the rare path (a volatile load the compiler cannot hoist
// into the registers every step carries): the step bodies keep the registers they had.
template <class P>
__device__ __forceinline__ unsigned long long stuck_key(const SolveStepDev<P> &s) {
    const uint32_t level = *(const volatile uint32_t *)&s.level;
    return (unsigned long long)level << 32 | s.row;
}

// the step bodies' sink on the device (solve_steps.cuh): the assignment's stuck word, lowered by a 64-bit atomic minimum
struct StuckWord {
    unsigned long long *word;
    template <class P>
    __device__ __forceinline__ void operator()(const SolveStepDev<P> &s) const {
        atomicMin(word, stuck_key<P>(s));
    }
};

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

template <class P>
__global__ __launch_bounds__(256) void k_solve_inv(Csr A, Csr B, Csr Cm, SolveStepDev<P> *steps, uint64_t count, SolvePairDev<P> *pairs, uint64_t n_pairs,
                                                   const SolveDivDev *divs) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count + 2 * n_pairs) return;
    solve_inverse<P>(A, B, Cm, steps, count, pairs, divs, t);
}

template <class P, bool DIV>
__global__ __launch_bounds__(256) void k_solve_level(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, uint32_t lo, uint32_t hi, Fp<P> *xw,
                                                     uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_step<P, DIV>(A, B, Cm, steps[t], xw + b * ncols, StuckWord{stuck + b});
}

template <class P, bool DIV>
__global__ __launch_bounds__(256) void k_solve_bits(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, const uint32_t *__restrict__ bit_cols,
                                                    uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_bits<P, DIV>(A, B, Cm, steps[t], bit_cols, xw + b * ncols, StuckWord{stuck + b});
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_iszero(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, const SolvePairDev<P> *__restrict__ pairs,
                                                      uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_iszero<P>(A, B, Cm, steps[t], pairs[steps[t].bits], xw + b * ncols);
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_divrem(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, const SolveDivDev *__restrict__ divs,
                                                      uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_divrem<P>(A, B, Cm, steps[t], divs[steps[t].bits], xw + b * ncols, StuckWord{stuck + b});
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_indicator(Csr A, Csr B, const SolveStepDev<P> *__restrict__ steps, uint32_t lo, uint32_t hi, Fp<P> *xw,
                                                         uint64_t ncols) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_indicator<P>(A, B, steps[t], xw + b * ncols);
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_sqrt(Csr Cm, const SolveStepDev<P> *__restrict__ steps, uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols,
                                                    unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_sqrt<P>(Cm, steps[t], xw + b * ncols, StuckWord{stuck + b});
}

// One WAVE per (block, assignment), four to a workgroup.  Lane i < k forms the right-hand side of the block's row i (two dot products
// and one sweep of C_r that passes over the markers) and leaves it in LDS, 32 B per lane; after the barrier lane j < k accumulates
// column j from the k LDS values (the same address in every lane: a broadcast) and row i of the transposed inverse (consecutive
// elements across the lanes), and does its one store.  Every load of the assignment precedes the barrier and every store follows it,
// and the four blocks of a workgroup have disjoint columns at one level.  No lane leaves before the barrier; a wave past the range
// has k = 0.
template <class P>
__global__ __launch_bounds__(256) void k_solve_block(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, const SolveBlockDev *__restrict__ blocks,
                                                     const uint32_t *__restrict__ block_idx, const Fp<P> *__restrict__ block_inv, uint32_t lo, uint32_t hi, Fp<P> *xw,
                                                     uint64_t ncols) {
    __shared__ Fp<P> rhs[4][pmsolve::MAX_BLOCK];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * 4 + wave, b = blockIdx.y;
    Fp<P> *z = xw + b * ncols;
    SolveBlockDev blk{0, 0, 0, 0, 0};
    if (t < hi) blk = blocks[steps[t].bits];
    if (lane < blk.k) rhs[wave][lane] = solve_block_rhs<P>(A, B, Cm, block_idx[blk.rows_off + lane], z);
    __syncthreads();
    if (lane < blk.k) z[block_idx[blk.cols_off + lane]] = solve_block_out<P>(block_inv + blk.inv_off, blk.k, lane, rhs[wave]);
}

// One lane per (hint, assignment); 64 lanes to a workgroup, so that a level of a few hundred hints spreads over the device.  The lane
// holds the dividend (32 words), the divisor (16), the remainder (17) and the trial difference (17) in registers.
template <class P>
__global__ __launch_bounds__(64) void k_solve_longdiv(const SolveStepDev<P> *__restrict__ steps, const SolveHintDev *__restrict__ hints,
                                                      const uint32_t *__restrict__ hint_idx, uint32_t rounds, uint32_t lo, uint32_t hi, Fp<P> *xw,
                                                      uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_longdiv<P>(steps[t], hints[steps[t].bits], hint_idx, rounds, xw + b * ncols, StuckWord{stuck + b});
}

// One lane per (hint, assignment), as k_solve_longdiv.  The phases reuse registers: a list's 32-word sum, the 17-word remainder and
// trial difference are dead when the next list begins and when the Euclid's v and x2 come to life; the modulus, N and D (16 words
// each) live throughout.
template <class P>
__global__ __launch_bounds__(64) void k_solve_moddiv(const SolveStepDev<P> *__restrict__ steps, const SolveModDev *__restrict__ mods,
                                                     const uint32_t *__restrict__ hint_idx, uint32_t rounds, uint32_t inv_rounds, uint32_t lo, uint32_t hi,
                                                     Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_moddiv<P>(steps[t], mods[steps[t].bits], hint_idx, rounds, inv_rounds, xw + b * ncols, StuckWord{stuck + b});
}

// One lane per (hint, assignment), as k_solve_moddiv.  The modulus and the two residues (16 words each) live throughout; a phase's
// 32-word value, its 17-word remainder and trial difference and the product's two factors are dead when the next phase begins.
template <class P>
__global__ __launch_bounds__(64) void k_solve_modmuldiv(const SolveStepDev<P> *__restrict__ steps, const SolveMulDev *__restrict__ muls,
                                                        const uint32_t *__restrict__ hint_idx, uint32_t rounds, uint32_t inv_rounds, uint32_t lo, uint32_t hi,
                                                        Fp<P> *xw, uint64_t ncols, unsigned long long *stuck) {
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (t >= hi) return;
    solve_modmuldiv<P>(steps[t], muls[steps[t].bits], hint_idx, rounds, inv_rounds, xw + b * ncols, StuckWord{stuck + b});
}

// ---- k_solve_longdiv_wide: one wave, one division.  The wave's slice of LDS (5888 B; four waves to a workgroup: 23 KB):
//   stage  1024 words: the eight words of up to 128 staged limbs (dividend, then divisor); afterwards the quotient's 257 words
//   u      WIDE_SUM_D + 6 words: the dividend's column sums, then the normalised window of algorithm D, then the remainder
//   v      WIDE_SUM_E + 6 words: the divisor, normalised in place
// A lane writes words that other lanes read, so every such hand-over is a wave_sync(): LDS operations of one wave complete in order,
// the fence keeps the compiler from moving them across and waits for them.  No __syncthreads() after the kernel's head: the four
// waves of a workgroup have trip counts of their own.
struct WideLds {
    uint32_t stage[1024], u[WIDE_SUM_D + 6], v[WIDE_SUM_E + 6];
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The carry (or borrow) INTO each of a wave's 64 consecutive words of a multi-word addition, from the words' own bits: g, this word
// generates a carry whatever comes in; p, it passes one on (never both).  With G and P the ballots and h = G << 1 | cin, the binary
// addition P + h runs the same recurrence c[i + 1] = g[i] | p[i] & c[i] through its own carry chain, and (P + h) ^ P has c[i] in bit
// i.  -> this lane's carry-in; *cout: the carry out of word 63, the next 64 words' cin.
__device__ __forceinline__ uint32_t wave_carry(bool g, bool p, uint32_t lane, uint32_t cin, uint32_t *cout) {
    const uint64_t G = __ballot(g), Pm = __ballot(p);
    const uint64_t c = (Pm + (G << 1 | cin)) ^ Pm;
    *cout = (uint32_t)((G >> 63) | ((Pm >> 63) & (c >> 63)));
    return (uint32_t)(c >> lane) & 1u;
}

// Word w of sum_j limb_j 2^(n j) over the k staged limbs, before carries: below 2^39 (k <= 128 pieces of 32 bits).  Limb j reaches
// word w where n j < 32 w + 32 and n j + 256 > 32 w; its piece is 32 bits of the limb at the bit offset 32 w - n j in (-32, 256).
__device__ __forceinline__ uint64_t wide_column(const uint32_t *stage, uint32_t k, uint32_t n, uint32_t w) {
    if (k == 0) return 0;
    const uint32_t top = 32u * w + 31u, j_hi = min(k - 1u, top / n), j_lo = 32u * w >= 256u ? (32u * w - 256u) / n + 1u : 0u;
    uint64_t sum = 0;
    for (uint32_t j = j_lo; j <= j_hi; ++j) {
        const int r = (int)(32u * w) - (int)(n * j), wi = r >> 5;      // wi in -1..7
        const uint32_t bs = (uint32_t)r & 31u;
        const uint32_t lo = wi >= 0 ? stage[8 * j + wi] : 0u, hi = wi < 7 ? stage[8 * j + wi + 1] : 0u;
        sum += (uint32_t)(((uint64_t)hi << 32 | lo) >> bs);
    }
    return sum;
}

// The operand of k limbs (columns `cols` of z) into dst[0 .. cap): staged, summed by columns, carried.  Words are taken 64 at a time, lane i word 64 c + i.  dst[w] for w < cap is written, zero where the sum does not reach.
template <class P>
__device__ __forceinline__ void wide_gather(const Fp<P> *z, const uint32_t *__restrict__ cols, uint32_t k, uint32_t n, uint32_t *stage, uint32_t *dst, uint32_t cap,
                                            uint32_t lane) {
    for (uint32_t j = lane; j < k; j += 64) {
        const Fp<P> limb = from_mont<P>(z[cols[j]]);
#pragma unroll
        for (int w = 0; w < 8; ++w) stage[8 * j + w] = limb.l[w];
    }
    wave_sync();
    uint32_t cin = 0, hi_in = 0;          // uniform: the carry and the column's high part that the previous 64 words hand on
    for (uint32_t base = 0; base < cap; base += 64) {
        const uint32_t w = base + lane;
        const uint64_t col = w < cap ? wide_column(stage, k, n, w) : 0;
        uint32_t hi_prev = __shfl_up((uint32_t)(col >> 32), 1);
        if (lane == 0) hi_prev = hi_in;
        hi_in = wave_uniform(__shfl((uint32_t)(col >> 32), 63));
        const uint64_t sum = (uint64_t)(uint32_t)col + hi_prev;
        const uint32_t c = wave_carry((sum >> 32) != 0, (uint32_t)sum == 0xffffffffu, lane, cin, &cin);
        if (w < cap) dst[w] = (uint32_t)sum + c;
    }
    wave_sync();
}

// the significant words of a[0 .. cap): wave-uniform
__device__ __forceinline__ uint32_t wide_significant(const uint32_t *a, uint32_t cap, uint32_t lane) {
    uint32_t count = 0;
    for (uint32_t base = 0; base < cap; base += 64) {
        const uint64_t set = __ballot(base + lane < cap && a[base + lane] != 0);
        if (set) count = base + 64u - (uint32_t)__builtin_clzll(set);
    }
    return wave_uniform(count);
}

// non-zero where a[0 .. cap) has a bit at or above bit `from`: wave-uniform
__device__ __forceinline__ uint32_t wide_bits_from(const uint32_t *a, uint32_t cap, uint32_t from, uint32_t lane) {
    uint32_t any = 0;
    for (uint32_t base = 0; base < cap; base += 64) any |= __ballot(base + lane < cap && word_bits_from(a[base + lane], base + lane, from) != 0) != 0;
    return any;
}

template <class P>
__global__ __launch_bounds__(256) void k_solve_longdiv_wide(const SolveStepDev<P> *__restrict__ steps, const SolveHintDev *__restrict__ hints,
                                                            const uint32_t *__restrict__ hint_idx, uint32_t lo, uint32_t hi, Fp<P> *xw, uint64_t ncols,
                                                            unsigned long long *stuck) {
    __shared__ WideLds lds[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)lo + (uint64_t)blockIdx.x * 4 + wave, b = blockIdx.y;
    Fp<P> *z = xw + b * ncols;
    SolveHintDev h{1, 0, 0, 0, 0, 0, 0, 0};          // a wave past the range: an empty hint, every loop of zero trips
    if (t < hi) h = hints[steps[t].bits];
    const uint32_t n = h.n, kq = min(h.kq, (uint32_t)pmsolve::WIDE_MAX_KQ), kr = min(h.kr, (uint32_t)pmsolve::WIDE_MAX_KR), kD = min(h.kD, (uint32_t)pmsolve::WIDE_MAX_KD),
                   kE = min(h.kE, (uint32_t)pmsolve::WIDE_MAX_KE);
    const uint32_t *q_cols = hint_idx + h.off, *r_cols = q_cols + h.kq, *d_cols = r_cols + h.kr, *e_words = d_cols + h.kD;
    uint32_t *stage = lds[wave].stage, *u = lds[wave].u, *v = lds[wave].v, *q = stage;
    constexpr uint32_t U_CAP = WIDE_SUM_D + 6, V_CAP = WIDE_SUM_E + 6;

    // ---- gather
    uint32_t bad = 0;
    wide_gather<P>(z, d_cols, kD, n, stage, u, U_CAP, lane);
    if (h.literal) {
        for (uint32_t w = lane; w < V_CAP; w += 64) v[w] = w < (uint32_t)WIDE_WE ? e_words[w] : 0u;
        bad |= e_words[WIDE_WE];
        wave_sync();
    } else {
        wide_gather<P>(z, e_words, kE, n, stage, v, V_CAP, lane);
    }
    const uint32_t t_all = wide_significant(u, U_CAP, lane), m_all = wide_significant(v, V_CAP, lane);
    bad |= (uint32_t)(t_all > (uint32_t)WIDE_WD) | (uint32_t)(m_all > (uint32_t)WIDE_WE) | (uint32_t)(m_all == 0);
    bad = wave_uniform(bad);
    // a stuck division divides nothing: zero trips below, zero in every output
    const uint32_t m = bad ? 0u : m_all, tw = bad ? 0u : t_all;
    for (uint32_t w = lane; w < 260; w += 64) q[w] = 0;          // the staged limbs are dead (wide_gather ends in a wave_sync)

    // ---- divide.  Normalise: v <<= s over m words, u <<= s over tw + 1 words, every word read before any is written
    const uint32_t v_top = m ? v[m - 1] : 1u, s = wave_uniform((uint32_t)__builtin_clz(v_top | (m ? 0u : 0x80000000u)));
    {
        uint32_t keep_v[2], keep_u[5];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t i = 64 * c + lane;
            keep_v[c] = i < m ? (s ? v[i] << s | (i ? v[i - 1] >> (32 - s) : 0u) : v[i]) : 0u;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const uint32_t i = 64 * c + lane;
            keep_u[c] = i <= tw ? (s ? u[i] << s | (i ? u[i - 1] >> (32 - s) : 0u) : u[i]) : 0u;
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (64 * c + lane < m) v[64 * c + lane] = keep_v[c];
#pragma unroll
        for (int c = 0; c < 5; ++c)
            if (64 * c + lane <= tw) u[64 * c + lane] = keep_u[c];
        wave_sync();
    }
    const uint32_t v1 = wave_uniform(m ? v[m - 1] : 1u), v0 = wave_uniform(m >= 2 ? v[m - 2] : 0u);
    for (uint32_t j = m && tw >= m ? tw - m + 1 : 0; j-- > 0;) {
        uint32_t saturated;
        uint32_t qhat = wave_uniform(wide_estimate(u[j + m], u[j + m - 1], m >= 2 ? u[j + m - 2] : 0u, v1, v0, &saturated));
        // u[j .. j + m) -= qhat v, 64 words at a time: the product's words first (lane i: the low half of qhat v[i] plus the high half
        // of qhat v[i - 1], carried), then the difference; a lane past the divisor passes carries and borrows on
        uint32_t carry = 0, borrow = 0;
        for (uint32_t base = 0; base < m; base += 64) {
            const uint32_t i = base + lane;
            const bool on = i < m;
            const uint64_t sum = on ? (uint64_t)(qhat * v[i]) + (i ? __umulhi(qhat, v[i - 1]) : 0u) : 0u;
            const uint32_t c = wave_carry(on && (sum >> 32) != 0, !on || (uint32_t)sum == 0xffffffffu, lane, carry, &carry);
            const uint32_t prod = (uint32_t)sum + c, word = on ? u[j + i] : 0u;
            const uint32_t bw = wave_carry(on && word < prod, !on || word == prod, lane, borrow, &borrow);
            if (on) u[j + i] = word - prod - bw;
        }
        // the window's top word, in every lane alike: the product's last word is the high half of qhat v[m - 1] and the last carry
        const uint64_t top = (uint64_t)__umulhi(qhat, v1) + carry + borrow;
        const uint32_t u_top = u[j + m];
        const bool back = wave_uniform(top > u_top) != 0;
        wave_sync();
        if (back) {          // the estimate was one too large: add the divisor back
            uint32_t c_in = 0;
            for (uint32_t base = 0; base < m; base += 64) {
                const uint32_t i = base + lane;
                const bool on = i < m;
                const uint64_t sum = on ? (uint64_t)u[j + i] + v[i] : 0u;
                const uint32_t c = wave_carry(on && (sum >> 32) != 0, !on || (uint32_t)sum == 0xffffffffu, lane, c_in, &c_in);
                if (on) u[j + i] = (uint32_t)sum + c;
            }
            --qhat;          // the carry out cancels the borrow: the top word is zero
        }
        if (lane == 0) {
            u[j + m] = back ? 0u : u_top - (uint32_t)top;
            q[j] = qhat;
        }
        wave_sync();
    }
    // de-normalise: rem = u >> s over m words, read before written
    {
        uint32_t keep[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t i = 64 * c + lane;
            keep[c] = i < m ? (s ? u[i] >> s | u[i + 1] << (32 - s) : u[i]) : 0u;
        }
        wave_sync();
        for (uint32_t w = lane; w < U_CAP; w += 64) u[w] = w < 64 ? keep[0] : w < 128 ? keep[1] : 0u;
        wave_sync();
    }

    // ---- scatter
    bad |= wide_bits_from(q, 260, n * kq, lane) | wide_bits_from(u, WIDE_WE, n * kr, lane);
    bad = wave_uniform(bad);
    const uint32_t mask = bad ? 0u : ~0u;
    for (uint32_t i = lane; i < kq + kr; i += 64) {
        Fp<P> limb = i < kq ? limb_at_words<P>(q, 260, n * i, n) : limb_at_words<P>(u, WIDE_WE, n * (i - kq), n);
#pragma unroll
        for (int w = 0; w < P::N; ++w) limb.l[w] &= mask;
        z[q_cols[i]] = to_mont<P>(limb);          // the remainder's columns follow the quotient's in the pool
    }
    if (bad && lane == 0 && t < hi) StuckWord{stuck + b}(steps[t]);
}

// the step index is the same in every lane: the step record, the pair record, the row's CSR metadata and a decomposition's column
// list are uniform loads (solve_steps.cuh: solve_any, the dispatch by kind).
template <class P, bool DIV>
__global__ __launch_bounds__(64) void k_solve_chain(Csr A, Csr B, Csr Cm, const SolveStepDev<P> *__restrict__ steps, const uint32_t *__restrict__ bit_cols,
                                                    const SolvePairDev<P> *__restrict__ pairs, const SolveDivDev *__restrict__ divs, uint32_t lo, uint32_t hi,
                                                    Fp<P> *xw, uint64_t ncols, unsigned long long *stuck, uint64_t rows) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    Fp<P> *z = xw + b * ncols;
    for (uint32_t t = lo; t < hi; ++t) solve_any<P, DIV>(A, B, Cm, steps[t], bit_cols, pairs, divs, z, StuckWord{stuck + b});
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

inline Csr csr_dev(const pm_pk *pk, int i) { return Csr{pk->d_rowptr[i], pk->d_col[i], pk->d_val[i]}; }

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
    if (sv.plan_key == pk->serial && sv.plan_hint_gen == pk->hint_gen && sv.plan_pattern == pattern) return PM_OK;
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
    sv.plan = pmsolve::build_plan_any_order(m, nr, pk->m0, pk->mw, pattern.data(), pmsolve::WIDE_STEPS, modulus, pk->hints.empty() ? nullptr : &pk->hints);
    if (sv.plan.error != pmsolve::OK) {
        ctx->err = "pm solve: " + sv.plan.message;
        return PM_ERR_INVALID_ARG;
    }
    // every launch against KIND_INFO: a step of a chain must be one that a lane can walk, a step of any other launch must map to that
    // launch's kind, and a dividing kind needs a dividing launch -- the DIV = false kernels have no is-zero step, no division step and
    // no square-root step in them, and no inverse<P>
    for (const pmsolve::Launch &l : sv.plan.launches)
        for (uint32_t t = l.lo; t < l.hi; ++t) {
            const pmsolve::Step &s = sv.plan.steps[t];
            const pmsolve::KindInfo info = s.kind < pmsolve::NUM_MULDIV_KINDS ? pmsolve::KIND_INFO[s.kind] : pmsolve::KindInfo{0xff, 0, 0};
            const char *why = l.kind == pmsolve::LAUNCH_CHAIN ? (info.chained ? nullptr : "into a chain, where no lane can walk it")
                              : info.launch != l.kind         ? "into a launch of another kind"
                                                              : nullptr;
            if (!why && info.divides && !l.divides) why = "into a launch that does not divide";
            if (why) {
                ctx->err = std::string("pm solve: the plan puts the ") +
                           (s.kind == pmsolve::KIND_ISZERO ? "is-zero pair" : s.kind == pmsolve::KIND_SQRT ? "square root" : s.kind == pmsolve::KIND_DIVREM ? "division" : "step") +
                           " of row " + std::to_string(s.row) + " " + why;
                return PM_ERR_STATE;
            }
        }
    const size_t n_steps = sv.plan.steps.size();
    sv.n_hints = sv.n_mods = sv.n_muls = 0;
    if (n_steps) {
        SolveRecords<P> rec = solve_records<P>(sv.plan);
        // the linear blocks' matrices are constants of the key: each distinct one is inverted here, once per plan, from the words the
        // planner copied out of C; a singular one refuses the call before any assignment is touched
        if (!rec.blocks.empty()) {
            uint32_t column = 0;
            const size_t bad = solve_block_inverses<P>(sv.plan, rec, &column);
            if (bad != sv.plan.blocks.size()) {
                const pmsolve::BlockRows &blk = sv.plan.blocks[bad];
                const auto list = [](const std::vector<uint32_t> &v) {
                    std::string out;
                    for (size_t i = 0; i < v.size(); ++i) out += (i ? ", " : "") + std::to_string(v[i]);
                    return out;
                };
                ctx->err = "pm solve: rows " + list(blk.rows) + ": the linear block over columns " + list(blk.cols) + " is singular (no pivot in column " +
                           std::to_string(blk.cols[column]) + ")";
                return PM_ERR_INVALID_ARG;
            }
        }
        sv.n_hints = rec.hints.size();
        sv.n_mods = rec.mods.size();
        sv.n_muls = rec.muls.size();
        PM_HIP(ctx, sv.blocks.upload(rec.blocks, st));
        PM_HIP(ctx, sv.block_idx.upload(rec.block_idx, st));
        PM_HIP(ctx, sv.block_inv.upload(rec.block_inv, st));
        PM_HIP(ctx, sv.hints.upload(rec.hints, st));
        PM_HIP(ctx, sv.mods.upload(rec.mods, st));
        PM_HIP(ctx, sv.muls.upload(rec.muls, st));
        PM_HIP(ctx, sv.hint_idx.upload(rec.hint_idx, st));
        PM_HIP(ctx, sv.pairs.upload(rec.pairs, st));
        PM_HIP(ctx, sv.divs.upload(rec.divs, st));
        PM_HIP(ctx, sv.bit_cols.upload(sv.plan.bit_cols, st));
        PM_HIP(ctx, sv.steps.upload(rec.steps, st));
        PM_LAUNCH(ctx, k_solve_inv<P>, dim3(nblk(n_steps + 2 * rec.pairs.size())), dim3(256), 0, st, csr_dev(pk, 0), csr_dev(pk, 1), csr_dev(pk, 2),
                       sv.steps.as<SolveStepDev<P>>(), (uint64_t)n_steps, rec.pairs.empty() ? nullptr : sv.pairs.as<SolvePairDev<P>>(), (uint64_t)rec.pairs.size(),
                       rec.divs.empty() ? nullptr : sv.divs.as<SolveDivDev>());
        PM_HIP(ctx, hipStreamSynchronize(st));   // `rec` goes out of scope
    }
    sv.plan_pattern.swap(pattern);
    sv.plan_key = pk->serial;
    sv.plan_hint_gen = pk->hint_gen;
    return PM_OK;
}

template <class C>
int solve_group(pm_ctx *ctx, const pm_pk *pk, Fp<typename C::FrP> *d_xw, size_t g, size_t g0, int timing_slot) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    SolveWs &sv = ctx->sv;
    const uint64_t m0 = pk->m0, ncols = m0 + pk->mw;
    if (g == 0 || g > 65535 || sv.plan_key != pk->serial || sv.plan_hint_gen != pk->hint_gen || (g0 + g) * 4 * (1 + m0) > sv.tap9.size()) return PM_ERR_STATE;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    PM_HIP(ctx, sv.stuck.reserve(g * sizeof(unsigned long long)));
    unsigned long long *stuck = sv.stuck.as<unsigned long long>();
    PM_HIP(ctx, hipMemsetAsync(stuck, 0xff, g * sizeof(unsigned long long), st));
    const Csr A = csr_dev(pk, 0), B = csr_dev(pk, 1), Cm = csr_dev(pk, 2);
    const SolveStepDev<P> *steps = sv.steps.as<SolveStepDev<P>>();
    const uint32_t *bit_cols = sv.plan.bit_cols.empty() ? nullptr : sv.bit_cols.as<uint32_t>();
    const SolvePairDev<P> *pairs = sv.plan.pairs.empty() ? nullptr : sv.pairs.as<SolvePairDev<P>>();
    const SolveDivDev *divs = sv.plan.divs.empty() ? nullptr : sv.divs.as<SolveDivDev>();
    const SolveHintDev *hints = sv.hints.as<SolveHintDev>();
    const uint32_t *hint_idx = sv.hint_idx.as<uint32_t>();
    {
        StageTimer t(ctx, timing_slot);
        for (const pmsolve::Launch &l : sv.plan.launches) {
            const uint32_t count = l.hi - l.lo;
            const dim3 lanes(nblk(count), (unsigned)g), waves(nblk(count, 4), (unsigned)g), hint_lanes(nblk(count, 64), (unsigned)g), chain(nblk(g, 64));
            switch (l.kind) {   // the cases stand in the order the kernels have in the code object: they are instantiated here
            case pmsolve::LAUNCH_BLOCK:
                if (sv.plan.blocks.empty()) return PM_ERR_STATE;
                hipLaunchKernelGGL((k_solve_block<P>), waves, dim3(256), 0, st, A, B, Cm, steps, sv.blocks.as<SolveBlockDev>(), sv.block_idx.as<uint32_t>(),
                                   sv.block_inv.as<Fp<P>>(), l.lo, l.hi, d_xw, ncols);
                break;
            case pmsolve::LAUNCH_LONGDIV:
                if (!sv.n_hints || l.rounds < 256 || l.rounds > 1024) return PM_ERR_STATE;
                hipLaunchKernelGGL((k_solve_longdiv<P>), hint_lanes, dim3(64), 0, st, steps, hints, hint_idx, l.rounds, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            case pmsolve::LAUNCH_MODDIV:
                if (!sv.n_mods || l.rounds < 256 || l.rounds > 1024 || l.inv_rounds < 512 || l.inv_rounds > 1024) return PM_ERR_STATE;
                hipLaunchKernelGGL((k_solve_moddiv<P>), hint_lanes, dim3(64), 0, st, steps, sv.mods.as<SolveModDev>(), hint_idx, l.rounds, l.inv_rounds, l.lo, l.hi, d_xw,
                                   ncols, stuck);
                break;
            case pmsolve::LAUNCH_MODMULDIV:
                if (!sv.n_muls || l.rounds < 256 || l.rounds > 1024 || l.inv_rounds < 512 || l.inv_rounds > 1024) return PM_ERR_STATE;
                hipLaunchKernelGGL((k_solve_modmuldiv<P>), hint_lanes, dim3(64), 0, st, steps, sv.muls.as<SolveMulDev>(), hint_idx, l.rounds, l.inv_rounds, l.lo, l.hi, d_xw,
                                   ncols, stuck);
                break;
            case pmsolve::LAUNCH_LONGDIV_WIDE:
                if (!sv.n_hints || l.rounds < 256 || l.rounds > pmsolve::WIDE_D_BITS) return PM_ERR_STATE;
                hipLaunchKernelGGL((k_solve_longdiv_wide<P>), waves, dim3(256), 0, st, steps, hints, hint_idx, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            case pmsolve::LAUNCH_CHAIN:
                if (l.divides) hipLaunchKernelGGL((k_solve_chain<P, true>), chain, dim3(64), 0, st, A, B, Cm, steps, bit_cols, pairs, divs, l.lo, l.hi, d_xw, ncols, stuck, (uint64_t)g);
                else hipLaunchKernelGGL((k_solve_chain<P, false>), chain, dim3(64), 0, st, A, B, Cm, steps, bit_cols, pairs, divs, l.lo, l.hi, d_xw, ncols, stuck, (uint64_t)g);
                break;
            case pmsolve::LAUNCH_SQRT:
                hipLaunchKernelGGL((k_solve_sqrt<P>), lanes, dim3(256), 0, st, Cm, steps, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            case pmsolve::LAUNCH_INDICATOR:
                hipLaunchKernelGGL((k_solve_indicator<P>), lanes, dim3(256), 0, st, A, B, steps, l.lo, l.hi, d_xw, ncols);
                break;
            case pmsolve::LAUNCH_DIVREM:
                hipLaunchKernelGGL((k_solve_divrem<P>), lanes, dim3(256), 0, st, A, B, Cm, steps, divs, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            case pmsolve::LAUNCH_ISZERO:
                hipLaunchKernelGGL((k_solve_iszero<P>), lanes, dim3(256), 0, st, A, B, Cm, steps, pairs, l.lo, l.hi, d_xw, ncols);
                break;
            case pmsolve::LAUNCH_BITS:
                if (l.divides) hipLaunchKernelGGL((k_solve_bits<P, true>), lanes, dim3(256), 0, st, A, B, Cm, steps, bit_cols, l.lo, l.hi, d_xw, ncols, stuck);
                else hipLaunchKernelGGL((k_solve_bits<P, false>), lanes, dim3(256), 0, st, A, B, Cm, steps, bit_cols, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            case pmsolve::LAUNCH_LEVEL:
                if (l.divides) hipLaunchKernelGGL((k_solve_level<P, true>), lanes, dim3(256), 0, st, A, B, Cm, steps, l.lo, l.hi, d_xw, ncols, stuck);
                else hipLaunchKernelGGL((k_solve_level<P, false>), lanes, dim3(256), 0, st, A, B, Cm, steps, l.lo, l.hi, d_xw, ncols, stuck);
                break;
            default:
                return PM_ERR_STATE;
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
