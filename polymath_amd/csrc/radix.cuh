// Window radix R = m 2^a of the table-mode MSM (m = 5; m = 1 is the ragged power-of-two layout of msm_plan.h: win_off / win_width).
//
// A power-of-two radix quantises the window count: 12 windows need 22-bit digits (2^21 buckets, two thirds of the windows fill only
// the lower half), 11 need 2^23 buckets.  R = 5 2^a sits between: 12 windows on 5 2^19 (1.31 M buckets), 11 on 5 2^21 (5.24 M).
// The recoding is exact integer arithmetic on the canonical scalar: per window the low `a` bits, then a division by 5 (limb-wise
// long division from the top limb, a 3-bit remainder and a multiply-high by the reciprocal of 5 -- no hardware division), then
// msm.hip's signed-digit rule with full = R, half = R / 2.
//
// Plain C++: the kernels of msm.hip, the planners of msm_plan.h and the CPU self-tests (tests/native/radix_selftest.cpp, msm_plan_selftest.cpp) share it.
// Every shift, limb count and limb index below is a compile-time constant of (windows, a): the recursion over the window index is
// what makes them so (a loop over a run-time layout makes the compiler park the scalar in LDS, see msm.hip: digit_at).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_RADIX_HD __host__ __device__ __forceinline__
#else
#define PM_RADIX_HD inline
#endif

namespace pm {

constexpr uint32_t RADIX_NO_DIGIT = 0xFFFFFFFFu;

// The top digit never carries out:  (r - 1) div R^(W-1) + 1 <= R / 2,  R = m 2^a, r = P::MOD (odd).  With X = R^(W-1), H = R / 2:
// floor((r - 1) / X) <= H - 1  <=>  r - 1 < H X = m^W 2^(aW - 1)  <=>  (r - 1) >> (aW - 1) < m^W.   Exact, on 32-bit limbs.
template <class P>
constexpr bool radix_top_fits(unsigned m, unsigned W, unsigned a) {
    static_assert(P::N == 8, "256-bit scalars");
    if (m == 0 || m > 7 || W == 0 || a == 0 || a > 28) return false;
    uint32_t p[8] = {1, 0, 0, 0, 0, 0, 0, 0};                     // m^W
    for (unsigned j = 0; j < W; ++j) {
        uint64_t c = 0;
        for (int i = 0; i < 8; ++i) {
            c += (uint64_t)p[i] * m;
            p[i] = (uint32_t)c;
            c >>= 32;
        }
        if (c) return true;                                        // m^W >= 2^256 > r
    }
    const unsigned s = a * W - 1;
    if (s >= 256) return true;                                     // (r - 1) >> s = 0 < m^W
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};                      // (r - 1) >> s
    for (int i = 0; i < 8; ++i) {
        const unsigned src = (unsigned)i + s / 32;
        if (src >= 8) break;
        const uint32_t lo = P::MOD[src] - (src == 0 ? 1u : 0u);    // r is odd: r - 1 borrows nothing
        const uint32_t hi = src + 1 < 8 ? P::MOD[src + 1] : 0u;
        t[i] = s % 32 ? (lo >> (s % 32)) | (hi << (32 - s % 32)) : lo;
    }
    for (int i = 7; i >= 0; --i)
        if (t[i] != p[i]) return t[i] < p[i];
    return false;
}
// the smallest shift whose radix m 2^a covers the field in W windows; 0 if none does
template <class P>
constexpr unsigned radix_min_shift(unsigned m, unsigned W) {
    for (unsigned a = 1; a <= 28; ++a)
        if (radix_top_fits<P>(m, W, a)) return a;
    return 0;
}

// Window w of the recoding below: k = the scalar div R^w on entry, div R^(w+1) on exit.  A division by 5 2^A takes off at least
// A + 2 bits, so no more than 256 - w (A + 2) bits of k are live here: the limbs above them are zero and are not touched.
template <unsigned W, unsigned A, unsigned w>
PM_RADIX_HD void radix5_recode_from(uint32_t (&k)[8], uint32_t &carry, uint32_t (&out)[W]) {
    if constexpr (w < W) {
        constexpr int bits = 256 - (int)(w * (A + 2));
        constexpr int nl = bits > 0 ? (bits + 31) / 32 : 0;                    // live limbs before the shift ...
        constexpr int nl2 = bits > (int)A ? (bits - (int)A + 31) / 32 : 0;     // ... and after it
        const uint32_t low = nl ? k[0] & ((1u << A) - 1) : 0u;
#pragma unroll
        for (int i = 0; i < nl; ++i) k[i] = (k[i] >> A) | (i + 1 < nl ? k[i + 1] << (32 - A) : 0u);
        // (k, rem) = divmod(k, 5) from the top limb:  rem 2^32 + x = 5 (rem 0x33333333 + t) + (rem + xr),  x = 5 t + xr
        uint32_t rem = 0;
#pragma unroll
        for (int i = nl2 - 1; i >= 0; --i) {
            const uint32_t x = k[i];
            const uint32_t t = (uint32_t)(((uint64_t)x * 0xCCCCCCCDu) >> 34);   // x div 5: one multiply-high
            const uint32_t s = rem + (x - 5u * t);                              // <= 8
            const uint32_t e = s >= 5u ? 1u : 0u;
            k[i] = rem * 0x33333333u + t + e;
            rem = s - 5u * e;
        }
        // the signed step (msm.hip: digit_at), full = R, half = R / 2; branch-free
        constexpr uint32_t full = 5u << A, half = 5u << (A - 1);
        const uint32_t d = (rem << A) + low + carry;
        const bool over = d > half;
        const uint32_t m = over ? full - d : d;
        carry = over ? 1u : 0u;
        out[w] = m ? ((m - 1) << 1) | carry : RADIX_NO_DIGIT;
        radix5_recode_from<W, A, w + 1>(k, carry, out);
    }
}

// Signed digits of the canonical scalar k < r (eight 32-bit limbs) in radix R = 5 2^A over W windows:  k = sum_j d_j R^j,
// |d_j| <= R / 2.  out[j] = (|d_j| - 1) << 1 | (d_j < 0), the bucket and the negate flag; RADIX_NO_DIGIT for d_j = 0.
// Returns the carry out of the last window: 0 whenever radix_top_fits<P>(5, W, A) holds for k's field.
template <unsigned W, unsigned A>
PM_RADIX_HD uint32_t radix5_recode(const uint32_t (&scalar)[8], uint32_t (&out)[W]) {
    static_assert(A >= 1 && A <= 28, "R / 2 + 1 and (bucket << 1 | sign) fit 32 bits");
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = scalar[i];
    uint32_t carry = 0;
    radix5_recode_from<W, A, 0>(k, carry, out);
    return carry;
}

}  // namespace pm
