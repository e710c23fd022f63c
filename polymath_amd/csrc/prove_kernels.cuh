// The prover's kernels on whole vectors, written once for prove.hip (one proof) and prove_batch.hip (a group of proofs as [rows][len]
// arrays).  A proof's vectors, and with them its three points, are the same bytes from either file because both launch this text.
//
// Kernels whose arguments are the same for every proof take the proof as blockIdx.y and explicit row strides; prove.hip launches them
// with grid y = 1.  Where a value differs from proof to proof (x1, the numerator's constants and reduced-radix multipliers, the
// division's level multipliers) the body is a __device__ function on one proof's pointers and values with two entry points: `k_x`
// takes the values as kernel arguments (prove.hip), `k_x_rows` reads them from the BatchRow record (batch_row.cuh) of row blockIdx.y (prove_batch.hip).
#pragma once
#include "internal.h"
#include "fq28.cuh"
#include "prove_common.cuh"

namespace pm {

// ------------------------------------------------------------------------------- witness map
template <class P>
__global__ void k_witness_rows(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *xw, uint64_t xw_stride, Fp<P> *ue, Fp<P> *we, uint64_t n,
                               Fp<P> *y, uint64_t y_stride, uint64_t m0, uint64_t nr) {
    const uint64_t b = blockIdx.y;
    xw += b * xw_stride; ue += b * n; we += b * n; y += b * y_stride;
    uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    Fp<P> az = csr_row_dot<P>(A.rowptr, A.col, A.val, xw, r);
    Fp<P> bz = csr_row_dot<P>(B.rowptr, B.col, B.val, xw, r);
    Fp<P> cz = csr_row_dot<P>(Cm.rowptr, Cm.col, Cm.val, xw, r);
    Fp<P> d = sub<P>(az, bz), d2 = sqr<P>(d);
    Fp<P> c4 = dbl<P>(dbl<P>(cz));
    y[m0 + r] = d2;
    ue[2 * m0 + r] = add<P>(az, bz);
    we[2 * m0 + r] = add<P>(c4, d2);
    ue[2 * m0 + nr + r] = d;
    we[2 * m0 + nr + r] = d2;
}

// rows < 2 m0 (public-input rows), the x||w prefix of z_tail, and zero padding rows >= 2(m0+nr)
template <class P>
__global__ void k_witness_head(const Fp<P> *xw, uint64_t xw_stride, Fp<P> *ue, Fp<P> *we, Fp<P> *ztail, uint64_t z_stride, uint64_t m0,
                               uint64_t mw, uint64_t nr, uint64_t n) {
    const uint64_t b = blockIdx.y;
    xw += b * xw_stride; ue += b * n; we += b * n; ztail += b * z_stride;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fp<P> one = Fp<P>::one();
    if (i < m0 + mw) ztail[i] = xw[i];
    Fp<P> *y = ztail + m0 + mw;
    if (i < m0) {
        Fp<P> xi = xw[i];
        Fp<P> omx = sub<P>(one, xi), yi = i ? sqr<P>(omx) : Fp<P>::zero();
        y[i] = yi;
        if (i == 0) {
            ue[0] = dbl<P>(one);
            we[0] = dbl<P>(dbl<P>(one));
            ue[m0] = Fp<P>::zero();
            we[m0] = Fp<P>::zero();
        } else {
            ue[i] = add<P>(one, xi);
            we[i] = add<P>(dbl<P>(dbl<P>(xi)), yi);
            ue[m0 + i] = omx;
            we[m0 + i] = yi;
        }
    }
    uint64_t rows = 2 * (m0 + nr);
    if (i >= rows && i < n) {
        ue[i] = Fp<P>::zero();
        we[i] = Fp<P>::zero();
    }
}

// flags (one word per proof): bit0 = (Uz)^2 != Wz somewhere (== rem != 0, prover.rs:108), bit1 = h[n-1] != 0 (deg h > n-2),
// bit2 = h has a non-zero coefficient (cleared means h == 0, prover.rs:107), bit3 = division remainder != 0
template <class P>
__global__ void k_check_sap(const Fp<P> *ue, const Fp<P> *we, uint64_t n, unsigned *flags) {
    const uint64_t b = blockIdx.y;
    ue += b * n; we += b * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!sqr<P>(ue[i]).eq(we[i])) atomicOr(flags + b, 1u);
}

template <class P>
__global__ void k_copy_zero_head(const Fp<P> *src, Fp<P> *dst, uint64_t n, uint64_t zero_rows) {
    const uint64_t b = blockIdx.y;
    src += b * n; dst += b * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = i < zero_rows ? Fp<P>::zero() : src[i];
}

// Coefficients of the witness-only part of u (N5, prover.rs:160-162) without a transform: its evaluations are
// u's with the first `head` rows zeroed, so  wit_u = u - iNTT(head rows)  and the iNTT of a `head`-sparse
// vector is a direct sum:  wit_u[k] = u[k] - n^-1 sum_{j < head} ue[j] w^(-jk)   (head = 2 m0, Horner in w^-k).
// winv[k] = w^-k for k < n/2 (the inverse twiddle table); w^-(k + n/2) = -w^-k.
template <class P>
__global__ void k_wit_u_sparse(const Fp<P> *u, const Fp<P> *ue, const Fp<P> *winv, Fp<P> ninv, uint64_t n, unsigned head, Fp<P> *wit_u) {
    const uint64_t b = blockIdx.y;
    u += b * n; ue += b * n; wit_u += b * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t half = n >> 1;
    Fp<P> wk = winv[k < half ? k : k - half];
    if (k >= half) wk = neg<P>(wk);
    Fp<P> s = ue[head - 1];
    for (int j = (int)head - 2; j >= 0; --j) s = add<P>(mul<P>(s, wk), ue[j]);
    wit_u[k] = sub<P>(u[k], mul<P>(s, ninv));
}

// u^2 without a size-2n transform.  Once (Uz)^2 == Wz holds on the domain (k_check_sap), u^2 = w  (mod X^n - 1),
// i.e. lo + hi = w for u^2 = lo + X^n hi.  The negacyclic product neg = u^2 mod (X^n + 1) = lo - hi comes from ONE
// size-n transform pair on the twisted input u_k psi^k (psi = omega_2n):  lo = (w + neg) / 2, hi = (w - neg) / 2.
// Same coefficients as square_polynomial (prover.rs:315-328) at half the NTT work.
template <class P>
__global__ void k_twist(const Fp<P> *u, const Fp<P> *psi_pow, Fp<P> *out, uint64_t n) {
    const uint64_t b = blockIdx.y;
    u += b * n; out += b * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = mul<P>(u[k], psi_pow[k]);
}
template <class P>
__global__ void k_untwist_combine(const Fp<P> *neg_tw, const Fp<P> *psi_inv_pow, const Fp<P> *w, Fp<P> *u2, uint64_t n, Fp<P> half) {
    const uint64_t b = blockIdx.y;
    neg_tw += b * n; w += b * n; u2 += b * 2 * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Fp<P> neg = mul<P>(neg_tw[k], psi_inv_pow[k]), wk = w[k];
    u2[k] = mul<P>(add<P>(wk, neg), half);
    u2[n + k] = mul<P>(sub<P>(wk, neg), half);
}

template <class P>
__global__ void k_square(Fp<P> *a, uint64_t n) {
    a += (uint64_t)blockIdx.y * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = sqr<P>(a[i]);
}

// ------------------------------------------------------------------------------- phase-1 scalars
// Scalar vectors of the two phase-1 MSMs, laid out to match the pk's base concatenation:
//   sc_c = [ z_tail (Lz) | h (n-1) | 2 r_a(X) u(X) (n+1) | r_a^2 (3) | r_a (2) ]     prover.rs:118-123,340-357
//   sc_a = [ u (n) | 0 | r_a (2) ]                                                   prover.rs:330-338
// h = u2[n .. 2n-1)  (divide_by_vanishing_poly, prover.rs:105); also the degree checks.
// Row b: r_a at ra + b ra_stride, the [c] row after its z_tail at stride len_c, the [a] row (sc_a may be null: k_sc_a wrote it) at
// stride len_a, its own flag word.
template <class P>
__global__ void k_phase1_scalars(const Fp<P> *u, const Fp<P> *u2, const Fp<P> *ra /*r0,r1*/, uint64_t ra_stride, Fp<P> *sc_c_after_z,
                                 uint64_t len_c, Fp<P> *sc_a, uint64_t len_a, uint64_t n, unsigned *flags) {
    const uint64_t b = blockIdx.y;
    u += b * n; u2 += b * 2 * n; ra += b * ra_stride; sc_c_after_z += b * len_c; flags += b;
    if (sc_a) sc_a += b * len_a;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fp<P> r0 = ra[0], r1 = ra[1];
    if (i < n) {
        Fp<P> hi = u2[n + i];
        if (i < n - 1) {
            sc_c_after_z[i] = hi;
            // "h is not identically zero": nearly every lane sees it, and one atomic per wave on ONE word (the compiler already folds the lanes)
            // is 131 K serialised L2 operations -- 0.3 of this kernel's 0.39 ms.  A wave that reads the bit as set has nothing to add.
            if (!hi.is_zero() && !(*(const volatile unsigned *)flags & 4u)) atomicOr(flags, 4u);
        } else if (!hi.is_zero()) {
            atomicOr(flags, 2u);
        }
        if (sc_a) sc_a[i] = u[i];
    }
    if (i <= n) {  // coefficient i of 2 r_a(X) u(X) = 2 (r0 u_i + r1 u_{i-1})
        Fp<P> t = Fp<P>::zero();
        if (i < n) t = mul<P>(r0, u[i]);
        if (i > 0) t = add<P>(t, mul<P>(r1, u[i - 1]));
        sc_c_after_z[(n - 1) + i] = dbl<P>(t);
    }
    if (i == 0) {
        Fp<P> *tail = sc_c_after_z + (n - 1) + (n + 1);
        tail[0] = sqr<P>(r0);
        tail[1] = dbl<P>(mul<P>(r0, r1));
        tail[2] = sqr<P>(r1);
        tail[3] = r0;
        tail[4] = r1;
        if (sc_a) {
            sc_a[n] = Fp<P>::zero();
            sc_a[n + 1] = r0;
            sc_a[n + 2] = r1;
        }
    }
}

// sc_a alone, as soon as u is known: lets the [a]_1 MSM start while the rest of phase 1 still runs
template <class P>
__global__ void k_sc_a(const Fp<P> *u, const Fp<P> *ra, uint64_t ra_stride, Fp<P> *sc_a, uint64_t len_a, uint64_t n) {
    const uint64_t b = blockIdx.y;
    u += b * n; ra += b * ra_stride; sc_a += b * len_a;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sc_a[i] = u[i];
    if (i == 0) {
        sc_a[n] = Fp<P>::zero();
        sc_a[n + 1] = ra[0];
        sc_a[n + 2] = ra[1];
    }
}

// ------------------------------------------------------------------------ Horner (phase 2)
// u(x1) = sum_k u_k x1^k.  Lane t owns L consecutive coefficients: local Horner, times x1^(tL),
// workgroup LDS tree sum; one partial per workgroup, summed by the last tiny launch.
template <class P>
__device__ __forceinline__ void horner_partial(const Fp<P> *u, uint64_t n, const Fp<P> &x1, unsigned L, Fp<P> *partials) {
    __shared__ Fp<P> sh[256];
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > n) hi = n;
    Fp<P> acc = Fp<P>::zero();
    if (lo < n) {
        for (uint64_t k = hi; k-- > lo;) acc = add<P>(mul<P>(acc, x1), u[k]);
        acc = mul<P>(acc, pow_u64<P>(x1, lo));
    }
    const Fp<P> sum = block_sum<P, 256>(sh, acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
template <class P>
__global__ __launch_bounds__(256) void k_horner_partial(const Fp<P> *u, uint64_t n, Fp<P> x1, unsigned L, Fp<P> *partials) {
    horner_partial<P>(u, n, x1, L, partials);
}
template <class P>
__global__ __launch_bounds__(256) void k_horner_partial_rows(const Fp<P> *u, uint64_t n, const BatchRow<P> *rows, unsigned L, Fp<P> *partials) {
    const uint64_t b = blockIdx.y;
    horner_partial<P>(u + b * n, n, rows[b].x1, L, partials + b * gridDim.x);
}

// one workgroup per row: out[row] = sum of the row's `count` partials
template <class P>
__global__ __launch_bounds__(256) void k_sum_small(const Fp<P> *in, unsigned count, Fp<P> *out) {
    __shared__ Fp<P> sh[256];
    in += (uint64_t)blockIdx.x * count;
    Fp<P> acc = Fp<P>::zero();
    for (unsigned i = threadIdx.x; i < count; i += 256) acc = add<P>(acc, in[i]);
    const Fp<P> sum = block_sum<P, 256>(sh, acc);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// ------------------------------------------------------------- division (phase 3)
// numerator_at / numerator28_at / horner28_step: prove_common.cuh
//
// Synthetic division by (X - x1): H_k = N_k + x1 H_{k+1}, quotient q_{k-1} = H_k, remainder H_0.
// Level 0: lane t owns coefficients [tL, tL+L): V_t = local Horner value (carry-in 0).
// Then carry_t = V_t + x1^L carry_{t+1} is the same recurrence on V with multiplier x1^L: recurse.

// 6n of the 10n indices lie in the zero stretches between the blocks (numerator_at's table)
__device__ __forceinline__ bool zero_stretch(const NumParams &np, uint64_t lo, uint64_t hi) {
    const uint64_t s = np.sigma, n = np.n;
    return (lo >= 2 && hi <= 2 * s) || (lo >= 2 * s + 3 && hi <= 3 * s) || (lo >= 3 * s + n && hi <= 5 * s) || (lo >= 5 * s + n + 1 && hi <= 8 * s);
}

template <class P>
__device__ __forceinline__ void div_level0(const NumParams &np, const NumConsts<P> &nc, const NumMul28<typename Radix28<P>::RR> &m28, const Fp<P> *u,
                                           const Fp<P> *wit_u, const Fp<P> *u2, unsigned L, uint64_t nchunks, Fp<P> *V) {
    typedef typename Radix28<P>::RR RR;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > np.len) hi = np.len;
    if (zero_stretch(np, lo, hi)) { V[t] = Fp<P>::zero(); return; }   // a chunk inside a zero stretch has V = 0
    F28<RR> acc = f28_zero<RR>();
    for (uint64_t k = hi; k-- > lo;) acc = horner28_step<P, RR>(acc, k, np, nc, m28, u, wit_u, u2);
    Fp<P> out;
    f28_pack_canonical<RR>(f28_canonical_lazy<RR, 3>(acc), out.l);       // < 9p < 16p
    V[t] = out;
}
template <class P>
__global__ void k_div_level0(NumParams np, NumConsts<P> nc, NumMul28<typename Radix28<P>::RR> m28, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2,
                             unsigned L, uint64_t nchunks, Fp<P> *V) {
    div_level0<P>(np, nc, m28, u, wit_u, u2, L, nchunks, V);
}
template <class P>
__global__ void k_div_level0_rows(NumParams np, const BatchRow<P> *rows, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2, unsigned L,
                                  uint64_t nchunks, Fp<P> *V, uint64_t v_stride) {
    const uint64_t b = blockIdx.y;
    div_level0<P>(np, rows[b].nc, rows[b].m28, u + b * np.n, wit_u + b * np.n, u2 + b * 2 * np.n, L, nchunks, V + b * v_stride);
}

template <class P>
__device__ __forceinline__ void div_levelN(const Fp<P> *in, uint64_t count, const Fp<P> &xp, unsigned L, uint64_t nchunks, Fp<P> *V) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const Fp<P> x = xp;          // read behind the bounds test
    uint64_t lo = t * L, hi = lo + L;
    if (hi > count) hi = count;
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = hi; k-- > lo;) acc = add<P>(mul<P>(acc, x), in[k]);
    V[t] = acc;
}
template <class P>
__global__ void k_div_levelN(const Fp<P> *in, uint64_t count, Fp<P> xp, unsigned L, uint64_t nchunks, Fp<P> *V) {
    div_levelN<P>(in, count, xp, L, nchunks, V);
}
template <class P>
__global__ void k_div_levelN_rows(const Fp<P> *in, uint64_t in_stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned L,
                                  uint64_t nchunks, Fp<P> *V, uint64_t v_stride) {
    const uint64_t b = blockIdx.y;
    div_levelN<P>(in + b * in_stride, count, rows[b].xp[level], L, nchunks, V + b * v_stride);
}

// top level: one LANE per row, sequential over <= 64 values; out[k] = H_k (suffix value INCLUDING element k), out[count] = 0
template <class P>
__device__ __forceinline__ void div_top(const Fp<P> *in, uint64_t count, const Fp<P> &xp, Fp<P> *H) {
    Fp<P> acc = Fp<P>::zero();
    H[count] = acc;
    for (uint64_t k = count; k-- > 0;) {
        acc = add<P>(mul<P>(acc, xp), in[k]);
        H[k] = acc;
    }
}
template <class P>
__global__ void k_div_top(const Fp<P> *in, uint64_t stride, uint64_t count, Fp<P> xp, unsigned nrows, Fp<P> *H) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nrows) div_top<P>(in + b * stride, count, xp, H + b * stride);
}
template <class P>
__global__ void k_div_top_rows(const Fp<P> *in, uint64_t stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned nrows, Fp<P> *H) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nrows) div_top<P>(in + b * stride, count, rows[b].xp[level], H + b * stride);
}

// Expand one level down: given Hup[t] = true suffix value at the START of chunk t (and Hup[nchunks] = 0),
// recompute chunk t of `in` with carry-in Hup[t+1] and write H[k] for every k in the chunk.
template <class P>
__device__ __forceinline__ void div_expandN(const Fp<P> *in, uint64_t count, const Fp<P> &xp, unsigned L, uint64_t nchunks, const Fp<P> *Hup,
                                            Fp<P> *H) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const Fp<P> x = xp;          // read behind the bounds test
    uint64_t lo = t * L, hi = lo + L;
    if (hi > count) hi = count;
    Fp<P> acc = Hup[t + 1];
    for (uint64_t k = hi; k-- > lo;) {
        acc = add<P>(mul<P>(acc, x), in[k]);
        H[k] = acc;
    }
    if (t == nchunks - 1) H[count] = Fp<P>::zero();
}
template <class P>
__global__ void k_div_expandN(const Fp<P> *in, uint64_t count, Fp<P> xp, unsigned L, uint64_t nchunks, const Fp<P> *Hup, Fp<P> *H) {
    div_expandN<P>(in, count, xp, L, nchunks, Hup, H);
}
template <class P>
__global__ void k_div_expandN_rows(const Fp<P> *in, uint64_t stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned L,
                                   uint64_t nchunks, const Fp<P> *Hup, uint64_t hup_stride, Fp<P> *H) {
    const uint64_t b = blockIdx.y;
    div_expandN<P>(in + b * stride, count, rows[b].xp[level], L, nchunks, Hup + b * hup_stride, H + b * stride);
}

// Level 0 expansion writes the quotient: q_{k-1} = H_k for k >= 1; H_0 is the remainder.  Hup == nullptr: carry-in 0 (the one-lane
// division of a numerator of <= 64 coefficients).
template <class P>
__device__ __forceinline__ void div_expand0(const NumParams &np, const NumConsts<P> &nc, const NumMul28<typename Radix28<P>::RR> &m28, const Fp<P> *u,
                                            const Fp<P> *wit_u, const Fp<P> *u2, unsigned L, uint64_t nchunks, const Fp<P> *Hup, Fp<P> *q,
                                            unsigned *flags) {
    typedef typename Radix28<P>::RR RR;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > np.len) hi = np.len;
    F28<RR> acc = Hup ? f28_unpack<RR>(Hup[t + 1].l) : f28_zero<RR>();
    if (zero_stretch(np, lo, hi)) {   // the quotient is a geometric tail: one product per coefficient, no table walk
        for (uint64_t k = hi; k-- > lo;) {
            acc = f28_mul<RR>(acc, m28.x1);                     // < 2p, tight: one conditional subtraction on the way out
            Fp<P> out;
            f28_pack_reduced<RR>(acc, out.l);
            q[k - 1] = out;        // lo >= 2 here
        }
        return;
    }
    for (uint64_t k = hi; k-- > lo;) {
        acc = f28_canonical_lazy<RR, 3>(horner28_step<P, RR>(acc, k, np, nc, m28, u, wit_u, u2));   // the stored element: canonical
        Fp<P> out;
        f28_pack_canonical<RR>(acc, out.l);
        if (k > 0) q[k - 1] = out;
        else if (!out.is_zero()) atomicOr(flags, 8u);  // rem != 0, prover.rs:221
    }
}
template <class P>
__global__ void k_div_expand0(NumParams np, NumConsts<P> nc, NumMul28<typename Radix28<P>::RR> m28, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2,
                              unsigned L, uint64_t nchunks, const Fp<P> *Hup, Fp<P> *q, unsigned *flags) {
    div_expand0<P>(np, nc, m28, u, wit_u, u2, L, nchunks, Hup, q, flags);
}
template <class P>
__global__ void k_div_expand0_rows(NumParams np, const BatchRow<P> *rows, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2, unsigned L,
                                   uint64_t nchunks, const Fp<P> *Hup, uint64_t hup_stride, Fp<P> *q, uint64_t q_stride, unsigned *flags) {
    const uint64_t b = blockIdx.y;
    div_expand0<P>(np, rows[b].nc, rows[b].m28, u + b * np.n, wit_u + b * np.n, u2 + b * 2 * np.n, L, nchunks,
                   Hup ? Hup + b * hup_stride : nullptr, q + b * q_stride, flags + b);
}

}  // namespace pm
