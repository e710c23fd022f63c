// Device side of the circuit-specific setup: the reference builds every
// ProvingKey vector by a serial `g * f(j)` loop with a fresh x.pow([j]) per element
// (/root/reference/src/generator.rs:169-177).  Here: scalar vectors scale * x^j by a chunked power
// kernel, then a batched fixed-base multiplication of the G1 generator with an 8-bit windowed table
// (32 mixed adds per point) and a per-lane Montgomery batch inversion back to affine -- the layout
// the MSM kernels gather from.
#include <cstdlib>
#include <cstring>

#include "internal.h"
#include <algorithm>
#include "fq28.cuh"
#include "prove_common.cuh"

namespace pm {

template <class P>
__global__ void k_powers(Fp<P> *out, size_t count, Fp<P> scale, Fp<P> x, unsigned L) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t lo = t * L, hi = lo + L;
    if (lo >= count) return;
    if (hi > count) hi = count;
    Fp<P> acc = mul<P>(scale, pow_u64<P>(x, lo));
    for (size_t j = lo; j < hi; ++j) {
        out[j] = acc;
        acc = mul<P>(acc, x);
    }
}

template <class C>
int powers_fill(pm_ctx *ctx, Fp<typename C::FrP> *d_out, size_t count, const Fp<typename C::FrP> &scale,
                const Fp<typename C::FrP> &x) {
    typedef typename C::FrP P;
    if (!count) return PM_OK;
    const unsigned L = 64;
    size_t lanes = (count + L - 1) / L;
    PM_LAUNCH(ctx, k_powers<P>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_out, count, scale, x, L);
    return PM_OK;
}

// table[w * 255 + (d - 1)] = d * 2^(8w) * G, affine
constexpr int FB_WINDOWS = 32;
constexpr int FB_BATCH = 8;

template <class C>
__global__ __launch_bounds__(128) void k_fixed_base(const Fp<typename C::FrP> *scalars, size_t len,
                                                    const Affine<C> *table, Affine<C> *out) {
    typedef typename C::FqP Q;
    typedef Fp<Q> Fq;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t lo = t * FB_BATCH;
    if (lo >= len) return;
    size_t cnt = len - lo < (size_t)FB_BATCH ? len - lo : (size_t)FB_BATCH;
    // Montgomery batch inversion of the ZZZ coordinates across this lane's FB_BATCH points:
    // pass 1 computes the points and prefix products (kept in `out` as scratch: X,Y of the XYZZ
    // result are parked in the output slot, ZZ/ZZZ and the prefix in registers is too much for
    // 8 points, so recompute-free two-pass with small local arrays).
    Fq zz[FB_BATCH], zzz[FB_BATCH], pre[FB_BATCH];
    Fq run = Fq::one();
    for (size_t i = 0; i < cnt; ++i) {
        Fp<typename C::FrP> k = from_mont<typename C::FrP>(scalars[lo + i]);
        XYZZ<C> acc = XYZZ<C>::identity();
        for (int w = 0; w < FB_WINDOWS; ++w) {
            unsigned d = (k.l[w >> 2] >> (8 * (w & 3))) & 0xffu;
            if (d) xyzz_madd<C>(acc, table[w * 255 + (d - 1)], false);
        }
        out[lo + i].x = acc.X;
        out[lo + i].y = acc.Y;
        zz[i] = acc.ZZ;
        zzz[i] = acc.ZZZ;
        pre[i] = run;
        if (!acc.ZZZ.is_zero()) run = mul<Q>(run, acc.ZZZ);
    }
    Fq inv = inverse<Q>(run);
    for (size_t ii = cnt; ii-- > 0;) {
        if (zzz[ii].is_zero()) {
            out[lo + ii] = Affine<C>::infinity();
            continue;
        }
        Fq i3 = mul<Q>(inv, pre[ii]);      // 1 / ZZZ_i
        inv = mul<Q>(inv, zzz[ii]);
        Fq i2 = sqr<Q>(mul<Q>(i3, zz[ii]));  // 1 / ZZ_i
        Affine<C> a;
        a.x = mul<Q>(out[lo + ii].x, i2);
        a.y = mul<Q>(out[lo + ii].y, i3);
        out[lo + ii] = a;
    }
}

template <class C>
static int fixed_base_table(pm_ctx *ctx, const Affine<C> **d_table) {
    typedef typename C::FqP Q;
    typedef Fp<Q> Fq;
    DevBuf &buf = ctx->fb_table[C::ID];   // owned by the context: no process-wide state, freed with it
    if (!buf.p) {
        const int NT = FB_WINDOWS * 255;
        std::vector<XYZZ<C>> pts(NT);
        Affine<C> g;
        for (int i = 0; i < Q::N; ++i) { g.x.l[i] = C::GX_MONT[i]; g.y.l[i] = C::GY_MONT[i]; }
        XYZZ<C> base = XYZZ<C>::from_affine(g);
        for (int w = 0; w < FB_WINDOWS; ++w) {
            XYZZ<C> acc = XYZZ<C>::identity();
            for (int d = 0; d < 255; ++d) {
                acc = xyzz_add<C>(acc, base);
                pts[w * 255 + d] = acc;
            }
            for (int k = 0; k < 8; ++k) base = xyzz_dbl<C>(base);
        }
        // host batch inversion of ZZZ
        std::vector<Fq> pre(NT);
        Fq run = Fq::one();
        for (int i = 0; i < NT; ++i) { pre[i] = run; run = mul<Q>(run, pts[i].ZZZ); }
        Fq inv = inverse<Q>(run);
        std::vector<Affine<C>> aff(NT);
        for (int i = NT; i-- > 0;) {
            Fq i3 = mul<Q>(inv, pre[i]);
            inv = mul<Q>(inv, pts[i].ZZZ);
            Fq i2 = sqr<Q>(mul<Q>(i3, pts[i].ZZ));
            aff[i].x = mul<Q>(pts[i].X, i2);
            aff[i].y = mul<Q>(pts[i].Y, i3);
        }
        PM_HIP(ctx, buf.reserve(NT * sizeof(Affine<C>)));
        hipError_t he = hipMemcpy(buf.p, aff.data(), NT * sizeof(Affine<C>), hipMemcpyHostToDevice);
        if (he != hipSuccess) {
            buf.release();
            PM_HIP(ctx, he);
        }
    }
    *d_table = buf.as<Affine<C>>();
    return PM_OK;
}

template <class C>
int fixed_base_batch(pm_ctx *ctx, const Fp<typename C::FrP> *d_scalars, size_t len, Affine<C> *d_out) {
    if (!len) return PM_OK;
    const Affine<C> *table = nullptr;
    PM_TRY(fixed_base_table<C>(ctx, &table));
    size_t lanes = (len + FB_BATCH - 1) / FB_BATCH;
    PM_LAUNCH(ctx, k_fixed_base<C>, dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, ctx->stream, d_scalars, len,
                   table, d_out);
    return PM_OK;
}

template <class P>
__global__ void k_iota_mont(Fp<P> *out, size_t len, uint64_t first) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    uint64_t v = first + i;
    Fp<P> r = Fp<P>::zero();
    r.l[0] = (uint32_t)v;
    r.l[1] = (uint32_t)(v >> 32);
    out[i] = to_mont<P>(r);
}

// P_i = (i+1) * G   (SURVEY.md §8d MSM micro-inputs)
template <class C>
int bases_generate_multiples(pm_ctx *ctx, size_t len, Affine<C> *d_out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const size_t CH = (size_t)1 << 22;
    PM_HIP(ctx, ctx->scratch.reserve((len < CH ? len : CH) * sizeof(Fr)));
    for (size_t s = 0; s < len; s += CH) {
        size_t cnt = len - s < CH ? len - s : CH;
        PM_LAUNCH(ctx, k_iota_mont<P>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->scratch.as<Fr>(), cnt, (uint64_t)(s + 1));
        PM_TRY(fixed_base_batch<C>(ctx, ctx->scratch.as<Fr>(), cnt, d_out + s));
        PM_TRY(bases_convert<C>(ctx, d_out + s, cnt, true));
    }
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

template <class C>
__global__ void k_bases_convert(Affine<C> *pts, size_t len, int to_internal) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    Affine<C> a = pts[i];
    if (to_internal) {
        a.x = fq_std_to_int<C>(a.x);
        a.y = fq_std_to_int<C>(a.y);
    } else {
        a.x = fq_int_to_std<C>(a.x);
        a.y = fq_int_to_std<C>(a.y);
    }
    pts[i] = a;
}

template <class C>
int bases_convert(pm_ctx *ctx, Affine<C> *d_points, size_t len, bool to_internal) {
    if (!len) return PM_OK;
    PM_LAUNCH(ctx, k_bases_convert<C>, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, d_points, len,
                   to_internal ? 1 : 0);
    return PM_OK;
}

// ------------------------------------------------------------------------------ window tables
// Window 0 = the resident (internal-form, dense) points re-limbed into 128-byte TablePoint records;
// T_w[i] = 2^(width of window w-1) T_{w-1}[i]: doublings on F28 registers, then back to affine with a
// per-lane Montgomery batch inversion over TB_BATCH points (all in the internal radix).
constexpr int TB_BATCH = 8;

template <class C>
__global__ void k_table_window0(const Affine<C> *src, TablePoint<C> *dst, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = table_point_from_affine<C>(src[i]);   // infinity (all-zero) stays all-zero
}

// M = 5 (radix 5 2^c, radix.cuh): T_w = 5 2^c T_{w-1} -- c doublings to A, then 5 A = 2 (2 A) + A.  4 A = +-A only for the identity
// (odd group order), the addition goes through the exceptional-safe form all the same.
template <class C, unsigned M>
__global__ __launch_bounds__(128) void k_table_next(const TablePoint<C> *prev, TablePoint<C> *next, size_t count, unsigned c) {
    typedef typename C::FqRR RR;
    typedef F28<RR> F;
    constexpr int N = RR::N;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t lo = t * TB_BATCH;
    if (lo >= count) return;
    size_t cnt = count - lo < (size_t)TB_BATCH ? count - lo : (size_t)TB_BATCH;
    F zz[TB_BATCH], zzz[TB_BATCH], pre[TB_BATCH];
    bool live[TB_BATCH];
    F run = f28_one<RR>();
    for (size_t i = 0; i < cnt; ++i) {
        const TablePoint<C> p = prev[lo + i];
        uint32_t any = 0;
        XYZZ28<C> a;
        for (int k = 0; k < N; ++k) { a.X.l[k] = p.x[k]; a.Y.l[k] = p.y[k]; any |= p.x[k] | p.y[k]; }
        live[i] = any != 0;
        pre[i] = run;
        if (!live[i]) continue;
        a.ZZ = f28_one<RR>();
        a.ZZZ = f28_one<RR>();
        for (unsigned k = 0; k < c; ++k) xyzz28_dbl<C>(a);
        if constexpr (M == 5) {
            const XYZZ28<C> one = a;
            xyzz28_dbl<C>(a);
            xyzz28_dbl<C>(a);
            xyzz28_add_full<C>(a, one);
        }
        TablePoint<C> park;                          // X, Y (tight limbs) parked until the inverses are known
        for (int k = 0; k < N; ++k) { park.x[k] = a.X.l[k]; park.y[k] = a.Y.l[k]; }
        next[lo + i] = park;
        zz[i] = a.ZZ;
        zzz[i] = a.ZZZ;
        run = f28_mul<RR>(run, a.ZZZ);
    }
    F inv = f28_inverse<RR>(run);
    for (size_t ii = cnt; ii-- > 0;) {
        TablePoint<C> out;
        if (!live[ii]) {
            for (int k = 0; k < N; ++k) out.x[k] = out.y[k] = 0;
            next[lo + ii] = out;
            continue;
        }
        F i3 = f28_mul<RR>(inv, pre[ii]);           // 1 / ZZZ
        inv = f28_mul<RR>(inv, zzz[ii]);
        F i2 = f28_sqr<RR>(f28_mul<RR>(i3, zz[ii]));  // 1 / ZZ
        const TablePoint<C> park = next[lo + ii];
        F X, Y;
        for (int k = 0; k < N; ++k) { X.l[k] = park.x[k]; Y.l[k] = park.y[k]; }
        X = f28_canonical<RR>(f28_mul<RR>(X, i2));
        Y = f28_canonical<RR>(f28_mul<RR>(Y, i3));
        for (int k = 0; k < N; ++k) { out.x[k] = X.l[k]; out.y[k] = Y.l[k]; }
        next[lo + ii] = out;
    }
}

template <class C>
int tables_build(pm_ctx *ctx, const Affine<C> *d_points, TablePoint<C> *d_table, size_t count, const MsmTables &t) {
    if (!t.planned() || !count) return PM_OK;
    PM_LAUNCH(ctx, k_table_window0<C>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, d_points, d_table, count);
    size_t lanes = (count + TB_BATCH - 1) / TB_BATCH;
    if (t.m != 1 && t.m != 5) return PM_ERR_INVALID_ARG;
    for (unsigned w = 1; w < t.nwin; ++w) {   // T_w = 2^(win_width of window w-1) * T_{w-1}; radix 5 2^a: T_w = 5 2^a T_{w-1}
        const TablePoint<C> *prev = d_table + (size_t)(w - 1) * t.stride;
        TablePoint<C> *next = d_table + (size_t)w * t.stride;
        if (t.m == 5) PM_LAUNCH(ctx, (k_table_next<C, 5>), dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, ctx->stream, prev, next, count, t.a);
        else PM_LAUNCH(ctx, (k_table_next<C, 1>), dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, ctx->stream, prev, next, count, win_width(t.nwin, w - 1));
    }
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

template <class C>
__global__ void k_inf_flags(const Affine<C> *pts, size_t count, unsigned char *flags) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t *w = (const uint32_t *)&pts[i];
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 2 * C::FqP::N; ++t) any |= w[t];
    flags[i] = any ? 0 : 1;
}

template <class C>
int infinity_flags(pm_ctx *ctx, const Affine<C> *d_points, size_t count, unsigned char *d_flags) {
    if (!count) return PM_OK;
    PM_LAUNCH(ctx, k_inf_flags<C>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, d_points, count, d_flags);
    return PM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The uj_wj_lcs scalars on the device (generator.rs:112-136; round 4, VERDICT r3 item 7 -- until round 3 the Lagrange coefficients
// and the sparse pass below ran on <= 32 host threads: ~10 s at 2^24 gates, per rank).
//
//   L_i      = zh / n * w^i / (x - w^i),  i < n                                        (generator.rs:113)
//   ucol[c]  = sum_r A[r, c] (L_{2m0+r} + L_{2m0+nr+r}) + B[r, c] (L_{2m0+r} - L_{2m0+nr+r})
//   wcol[c]  = sum_r C[r, c] 4 L_{2m0+r}   (c < m0 + mw);  + 4 L_c for c < m0;
//   wcol[m0 + mw + i] = L_i + L_{m0+i} (i < m0);   wcol[m0 + mw + m0 + r] = L_{2m0+r} + L_{2m0+nr+r}
//   lcs[j]   = (ucol[j] y^gamma + wcol[j]) y^(-alpha)                                   (generator.rs:134)
//
// The two sums run over the ROWS of the CSR matrices the prover already holds in HBM; a column's terms come from many rows, so
// they are accumulated with atomics -- exactly: every product (a canonical residue) is split into eight 32-bit words and each word
// is added to its own 64-bit counter (2^32 terms of 32 bits fit), the counters are carried and reduced once per column
// (k_lcs_finish).  Integer sums commute, so the result does not depend on the order the rows arrive in: bit-identical to the host
// pass it replaces (the parity tests compare the bases with the committed fixtures and with the CPU restatement).
template <class P>
__global__ void k_lagrange(Fp<P> *L, Fp<P> *pre, size_t n, Fp<P> x, Fp<P> omega, Fp<P> kscale, unsigned CH) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lo = t * CH;
    if (lo >= n) return;
    const size_t hi = lo + CH < n ? lo + CH : n;
    Fp<P> wi = pow_u64<P>(omega, lo), run = Fp<P>::one();
    for (size_t i = lo; i < hi; ++i) {       // L holds w^i, pre the running product of the denominators before i
        L[i] = wi;
        pre[i] = run;
        run = mul<P>(run, sub<P>(x, wi));
        wi = mul<P>(wi, omega);
    }
    Fp<P> inv = inverse<P>(run);             // x^n != 1 (api.hip: pk_generate_impl returns PM_ERR_INVALID_ARG otherwise): no denominator is zero
    for (size_t i = hi; i-- > lo;) {
        const Fp<P> w = L[i];
        const Fp<P> di = mul<P>(inv, pre[i]);
        inv = mul<P>(inv, sub<P>(x, w));
        L[i] = mul<P>(mul<P>(w, di), kscale);
    }
}

template <class P>
__device__ __forceinline__ void lcs_accumulate(unsigned long long *acc, uint32_t col, const Fp<P> &v) {
#pragma unroll
    for (int q = 0; q < 8; ++q) atomicAdd(&acc[(size_t)col * 8 + q], (unsigned long long)v.l[q]);
}

template <class P>
__global__ void k_lcs_rows(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *L, uint64_t m0, uint64_t nr, unsigned long long *uacc,
                           unsigned long long *wacc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const Fp<P> L1 = L[2 * m0 + r], L2 = L[2 * m0 + nr + r];
    const Fp<P> sp = add<P>(L1, L2), sm = sub<P>(L1, L2), L1x4 = dbl<P>(dbl<P>(L1));
    for (uint64_t k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) lcs_accumulate<P>(uacc, A.col[k], mul<P>(*(const Fp<P> *)(A.val + 4 * k), sp));
    for (uint64_t k = B.rowptr[r]; k < B.rowptr[r + 1]; ++k) lcs_accumulate<P>(uacc, B.col[k], mul<P>(*(const Fp<P> *)(B.val + 4 * k), sm));
    for (uint64_t k = Cm.rowptr[r]; k < Cm.rowptr[r + 1]; ++k) lcs_accumulate<P>(wacc, Cm.col[k], mul<P>(*(const Fp<P> *)(Cm.val + 4 * k), L1x4));
}

// sum of < 2^32 canonical residues held as eight 64-bit word counters -> the residue of the sum
template <class P>
__device__ __forceinline__ Fp<P> lcs_reduce(const unsigned long long *acc) {
    Fp<P> lo;
    unsigned long long c = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const unsigned long long a = acc[q];
        c += a & 0xffffffffull;
        lo.l[q] = (uint32_t)c;
        c = (c >> 32) + (a >> 32);
    }
    // value = lo + c 2^256, c < 2^33: lo is below 2^256 < 6 MOD (BN254's scalar field is 0.19 x 2^256, BLS12-381's 0.45 x 2^256)
    Fp<P> t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        reduce_once<P>(t.l, lo.l, 0);
        reduce_once<P>(lo.l, t.l, 0);
    }
    Fp<P> hi = Fp<P>::zero();
    hi.l[0] = (uint32_t)c;
    hi.l[1] = (uint32_t)(c >> 32);
    return add<P>(lo, mul<P>(hi, Fp<P>::r2()));      // Montgomery product with 2^512: c 2^256 mod MOD as a plain residue
}

template <class P>
__global__ void k_lcs_finish(const unsigned long long *uacc, const unsigned long long *wacc, const Fp<P> *L, uint64_t m0, uint64_t mw,
                             uint64_t nr, Fp<P> y_gamma, Fp<P> y_to_minus_alpha, Fp<P> *lcs) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, mcols = m0 + mw, Lz = 2 * m0 + mw + nr;
    if (j >= Lz) return;
    Fp<P> u = Fp<P>::zero(), w;
    if (j < mcols) {
        u = lcs_reduce<P>(uacc + j * 8);
        w = lcs_reduce<P>(wacc + j * 8);
        if (j < m0) w = add<P>(w, dbl<P>(dbl<P>(L[j])));
    } else if (j < mcols + m0) {
        const uint64_t i = j - mcols;
        w = add<P>(L[i], L[i + m0]);
    } else {
        const uint64_t r = j - mcols - m0;
        w = add<P>(L[2 * m0 + r], L[2 * m0 + nr + r]);
    }
    lcs[j] = mul<P>(add<P>(mul<P>(u, y_gamma), w), y_to_minus_alpha);
}

// d_lcs: Lz = 2 m0 + mw + nr scalars.  rowptr / col / val of A, B, C as the prover holds them (first-entry semantics applied).
template <class C>
int lcs_scalars(pm_ctx *ctx, const pm_pk *pk, const Fp<typename C::FrP> &x, const Fp<typename C::FrP> &omega, const Fp<typename C::FrP> &kscale,
                const Fp<typename C::FrP> &y_gamma, const Fp<typename C::FrP> &y_to_minus_alpha, DevBuf &lagrange, DevBuf &work,
                Fp<typename C::FrP> *d_lcs) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const uint64_t n = pk->n, m0 = pk->m0, mw = pk->mw, nr = pk->nr, mcols = m0 + mw, Lz = 2 * m0 + mw + nr;
    const size_t acc_bytes = (size_t)mcols * 8 * sizeof(unsigned long long);
    PM_HIP(ctx, lagrange.reserve(n * sizeof(Fr)));
    PM_HIP(ctx, work.reserve(std::max((size_t)n * sizeof(Fr), 2 * acc_bytes)));
    Fr *L = lagrange.as<Fr>();
    const unsigned CH = 64;
    PM_LAUNCH(ctx, k_lagrange<P>, dim3(nblk((n + CH - 1) / CH)), dim3(256), 0, ctx->stream, L, work.as<Fr>(), (size_t)n, x, omega, kscale, CH);
    unsigned long long *uacc = work.as<unsigned long long>(), *wacc = uacc + (size_t)mcols * 8;
    PM_HIP(ctx, hipMemsetAsync(uacc, 0, 2 * acc_bytes, ctx->stream));       // `pre` is dead: the stream orders the two uses
    if (nr) {
        const CsrDev A{pk->d_rowptr[0], pk->d_col[0], pk->d_val[0]}, B{pk->d_rowptr[1], pk->d_col[1], pk->d_val[1]},
            Cm{pk->d_rowptr[2], pk->d_col[2], pk->d_val[2]};
        PM_LAUNCH(ctx, k_lcs_rows<P>, dim3(nblk(nr)), dim3(256), 0, ctx->stream, A, B, Cm, (const Fr *)L, m0, nr, uacc, wacc);
    }
    PM_LAUNCH(ctx, k_lcs_finish<P>, dim3(nblk(Lz)), dim3(256), 0, ctx->stream, (const unsigned long long *)uacc, (const unsigned long long *)wacc,
                   (const Fr *)L, m0, mw, nr, y_gamma, y_to_minus_alpha, d_lcs);
    return PM_OK;
}

#define PM_INST(C)                                                                                              \
    template int lcs_scalars<C>(pm_ctx *, const pm_pk *, const Fp<typename C::FrP> &, const Fp<typename C::FrP> &,                    \
                                const Fp<typename C::FrP> &, const Fp<typename C::FrP> &, const Fp<typename C::FrP> &, DevBuf &,     \
                                DevBuf &, Fp<typename C::FrP> *);                                                                    \
    template int powers_fill<C>(pm_ctx *, Fp<typename C::FrP> *, size_t, const Fp<typename C::FrP> &,           \
                                const Fp<typename C::FrP> &);                                                   \
    template int fixed_base_batch<C>(pm_ctx *, const Fp<typename C::FrP> *, size_t, Affine<C> *);               \
    template int bases_generate_multiples<C>(pm_ctx *, size_t, Affine<C> *);                                    \
    template int bases_convert<C>(pm_ctx *, Affine<C> *, size_t, bool);                                          \
    template int tables_build<C>(pm_ctx *, const Affine<C> *, TablePoint<C> *, size_t, const MsmTables &);                             \
    template int infinity_flags<C>(pm_ctx *, const Affine<C> *, size_t, unsigned char *);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
