// Pairing product checks on the device, one check per group of WAVE_GROUP lanes of one wave (pm_verify_batch2 with
// PM_VERIFY_PAIRING_DEVICE_WAVE; DESIGN.md "Batch verification").  The same line tables and Consts as pairing_batch.hip
// (pairing_prepare), the same algorithm as Tower<C>::product_is_one; pairing_wave.cuh says which lane does what.
//
//   host  : fixed_base_prepare -- the table d 2^(4 t) G of this call's G, beside the line tables
//   device: k_pairing_check_wave -- one wave a workgroup, WAVE_CHECKS checks a wave.  The operands of a product are an image in LDS
//           (six Fq2 a value, read by all lanes of the group), the 36 products go through LDS to the six collecting lanes; the
//           accumulator of the Miller loop and of the x-chains is the image itself, nothing of the loops lives in scratch.  The barrier
//           is the wave's own.  Every barrier and the ballot sit outside data-dependent branches: a group without a check, a leaf that
//           is not live and a pair at infinity all run along (on the last check's data, on the line 1) and only the store is masked.
// The kernel takes k_pairing_check's arguments, dense points included, but only the batch verifier launches it (tree nodes): no entry
// point carries a choice of kernel to pm_pairing_check_batch, so the dense-points form has not run yet.
#include <cstring>
#include <new>

#include "internal.h"
#include "pairing_wave.cuh"
#include "verify_batch.cuh"

namespace pm {

template <class C>
struct alignas(16) WaveLds {
    typename WaveTower<C>::Image a, b;                          // the operands; a round leaves its result in a
    typename Tower<C>::Fq2 prod[WAVE_GROUP];
    XYZZ<C> pts[WAVE_FB_LANES + 1];                             // the prelude's sum tree, U behind it
    Affine<C> P[PAIRING_MAX_PAIRS];
};

// a <- a b (b may be a itself, or the three slots of a line).  a and b are published and the group has met; it has met again on return.
template <class C>
__device__ __noinline__ void wave_round(WaveLds<C> *s, int l, const typename WaveTower<C>::Image *b, bool line) {
    typedef WaveTower<C> W;
    if (l < W::products(line)) s->prod[l] = W::product(l, s->a, *b, line);
    __syncthreads();
    if (l < 6) s->a.c[l] = W::collect(l, s->prod, line);
    __syncthreads();
}
// b <- the line L at P[j], then a <- a b
template <class C>
__device__ __noinline__ void wave_line(WaveLds<C> *s, int l, const typename Tower<C>::Line *L, int j) {
    typedef WaveTower<C> W;
    if (l < 3) s->b.c[l] = W::line_coeff(l, *L, s->P[j]);
    __syncthreads();
    wave_round<C>(s, l, &s->b, true);
}
// a <- a^p: every lane on its own coefficient
template <class C>
__device__ __noinline__ void wave_frob(WaveLds<C> *s, int l, const typename Tower<C>::Consts *K) {
    typedef WaveTower<C> W;
    if (l < 6) s->a.c[l] = W::frob_coeff(l, s->a.c[l], *K);
}

// The group's view of the tower: values are one Fq2 a lane (lane l < 6 holds coefficient l, the others zero).
template <class C>
struct WaveGroup {
    typedef WaveTower<C> W;
    typedef Tower<C> T;
    typedef PairingParams<C> PP;
    typedef typename T::Fq2 V;
    WaveLds<C> *s;
    int l;                                                      // lane of the group; >= WAVE_GROUP: a lane without a group
    const typename T::Consts *K;

    __device__ V cur() const { return l < 6 ? s->a.c[l] : T::zero2(); }
    __device__ void put_a(const V &x) const { if (l < 6) s->a.c[l] = x; }
    __device__ void put_b(const V &x) const { if (l < 6) s->b.c[l] = x; }
    __device__ V conj(const V &x) const { return l < 6 ? W::conj_coeff(l, x) : x; }
    __device__ V mul(const V &x, const V &y) const {
        put_a(x); put_b(y);
        __syncthreads();
        wave_round<C>(s, l, &s->b, false);
        return cur();
    }
    __device__ V sqr(const V &x) const {
        put_a(x);
        __syncthreads();
        wave_round<C>(s, l, &s->a, false);
        return cur();
    }
    __device__ V frob(const V &x) const {
        put_a(x);
        wave_frob<C>(s, l, K);
        return cur();
    }
    // T::pow_x: the accumulator is the image a, g stays in b
    __device__ V pow_x(const V &g) const {
        put_a(g); put_b(g);
        __syncthreads();
#pragma unroll 1
        for (int b = 62; b >= 0; --b) {
            if (b == 62 && !(PP::X_ABS >> 63)) continue;
            wave_round<C>(s, l, &s->a, false);
            if ((PP::X_ABS >> b) & 1) wave_round<C>(s, l, &s->b, false);
        }
        return PP::X_NEGATIVE ? conj(cur()) : cur();
    }
    __device__ V pow_small(const V &g, unsigned e) const {      // T::pow_small, 1 <= e < 64
        int top = 5;
        while (!((e >> top) & 1u)) --top;
        put_a(g); put_b(g);
        __syncthreads();
#pragma unroll 1
        for (int b = top - 1; b >= 0; --b) {
            wave_round<C>(s, l, &s->a, false);
            if ((e >> b) & 1u) wave_round<C>(s, l, &s->b, false);
        }
        return cur();
    }
    // T::miller over the points s->P; leaves f in the image a
    __device__ void miller(const typename T::Line *tab, int k, unsigned pairs) const {
        if (l < 6) s->a.c[l] = W::one_coeff(l);
        __syncthreads();
        int idx = 0;
#pragma unroll 1
        for (int i = PP::LOOP_TOP - 1; i >= -1; --i) {
            if (i < 0 && !PP::FROBENIUS_STEPS) break;
            if (i >= 0) wave_round<C>(s, l, &s->a, false);
            const int steps = i < 0 || T::loop_bit(i) ? 2 : 1;
#pragma unroll 1
            for (int st = 0; st < steps; ++st, ++idx) {
#pragma unroll 1
                for (int j = 0; j < k; ++j)
                    if ((pairs >> j) & 1u) wave_line<C>(s, l, tab + j * PP::LINES + idx, j);   // k, pairs: the launch's, uniform
            }
        }
    }
    // T::final_exp of the image a; the one inversion on the group's first lane
    __device__ V final_exp() const {
        const V f0 = cur();
        if (l == 0) W::store_tower(T::inv12(W::to_tower(s->a)), s->b);
        __syncthreads();                                        // lane 0 has read all six coefficients
        put_a(conj(f0));
        __syncthreads();
        wave_round<C>(s, l, &s->b, false);                      // ^(p^6 - 1)
        V f = cur();
        f = mul(frob(frob(f)), f);                              // ^(p^2 + 1)
        if (PP::FROBENIUS_STEPS) {                              // BN254
            const V fx = pow_x(f), fx2 = pow_x(fx), fx3 = pow_x(fx2);
            const V c36 = pow_small(fx3, 36);
            const V l0 = conj(mul(mul(c36, pow_small(fx2, 30)), mul(pow_small(fx, 18), sqr(f))));
            const V l1 = mul(conj(mul(mul(c36, pow_small(fx2, 18)), pow_small(fx, 12))), f);
            const V l2 = mul(pow_small(fx2, 6), f);
            V r = frob(f);
            r = frob(mul(r, l2));
            r = frob(mul(r, l1));
            return mul(r, l0);
        }
        V a = mul(pow_x(f), conj(f));                           // BLS12-381
        a = mul(pow_x(a), conj(a));
        const V b = mul(pow_x(a), frob(a));
        const V c = mul(mul(pow_x(pow_x(b)), frob(frob(b))), conj(b));
        return mul(c, mul(sqr(f), f));
    }
};

template <class C>
__global__ __launch_bounds__(64) void k_pairing_check_wave(const typename Tower<C>::Line *tab, const typename Tower<C>::Consts *consts, int k, unsigned pairs,
                                                           const Affine<C> *pts, const VerifyTerm<C> *terms, const uint32_t *neg_g, const uint8_t *live,
                                                           const XYZZ<C> *fixed_base, size_t count, uint8_t *is_one) {
    typedef WaveTower<C> W;
    __shared__ WaveLds<C> lds[WAVE_CHECKS];
    const int g = threadIdx.x / WAVE_GROUP;
    const bool grouped = g < WAVE_CHECKS;
    const int l = grouped ? (int)threadIdx.x % WAVE_GROUP : WAVE_GROUP;
    WaveLds<C> *s = &lds[grouped ? g : 0];
    const size_t i = (size_t)blockIdx.x * WAVE_CHECKS + (grouped ? g : 0);
    const size_t src = i < count ? i : count - 1;               // a group without a check runs along on the last one's data

    if (terms) {                                                // k == 3: e(U - g G, [z]_2) e(-V, [x]_2) e(W, [1]_2)
        if (l < WAVE_FB_LANES) s->pts[l] = W::fixed_base_lane(l, fixed_base, neg_g + 8 * src);
        if (l == WAVE_FB_LANES) s->pts[l] = terms[src].U;
        __syncthreads();
#pragma unroll 1
        for (int stride = WAVE_FB_LANES / 2; stride >= 1; stride >>= 1) {
            if (l < stride) W::fixed_base_tree_step(l, stride, s->pts);
            __syncthreads();
        }
        if (l == 1) s->pts[1] = terms[src].V;
        if (l == 2) s->pts[2] = terms[src].W;
        if (l < 3) {                                            // three lanes, three conversions to affine
            const XYZZ<C> p = l == 0 ? xyzz_add<C>(s->pts[0], s->pts[WAVE_FB_LANES]) : s->pts[l];
            Affine<C> q = xyzz_to_affine<C>(p);
            if (l == 1) q.y = neg<typename C::FqP>(q.y);
            s->P[l] = q;
        }
        if (l == 3) s->P[3] = Affine<C>::infinity();
    } else if (l < PAIRING_MAX_PAIRS) {
        s->P[l] = l < k ? pts[src * (size_t)k + l] : Affine<C>::infinity();
    }
    __syncthreads();
    // PM_WAVE_STOP_AFTER (PM_BUILD_FLAGS, profiling builds only: the byte written is no verdict): 1 ends the kernel after the prelude,
    // 2 after the Miller loop, so that the launch's GPU ms of three builds split the kernel's time (profiles/verify_batch_wave_pairing.txt)
#if defined(PM_WAVE_STOP_AFTER)
    if (PM_WAVE_STOP_AFTER == 1) {
        if (l == 0 && i < count) is_one[i] = (uint8_t)(s->P[0].x.l[0] & 1u);
        return;
    }
#endif

    const WaveGroup<C> grp{s, l, consts};
    grp.miller(tab, k, pairs);
#if defined(PM_WAVE_STOP_AFTER)
    if (PM_WAVE_STOP_AFTER == 2) {
        if (l == 0 && i < count) is_one[i] = (uint8_t)(s->a.c[0].c0.l[0] & 1u);
        return;
    }
#endif
    const typename Tower<C>::Fq2 r = grp.final_exp();
    const unsigned long long votes = __ballot(l < 6 ? W::is_one_coeff(l, r) : true);
    const bool one = ((votes >> (grouped ? g * WAVE_GROUP : 0)) & 63ull) == 63ull;
    if (l == 0 && i < count) is_one[i] = one && !(terms && live && !live[i]) ? 1 : 0;
}

template <class C>
int fixed_base_prepare(pm_ctx *ctx, const Affine<C> &G, ScopedDevBuf *out) {
    std::vector<XYZZ<C>> tab(WAVE_FB_ENTRIES);
    WaveTower<C>::fixed_base_build(G, tab.data());
    PM_HIP(ctx, out->reserve(tab.size() * sizeof(XYZZ<C>)));
    PM_HIP(ctx, hipMemcpyAsync(out->p, tab.data(), tab.size() * sizeof(XYZZ<C>), hipMemcpyHostToDevice, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));             // tab is this call's
    return PM_OK;
}

template <class C>
int pairing_check_wave_launch(pm_ctx *ctx, const PairingPrepared &prep, const ScopedDevBuf &fixed_base, const Affine<C> *d_pts, const VerifyTerm<C> *d_terms,
                              const uint32_t *d_neg_g, const uint8_t *d_live, size_t count, uint8_t *d_is_one, int timing_slot) {
    typedef Tower<C> T;
    if (!count) return PM_OK;
    if (d_terms ? prep.k != 3 || !fixed_base.p || !d_neg_g : !d_pts) return PM_ERR_INVALID_ARG;
    StageTimer t(ctx, timing_slot);
    PM_LAUNCH(ctx, k_pairing_check_wave<C>, dim3((unsigned)((count + WAVE_CHECKS - 1) / WAVE_CHECKS)), dim3(64), 0, ctx->stream,
                   (const typename T::Line *)prep.buf.p, (const typename T::Consts *)((const uint8_t *)prep.buf.p + prep.consts_offset), prep.k, prep.pairs,
                   d_pts, d_terms, d_neg_g, d_live, (const XYZZ<C> *)fixed_base.p, count, d_is_one);
    return PM_OK;
}

#define PM_INSTANTIATE_PAIRING_WAVE(C)                                                                                                         \
    template int fixed_base_prepare<C>(pm_ctx *, const Affine<C> &, ScopedDevBuf *);                                                           \
    template int pairing_check_wave_launch<C>(pm_ctx *, const PairingPrepared &, const ScopedDevBuf &, const Affine<C> *, const VerifyTerm<C> *, \
                                              const uint32_t *, const uint8_t *, size_t, uint8_t *, int);
PM_INSTANTIATE_PAIRING_WAVE(BlsCurve)
PM_INSTANTIATE_PAIRING_WAVE(BnCurve)

}  // namespace pm
