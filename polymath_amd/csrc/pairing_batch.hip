// Pairing product checks on the device, one lane per check (include/polymath_hip.h: pm_pairing_check_batch; pm_verify_batch2 with
// PM_VERIFY_PAIRING_DEVICE; DESIGN.md "Batch verification").  The G2 arguments of every check are the same k points, so the host
// prepares their Miller-loop lines once (pairing.cuh: prepare) and all lanes read the table at wave-uniform addresses; what a lane
// does is Fq12 arithmetic on its own G1 points: a shared-squaring Miller loop and the x-chain final exponentiation.
//
//   host  : Frobenius constants, k line tables (68 lines a point on BLS12-381, 102 on BN254), upload
//   device: k_pairing_check -- lane i takes its k points from a dense array, or (batch verification) forms them from node i of the
//           sum tree: U_i + (-g_i) G, -V_i, W_i, each brought to affine coordinates with one inversion
//
// An Fq12 is 576 bytes on BLS12-381: the tower lives in scratch and its functions are real calls (PM_HD_COLD), no LDS.
#include <cstring>
#include <new>

#include "internal.h"
#include "pairing.cuh"
#include "verify_batch.cuh"

namespace pm {

template <class C>
__global__ __launch_bounds__(64) void k_pairing_check(const typename Tower<C>::Line *tab, const typename Tower<C>::Consts *consts, int k, unsigned pairs,
                                                      const Affine<C> *pts, const VerifyTerm<C> *terms, const uint32_t *neg_g, const uint8_t *live,
                                                      Affine<C> G, size_t count, uint8_t *is_one) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Affine<C> P[PAIRING_MAX_PAIRS];
    if (terms) {                                                // k == 3: e(U - g G, [z]_2) e(-V, [x]_2) e(W, [1]_2)
        if (live && !live[i]) { is_one[i] = 0; return; }
        verify_node_points<C>(terms[i], neg_g + 8 * i, G, P);
        P[3] = Affine<C>::infinity();
    } else {
#pragma unroll 1
        for (int j = 0; j < PAIRING_MAX_PAIRS; ++j) P[j] = j < k ? pts[i * (size_t)k + j] : Affine<C>::infinity();
    }
    is_one[i] = Tower<C>::product_is_one(tab, k, pairs, P, *consts) ? 1 : 0;
}

template <class C>
int pairing_prepare(pm_ctx *ctx, const uint32_t *g2, int k, unsigned pairs, PairingPrepared *out) {
    typedef Tower<C> T;
    typedef PairingParams<C> PP;
    constexpr int N = C::FqP::N;
    if (k < 1 || k > PAIRING_MAX_PAIRS) return PM_ERR_INVALID_ARG;
    const typename T::Consts K = T::make_consts();
    std::vector<typename T::Line> tab((size_t)k * PP::LINES);
    memset((void *)tab.data(), 0, tab.size() * sizeof(typename T::Line));
    for (int j = 0; j < k; ++j) {
        if (!((pairs >> j) & 1u)) continue;
        typename T::G2Affine A;
        memcpy((void *)&A, g2 + (size_t)j * 4 * N, sizeof A);   // x.c0 || x.c1 || y.c0 || y.c1
        if (!T::g2_on_twist(A)) return PM_ERR_INVALID_ARG;
        T::prepare(A, K, &tab[(size_t)j * PP::LINES]);
    }
    const size_t tab_bytes = tab.size() * sizeof(typename T::Line);
    PM_HIP(ctx, out->buf.reserve(tab_bytes + sizeof K));
    PM_HIP(ctx, hipMemcpyAsync(out->buf.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP(ctx, hipMemcpyAsync((uint8_t *)out->buf.p + tab_bytes, &K, sizeof K, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));             // tab and K are this call's
    out->k = k;
    out->pairs = pairs;
    out->consts_offset = tab_bytes;
    return PM_OK;
}

template <class C>
int pairing_check_launch(pm_ctx *ctx, const PairingPrepared &prep, const Affine<C> *d_pts, const VerifyTerm<C> *d_terms, const uint32_t *d_neg_g,
                         const uint8_t *d_live, const Affine<C> &G, size_t count, uint8_t *d_is_one, int timing_slot) {
    typedef Tower<C> T;
    if (!count) return PM_OK;
    if (d_terms && prep.k != 3) return PM_ERR_INVALID_ARG;
    StageTimer t(ctx, timing_slot);
    PM_LAUNCH(ctx, k_pairing_check<C>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, ctx->stream, (const typename T::Line *)prep.buf.p,
                   (const typename T::Consts *)((const uint8_t *)prep.buf.p + prep.consts_offset), prep.k, prep.pairs, d_pts, d_terms, d_neg_g, d_live,
                   G, count, d_is_one);
    return PM_OK;
}

#define PM_INSTANTIATE_PAIRING(C)                                                                                                               \
    template int pairing_prepare<C>(pm_ctx *, const uint32_t *, int, unsigned, PairingPrepared *);                                              \
    template int pairing_check_launch<C>(pm_ctx *, const PairingPrepared &, const Affine<C> *, const VerifyTerm<C> *, const uint32_t *, const uint8_t *, \
                                         const Affine<C> &, size_t, uint8_t *, int);
PM_INSTANTIATE_PAIRING(BlsCurve)
PM_INSTANTIATE_PAIRING(BnCurve)

}  // namespace pm

namespace {

using namespace pm;

constexpr size_t PAIRING_MAX_COUNT = (size_t)1 << 22;

template <class C>
int pairing_check_batch_impl(pm_ctx *ctx, const uint64_t *g2, size_t k, const void *g1, size_t stride, size_t count, uint8_t *is_one) {
    const size_t PT = sizeof(Affine<C>);
    if (stride < PT) return PM_ERR_INVALID_ARG;
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PairingPrepared prep;
    ScopedDevBuf d_pts, d_out;
    TimingGuard flush{ctx};
    timing_reset(ctx);
    PM_TRY(pairing_prepare<C>(ctx, (const uint32_t *)g2, (int)k, (1u << k) - 1u, &prep));
    std::vector<Affine<C>> pts(count * k);
    const uint8_t *s = (const uint8_t *)g1;
    for (size_t i = 0; i < count * k; ++i) {
        memcpy((void *)&pts[i], s + i * stride, PT);
        if (stride > PT && s[i * stride + PT] != 0) pts[i] = Affine<C>::infinity();   // arkworks' `infinity: bool`
    }
    PM_HIP(ctx, d_pts.reserve(pts.size() * PT));
    PM_HIP(ctx, d_out.reserve(count));
    PM_HIP(ctx, hipMemcpyAsync(d_pts.p, pts.data(), pts.size() * PT, hipMemcpyHostToDevice, ctx->stream));
    PM_TRY(pairing_check_launch<C>(ctx, prep, d_pts.as<Affine<C>>(), nullptr, nullptr, nullptr, Affine<C>::infinity(), count, d_out.as<uint8_t>(), T_PHASE));
    PM_HIP(ctx, hipMemcpyAsync(is_one, d_out.p, count, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

}  // namespace

extern "C" int pm_pairing_check_batch(pm_ctx *ctx, int curve, const uint64_t *g2, size_t k, const void *g1, size_t g1_stride, size_t count,
                                      uint8_t *is_one) {
    if (!ctx || !g2 || k < 1 || k > (size_t)PAIRING_MAX_PAIRS || count > PAIRING_MAX_COUNT) return PM_ERR_INVALID_ARG;
    if (curve != PM_BLS12_381 && curve != PM_BN254) return PM_ERR_INVALID_ARG;
    if (!count) return PM_OK;
    if (!g1 || !is_one) return PM_ERR_INVALID_ARG;
    try {
        return with_curve(curve, [&](auto cv) { return pairing_check_batch_impl<type_of<decltype(cv)>>(ctx, g2, k, g1, g1_stride, count, is_one); });
    } catch (const std::bad_alloc &) {
        ctx->err = "pm_pairing_check_batch: out of host memory";
        return PM_ERR_STATE;
    }
}
