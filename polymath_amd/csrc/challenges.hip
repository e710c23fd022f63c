// The verifier's Fiat-Shamir challenges on the device (include/polymath_hip.h: pm_verify_batch2 with PM_VERIFY_CHALLENGES_DEVICE;
// DESIGN.md "Batch verification").  One proof per lane runs what Polymath::verifier_challenges runs on
// the host (host/polymath.hpp; verifier.rs:24-42): the transcript over the public inputs and the records of [a]_1 and [c]_1, x1,
// pi(x1) and c(x1), the transcript again, x2 -- transcript.cuh has the code, PM_HD, checked bit for bit on the CPU
// (tests/native/transcript_selftest.cpp).  Inside the batch verifier the lane goes on to the weighted scalars and g_i, so that
// the host does no field work per proof.
#include "internal.h"
#include "transcript.cuh"
#include "verify_batch.cuh"

namespace pm {

namespace {

constexpr unsigned CHALLENGE_BLOCK = 256;

template <class C>
struct ChallengeOut {
    Fp<typename C::FrP> *x1, *x2, *c_at_x1, *g;
    uint8_t *ok;
    VerifyScalars *scalars;
};

// One proof per lane.  Plain C++: the sponge states are per-lane private memory (transcript.cuh says why), no LDS.  The Merlin
// lanes repeat a rejected draw on their own; a wave is through when its last lane is.
template <class C, int KIND>
__global__ __launch_bounds__(CHALLENGE_BLOCK) void k_verifier_challenges(fs::FsVk<C> vk, ChallengeRows rows, ChallengeOut<C> out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows.count) return;
    fs::FsChallenges<C> ch;
    Fr a_at;
    const bool ok = fs::fs_verifier_challenges<C, KIND>(vk, (const Fr *)rows.d_inputs + i * rows.n_inputs, rows.n_inputs, rows.d_a + i * rows.a_stride,
                                                        rows.d_c + i * rows.c_stride, rows.d_a_at + i * rows.a_at_stride, &ch, &a_at);
    if (!ok) ch.x1 = ch.x2 = ch.c_at_x1 = a_at = Fr::zero();
    if (out.ok) out.ok[i] = ok ? 1 : 0;
    if (out.x1) out.x1[i] = ch.x1;
    if (out.x2) out.x2[i] = ch.x2;
    if (out.c_at_x1) out.c_at_x1[i] = ch.c_at_x1;
    if (out.scalars) {
        // the glue the host mode runs too (verify_batch.cuh: verify_weigh); a row that is not ok, or with a refused point, takes no part
        VerifyScalars sc = out.scalars[i];
        const uint8_t *st = rows.d_point_status;
        const bool live = ok && !(st && (st[3 * i] | st[3 * i + 1] | st[3 * i + 2]));
        out.g[i] = verify_weigh<C>(sc, ch.x1, ch.x2, ch.c_at_x1, a_at, live);
        out.scalars[i] = sc;
    }
}

template <class C, int KIND>
int launch_kind(pm_ctx *ctx, const fs::FsVk<C> &vk, const ChallengeRows &rows, const ChallengeOut<C> &out, int timing_slot) {
    StageTimer t(ctx, timing_slot);
    PM_LAUNCH(ctx, (k_verifier_challenges<C, KIND>), dim3((unsigned)((rows.count + CHALLENGE_BLOCK - 1) / CHALLENGE_BLOCK)), dim3(CHALLENGE_BLOCK), 0,
                   ctx->stream, vk, rows, out);
    return PM_OK;
}

}  // namespace

template <class C>
int verifier_challenges_launch(pm_ctx *ctx, int transcript, uint64_t n, uint64_t sigma, const Fp<typename C::FrP> &omega, const ChallengeRows &rows,
                               Fp<typename C::FrP> *d_x1, Fp<typename C::FrP> *d_x2, Fp<typename C::FrP> *d_c_at_x1, uint8_t *d_ok,
                               VerifyScalars *d_scalars, Fp<typename C::FrP> *d_g, int timing_slot) {
    typedef typename C::FrP P;
    if (!rows.count) return PM_OK;
    if (d_scalars && !d_g) return PM_ERR_INVALID_ARG;
    fs::FsVk<C> vk;
    vk.n = n;
    vk.sigma = sigma;
    vk.omega = omega;
    vk.n_inv = inverse<P>(from_u64<P>(n));   // compute_pi_at_x1's F::inv(F::from_u64(pk.n)), once per call
    const ChallengeOut<C> out{d_x1, d_x2, d_c_at_x1, d_g, d_ok, d_scalars};
    switch (transcript) {
        case PM_TRANSCRIPT_MERLIN: return launch_kind<C, fs::KIND_MERLIN>(ctx, vk, rows, out, timing_slot);
        case PM_TRANSCRIPT_KECCAK256: return launch_kind<C, fs::KIND_KECCAK256>(ctx, vk, rows, out, timing_slot);
        case PM_TRANSCRIPT_BLAKE3: return launch_kind<C, fs::KIND_BLAKE3>(ctx, vk, rows, out, timing_slot);
        default: return PM_ERR_INVALID_ARG;
    }
}
template int verifier_challenges_launch<BlsCurve>(pm_ctx *, int, uint64_t, uint64_t, const Fp<BlsFrP> &, const ChallengeRows &, Fp<BlsFrP> *, Fp<BlsFrP> *,
                                                  Fp<BlsFrP> *, uint8_t *, VerifyScalars *, Fp<BlsFrP> *, int);
template int verifier_challenges_launch<BnCurve>(pm_ctx *, int, uint64_t, uint64_t, const Fp<BnFrP> &, const ChallengeRows &, Fp<BnFrP> *, Fp<BnFrP> *,
                                                 Fp<BnFrP> *, uint8_t *, VerifyScalars *, Fp<BnFrP> *, int);

}  // namespace pm
