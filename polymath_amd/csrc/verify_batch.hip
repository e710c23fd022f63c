// pm_verify_batch: many Polymath proofs against one verifying key, one verdict each (include/polymath_hip.h; DESIGN.md "Batch
// verification").  A single verification is O(1) and stays host code (pm_host_verify); a batch is dominated by per-proof G1 work --
// three decompressions with a subgroup check and four scalar multiplications -- which runs here on the device.  The pairing checks,
// a handful per valid batch, run on the host (host/pairing.hpp; pm_verify_batch, PM_VERIFY_PAIRING_HOST) or on the device
// (pairing_batch.hip; pm_verify_batch2 with PM_VERIFY_PAIRING_DEVICE: the root in a launch of one lane, then every live leaf in ONE launch).
//
//   host   : repack the 3 point records of every proof, upload                       |  device: k_g1_decode (validate = 1)
//   host   : per proof x1, x2, c(x1) as Polymath::verify computes them (threads)      |
//   host   : weights rho_i from the batch's hash; scalars rho, rho x2, rho x1; g_i    |  device: k_verify_terms, k_verify_tree per level
//   host   : root check (3 Miller loops, one final exponentiation); on failure bisect over the device's sum tree
//   device mode instead: line tables of [z]_2, [x]_2, [1]_2 (host, once) | k_pairing_check on the root; on failure on all leaves
#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <thread>

#include "internal.h"
#include "verify_batch.cuh"
#include "../host/polymath.hpp"
#include "../host/wire.hpp"

namespace {

using namespace pm;

constexpr size_t VERIFY_MAX_COUNT = (size_t)1 << 20;

// body(i) for i < count on the host's glue threads (PM_HOST_THREADS, else up to 16); the first exception is re-thrown here
template <class F>
void glue_threads(size_t count, F body) {
    unsigned T = (unsigned)host_threads_env();
    if (!T) T = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (count < 2 * (size_t)T) T = 1;
    std::vector<std::exception_ptr> errs(T);
    auto run = [&](unsigned t) {
        try {
            for (size_t i = count * t / T; i < count * (t + 1) / T; ++i) body(i);
        } catch (...) { errs[t] = std::current_exception(); }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) {
        try { th.emplace_back(run, t); } catch (const std::system_error &) { run(t); }
    }
    run(0);
    for (auto &x : th) x.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}

struct DevBufs {   // the call's device memory: released on every way out
    DevBuf in, pts, status, scalars, tree, neg_g, live, is_one, a_at, inputs, g, ok, tap;
    PairingPrepared prep;
    ~DevBufs() {
        in.release(); pts.release(); status.release(); scalars.release(); tree.release();
        neg_g.release(); live.release(); is_one.release(); prep.buf.release();
        a_at.release(); inputs.release(); g.release(); ok.release(); tap.release();
    }
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <class C, class T>
int verify_batch_impl(pm_ctx *ctx, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *inputs, size_t n_inputs, const uint8_t *proofs,
                      size_t count, const uint8_t *seed32, int pairing, int challenges, uint8_t *verdicts, int *all_accepted, size_t *n_checks) {
    typedef pmhost::FrOps<C> F;
    typedef typename F::Fr Fr;
    typedef typename C::FrP R;
    typedef pmhost::Polymath<C, T> PMath;
    typedef typename PMath::Pairing Pairing;
    constexpr size_t NB = 4 * C::FqP::N, PL = 3 * NB + 32;
    const size_t off_pt[3] = {0, NB, 2 * NB + 32};                 // a_g1, c_g1, (a_at_x1), d_g1: data_structures.rs:10-19

    pmhost::Reader rd(vk_bytes, vk_len);
    const pmhost::VerifyingKeyT<C> vk = pmhost::read_vk_c<C>(rd);   // throws on malformed bytes (-> PM_ERR_INVALID_ARG)
    if (rd.off != vk_len) return PM_ERR_INVALID_ARG;

    size_t padded = 1;
    unsigned depth = 0;
    while (padded < count) { padded <<= 1; ++depth; }

    // ---- device: decode the 3 count points
    DevBufs d;
    TimingGuard flush{ctx};
    timing_reset(ctx);
    StageTimer t_all(ctx, T_PHASE);
    std::vector<uint8_t> packed(3 * count * NB);
    for (size_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k) memcpy(&packed[(3 * i + k) * NB], proofs + i * PL + off_pt[k], NB);
    PM_HIP(ctx, d.in.reserve(packed.size()));
    PM_HIP(ctx, d.pts.reserve(3 * count * sizeof(Affine<C>)));
    PM_HIP(ctx, d.status.reserve(3 * count));
    PM_HIP(ctx, d.scalars.reserve(count * sizeof(VerifyScalars)));
    PM_HIP(ctx, d.tree.reserve((2 * padded - 1) * sizeof(VerifyTerm<C>)));
    PM_HIP(ctx, hipMemcpyAsync(d.in.p, packed.data(), packed.size(), hipMemcpyHostToDevice, ctx->stream));
    {
        StageTimer t(ctx, T_WITNESS_MAP);
        PM_TRY(g1_decode_device<C>(ctx, d.in.as<uint8_t>(), 3 * count, true, d.pts.as<Affine<C>>(), d.status.as<uint8_t>(), nullptr, 0));
    }

    // ---- host, meanwhile: the weights' key, then per proof the transcript and scalar glue of verify_proof (verifier.rs:24-42)
    const auto t_glue = std::chrono::steady_clock::now();
    pmhost::StdRng rng;
    {
        static const char tag[] = "polymath-verify-batch";
        pmhost::Bytes h(tag, tag + sizeof(tag) - 1);
        const uint8_t zero_seed[32] = {0};
        const uint8_t *seed = seed32 ? seed32 : zero_seed;
        h.insert(h.end(), seed, seed + 32);
        h.insert(h.end(), vk_bytes, vk_bytes + vk_len);
        pmhost::ser_u64((uint64_t)transcript, h);
        const uint8_t *in_bytes = (const uint8_t *)inputs;
        h.insert(h.end(), in_bytes, in_bytes + count * n_inputs * sizeof(Fr));
        h.insert(h.end(), proofs, proofs + count * PL);
        const pmhost::Bytes key = pmhost::keccak256(h);
        rng = pmhost::StdRng::from_seed(key.data());
    }
    std::vector<VerifyScalars> sc(count);
    std::vector<Fr> g(count);                                       // g_i = rho_i (a_at_x1 + x2 c_at_x1), Montgomery; 0 without weight
    std::vector<uint8_t> bad(count, 0);                             // malformed: a_at_x1 >= r here, refused points below
    for (size_t i = 0; i < count; ++i) {
        uint64_t lo = rng.next_u64(), hi = rng.next_u64();
        if (!(lo | hi)) lo = 1;
        sc[i].rho[0] = (uint32_t)lo; sc[i].rho[1] = (uint32_t)(lo >> 32); sc[i].rho[2] = (uint32_t)hi; sc[i].rho[3] = (uint32_t)(hi >> 32);
    }
    const bool device_challenges = challenges == PM_VERIFY_CHALLENGES_DEVICE;
    std::vector<uint8_t> st(3 * count);
    if (device_challenges) {
        // The per-proof transcript and scalar glue as ONE launch behind the decode (challenges.hip): the lanes read [a]_1 and [c]_1
        // from the packed records the decoder reads, a(x1) and the public inputs from two more uploads -- no byte goes up twice --
        // and write the scalars where k_verify_terms takes them.  Back come one byte and g_i per proof,
        // and the three challenges for pm_prove_tap(8).
        std::vector<uint8_t> a_at(32 * count), ok(count);
        for (size_t i = 0; i < count; ++i) memcpy(&a_at[32 * i], proofs + i * PL + 2 * NB, 32);
        const size_t in_bytes = count * n_inputs * sizeof(Fr);
        PM_HIP(ctx, d.a_at.reserve(a_at.size()));
        if (in_bytes) PM_HIP(ctx, d.inputs.reserve(in_bytes));
        PM_HIP(ctx, d.g.reserve(count * sizeof(Fr)));
        PM_HIP(ctx, d.ok.reserve(count));
        PM_HIP(ctx, hipMemcpyAsync(d.a_at.p, a_at.data(), a_at.size(), hipMemcpyHostToDevice, ctx->stream));
        if (in_bytes) PM_HIP(ctx, hipMemcpyAsync(d.inputs.p, inputs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(d.scalars.p, sc.data(), count * sizeof(VerifyScalars), hipMemcpyHostToDevice, ctx->stream));   // the weights
        const uint8_t *in = d.in.as<uint8_t>();
        const ChallengeRows rows{in, in + NB, d.a_at.as<uint8_t>(), 3 * NB, 3 * NB, 32, d.inputs.as<uint64_t>(), n_inputs, count, d.status.as<uint8_t>()};
        PM_HIP(ctx, d.tap.reserve(3 * count * sizeof(Fr)));
        Fr *tap = d.tap.as<Fr>();
        PM_TRY(verifier_challenges_launch<C>(ctx, transcript, vk.n, vk.sigma, vk.omega, rows, tap, tap + count, tap + 2 * count, d.ok.as<uint8_t>(),
                                             d.scalars.as<VerifyScalars>(), d.g.as<Fr>(), T_MSM_TOTAL));
        ctx->timing_ms[T_MSM_SORT] = ms_since(t_glue);
        std::vector<Fr> tap_host(3 * count);
        PM_HIP(ctx, hipMemcpyAsync(ok.data(), d.ok.p, count, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync((void *)g.data(), d.g.p, count * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(st.data(), d.status.p, st.size(), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync((void *)tap_host.data(), d.tap.p, 3 * count * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        // what the lanes derived, kept for pm_prove_tap(8): per proof x1, x2, c(x1) (Montgomery) and a word that is 1 iff a(x1) < r
        ctx->verify_tap.assign(16 * count, 0);
        for (size_t i = 0; i < count; ++i) {
            for (int k = 0; k < 3; ++k) memcpy(&ctx->verify_tap[16 * i + 4 * k], tap_host[k * count + i].l, sizeof(Fr));
            ctx->verify_tap[16 * i + 12] = ok[i];
        }
        // `sc` holds the weights only from here on: the records are the device's (d.scalars), rows without weight zeroed by the lane
        // the malformed-point merge on the host's side: `bad` and g_i
        for (size_t i = 0; i < count; ++i) {
            bad[i] = !ok[i] || (st[3 * i] | st[3 * i + 1] | st[3 * i + 2]);
            if (bad[i]) g[i] = Fr::zero();
        }
    } else {
        ctx->verify_tap.clear();
        glue_threads(count, [&](size_t i) {
            const uint8_t *p = proofs + i * PL;
            Fr a_at_x1;
            try {
                a_at_x1 = F::from_le_bytes_canonical(p + 2 * NB);
            } catch (const std::runtime_error &) {
                bad[i] = 1;
                return;
            }
            std::vector<Fr> pub(n_inputs);
            if (n_inputs) memcpy((void *)pub.data(), inputs + i * n_inputs * PM_FR_LIMBS, n_inputs * sizeof(Fr));
            const typename PMath::Challenges ch = PMath::verifier_challenges(vk, pub, p, p + NB, a_at_x1);
            Fr rho = Fr::zero();
            memcpy(rho.l, sc[i].rho, 16);
            rho = to_mont<R>(rho);
            const Fr rx2 = from_mont<R>(F::mul(rho, ch.x2)), rx1 = from_mont<R>(F::mul(rho, ch.x1));
            memcpy(sc[i].rx2, rx2.l, 32);
            memcpy(sc[i].rx1, rx1.l, 32);
            g[i] = F::mul(rho, F::add(a_at_x1, F::mul(ch.x2, ch.c_at_x1)));
        });
        ctx->timing_ms[T_MSM_SORT] = ms_since(t_glue);
        PM_HIP(ctx, hipMemcpyAsync(st.data(), d.status.p, st.size(), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < count; ++i) {
            if (st[3 * i] | st[3 * i + 1] | st[3 * i + 2]) bad[i] = 1;
            if (bad[i]) { memset(&sc[i], 0, sizeof(VerifyScalars)); g[i] = Fr::zero(); }   // no weight: never enters a sum
        }
    }

    // ---- device: the terms and their sum tree
    if (!device_challenges) PM_HIP(ctx, hipMemcpyAsync(d.scalars.p, sc.data(), count * sizeof(VerifyScalars), hipMemcpyHostToDevice, ctx->stream));
    VerifyTerm<C> *tree = d.tree.as<VerifyTerm<C>>();
    {
        StageTimer t(ctx, T_NTT);
        PM_LAUNCH(ctx, k_verify_terms<C>, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, ctx->stream, d.pts.as<Affine<C>>(),
                       d.status.as<uint8_t>(), d.scalars.as<VerifyScalars>(), count, padded, tree);
    }
    {
        StageTimer t(ctx, T_POLY);
        for (unsigned l = 1; l <= depth; ++l) {
            const size_t nodes = padded >> l;
            PM_LAUNCH(ctx, k_verify_tree<C>, dim3((unsigned)((3 * nodes + 255) / 256)), dim3(256), 0, ctx->stream,
                           tree + verify_level_offset(padded, l - 1), tree + verify_level_offset(padded, l), nodes);
        }
    }
    t_all.stop();
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // ---- host: one check per visited node
    std::vector<Fr> g_pre(count + 1, Fr::zero());
    std::vector<size_t> live_pre(count + 1, 0);
    for (size_t i = 0; i < count; ++i) {
        g_pre[i + 1] = F::add(g_pre[i], g[i]);
        live_pre[i + 1] = live_pre[i] + (bad[i] ? 0 : 1);
    }
    auto lo_of = [&](unsigned level, size_t idx) { return std::min(count, idx << level); };
    auto live_in = [&](unsigned level, size_t idx) { return live_pre[lo_of(level, idx + 1)] - live_pre[lo_of(level, idx)]; };
    size_t checks = 0;
    int hip_status = PM_OK;
    double pairing_ms = 0;
    // e(U_S - g_S G, [z]_2) e(-V_S, [x]_2) e(W_S, [1]_2) == 1 for the node's set S
    auto check = [&](unsigned level, size_t idx) -> bool {
        VerifyTerm<C> nd;
        if (hipMemcpyAsync(&nd, tree + verify_level_offset(padded, level) + idx, sizeof(nd), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            hip_status = PM_ERR_HIP;
            return false;
        }
        const auto t0 = std::chrono::steady_clock::now();
        ++checks;
        const Fr gs = from_mont<R>(F::neg(F::sub(g_pre[lo_of(level, idx + 1)], g_pre[lo_of(level, idx)])));
        XYZZ<C> lhs = nd.U;
        if (!vk.one_g1.inf) {
            XYZZ<C> acc = XYZZ<C>::identity();
            for (int i = R::N - 1; i >= 0; --i)
                for (int b = 31; b >= 0; --b) {
                    acc = xyzz_dbl<C>(acc);
                    if ((gs.l[i] >> b) & 1) xyzz_madd<C>(acc, vk.one_g1.p, false);
                }
            lhs = xyzz_add<C>(lhs, acc);
        }
        Affine<C> neg_v = xyzz_to_affine<C>(nd.V);
        neg_v.y = neg<typename C::FqP>(neg_v.y);
        const std::vector<typename Pairing::Pair> pairs{{xyzz_to_affine<C>(lhs), lhs.is_identity(), vk.z_g2},
                                                        {neg_v, nd.V.is_identity(), vk.x_g2},
                                                        {xyzz_to_affine<C>(nd.W), nd.W.is_identity(), vk.one_g2}};
        const bool ok = Pairing::product_is_one(pairs);
        pairing_ms += ms_since(t0);
        return ok;
    };
    std::vector<uint8_t> verdict(count);
    for (size_t i = 0; i < count; ++i) verdict[i] = bad[i] ? PM_VERIFY_MALFORMED : PM_VERIFY_ACCEPTED;
    const bool any_bad = live_pre[count] != count;
    if (pairing == PM_VERIFY_PAIRING_DEVICE) {
        // The same equation, one lane per node: the root alone, then -- a leaf's check being the reference's own equation raised to
        // a non-zero weight, hence exact -- every live leaf at once.  The lanes form -g G, -V and the affine points themselves.
        const auto t0 = std::chrono::steady_clock::now();
        bool root_ok = true;
        if (live_pre[count]) {
            constexpr int N = C::FqP::N;
            const typename Pairing::G2 *q[3] = {&vk.z_g2, &vk.x_g2, &vk.one_g2};
            uint32_t g2[3][4 * N] = {};
            unsigned pairs = 0;
            for (int j = 0; j < 3; ++j) {
                if (q[j]->inf) continue;
                pairs |= 1u << j;
                memcpy(&g2[j][0], q[j]->x.c0.l, 4 * N); memcpy(&g2[j][N], q[j]->x.c1.l, 4 * N);
                memcpy(&g2[j][2 * N], q[j]->y.c0.l, 4 * N); memcpy(&g2[j][3 * N], q[j]->y.c1.l, 4 * N);
            }
            PM_TRY(pairing_prepare<C>(ctx, &g2[0][0], 3, pairs, &d.prep));
            const Affine<C> G = vk.one_g1.inf ? Affine<C>::infinity() : vk.one_g1.p;
            std::vector<Fr> neg_g(count + 1);                    // canonical; the root's behind the leaves'
            std::vector<uint8_t> live(count), is_one(count + 1, 0);
            for (size_t i = 0; i < count; ++i) { neg_g[i] = from_mont<R>(F::neg(g[i])); live[i] = bad[i] ? 0 : 1; }
            neg_g[count] = from_mont<R>(F::neg(g_pre[count]));
            PM_HIP(ctx, d.neg_g.reserve((count + 1) * sizeof(Fr)));
            PM_HIP(ctx, d.live.reserve(count));
            PM_HIP(ctx, d.is_one.reserve(count + 1));
            PM_HIP(ctx, hipMemcpyAsync(d.neg_g.p, neg_g.data(), (count + 1) * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
            PM_HIP(ctx, hipMemcpyAsync(d.live.p, live.data(), count, hipMemcpyHostToDevice, ctx->stream));
            PM_TRY(pairing_check_launch<C>(ctx, d.prep, nullptr, tree + verify_level_offset(padded, depth), d.neg_g.as<uint32_t>() + 8 * count, nullptr, G, 1,
                                           d.is_one.as<uint8_t>() + count, T_MSM_REDUCE));
            PM_HIP(ctx, hipMemcpyAsync(&is_one[count], d.is_one.as<uint8_t>() + count, 1, hipMemcpyDeviceToHost, ctx->stream));
            PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            checks = 1;
            root_ok = is_one[count] != 0;
            if (!root_ok && verdicts) {
                PM_TRY(pairing_check_launch<C>(ctx, d.prep, nullptr, tree, d.neg_g.as<uint32_t>(), d.live.as<uint8_t>(), G, count, d.is_one.as<uint8_t>(),
                                               T_MSM_REDUCE));
                PM_HIP(ctx, hipMemcpyAsync(is_one.data(), d.is_one.p, count, hipMemcpyDeviceToHost, ctx->stream));
                PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
                for (size_t i = 0; i < count; ++i)
                    if (!bad[i] && !is_one[i]) verdict[i] = PM_VERIFY_REJECTED;
                checks += live_pre[count];
            }
        }
        ctx->timing_ms[T_MSM_ACCUMULATE] = ms_since(t0);
        if (verdicts) memcpy(verdicts, verdict.data(), count);
        *all_accepted = root_ok && !any_bad ? 1 : 0;
        if (n_checks) *n_checks = checks;
        return PM_OK;
    }
    const bool root_ok = live_pre[count] == 0 || check(depth, 0);
    if (!root_ok && verdicts && hip_status == PM_OK) {
        // A failing node has a failing child.  The Miller product of a node is the product of its children's, so when the left child
        // passes the right one is known to fail: no check.  A node without a live proof passes by construction.
        struct Item { unsigned level; size_t idx; };
        std::vector<Item> failing{{depth, 0}};
        while (!failing.empty() && hip_status == PM_OK) {
            const Item it = failing.back();
            failing.pop_back();
            if (it.level == 0) { verdict[it.idx] = PM_VERIFY_REJECTED; continue; }
            const unsigned cl = it.level - 1;
            const size_t left = 2 * it.idx, right = 2 * it.idx + 1;
            const bool left_ok = live_in(cl, left) == 0 || check(cl, left);
            if (!left_ok) failing.push_back({cl, left});
            if (live_in(cl, right) == 0) continue;
            if (left_ok || !check(cl, right)) failing.push_back({cl, right});
        }
    }
    if (hip_status != PM_OK) { ctx->err = "pm_verify_batch: reading a node of the sum tree failed"; return hip_status; }
    ctx->timing_ms[T_MSM_ACCUMULATE] = pairing_ms;
    if (verdicts) memcpy(verdicts, verdict.data(), count);
    *all_accepted = root_ok && !any_bad ? 1 : 0;
    if (n_checks) *n_checks = checks;
    return PM_OK;
}

}  // namespace

extern "C" int pm_verify_batch2(pm_ctx *ctx, int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                                const uint8_t *proofs, size_t proof_len, size_t count, const uint8_t *seed32, int pairing, uint8_t *verdicts,
                                int *all_accepted, size_t *n_checks) {
    // `pairing` is a pm_verify_pairing value, optionally OR-ed with PM_VERIFY_CHALLENGES_DEVICE
    const int challenges = pairing & PM_VERIFY_CHALLENGES_DEVICE;
    pairing &= ~PM_VERIFY_CHALLENGES_DEVICE;
    if (pairing != PM_VERIFY_PAIRING_HOST && pairing != PM_VERIFY_PAIRING_DEVICE) return PM_ERR_INVALID_ARG;
    if (!ctx || !vk_bytes || !all_accepted || (count && (!proofs || (n_inputs && !public_inputs)))) return PM_ERR_INVALID_ARG;
    if (curve != PM_BLS12_381 && curve != PM_BN254) return PM_ERR_INVALID_ARG;
    if (!pmhost::transcript_ok(transcript)) return PM_ERR_INVALID_ARG;
    if (proof_len != (curve == PM_BLS12_381 ? 176u : 128u) || count > VERIFY_MAX_COUNT) return PM_ERR_INVALID_ARG;
    *all_accepted = 0;
    if (n_checks) *n_checks = 0;
    try {
        if (!count) {                                   // the vk is still parsed: a malformed key is an error at every count
            pmhost::Reader rd(vk_bytes, vk_len);
            if (curve == PM_BLS12_381) (void)pmhost::read_vk_c<BlsCurve>(rd);
            else (void)pmhost::read_vk_c<BnCurve>(rd);
            if (rd.off != vk_len) return PM_ERR_INVALID_ARG;
            *all_accepted = 1;
            return PM_OK;
        }
        if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
        return with_curve(curve, [&](auto cv) {
            typedef type_of<decltype(cv)> C;
            return pmhost::with_transcript<C>(transcript, [&](auto t) {
                return verify_batch_impl<C, type_of<decltype(t)>>(ctx, transcript, vk_bytes, vk_len, public_inputs, n_inputs, proofs, count, seed32, pairing,
                                                                  challenges, verdicts, all_accepted, n_checks);
            });
        });
    } catch (const pmhost::WireError &) {               // malformed vk bytes
        return PM_ERR_INVALID_ARG;
    } catch (const std::bad_alloc &) {
        ctx->err = "pm_verify_batch: out of host memory";
        return PM_ERR_STATE;
    } catch (const std::exception &e) {                 // Fr: non-canonical encoding in the vk (omega)
        ctx->err = e.what();
        return PM_ERR_INVALID_ARG;
    }
}

extern "C" int pm_verify_batch(pm_ctx *ctx, int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                               const uint8_t *proofs, size_t proof_len, size_t count, const uint8_t *seed32, uint8_t *verdicts, int *all_accepted,
                               size_t *n_checks) {
    return pm_verify_batch2(ctx, curve, transcript, vk_bytes, vk_len, public_inputs, n_inputs, proofs, proof_len, count, seed32, PM_VERIFY_PAIRING_HOST,
                            verdicts, all_accepted, n_checks);
}
