// pm_verify_batch: many Polymath proofs against one verifying key, one verdict each (include/polymath_hip.h; DESIGN.md "Batch
// verification").  A single verification is O(1) and stays host code (pm_host_verify); a batch is dominated by per-proof G1 work --
// three decompressions with a subgroup check and four scalar multiplications -- which runs here on the device.  The pairing checks,
// a handful per valid batch, run on the host (host/pairing.hpp; pm_verify_batch, PM_VERIFY_PAIRING_HOST) or on the device
// (pairing_batch.hip; pm_verify_batch2 with PM_VERIFY_PAIRING_DEVICE: the root in a launch of one lane, then every live leaf in ONE launch).
// PM_VERIFY_PAIRING_DEVICE_WAVE is that mode with a check spread over 36 lanes of a wave (pairing_wave.hip): the root, and the leaves while few.
// The call is a sequence of stages over one state struct (VerifyCall), in stream order:
//   decode_points         host: repack the 3 point records of every proof, upload     | device: k_g1_decode (validate = 1)
//   batch_weights         host: weights rho_i from the batch's hash
//   challenges_on_host    host: per proof x1, x2, c(x1) as Polymath::verify computes them (threads), verify_weigh; upload
//   challenges_on_device  instead: k_verifier_challenges, one lane per proof, verify_weigh in the lane; pm_prove_tap(8) is filled
//   build_tree            device: k_verify_terms, k_verify_tree per level              | host: prefix sums of g_i and of the live proofs
//   pairing_on_host       root check (3 Miller loops, one final exponentiation); on failure bisect over the device's sum tree
//   pairing_on_device     instead: line tables of [z]_2, [x]_2, [1]_2 (host, once) | k_pairing_check on the root; on failure on all leaves
// and ONE epilogue (verify_batch_impl).  The stage timers carry the verifier's names for the slots (internal.h: TV_*).
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

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// One call's state and its stages.  Declared before the call's timers, so the device memory outlives them.
template <class C>
struct VerifyCall {
    typedef typename C::FrP R;
    typedef Fp<R> Fr;
    typedef typename pmhost::PairingOf<C>::type Pairing;
    static constexpr size_t NB = 4 * C::FqP::N, PL = 3 * NB + 32;   // a point record; a proof: a_g1, c_g1, a_at_x1, d_g1 (data_structures.rs:10-19)
    pm_ctx *ctx;
    int transcript;
    const uint8_t *vk_bytes, *proofs, *seed32;   // the caller's
    const uint64_t *inputs;
    size_t vk_len, n_inputs, count;
    bool want_verdicts;
    pmhost::VerifyingKeyT<C> vk;
    size_t padded = 1;                           // 2^depth >= count: the leaves of the sum tree
    unsigned depth = 0;
    ScopedDevBuf in, pts, status, scalars, tree, neg_g, live, is_one, a_at, pub, g_dev, ok, tap;
    PairingPrepared prep;
    ScopedDevBuf fixed_base;         // wave mode: the table of G's multiples (pairing_wave.hip)
    std::vector<uint8_t> packed;     // the point records as uploaded: stay until the call is over
    std::chrono::steady_clock::time_point t_glue;   // the host's side of the challenges stage starts here
    // After the challenges stage: the scalar records are on the device (scalars), g_i = rho_i (a_at_x1 + x2 c_at_x1) (Montgomery) and
    // bad[i] (malformed: a_at_x1 >= r or a refused point) are here, and a row without weight is zero in all three.
    std::vector<VerifyScalars> sc;   // the host's copy: complete in host mode, the weights alone in device mode
    std::vector<Fr> g, g_pre;        // g_pre, live_pre: prefix sums of g and of the live proofs -- a node's share is a difference
    std::vector<uint8_t> bad, verdict;
    std::vector<size_t> live_pre;
    size_t checks = 0;
    bool root_ok = true;
    VerifyTerm<C> *nodes(unsigned level) const { return tree.as<VerifyTerm<C>>() + verify_level_offset(padded, level); }
    size_t lo_of(unsigned level, size_t idx) const { return std::min(count, idx << level); }
    size_t live_in(unsigned level, size_t idx) const { return live_pre[lo_of(level, idx + 1)] - live_pre[lo_of(level, idx)]; }
    size_t live_total() const { return live_pre[count]; }
    // -g_S mod r of node idx of a level, canonical: what verify_node_points takes
    Fr neg_g_of(unsigned level, size_t idx) const { return from_mont<R>(neg<R>(sub<R>(g_pre[lo_of(level, idx + 1)], g_pre[lo_of(level, idx)]))); }
    Affine<C> one_g1() const { return vk.one_g1.inf ? Affine<C>::infinity() : vk.one_g1.p; }

    int decode_points() {
        const size_t off_pt[3] = {0, NB, 2 * NB + 32};
        packed.resize(3 * count * NB);
        for (size_t i = 0; i < count; ++i)
            for (int k = 0; k < 3; ++k) memcpy(&packed[(3 * i + k) * NB], proofs + i * PL + off_pt[k], NB);
        PM_HIP(ctx, in.reserve(packed.size()));
        PM_HIP(ctx, pts.reserve(3 * count * sizeof(Affine<C>)));
        PM_HIP(ctx, status.reserve(3 * count));
        PM_HIP(ctx, scalars.reserve(count * sizeof(VerifyScalars)));
        PM_HIP(ctx, tree.reserve((2 * padded - 1) * sizeof(VerifyTerm<C>)));
        PM_HIP(ctx, hipMemcpyAsync(in.p, packed.data(), packed.size(), hipMemcpyHostToDevice, ctx->stream));
        StageTimer t(ctx, TV_DECODE);
        return g1_decode_device<C>(ctx, in.as<uint8_t>(), 3 * count, true, pts.as<Affine<C>>(), status.as<uint8_t>(), nullptr, 0);
    }

    // rho_i != 0 of 128 bits, keyed by the hash of everything the batch consists of
    void batch_weights() {
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
        pmhost::StdRng rng = pmhost::StdRng::from_seed(key.data());
        sc.assign(count, VerifyScalars{});
        for (size_t i = 0; i < count; ++i) {
            uint64_t lo = rng.next_u64(), hi = rng.next_u64();
            if (!(lo | hi)) lo = 1;
            sc[i].rho[0] = (uint32_t)lo; sc[i].rho[1] = (uint32_t)(lo >> 32); sc[i].rho[2] = (uint32_t)hi; sc[i].rho[3] = (uint32_t)(hi >> 32);
        }
    }

    // The end of both challenge stages, once the decoder's verdicts (st: three bytes a proof) are down: a proof with a refused point
    // joins the malformed ones; whatever is malformed loses its weight here (on the device: the zeroed record's upload, or the lane's `live`)
    void merge_refused_points(const std::vector<uint8_t> &st) {
        for (size_t i = 0; i < count; ++i) {
            if (st[3 * i] | st[3 * i + 1] | st[3 * i + 2]) bad[i] = 1;
            if (bad[i]) { sc[i] = VerifyScalars{}; g[i] = Fr::zero(); }   // no weight: never enters a sum
        }
    }

    // Per proof the transcript of verify_proof (verifier.rs:24-42) and verify_weigh on the glue threads, while the device decodes;
    // then the scalar records go up.  T: the host transcript class.
    template <class T>
    int challenges_on_host() {
        typedef pmhost::Polymath<C, T> PMath;
        ctx->verify_tap.clear();
        glue_threads(count, [&](size_t i) {
            const uint8_t *p = proofs + i * PL;
            Fr a_at_x1;
            try {
                a_at_x1 = pmhost::FrOps<C>::from_le_bytes_canonical(p + 2 * NB);
            } catch (const std::runtime_error &) {
                bad[i] = 1;
                return;
            }
            std::vector<Fr> pub_in(n_inputs);
            if (n_inputs) memcpy((void *)pub_in.data(), inputs + i * n_inputs * PM_FR_LIMBS, n_inputs * sizeof(Fr));
            const typename PMath::Challenges ch = PMath::verifier_challenges(vk, pub_in, p, p + NB, a_at_x1);
            g[i] = verify_weigh<C>(sc[i], ch.x1, ch.x2, ch.c_at_x1, a_at_x1, true);
        });
        ctx->timing_ms[TV_HOST_GLUE] = ms_since(t_glue);
        std::vector<uint8_t> st(3 * count);
        PM_HIP(ctx, hipMemcpyAsync(st.data(), status.p, st.size(), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        merge_refused_points(st);
        PM_HIP(ctx, hipMemcpyAsync(scalars.p, sc.data(), count * sizeof(VerifyScalars), hipMemcpyHostToDevice, ctx->stream));
        return PM_OK;
    }

    // The same as ONE launch behind the decode (challenges.hip).  The lanes read [a]_1 and [c]_1 from the packed records the decoder
    // reads, a(x1) and the public inputs from two more uploads -- no byte goes up twice -- and write the scalar records where
    // k_verify_terms takes them.  Back come one byte and g_i per proof, and the three challenges for pm_prove_tap(8).
    int challenges_on_device() {
        const size_t in_bytes = count * n_inputs * sizeof(Fr);
        std::vector<uint8_t> a_at_host(32 * count), ok_host(count), st(3 * count);
        for (size_t i = 0; i < count; ++i) memcpy(&a_at_host[32 * i], proofs + i * PL + 2 * NB, 32);
        PM_HIP(ctx, a_at.reserve(a_at_host.size()));
        if (in_bytes) PM_HIP(ctx, pub.reserve(in_bytes));
        PM_HIP(ctx, g_dev.reserve(count * sizeof(Fr)));
        PM_HIP(ctx, ok.reserve(count));
        PM_HIP(ctx, hipMemcpyAsync(a_at.p, a_at_host.data(), a_at_host.size(), hipMemcpyHostToDevice, ctx->stream));
        if (in_bytes) PM_HIP(ctx, hipMemcpyAsync(pub.p, inputs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(scalars.p, sc.data(), count * sizeof(VerifyScalars), hipMemcpyHostToDevice, ctx->stream));   // the weights
        const uint8_t *rec = in.as<uint8_t>();
        const ChallengeRows rows{rec, rec + NB, a_at.as<uint8_t>(), 3 * NB, 3 * NB, 32, pub.as<uint64_t>(), n_inputs, count, status.as<uint8_t>()};
        PM_HIP(ctx, tap.reserve(3 * count * sizeof(Fr)));
        Fr *d_tap = tap.as<Fr>();
        PM_TRY(verifier_challenges_launch<C>(ctx, transcript, vk.n, vk.sigma, vk.omega, rows, d_tap, d_tap + count, d_tap + 2 * count, ok.as<uint8_t>(),
                                             scalars.as<VerifyScalars>(), g_dev.as<Fr>(), TV_CHALLENGE_KERNEL));
        ctx->timing_ms[TV_HOST_GLUE] = ms_since(t_glue);
        std::vector<Fr> tap_host(3 * count);
        PM_HIP(ctx, hipMemcpyAsync(ok_host.data(), ok.p, count, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync((void *)g.data(), g_dev.p, count * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(st.data(), status.p, st.size(), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync((void *)tap_host.data(), tap.p, 3 * count * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        // what the lanes derived, kept for pm_prove_tap(8): per proof x1, x2, c(x1) (Montgomery) and a word that is 1 iff a(x1) < r
        ctx->verify_tap.assign(16 * count, 0);
        for (size_t i = 0; i < count; ++i) {
            for (int k = 0; k < 3; ++k) memcpy(&ctx->verify_tap[16 * i + 4 * k], tap_host[k * count + i].l, sizeof(Fr));
            ctx->verify_tap[16 * i + 12] = ok_host[i];
            bad[i] = !ok_host[i];
        }
        merge_refused_points(st);
        return PM_OK;
    }

    // The terms (U, V, W) of every proof, then their sums level by level; meanwhile the prefix sums the pairing stage needs
    int build_tree() {
        StageTimer t_terms(ctx, TV_TERMS);
        PM_LAUNCH(ctx, k_verify_terms<C>, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, ctx->stream, pts.as<Affine<C>>(),
                       status.as<uint8_t>(), scalars.as<VerifyScalars>(), count, padded, nodes(0));
        t_terms.stop();
        StageTimer t_tree(ctx, TV_TREE);
        for (unsigned l = 1; l <= depth; ++l)
            PM_LAUNCH(ctx, k_verify_tree<C>, dim3((unsigned)((3 * (padded >> l) + 255) / 256)), dim3(256), 0, ctx->stream, nodes(l - 1), nodes(l), padded >> l);
        t_tree.stop();
        g_pre.assign(count + 1, Fr::zero());
        live_pre.assign(count + 1, 0);
        for (size_t i = 0; i < count; ++i) {
            g_pre[i + 1] = add<R>(g_pre[i], g[i]);
            live_pre[i + 1] = live_pre[i] + (bad[i] ? 0 : 1);
        }
        return PM_OK;
    }

    // One host check: e(U_S - g_S G, [z]_2) e(-V_S, [x]_2) e(W_S, [1]_2) == 1 for the set S of a node
    int host_node_check(unsigned level, size_t idx, bool *is_one) {
        VerifyTerm<C> nd;
        if (hipMemcpyAsync(&nd, nodes(level) + idx, sizeof(nd), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            ctx->err = "pm_verify_batch: reading a node of the sum tree failed";
            return PM_ERR_HIP;
        }
        const auto t0 = std::chrono::steady_clock::now();
        ++checks;
        Affine<C> P[3];
        verify_node_points<C>(nd, neg_g_of(level, idx).l, one_g1(), P);
        *is_one = Pairing::product_is_one({{P[0], P[0].is_inf(), vk.z_g2}, {P[1], P[1].is_inf(), vk.x_g2}, {P[2], P[2].is_inf(), vk.one_g2}});
        ctx->timing_ms[TV_PAIRING_HOST] += ms_since(t0);
        return PM_OK;
    }

    // The root; if it fails and verdicts are wanted, a bisection over the tree.  A failing node has a failing child.  The Miller
    // product of a node is the product of its children's, so when the left child passes the right one is known to fail: no check.
    // A node without a live proof passes by construction.
    int pairing_on_host() {
        if (live_total()) PM_TRY(host_node_check(depth, 0, &root_ok));
        if (root_ok || !want_verdicts) return PM_OK;
        struct Item { unsigned level; size_t idx; };
        std::vector<Item> failing{{depth, 0}};
        while (!failing.empty()) {
            const Item it = failing.back();
            failing.pop_back();
            if (it.level == 0) { verdict[it.idx] = PM_VERIFY_REJECTED; continue; }
            const unsigned cl = it.level - 1;
            const size_t left = 2 * it.idx, right = 2 * it.idx + 1;
            bool left_ok = true, right_ok = false;
            if (live_in(cl, left)) PM_TRY(host_node_check(cl, left, &left_ok));
            if (!left_ok) failing.push_back({cl, left});
            if (live_in(cl, right) == 0) continue;
            if (!left_ok) PM_TRY(host_node_check(cl, right, &right_ok));
            if (!right_ok) failing.push_back({cl, right});
        }
        return PM_OK;
    }

    // The same equation, one lane per node (pairing_batch.hip): the root alone, then -- a leaf's check being the reference's own
    // equation raised to a non-zero weight, hence exact -- every live leaf at once.  The lanes form -g G, -V and the affine points
    // themselves (verify_node_points).  Called with at least one live proof.
    // wave: the root by a group of lanes of one wave (pairing_wave.hip), and the leaves too while at most VERIFY_WAVE_LEAF_MAX are live;
    // the same equation on the same tables, so the same verdicts and the same count of checks.
    int pairing_on_device(bool wave) {
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
        PM_TRY(pairing_prepare<C>(ctx, &g2[0][0], 3, pairs, &prep));
        if (wave) PM_TRY(fixed_base_prepare<C>(ctx, one_g1(), &fixed_base));
        std::vector<Fr> neg_g_host(count + 1);               // canonical; the root's behind the leaves'
        std::vector<uint8_t> live_host(count), one_host(count + 1, 0);
        for (size_t i = 0; i < count; ++i) { neg_g_host[i] = from_mont<R>(neg<R>(g[i])); live_host[i] = bad[i] ? 0 : 1; }
        neg_g_host[count] = neg_g_of(depth, 0);
        PM_HIP(ctx, neg_g.reserve((count + 1) * sizeof(Fr)));
        PM_HIP(ctx, live.reserve(count));
        PM_HIP(ctx, is_one.reserve(count + 1));
        PM_HIP(ctx, hipMemcpyAsync(neg_g.p, neg_g_host.data(), (count + 1) * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(live.p, live_host.data(), count, hipMemcpyHostToDevice, ctx->stream));
        uint32_t *d_neg_g = neg_g.as<uint32_t>();
        uint8_t *d_is_one = is_one.as<uint8_t>();
        if (wave) PM_TRY(pairing_check_wave_launch<C>(ctx, prep, fixed_base, nullptr, nodes(depth), d_neg_g + 8 * count, nullptr, 1, d_is_one + count, TV_PAIRING_KERNELS));
        else PM_TRY(pairing_check_launch<C>(ctx, prep, nullptr, nodes(depth), d_neg_g + 8 * count, nullptr, one_g1(), 1, d_is_one + count, TV_PAIRING_KERNELS));
        PM_HIP(ctx, hipMemcpyAsync(&one_host[count], d_is_one + count, 1, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        checks = 1;
        root_ok = one_host[count] != 0;
        if (root_ok || !want_verdicts) return PM_OK;
        if (wave && live_total() <= VERIFY_WAVE_LEAF_MAX) PM_TRY(pairing_check_wave_launch<C>(ctx, prep, fixed_base, nullptr, nodes(0), d_neg_g, live.as<uint8_t>(), count, d_is_one, TV_PAIRING_KERNELS));
        else PM_TRY(pairing_check_launch<C>(ctx, prep, nullptr, nodes(0), d_neg_g, live.as<uint8_t>(), one_g1(), count, d_is_one, TV_PAIRING_KERNELS));
        PM_HIP(ctx, hipMemcpyAsync(one_host.data(), d_is_one, count, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < count; ++i)
            if (!bad[i] && !one_host[i]) verdict[i] = PM_VERIFY_REJECTED;
        checks += live_total();
        return PM_OK;
    }
};

template <class C, class T>
int verify_batch_impl(pm_ctx *ctx, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *inputs, size_t n_inputs, const uint8_t *proofs,
                      size_t count, const uint8_t *seed32, int pairing, int challenges, uint8_t *verdicts, int *all_accepted, size_t *n_checks) {
    VerifyCall<C> s{ctx, transcript, vk_bytes, proofs, seed32, inputs, vk_len, n_inputs, count, verdicts != nullptr,
                    pmhost::read_vk_exact<C>(vk_bytes, vk_len)};   // throws on malformed bytes (-> PM_ERR_INVALID_ARG)
    while (s.padded < count) { s.padded <<= 1; ++s.depth; }
    s.g.resize(count);
    s.bad.assign(count, 0);
    TimingGuard flush{ctx};
    timing_reset(ctx);
    StageTimer t_all(ctx, TV_DEVICE_TOTAL);
    PM_TRY(s.decode_points());
    s.t_glue = std::chrono::steady_clock::now();   // host, meanwhile
    s.batch_weights();
    PM_TRY(challenges == PM_VERIFY_CHALLENGES_DEVICE ? s.challenges_on_device() : s.template challenges_on_host<T>());
    PM_TRY(s.build_tree());
    t_all.stop();
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s.verdict.resize(count);
    for (size_t i = 0; i < count; ++i) s.verdict[i] = s.bad[i] ? PM_VERIFY_MALFORMED : PM_VERIFY_ACCEPTED;
    if (pairing != PM_VERIFY_PAIRING_HOST) {
        const auto t0 = std::chrono::steady_clock::now();
        if (s.live_total()) PM_TRY(s.pairing_on_device(pairing == PM_VERIFY_PAIRING_DEVICE_WAVE));
        ctx->timing_ms[TV_PAIRING_HOST] = ms_since(t0);
    } else {
        PM_TRY(s.pairing_on_host());
    }
    // the ONE way out with a result
    if (verdicts) memcpy(verdicts, s.verdict.data(), count);
    *all_accepted = s.root_ok && s.live_total() == count ? 1 : 0;
    if (n_checks) *n_checks = s.checks;
    return PM_OK;
}

}  // namespace

extern "C" int pm_verify_batch2(pm_ctx *ctx, int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                                const uint8_t *proofs, size_t proof_len, size_t count, const uint8_t *seed32, int pairing, uint8_t *verdicts,
                                int *all_accepted, size_t *n_checks) {
    // `pairing` is a pm_verify_pairing value, optionally OR-ed with PM_VERIFY_CHALLENGES_DEVICE
    const int challenges = pairing & PM_VERIFY_CHALLENGES_DEVICE;
    pairing &= ~PM_VERIFY_CHALLENGES_DEVICE;
    if (pairing != PM_VERIFY_PAIRING_HOST && pairing != PM_VERIFY_PAIRING_DEVICE && pairing != PM_VERIFY_PAIRING_DEVICE_WAVE) return PM_ERR_INVALID_ARG;
    if (!ctx || !vk_bytes || !all_accepted || (count && (!proofs || (n_inputs && !public_inputs)))) return PM_ERR_INVALID_ARG;
    if (curve != PM_BLS12_381 && curve != PM_BN254) return PM_ERR_INVALID_ARG;
    if (!pmhost::transcript_ok(transcript)) return PM_ERR_INVALID_ARG;
    if (proof_len != (curve == PM_BLS12_381 ? 176u : 128u) || count > VERIFY_MAX_COUNT) return PM_ERR_INVALID_ARG;
    *all_accepted = 0;
    if (n_checks) *n_checks = 0;
    try {
        if (!count) {                                   // the vk is still parsed: a malformed key is an error at every count
            if (curve == PM_BLS12_381) (void)pmhost::read_vk_exact<BlsCurve>(vk_bytes, vk_len);
            else (void)pmhost::read_vk_exact<BnCurve>(vk_bytes, vk_len);
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
