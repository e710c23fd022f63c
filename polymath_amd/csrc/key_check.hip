// PM_KEY_CHECK_RELATIONS of pm_pk_load_bytes: is the key that was just decoded what generate_proving_key would have produced for some
// (x, z)?  host/key_check.hpp states the relations, their order and texts, the weight indices and the indices into T, and makes the
// same decision on the CPU with naive sums; this file makes it with what is resident:
//   k_key_weights     the call's 32-byte seed expanded by ChaCha12 (host/rng.hpp: chacha12_weight), weight i = block i, 128 bits,
//                     written as the Montgomery Fr msm_run reads
//   k_key_sap_eval    one lane per domain row: the evaluations of U = sum_j rho_j u_j and W = sum_j rho_j w_j -- csr_row_dot over the
//                     key's A, B, C with z = rho, plus the unit entries of the y columns (common.rs:138-207, by rows)
//   ntt_run_batch     both rows to coefficients in one inverse transform
//   msm_run           thirteen MSMs over the PLAIN resident points (the window tables do not exist yet): two per ratio, one over
//                     uj_wj_lcs, two over T
//   k_key_points      the three G1 points of every pairing product from the MSM results and single resident points (the anchors'
//                     difference, the negations), and relation 0's comparison
//   pairing_check_wave_launch   ONE launch, a wave a relation, on the tables of one pairing_prepare of the vk's [1]_2, [x]_2, [z]_2
// Everything the check reserves is call-scoped and the MSM workspace it grew is released before it returns, so that the table
// planner sees the HBM a load without the check would have left it.
#include "internal.h"
#include "fq28.cuh"
#include "prove_common.cuh"
#include "../host/key_check.hpp"

namespace pm {

struct KeySeed {
    uint32_t key[8];
};

template <class P>
__global__ void k_key_weights(KeySeed seed, uint64_t count, Fp<P> *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t w[4];
    pmhost::chacha12_weight(seed.key, i, w);
    Fp<P> c = Fp<P>::zero();
    for (int k = 0; k < 4; ++k) c.l[k] = w[k];
    out[i] = to_mont<P>(c);
}

// rho: the Lz weights of uj_wj_lcs, indexed by SAP column j - m0: m = m0 + mw R1CS columns, then the m0 + nr y columns
template <class P>
__global__ void k_key_sap_eval(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *rho, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t n, Fp<P> *ue,
                               Fp<P> *we) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t m = m0 + mw;
    Fp<P> u = Fp<P>::zero(), w = Fp<P>::zero();
    if (i < m0) {
        w = add<P>(dbl<P>(dbl<P>(rho[i])), rho[m + i]);
    } else if (i < 2 * m0) {
        w = rho[m + i - m0];
    } else if (i < 2 * m0 + 2 * nr) {
        const bool upper = i >= 2 * m0 + nr;
        const uint64_t r = i - 2 * m0 - (upper ? nr : 0);
        const Fp<P> az = csr_row_dot<P>(A.rowptr, A.col, A.val, rho, r), bz = csr_row_dot<P>(B.rowptr, B.col, B.val, rho, r);
        w = rho[m + m0 + r];
        if (upper) {
            u = sub<P>(az, bz);
        } else {
            u = add<P>(az, bz);
            w = add<P>(dbl<P>(dbl<P>(csr_row_dot<P>(Cm.rowptr, Cm.col, Cm.val, rho, r))), w);
        }
    }
    ue[i] = u;
    we[i] = w;
}

// where k_key_points reads: element offsets into the key's resident base array, and the MSM results in the order the driver ran them
enum { KEY_MSM_RATIO = 0 /* hi, lo per ratio */, KEY_MSM_LCS = 10, KEY_MSM_TU = 11, KEY_MSM_TW = 12, KEY_MSMS = 13 };
constexpr int KEY_PAIRINGS = pmhost::KEY_REL_COUNT - 1;   // every relation but the comparison
struct KeyPointRefs {
    uint64_t xp0, t_z, t_gamma, t_alpha, t_zh_lo, t_zh_hi, yg0, ya0, zh0;
};

template <class C>
__device__ static Affine<C> key_resident_point(const Affine<C> *bases, uint64_t at) {   // internal form -> standard Montgomery
    const Affine<C> a = bases[at];
    if (a.is_inf()) return a;
    return Affine<C>{fq_int_to_std<C>(a.x), fq_int_to_std<C>(a.y)};
}
template <class C>
__device__ static Affine<C> key_negated(Affine<C> a) {
    if (!a.is_inf()) a.y = neg<typename C::FqP>(a.y);
    return a;
}

// lane t < KEY_PAIRINGS: the points of relation t + 1 against [1]_2, [x]_2, [z]_2; lane KEY_PAIRINGS: relation 0
template <class C>
__global__ void k_key_points(const Affine<C> *bases, KeyPointRefs at, const Affine<C> *msm, Affine<C> one_g1, Affine<C> *pts, uint8_t *first_ok) {
    const int t = (int)threadIdx.x;
    if (t > KEY_PAIRINGS) return;
    if (t == KEY_PAIRINGS) {
        const Affine<C> a = key_resident_point<C>(bases, at.xp0);
        *first_ok = a.x.eq(one_g1.x) && a.y.eq(one_g1.y) ? 1 : 0;
        return;
    }
    const int rel = t + 1;
    Affine<C> p1 = Affine<C>::infinity(), px = p1, pz = p1;
    if (rel < pmhost::KEY_REL_ANCHOR) {                       // e(hi, [1]_2) e(-lo, [x]_2)
        const int r = rel - pmhost::KEY_REL_RATIO;
        p1 = msm[KEY_MSM_RATIO + 2 * r];
        px = key_negated<C>(msm[KEY_MSM_RATIO + 2 * r + 1]);
    } else if (rel == pmhost::KEY_REL_ANCHOR) {               // e(T[g s], [1]_2) e(-one_g1, [z]_2)
        p1 = key_resident_point<C>(bases, at.t_z);
        pz = key_negated<C>(one_g1);
    } else if (rel == pmhost::KEY_REL_ANCHOR + 1) {           // e(-T[0], [1]_2) e(y_gamma[0], [z]_2)
        p1 = key_negated<C>(key_resident_point<C>(bases, at.t_gamma));
        pz = key_resident_point<C>(bases, at.yg0);
    } else if (rel == pmhost::KEY_REL_ANCHOR + 2) {           // e(-T[(g - a) s], [1]_2) e(y_alpha[0], [z]_2)
        p1 = key_negated<C>(key_resident_point<C>(bases, at.t_alpha));
        pz = key_resident_point<C>(bases, at.ya0);
    } else if (rel == pmhost::KEY_REL_ANCHOR + 3) {           // e(T[(a + g) s] - T[n + (a + g) s], [1]_2) e(zh[0], [z]_2)
        XYZZ<C> d = XYZZ<C>::from_affine(key_resident_point<C>(bases, at.t_zh_lo));
        xyzz_madd<C>(d, key_resident_point<C>(bases, at.t_zh_hi), true);
        p1 = xyzz_to_affine<C>(d);
        pz = key_resident_point<C>(bases, at.zh0);
    } else {                                                  // e(-(TU + TW), [1]_2) e(sum rho lcs, [z]_2)
        XYZZ<C> s = XYZZ<C>::from_affine(msm[KEY_MSM_TU]);
        xyzz_madd<C>(s, msm[KEY_MSM_TW], false);
        p1 = key_negated<C>(xyzz_to_affine<C>(s));
        pz = msm[KEY_MSM_LCS];
    }
    pts[3 * t] = p1;
    pts[3 * t + 1] = px;
    pts[3 * t + 2] = pz;
}

// The timers the check's stages leave pending are this call's: they go back to the pool unread on every way out, so that the stage
// times of the context's last proof stay what they were.
struct KeyCheckTimers {
    pm_ctx *ctx;
    size_t keep;
    explicit KeyCheckTimers(pm_ctx *c) : ctx(c), keep(c->pending_timers.size()) {}
    ~KeyCheckTimers() {
        for (size_t i = keep; i < ctx->pending_timers.size(); ++i) {
            ctx->event_pool.push_back(ctx->pending_timers[i].a);
            ctx->event_pool.push_back(ctx->pending_timers[i].b);
        }
        ctx->pending_timers.resize(keep);
    }
};
struct KeyCheckWorkspace {   // the MSM workspace and the transforms' temporary, released unless an MSM of the caller's is in flight
    pm_ctx *ctx;
    ~KeyCheckWorkspace() {
        if (ctx->msm_async) return;
        (void)hipStreamSynchronize(ctx->stream);
        MsmWorkspace &m = ctx->msm;
        for (DevBuf *b : {&m.set.sorted, &m.set.counts, &m.set.bucket_off, &m.set.task_off, &m.set.tasks, &m.set.partials, &m.set.task_cnt, &m.digits,
                          &m.cursor, &m.wsum, &m.region, &m.sub, &m.digits2, &m.len_bins, &m.block_cnt, &m.hot, &m.batch, &ctx->ntt_tmp})
            b->release();
    }
};

template <class C>
int key_check_run(pm_ctx *ctx, const pm_pk *pk, const Affine<C> &one_g1, const uint32_t *g2, const uint8_t seed[32], int *failed) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    *failed = pmhost::KEY_REL_NONE;
    if (!pk->whole_resident()) return PM_ERR_INVALID_ARG;
    const pmhost::KeyCheckPlan p = pmhost::key_check_plan(pk->n, pk->m0, pk->mw, pk->nr);
    for (int v = 0; v < PM_NUM_BASE_VECS; ++v)
        if (p.len[v] != pk->base_len[v]) return PM_ERR_STATE;
    HostProfile hp("key check", 0);
    auto mark = [&](const char *label) {   // PM_PROFILE_HOST=1: the stage split, each stage synchronised
        if (hp.on) { (void)hipStreamSynchronize(ctx->stream); hp.mark(label); }
    };
    KeyCheckTimers timers(ctx);
    KeyCheckWorkspace workspace{ctx};
    ScopedDevBuf d_w, d_uw, d_msm, d_pts, d_ok;
    PM_HIP(ctx, d_w.reserve(p.weights * sizeof(Fr)));
    PM_HIP(ctx, d_uw.reserve(2 * p.n * sizeof(Fr)));
    PM_HIP(ctx, d_msm.reserve(KEY_MSMS * sizeof(Affine<C>)));
    PM_HIP(ctx, d_pts.reserve(3 * KEY_PAIRINGS * sizeof(Affine<C>)));
    PM_HIP(ctx, d_ok.reserve(pmhost::KEY_REL_COUNT));
    Fr *w = d_w.as<Fr>(), *ue = d_uw.as<Fr>(), *we = ue + p.n;

    KeySeed ks;
    for (int i = 0; i < 8; ++i) ks.key[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) | ((uint32_t)seed[4 * i + 3] << 24);
    PM_LAUNCH(ctx, k_key_weights<P>, dim3(nblk(p.weights)), dim3(256), 0, ctx->stream, ks, p.weights, w);
    mark("weights");

    const CsrDev A{pk->d_rowptr[0], pk->d_col[0], pk->d_val[0]}, B{pk->d_rowptr[1], pk->d_col[1], pk->d_val[1]}, Cm{pk->d_rowptr[2], pk->d_col[2], pk->d_val[2]};
    PM_LAUNCH(ctx, k_key_sap_eval<P>, dim3(nblk(p.n)), dim3(256), 0, ctx->stream, A, B, Cm, w + p.w_off[PM_UJ_WJ_LCS_BY_Y_ALPHA], p.m0, p.mw, p.nr, p.n, ue, we);
    PM_TRY(ntt_run_batch<C>(ctx, ue, pk->log_n, true, 2, p.n));
    mark("sap evaluations + transforms");

    const Affine<C> *bases = (const Affine<C> *)pk->d_bases;   // whole_resident: device offsets are the concatenation's
    Affine<C> h_msm[KEY_MSMS];
    auto msm = [&](int slot, const Affine<C> *d_b, const Fr *d_s, uint64_t len) -> int {
        int inf = 0;
        PM_TRY(msm_run<C>(ctx, d_b, d_s, (size_t)len, &h_msm[slot], &inf));
        if (inf) h_msm[slot] = Affine<C>::infinity();
        return PM_OK;
    };
    for (int r = 0; r < 5; ++r) {
        const int v = pmhost::KEY_RATIO_VECS[r];
        const Affine<C> *vb = bases + pk->seg_off[v];
        PM_TRY(msm(KEY_MSM_RATIO + 2 * r, vb + 1, w + p.w_off[v], p.len[v] - 1));
        PM_TRY(msm(KEY_MSM_RATIO + 2 * r + 1, vb, w + p.w_off[v], p.len[v] - 1));
    }
    PM_TRY(msm(KEY_MSM_LCS, bases + pk->off_lcs, w + p.w_off[PM_UJ_WJ_LCS_BY_Y_ALPHA], p.Lz));
    PM_TRY(msm(KEY_MSM_TU, bases + pk->off_ygz + p.t_u, ue, p.n));
    PM_TRY(msm(KEY_MSM_TW, bases + pk->off_ygz + p.t_w, we, p.n));
    mark("msms");

    PM_HIP(ctx, hipMemcpyAsync(d_msm.p, h_msm, sizeof(h_msm), hipMemcpyHostToDevice, ctx->stream));
    const KeyPointRefs at{pk->off_xp, pk->off_ygz + p.t_z, pk->off_ygz + p.t_gamma, pk->off_ygz + p.t_alpha, pk->off_ygz + p.t_zh_lo,
                          pk->off_ygz + p.t_zh_hi, pk->off_yg, pk->off_ya, pk->off_zh};
    uint8_t *ok = d_ok.as<uint8_t>();
    PM_LAUNCH(ctx, k_key_points<C>, dim3(1), dim3(64), 0, ctx->stream, bases, at, d_msm.as<Affine<C>>(), one_g1, d_pts.as<Affine<C>>(), ok);
    PairingPrepared prep;
    PM_TRY(pairing_prepare<C>(ctx, g2, 3, 7u, &prep));
    PM_TRY(pairing_check_wave_launch<C>(ctx, prep, ScopedDevBuf(), d_pts.as<Affine<C>>(), nullptr, nullptr, nullptr, KEY_PAIRINGS, ok + 1, T_PHASE));
    uint8_t h_ok[pmhost::KEY_REL_COUNT];
    PM_HIP(ctx, hipMemcpyAsync(h_ok, ok, sizeof(h_ok), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hp.mark("points + pairing launch");
    for (int rel = pmhost::KEY_REL_COUNT - 1; rel >= 0; --rel)
        if (!h_ok[rel]) *failed = rel;
    return PM_OK;
}

template int key_check_run<BlsCurve>(pm_ctx *, const pm_pk *, const Affine<BlsCurve> &, const uint32_t *, const uint8_t *, int *);
template int key_check_run<BnCurve>(pm_ctx *, const pm_pk *, const Affine<BnCurve> &, const uint32_t *, const uint8_t *, int *);

}  // namespace pm
