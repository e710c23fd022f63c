// The three GPU phases of create_proof_with_assignment (/root/reference/src/prover.rs:66-237),
// split at its two Fiat-Shamir calls (:126, :189).  Everything between the FFI and the three
// output points stays in HBM, in the context's ProveWs `pw` (internal.h).  The kernels are prove_kernels.cuh's, shared with the batch
// prover (prove_batch.hip), and so is phase 1's enqueue list: phase1_enqueue_u / phase1_enqueue_rest below run it for `rows` proofs
// of a ProveWs, here with rows = 1.  Phases 2 and 3 launch the kernels that take the per-proof values as arguments.
//
// The reference materialises U and W densely (prover.rs:87-96, O(n*M)); here the same u_evals /
// w_evals come from the closed form of SURVEY.md App. A in O(nnz): one lane per R1CS row.
#include <cstring>

#include <thread>

#include "internal.h"
#include "fq28.cuh"
#include "prove_common.cuh"
#include "prove_kernels.cuh"

namespace pm {

// MSM `which` over THIS rank's resident pairs.  d_scalars: the rank's scalars in the order of pk->pieces[which].
template <class C>
int msm_resident(pm_ctx *ctx, const pm_pk *pk, int which, const Fp<typename C::FrP> *d_scalars, uint64_t *out_xy, int *out_inf) {
    const Affine<C> *bases = (const Affine<C> *)pk->d_bases + pk->res_dev_off[which];
    Affine<C> r;
    int inf = 1;
    if (pk->tables[which].planned()) {   // this MSM's own window tables (window 0 = its resident pairs), or the wide mode on the plain array
        MsmTables tb = pk->tables[which];
        tb.base_index = 0;
        PM_TRY(msm_run<C>(ctx, tb.wide ? bases : (const Affine<C> *)nullptr, d_scalars, (size_t)pk->res_cnt[which], &r, &inf, &tb));
    } else {
        PM_TRY(msm_run<C>(ctx, bases, d_scalars, (size_t)pk->res_cnt[which], &r, &inf));
    }
    store_affine_host<C>(r, inf, out_xy, out_inf);
    return PM_OK;
}

// pairs [lo, lo + count) of MSM `which` (count = 0: all of them); d_scalars points at the MSM's FIRST scalar
template <class C>
int msm_resident_begin(pm_ctx *ctx, const pm_pk *pk, int which, const Fp<typename C::FrP> *d_scalars, uint64_t lo, uint64_t count) {
    const Affine<C> *bases = (const Affine<C> *)pk->d_bases + pk->res_dev_off[which];
    if (count == 0) { lo = 0; count = pk->res_cnt[which]; }
    if (lo + count > pk->res_cnt[which]) return PM_ERR_INVALID_ARG;
    if (pk->tables[which].planned()) {
        MsmTables tb = pk->tables[which];
        tb.base_index = (size_t)lo;
        return msm_begin<C>(ctx, tb.wide ? bases : (const Affine<C> *)nullptr, d_scalars + lo, (size_t)count, &tb);
    }
    return msm_begin<C>(ctx, bases + lo, d_scalars + lo, (size_t)count, (const MsmTables *)nullptr);
}
template <class C>
int msm_resident_end(pm_ctx *ctx, uint64_t *out_xy, int *out_inf) {
    Affine<C> r;
    int inf = 1;
    PM_TRY(msm_end<C>(ctx, &r, &inf));
    store_affine_host<C>(r, inf, out_xy, out_inf);
    return PM_OK;
}

// PM_SHARD_PAIRS: the scalar vector is the whole logical one; this rank's pairs are its one piece of the MSM's range
template <class C>
static int msm_shard(pm_ctx *ctx, const pm_pk *pk, int which, const Fp<typename C::FrP> *d_scalars, uint64_t *out_xy,
                     int *out_inf) {
    return msm_resident<C>(ctx, pk, which, d_scalars + (pk->pieces[which][0].cat_lo - pk->msm_lo[which]), out_xy, out_inf);
}

// ------------------------------------------------------------------------------- phase 1
// Phase 1 between the uploads and the MSMs, for the `rows` proofs whose x || w rows, r_a ([rows][2] in ws.rows) and zeroed flag words
// are in `ws`: the one enqueue list of both provers, in two halves so that the single prover can start its [a]_1 MSM in between.
// First half: witness map and SAP check, then u's coefficients (N1, prover.rs:94) and, with sc_a_now, the [a]_1 scalars.
template <class C>
int phase1_enqueue_u(pm_ctx *ctx, const pm_pk *pk, const ProofShape &d, ProveWs &ws, size_t rows, bool sc_a_now) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const uint64_t n = d.n, m0 = d.m0, mw = d.mw, nr = d.nr;
    const unsigned gy = (unsigned)rows;
    hipStream_t st = ctx->stream;
    Fr *xw = ws.xw.as<Fr>(), *ue = ws.ue.as<Fr>(), *we = ws.we.as<Fr>(), *u = ws.u.as<Fr>(), *wv = ws.w.as<Fr>();
    Fr *ztail = ws.sc_c.as<Fr>();  // z_tail is the head of the c-MSM scalar vector
    {
        StageTimer t(ctx, T_WITNESS_MAP);
        CsrDev A{pk->d_rowptr[0], pk->d_col[0], pk->d_val[0]}, B{pk->d_rowptr[1], pk->d_col[1], pk->d_val[1]},
            Cm{pk->d_rowptr[2], pk->d_col[2], pk->d_val[2]};
        const uint64_t head = n > m0 + mw ? n : m0 + mw;
        PM_LAUNCH(ctx, k_witness_head<P>, dim3(nblk(head), gy), dim3(256), 0, st, xw, m0 + mw, ue, we, ztail, d.len_c, m0, mw, nr, n);
        if (nr)
            PM_LAUNCH(ctx, k_witness_rows<P>, dim3(nblk(nr), gy), dim3(256), 0, st, A, B, Cm, xw, m0 + mw, ue, we, n, ztail + m0 + mw, d.len_c,
                      m0, nr);
        // rem == 0 of prover.rs:108  <=>  (Uz)^2 == Wz on the whole domain
        PM_LAUNCH(ctx, k_check_sap<P>, dim3(nblk(n), gy), dim3(256), 0, st, ue, we, n, ws.flags.as<unsigned>());
    }
    // N1, N2, N5 (prover.rs:94,96,160-162): coefficients of u, w and of the witness-only U part
    PM_HIP(ctx, hipMemcpyAsync(u, ue, rows * n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    PM_HIP(ctx, hipMemcpyAsync(wv, we, rows * n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    PM_TRY(ntt_run_batch<C>(ctx, u, pk->log_n, true, rows, n));
    if (sc_a_now) PM_LAUNCH(ctx, k_sc_a<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, ws.rows.as<Fr>(), (uint64_t)2, ws.sc_a.as<Fr>(), d.len_a, n);
    return PM_OK;
}

// Second half: w's coefficients, the witness-only part of u, u^2, and the [c]_1 scalars -- which also writes the [a]_1 scalars into
// `sc_a` unless that is null (k_sc_a has written them).
template <class C>
int phase1_enqueue_rest(pm_ctx *ctx, const pm_pk *pk, const ProofShape &d, ProveWs &ws, size_t rows, Fp<typename C::FrP> *sc_a) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const uint64_t n = d.n, m0 = d.m0;
    const unsigned gy = (unsigned)rows;
    hipStream_t st = ctx->stream;
    Fr *ue = ws.ue.as<Fr>(), *u = ws.u.as<Fr>(), *wv = ws.w.as<Fr>(), *wit_u = ws.wit_u.as<Fr>(), *u2 = ws.u2.as<Fr>(), *tmp = ws.tmp.as<Fr>();
    PM_TRY(ntt_run_batch<C>(ctx, wv, pk->log_n, true, rows, n));
    if (2 * m0 <= 16 && pk->log_n >= 1) {   // few public inputs: the sparse sum beats a fifth transform
        const Fr *winv = nullptr;
        PM_TRY(twiddles_get<C>(ctx, pk->log_n, true, &winv));
        StageTimer t(ctx, T_NTT);
        PM_LAUNCH(ctx, k_wit_u_sparse<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, ue, winv, inverse<P>(from_u64<P>(n)), n, (unsigned)(2 * m0),
                  wit_u);
    } else {
        PM_LAUNCH(ctx, k_copy_zero_head<P>, dim3(nblk(n), gy), dim3(256), 0, st, ue, wit_u, n, 2 * m0);
        PM_TRY(ntt_run_batch<C>(ctx, wit_u, pk->log_n, true, rows, n));
    }
    // square_polynomial (prover.rs:315-328) via the negacyclic half (see k_twist); the 2n-point domain of
    // the reference must still exist (the callers check it), its root psi = omega_2n is the twist.
    {
        const Fr *psi = nullptr, *psi_inv = nullptr;
        PM_TRY(twiddles_get<C>(ctx, pk->log_n + 1, false, &psi));
        PM_TRY(twiddles_get<C>(ctx, pk->log_n + 1, true, &psi_inv));
        PM_LAUNCH(ctx, k_twist<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, psi, tmp, n);
        PM_TRY(ntt_run_batch<C>(ctx, tmp, pk->log_n, false, rows, n));
        PM_LAUNCH(ctx, k_square<P>, dim3(nblk(n), gy), dim3(256), 0, st, tmp, n);
        PM_TRY(ntt_run_batch<C>(ctx, tmp, pk->log_n, true, rows, n));
        PM_LAUNCH(ctx, k_untwist_combine<P>, dim3(nblk(n), gy), dim3(256), 0, st, tmp, psi_inv, wv, u2, n, inverse<P>(from_u64<P>(2)));
    }
    {
        StageTimer t(ctx, T_POLY);
        PM_LAUNCH(ctx, k_phase1_scalars<P>, dim3(nblk(n + 1), gy), dim3(256), 0, st, u, u2, ws.rows.as<Fr>(), (uint64_t)2, ws.sc_c.as<Fr>() + d.Lz,
                  d.len_c, sc_a, d.len_a, n, ws.flags.as<unsigned>());
    }
    return PM_OK;
}

template <class C>
int prove_phase1_impl(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, const uint64_t *r_a,
                      uint64_t *a_xy, int *a_inf, uint64_t *c_xy, int *c_inf, bool assignment_on_device) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const ProofShape d = proof_shape(pk);
    const uint64_t n = d.n, m0 = d.m0, mw = d.mw;
    if (pk->log_n + 1 > (unsigned)C::TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;  // prover.rs:317
    hipStream_t st = ctx->stream;
    PhaseTimers timers(ctx, pk);
    ProveWs &ws = ctx->pw;
    PM_HIP(ctx, ws.xw.reserve((m0 + mw) * sizeof(Fr)));
    for (DevBuf *b : {&ws.ue, &ws.we, &ws.u, &ws.w, &ws.wit_u, &ws.tmp}) PM_HIP(ctx, b->reserve(n * sizeof(Fr)));
    PM_HIP(ctx, ws.u2.reserve(2 * n * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_c.reserve(d.len_c * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_a.reserve(d.len_a * sizeof(Fr)));
    PM_HIP(ctx, ws.rows.reserve(2 * sizeof(Fr)));      // r_a
    PM_HIP(ctx, ws.flags.reserve(64));
    Fr *xw = ws.xw.as<Fr>(), *sc_c = ws.sc_c.as<Fr>(), *sc_a = ws.sc_a.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    PM_HIP(ctx, hipMemsetAsync(flags, 0, 64, st));
    const hipMemcpyKind kind = assignment_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    PM_HIP(ctx, hipMemcpyAsync(xw, x, m0 * sizeof(Fr), kind, st));
    if (mw) PM_HIP(ctx, hipMemcpyAsync(xw + m0, w, mw * sizeof(Fr), kind, st));
    PM_HIP(ctx, hipMemcpyAsync(ws.rows.p, r_a, 2 * sizeof(Fr), hipMemcpyHostToDevice, st));
    memcpy(ctx->ra_host, r_a, 2 * sizeof(Fr));
    // [a]_1 = M1 + M2 needs only u and r_a, and is independent of [c]_1 = M7 + M6 + M3 + M4 + M5: it runs on a helper
    // context (own stream and workspace) from a second host thread, started after u's transform -- its sort, bucket reduction and
    // host finish are dependent chains that leave the chip mostly idle, and hide under the remaining transforms and
    // the larger MSM's accumulation.  The helper stream waits on an event, the host does not.  PM_OPT_MSM_OVERLAP = 0
    // runs the two MSMs back to back after the checks.
    const bool overlap = ctx->opt.v[PM_OPT_MSM_OVERLAP] != 0;
    pm_ctx *const aux_ctx = overlap ? ctx_aux(ctx) : nullptr;
    int st_a = PM_OK;   // written by the helper thread: declared before the joiner so that it outlives the join
    struct Joiner {     // an early error return must not leave the helper job running into freed stack variables
        pm_worker *w;
        bool pending;
        void join() { if (pending) { w->wait(); pending = false; } }
        ~Joiner() { join(); }
    } helper{&ctx->worker, false};
    // (Enqueueing [a]_1 late, next to [c]_1 after the transforms, measured neutral on one GPU: profiles/r03_a_late_msm_single_gpu_ab.txt.)
    bool a_early = aux_ctx != nullptr;
    PM_TRY(phase1_enqueue_u<C>(ctx, pk, d, ws, 1, a_early));
    if (a_early) {
        pm_ctx *aux = ctx->aux;
        PM_HIP(ctx, hipEventRecord(ctx->ev_sc_a, st));
        timing_reset_aux(ctx, aux);
        {
            helper.pending = ctx->worker.submit([&, aux] {
                if (hipSetDevice(aux->device) != hipSuccess || hipStreamWaitEvent(aux->stream, ctx->ev_sc_a, 0) != hipSuccess) {
                    st_a = PM_ERR_HIP;
                    aux->err = "helper stream setup failed";
                    return;
                }
                try {
                    st_a = msm_shard<C>(aux, pk, 0, sc_a, a_xy, a_inf);
                } catch (const std::exception &e) {   // bad_alloc in the MSM's host vectors: a status, never a terminate
                    st_a = PM_ERR_STATE;
                    aux->err = e.what();
                }
                timing_flush(aux);
            });
            if (!helper.pending) a_early = false;   // no helper thread: the two MSMs run back to back below (sc_a is already filled)
        }
    }
    PM_TRY(phase1_enqueue_rest<C>(ctx, pk, d, ws, 1, a_early ? (Fr *)nullptr : sc_a));
    // The status flags ride behind the MSMs (round 4): they land in pinned staging and are read after the MSM's own final
    // synchronisation, so the host does not wait here and the sort's fifteen launches are enqueued while the transforms still run.
    // An unsatisfied witness (prover.rs:107-108) is reported after the MSMs it no longer stops -- the rare path pays, not the proof.
    volatile unsigned *hflags_p = nullptr;
    PM_TRY(stage_flags(ctx, flags, &hflags_p));
    if (a_early) {
        const int st_c = msm_shard<C>(ctx, pk, 1, sc_c, c_xy, c_inf);
        helper.join();
        timing_absorb_aux(ctx, ctx->aux);
        // always synchronise before the staged flags are read: with both MSMs failed the copy may still be in flight
        // and the host-written 0 would read as a degree-bound violation instead of the MSMs' own status
        const hipError_t e_sync = hipStreamSynchronize(st);
        if (st_a != PM_OK && st_c != PM_OK) { ctx->err = ctx->aux->err; return st_a; }
        PM_HIP(ctx, e_sync);
        if (const int s_flags = phase1_flag_status(*hflags_p)) return s_flags;
        if (st_a != PM_OK) { ctx->err = ctx->aux->err; return st_a; }
        PM_TRY(st_c);
    } else {
        const int s_a = msm_shard<C>(ctx, pk, 0, sc_a, a_xy, a_inf);
        const int s_c = s_a == PM_OK ? msm_shard<C>(ctx, pk, 1, sc_c, c_xy, c_inf) : (int)PM_OK;
        const hipError_t e_sync = hipStreamSynchronize(st);
        PM_TRY(s_a);                                                  // an MSM's own failure first: the flags may not have landed
        PM_HIP(ctx, e_sync);
        if (const int s_flags = phase1_flag_status(*hflags_p)) return s_flags;
        PM_TRY(s_c);
    }
    timers.done();
    ctx->phase = 1;
    return PM_OK;
}

// ------------------------------------------------------------------------------- phase 2
template <class C>
int prove_phase2_impl(pm_ctx *ctx, const uint64_t *x1_in, uint64_t *u_at_x1) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    if (ctx->phase < 1 || !ctx->pk) return PM_ERR_STATE;
    const uint64_t n = ctx->pk->n;
    hipStream_t st = ctx->stream;
    Fr x1 = load_fr<P>(x1_in);
    const unsigned L = HORNER_L;
    uint64_t lanes = (n + L - 1) / L;
    unsigned blocks = nblk(lanes);
    PM_HIP(ctx, ctx->pw.part.reserve(((size_t)blocks + 1) * sizeof(Fr)));
    Fr *part = ctx->pw.part.as<Fr>();
    PM_LAUNCH(ctx, k_horner_partial<P>, dim3(blocks), dim3(256), 0, st, ctx->pw.u.as<Fr>(), n, x1, L, part);
    PM_LAUNCH(ctx, k_sum_small<P>, dim3(1), dim3(256), 0, st, part, blocks, part + blocks);
    PM_HIP(ctx, hipMemcpyAsync(u_at_x1, part + blocks, sizeof(Fr), hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    ctx->phase = 2;
    return PM_OK;
}

// ------------------------------------------------------------------------------- phase 3
template <class C>
int prove_phase3_impl(pm_ctx *ctx, const uint64_t *x1_in, const uint64_t *x2_in, const uint64_t *a_in,
                      const uint64_t *c_in, uint64_t *d_xy, int *d_inf) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    if (ctx->phase < 1 || !ctx->pk) return PM_ERR_STATE;
    const pm_pk *pk = ctx->pk;
    hipStream_t st = ctx->stream;
    PhaseTimers timers(ctx);
    const ProofShape d = proof_shape(pk);
    const uint64_t *cnt = d.cnt;
    const int levels = d.levels;
    const unsigned L = DIV_L;
    Fr x1 = load_fr<P>(x1_in), x2 = load_fr<P>(x2_in), a_at = load_fr<P>(a_in), c_at = load_fr<P>(c_in);
    Fr rah[2];
    memcpy(rah, ctx->ra_host, sizeof(rah));          // phase 1 kept the host copy of r_a: no device read-back, no synchronisation here
    NumParams np{d.n, d.sigma, d.num_len};
    const NumConsts<P> nc = make_num_consts<P>(x2, rah, a_at, c_at);
    const NumMul28<typename Radix28<P>::RR> m28 = make_num_mul28<P>(x1, nc);     // the chains' multipliers in reduced radix, internal form
    ProveWs &ws = ctx->pw;
    DivLevels<Fr> lv;
    PM_HIP(ctx, div_levels_reserve(ws, d, 1, lv));
    Fr *const *V = lv.V, *const *H = lv.H;
    PM_HIP(ctx, ws.quotient.reserve((np.len + 1) * sizeof(Fr)));
    Fr *q = ws.quotient.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    const Fr *u = ws.u.as<Fr>(), *wit_u = ws.wit_u.as<Fr>(), *u2 = ws.u2.as<Fr>();
    {
        StageTimer t(ctx, T_POLY);
        PM_HIP(ctx, hipMemsetAsync(flags, 0, 64, st));
        Fr xp[8];
        xp[0] = x1;
        for (int l = 1; l <= levels; ++l) xp[l] = pow_u64<P>(xp[l - 1], L);
        if (levels == 0) {
            // small: one lane does the whole division (q written directly)
            PM_LAUNCH(ctx, k_div_expand0<P>, dim3(1), dim3(64), 0, st, np, nc, m28, u, wit_u, u2, (unsigned)np.len, (uint64_t)1,
                           (const Fr *)nullptr, q, flags);
        } else {
            PM_LAUNCH(ctx, k_div_level0<P>, dim3(nblk(cnt[1])), dim3(256), 0, st, np, nc, m28, u, wit_u, u2, L, cnt[1], V[1]);
            for (int l = 1; l < levels; ++l) {
                PM_LAUNCH(ctx, k_div_levelN<P>, dim3(nblk(cnt[l + 1])), dim3(256), 0, st, V[l], cnt[l], xp[l], L,
                               cnt[l + 1], V[l + 1]);
            }
            PM_LAUNCH(ctx, k_div_top<P>, dim3(1), dim3(64), 0, st, V[levels], (uint64_t)0, cnt[levels], xp[levels], 1u,
                           H[levels]);
            for (int l = levels - 1; l >= 1; --l) {
                PM_LAUNCH(ctx, k_div_expandN<P>, dim3(nblk(cnt[l + 1])), dim3(256), 0, st, V[l], cnt[l], xp[l], L,
                               cnt[l + 1], H[l + 1], H[l]);
            }
            PM_LAUNCH(ctx, k_div_expand0<P>, dim3(nblk(cnt[1])), dim3(256), 0, st, np, nc, m28, u, wit_u, u2, L, cnt[1],
                           H[1], q, flags);
        }
    }
    // rem == 0 (prover.rs:221) is read after the MSM's final synchronisation: no host wait between the division and the sort
    volatile unsigned *hflags_p = nullptr;
    PM_TRY(stage_flags(ctx, flags, &hflags_p));
    const int st_d = msm_shard<C>(ctx, pk, 2, q, d_xy, d_inf);   // [d]_1 = M8, prover.rs:229
    PM_HIP(ctx, hipStreamSynchronize(st));
    if (const int s_flags = phase3_flag_status(*hflags_p)) return s_flags;
    PM_TRY(st_d);
    timers.done();
    ctx->phase = 3;
    return PM_OK;
}

#define PM_INST(C)                                                                                                     \
    template int msm_resident<C>(pm_ctx *, const pm_pk *, int, const Fp<typename C::FrP> *, uint64_t *, int *);        \
    template int msm_resident_begin<C>(pm_ctx *, const pm_pk *, int, const Fp<typename C::FrP> *, uint64_t, uint64_t);  \
    template int msm_resident_end<C>(pm_ctx *, uint64_t *, int *);                                                     \
    template int phase1_enqueue_u<C>(pm_ctx *, const pm_pk *, const ProofShape &, ProveWs &, size_t, bool);            \
    template int phase1_enqueue_rest<C>(pm_ctx *, const pm_pk *, const ProofShape &, ProveWs &, size_t, Fp<typename C::FrP> *); \
    template int prove_phase1_impl<C>(pm_ctx *, const pm_pk *, const uint64_t *, const uint64_t *, const uint64_t *,   \
                                      uint64_t *, int *, uint64_t *, int *, bool);                                         \
    template int prove_phase2_impl<C>(pm_ctx *, const uint64_t *, uint64_t *);                                         \
    template int prove_phase3_impl<C>(pm_ctx *, const uint64_t *, const uint64_t *, const uint64_t *,                  \
                                      const uint64_t *, uint64_t *, int *);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
