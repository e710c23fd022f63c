// pm_host_prove_batch, device side: the three phases of prove.hip over a GROUP of proofs against one unsharded key.  Every vector of
// prove.hip is a [rows][len] array here -- the same ProveWs type, the context's second instance `pb`, so that a proof in flight in `pw`
// is left alone -- every kernel has the proof as grid y, and the three MSMs of a proof become three msm_run_batch calls per group: row b
// of the [a] / [c] / [d] scalar matrices is proof b's scalar vector, laid out at the stride msm_run_batch reads (the MSM's pair count).
//
// The kernels are prove_kernels.cuh's, the ones prove.hip launches for one proof, and phase 1 between the uploads and the MSMs is
// prove.hip's phase1_enqueue_u / phase1_enqueue_rest with rows = the group.  r_a goes up as a [rows][2] array; what else differs
// from proof to proof (x1, the numerator's constants and reduced-radix multipliers, the division's level multipliers) is one BatchRow
// record per proof in device memory (batch_row.cuh), written once per phase and indexed by blockIdx.y.  Each proof has its own flag word.
// A proof whose witness fails a check keeps running (every operation is defined on any field values); its result is dropped.
//
// The phases only enqueue.  Who writes the records and reads the results between them is the caller's glue provider (internal.h): the
// host, through the fetch / rows functions at the end of this file, or the kernels of prove_glue.hip, which leave the stream alone.
#include <cstring>

#include "internal.h"
#include "fq28.cuh"
#include "prove_common.cuh"
#include "prove_kernels.cuh"

namespace pm {

// ------------------------------------------------------------------------------- host side
namespace {

// the key's MSM ranges are the scalar rows this file writes
bool layout_ok(const pm_pk *pk, const ProofShape &d) {
    const uint64_t len[3] = {d.len_a, d.len_c, d.len_d};
    for (int k = 0; k < 3; ++k)   // one piece per MSM: all of its range
        if (pk->pieces[k].size() != 1 || pk->pieces[k][0].cat_lo != pk->msm_lo[k] || pk->pieces[k][0].count != len[k]) return false;
    return pk->whole_resident();
}

// Fr elements of the group's vectors per proof (pm_ctx::pb and the transforms' out-of-place temporary)
uint64_t row_elems(const ProofShape &d) {
    uint64_t e = (d.m0 + d.mw) + 7 * d.n + 2 * d.n + d.len_a + d.len_c + (d.num_len + 1) + (d.n / (HORNER_L * 256) + 2);
    for (int l = 1; l <= d.levels; ++l) e += 2 * d.cnt[l] + 2;
    return e;
}

}  // namespace

// Group size.  (1) rows * len_d <= msm_max_piece: the [d] batch of a group is one bucket pipeline (msm_run_batch splits further where its
// own grid limits ask for it).  (2) HBM: a group may take HALF of what is free (plus what pm_ctx::pb already holds, which is reused):
// the other half is the caller's -- a second context, the verifier's batch, the next key.  Per proof: the vectors (row_elems: about 23 n Fr) and
// the batched MSM's workspace for its longest row, estimated as 16 bytes per (window, pair) for digits, sorted entries and task
// descriptors plus one XYZZ partial and 16 bytes of counters per bucket.
template <class C>
int prove_batch_group(pm_ctx *ctx, const pm_pk *pk, size_t count, size_t *group) {
    typedef Fp<typename C::FrP> Fr;
    *group = 0;
    const ProofShape d = proof_shape(pk);
    const size_t max_piece = msm_max_piece(ctx);
    if (!layout_ok(pk, d) || d.len_d > max_piece) return PM_OK;
    size_t g = max_piece / d.len_d;
    if (g > 65535) g = 65535;                       // grid y
    size_t free_b = 0, total_b = 0;
    PM_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t held = ctx->pb.bytes_held();
    unsigned nwin = 0, c = 0;
    msm_plan_query((size_t)d.len_d, (unsigned)C::FrP::BITS, &nwin, &c);
    const size_t per_row = row_elems(d) * sizeof(Fr) + (size_t)nwin * d.len_d * 16 +
                           (size_t)nwin * ((size_t)1 << (c ? c - 1 : 0)) * (sizeof(XYZZ<C>) + 16);
    const size_t fit = ((free_b + held) / 2) / per_row;
    if (g > fit) g = fit;
    if (g > count) g = count;
    *group = g;                                     // 0: not even one proof fits the share -- the per-proof path has the smaller footprint
    return PM_OK;
}

// the records go up from the context's own staging: the copy is only enqueued, and the staging outlives it (its next writer comes
// after the phase's synchronisation)
template <class P>
static BatchRow<P> *stage_rows(pm_ctx *ctx, size_t rows) {
    ctx->gw.rows_host.assign(rows * sizeof(BatchRow<P>), 0);
    return (BatchRow<P> *)ctx->gw.rows_host.data();
}
static int upload_rows(pm_ctx *ctx) {
    PM_HIP(ctx, ctx->pb.rows.reserve(ctx->gw.rows_host.size()));
    PM_HIP(ctx, hipMemcpyAsync(ctx->pb.rows.p, ctx->gw.rows_host.data(), ctx->gw.rows_host.size(), hipMemcpyHostToDevice, ctx->stream));
    return PM_OK;
}

template <class C>
int prove_batch_xw(pm_ctx *ctx, const pm_pk *pk, size_t rows, Fp<typename C::FrP> **xw) {
    PM_HIP(ctx, ctx->pb.xw.reserve(rows * (pk->m0 + pk->mw) * sizeof(Fp<typename C::FrP>)));
    *xw = ctx->pb.xw.as<Fp<typename C::FrP>>();
    return PM_OK;
}

// What the glue provider touches between the phases, sized for groups of up to `rows` proofs before the first of them starts: the
// BatchRow records (phase 1 keeps r_a at their place), the flag words, phase 2's sums, the three arrays of point records.
template <class C>
int prove_batch_reserve(pm_ctx *ctx, const pm_pk *pk, size_t rows) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const ProofShape d = proof_shape(pk);
    if (rows == 0 || rows > 65535) return PM_ERR_INVALID_ARG;
    ProveWs &ws = ctx->pb;
    PM_HIP(ctx, ws.rows.reserve(rows * sizeof(BatchRow<P>)));          // > rows * 2 * sizeof(Fr)
    PM_HIP(ctx, ws.flags.reserve(rows * sizeof(unsigned)));
    PM_HIP(ctx, ws.part.reserve(rows * ((size_t)nblk((d.n + HORNER_L - 1) / HORNER_L) + 1) * sizeof(Fr)));
    PM_HIP(ctx, ctx->gw.pts.reserve(3 * rows * sizeof(BatchPoint<C>)));   // (a record's size is the curve's: the stride is set per call)
    ctx->gw.cap = rows;
    return PM_OK;
}

template <class C>
static BatchPoint<C> *batch_points(pm_ctx *ctx, int which) { return ctx->gw.pts.as<BatchPoint<C>>() + (size_t)which * ctx->gw.cap; }

// xw_resident: the group's x || w rows are already in the workspace (prove_batch_xw: the witness solver completed them there);
// x and w are then not read
template <class C>
int prove_batch_phase1(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *x, const uint64_t *w, bool assignment_on_device,
                       const uint64_t *r_a, bool xw_resident) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const ProofShape d = proof_shape(pk);
    if (!layout_ok(pk, d) || rows == 0 || rows > 65535 || rows > ctx->gw.cap) return PM_ERR_INVALID_ARG;
    if (pk->log_n + 1 > (unsigned)C::TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;  // prover.rs:317
    const uint64_t n = d.n, m0 = d.m0, mw = d.mw, len_a = d.len_a, len_c = d.len_c;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    StageTimer t_phase(ctx, T_PHASE);
    ProveWs &ws = ctx->pb;
    PM_HIP(ctx, ws.xw.reserve(rows * (m0 + mw) * sizeof(Fr)));
    for (DevBuf *b : {&ws.ue, &ws.we, &ws.u, &ws.w, &ws.wit_u, &ws.tmp}) PM_HIP(ctx, b->reserve(rows * n * sizeof(Fr)));
    PM_HIP(ctx, ws.u2.reserve(rows * 2 * n * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_c.reserve(rows * len_c * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_a.reserve(rows * len_a * sizeof(Fr)));
    Fr *xw = ws.xw.as<Fr>(), *sc_c = ws.sc_c.as<Fr>(), *sc_a = ws.sc_a.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    PM_HIP(ctx, hipMemsetAsync(flags, 0, rows * sizeof(unsigned), st));
    const hipMemcpyKind kind = assignment_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // rows of x (m0) and of w (mw) interleave into rows of x || w
    if (!xw_resident) {
        PM_HIP(ctx, hipMemcpy2DAsync(xw, (m0 + mw) * sizeof(Fr), x, m0 * sizeof(Fr), m0 * sizeof(Fr), rows, kind, st));
        if (mw) PM_HIP(ctx, hipMemcpy2DAsync(xw + m0, (m0 + mw) * sizeof(Fr), w, mw * sizeof(Fr), mw * sizeof(Fr), rows, kind, st));
    }
    // this phase's per-proof values are r_a alone: [rows][2] where the later phases keep their records
    PM_HIP(ctx, hipMemcpyAsync(ws.rows.p, r_a, rows * 2 * sizeof(Fr), hipMemcpyHostToDevice, st));
    PM_TRY(phase1_enqueue_u<C>(ctx, pk, d, ws, rows, true));
    PM_TRY(phase1_enqueue_rest<C>(ctx, pk, d, ws, rows, (Fr *)nullptr));
    // [a]_1 and [c]_1 of every proof of the group: two batches over the key's PLAIN points (no tables, no wide plan)
    const Affine<C> *bases = (const Affine<C> *)pk->d_bases;
    PM_TRY(msm_run_batch_device<C>(ctx, bases + pk->res_dev_off[0], sc_a, (size_t)len_a, rows, batch_points<C>(ctx, 0)));
    PM_TRY(msm_run_batch_device<C>(ctx, bases + pk->res_dev_off[1], sc_c, (size_t)len_c, rows, batch_points<C>(ctx, 1)));
    return PM_OK;
}

template <class C>
const Fp<typename C::FrP> *prove_batch_sums(pm_ctx *ctx, const pm_pk *pk, size_t rows) {
    const ProofShape d = proof_shape(pk);
    return ctx->pb.part.as<Fp<typename C::FrP>>() + rows * nblk((d.n + HORNER_L - 1) / HORNER_L);
}

template <class C>
int prove_batch_phase2(pm_ctx *ctx, const pm_pk *pk, size_t rows) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const ProofShape d = proof_shape(pk);
    if (rows == 0 || rows > 65535) return PM_ERR_INVALID_ARG;
    hipStream_t st = ctx->stream;
    ProveWs &ws = ctx->pb;
    const uint64_t lanes = (d.n + HORNER_L - 1) / HORNER_L;
    const unsigned blocks = nblk(lanes);
    PM_HIP(ctx, ws.part.reserve(rows * ((size_t)blocks + 1) * sizeof(Fr)));
    Fr *part = ws.part.as<Fr>(), *sums = part + rows * blocks;
    PM_LAUNCH(ctx, k_horner_partial_rows<P>, dim3(blocks, (unsigned)rows), dim3(256), 0, st, ws.u.as<Fr>(), d.n, ws.rows.as<BatchRow<P>>(), HORNER_L, part);
    PM_LAUNCH(ctx, k_sum_small<P>, dim3((unsigned)rows), dim3(256), 0, st, part, blocks, sums);
    return PM_OK;
}

template <class C>
int prove_batch_phase3(pm_ctx *ctx, const pm_pk *pk, size_t rows) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const ProofShape d = proof_shape(pk);
    if (!layout_ok(pk, d) || rows == 0 || rows > 65535 || rows > ctx->gw.cap) return PM_ERR_INVALID_ARG;
    const unsigned gy = (unsigned)rows, L = DIV_L;
    const int levels = d.levels;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    StageTimer t_phase(ctx, T_PHASE);
    ProveWs &ws = ctx->pb;
    NumParams np{d.n, d.sigma, d.num_len};
    const BatchRow<P> *drows = ws.rows.as<BatchRow<P>>();
    DivLevels<Fr> lv;
    PM_HIP(ctx, div_levels_reserve(ws, d, rows, lv));
    Fr *const *V = lv.V, *const *H = lv.H;
    const uint64_t *vs = lv.vs;
    PM_HIP(ctx, ws.quotient.reserve((rows * d.len_d + 2) * sizeof(Fr)));
    Fr *q = ws.quotient.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    const Fr *u = ws.u.as<Fr>(), *wit_u = ws.wit_u.as<Fr>(), *u2 = ws.u2.as<Fr>();
    {
        StageTimer t(ctx, T_POLY);
        if (levels == 0) {   // small: one lane per proof does the whole division
            PM_LAUNCH(ctx, k_div_expand0_rows<P>, dim3(1, gy), dim3(64), 0, st, np, drows, u, wit_u, u2, (unsigned)np.len, (uint64_t)1,
                           (const Fr *)nullptr, (uint64_t)0, q, d.len_d, flags);
        } else {
            PM_LAUNCH(ctx, k_div_level0_rows<P>, dim3(nblk(d.cnt[1]), gy), dim3(256), 0, st, np, drows, u, wit_u, u2, L, d.cnt[1], V[1], vs[1]);
            for (int l = 1; l < levels; ++l) {
                PM_LAUNCH(ctx, k_div_levelN_rows<P>, dim3(nblk(d.cnt[l + 1]), gy), dim3(256), 0, st, V[l], vs[l], d.cnt[l], drows, l, L, d.cnt[l + 1],
                               V[l + 1], vs[l + 1]);
            }
            PM_LAUNCH(ctx, k_div_top_rows<P>, dim3(nblk(rows, 64)), dim3(64), 0, st, V[levels], vs[levels], d.cnt[levels], drows, levels, gy,
                           H[levels]);
            for (int l = levels - 1; l >= 1; --l) {
                PM_LAUNCH(ctx, k_div_expandN_rows<P>, dim3(nblk(d.cnt[l + 1]), gy), dim3(256), 0, st, V[l], vs[l], d.cnt[l], drows, l, L, d.cnt[l + 1],
                               H[l + 1], vs[l + 1], H[l]);
            }
            PM_LAUNCH(ctx, k_div_expand0_rows<P>, dim3(nblk(d.cnt[1]), gy), dim3(256), 0, st, np, drows, u, wit_u, u2, L, d.cnt[1], H[1], vs[1], q,
                           d.len_d, flags);
        }
    }
    return msm_run_batch_device<C>(ctx, (const Affine<C> *)pk->d_bases + pk->res_dev_off[2], q, (size_t)d.len_d, rows, batch_points<C>(ctx, 2));   // [d]_1 = M8
}

// ------------------------------------------------------------------------------- the host as glue provider
// `n_pts` arrays of point records starting with array `first`, and the flag words: enqueued copies, then the phase's synchronisation
template <class C>
static int fetch_points(pm_ctx *ctx, size_t rows, int first, int n_pts, Affine<C> *const *pt, int *const *inf, unsigned *flags_out) {
    std::vector<BatchPoint<C>> res((size_t)n_pts * rows);
    for (int k = 0; k < n_pts; ++k)
        PM_HIP(ctx, hipMemcpyAsync(res.data() + k * rows, batch_points<C>(ctx, first + k), rows * sizeof(BatchPoint<C>), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipMemcpyAsync(flags_out, ctx->pb.flags.p, rows * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_pts; ++k)
        for (size_t r = 0; r < rows; ++r) { pt[k][r] = res[k * rows + r].p; inf[k][r] = (int)res[k * rows + r].inf; }
    return PM_OK;
}

template <class C>
int prove_batch_fetch1(pm_ctx *ctx, size_t rows, Affine<C> *a, int *a_inf, Affine<C> *c, int *c_inf, unsigned *flags_out) {
    Affine<C> *const pt[2] = {a, c};
    int *const inf[2] = {a_inf, c_inf};
    return fetch_points<C>(ctx, rows, 0, 2, pt, inf, flags_out);
}

template <class C>
int prove_batch_fetch3(pm_ctx *ctx, size_t rows, Affine<C> *dpt, int *d_inf, unsigned *flags_out) {
    return fetch_points<C>(ctx, rows, 2, 1, &dpt, &d_inf, flags_out);
}

template <class C>
int prove_batch_rows2(pm_ctx *ctx, size_t rows, const uint64_t *x1) {
    typedef typename C::FrP P;
    BatchRow<P> *par = stage_rows<P>(ctx, rows);
    for (size_t b = 0; b < rows; ++b) par[b].x1 = load_fr<P>(x1 + 4 * b);
    return upload_rows(ctx);
}

template <class C>
int prove_batch_fetch2(pm_ctx *ctx, const pm_pk *pk, size_t rows, uint64_t *u_at_x1) {
    typedef Fp<typename C::FrP> Fr;
    PM_HIP(ctx, hipMemcpyAsync(u_at_x1, prove_batch_sums<C>(ctx, pk, rows), rows * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

template <class C>
int prove_batch_rows3(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *r_a, const uint64_t *x1_in, const uint64_t *x2_in,
                      const uint64_t *a_in, const uint64_t *c_in) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const int levels = proof_shape(pk).levels;
    BatchRow<P> *par = stage_rows<P>(ctx, rows);
    for (size_t b = 0; b < rows; ++b) {
        const Fr ra[2] = {load_fr<P>(r_a + 8 * b), load_fr<P>(r_a + 8 * b + 4)};
        fill_batch_row<P>(par[b], load_fr<P>(x1_in + 4 * b), load_fr<P>(x2_in + 4 * b), ra, load_fr<P>(a_in + 4 * b), load_fr<P>(c_in + 4 * b), levels);
    }
    return upload_rows(ctx);
}

#define PM_INST(C)                                                                                                                          \
    template int prove_batch_group<C>(pm_ctx *, const pm_pk *, size_t, size_t *);                                                           \
    template int prove_batch_xw<C>(pm_ctx *, const pm_pk *, size_t, Fp<typename C::FrP> **);                                                \
    template int prove_batch_reserve<C>(pm_ctx *, const pm_pk *, size_t);                                                                   \
    template int prove_batch_phase1<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, bool, const uint64_t *, bool);  \
    template int prove_batch_phase2<C>(pm_ctx *, const pm_pk *, size_t);                                                                    \
    template int prove_batch_phase3<C>(pm_ctx *, const pm_pk *, size_t);                                                                    \
    template const Fp<typename C::FrP> *prove_batch_sums<C>(pm_ctx *, const pm_pk *, size_t);                                               \
    template int prove_batch_fetch1<C>(pm_ctx *, size_t, Affine<C> *, int *, Affine<C> *, int *, unsigned *);                               \
    template int prove_batch_rows2<C>(pm_ctx *, size_t, const uint64_t *);                                                                  \
    template int prove_batch_fetch2<C>(pm_ctx *, const pm_pk *, size_t, uint64_t *);                                                        \
    template int prove_batch_rows3<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, const uint64_t *,               \
                                      const uint64_t *, const uint64_t *);                                                                  \
    template int prove_batch_fetch3<C>(pm_ctx *, size_t, Affine<C> *, int *, unsigned *);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
