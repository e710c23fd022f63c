// pm_host_prove: the reference's create_proof_with_assignment glue (prover.rs:66-237) inside the library,
// for hosts that do not bring their own Transcript: the C++ host mirror (polymath_amd/host/polymath.hpp --
// transcripts of src/transcript/*.rs, challenge arithmetic of common.rs:21-98, ark wire format) driven on the
// caller's context.  The three phases stay the boundary; this is their caller, compiled once.
#include "internal.h"
#include "prove_common.cuh"
#include "divrem.cuh"
#include "../host/polymath.hpp"
#include "../host/wire.hpp"

namespace {

template <class C, class T>
int host_prove_impl(pm_ctx *ctx, const pm_pk *pk, const uint64_t *instance_host, const uint64_t *x, const uint64_t *w, int on_device,
                    const uint64_t *r_a, pm_combine_fn combine, void *user, uint8_t *proof_bytes, size_t cap, size_t *proof_len) {
    typedef pmhost::FrOps<C> F;
    typedef typename F::Fr Fr;
    pmhost::Context view(ctx, pmhost::Context::Borrow{});
    pmhost::ProvingKey<C> key;
    key.h = const_cast<pm_pk *>(pk);
    key.n = pk->n; key.m0 = pk->m0; key.sigma = pk->sigma;
    memcpy(key.omega.l, pk->omega, 32);
    std::vector<Fr> instance(pk->m0);
    memcpy((void *)instance.data(), instance_host, pk->m0 * sizeof(Fr));
    Fr ra[2];
    memcpy(ra, r_a, sizeof(ra));
    int status = PM_OK;
    pm::timing_reset(ctx);
    ctx->keep_timings = true;      // pm_last_timings then covers the whole proof
    ctx->lazy_timings = true;      // ... and reads the stage timers when asked, not between the phases
    try {
        pmhost::Polymath<C, T> pm(view);
        typename pmhost::Polymath<C, T>::Combine cb = nullptr;
        if (pk->layout == PM_SHARD_VECTOR) {
            combine = nullptr;     // the phases of a PM_SHARD_VECTOR key return points already summed over the ranks (one exchange per phase)
        } else if (!combine && pk->shard_count != 1 && ctx->comm) {   // the context's own communicator: all-gather + pm_g1_sum, no callback
            combine = [](void *user, int count, uint64_t *xy, int *inf) -> int { return pm_comm_combine_points((pm_comm *)user, C::ID, count, xy, inf); };
            user = ctx->comm;
        }
        if (combine)
            cb = [&](pmhost::G1Point<C> *pts, int count) -> int {
                uint64_t xy[2][sizeof(pm::Affine<C>) / 8];
                int inf[2];
                for (int i = 0; i < count; ++i) { memcpy(xy[i], &pts[i].p, sizeof(pm::Affine<C>)); inf[i] = pts[i].inf ? 1 : 0; }
                const int rc = combine(user, count, &xy[0][0], inf);
                for (int i = 0; i < count; ++i) { memcpy(&pts[i].p, xy[i], sizeof(pm::Affine<C>)); pts[i].inf = inf[i] != 0; }
                return rc;
            };
        pmhost::Proof<C> proof = pm.prove_raw(key, instance, x, w, on_device != 0, ra, cb);
        pmhost::Bytes b = proof.to_bytes();
        if (proof_len) *proof_len = b.size();
        if (b.size() > cap) status = PM_ERR_INVALID_ARG;
        else memcpy(proof_bytes, b.data(), b.size());
    } catch (const pmhost::PolymathError &e) {
        status = e.status ? e.status : PM_ERR_STATE;
    } catch (const std::exception &e) {
        ctx->err = e.what();
        status = PM_ERR_STATE;
    }
    ctx->keep_timings = false;
    ctx->lazy_timings = false;
    if (ctx->aux) ctx->aux->lazy_timings = false;
    key.h = nullptr;   // borrowed: the destructor must not free the caller's key
    return status;
}

}  // namespace

extern "C" int pm_host_prove_sharded(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x,
                                     const uint64_t *w, int assignment_on_device, const uint64_t *r_a, pm_combine_fn combine, void *user,
                                     uint8_t *proof_bytes, size_t capacity, size_t *proof_len) {
    if (!ctx || !pk || !instance_host || !x || !r_a || !proof_bytes || (pk->mw && !w)) return PM_ERR_INVALID_ARG;
    if (pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    if (pk->shard_count != 1 && !combine && !ctx->comm) return PM_ERR_INVALID_ARG;   // a shard's points are partial sums: somebody has to add them
    if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
    return pm::with_curve(pk->curve, [&](auto cv) {
        typedef pm::type_of<decltype(cv)> C;
        return pmhost::with_transcript<C>(transcript, [&](auto t) {
            return host_prove_impl<C, pm::type_of<decltype(t)>>(ctx, pk, instance_host, x, w, assignment_on_device, r_a, combine, user, proof_bytes,
                                                                capacity, proof_len);
        });
    });
}

// ---- PM_ASSIGNMENT_SOLVE (solve.hip): the unknown entries of the assignment are computed on the device first ----
namespace {

constexpr uint64_t NOT_STUCK = ~(uint64_t)0;

// any marker of an unknown entry (divrem.cuh: marker_byte_limbs, the one statement of the test)
inline bool is_marker(const uint64_t *fr) {
    uint32_t limbs[8];
    memcpy(limbs, fr, sizeof limbs);
    return pm::marker_byte_limbs(limbs) != 0;
}

// instance_host with its unknown entries replaced by the solved values of assignment i (tap 9): what gets hashed
void solved_instance(const pm_ctx *ctx, const pm_pk *pk, size_t i, const uint64_t *instance_host, uint64_t *out) {
    const uint64_t *solved = pm::solve_tap9_row(ctx, pk, i) + 4;
    for (size_t j = 0; j < pk->m0; ++j) memcpy(out + 4 * j, is_marker(instance_host + 4 * j) ? solved + 4 * j : instance_host + 4 * j, 32);
}

// One proof from a partial assignment: solved into the context's own row, proved from there as a device assignment.
// *stage: 0 the solver refused the structure (nothing computed), 1 the assignment is stuck, 2 the prover ran (the status is its own).
template <class C>
int host_prove_solve(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x, const uint64_t *w,
                     bool on_device, const uint64_t *r_a, uint8_t *proof_bytes, size_t cap, size_t *proof_len, int *stage) {
    *stage = 0;
    pm::timing_reset(ctx);
    {
        pm::TimingGuard timing_guard{ctx};
        PM_TRY(pm::solve_all<C>(ctx, pk, 1, x, w, on_device, 1, pm::T_WITNESS_MAP));
    }
    ctx->sv.tap10_rows = 0;     // a prove call: tap 10 belongs to the check calls
    const uint64_t stuck = pm::solve_tap9_row(ctx, pk, 0)[0];
    if (stuck != NOT_STUCK) {
        *stage = 1;
        ctx->err = "pm_host_prove: the assignment is stuck at row " + std::to_string(stuck) + " (division by zero)";
        return PM_ERR_INVALID_ARG;
    }
    *stage = 2;
    std::vector<uint64_t> inst(4 * pk->m0);
    solved_instance(ctx, pk, 0, instance_host, inst.data());
    const double solve_ms = ctx->timing_ms[pm::T_WITNESS_MAP];
    const uint64_t *xw = (const uint64_t *)ctx->sv.xw.p;
    const int rc = pmhost::with_transcript<C>(transcript, [&](auto t) {
        return host_prove_impl<C, pm::type_of<decltype(t)>>(ctx, pk, inst.data(), xw, xw + 4 * pk->m0, 1, r_a, nullptr, nullptr, proof_bytes, cap, proof_len);
    });
    ctx->timing_ms[pm::T_WITNESS_MAP] += solve_ms;   // the proof's slots start from zero; its pending timers are added when they are read
    return rc;
}

int host_prove_solve_any(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x, const uint64_t *w,
                         bool on_device, const uint64_t *r_a, uint8_t *proof_bytes, size_t cap, size_t *proof_len, int *stage) {
    *stage = 0;
    if (!ctx || !pk || !instance_host || !x || !r_a || !proof_bytes || (pk->mw && !w)) return PM_ERR_INVALID_ARG;
    if (!pmhost::transcript_ok(transcript)) return PM_ERR_INVALID_ARG;
    if (pk->shard_count != 1 || pk->layout != PM_SHARD_PAIRS || pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
    try {
        return pm::with_curve(pk->curve, [&](auto cv) {
            return host_prove_solve<pm::type_of<decltype(cv)>>(ctx, pk, transcript, instance_host, x, w, on_device, r_a, proof_bytes, cap, proof_len, stage);
        });
    } catch (const std::bad_alloc &) {
        ctx->err = "pm_host_prove: out of host memory";
        return PM_ERR_STATE;
    }
}

}  // namespace

extern "C" int pm_host_prove(pm_ctx *ctx, const pm_pk *pk, int transcript, const uint64_t *instance_host, const uint64_t *x,
                             const uint64_t *w, int assignment_on_device, const uint64_t *r_a, uint8_t *proof_bytes, size_t capacity,
                             size_t *proof_len) {
    if (!pm::assignment_flags_ok(assignment_on_device)) return PM_ERR_INVALID_ARG;
    if (pk && pk->shard_count != 1) return PM_ERR_INVALID_ARG;
    if (assignment_on_device & PM_ASSIGNMENT_SOLVE) {
        int stage = 0;
        return host_prove_solve_any(ctx, pk, transcript, instance_host, x, w, (assignment_on_device & PM_ASSIGNMENT_DEVICE) != 0, r_a, proof_bytes,
                                    capacity, proof_len, &stage);
    }
    return pm_host_prove_sharded(ctx, pk, transcript, instance_host, x, w, assignment_on_device, r_a, nullptr, nullptr, proof_bytes, capacity,
                                 proof_len);
}

// ---- pm_host_prove_batch: `count` proofs against one unsharded key, in groups whose vectors are [rows][len] arrays (prove_batch.hip) ----
namespace {

// What runs between the phases of a group: a glue provider.  after1 / after2 come after phases 1 and 2 and leave the BatchRow records
// of the next phase in the workspace; finish comes after phase 3 and writes the group's proofs and statuses.  begin: once per group,
// before phase 1 (stat / out are the group's first row's).

// The host: every phase's results come down (one synchronisation each), Polymath::glue_x1 / glue_x2 run per proof, the records go up.
template <class C, class T>
struct HostGlue {
    typedef pmhost::Polymath<C, T> PMH;
    typedef typename PMH::Fr Fr;
    typedef typename PMH::Glue Glue;
    pm_ctx *ctx;
    const pm_pk *pk;
    bool solve;
    const uint64_t *instance_host;
    size_t proof_len;
    pmhost::ProvingKey<C> key;          // n / m0 / sigma / omega carrier of the host glue: no device handle
    std::vector<pm::Affine<C>> pa, pc, pd;
    std::vector<int> ia, ic, id;
    std::vector<unsigned> flags;
    std::vector<Fr> x1, x2, a_at, c_at, u_at;
    std::vector<std::vector<Fr>> inst;
    std::vector<pmhost::Proof<C>> proof;
    std::vector<Glue> glue;
    size_t g0 = 0, rows = 0;
    const uint64_t *ra = nullptr;
    int *stat = nullptr;
    uint8_t *out = nullptr;
    HostGlue(pm_ctx *c, const pm_pk *k, int, size_t, size_t group, bool sv, const uint64_t *inst_host, size_t plen)
        : ctx(c), pk(k), solve(sv), instance_host(inst_host), proof_len(plen), pa(group), pc(group), pd(group), ia(group), ic(group), id(group),
          flags(group), x1(group), x2(group), a_at(group), c_at(group), u_at(group), inst(group, std::vector<Fr>(k->m0)), proof(group) {
        key.n = pk->n; key.m0 = pk->m0; key.sigma = pk->sigma;
        memcpy(key.omega.l, pk->omega, 32);
    }
    int start() { return PM_OK; }
    int begin(size_t first, size_t n, const uint64_t *r_a, int *status, uint8_t *proofs) {
        g0 = first; rows = n; ra = r_a; stat = status; out = proofs;
        return PM_OK;
    }
    int after1() {
        PM_TRY(pm::prove_batch_fetch1<C>(ctx, rows, pa.data(), ia.data(), pc.data(), ic.data(), flags.data()));
        const size_t m0 = pk->m0;
        glue.assign(rows, Glue());
        for (size_t b = 0; b < rows; ++b) {
            stat[b] = pm::phase1_flag_status(flags[b]);
            x1[b] = x2[b] = a_at[b] = c_at[b] = Fr::zero();     // a refused proof rides along on zeros; its results are dropped
            if (solve && pm::solve_tap9_row(ctx, pk, g0 + b)[0] != NOT_STUCK) stat[b] = PM_ERR_INVALID_ARG;   // stuck: its row holds no assignment
            if (stat[b] != PM_OK) continue;
            if (solve) solved_instance(ctx, pk, g0 + b, instance_host + 4 * m0 * (g0 + b), (uint64_t *)inst[b].data());
            else memcpy((void *)inst[b].data(), instance_host + 4 * m0 * (g0 + b), m0 * sizeof(Fr));
            proof[b].a_g1.p = pa[b]; proof[b].a_g1.inf = ia[b] != 0;
            proof[b].c_g1.p = pc[b]; proof[b].c_g1.inf = ic[b] != 0;
            PMH::glue_x1(glue[b], key, inst[b], proof[b]);
            x1[b] = glue[b].x1;
        }
        return pm::prove_batch_rows2<C>(ctx, rows, (const uint64_t *)x1.data());
    }
    int after2() {
        PM_TRY(pm::prove_batch_fetch2<C>(ctx, pk, rows, (uint64_t *)u_at.data()));
        for (size_t b = 0; b < rows; ++b) {
            if (stat[b] != PM_OK) continue;
            PMH::glue_x2(glue[b], key, inst[b], (const Fr *)(ra + 8 * b), u_at[b], proof[b]);
            x2[b] = glue[b].x2; a_at[b] = proof[b].a_at_x1; c_at[b] = glue[b].c_at_x1;
        }
        return pm::prove_batch_rows3<C>(ctx, pk, rows, ra, (const uint64_t *)x1.data(), (const uint64_t *)x2.data(), (const uint64_t *)a_at.data(),
                                        (const uint64_t *)c_at.data());
    }
    int finish() {
        PM_TRY(pm::prove_batch_fetch3<C>(ctx, rows, pd.data(), id.data(), flags.data()));
        for (size_t b = 0; b < rows; ++b) {
            uint8_t *o = out + b * proof_len;
            if (stat[b] == PM_OK) stat[b] = pm::phase3_flag_status(flags[b]);
            if (stat[b] == PM_OK) {
                proof[b].d_g1.p = pd[b]; proof[b].d_g1.inf = id[b] != 0;
                const pmhost::Bytes bytes = proof[b].to_bytes();
                if (bytes.size() == proof_len) memcpy(o, bytes.data(), proof_len);
                else stat[b] = PM_ERR_STATE;
            }
            if (stat[b] != PM_OK) memset(o, 0, proof_len);
        }
        return PM_OK;
    }
    void end(bool) {}
};

// The device (prove_glue.hip): three launches of one lane per proof; nothing comes down before finish, which makes the group's one copy
// and one synchronisation.  The stage timers stay pending (lazy_timings, as in pm_host_prove): reading them would wait for the stream.
template <class C, class T>
struct DeviceGlue {
    pm_ctx *ctx;
    const pm_pk *pk;
    int transcript;
    size_t count;
    bool solve;
    const uint64_t *instance_host;
    size_t proof_len;
    size_t g0 = 0, rows = 0;
    int *stat = nullptr;
    uint8_t *out = nullptr;
    DeviceGlue(pm_ctx *c, const pm_pk *k, int tr, size_t cnt, size_t, bool sv, const uint64_t *inst_host, size_t plen)
        : ctx(c), pk(k), transcript(tr), count(cnt), solve(sv), instance_host(inst_host), proof_len(plen) {}
    int start() {
        ctx->lazy_timings = true;
        return pm::glue_begin<C>(ctx, pk, count);
    }
    int begin(size_t first, size_t n, const uint64_t *r_a, int *status, uint8_t *proofs) {
        g0 = first; rows = n; stat = status; out = proofs;
        return pm::glue_upload<C>(ctx, pk, rows, instance_host + 4 * pk->m0 * g0, r_a, proof_len);
    }
    int after1() { return pm::glue_x1<C>(ctx, pk, transcript, rows, solve); }
    int after2() { return pm::glue_x2<C>(ctx, pk, transcript, rows, g0); }
    int finish() { return pm::glue_finish<C>(ctx, pk, rows, solve, out, proof_len, stat); }
    void end(bool ok) {
        ctx->lazy_timings = false;
        if (ok) ctx->gw.tap_rows = count;
    }
};

template <class C, class T, template <class, class> class GlueT>
int host_prove_batch_impl(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t count, const uint64_t *instance_host, const uint64_t *x,
                          const uint64_t *w, int on_device, bool solve, const uint64_t *r_a, uint8_t *proofs, size_t proof_len, int *status) {
    const size_t m0 = pk->m0, mw = pk->mw;
    size_t group = 0;
    PM_TRY(pm::prove_batch_group<C>(ctx, pk, count, &group));
    if (group == 0) {
        // one proof's [d]_1 row exceeds an MSM piece (or not even one proof fits the memory share): the per-proof path, which splits
        // its MSMs into pieces, with the host's glue whatever the caller chose; the stage times are summed over the proofs
        double sum[pm::T_NUM_SLOTS] = {0};
        size_t xs = m0, ws = mw;        // elements between consecutive x rows / w rows
        std::vector<uint64_t> solved_inst(solve ? 4 * m0 : 0);
        if (solve) {
            // the whole batch is completed first, in the check's groups, into the context's [count][m0 + mw] rows; the proofs read them there
            size_t sg = pm::msm_max_piece(ctx) / (m0 + mw);
            pm::timing_reset(ctx);
            {
                pm::TimingGuard timing_guard{ctx};
                PM_TRY(pm::solve_all<C>(ctx, pk, count, x, w, on_device != 0, sg < count ? sg : count, pm::T_WITNESS_MAP));
            }
            ctx->sv.tap10_rows = 0;
            sum[pm::T_WITNESS_MAP] = ctx->timing_ms[pm::T_WITNESS_MAP];
            x = (const uint64_t *)ctx->sv.xw.p;
            w = x + 4 * m0;
            xs = ws = m0 + mw;
            on_device = 1;
        }
        for (size_t i = 0; i < count; ++i) {
            size_t len = 0;
            uint8_t *out = proofs + i * proof_len;
            const uint64_t *inst = instance_host + 4 * m0 * i;
            if (solve && pm::solve_tap9_row(ctx, pk, i)[0] != NOT_STUCK) {
                status[i] = PM_ERR_INVALID_ARG;
                memset(out, 0, proof_len);
                continue;
            }
            if (solve) {
                solved_instance(ctx, pk, i, inst, solved_inst.data());
                inst = solved_inst.data();
            }
            status[i] = host_prove_impl<C, T>(ctx, pk, inst, x + 4 * xs * i, w ? w + 4 * ws * i : nullptr, on_device,
                                              r_a + 8 * i, nullptr, nullptr, out, proof_len, &len);
            if (status[i] == PM_OK && len != proof_len) status[i] = PM_ERR_STATE;
            if (status[i] != PM_OK) memset(out, 0, proof_len);
            if (status[i] == PM_ERR_HIP) {      // a device error is the call's, not the row's: stop, the rows not reached carry it too
                for (size_t j = i + 1; j < count; ++j) { status[j] = PM_ERR_HIP; memset(proofs + j * proof_len, 0, proof_len); }
                return PM_ERR_HIP;
            }
            pm::timing_flush_now(ctx);
            for (int s = 0; s < pm::T_NUM_SLOTS; ++s) sum[s] += ctx->timing_ms[s];
        }
        pm::timing_reset(ctx);
        for (int s = 0; s < pm::T_NUM_SLOTS; ++s) ctx->timing_ms[s] = sum[s];
        return PM_OK;
    }
    pm::timing_reset(ctx);             // the phases below add to the slots and never reset them: the sums over the batch
    pm::Fp<typename C::FrP> *gxw = nullptr;   // solve: the group's x || w rows in the prover's workspace
    const size_t n_groups = (count + group - 1) / group;
    if (solve) {
        // every assignment must mark the columns assignment 0 marks, and the structure must be solvable, before anything is computed:
        // one pass of the pattern kernel over all groups (with one group, its rows then stay where the prover reads them)
        PM_TRY(pm::solve_begin<C>(ctx, pk, count));
        PM_TRY(pm::prove_batch_xw<C>(ctx, pk, group, &gxw));
        for (size_t g0 = 0; g0 < count; g0 += group)
            PM_TRY(pm::solve_load<C>(ctx, pk, gxw, count - g0 < group ? count - g0 : group, g0, x, w, on_device != 0));
        PM_TRY(pm::solve_plan<C>(ctx, pk));
    }
    PM_TRY(pm::prove_batch_reserve<C>(ctx, pk, group));
    int rc = PM_OK;
    size_t done = 0;                   // proofs of finished groups
    try {
        GlueT<C, T> glue(ctx, pk, transcript, count, group, solve, instance_host, proof_len);
        rc = glue.start();
        // ONE loop over the groups for both providers: upload, phase 1, glue, phase 2, glue, phase 3, the proofs
        for (size_t g0 = 0; g0 < count && rc == PM_OK; g0 += group) {
            const size_t rows = count - g0 < group ? count - g0 : group;
            const uint64_t *ra = r_a + 8 * g0;
            if (solve) {
                if (n_groups > 1) rc = pm::solve_load<C>(ctx, pk, gxw, rows, g0, x, w, on_device != 0);   // (compares the rows once more: harmless)
                if (rc == PM_OK) rc = pm::solve_group<C>(ctx, pk, gxw, rows, g0, pm::T_WITNESS_MAP);
                if (rc != PM_OK) break;
            }
            if ((rc = glue.begin(g0, rows, ra, status + g0, proofs + g0 * proof_len)) != PM_OK) break;
            if ((rc = pm::prove_batch_phase1<C>(ctx, pk, rows, x + 4 * m0 * g0, w ? w + 4 * mw * g0 : nullptr, on_device != 0, ra, solve)) != PM_OK) break;
            if ((rc = glue.after1()) != PM_OK) break;
            if ((rc = pm::prove_batch_phase2<C>(ctx, pk, rows)) != PM_OK) break;
            if ((rc = glue.after2()) != PM_OK) break;
            if ((rc = pm::prove_batch_phase3<C>(ctx, pk, rows)) != PM_OK) break;
            if ((rc = glue.finish()) != PM_OK) break;
            done = g0 + rows;
        }
        glue.end(rc == PM_OK);
    } catch (const std::exception &e) {
        ctx->err = e.what();
        ctx->lazy_timings = false;
        rc = PM_ERR_STATE;
    }
    if (rc != PM_OK) (void)hipStreamSynchronize(ctx->stream);   // nothing of a failed group stays in flight behind the call
    // the call failed inside a group: that group's rows and the ones not reached carry the call's status and zeroed bytes
    for (size_t i = done; rc != PM_OK && i < count; ++i) { status[i] = rc; memset(proofs + i * proof_len, 0, proof_len); }
    return rc;
}

}  // namespace

extern "C" int pm_host_prove_batch(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t count, const uint64_t *instance_host, const uint64_t *x,
                                   const uint64_t *w, int assignment_on_device, const uint64_t *r_a, uint8_t *proofs, size_t proof_len,
                                   int *status) {
    if (!pm::assignment_flags_ok(assignment_on_device) || !ctx || !pk) return PM_ERR_INVALID_ARG;
    const bool solve = (assignment_on_device & PM_ASSIGNMENT_SOLVE) != 0;
    const int on_device = assignment_on_device & PM_ASSIGNMENT_DEVICE;
    if (transcript & ~(255 | PM_PROVE_GLUE_DEVICE)) return PM_ERR_INVALID_ARG;
    const bool device_glue = (transcript & PM_PROVE_GLUE_DEVICE) != 0;
    transcript &= 255;
    if (!pmhost::transcript_ok(transcript)) return PM_ERR_INVALID_ARG;
    if (pk->shard_count != 1 || pk->layout != PM_SHARD_PAIRS || pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    const size_t fq_bytes = pk->curve == PM_BLS12_381 ? sizeof(pm::Fp<pm::BlsFqP>) : sizeof(pm::Fp<pm::BnFqP>);
    if (proof_len != 3 * fq_bytes + 32) return PM_ERR_INVALID_ARG;     // Proof::serialize_compressed: three G1 points and one Fr
    if (count == 0) return PM_OK;
    if (!instance_host || !x || !r_a || !proofs || !status || (pk->mw && !w)) return PM_ERR_INVALID_ARG;
    if (count == 1 && solve && !device_glue) {   // as below; what the solver refuses is the CALL's status and leaves the outputs alone
        size_t len = 0;
        int stage = 0;
        const int rc = host_prove_solve_any(ctx, pk, transcript, instance_host, x, w, on_device != 0, r_a, proofs, proof_len, &len, &stage);
        if (stage == 0) return rc;
        status[0] = rc;
        if (rc != PM_OK) memset(proofs, 0, proof_len);
        return rc == PM_ERR_HIP ? (int)PM_ERR_HIP : (int)PM_OK;
    }
    if (count == 1 && !device_glue) {   // one proof: forwarded to the per-proof chain (permitted by the contract; the two routes have not been measured at B = 1)
        size_t len = 0;
        status[0] = pm_host_prove(ctx, pk, transcript, instance_host, x, w, assignment_on_device, r_a, proofs, proof_len, &len);
        if (status[0] != PM_OK) memset(proofs, 0, proof_len);
        return status[0] == PM_ERR_HIP ? (int)PM_ERR_HIP : (int)PM_OK;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
    if (device_glue) ctx->gw.tap_rows = 0;   // tap 11 is the last device-glue call's; one that falls back per proof leaves none
    return pm::with_curve(pk->curve, [&](auto cv) {
        typedef pm::type_of<decltype(cv)> C;
        return pmhost::with_transcript<C>(transcript, [&](auto t) {
            typedef pm::type_of<decltype(t)> T;
            if (device_glue)
                return host_prove_batch_impl<C, T, DeviceGlue>(ctx, pk, transcript, count, instance_host, x, w, on_device, solve, r_a, proofs, proof_len, status);
            return host_prove_batch_impl<C, T, HostGlue>(ctx, pk, transcript, count, instance_host, x, w, on_device, solve, r_a, proofs, proof_len, status);
        });
    });
}

// ---- verify (lib.rs:80-90 -> verifier.rs:19-62) and the verifying key (generator.rs:139-157): host code, no GPU --------------
namespace {

template <class C>
int make_vk_impl(uint64_t n, uint64_t m0, uint64_t sigma, const uint64_t *omega, const uint64_t *x_trap, const uint64_t *z_trap, uint8_t *out,
                 size_t cap, size_t *len) {
    typedef typename pmhost::FrOps<C>::Fr Fr;
    pmhost::ProvingKey<C> shape;           // carries n / m0 / sigma / omega only (no device handle)
    shape.n = n; shape.m0 = m0; shape.sigma = sigma;
    memcpy(shape.omega.l, omega, 32);
    Fr x, z;
    memcpy(x.l, x_trap, 32);
    memcpy(z.l, z_trap, 32);
    const pmhost::VerifyingKeyT<C> vk = pmhost::Polymath<C, pmhost::MerlinFieldTranscript<C>>::make_vk(shape, x, z);
    pmhost::Bytes b;
    pmhost::ser_vk_c<C>(vk, b);
    if (len) *len = b.size();
    if (b.size() > cap) return PM_ERR_INVALID_ARG;
    memcpy(out, b.data(), b.size());
    return PM_OK;
}

template <class C, class T>
int verify_impl(const uint8_t *vk_bytes, size_t vk_len, const uint64_t *inputs, size_t n_inputs, const uint8_t *proof_bytes, size_t proof_len,
                int *accepted) {
    typedef typename pmhost::FrOps<C>::Fr Fr;
    const pmhost::VerifyingKeyT<C> vk = pmhost::read_vk_exact<C>(vk_bytes, vk_len);
    const pmhost::Proof<C> proof = pmhost::read_proof<C>(proof_bytes, proof_len);
    std::vector<Fr> pub(n_inputs);
    if (n_inputs) memcpy((void *)pub.data(), inputs, n_inputs * sizeof(Fr));
    *accepted = pmhost::Polymath<C, T>::verify(vk, pub, proof) ? 1 : 0;
    return PM_OK;
}

}  // namespace

extern "C" int pm_host_make_vk(int curve, uint64_t n, uint64_t m0, uint64_t sigma, const uint64_t *omega, const uint64_t *x_trapdoor,
                               const uint64_t *z_trapdoor, uint8_t *vk_bytes, size_t capacity, size_t *vk_len) {
    if (!omega || !x_trapdoor || !z_trapdoor || !vk_bytes) return PM_ERR_INVALID_ARG;
    try {
        return pm::with_curve(curve, [&](auto cv) {
            return make_vk_impl<pm::type_of<decltype(cv)>>(n, m0, sigma, omega, x_trapdoor, z_trapdoor, vk_bytes, capacity, vk_len);
        });
    } catch (const std::exception &) {
        return PM_ERR_STATE;
    }
}

extern "C" int pm_host_verify(int curve, int transcript, const uint8_t *vk_bytes, size_t vk_len, const uint64_t *public_inputs, size_t n_inputs,
                              const uint8_t *proof_bytes, size_t proof_len, int *accepted) {
    if (!vk_bytes || !proof_bytes || !accepted || (n_inputs && !public_inputs)) return PM_ERR_INVALID_ARG;
    *accepted = 0;
    try {
        return pm::with_curve(curve, [&](auto cv) {
            typedef pm::type_of<decltype(cv)> C;
            return pmhost::with_transcript<C>(transcript, [&](auto t) {
                return verify_impl<C, pm::type_of<decltype(t)>>(vk_bytes, vk_len, public_inputs, n_inputs, proof_bytes, proof_len, accepted);
            });
        });
    } catch (const std::exception &) {      // malformed vk / proof bytes (off-curve points, non-canonical scalars, truncation)
        return PM_ERR_INVALID_ARG;
    }
}
