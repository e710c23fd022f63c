// pm_host_prove_batch with PM_PROVE_GLUE_DEVICE: what the host does between the phases of a group of proofs -- Polymath::glue_x1,
// glue_x2 and Proof::to_bytes of host/polymath.hpp (prover.rs:125-138, 189, 231-236) -- as three kernels with ONE LANE PER PROOF, so
// that a group runs from its uploads to its proof bytes without the host: the phases of prove_batch.hip read the BatchRow records these
// kernels write, and the kernels read the phases' results where they lie (the flag words, the (point, flag) records of the batched
// MSMs, phase 2's sums).  The arithmetic is transcript.cuh's fs_prover_x1 / fs_prover_x2, batch_row.cuh's fill_batch_row and
// g1_record.cuh's g1_record_words: PM_HD code that tests/native/prover_glue_selftest.cpp compares with the host's on the CPU.
//
// These are cold, branchy kernels like k_verifier_challenges (challenges.hip): plain C++, the sponge in per-lane private memory, no
// LDS.  A refused proof (a phase-1 flag, or a stuck row under PM_ASSIGNMENT_SOLVE) rides along on zero challenges, as in host mode.
#include <cstring>

#include "internal.h"
#include "g1_record.cuh"
#include "prove_common.cuh"
#include "divrem.cuh"
#include "transcript.cuh"

namespace pm {

namespace {

constexpr unsigned GLUE_BLOCK = 256;
constexpr unsigned long long GLUE_NOT_STUCK = ~0ull;   // solve.hip: the stuck word of a row that completed

// from k_glue_x1 to k_glue_x2: the transcript after x1, x1 and the powers of y1; live = the proof is still in the running
template <class C, int KIND>
struct GlueKeep {
    fs::FsProverState<C, KIND> s;
    uint32_t live;
};

template <class C>
struct GlueRows {
    unsigned rows;
    uint64_t m0;
    const unsigned *flags;                  // the proofs' flag words (prove.hip: k_check_sap)
    const unsigned long long *stuck;        // under PM_ASSIGNMENT_SOLVE: the solver's stuck words; else null
    Fp<typename C::FrP> *inst;              // [rows][m0]
    const Fp<typename C::FrP> *ra;          // [rows][2]
    BatchRow<typename C::FrP> *brow;        // pm_ctx::pb.rows
    uint8_t *out;                           // [rows][proof_len], then one status word per row
    unsigned proof_len;
};

template <class C>
__device__ __forceinline__ bool glue_row_live(const GlueRows<C> &g, unsigned i) {
    return phase1_flag_status(g.flags[i]) == PM_OK && !(g.stuck && g.stuck[i] != GLUE_NOT_STUCK);
}

// any marker of an unknown entry (include/polymath_hip.h: PM_ASSIGNMENT_SOLVE; divrem.cuh: marker_byte, the one statement of the test)
template <class P>
__device__ __forceinline__ bool glue_is_marker(const Fp<P> &v) {
    return marker_byte<P>(v) != 0;
}

// After phase 1.  xw: under PM_ASSIGNMENT_SOLVE the group's completed x || w rows (stride ncols), whose first m0 entries replace the
// marker entries of the instance; else null.
template <class C, int KIND>
__global__ __launch_bounds__(GLUE_BLOCK) void k_glue_x1(fs::FsVk<C> vk, GlueRows<C> g, const BatchPoint<C> *pa, const BatchPoint<C> *pc,
                                                        const Fp<typename C::FrP> *xw, uint64_t ncols, GlueKeep<C, KIND> *keep) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    constexpr int NW = C::FqP::N;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.rows) return;
    GlueKeep<C, KIND> K;
    memset((void *)&K, 0, sizeof(K));
    BatchRow<P> R;
    memset((void *)&R, 0, sizeof(R));
    if (glue_row_live<C>(g, i)) {
        K.live = 1u;
        Fr *inst = g.inst + (size_t)i * g.m0;
        if (xw)
            for (uint64_t j = 0; j < g.m0; ++j)
                if (glue_is_marker<P>(inst[j])) inst[j] = xw[(size_t)i * ncols + j];
        uint32_t rec[2][NW];
        g1_record_words<C>(pa[i].p, pa[i].inf != 0, rec[0]);
        g1_record_words<C>(pc[i].p, pc[i].inf != 0, rec[1]);
        uint32_t *out = (uint32_t *)(g.out + (size_t)i * g.proof_len);     // a_g1 | c_g1 | ...
        for (int k = 0; k < NW; ++k) { out[k] = rec[0][k]; out[NW + k] = rec[1][k]; }
        fs::fs_prover_x1<C, KIND>(vk, inst, (size_t)g.m0, (const uint8_t *)rec[0], (const uint8_t *)rec[1], &K.s);
        R.x1 = K.s.x1;
    }
    keep[i] = K;
    g.brow[i] = R;
}

// After phase 2.  sums[i] = u(x1) of row i; tap: four elements per proof (x1, x2, a(x1), c(x1)), this group's first
template <class C, int KIND>
__global__ __launch_bounds__(GLUE_BLOCK) void k_glue_x2(fs::FsVk<C> vk, GlueRows<C> g, const Fp<typename C::FrP> *sums, int levels,
                                                        const GlueKeep<C, KIND> *keep, Fp<typename C::FrP> *tap) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    constexpr int NW = C::FqP::N;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.rows) return;
    Fr x1 = Fr::zero(), x2 = Fr::zero(), a_at = Fr::zero(), c_at = Fr::zero();
    const Fr ra[2] = {g.ra[2 * (size_t)i], g.ra[2 * (size_t)i + 1]};
    if (keep[i].live) {
        GlueKeep<C, KIND> K = keep[i];
        fs::FsProverOut<C> o;
        fs::fs_prover_x2<C, KIND>(vk, g.inst + (size_t)i * g.m0, (size_t)g.m0, &K.s, sums[i], ra, &o);
        x1 = K.s.x1; x2 = o.x2; a_at = o.a_at_x1; c_at = o.c_at_x1;
        uint64_t w[4];
        fs::fr_canonical_words<C>(a_at, w);
        uint32_t *out = (uint32_t *)(g.out + (size_t)i * g.proof_len) + 2 * NW;   // ... | a_at_x1 | ...
        for (int k = 0; k < 4; ++k) { out[2 * k] = (uint32_t)w[k]; out[2 * k + 1] = (uint32_t)(w[k] >> 32); }
    }
    BatchRow<P> R;
    memset((void *)&R, 0, sizeof(R));
    fill_batch_row<P>(R, x1, x2, ra, a_at, c_at, levels);
    g.brow[i] = R;
    tap[4 * (size_t)i] = x1;
    tap[4 * (size_t)i + 1] = x2;
    tap[4 * (size_t)i + 2] = a_at;
    tap[4 * (size_t)i + 3] = c_at;
}

// After phase 3: ... | d_g1, the proof's status from its flag word and stuck word, zeroed bytes where it is not PM_OK
template <class C>
__global__ __launch_bounds__(GLUE_BLOCK) void k_proof_bytes(GlueRows<C> g, const BatchPoint<C> *pd) {
    constexpr int NW = C::FqP::N;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.rows) return;
    const unsigned f = g.flags[i];
    int st = phase1_flag_status(f);
    if (g.stuck && g.stuck[i] != GLUE_NOT_STUCK) st = PM_ERR_INVALID_ARG;
    if (st == PM_OK) st = phase3_flag_status(f);
    uint32_t *out = (uint32_t *)(g.out + (size_t)i * g.proof_len);
    if (st == PM_OK) {
        uint32_t rec[NW];
        g1_record_words<C>(pd[i].p, pd[i].inf != 0, rec);
        for (int k = 0; k < NW; ++k) out[2 * NW + 8 + k] = rec[k];
    } else {
        for (unsigned k = 0; k < g.proof_len / 4; ++k) out[k] = 0u;
    }
    ((int *)(g.out + (size_t)g.rows * g.proof_len))[i] = st;
}

template <class C>
fs::FsVk<C> glue_vk(const pm_pk *pk) {
    typedef typename C::FrP P;
    fs::FsVk<C> vk;
    vk.n = pk->n;
    vk.sigma = pk->sigma;
    memcpy(vk.omega.l, pk->omega, 32);
    vk.n_inv = inverse<P>(from_u64<P>(pk->n));   // compute_pi_at_x1's F::inv(F::from_u64(pk.n)), once per launch
    return vk;
}

template <class C>
GlueRows<C> glue_rows(pm_ctx *ctx, const pm_pk *pk, size_t rows, bool solve, size_t proof_len) {
    typedef typename C::FrP P;
    GlueRows<C> g;
    g.rows = (unsigned)rows;
    g.m0 = pk->m0;
    g.flags = ctx->pb.flags.as<unsigned>();
    g.stuck = solve ? ctx->sv.stuck.as<unsigned long long>() : nullptr;
    g.inst = ctx->gw.inst.as<Fp<P>>();
    g.ra = ctx->gw.ra.as<Fp<P>>();
    g.brow = ctx->pb.rows.as<BatchRow<P>>();
    g.out = ctx->gw.out.as<uint8_t>();
    g.proof_len = (unsigned)proof_len;
    return g;
}

template <class C>
size_t glue_proof_len() { return 3 * 4 * (size_t)C::FqP::N + 32; }

template <class C, int KIND>
int launch_x1(pm_ctx *ctx, const pm_pk *pk, size_t rows, bool solve) {
    typedef Fp<typename C::FrP> Fr;
    const BatchPoint<C> *pts = ctx->gw.pts.as<BatchPoint<C>>();
    StageTimer t(ctx, T_POLY);
    PM_LAUNCH(ctx, (k_glue_x1<C, KIND>), dim3(nblk(rows, GLUE_BLOCK)), dim3(GLUE_BLOCK), 0, ctx->stream, glue_vk<C>(pk),
                   glue_rows<C>(ctx, pk, rows, solve, glue_proof_len<C>()), pts, pts + ctx->gw.cap, solve ? ctx->pb.xw.as<Fr>() : (const Fr *)nullptr,
                   (uint64_t)(pk->m0 + pk->mw), ctx->gw.keep.as<GlueKeep<C, KIND>>());
    return PM_OK;
}

template <class C, int KIND>
int launch_x2(pm_ctx *ctx, const pm_pk *pk, size_t rows, size_t g0) {
    typedef Fp<typename C::FrP> Fr;
    StageTimer t(ctx, T_POLY);
    PM_LAUNCH(ctx, (k_glue_x2<C, KIND>), dim3(nblk(rows, GLUE_BLOCK)), dim3(GLUE_BLOCK), 0, ctx->stream, glue_vk<C>(pk),
                   glue_rows<C>(ctx, pk, rows, false, glue_proof_len<C>()), prove_batch_sums<C>(ctx, pk, rows), proof_shape(pk).levels,
                   ctx->gw.keep.as<GlueKeep<C, KIND>>(), ctx->gw.tap.as<Fr>() + 4 * g0);
    return PM_OK;
}

}  // namespace

template <class C>
int glue_begin(pm_ctx *ctx, const pm_pk *pk, size_t count) {
    (void)pk;
    ctx->gw.tap_rows = 0;
    PM_HIP(ctx, ctx->gw.tap.reserve(count * 4 * sizeof(Fp<typename C::FrP>)));
    return PM_OK;
}

template <class C>
int glue_upload(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *instance_host, const uint64_t *r_a, size_t proof_len) {
    typedef Fp<typename C::FrP> Fr;
    if (rows == 0 || rows > ctx->gw.cap || proof_len != glue_proof_len<C>()) return PM_ERR_INVALID_ARG;
    GlueWs &gw = ctx->gw;
    PM_HIP(ctx, gw.inst.reserve(rows * pk->m0 * sizeof(Fr)));
    PM_HIP(ctx, gw.ra.reserve(rows * 2 * sizeof(Fr)));
    PM_HIP(ctx, gw.keep.reserve(rows * sizeof(GlueKeep<C, fs::KIND_BLAKE3>)));    // the largest of the three
    PM_HIP(ctx, gw.out.reserve(rows * (proof_len + sizeof(int))));
    PM_HIP(ctx, hipMemcpyAsync(gw.inst.p, instance_host, rows * pk->m0 * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    PM_HIP(ctx, hipMemcpyAsync(gw.ra.p, r_a, rows * 2 * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return PM_OK;
}

template <class C>
int glue_x1(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t rows, bool solve) {
    static_assert(sizeof(GlueKeep<C, fs::KIND_BLAKE3>) >= sizeof(GlueKeep<C, fs::KIND_MERLIN>) &&
                  sizeof(GlueKeep<C, fs::KIND_BLAKE3>) >= sizeof(GlueKeep<C, fs::KIND_KECCAK256>), "glue_upload reserves the BLAKE3 record");
    switch (transcript) {
        case PM_TRANSCRIPT_MERLIN: return launch_x1<C, fs::KIND_MERLIN>(ctx, pk, rows, solve);
        case PM_TRANSCRIPT_KECCAK256: return launch_x1<C, fs::KIND_KECCAK256>(ctx, pk, rows, solve);
        case PM_TRANSCRIPT_BLAKE3: return launch_x1<C, fs::KIND_BLAKE3>(ctx, pk, rows, solve);
        default: return PM_ERR_INVALID_ARG;
    }
}

template <class C>
int glue_x2(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t rows, size_t g0) {
    switch (transcript) {
        case PM_TRANSCRIPT_MERLIN: return launch_x2<C, fs::KIND_MERLIN>(ctx, pk, rows, g0);
        case PM_TRANSCRIPT_KECCAK256: return launch_x2<C, fs::KIND_KECCAK256>(ctx, pk, rows, g0);
        case PM_TRANSCRIPT_BLAKE3: return launch_x2<C, fs::KIND_BLAKE3>(ctx, pk, rows, g0);
        default: return PM_ERR_INVALID_ARG;
    }
}

template <class C>
int glue_finish(pm_ctx *ctx, const pm_pk *pk, size_t rows, bool solve, uint8_t *proofs, size_t proof_len, int *status) {
    GlueWs &gw = ctx->gw;
    {
        StageTimer t(ctx, T_POLY);
        PM_LAUNCH(ctx, k_proof_bytes<C>, dim3(nblk(rows, GLUE_BLOCK)), dim3(GLUE_BLOCK), 0, ctx->stream, glue_rows<C>(ctx, pk, rows, solve, proof_len),
                       gw.pts.as<BatchPoint<C>>() + 2 * gw.cap);
    }
    const size_t bytes = rows * (proof_len + sizeof(int));
    gw.host.resize(bytes);
    PM_HIP(ctx, hipMemcpyAsync(gw.host.data(), gw.out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));   // the group's one copy ...
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));                                                     // ... and one synchronisation
    memcpy(proofs, gw.host.data(), rows * proof_len);
    memcpy(status, gw.host.data() + rows * proof_len, rows * sizeof(int));
    return PM_OK;
}

#define PM_INST(C)                                                                                                  \
    template int glue_begin<C>(pm_ctx *, const pm_pk *, size_t);                                                    \
    template int glue_upload<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, size_t);       \
    template int glue_x1<C>(pm_ctx *, const pm_pk *, int, size_t, bool);                                            \
    template int glue_x2<C>(pm_ctx *, const pm_pk *, int, size_t, size_t);                                          \
    template int glue_finish<C>(pm_ctx *, const pm_pk *, size_t, bool, uint8_t *, size_t, int *);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
