// Pieces shared by the two provers (prove.hip: whole vectors on one GPU; prove_sharded.hip: PM_SHARD_VECTOR).
#pragma once
#include <cstring>

#include "internal.h"
#include "fq28.cuh"
#include "batch_row.cuh"

namespace pm {

// --------------------------------------------------------------------------- witness map
// rows 2m0+r and 2m0+nr+r of (U z, W z) and y_{m0+r} = ((A-B) xw)_r^2  (prover.rs:279-302,
// common.rs:138-207).  CSR values are Montgomery Fr.
template <class P>
__device__ __forceinline__ Fp<P> csr_row_dot(const uint64_t *rowptr, const uint32_t *col, const uint64_t *val,
                                             const Fp<P> *z, uint64_t r) {
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
        Fp<P> v = *(const Fp<P> *)(val + 4 * k);
        acc = add<P>(acc, mul<P>(v, z[col[k]]));
    }
    return acc;
}

// the same dot product with z = x || w read from the caller's two arrays in place (r1cs_check.hip): column j < m0 is x[j]
template <class P>
__device__ __forceinline__ Fp<P> csr_row_dot(const uint64_t *rowptr, const uint32_t *col, const uint64_t *val,
                                             const Fp<P> *x, const Fp<P> *w, uint64_t m0, uint64_t r) {
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
        Fp<P> v = *(const Fp<P> *)(val + 4 * k);
        const uint64_t j = col[k];
        acc = add<P>(acc, mul<P>(v, j < m0 ? x[j] : w[j - m0]));
    }
    return acc;
}

struct CsrDev {
    const uint64_t *rowptr;
    const uint32_t *col;
    const uint64_t *val;
};

struct NumParams {
    uint64_t n, sigma, len;
};

// The lengths of one proof's vectors on an unsharded key, and the level plan of the division scan (prove_kernels.cuh): level l holds
// cnt[l] values, DIV_L of them per lane, until the top level is <= 64 values for one lane (16^6 covers every domain of both curves).
constexpr unsigned HORNER_L = 16;   // coefficients per lane of the phase-2 Horner sum
struct ProofShape {
    uint64_t n, m0, mw, nr, sigma;
    uint64_t Lz;        // |z_tail| = M - m0
    uint64_t len_a;     // [a]_1 scalars: u (n) | 0 | r_a (2)
    uint64_t len_c;     // [c]_1 scalars: z_tail | h (n-1) | 2 r_a u (n+1) | r_a^2 (3) | r_a (2)
    uint64_t num_len;   // coefficients of the numerator (numerator_at's table)
    uint64_t len_d;     // [d]_1 scalars: the quotient
    uint64_t cnt[8];
    int levels;
};
static inline ProofShape proof_shape(uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma) {
    ProofShape s{};
    s.n = n; s.m0 = m0; s.mw = mw; s.nr = nr; s.sigma = sigma;
    s.Lz = 2 * m0 + mw + nr;
    s.len_a = n + 3;
    s.len_c = s.Lz + (n - 1) + (n + 1) + 3 + 2;
    s.num_len = pmlayout::numerator_len(n);   // sigma = n + 3 on every key (key_shape)
    s.len_d = s.num_len - 1;
    s.cnt[0] = s.num_len;
    while (s.cnt[s.levels] > 64 && s.levels < 6) {
        s.cnt[s.levels + 1] = (s.cnt[s.levels] + DIV_L - 1) / DIV_L;
        ++s.levels;
    }
    return s;
}
static inline ProofShape proof_shape(const pm_pk *pk) { return proof_shape(pk->n, pk->m0, pk->mw, pk->nr, pk->sigma); }

// Phase 3: the division's level buffers of `rows` proofs in ws.lvl, reserved.  Level l >= 1 of a proof is V[l] (cnt[l] values) followed
// by H[l] (cnt[l] + 1 suffix values); proof b's are vs[l] elements further on than proof b - 1's.
template <class Fr>
struct DivLevels {
    Fr *V[8] = {nullptr}, *H[8] = {nullptr};
    uint64_t vs[8] = {0};
};
template <class Fr>
static inline hipError_t div_levels_reserve(ProveWs &ws, const ProofShape &d, size_t rows, DivLevels<Fr> &lv) {
    for (int l = 1; l <= d.levels; ++l) {
        lv.vs[l] = 2 * d.cnt[l] + 2;
        const hipError_t e = ws.lvl[l - 1].reserve(rows * lv.vs[l] * sizeof(Fr));
        if (e != hipSuccess) return e;
        lv.V[l] = ws.lvl[l - 1].template as<Fr>();
        lv.H[l] = lv.V[l] + d.cnt[l];
    }
    return hipSuccess;
}

// The flag word of a proof (k_check_sap) as a status.  Phase 1 reads bits 0-2, phase 3 bit 3.
__host__ __device__ static inline int phase1_flag_status(unsigned flags) {
    if (flags & 1u) return PM_ERR_REMAINDER_NONZERO;                  // prover.rs:108
    if ((flags & 2u) || !(flags & 4u)) return PM_ERR_DEGREE_BOUND;    // prover.rs:107
    return PM_OK;
}
__host__ __device__ static inline int phase3_flag_status(unsigned flags) { return (flags & 8u) ? PM_ERR_REMAINDER_NONZERO : PM_OK; }   // prover.rs:221

// ------------------------------------------------------------------------------- helpers
template <class P>
static inline Fp<P> load_fr(const uint64_t *p) {
    Fp<P> r;
    memcpy(r.l, p, sizeof(r.l));
    return r;
}
template <class C>
static inline void store_affine_host(const Affine<C> &a, int inf, uint64_t *xy, int *out_inf) {
    if (inf) memset(xy, 0, sizeof(Affine<C>));
    else memcpy(xy, &a, sizeof(Affine<C>));
    *out_inf = inf;
}

static inline unsigned nblk(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

// omega^e from the half-size table tw[j] = omega^j, j < n/2 (omega^(n/2) = -1)
template <class P>
__device__ __forceinline__ Fp<P> tw_pow(const Fp<P> *tw, uint64_t n, uint64_t e) {
    e &= n - 1;
    const uint64_t half = n >> 1;
    return e < half ? tw[e] : neg<P>(tw[e - half]);
}

// The sum of one value per lane over a workgroup of THREADS lanes, by a tree in `sh` (THREADS elements of LDS): lane 0 gets the sum, the
// other lanes zero.  The tree's last barrier is the trailing one -- only lane 0 reads sh[0] after it and only lane 0 writes it next, so
// `sh` can take the next sum at once.
template <class P, unsigned THREADS>
__device__ __forceinline__ Fp<P> block_sum(Fp<P> *sh, const Fp<P> &v) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (unsigned off = THREADS / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] = add<P>(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    return threadIdx.x == 0 ? sh[0] : Fp<P>::zero();
}

// The opening of a prover phase: the context's stage times start afresh (unless the caller keeps them) and T_PHASE brackets the phase;
// `start` = the key of a proof that begins here (phase 1).  Every return path stops the phase timer and then reads the timers.
struct PhaseTimers {
    TimingGuard guard;
    StageTimer t_phase;
    static pm_ctx *open(pm_ctx *ctx, const pm_pk *start) {
        if (!ctx->keep_timings) timing_reset(ctx);
        if (start) { ctx->pk = start; ctx->phase = 0; }
        return ctx;
    }
    explicit PhaseTimers(pm_ctx *ctx, const pm_pk *start = nullptr) : guard{open(ctx, start)}, t_phase(ctx, T_PHASE) {}
    void done() { t_phase.stop(); timing_flush(guard.ctx); }   // on success: the times are read before the phase returns
};

// The flag word of a proof rides behind the phase's MSMs: its copy to the host is enqueued here and read after the MSM's own final
// synchronisation, so the host does not wait between the kernels and the sort.  It lands in the pinned slot PINNED_FLAGS (a pageable
// destination would make the copy wait for the stream) unless the caller names another destination; zeroed first.
static inline int stage_flags(pm_ctx *ctx, const unsigned *d_flags, volatile unsigned **h_flags, unsigned *dst = nullptr) {
    if (!dst && !ctx_pinned(ctx)) { ctx->err = "pinned staging allocation failed"; return PM_ERR_HIP; }
    *h_flags = dst ? dst : pinned_slot<volatile unsigned>(ctx, PINNED_FLAGS);
    **h_flags = 0;
    PM_HIP(ctx, hipMemcpyAsync((void *)*h_flags, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    return PM_OK;
}


// ------------------------------------------------------------- numerator + division (phase 3)
// Numerator of prover.rs:211-216, multiplied through by Y^-gamma = X^(5 sigma), as a function of
// the coefficient index k (never materialised):
//   [0,2)            x2 r_a
//   2s + [0,3)       r_a + x2 r_a^2
//   3s + [0,n)       x2 * witness_u                          (prover.rs:168-171)
//   5s + [0,n+1)     u + x2 * 2 r_a u  - (a + x2 c) at +0    (prover.rs:145-152,366-368,196-197)
//   8s + [0,2n-1)    x2 * u^2     (witness_w + (u^2 - w) = u^2: N6 == N2)
template <class P>
__device__ __forceinline__ Fp<P> numerator_at(uint64_t k, const NumParams &np, const NumConsts<P> &nc, const Fp<P> *u,
                                              const Fp<P> *wit_u, const Fp<P> *u2) {
    const uint64_t s = np.sigma, n = np.n;
    if (k >= 8 * s) {
        uint64_t i = k - 8 * s;
        return i < 2 * n - 1 ? mul<P>(nc.x2, u2[i]) : Fp<P>::zero();
    }
    if (k >= 5 * s) {
        uint64_t i = k - 5 * s;
        if (i > n) return Fp<P>::zero();
        Fp<P> t = Fp<P>::zero();
        if (i < n) t = add<P>(u[i], mul<P>(nc.two_x2_r0, u[i]));
        if (i > 0) t = add<P>(t, mul<P>(nc.two_x2_r1, u[i - 1]));
        if (i == 0) t = add<P>(t, nc.minus_const);
        return t;
    }
    if (k >= 3 * s) {
        uint64_t i = k - 3 * s;
        return i < n ? mul<P>(nc.x2, wit_u[i]) : Fp<P>::zero();
    }
    if (k >= 2 * s) {
        uint64_t i = k - 2 * s;
        return i < 3 ? nc.b2[i] : Fp<P>::zero();
    }
    if (k == 0) return nc.x2r0;
    if (k == 1) return nc.x2r1;
    return Fp<P>::zero();
}

// (batch_row.cuh: NumMul28 -- the Horner chains of the two kernels that walk the numerator run in reduced radix)
// numerator_at on reduced-radix limbs: a LAZY standard-form value, limbs < 4 * 2^29, value < 7p (u + two products + a constant)
template <class P, class RR>
__device__ __forceinline__ F28<RR> numerator28_at(uint64_t k, const NumParams &np, const NumConsts<P> &nc, const NumMul28<RR> &m, const Fp<P> *u,
                                                  const Fp<P> *wit_u, const Fp<P> *u2) {
    const uint64_t s = np.sigma, n = np.n;
    if (k >= 8 * s) {
        const uint64_t i = k - 8 * s;
        return i < 2 * n - 1 ? f28_mul<RR>(f28_unpack<RR>(u2[i].l), m.x2) : f28_zero<RR>();
    }
    if (k >= 5 * s) {
        const uint64_t i = k - 5 * s;
        if (i > n) return f28_zero<RR>();
        F28<RR> t = f28_zero<RR>();
        if (i < n) {
            const F28<RR> ui = f28_unpack<RR>(u[i].l);
            t = f28_add<RR>(ui, f28_mul<RR>(ui, m.two_x2_r0));
        }
        if (i > 0) t = f28_add<RR>(t, f28_mul<RR>(f28_unpack<RR>(u[i - 1].l), m.two_x2_r1));
        if (i == 0) t = f28_add<RR>(t, f28_unpack<RR>(nc.minus_const.l));
        return t;
    }
    if (k >= 3 * s) {
        const uint64_t i = k - 3 * s;
        return i < n ? f28_mul<RR>(f28_unpack<RR>(wit_u[i].l), m.x2) : f28_zero<RR>();
    }
    if (k >= 2 * s) {
        const uint64_t i = k - 2 * s;
        return i < 3 ? f28_unpack<RR>(nc.b2[i].l) : f28_zero<RR>();
    }
    if (k == 0) return f28_unpack<RR>(nc.x2r0.l);
    if (k == 1) return f28_unpack<RR>(nc.x2r1.l);
    return f28_zero<RR>();
}
// one Horner step: acc (tight limbs, value < 9p) -> acc x1 + N_k: the product is < 2p, the sum < 9p; carries propagated so that the
// next product's columns stay inside 64 bits (9 * 2^29 * 2^29 * 2 < 2^63)
template <class P, class RR>
__device__ __forceinline__ F28<RR> horner28_step(const F28<RR> &acc, uint64_t k, const NumParams &np, const NumConsts<P> &nc, const NumMul28<RR> &m,
                                                 const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2) {
    return f28_weak_norm<RR>(f28_add<RR>(f28_mul<RR>(acc, m.x1), numerator28_at<P, RR>(k, np, nc, m, u, wit_u, u2)));
}

}  // namespace pm
