// pm_host_prove_batch, device side: the three phases of prove.hip over a GROUP of proofs against one unsharded key.  Every vector of
// prove.hip is a [rows][len] array here (pm_ctx::pb), every kernel has the proof as grid y, and the three MSMs of a proof become three
// msm_run_batch calls per group: row b of the [a] / [c] / [d] scalar matrices is proof b's scalar vector, laid out at the stride
// msm_run_batch reads (the MSM's pair count).
//
// The kernels are the `_B` siblings of prove.hip's, body for body: the same field operations in the same order on the same values, so
// a row's vectors -- and with them its three points -- are those of the single prover.  What is a kernel argument there and differs
// from proof to proof (r_a, x1, the numerator's constants and reduced-radix multipliers, the division's level multipliers) is one
// BatchRow record per proof in device memory, uploaded once per phase and indexed by blockIdx.y.  Each proof has its own flag word.
// A proof whose witness fails a check keeps running (every operation is defined on any field values); the host drops its result.
#include <cstring>

#include "internal.h"
#include "fq28.cuh"
#include "prove_common.cuh"

namespace pm {

template <class P>
struct BatchRow {
    Fp<P> ra[2], x1;
    NumConsts<P> nc;
    NumMul28<typename Radix28<P>::RR> m28;
    Fp<P> xp[8];          // xp[l] = x1^(L^l): the multiplier of level l of the division scan
};

// ------------------------------------------------------------------------------- phase 1
template <class P>
__global__ void k_witness_rows_B(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *xw, uint64_t xw_stride, Fp<P> *ue, Fp<P> *we, uint64_t n,
                                 Fp<P> *y, uint64_t y_stride, uint64_t m0, uint64_t nr) {
    const uint64_t b = blockIdx.y;
    xw += b * xw_stride; ue += b * n; we += b * n; y += b * y_stride;
    uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    Fp<P> az = csr_row_dot<P>(A.rowptr, A.col, A.val, xw, r);
    Fp<P> bz = csr_row_dot<P>(B.rowptr, B.col, B.val, xw, r);
    Fp<P> cz = csr_row_dot<P>(Cm.rowptr, Cm.col, Cm.val, xw, r);
    Fp<P> d = sub<P>(az, bz), d2 = sqr<P>(d);
    Fp<P> c4 = dbl<P>(dbl<P>(cz));
    y[m0 + r] = d2;
    ue[2 * m0 + r] = add<P>(az, bz);
    we[2 * m0 + r] = add<P>(c4, d2);
    ue[2 * m0 + nr + r] = d;
    we[2 * m0 + nr + r] = d2;
}

template <class P>
__global__ void k_witness_head_B(const Fp<P> *xw, uint64_t xw_stride, Fp<P> *ue, Fp<P> *we, Fp<P> *ztail, uint64_t z_stride, uint64_t m0,
                                 uint64_t mw, uint64_t nr, uint64_t n) {
    const uint64_t b = blockIdx.y;
    xw += b * xw_stride; ue += b * n; we += b * n; ztail += b * z_stride;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fp<P> one = Fp<P>::one();
    if (i < m0 + mw) ztail[i] = xw[i];
    Fp<P> *y = ztail + m0 + mw;
    if (i < m0) {
        Fp<P> xi = xw[i];
        Fp<P> omx = sub<P>(one, xi), yi = i ? sqr<P>(omx) : Fp<P>::zero();
        y[i] = yi;
        if (i == 0) {
            ue[0] = dbl<P>(one);
            we[0] = dbl<P>(dbl<P>(one));
            ue[m0] = Fp<P>::zero();
            we[m0] = Fp<P>::zero();
        } else {
            ue[i] = add<P>(one, xi);
            we[i] = add<P>(dbl<P>(dbl<P>(xi)), yi);
            ue[m0 + i] = omx;
            we[m0 + i] = yi;
        }
    }
    uint64_t rows = 2 * (m0 + nr);
    if (i >= rows && i < n) {
        ue[i] = Fp<P>::zero();
        we[i] = Fp<P>::zero();
    }
}

template <class P>
__global__ void k_check_sap_B(const Fp<P> *ue, const Fp<P> *we, uint64_t n, unsigned *flags) {
    const uint64_t b = blockIdx.y;
    ue += b * n; we += b * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!sqr<P>(ue[i]).eq(we[i])) atomicOr(flags + b, 1u);
}

template <class P>
__global__ void k_copy_zero_head_B(const Fp<P> *src, Fp<P> *dst, uint64_t n, uint64_t zero_rows) {
    const uint64_t b = blockIdx.y;
    src += b * n; dst += b * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = i < zero_rows ? Fp<P>::zero() : src[i];
}

template <class P>
__global__ void k_wit_u_sparse_B(const Fp<P> *u, const Fp<P> *ue, const Fp<P> *winv, Fp<P> ninv, uint64_t n, unsigned head, Fp<P> *wit_u) {
    const uint64_t b = blockIdx.y;
    u += b * n; ue += b * n; wit_u += b * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t half = n >> 1;
    Fp<P> wk = winv[k < half ? k : k - half];
    if (k >= half) wk = neg<P>(wk);
    Fp<P> s = ue[head - 1];
    for (int j = (int)head - 2; j >= 0; --j) s = add<P>(mul<P>(s, wk), ue[j]);
    wit_u[k] = sub<P>(u[k], mul<P>(s, ninv));
}

template <class P>
__global__ void k_twist_B(const Fp<P> *u, const Fp<P> *psi_pow, Fp<P> *out, uint64_t n) {
    const uint64_t b = blockIdx.y;
    u += b * n; out += b * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = mul<P>(u[k], psi_pow[k]);
}
template <class P>
__global__ void k_untwist_combine_B(const Fp<P> *neg_tw, const Fp<P> *psi_inv_pow, const Fp<P> *w, Fp<P> *u2, uint64_t n, Fp<P> half) {
    const uint64_t b = blockIdx.y;
    neg_tw += b * n; w += b * n; u2 += b * 2 * n;
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Fp<P> neg = mul<P>(neg_tw[k], psi_inv_pow[k]), wk = w[k];
    u2[k] = mul<P>(add<P>(wk, neg), half);
    u2[n + k] = mul<P>(sub<P>(wk, neg), half);
}
template <class P>
__global__ void k_square_B(Fp<P> *a, uint64_t n) {
    a += (uint64_t)blockIdx.y * n;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = sqr<P>(a[i]);
}

// row b of the [c] scalar matrix after its z_tail, at stride len_c (prove.hip: k_phase1_scalars); the flag word is the row's own, and
// a wave that reads the row's "h != 0" bit as set still skips the atomic
template <class P>
__global__ void k_phase1_scalars_B(const Fp<P> *u, const Fp<P> *u2, const BatchRow<P> *rows, Fp<P> *sc_c_after_z, uint64_t len_c, uint64_t n,
                                   unsigned *flags) {
    const uint64_t b = blockIdx.y;
    u += b * n; u2 += b * 2 * n; sc_c_after_z += b * len_c; flags += b;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fp<P> r0 = rows[b].ra[0], r1 = rows[b].ra[1];
    if (i < n) {
        Fp<P> hi = u2[n + i];
        if (i < n - 1) {
            sc_c_after_z[i] = hi;
            if (!hi.is_zero() && !(*(const volatile unsigned *)flags & 4u)) atomicOr(flags, 4u);
        } else if (!hi.is_zero()) {
            atomicOr(flags, 2u);
        }
    }
    if (i <= n) {  // coefficient i of 2 r_a(X) u(X) = 2 (r0 u_i + r1 u_{i-1})
        Fp<P> t = Fp<P>::zero();
        if (i < n) t = mul<P>(r0, u[i]);
        if (i > 0) t = add<P>(t, mul<P>(r1, u[i - 1]));
        sc_c_after_z[(n - 1) + i] = dbl<P>(t);
    }
    if (i == 0) {
        Fp<P> *tail = sc_c_after_z + (n - 1) + (n + 1);
        tail[0] = sqr<P>(r0);
        tail[1] = dbl<P>(mul<P>(r0, r1));
        tail[2] = sqr<P>(r1);
        tail[3] = r0;
        tail[4] = r1;
    }
}

// row b of the [a] scalar matrix at stride len_a = n + 3 (prove.hip: k_sc_a)
template <class P>
__global__ void k_sc_a_B(const Fp<P> *u, const BatchRow<P> *rows, Fp<P> *sc_a, uint64_t len_a, uint64_t n) {
    const uint64_t b = blockIdx.y;
    u += b * n; sc_a += b * len_a;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sc_a[i] = u[i];
    if (i == 0) {
        sc_a[n] = Fp<P>::zero();
        sc_a[n + 1] = rows[b].ra[0];
        sc_a[n + 2] = rows[b].ra[1];
    }
}

// ------------------------------------------------------------------------------- phase 2
template <class P>
__global__ __launch_bounds__(256) void k_horner_partial_B(const Fp<P> *u, uint64_t n, const BatchRow<P> *rows, unsigned L, Fp<P> *partials) {
    __shared__ Fp<P> sh[256];
    const uint64_t b = blockIdx.y;
    u += b * n; partials += b * gridDim.x;
    const Fp<P> x1 = rows[b].x1;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > n) hi = n;
    Fp<P> acc = Fp<P>::zero();
    if (lo < n) {
        for (uint64_t k = hi; k-- > lo;) acc = add<P>(mul<P>(acc, x1), u[k]);
        acc = mul<P>(acc, pow_u64<P>(x1, lo));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] = add<P>(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

template <class P>
__global__ __launch_bounds__(256) void k_sum_small_B(const Fp<P> *in, unsigned count, Fp<P> *out) {   // one workgroup per row
    __shared__ Fp<P> sh[256];
    in += (uint64_t)blockIdx.x * count;
    Fp<P> acc = Fp<P>::zero();
    for (unsigned i = threadIdx.x; i < count; i += 256) acc = add<P>(acc, in[i]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] = add<P>(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// ------------------------------------------------------------------------------- phase 3: the division scan, every level with a row
template <class P>
__device__ __forceinline__ bool zero_stretch(const NumParams &np, uint64_t lo, uint64_t hi) {
    const uint64_t s = np.sigma, n = np.n;
    return (lo >= 2 && hi <= 2 * s) || (lo >= 2 * s + 3 && hi <= 3 * s) || (lo >= 3 * s + n && hi <= 5 * s) || (lo >= 5 * s + n + 1 && hi <= 8 * s);
}

template <class P>
__global__ void k_div_level0_B(NumParams np, const BatchRow<P> *rows, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2, unsigned L,
                               uint64_t nchunks, Fp<P> *V, uint64_t v_stride) {
    typedef typename Radix28<P>::RR RR;
    const uint64_t b = blockIdx.y;
    u += b * np.n; wit_u += b * np.n; u2 += b * 2 * np.n; V += b * v_stride;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > np.len) hi = np.len;
    if (zero_stretch<P>(np, lo, hi)) { V[t] = Fp<P>::zero(); return; }
    const BatchRow<P> &R = rows[b];
    F28<RR> acc = f28_zero<RR>();
    for (uint64_t k = hi; k-- > lo;) acc = horner28_step<P, RR>(acc, k, np, R.nc, R.m28, u, wit_u, u2);
    Fp<P> out;
    f28_pack_canonical<RR>(f28_canonical_lazy<RR, 3>(acc), out.l);
    V[t] = out;
}

template <class P>
__global__ void k_div_levelN_B(const Fp<P> *in, uint64_t in_stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned L,
                               uint64_t nchunks, Fp<P> *V, uint64_t v_stride) {
    const uint64_t b = blockIdx.y;
    in += b * in_stride; V += b * v_stride;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const Fp<P> xp = rows[b].xp[level];
    uint64_t lo = t * L, hi = lo + L;
    if (hi > count) hi = count;
    Fp<P> acc = Fp<P>::zero();
    for (uint64_t k = hi; k-- > lo;) acc = add<P>(mul<P>(acc, xp), in[k]);
    V[t] = acc;
}

// top level: one LANE per row, sequential over <= 64 values
template <class P>
__global__ void k_div_top_B(const Fp<P> *in, uint64_t stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned nrows, Fp<P> *H) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nrows) return;
    in += b * stride; H += b * stride;
    const Fp<P> xp = rows[b].xp[level];
    Fp<P> acc = Fp<P>::zero();
    H[count] = acc;
    for (uint64_t k = count; k-- > 0;) {
        acc = add<P>(mul<P>(acc, xp), in[k]);
        H[k] = acc;
    }
}

template <class P>
__global__ void k_div_expandN_B(const Fp<P> *in, uint64_t stride, uint64_t count, const BatchRow<P> *rows, int level, unsigned L,
                                uint64_t nchunks, const Fp<P> *Hup, uint64_t hup_stride, Fp<P> *H) {
    const uint64_t b = blockIdx.y;
    in += b * stride; H += b * stride; Hup += b * hup_stride;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const Fp<P> xp = rows[b].xp[level];
    uint64_t lo = t * L, hi = lo + L;
    if (hi > count) hi = count;
    Fp<P> acc = Hup[t + 1];
    for (uint64_t k = hi; k-- > lo;) {
        acc = add<P>(mul<P>(acc, xp), in[k]);
        H[k] = acc;
    }
    if (t == nchunks - 1) H[count] = Fp<P>::zero();
}

// level 0 writes row b of the [d] scalar matrix (the quotient) at stride q_stride; Hup == nullptr: carry-in 0 (the one-lane division)
template <class P>
__global__ void k_div_expand0_B(NumParams np, const BatchRow<P> *rows, const Fp<P> *u, const Fp<P> *wit_u, const Fp<P> *u2, unsigned L,
                                uint64_t nchunks, const Fp<P> *Hup, uint64_t hup_stride, Fp<P> *q, uint64_t q_stride, unsigned *flags) {
    typedef typename Radix28<P>::RR RR;
    const uint64_t b = blockIdx.y;
    u += b * np.n; wit_u += b * np.n; u2 += b * 2 * np.n; q += b * q_stride;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    uint64_t lo = t * L, hi = lo + L;
    if (hi > np.len) hi = np.len;
    const BatchRow<P> &R = rows[b];
    F28<RR> acc = Hup ? f28_unpack<RR>(Hup[b * hup_stride + t + 1].l) : f28_zero<RR>();
    if (zero_stretch<P>(np, lo, hi)) {
        for (uint64_t k = hi; k-- > lo;) {
            acc = f28_mul<RR>(acc, R.m28.x1);
            Fp<P> out;
            f28_pack_reduced<RR>(acc, out.l);
            q[k - 1] = out;        // lo >= 2 here
        }
        return;
    }
    for (uint64_t k = hi; k-- > lo;) {
        acc = f28_canonical_lazy<RR, 3>(horner28_step<P, RR>(acc, k, np, R.nc, R.m28, u, wit_u, u2));
        Fp<P> out;
        f28_pack_canonical<RR>(acc, out.l);
        if (k > 0) q[k - 1] = out;
        else if (!out.is_zero()) atomicOr(flags + b, 8u);  // rem != 0, prover.rs:221
    }
}

// ------------------------------------------------------------------------------- host side
namespace {

struct BatchDims {
    uint64_t n, m0, mw, nr, Lz, len_a, len_c, len_d, num_len;
    uint64_t cnt[8];
    int levels;
    bool layout_ok;        // the key's MSM ranges are the scalar rows this file writes
};
constexpr unsigned DIV_L = 16, HORNER_L = 16;   // prove.hip's chunk lengths: the same partial sums in the same order

BatchDims batch_dims(const pm_pk *pk) {
    BatchDims d;
    d.n = pk->n; d.m0 = pk->m0; d.mw = pk->mw; d.nr = pk->nr;
    d.Lz = 2 * d.m0 + d.mw + d.nr;
    d.len_a = d.n + 3;
    d.len_c = d.Lz + (d.n - 1) + (d.n + 1) + 3 + 2;
    d.num_len = 8 * pk->sigma + 2 * d.n - 1;
    d.len_d = d.num_len - 1;
    d.layout_ok = pk->shard_count == 1 && pk->layout == PM_SHARD_PAIRS && pk->res_cnt[0] == d.len_a && pk->res_cnt[1] == d.len_c &&
                  pk->res_cnt[2] == d.len_d && pk->res_lo[0] == 0 && pk->res_lo[1] == 0 && pk->res_lo[2] == 0;
    d.cnt[0] = d.num_len;
    d.levels = 0;
    while (d.cnt[d.levels] > 64 && d.levels < 6) {
        d.cnt[d.levels + 1] = (d.cnt[d.levels] + DIV_L - 1) / DIV_L;
        ++d.levels;
    }
    return d;
}

// Fr elements of the group's vectors per proof (pm_ctx::pb and the transforms' out-of-place temporary)
uint64_t row_elems(const BatchDims &d) {
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
    const BatchDims d = batch_dims(pk);
    const size_t max_piece = msm_max_piece(ctx);
    if (!d.layout_ok || d.len_d > max_piece) return PM_OK;
    size_t g = max_piece / d.len_d;
    if (g > 65535) g = 65535;                       // grid y
    size_t free_b = 0, total_b = 0;
    PM_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    size_t held = 0;
    ProveBatchWs &ws = ctx->pb;
    for (const DevBuf *b : {&ws.xw, &ws.ue, &ws.we, &ws.u, &ws.w, &ws.wit_u, &ws.u2, &ws.tmp, &ws.sc_a, &ws.sc_c, &ws.quotient, &ws.part, &ws.rows, &ws.flags})
        held += b->bytes;
    for (const DevBuf &b : ws.lvl) held += b.bytes;
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

template <class C>
static int upload_rows(pm_ctx *ctx, const std::vector<BatchRow<typename C::FrP>> &host) {
    PM_HIP(ctx, ctx->pb.rows.reserve(host.size() * sizeof(host[0])));
    PM_HIP(ctx, hipMemcpyAsync(ctx->pb.rows.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, ctx->stream));
    return PM_OK;
}

template <class C>
int prove_batch_xw(pm_ctx *ctx, const pm_pk *pk, size_t rows, Fp<typename C::FrP> **xw) {
    PM_HIP(ctx, ctx->pb.xw.reserve(rows * (pk->m0 + pk->mw) * sizeof(Fp<typename C::FrP>)));
    *xw = ctx->pb.xw.as<Fp<typename C::FrP>>();
    return PM_OK;
}

// xw_resident: the group's x || w rows are already in the workspace (prove_batch_xw: the witness solver completed them there);
// x and w are then not read
template <class C>
int prove_batch_phase1(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *x, const uint64_t *w, bool assignment_on_device,
                       const uint64_t *r_a, Affine<C> *a, int *a_inf, Affine<C> *c, int *c_inf, unsigned *flags_out, bool xw_resident) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const BatchDims d = batch_dims(pk);
    if (!d.layout_ok || rows == 0 || rows > 65535) return PM_ERR_INVALID_ARG;
    if (pk->log_n + 1 > (unsigned)C::TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;  // prover.rs:317
    const uint64_t n = d.n, m0 = d.m0, mw = d.mw, nr = d.nr, Lz = d.Lz, len_a = d.len_a, len_c = d.len_c;
    const unsigned gy = (unsigned)rows;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    StageTimer t_phase(ctx, T_PHASE);
    ProveBatchWs &ws = ctx->pb;
    PM_HIP(ctx, ws.xw.reserve(rows * (m0 + mw) * sizeof(Fr)));
    for (DevBuf *b : {&ws.ue, &ws.we, &ws.u, &ws.w, &ws.wit_u, &ws.tmp}) PM_HIP(ctx, b->reserve(rows * n * sizeof(Fr)));
    PM_HIP(ctx, ws.u2.reserve(rows * 2 * n * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_c.reserve(rows * len_c * sizeof(Fr)));
    PM_HIP(ctx, ws.sc_a.reserve(rows * len_a * sizeof(Fr)));
    PM_HIP(ctx, ws.flags.reserve(rows * sizeof(unsigned)));
    Fr *xw = ws.xw.as<Fr>(), *ue = ws.ue.as<Fr>(), *we = ws.we.as<Fr>(), *u = ws.u.as<Fr>(), *wv = ws.w.as<Fr>();
    Fr *wit_u = ws.wit_u.as<Fr>(), *u2 = ws.u2.as<Fr>(), *tmp = ws.tmp.as<Fr>(), *sc_c = ws.sc_c.as<Fr>(), *sc_a = ws.sc_a.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    PM_HIP(ctx, hipMemsetAsync(flags, 0, rows * sizeof(unsigned), st));
    const hipMemcpyKind kind = assignment_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // rows of x (m0) and of w (mw) interleave into rows of x || w
    if (!xw_resident) {
        PM_HIP(ctx, hipMemcpy2DAsync(xw, (m0 + mw) * sizeof(Fr), x, m0 * sizeof(Fr), m0 * sizeof(Fr), rows, kind, st));
        if (mw) PM_HIP(ctx, hipMemcpy2DAsync(xw + m0, (m0 + mw) * sizeof(Fr), w, mw * sizeof(Fr), mw * sizeof(Fr), rows, kind, st));
    }
    std::vector<BatchRow<P>> par(rows);
    memset((void *)par.data(), 0, rows * sizeof(BatchRow<P>));
    for (size_t b = 0; b < rows; ++b) memcpy((void *)par[b].ra, r_a + 8 * b, 2 * sizeof(Fr));
    PM_TRY(upload_rows<C>(ctx, par));
    const BatchRow<P> *drows = ws.rows.as<BatchRow<P>>();
    {
        StageTimer t(ctx, T_WITNESS_MAP);
        CsrDev A{pk->d_rowptr[0], pk->d_col[0], pk->d_val[0]}, B{pk->d_rowptr[1], pk->d_col[1], pk->d_val[1]},
            Cm{pk->d_rowptr[2], pk->d_col[2], pk->d_val[2]};
        const uint64_t head = n > m0 + mw ? n : m0 + mw;
        hipLaunchKernelGGL(k_witness_head_B<P>, dim3(nblk(head), gy), dim3(256), 0, st, xw, m0 + mw, ue, we, sc_c, len_c, m0, mw, nr, n);
        PM_HIP(ctx, hipGetLastError());
        if (nr) {
            hipLaunchKernelGGL(k_witness_rows_B<P>, dim3(nblk(nr), gy), dim3(256), 0, st, A, B, Cm, xw, m0 + mw, ue, we, n, sc_c + m0 + mw, len_c,
                               m0, nr);
            PM_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_check_sap_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, ue, we, n, flags);
        PM_HIP(ctx, hipGetLastError());
    }
    PM_HIP(ctx, hipMemcpyAsync(u, ue, rows * n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    PM_HIP(ctx, hipMemcpyAsync(wv, we, rows * n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    PM_TRY(ntt_run_batch<C>(ctx, u, pk->log_n, true, rows, n));
    hipLaunchKernelGGL(k_sc_a_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, drows, sc_a, len_a, n);
    PM_HIP(ctx, hipGetLastError());
    PM_TRY(ntt_run_batch<C>(ctx, wv, pk->log_n, true, rows, n));
    if (2 * m0 <= 16 && pk->log_n >= 1) {   // few public inputs: the sparse sum beats a fifth transform (prove.hip)
        const Fr *winv = nullptr;
        PM_TRY(twiddles_get<C>(ctx, pk->log_n, true, &winv));
        StageTimer t(ctx, T_NTT);
        hipLaunchKernelGGL(k_wit_u_sparse_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, ue, winv, inverse<P>(from_u64<P>(n)), n, (unsigned)(2 * m0),
                           wit_u);
        PM_HIP(ctx, hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_copy_zero_head_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, ue, wit_u, n, 2 * m0);
        PM_HIP(ctx, hipGetLastError());
        PM_TRY(ntt_run_batch<C>(ctx, wit_u, pk->log_n, true, rows, n));
    }
    {
        const Fr *psi = nullptr, *psi_inv = nullptr;
        PM_TRY(twiddles_get<C>(ctx, pk->log_n + 1, false, &psi));
        PM_TRY(twiddles_get<C>(ctx, pk->log_n + 1, true, &psi_inv));
        hipLaunchKernelGGL(k_twist_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, u, psi, tmp, n);
        PM_HIP(ctx, hipGetLastError());
        PM_TRY(ntt_run_batch<C>(ctx, tmp, pk->log_n, false, rows, n));
        hipLaunchKernelGGL(k_square_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, tmp, n);
        PM_HIP(ctx, hipGetLastError());
        PM_TRY(ntt_run_batch<C>(ctx, tmp, pk->log_n, true, rows, n));
        hipLaunchKernelGGL(k_untwist_combine_B<P>, dim3(nblk(n), gy), dim3(256), 0, st, tmp, psi_inv, wv, u2, n, inverse<P>(from_u64<P>(2)));
        PM_HIP(ctx, hipGetLastError());
    }
    {
        StageTimer t(ctx, T_POLY);
        hipLaunchKernelGGL(k_phase1_scalars_B<P>, dim3(nblk(n + 1), gy), dim3(256), 0, st, u, u2, drows, sc_c + Lz, len_c, n, flags);
        PM_HIP(ctx, hipGetLastError());
    }
    // [a]_1 and [c]_1 of every proof of the group: two batches over the key's PLAIN points (no tables, no wide plan)
    const Affine<C> *bases = (const Affine<C> *)pk->d_bases;
    PM_TRY(msm_run_batch<C>(ctx, bases + pk->res_dev_off[0], sc_a, (size_t)len_a, rows, a, a_inf));
    PM_TRY(msm_run_batch<C>(ctx, bases + pk->res_dev_off[1], sc_c, (size_t)len_c, rows, c, c_inf));
    PM_HIP(ctx, hipMemcpyAsync(flags_out, flags, rows * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    return PM_OK;
}

template <class C>
int prove_batch_phase2(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *x1, uint64_t *u_at_x1) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const BatchDims d = batch_dims(pk);
    if (rows == 0 || rows > 65535) return PM_ERR_INVALID_ARG;
    hipStream_t st = ctx->stream;
    ProveBatchWs &ws = ctx->pb;
    std::vector<BatchRow<P>> par(rows);
    memset((void *)par.data(), 0, rows * sizeof(BatchRow<P>));
    for (size_t b = 0; b < rows; ++b) par[b].x1 = load_fr<P>(x1 + 4 * b);
    PM_TRY(upload_rows<C>(ctx, par));
    const uint64_t lanes = (d.n + HORNER_L - 1) / HORNER_L;
    const unsigned blocks = nblk(lanes);
    PM_HIP(ctx, ws.part.reserve(rows * ((size_t)blocks + 1) * sizeof(Fr)));
    Fr *part = ws.part.as<Fr>(), *sums = part + rows * blocks;
    hipLaunchKernelGGL(k_horner_partial_B<P>, dim3(blocks, (unsigned)rows), dim3(256), 0, st, ws.u.as<Fr>(), d.n, ws.rows.as<BatchRow<P>>(), HORNER_L, part);
    PM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sum_small_B<P>, dim3((unsigned)rows), dim3(256), 0, st, part, blocks, sums);
    PM_HIP(ctx, hipGetLastError());
    PM_HIP(ctx, hipMemcpyAsync(u_at_x1, sums, rows * sizeof(Fr), hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    return PM_OK;
}

template <class C>
int prove_batch_phase3(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *r_a, const uint64_t *x1_in, const uint64_t *x2_in,
                       const uint64_t *a_in, const uint64_t *c_in, Affine<C> *dpt, int *d_inf, unsigned *flags_out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const BatchDims d = batch_dims(pk);
    if (!d.layout_ok || rows == 0 || rows > 65535) return PM_ERR_INVALID_ARG;
    const unsigned gy = (unsigned)rows, L = DIV_L;
    const int levels = d.levels;
    hipStream_t st = ctx->stream;
    TimingGuard timing_guard{ctx};
    StageTimer t_phase(ctx, T_PHASE);
    ProveBatchWs &ws = ctx->pb;
    NumParams np{d.n, pk->sigma, d.num_len};
    std::vector<BatchRow<P>> par(rows);
    memset((void *)par.data(), 0, rows * sizeof(BatchRow<P>));
    for (size_t b = 0; b < rows; ++b) {
        BatchRow<P> &R = par[b];
        memcpy((void *)R.ra, r_a + 8 * b, 2 * sizeof(Fr));
        R.x1 = load_fr<P>(x1_in + 4 * b);
        R.nc = make_num_consts<P>(load_fr<P>(x2_in + 4 * b), R.ra, load_fr<P>(a_in + 4 * b), load_fr<P>(c_in + 4 * b));
        R.m28 = make_num_mul28<P>(R.x1, R.nc);
        R.xp[0] = R.x1;
        for (int l = 1; l <= levels; ++l) R.xp[l] = pow_u64<P>(R.xp[l - 1], L);
    }
    PM_TRY(upload_rows<C>(ctx, par));
    const BatchRow<P> *drows = ws.rows.as<BatchRow<P>>();
    // V[l] | H[l] of level l >= 1, per row: cnt[l] values, then cnt[l] + 1 suffix values (prove.hip)
    Fr *V[8] = {nullptr}, *H[8] = {nullptr};
    uint64_t vs[8] = {0};
    for (int l = 1; l <= levels; ++l) {
        vs[l] = 2 * d.cnt[l] + 2;
        PM_HIP(ctx, ws.lvl[l - 1].reserve(rows * vs[l] * sizeof(Fr)));
        V[l] = ws.lvl[l - 1].as<Fr>();
        H[l] = V[l] + d.cnt[l];
    }
    PM_HIP(ctx, ws.quotient.reserve((rows * d.len_d + 2) * sizeof(Fr)));
    Fr *q = ws.quotient.as<Fr>();
    unsigned *flags = ws.flags.as<unsigned>();
    const Fr *u = ws.u.as<Fr>(), *wit_u = ws.wit_u.as<Fr>(), *u2 = ws.u2.as<Fr>();
    {
        StageTimer t(ctx, T_POLY);
        if (levels == 0) {   // small: one lane per proof does the whole division
            hipLaunchKernelGGL(k_div_expand0_B<P>, dim3(1, gy), dim3(64), 0, st, np, drows, u, wit_u, u2, (unsigned)np.len, (uint64_t)1,
                               (const Fr *)nullptr, (uint64_t)0, q, d.len_d, flags);
            PM_HIP(ctx, hipGetLastError());
        } else {
            hipLaunchKernelGGL(k_div_level0_B<P>, dim3(nblk(d.cnt[1]), gy), dim3(256), 0, st, np, drows, u, wit_u, u2, L, d.cnt[1], V[1], vs[1]);
            PM_HIP(ctx, hipGetLastError());
            for (int l = 1; l < levels; ++l) {
                hipLaunchKernelGGL(k_div_levelN_B<P>, dim3(nblk(d.cnt[l + 1]), gy), dim3(256), 0, st, V[l], vs[l], d.cnt[l], drows, l, L, d.cnt[l + 1],
                                   V[l + 1], vs[l + 1]);
                PM_HIP(ctx, hipGetLastError());
            }
            hipLaunchKernelGGL(k_div_top_B<P>, dim3(nblk(rows, 64)), dim3(64), 0, st, V[levels], vs[levels], d.cnt[levels], drows, levels, gy,
                               H[levels]);
            PM_HIP(ctx, hipGetLastError());
            for (int l = levels - 1; l >= 1; --l) {
                hipLaunchKernelGGL(k_div_expandN_B<P>, dim3(nblk(d.cnt[l + 1]), gy), dim3(256), 0, st, V[l], vs[l], d.cnt[l], drows, l, L, d.cnt[l + 1],
                                   H[l + 1], vs[l + 1], H[l]);
                PM_HIP(ctx, hipGetLastError());
            }
            hipLaunchKernelGGL(k_div_expand0_B<P>, dim3(nblk(d.cnt[1]), gy), dim3(256), 0, st, np, drows, u, wit_u, u2, L, d.cnt[1], H[1], vs[1], q,
                               d.len_d, flags);
            PM_HIP(ctx, hipGetLastError());
        }
    }
    PM_TRY(msm_run_batch<C>(ctx, (const Affine<C> *)pk->d_bases + pk->res_dev_off[2], q, (size_t)d.len_d, rows, dpt, d_inf));   // [d]_1 = M8
    PM_HIP(ctx, hipMemcpyAsync(flags_out, flags, rows * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    return PM_OK;
}

#define PM_INST(C)                                                                                                                          \
    template int prove_batch_group<C>(pm_ctx *, const pm_pk *, size_t, size_t *);                                                           \
    template int prove_batch_xw<C>(pm_ctx *, const pm_pk *, size_t, Fp<typename C::FrP> **);                                                \
    template int prove_batch_phase1<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, bool, const uint64_t *,         \
                                       Affine<C> *, int *, Affine<C> *, int *, unsigned *, bool);                                          \
    template int prove_batch_phase2<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, uint64_t *);                                      \
    template int prove_batch_phase3<C>(pm_ctx *, const pm_pk *, size_t, const uint64_t *, const uint64_t *, const uint64_t *,              \
                                       const uint64_t *, const uint64_t *, Affine<C> *, int *, unsigned *);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
