// pm_r1cs_check / pm_r1cs_check_batch: WHICH rows of the R1CS an assignment violates.  The prover only learns that some row does
// (prove.hip: k_check_sap ORs one bit); this pass names the rows, counts them and, on request, returns the three products of each
// listed row -- what ark-relations' ConstraintSystem::which_is_unsatisfied answers on the host.
//
// Three kernels over the key's resident CSR matrices (first-entry rule already applied, api.hip: dedupe_csr), assignment = grid y:
//   k_r1cs_mask       one lane per row: bad = (Az)_r (Bz)_r != (Cz)_r; a wave's 64 votes are ONE mask word
//   k_r1cs_scan       one workgroup per assignment: popcount scan of the mask words -> n_bad and the smallest failing rows, ascending
//   k_r1cs_residuals  one lane per listed row: (Az)_r, (Bz)_r, (Cz)_r
// No atomics anywhere: a mask word has one writer, a slot of `rows` has one writer (its position is the exclusive prefix of the
// popcounts), so the outputs are the same words on every run.  Nothing of the context's proof in flight is touched: the buffers are
// the call's own and are returned when it ends.
#include <cstring>
#include <vector>

#include "internal.h"
#include "prove_common.cuh"

namespace pm {

constexpr unsigned R1CS_SCAN_LANES = 256;                      // k_r1cs_scan's workgroup: one mask word per lane and iteration
constexpr unsigned R1CS_SCAN_ROWS = R1CS_SCAN_LANES * 64;      // rows covered by one iteration of the scan (2^14)
static_assert(R1CS_SCAN_LANES % 64 == 0 && R1CS_SCAN_ROWS <= (1u << 16), "the scan's waves are whole and an iteration's counts stay small");
constexpr uint64_t R1CS_NO_ROW = ~(uint64_t)0;                 // an unused slot of `rows`

// mask[b][r / 64] bit r % 64 = row r of assignment b fails.  xs, ws: elements between the x rows / the w rows of consecutive assignments
// (m0 and mw for the caller's two arrays; m0 + mw for both where the rows are x || w, as the solver leaves them).  blockDim.x is a multiple of 64, so a wave holds 64 consecutive rows
// starting at a multiple of 64; every lane reaches the ballot (lanes past nr vote 0), lane 0 of the wave stores the word.
template <class P>
__global__ __launch_bounds__(256) void k_r1cs_mask(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *x, const Fp<P> *w, uint64_t m0, uint64_t xs, uint64_t ws,
                                                   uint64_t nr, uint64_t words, unsigned long long *mask) {
    const uint64_t b = blockIdx.y;
    x += b * xs; w += b * ws; mask += b * words;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (r < nr) {
        Fp<P> az = csr_row_dot<P>(A.rowptr, A.col, A.val, x, w, m0, r);
        Fp<P> bz = csr_row_dot<P>(B.rowptr, B.col, B.val, x, w, m0, r);
        Fp<P> cz = csr_row_dot<P>(Cm.rowptr, Cm.col, Cm.val, x, w, m0, r);
        bad = !mul<P>(az, bz).eq(cz);
    }
    const unsigned long long votes = __ballot(bad);
    const uint64_t word = r >> 6;
    if ((threadIdx.x & 63) == 0 && word < words) mask[word] = votes;
}

// One workgroup per assignment walks its mask in iterations of R1CS_SCAN_LANES words.  Per iteration: popcount per lane, inclusive
// scan inside the wave (shuffles), the four wave totals through LDS, and `carry` = the failing rows of all earlier iterations (the
// same value in every lane).  A lane whose exclusive prefix is below max_rows writes its set bits, lowest first, from that slot on.
// rows: [assignment][max_rows], slots past n_bad = R1CS_NO_ROW.
__global__ __launch_bounds__(R1CS_SCAN_LANES) void k_r1cs_scan(const unsigned long long *mask, uint64_t words, uint64_t max_rows,
                                                               uint64_t *n_bad, uint64_t *rows) {
    __shared__ unsigned wave_total[R1CS_SCAN_LANES / 64];
    const uint64_t b = blockIdx.x;
    mask += b * words; rows += b * max_rows;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < words; base += R1CS_SCAN_LANES) {
        const uint64_t i = base + threadIdx.x;
        unsigned long long m = i < words ? mask[i] : 0ull;
        const unsigned cnt = (unsigned)__popcll(m);
        unsigned incl = cnt;
        for (unsigned off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (unsigned v = 0; v < R1CS_SCAN_LANES / 64; ++v) {
            const unsigned t = wave_total[v];
            if (v < wave) before += t;
            total += t;
        }
        __syncthreads();                       // wave_total is rewritten by the next iteration
        uint64_t pos = carry + before + (incl - cnt);
        while (m && pos < max_rows) {
            rows[pos++] = i * 64 + (uint64_t)(__ffsll(m) - 1);
            m &= m - 1;
        }
        carry += total;
    }
    for (uint64_t j = carry + threadIdx.x; j < max_rows; j += R1CS_SCAN_LANES) rows[j] = R1CS_NO_ROW;
    if (threadIdx.x == 0) n_bad[b] = carry;
}

// abc: [assignment][max_rows][3] = (Az)_r, (Bz)_r, (Cz)_r of the row in the slot, zero for an unused slot
template <class P>
__global__ __launch_bounds__(256) void k_r1cs_residuals(CsrDev A, CsrDev B, CsrDev Cm, const Fp<P> *x, const Fp<P> *w, uint64_t m0, uint64_t xs, uint64_t ws,
                                                        const uint64_t *rows, uint64_t max_rows, Fp<P> *abc) {
    const uint64_t b = blockIdx.y;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= max_rows) return;
    x += b * xs; w += b * ws;
    const uint64_t r = rows[b * max_rows + j];
    Fp<P> *out = abc + (b * max_rows + j) * 3;
    if (r == R1CS_NO_ROW) {
        out[0] = out[1] = out[2] = Fp<P>::zero();
        return;
    }
    out[0] = csr_row_dot<P>(A.rowptr, A.col, A.val, x, w, m0, r);
    out[1] = csr_row_dot<P>(B.rowptr, B.col, B.val, x, w, m0, r);
    out[2] = csr_row_dot<P>(Cm.rowptr, Cm.col, Cm.val, x, w, m0, r);
}

namespace {

// With `solve` (PM_ASSIGNMENT_SOLVE) the unknown entries are computed first (solve.hip) and the check reads the completed rows.
// Assignments run in GROUPS of as many as keep group * (m0 + mw) inside one MSM piece (the knob pm_host_prove_batch sizes its groups
// by), at least one, at most 65 535 (grid y).  Host assignments are uploaded group by group; device assignments are read where they
// are.  The device lists min(max_rows, nr) rows per assignment -- no more can fail -- and the host pads the caller's slots beyond.
template <class C>
int r1cs_check_impl(pm_ctx *ctx, const pm_pk *pk, size_t count, const uint64_t *x, const uint64_t *w, bool on_device, bool solve, size_t max_rows,
                    uint64_t *n_bad, uint64_t *rows, uint64_t *abc) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const uint64_t m0 = pk->m0, mw = pk->mw, nr = pk->nr;
    const uint64_t words = (nr + 63) / 64;
    const uint64_t listed = max_rows < nr ? max_rows : nr;
    size_t group = msm_max_piece(ctx) / (size_t)(m0 + mw);
    if (group < 1) group = 1;
    if (group > 65535) group = 65535;
    if (group > count) group = count;
    hipStream_t st = ctx->stream;
    ScopedDevBuf d_x, d_w, d_mask, d_n_bad, d_rows, d_abc;   // the call's device memory
    TimingGuard timing_guard{ctx};
    timing_reset(ctx);
    uint64_t xs = m0, ws = mw;
    if (solve) {
        // the assignments are completed first, in the same groups, into the context's [count][m0 + mw] buffer (pm_prove_tap(10)); the
        // check then reads those rows.  A structural error returns here: nothing has been written.
        PM_TRY(solve_all<C>(ctx, pk, count, x, w, on_device, group, T_NTT));
        x = (const uint64_t *)ctx->sv.xw.p;
        w = x + 4 * m0;
        xs = ws = m0 + mw;
        on_device = true;
    }
    if (!on_device) {
        PM_HIP(ctx, d_x.reserve(group * m0 * sizeof(Fr)));
        if (mw) PM_HIP(ctx, d_w.reserve(group * mw * sizeof(Fr)));
    }
    if (words) PM_HIP(ctx, d_mask.reserve(group * words * sizeof(unsigned long long)));
    PM_HIP(ctx, d_n_bad.reserve(group * sizeof(uint64_t)));
    if (listed) PM_HIP(ctx, d_rows.reserve(group * listed * sizeof(uint64_t)));
    if (listed && abc) PM_HIP(ctx, d_abc.reserve(group * listed * 3 * sizeof(Fr)));
    std::vector<uint64_t> h_rows(group * listed), h_abc(abc ? group * listed * 12 : 0);
    const CsrDev A{pk->d_rowptr[0], pk->d_col[0], pk->d_val[0]}, B{pk->d_rowptr[1], pk->d_col[1], pk->d_val[1]},
        Cm{pk->d_rowptr[2], pk->d_col[2], pk->d_val[2]};
    for (size_t g0 = 0; g0 < count; g0 += group) {
        const size_t g = count - g0 < group ? count - g0 : group;
        const Fr *gx = (const Fr *)x + g0 * xs, *gw = mw ? (const Fr *)w + g0 * ws : nullptr;
        if (!on_device) {
            PM_HIP(ctx, hipMemcpyAsync(d_x.p, gx, g * m0 * sizeof(Fr), hipMemcpyHostToDevice, st));
            if (mw) PM_HIP(ctx, hipMemcpyAsync(d_w.p, gw, g * mw * sizeof(Fr), hipMemcpyHostToDevice, st));
            gx = d_x.as<Fr>();
            gw = d_w.as<Fr>();
        }
        {
            StageTimer t(ctx, T_WITNESS_MAP);
            if (words) {
                PM_LAUNCH(ctx, k_r1cs_mask<P>, dim3(nblk(nr), (unsigned)g), dim3(256), 0, st, A, B, Cm, gx, gw, m0, xs, ws, nr, words,
                               d_mask.as<unsigned long long>());
            }
            PM_LAUNCH(ctx, k_r1cs_scan, dim3((unsigned)g), dim3(R1CS_SCAN_LANES), 0, st, d_mask.as<unsigned long long>(), words, listed,
                           d_n_bad.as<uint64_t>(), d_rows.as<uint64_t>());
            if (listed && abc) {
                PM_LAUNCH(ctx, k_r1cs_residuals<P>, dim3(nblk(listed), (unsigned)g), dim3(256), 0, st, A, B, Cm, gx, gw, m0, xs, ws,
                               d_rows.as<uint64_t>(), listed, d_abc.as<Fr>());
            }
        }
        PM_HIP(ctx, hipMemcpyAsync(n_bad + g0, d_n_bad.p, g * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (listed) PM_HIP(ctx, hipMemcpyAsync(h_rows.data(), d_rows.p, g * listed * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (listed && abc) PM_HIP(ctx, hipMemcpyAsync(h_abc.data(), d_abc.p, g * listed * 3 * sizeof(Fr), hipMemcpyDeviceToHost, st));
        PM_HIP(ctx, hipStreamSynchronize(st));
        for (size_t b = 0; b < g && max_rows; ++b) {
            uint64_t *out = rows + (g0 + b) * max_rows;
            memcpy(out, h_rows.data() + b * listed, listed * sizeof(uint64_t));
            for (size_t j = listed; j < max_rows; ++j) out[j] = R1CS_NO_ROW;
            if (!abc) continue;
            uint64_t *res = abc + (g0 + b) * max_rows * 12;
            memcpy(res, h_abc.data() + b * listed * 12, listed * 12 * sizeof(uint64_t));
            memset(res + listed * 12, 0, (max_rows - listed) * 12 * sizeof(uint64_t));
        }
        for (size_t b = 0; b < g && solve; ++b) {   // a stuck assignment has nothing to check: its stuck row instead
            const uint64_t stuck = solve_tap9_row(ctx, pk, g0 + b)[0];
            if (stuck == R1CS_NO_ROW) continue;
            n_bad[g0 + b] = R1CS_NO_ROW;
            for (size_t j = 0; j < max_rows; ++j) rows[(g0 + b) * max_rows + j] = j ? R1CS_NO_ROW : stuck;
            if (abc && max_rows) memset(abc + (g0 + b) * max_rows * 12, 0, max_rows * 12 * sizeof(uint64_t));
        }
    }
    return PM_OK;
}

}  // namespace
}  // namespace pm

extern "C" int pm_r1cs_check_batch(pm_ctx *ctx, const pm_pk *pk, size_t count, const uint64_t *x, const uint64_t *w, int assignment_on_device,
                                   size_t max_rows, uint64_t *n_bad, uint64_t *rows, uint64_t *abc) {
    if (!pm::assignment_flags_ok(assignment_on_device) || !ctx || !pk) return PM_ERR_INVALID_ARG;
    const bool on_device = (assignment_on_device & PM_ASSIGNMENT_DEVICE) != 0, solve = (assignment_on_device & PM_ASSIGNMENT_SOLVE) != 0;
    if (pk->shard_count != 1 || pk->layout != PM_SHARD_PAIRS || pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    if (count == 0) return PM_OK;
    if (!n_bad || !x || (pk->mw && !w) || (max_rows && !rows)) return PM_ERR_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
    try {
        return pm::with_curve(pk->curve, [&](auto cv) {
            return pm::r1cs_check_impl<pm::type_of<decltype(cv)>>(ctx, pk, count, x, w, on_device, solve, max_rows, n_bad, rows, abc);
        });
    } catch (const std::bad_alloc &) {
        ctx->err = "pm_r1cs_check: out of host memory";
        return PM_ERR_STATE;
    }
}

extern "C" int pm_r1cs_check(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, int assignment_on_device, size_t max_rows,
                             uint64_t *n_bad, uint64_t *rows, uint64_t *abc) {
    return pm_r1cs_check_batch(ctx, pk, 1, x, w, assignment_on_device, max_rows, n_bad, rows, abc);
}
