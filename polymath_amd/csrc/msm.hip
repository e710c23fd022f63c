// G1 variable-base multi-scalar multiplication for gfx950 (Pippenger bucket method).
//
// Replaces E::G1::msm_unchecked as the reference calls it (/root/reference/src/prover.rs:380-384,
// call sites :118,:121,:229,:335-354): result = sum_i scalar_i * base_i.  The result is a canonical
// group element, so the schedule below is free to differ from ark-ec's.
//
// Two pipelines share the task / accumulate / reduce kernels: (A) below, per-window Pippenger
// over a plain base array (one-shot pm_msm_g1, keys whose tables do not fit); (B) "Table mode" further down,
// the path every resident key takes.
// A batch of scalar rows against one base range (pm_msm_g1_resident_batch) is pipeline (A) over rows x windows bucket sets with its
// own digits kernel and a device-side final combine: msm_run_batch, at the end of this file.
// Pipeline (A), all on one HIP stream, no host round trip until the final point:
//   k_digits      scalar (Montgomery) -> canonical -> W signed c-bit digits, one u32 per
//                 (window, scalar): (bucket << 1 | negate), NONE for zero digits / infinity bases.
//   k_hist        LDS-staged histogram: a workgroup owns one (chunk, window) and counts into a
//                 2^(c-1)-entry LDS table (128 KiB at c = 16 -- this is what CDNA4's 160 KiB LDS
//                 buys), then flushes its non-zero bins with coalesced global atomics.
//   k_scan        exclusive scans: bucket offsets, and task offsets after splitting buckets
//                 longer than SEG entries into SEG-sized tasks (skewed scalars -> hot buckets).
//   k_scatter     same LDS staging: claim a range per (workgroup, bucket) with one global atomic,
//                 then place entries with LDS atomics -> base indices grouped by bucket.
//   k_task_bins   task descriptors ordered by descending length, so the lanes of a wave carry equal loads.
//   k_accumulate  persistent waves draw 64 descriptors at a time from a ticket counter; one lane per task: XYZZ
//                 mixed adds (8M+2S each) over its <= SEG entries;
//                 bases are gathered from HBM by index (96 B affine points, or 128 B TablePoint records).
//   k_task_fold   buckets that own many tasks (skewed scalars) have their partials summed in parallel.
//   k_bucket_reduce  per window sum_b (b+1) * B_b by per-lane running sums over K buckets, a
//                 small scalar multiple, and an LDS tree reduction per workgroup.
//   host_horner   Horner over the W window sums (c doublings each), then host_finish: one inversion to affine, on
//                 the host: an O(W) dependent chain (see host_horner).
#include <cstdlib>
#include <cstring>

#include "internal.h"
#include "fq28.cuh"

namespace pm {

constexpr uint32_t DIGIT_NONE = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------ digits
template <class C>
__global__ void k_digits(const Fp<typename C::FrP> *scalars, const Affine<C> *bases, uint32_t *digits, size_t len,
                         unsigned c, unsigned nwin) {
    typedef typename C::FrP P;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    Fp<P> k = from_mont<P>(scalars[i]);
    // a base at infinity contributes nothing (ark: msm adds the identity); drop it here so it
    // never reaches a bucket
    const uint32_t *bx = (const uint32_t *)&bases[i];
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 2 * C::FqP::N; ++t) any |= bx[t];
    const bool skip = (any == 0);
    uint32_t carry = 0;
    const uint32_t half = 1u << (c - 1), full = 1u << c, mask = full - 1;
    for (unsigned w = 0; w < nwin; ++w) {
        unsigned lo = w * c, limb = lo >> 5, off = lo & 31;
        uint32_t v = 0;
        if (limb < (unsigned)P::N) {
            uint64_t two = k.l[limb];
            if (limb + 1 < (unsigned)P::N) two |= (uint64_t)k.l[limb + 1] << 32;
            v = (uint32_t)(two >> off) & mask;
        }
        uint32_t d = v + carry;
        uint32_t out;
        if (d > half) {  // negative digit d - 2^c, magnitude m = 2^c - d in [0, 2^(c-1))
            uint32_t m = full - d;
            out = m ? (((m - 1) << 1) | 1u) : DIGIT_NONE;
            carry = 1;
        } else {
            out = d ? ((d - 1) << 1) : DIGIT_NONE;
            carry = 0;
        }
        digits[(size_t)w * len + i] = skip ? DIGIT_NONE : out;
    }
}

// --------------------------------------------------------------------- LDS-staged counting sort
__global__ __launch_bounds__(1024) void k_hist(const uint32_t *digits, uint32_t *counts, size_t len, unsigned chunk,
                                               unsigned nbuckets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *h = (uint32_t *)smem_raw;
    const unsigned w = blockIdx.y;
    for (unsigned b = threadIdx.x; b < nbuckets; b += blockDim.x) h[b] = 0;
    __syncthreads();
    size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk;
    if (hi > len) hi = len;
    const uint32_t *d = digits + (size_t)w * len;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t v = d[i];
        if (v != DIGIT_NONE) atomicAdd(&h[v >> 1], 1u);
    }
    __syncthreads();
    uint32_t *cw = counts + (size_t)w * nbuckets;
    for (unsigned b = threadIdx.x; b < nbuckets; b += blockDim.x) {
        uint32_t v = h[b];
        if (v) atomicAdd(&cw[b], v);
    }
}

// Exclusive scans over all G = nwin*nbuckets buckets, three small launches (tile scan, scan of the
// tile totals, offset add):
//   bucket_off[g] = sum_{g' < g} counts[g'],   task_off[g] = sum_{g' < g} ceil(counts[g'] / seg)
// (+ totals at index G).  A lane owns SCAN_PER contiguous counters (64 B), a workgroup SCAN_TILE.
constexpr unsigned SCAN_PER = 16, SCAN_TILE = 256 * SCAN_PER;

__global__ __launch_bounds__(256) void k_scan_tiles(const uint32_t *counts, uint32_t *bucket_off, uint32_t *task_off,
                                                    uint32_t *tile_tot, size_t G, unsigned seg) {
    __shared__ uint32_t s_a[256], s_b[256];
    const unsigned tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)tid * SCAN_PER;
    uint32_t c[SCAN_PER], nt[SCAN_PER];
    uint32_t sa = 0, sb = 0;
#pragma unroll
    for (unsigned k = 0; k < SCAN_PER; ++k) {
        c[k] = base + k < G ? counts[base + k] : 0u;
        nt[k] = (c[k] + seg - 1) / seg;
        sa += c[k];
        sb += nt[k];
    }
    s_a[tid] = sa;
    s_b[tid] = sb;
    __syncthreads();
    for (unsigned off = 1; off < 256; off <<= 1) {
        uint32_t va = 0, vb = 0;
        if (tid >= off) { va = s_a[tid - off]; vb = s_b[tid - off]; }
        __syncthreads();
        s_a[tid] += va;
        s_b[tid] += vb;
        __syncthreads();
    }
    uint32_t ra = s_a[tid] - sa, rb = s_b[tid] - sb;
#pragma unroll
    for (unsigned k = 0; k < SCAN_PER; ++k) {
        if (base + k < G) { bucket_off[base + k] = ra; task_off[base + k] = rb; }
        ra += c[k];
        rb += nt[k];
    }
    if (tid == 255) { tile_tot[2 * blockIdx.x] = s_a[255]; tile_tot[2 * blockIdx.x + 1] = s_b[255]; }
}

__global__ __launch_bounds__(1024) void k_scan_totals(uint32_t *tile_tot, unsigned ntiles, uint32_t *bucket_off,
                                                      uint32_t *task_off, size_t G) {
    __shared__ uint32_t s_a[1024], s_b[1024];
    const unsigned tid = threadIdx.x;
    uint32_t carry_a = 0, carry_b = 0;
    for (unsigned base = 0; base < ntiles; base += 1024) {
        unsigned i = base + tid;
        uint32_t a = i < ntiles ? tile_tot[2 * i] : 0u, b = i < ntiles ? tile_tot[2 * i + 1] : 0u;
        s_a[tid] = a;
        s_b[tid] = b;
        __syncthreads();
        for (unsigned off = 1; off < 1024; off <<= 1) {
            uint32_t va = 0, vb = 0;
            if (tid >= off) { va = s_a[tid - off]; vb = s_b[tid - off]; }
            __syncthreads();
            s_a[tid] += va;
            s_b[tid] += vb;
            __syncthreads();
        }
        if (i < ntiles) { tile_tot[2 * i] = carry_a + s_a[tid] - a; tile_tot[2 * i + 1] = carry_b + s_b[tid] - b; }
        carry_a += s_a[1023];
        carry_b += s_b[1023];
        __syncthreads();
    }
    if (tid == 0) { bucket_off[G] = carry_a; task_off[G] = carry_b; }
}

__global__ __launch_bounds__(256) void k_scan_add(uint32_t *bucket_off, uint32_t *task_off, const uint32_t *tile_tot, size_t G) {
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    const uint32_t oa = tile_tot[2 * blockIdx.x], ob = tile_tot[2 * blockIdx.x + 1];
#pragma unroll
    for (unsigned k = 0; k < SCAN_PER; ++k)
        if (base + k < G) { bucket_off[base + k] += oa; task_off[base + k] += ob; }
}

__global__ __launch_bounds__(1024) void k_scatter(const uint32_t *digits, const uint32_t *bucket_off, uint32_t *cursor,
                                                  uint32_t *sorted, size_t len, unsigned chunk, unsigned nbuckets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *h = (uint32_t *)smem_raw;
    const unsigned w = blockIdx.y;
    for (unsigned b = threadIdx.x; b < nbuckets; b += blockDim.x) h[b] = 0;
    __syncthreads();
    size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk;
    if (hi > len) hi = len;
    const uint32_t *d = digits + (size_t)w * len;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t v = d[i];
        if (v != DIGIT_NONE) atomicAdd(&h[v >> 1], 1u);
    }
    __syncthreads();
    const size_t gbase = (size_t)w * nbuckets;
    for (unsigned b = threadIdx.x; b < nbuckets; b += blockDim.x) {
        uint32_t v = h[b];
        if (v) h[b] = bucket_off[gbase + b] + atomicAdd(&cursor[gbase + b], v);
    }
    __syncthreads();
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t v = d[i];
        if (v != DIGIT_NONE) {
            uint32_t pos = atomicAdd(&h[v >> 1], 1u);
            sorted[pos] = ((uint32_t)i << 1) | (v & 1u);
        }
    }
}

// ------------------------------------------------------------------------------ task order
// k_accumulate gives every lane one task; a wave runs as long as its LONGEST task.  Bucket loads are
// Poisson (mean m, sigma sqrt(m)), so in launch order the 64 lanes of a wave idle ~2.5 sigma / m of the
// time (15 % at m = 168).  order[] lists the tasks by DESCENDING length (counting sort over the length,
// LDS histogram per workgroup): the lanes of a wave then carry (almost) equal loads and the longest
// tasks start first.  bin = (seg - L) >> lshift, L in [1, seg].
constexpr unsigned TASK_MAX_BINS = 8192;

// One lane per BUCKET g (its tasks are task_off[g] .. task_off[g + 1] - 1: all but the last are full, L = seg, bin 0; the last
// one has the remainder), so a lane issues at most two LDS atomics and no search.  (Round 2 ran one lane per TASK and found
// the task's bucket by a 21-step binary search over task_off: 0.19 ms for the two launches at 2^21 buckets.)
// The scatter pass writes each task's DESCRIPTOR at its place in the order: {partial slot t, first entry, end entry, 0}, so
// k_accumulate reads one 16-byte record per task and nothing else of the bucket metadata.
template <bool SCATTER>
__global__ __launch_bounds__(1024) void k_task_bins(const uint32_t *counts, const uint32_t *bucket_off, const uint32_t *task_off, size_t G,
                                                    unsigned seg, unsigned lshift, unsigned nbins, uint32_t *len_cnt, const uint32_t *len_off,
                                                    uint32_t *len_cursor, uint4 *tasks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *h = (uint32_t *)smem_raw;
    for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t t0 = 0, n = 0, rank_full = 0, rank_last = 0, cnt = 0;
    unsigned bin = 0;
    if (g < G) {
        t0 = task_off[g];
        n = task_off[g + 1] - t0;
        if (n) {
            cnt = counts[g];
            const uint32_t L = cnt - (n - 1) * seg;                 // 1 .. seg
            bin = (seg - L) >> lshift;
            if (n > 1) rank_full = atomicAdd(&h[0], n - 1);
            rank_last = atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    if (!SCATTER) {
        for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) {
            const uint32_t v = h[b];
            if (v) atomicAdd(&len_cnt[b], v);
        }
    } else {
        for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) {
            const uint32_t v = h[b];
            if (v) h[b] = len_off[b] + atomicAdd(&len_cursor[b], v);
        }
        __syncthreads();
        if (n) {
            const uint32_t at = h[0] + rank_full, first = bucket_off[g];
            for (uint32_t k = 0; k + 1 < n; ++k)                           // (a hot bucket: thousands; the rest: none or one)
                tasks[at + k] = make_uint4(t0 + k, first + k * seg, first + (k + 1) * seg, 0u);
            tasks[h[bin] + rank_last] = make_uint4(t0 + n - 1, first + (n - 1) * seg, first + cnt, 0u);
        }
    }
}

// ---------------------------------------------------------------------------- accumulate
// One lane per task; TABLE selects the point record (TablePoint of a window table, or the dense affine array of the per-window
// pipeline).  The accumulator lives in reduced-radix registers (fq28.cuh): 10 carry-free Montgomery products and 7 lazy add/sub
// per mixed add.  `bases` are in INTERNAL Montgomery form.
// The exceptional case acc == +-point (doubling / cancellation) is resolved on the dense path.
template <class C, bool TABLE>
__device__ __forceinline__ void accumulate_task(const uint32_t *sorted, const uint4 d, const void *points, XYZZ<C> *partials) {
    typedef typename C::FqRR RR;
    XYZZ28<C> acc;
    acc.X = acc.Y = acc.ZZ = acc.ZZZ = f28_zero<RR>();
    // The task's indices are read four at a time (one aligned 16-byte load per four additions): a lane's 4-byte load used to pull a
    // whole line of sorted[] through L2 for one entry, and by the lane's next addition (~4 500 instructions and 3 MB of gathered
    // points per XCD later) the line was gone again: 37 % fewer L2 reads, time neutral (profiles/r06_k_accumulate_l2_accounting.txt).
    // sorted[] carries 16 bytes of padding for the last quad.
    uint4 quad = make_uint4(0u, 0u, 0u, 0u);
    uint32_t quad_at = 0xffffffffu;
    for (uint32_t e = d.y; e < d.z; ++e) {
        if ((e & ~3u) != quad_at) {
            quad_at = e & ~3u;
            quad = *(const uint4 *)(sorted + quad_at);
        }
        const unsigned q = e & 3u;
        const uint32_t v = q == 0 ? quad.x : q == 1 ? quad.y : q == 2 ? quad.z : quad.w;
        const bool neg = (v & 1u) != 0;
        if (TABLE) {   // window tables: one aligned 128-byte record, already on 28-bit limbs
            const TablePoint<C> tp = ((const TablePoint<C> *)points)[v >> 1];
            F28<RR> x2, y2;
#pragma unroll
            for (int i = 0; i < RR::N; ++i) { x2.l[i] = tp.x[i]; y2.l[i] = tp.y[i]; }
            if (!xyzz28_madd_limbs<C>(acc, x2, y2, neg)) acc = xyzz28_madd_exceptional<C>(acc, table_point_to_affine<C>(tp), neg);
        } else {
            const Affine<C> p = ((const Affine<C> *)points)[v >> 1];
            if (!xyzz28_madd<C>(acc, p, neg)) acc = xyzz28_madd_exceptional<C>(acc, p, neg);
        }
    }
    partials[d.x] = xyzz28_store<C>(acc);   // INTERNAL form: the bucket reduction stays on reduced-radix arithmetic
}

// Persistent lanes: the grid holds only as many workgroups as can be resident (accumulate() below), and a wave takes the next 64
// descriptors of tasks[] (descending length: equal loads inside the wave) with one global atomic on the context's ticket
// counter, until the tasks run out.  Waves never wait on each other, so the kernel can share the chip with another context's
// launch.  (It replaced one lane per task over a grid of max_tasks lanes -- ~16 rounds of short-lived workgroups, ~1 M lanes
// that only read task_off[G], a 21-probe search over task_off[] before each task's first gather: -1.3 ms per proof, DESIGN.md
// §4.2.  Drawing the next ticket one batch early measured slower.)
template <class C, bool TABLE>
__global__ __launch_bounds__(128) void k_accumulate(const uint32_t *sorted, const uint32_t *task_off, const uint4 *tasks,
                                                    const void *points, XYZZ<C> *partials, size_t G, uint32_t *ticket) {
    const uint32_t total = task_off[G];
    const unsigned lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(ticket, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= total) break;
        const uint32_t i = base + lane;
        if (i < total) accumulate_task<C, TABLE>(sorted, tasks[i], points, partials);
    }
}

// ------------------------------------------------------------------------- bucket reduce
// Window sum S_w = sum_b (b+1) * B_b, B_b = sum of the bucket's task partials.  Lane j of the window
// owns RED_K consecutive buckets [jK, jK+K):  sum (b+1) B_b = jK * A + sum_i (i+1) B_{jK+i}  with
// A = running sum (descending), second term = sum of the running sums; jK * A by double-and-add
// (jK < 2^c).  Everything on F28 registers; workgroup LDS tree, then k_sum_parts per window.  RED_K: msm_plan.h.

// sh[threadIdx.x] holds each lane's value on entry; on exit sh[0] holds the workgroup sum
template <class C>
__device__ __forceinline__ void lds_tree_sum(XYZZ28<C> *sh) {
    __syncthreads();
    for (unsigned off = blockDim.x >> 1; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const XYZZ28<C> b = sh[threadIdx.x + off];
            xyzz28_add_into_full<C>(&sh[threadIdx.x], b);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------- hot buckets
// Skewed scalars (the reference's own bench circuit repeats one witness value 2^20 times, benches/bench.rs:
// 49-51) put ~len entries into one bucket per window: the task split keeps k_accumulate balanced, but the
// bucket then owns thousands of task partials, and the reduction's lane would add them one after the other
// (measured: 268 ms).  k_task_counts lists the buckets with many tasks; k_task_fold sums such a bucket's
// partials in parallel into its first slot and sets its effective task count to 1.
//   tier A: more than FOLD_BLOCK_MIN tasks -> one workgroup per bucket;  tier B: more than FOLD_MIN -> one wave.
constexpr uint32_t FOLD_MIN = 8, FOLD_BLOCK_MIN = 1024;

__global__ void k_task_counts(const uint32_t *task_off, size_t G, uint32_t *task_cnt, uint32_t *hot_a, uint32_t *hot_b,
                              uint32_t *hot_counts /*[2], zeroed*/, uint32_t cap) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t n = task_off[g + 1] - task_off[g];
    task_cnt[g] = n;
    if (n > FOLD_BLOCK_MIN) {
        const uint32_t i = atomicAdd(&hot_counts[0], 1u);
        if (i < cap) hot_a[i] = (uint32_t)g;   // an unlisted bucket keeps its sequential sum
    } else if (n > FOLD_MIN) {
        const uint32_t i = atomicAdd(&hot_counts[1], 1u);
        if (i < cap) hot_b[i] = (uint32_t)g;
    }
}

// LANES = 256: one workgroup per listed bucket (tier A);  LANES = 64: one wave per listed bucket (tier B)
template <class C, unsigned LANES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_task_fold(XYZZ<C> *partials, const uint32_t *task_off, uint32_t *task_cnt,
                                                   const uint32_t *hot, const uint32_t *hot_count, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XYZZ28<C> *sh = (XYZZ28<C> *)smem_raw;
    typedef typename C::FqRR RR;
    uint32_t listed = *hot_count;
    if (listed > cap) listed = cap;
    constexpr unsigned GROUPS = 256 / LANES;                       // buckets per workgroup per round
    const unsigned group = threadIdx.x / LANES, lane = threadIdx.x % LANES;
    for (uint32_t h0 = blockIdx.x * GROUPS; h0 < listed; h0 += gridDim.x * GROUPS) {   // uniform trip count per workgroup
        const uint32_t h = h0 + group;
        XYZZ28<C> *acc = &sh[threadIdx.x];
        acc->X = acc->Y = acc->ZZ = acc->ZZZ = f28_zero<RR>();
        uint32_t first = 0, n = 0;
        if (h < listed) {
            first = task_off[hot[h]];
            n = task_off[hot[h] + 1] - first;
            for (uint32_t i = lane; i < n; i += LANES) xyzz28_add_into_full<C>(acc, xyzz28_load<C>(partials[first + i]));
        }
        __syncthreads();
        for (unsigned off = LANES >> 1; off > 0; off >>= 1) {
            if (lane < off) {
                const XYZZ28<C> b = sh[threadIdx.x + off];
                xyzz28_add_into_full<C>(&sh[threadIdx.x], b);
            }
            __syncthreads();
        }
        if (h < listed && lane == 0) {
            partials[first] = xyzz28_store<C>(sh[threadIdx.x]);
            task_cnt[hot[h]] = 1;
        }
        __syncthreads();
    }
}

// Input bucket b = sum of its task partials, weight b + 1 (a Pippenger window).
template <class C>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_bucket_reduce(const XYZZ<C> *partials, const uint32_t *task_off, const uint32_t *task_cnt, unsigned nbuckets,
                                                       unsigned lanes_per_window, unsigned bpw, XYZZ<C> *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XYZZ28<C> *sh = (XYZZ28<C> *)smem_raw;
    typedef typename C::FqRR RR;
    const unsigned w = blockIdx.x / bpw, bw = blockIdx.x % bpw;
    const unsigned j = bw * blockDim.x + threadIdx.x;
    XYZZ28<C> run;
    run.X = run.Y = run.ZZ = run.ZZZ = f28_zero<RR>();
    XYZZ28<C> *acc = &sh[threadIdx.x];     // the weighted accumulator lives in LDS (register pressure)
    *acc = run;
    if (j < lanes_per_window) {
        const size_t gbase = (size_t)w * nbuckets + (size_t)j * RED_K;
        for (int i = (int)RED_K - 1; i >= 0; --i) {
            if ((size_t)j * RED_K + i >= nbuckets) continue;
            for (uint32_t q = task_off[gbase + i], qe = q + task_cnt[gbase + i]; q < qe; ++q) xyzz28_add_full<C>(run, xyzz28_load<C>(partials[q]));
            xyzz28_add_into_full<C>(acc, run);                 // weight i + 1
        }
        const uint32_t s = j * RED_K;          // acc += s * run
        if (s) {
            XYZZ28<C> m = run;
            for (int b = 30 - __clz((int)s); b >= 0; --b) {
                xyzz28_dbl<C>(m);
                if ((s >> b) & 1) xyzz28_add_full<C>(m, run);
            }
            xyzz28_add_into_full<C>(acc, m);
        }
    }
    lds_tree_sum<C>(sh);
    if (threadIdx.x == 0) out[blockIdx.x] = xyzz28_store<C>(sh[0]);
}

// out[w] = sum of parts[w * count .. + count)
template <class C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_sum_parts(const XYZZ<C> *parts, unsigned count, XYZZ<C> *out) {
    __shared__ XYZZ28<C> sh[64];
    typedef typename C::FqRR RR;
    XYZZ28<C> *acc = &sh[threadIdx.x];
    acc->X = acc->Y = acc->ZZ = acc->ZZZ = f28_zero<RR>();
    for (unsigned i = threadIdx.x; i < count; i += 64) xyzz28_add_into_full<C>(acc, xyzz28_load<C>(parts[(size_t)blockIdx.x * count + i]));
    lds_tree_sum<C>(sh);
    if (threadIdx.x == 0) out[blockIdx.x] = xyzz28_store<C>(sh[0]);
}

// =====================================================================================================
// Table mode: the base vector is resident together with its window tables T_w[i] = 2^(c w) P_i
// (setup.hip: tables_build), so every window's digits share ONE set of 2^(c-1) buckets: c = 22 gives
// 12 mixed adds per pair instead of 16, no per-window reduction and no doublings.  2^21 buckets do not
// fit an LDS histogram, so the sort is a three-level MSD radix over (u16 key, u32 table index) entries:
// k_tbl_count / k_block_sums + k_block_offsets / k_tbl_partition (64 regions of 2^15 buckets, atomic-free offsets),
// k_region_pass<HIST> + k_region_pass_staged<MID> (128 sub-regions of 256 buckets), <HIST> + the bucket
// scan + k_region_pass_staged<FINAL>; every scatter is staged through LDS and written out coalesced.
// Reduction: k_reduce_level0 / k_reduce_level1 / k_sum_final (chains of dependent point additions).
// =====================================================================================================
constexpr unsigned LO_BITS = SORT_REGION_BITS;   // msm_plan.h: 2^15 buckets per first-level region

// Inclusive scan of one value per lane across the workgroup (blockDim <= 1024): wave shuffles + one LDS hop
// (2 barriers; the LDS Hillis-Steele it replaces needed 2 log2(n)).  wt: 64 words of LDS scratch.
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t *wt) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    if (lane == 63) wt[wave] = v;
    __syncthreads();
    if (wave == 0) {
        uint32_t w = lane < (blockDim.x >> 6) ? wt[lane] : 0u;
#pragma unroll
        for (unsigned o = 1; o < 16; o <<= 1) {
            const uint32_t n = __shfl_up(w, o, 64);
            if (lane >= o) w += n;
        }
        wt[lane] = w;
    }
    __syncthreads();
    if (wave) v += wt[wave - 1];
    return v;
}

// canonical scalar (zero when the base is the point at infinity -- `inf` holds one flag byte per point of
// window 0, setup.hip: tables_build): digits are then pure bit extraction
template <class P>
__device__ __forceinline__ Fp<P> canon_scalar(const Fp<P> *scalars, const unsigned char *inf, size_t i) {
    Fp<P> k = from_mont<P>(scalars[i]);
    if (inf[i]) k = Fp<P>::zero();
    return k;
}

// signed digit of canonical scalar k in the window of c bits at bit lo (msm_plan.h: win_off / win_width / win_base, called with the
// kernels' NWIN): returns false for a zero digit; bucket = |d| - 1
template <class P>
__device__ __forceinline__ bool digit_at(const Fp<P> &k, unsigned lo, unsigned c, uint32_t &carry, uint32_t &bucket, uint32_t &neg) {
    const uint32_t half = 1u << (c - 1), full = 1u << c, mask = full - 1;
    const unsigned limb = lo >> 5, off = lo & 31;
    uint32_t v = 0;
    if (limb < (unsigned)P::N) {
        uint64_t two = k.l[limb];
        if (limb + 1 < (unsigned)P::N) two |= (uint64_t)k.l[limb + 1] << 32;
        v = (uint32_t)(two >> off) & mask;
    }
    // branch-free: the callers unroll this over compile-time (lo, c), lane divergence here would cost
    // an exec-mask region per window
    const uint32_t d = v + carry;
    const bool over = d > half;
    const uint32_t m = over ? full - d : d;
    carry = over ? 1u : 0u;
    neg = carry;
    bucket = m - 1;
    return m != 0;
}

// k_digits over a batch of scalar rows against ONE base range (msm_run_batch): lane i recodes scalar i of row blockIdx.y into set
// s = row * nwin + w, whose digits are digits[s * len ..): stores coalesced along i.  inf[i] = 1 for a base at infinity
// (setup.hip: infinity_flags, once per call, not once per row).
template <class C>
__global__ __launch_bounds__(256) void k_digits_batch(const Fp<typename C::FrP> *scalars, const unsigned char *inf, uint32_t *digits, size_t len,
                                                      unsigned c, unsigned nwin) {
    typedef typename C::FrP P;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const size_t row = blockIdx.y;
    const Fp<P> k = from_mont<P>(scalars[row * len + i]);
    const bool skip = inf[i] != 0;
    uint32_t carry = 0;
    uint32_t *d = digits + row * nwin * len + i;
#pragma unroll 1
    for (unsigned w = 0; w < nwin; ++w) {
        uint32_t bucket, neg;
        const bool some = digit_at<P>(k, w * c, c, carry, bucket, neg);
        d[(size_t)w * len] = some && !skip ? (bucket << 1) | neg : DIGIT_NONE;
    }
}

// Region populations PER WORKGROUP: block_cnt[workgroup][region], with the same workgroup -> scalar mapping
// as k_tbl_partition (one scalar per lane).  A column-wise scan (k_block_sums, k_block_offsets) turns them into each
// workgroup's offset inside each region, so neither kernel touches a global atomic: 41 K workgroups x 64
// regions hammering 64 addresses serialised in L2 and cost more than the rest of the kernel.
// M: the radix's multiplier (internal.h: MsmTables::m).  M = 5: the digits of radix 5 2^a (radix.cuh), a = the shift of (field, NWIN),
// one shared bucket set -- dg[w] = bucket << 1 | negate, so the region of a digit is dg >> (LO_BITS + 1).
template <class P, unsigned NWIN, unsigned M>
__global__ __launch_bounds__(1024) void k_tbl_count(const Fp<P> *scalars, const unsigned char *inf, size_t len, unsigned regions,
                                                   uint32_t *block_cnt, uint32_t win_buckets, uint32_t narrow_buckets) {
    __shared__ uint32_t cnt[SORT_MAX_REGIONS];
    for (unsigned r = threadIdx.x; r < regions; r += blockDim.x) cnt[r] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) {
        const Fp<P> k = canon_scalar<P>(scalars, inf, i);
        if constexpr (M == 5) {
            uint32_t dg[NWIN];
            radix5_recode<NWIN, radix_min_shift<P>(5, NWIN)>(k.l, dg);
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (dg[w] != RADIX_NO_DIGIT) atomicAdd(&cnt[dg[w] >> (LO_BITS + 1)], 1u);
        } else {
            uint32_t carry = 0, b, neg;
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (digit_at<P>(k, win_off(NWIN, w), win_width(NWIN, w), carry, b, neg)) atomicAdd(&cnt[(b + win_base(NWIN, w, win_buckets, narrow_buckets)) >> LO_BITS], 1u);
        }
    }
    __syncthreads();
    for (unsigned r = threadIdx.x; r < regions; r += blockDim.x) block_cnt[(size_t)blockIdx.x * regions + r] = cnt[r];
}

// block_cnt[nblocks][regions] -> per region the exclusive prefix over the workgroups (in place), totals -> region_count.
// Two launches of G workgroups.  Workgroup g owns the block rows [g span, (g + 1) span); lane (j, r) = (t / regions, t % regions),
// j < rows <= 16, owns `per` consecutive rows of region r, so a wave reads 64 consecutive regions of one row: whole cache lines.
// (Round 2's form -- one workgroup per REGION, every lane striding through the rows of its column -- kept 64 CUs busy with
// uncoalesced 4-byte loads: 0.16 ms at 41 K rows x 64 regions, profiles/r03_final_rocprofv3_kernel_stats_bench_2p20.csv.)
struct BlockScanShape { unsigned G, span, rows, per; };
static BlockScanShape block_scan_shape(unsigned nblocks, unsigned regions) {
    BlockScanShape h;
    h.rows = 1024 / regions < 16 ? 1024 / regions : 16;
    if (h.rows < 1) h.rows = 1;
    h.G = (nblocks + 15) / 16 < 256 ? (nblocks + 15) / 16 : 256;
    if (h.G < 1) h.G = 1;
    h.span = (nblocks + h.G - 1) / h.G;
    h.per = (h.span + h.rows - 1) / h.rows;
    return h;
}
__device__ __forceinline__ void block_scan_range(unsigned g, unsigned j, BlockScanShape h, unsigned nblocks, unsigned &lo, unsigned &hi) {
    const unsigned end = (g + 1) * h.span < nblocks ? (g + 1) * h.span : nblocks;
    lo = g * h.span + j * h.per;
    hi = lo + h.per < end ? lo + h.per : end;
}
__global__ __launch_bounds__(1024) void k_block_sums(const uint32_t *block_cnt, unsigned nblocks, unsigned regions, BlockScanShape h, uint32_t *partial) {
    __shared__ uint32_t s[1024];
    const unsigned t = threadIdx.x, j = t / regions, r = t % regions;
    if (j < h.rows) {
        unsigned lo, hi;
        block_scan_range(blockIdx.x, j, h, nblocks, lo, hi);
        uint32_t sum = 0;
        for (unsigned b = lo; b < hi; ++b) sum += block_cnt[(size_t)b * regions + r];
        s[t] = sum;
    }
    __syncthreads();
    if (t < regions) {
        uint32_t tot = 0;
        for (unsigned jj = 0; jj < h.rows; ++jj) tot += s[jj * regions + t];
        partial[(size_t)blockIdx.x * regions + t] = tot;
    }
}
__global__ __launch_bounds__(1024) void k_block_offsets(uint32_t *block_cnt, unsigned nblocks, unsigned regions, BlockScanShape h, const uint32_t *partial,
                                                        uint32_t *region_count) {
    __shared__ uint32_t s[1024], base[1024];
    const unsigned t = threadIdx.x, j = t / regions, r = t % regions, g = blockIdx.x;
    if (j < h.rows) {                                   // the earlier workgroups' totals, rows-way split
        uint32_t acc = 0;
        for (unsigned q = j; q < g; q += h.rows) acc += partial[(size_t)q * regions + r];
        s[t] = acc;
    }
    __syncthreads();
    if (t < regions) {
        uint32_t tot = 0;
        for (unsigned jj = 0; jj < h.rows; ++jj) tot += s[jj * regions + t];
        base[t] = tot;
    }
    __syncthreads();
    unsigned lo = 0, hi = 0;
    if (j < h.rows) {
        block_scan_range(g, j, h, nblocks, lo, hi);
        uint32_t sum = 0;
        for (unsigned b = lo; b < hi; ++b) sum += block_cnt[(size_t)b * regions + r];
        s[t] = sum;
    }
    __syncthreads();
    if (j < h.rows) {
        uint32_t run = base[r];
        for (unsigned jj = 0; jj < j; ++jj) run += s[jj * regions + r];
        for (unsigned b = lo; b < hi; ++b) {
            const uint32_t v = block_cnt[(size_t)b * regions + r];
            block_cnt[(size_t)b * regions + r] = run;
            run += v;
        }
    }
    if (g == gridDim.x - 1 && t < regions) {
        uint32_t tot = base[t];
        for (unsigned jj = 0; jj < h.rows; ++jj) tot += s[jj * regions + t];
        region_count[t] = tot;
    }
}

// region_off = exclusive scan of region_count (regions <= 1024); also clears the claim cursors
__global__ __launch_bounds__(1024) void k_region_offsets(const uint32_t *region_count, uint32_t *region_off, uint32_t *region_cursor,
                                                         unsigned regions) {
    __shared__ uint32_t s[1024];
    const unsigned t = threadIdx.x;
    uint32_t v = t < regions ? region_count[t] : 0u;
    s[t] = v;
    __syncthreads();
    for (unsigned off = 1; off < 1024; off <<= 1) {
        uint32_t a = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    if (t < regions) { region_off[t] = s[t] - v; region_cursor[t] = 0; }
    if (t == 1023) region_off[regions] = s[1023];
}

// entry (i, w) -> region of its bucket: key = low LO_BITS of the bucket, val = table index << 1 | negate.
// One scalar per lane.  The workgroup's entries are staged through LDS in region order so that the global
// stores are coalesced (consecutive lanes -> consecutive addresses of a region's run).
//   LDS: cnt[SORT_MAX_REGIONS] | delta[SORT_MAX_REGIONS] | staged vals (u32 x blockDim nwin) | staged region<<16|key (u32 x same)
template <class P, unsigned NWIN, unsigned M>
__global__ __launch_bounds__(1024) void k_tbl_partition(const Fp<P> *scalars, const unsigned char *inf, size_t len,
                                                       unsigned regions, const uint32_t *region_off, const uint32_t *block_off, size_t tbl_stride, size_t base_index, uint16_t *keys,
                                                       uint32_t *vals, uint32_t win_buckets, uint32_t narrow_buckets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *cnt = (uint32_t *)smem_raw, *delta = cnt + SORT_MAX_REGIONS;
    uint32_t *st_val = delta + 1024, *st_key = st_val + (size_t)blockDim.x * NWIN;
    __shared__ uint32_t tot, wt[64];
    const unsigned t = threadIdx.x, BD = blockDim.x;
    for (unsigned r = t; r < regions; r += BD) cnt[r] = 0;
    __syncthreads();
    // pass 1: count per region -- the counting atomic returns the entry's rank inside this workgroup, kept in
    // registers (NWIN per lane) so that pass 2 needs no second LDS atomic
    const size_t i = (size_t)blockIdx.x * BD + t;
    uint32_t rank[NWIN];
    uint32_t dg[M == 5 ? NWIN : 1];     // M = 5: the digits are recoded once and kept (bucket << 1 | negate, radix.cuh)
    Fp<P> k = Fp<P>::zero();
    if (i < len) {
        k = canon_scalar<P>(scalars, inf, i);
        if constexpr (M == 5) {
            radix5_recode<NWIN, radix_min_shift<P>(5, NWIN)>(k.l, dg);
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (dg[w] != RADIX_NO_DIGIT) rank[w] = atomicAdd(&cnt[dg[w] >> (LO_BITS + 1)], 1u);
        } else {
            uint32_t carry = 0, b, neg;
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (digit_at<P>(k, win_off(NWIN, w), win_width(NWIN, w), carry, b, neg)) rank[w] = atomicAdd(&cnt[(b + win_base(NWIN, w, win_buckets, narrow_buckets)) >> LO_BITS], 1u);
        }
    }
    __syncthreads();
    {   // exclusive scan over the regions: lane t owns region t (regions <= blockDim, checked by the host: bucket_plan)
        const uint32_t c = t < regions ? cnt[t] : 0u;
        const uint32_t incl = block_inclusive_scan(c, wt);
        if (t < regions) {
            const uint32_t ex = incl - c;
            cnt[t] = ex;                                                                  // first staged slot of the region
            delta[t] = region_off[t] + block_off[(size_t)blockIdx.x * regions + t] - ex;  // global = delta[region] + slot
        }
        if (t == BD - 1) tot = incl;
    }
    __syncthreads();
    if (i < len) {
        if constexpr (M == 5) {
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (dg[w] != RADIX_NO_DIGIT) {
                    const uint32_t b = dg[w] >> 1, rg = b >> LO_BITS, slot = cnt[rg] + rank[w];
                    st_key[slot] = (rg << 16) | (b & ((1u << LO_BITS) - 1));
                    st_val[slot] = (uint32_t)(((size_t)w * tbl_stride + base_index + i) << 1) | (dg[w] & 1u);
                }
        } else {
            uint32_t carry = 0, b, neg;
#pragma unroll
            for (unsigned w = 0; w < NWIN; ++w)
                if (digit_at<P>(k, win_off(NWIN, w), win_width(NWIN, w), carry, b, neg)) {
                    b += win_base(NWIN, w, win_buckets, narrow_buckets);
                    const uint32_t rg = b >> LO_BITS, slot = cnt[rg] + rank[w];
                    st_key[slot] = (rg << 16) | (b & ((1u << LO_BITS) - 1));
                    st_val[slot] = (uint32_t)(((size_t)w * tbl_stride + base_index + i) << 1) | neg;
                }
        }
    }
    __syncthreads();
    const uint32_t total = tot;
    for (uint32_t s = t; s < total; s += BD) {
        const uint32_t kv = st_key[s], pos = delta[kv >> 16] + s;
        keys[pos] = (uint16_t)kv;
        vals[pos] = st_val[s];
    }
}

// Levels 2 and 3: one generic LDS-staged pass over a segment-partitioned (key, val) array.  Workgroup
// `blockIdx.x` owns entries [x CH, (x+1) CH) and handles each segment piece inside it: bin = key >> bin_shift
// (nbins per segment, global bin id = segment * nbins + bin).
//   RS_HIST : counts[global bin] += occurrences
//   RS_MID  : entries move to (keys_out, vals_out) at out_off[global bin] + rank, key keeps its low bin_shift bits
//             (k_region_pass_staged only; k_region_pass keeps the two output arguments of its launch, unused)
//   RS_FINAL: sorted[out_off[global bin] + rank] = val
// With 64 regions -> 128 sub-regions -> 256 buckets every pass writes runs of ~100+ entries per bin instead
// of single scattered words (the two-level version spent most of its time on 4-byte scattered stores).
enum { RS_HIST = 0, RS_MID = 1, RS_FINAL = 2 };
constexpr unsigned ST_MAX_BINS_HIST = 256;   // k_hist_small: bins per segment
constexpr unsigned RS_CHUNK_LOG = 15, RS_PER_LANE = (1u << RS_CHUNK_LOG) / 1024;   // entries per lane of a 1024-lane workgroup

template <int MODE>
__global__ __launch_bounds__(1024) void k_region_pass(const uint16_t *keys, const uint32_t *vals, const uint32_t *seg_off,
                                                      unsigned nseg, unsigned bin_shift, unsigned nbins, unsigned chunk,
                                                      uint32_t *counts, const uint32_t *out_off, uint32_t *cursor,
                                                      uint32_t *sorted, uint16_t * /*keys_out*/, uint32_t * /*vals_out*/) {
    static_assert(MODE == RS_HIST || MODE == RS_FINAL, "the middle level runs staged (k_region_pass_staged<RS_MID>)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *h = (uint32_t *)smem_raw;
    const uint32_t total = seg_off[nseg];
    const uint32_t lo = blockIdx.x * chunk;
    if (lo >= total) return;
    uint32_t hi = lo + chunk;
    if (hi > total) hi = total;
    unsigned ra = 0, rb = nseg;   // segment containing `lo`: largest r with seg_off[r] <= lo
    while (rb - ra > 1) {
        unsigned mid = (ra + rb) >> 1;
        if (seg_off[mid] <= lo) ra = mid; else rb = mid;
    }
    for (unsigned r = ra; r < nseg; ++r) {
        const uint32_t s0 = seg_off[r] > lo ? seg_off[r] : lo;
        const uint32_t s1 = seg_off[r + 1] < hi ? seg_off[r + 1] : hi;
        if (s0 >= hi) break;
        if (s0 >= s1) continue;
        for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) h[b] = 0;
        __syncthreads();
        const size_t gbase = (size_t)r * nbins;
        if (MODE == RS_HIST) {
            for (uint32_t e = s0 + threadIdx.x; e < s1; e += blockDim.x) atomicAdd(&h[keys[e] >> bin_shift], 1u);
            __syncthreads();
            for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) {
                uint32_t v = h[b];
                if (v) atomicAdd(&counts[gbase + b], v);
            }
        } else {
            // the counting atomic already returns the entry's rank inside this workgroup: keep it in a
            // register (<= RS_PER_LANE entries per lane) instead of a second LDS atomic per entry
            uint32_t rank[RS_PER_LANE];
            uint16_t key[RS_PER_LANE];
#pragma unroll
            for (unsigned q = 0; q < RS_PER_LANE; ++q) {
                const uint32_t e = s0 + q * blockDim.x + threadIdx.x;
                if (e < s1) {
                    key[q] = keys[e];
                    rank[q] = atomicAdd(&h[key[q] >> bin_shift], 1u);
                }
            }
            __syncthreads();
            for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) {
                uint32_t v = h[b];
                if (v) h[b] = out_off[gbase + b] + atomicAdd(&cursor[gbase + b], v);
            }
            __syncthreads();
#pragma unroll
            for (unsigned q = 0; q < RS_PER_LANE; ++q) {
                const uint32_t e = s0 + q * blockDim.x + threadIdx.x;
                if (e < s1) sorted[h[key[q] >> bin_shift] + rank[q]] = vals[e];
            }
        }
        __syncthreads();
    }
}

// Histogram for SMALL bin counts (<= 256): counts[segment * nbins + (key >> bin_shift)] += 1.  Every wave counts
// into its own LDS copy: with one shared copy the 1024 lanes of a workgroup pile onto 128-256 addresses and the
// LDS serialises them (0.30 ms per pass over 252 M keys; the data is only 0.5 GB).
__global__ __launch_bounds__(1024) void k_hist_small(const uint16_t *keys, const uint32_t *seg_off, unsigned nseg, unsigned bin_shift,
                                                     unsigned nbins, unsigned chunk, uint32_t *counts) {
    __shared__ uint32_t h[16][ST_MAX_BINS_HIST];
    const uint32_t total = seg_off[nseg];
    const uint32_t lo = blockIdx.x * chunk;
    if (lo >= total) return;
    uint32_t hi = lo + chunk;
    if (hi > total) hi = total;
    unsigned ra = 0, rb = nseg;
    while (rb - ra > 1) {
        unsigned mid = (ra + rb) >> 1;
        if (seg_off[mid] <= lo) ra = mid; else rb = mid;
    }
    const unsigned wave = threadIdx.x >> 6;
    for (unsigned r = ra; r < nseg; ++r) {
        const uint32_t s0 = seg_off[r] > lo ? seg_off[r] : lo;
        const uint32_t s1 = seg_off[r + 1] < hi ? seg_off[r + 1] : hi;
        if (s0 >= hi) break;
        if (s0 >= s1) continue;
        for (unsigned b = threadIdx.x; b < 16 * ST_MAX_BINS_HIST; b += blockDim.x) (&h[0][0])[b] = 0;
        __syncthreads();
        // 8 keys per 16-byte load over the aligned body of the piece; scalar head and tail
        const uint32_t b0 = (s0 + 7u) & ~7u, b1 = s1 & ~7u;
        if (b0 < b1) {
            for (uint32_t e = s0 + threadIdx.x; e < b0; e += blockDim.x) atomicAdd(&h[wave][keys[e] >> bin_shift], 1u);
            for (uint32_t e = b0 + threadIdx.x * 8u; e < b1; e += blockDim.x * 8u) {
                const uint4 v = *(const uint4 *)(keys + e);
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    atomicAdd(&h[wave][(w4[q] & 0xffffu) >> bin_shift], 1u);
                    atomicAdd(&h[wave][(w4[q] >> 16) >> bin_shift], 1u);
                }
            }
            for (uint32_t e = b1 + threadIdx.x; e < s1; e += blockDim.x) atomicAdd(&h[wave][keys[e] >> bin_shift], 1u);
        } else {
            for (uint32_t e = s0 + threadIdx.x; e < s1; e += blockDim.x) atomicAdd(&h[wave][keys[e] >> bin_shift], 1u);
        }
        __syncthreads();
        for (unsigned b = threadIdx.x; b < nbins; b += blockDim.x) {
            uint32_t v = 0;
#pragma unroll
            for (unsigned w = 0; w < 16; ++w) v += h[w][b];
            if (v) atomicAdd(&counts[(size_t)r * nbins + b], v);
        }
        __syncthreads();
    }
}

// The same pass for SMALL bin counts (<= 256), with the chunk staged through LDS in bin order so that
// the global stores are coalesced: consecutive lanes write consecutive addresses of a bin's run
// (the direct version above issues 64 scattered 4-byte stores per wave-instruction).
//   LDS: h[nbins] | start[nbins] | delta[nbins] | staged vals (u32 x ST_CHUNK) | staged keys (u16 x ST_CHUNK)
// 1024 lanes x 8 entries: the workgroup shapes swept after the 16-byte loads went in, profiles/r05_sort_chunk_shapes_after_wide_loads.txt
constexpr unsigned ST_THREADS = 1024, ST_PER_LANE = 8, ST_CHUNK = ST_PER_LANE * ST_THREADS, ST_MAX_BINS = 256;

template <int MODE>
__global__ __launch_bounds__(ST_THREADS) void k_region_pass_staged(const uint16_t *keys, const uint32_t *vals, const uint32_t *seg_off,
                                                             unsigned nseg, unsigned bin_shift, unsigned nbins,
                                                             const uint32_t *out_off, uint32_t *cursor, uint32_t *sorted,
                                                             uint16_t *keys_out, uint32_t *vals_out) {
    __shared__ uint32_t h[ST_MAX_BINS], delta[ST_MAX_BINS], wt[64];
    __shared__ uint32_t st_val[ST_CHUNK];
    __shared__ uint16_t st_key[ST_CHUNK];
    const uint32_t total = seg_off[nseg];
    const uint32_t lo = blockIdx.x * ST_CHUNK;
    if (lo >= total) return;
    uint32_t hi = lo + ST_CHUNK;
    if (hi > total) hi = total;
    unsigned ra = 0, rb = nseg;
    while (rb - ra > 1) {
        unsigned mid = (ra + rb) >> 1;
        if (seg_off[mid] <= lo) ra = mid; else rb = mid;
    }
    const uint16_t low_mask = (uint16_t)((1u << bin_shift) - 1);
    const unsigned t = threadIdx.x;
    for (unsigned r = ra; r < nseg; ++r) {
        const uint32_t s0 = seg_off[r] > lo ? seg_off[r] : lo;
        const uint32_t s1 = seg_off[r + 1] < hi ? seg_off[r + 1] : hi;
        if (s0 >= hi) break;
        if (s0 >= s1) continue;
        const uint32_t cnt = s1 - s0;
        if (t < nbins) h[t] = 0;
        __syncthreads();
        // Round 5: a lane takes EIGHT CONSECUTIVE entries with three 16-byte loads (8 keys, 2 x 4 values) instead of eight strided
        // 2-byte + eight 4-byte ones.  The passes are bound by the number of vector-memory instructions, not by bytes (13.4 M wave
        // instructions for 2.4 GB per pass at ~3.3 TB/s; the address coalescer takes a wave's 64 lanes in 16 clocks whatever their
        // width): 16 -> 3 load instructions per lane.  The piece [s0, s1) is widened down to a multiple of 8 entries so that the loads are
        // aligned (the buffers are; a piece starts inside the chunk, so the workgroup's lanes still cover it); `vm` masks the entries outside it.
        uint32_t rank[ST_PER_LANE], val[ST_PER_LANE];
        uint16_t key[ST_PER_LANE];
        static_assert(ST_PER_LANE % 8 == 0, "whole uint4s of keys per lane");
        const uint32_t e0 = (s0 & ~(ST_PER_LANE - 1u)) + ST_PER_LANE * t;
        uint32_t vm = 0;
        if (e0 < s1 && e0 + ST_PER_LANE > s0) {
            uint32_t kw[ST_PER_LANE / 2], vw[ST_PER_LANE];
#pragma unroll
            for (unsigned g = 0; g < ST_PER_LANE / 8; ++g) {
                const uint4 kv = *(const uint4 *)(keys + e0 + 8 * g);
                kw[4 * g] = kv.x; kw[4 * g + 1] = kv.y; kw[4 * g + 2] = kv.z; kw[4 * g + 3] = kv.w;
            }
#pragma unroll
            for (unsigned g = 0; g < ST_PER_LANE / 4; ++g) {
                const uint4 va = *(const uint4 *)(vals + e0 + 4 * g);
                vw[4 * g] = va.x; vw[4 * g + 1] = va.y; vw[4 * g + 2] = va.z; vw[4 * g + 3] = va.w;
            }
#pragma unroll
            for (unsigned q = 0; q < ST_PER_LANE; ++q) {
                const uint32_t e = e0 + q;
                key[q] = (uint16_t)(kw[q >> 1] >> (16 * (q & 1)));
                val[q] = vw[q];
                if (e >= s0 && e < s1) {
                    vm |= 1u << q;
                    rank[q] = atomicAdd(&h[key[q] >> bin_shift], 1u);
                }
            }
        }
        __syncthreads();
        {   // exclusive scan of h over the bins (lane b owns bin b); claim the global runs
            const uint32_t c = t < nbins ? h[t] : 0u;
            const uint32_t incl = block_inclusive_scan(c, wt);
            if (t < nbins) {
                const uint32_t ex = incl - c;
                const size_t g = (size_t)r * nbins + t;
                const uint32_t gpos = c ? out_off[g] + atomicAdd(&cursor[g], c) : 0u;
                delta[t] = gpos - ex;                          // global position = delta[bin] + staged slot
                h[t] = ex;                                     // h now = local start of the bin
            }
        }
        __syncthreads();
#pragma unroll
        for (unsigned q = 0; q < ST_PER_LANE; ++q) {
            if ((vm >> q) & 1u) {
                const uint32_t slot = h[key[q] >> bin_shift] + rank[q];
                st_key[slot] = key[q];
                st_val[slot] = val[q];
            }
        }
        __syncthreads();
        // (Pair stores -- every bin's staged run at its destination's parity inside an even-sized area, two keys in one 4-byte and two
        // values in one 8-byte store, the <= 2 singles per bin in a second sweep -- were built and measured: parity-green, 2.43 -> 2.48 ms
        // for the sort of a 2^24-pair MSM.  Stores do not wait for anything; the loads did.  profiles/r05_sort_pair_stores_negative.txt)
        for (uint32_t i = t; i < cnt; i += ST_THREADS) {
            const uint16_t k = st_key[i];
            const uint32_t pos = delta[k >> bin_shift] + i;
            if (MODE == RS_FINAL) {
                sorted[pos] = st_val[i];
            } else {
                keys_out[pos] = k & low_mask;
                vals_out[pos] = st_val[i];
            }
        }
        __syncthreads();
    }
}

// exclusive scan of n <= 2^20 counters by one workgroup (sub-region offsets); off[n] = total; clears `zero`
__global__ __launch_bounds__(1024) void k_scan_small(const uint32_t *cnt, uint32_t *off, uint32_t *zero, unsigned n) {
    __shared__ uint32_t s[1024];
    __shared__ uint32_t carry;
    const unsigned t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (unsigned base = 0; base < n; base += 1024) {
        const unsigned i = base + t;
        const uint32_t v = i < n ? cnt[i] : 0u;
        s[t] = v;
        __syncthreads();
        for (unsigned o = 1; o < 1024; o <<= 1) {
            uint32_t a = t >= o ? s[t - o] : 0u;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (i < n) { off[i] = carry + s[t] - v; zero[i] = 0; }
        __syncthreads();
        if (t == 1023) carry += s[1023];
        __syncthreads();
    }
    if (t == 0) off[n] = carry;
}

// The plan every stage below reads -- BucketPlan, made by bucket_plan from the MSM's layout before the first launch -- is msm_plan.h's.
// ------------------------------------------------------------------------------- shared stages
// Each takes the context, the bucket set and the plan, and enqueues on ctx->stream.

// the set's buffers, the scan's tile totals
template <class C>
static int reserve_set(pm_ctx *ctx, MsmSet &S, const BucketPlan &p) {
    PM_HIP(ctx, S.sorted.reserve(p.E * 4 + 16));      // + 16: k_accumulate reads aligned quads of indices
    PM_HIP(ctx, S.counts.reserve(2 * p.NB * 4));      // counts | cursor, one memset
    PM_HIP(ctx, S.bucket_off.reserve((p.NB + 1) * 4));
    PM_HIP(ctx, S.task_off.reserve((p.NB + 1) * 4));
    PM_HIP(ctx, S.partials.reserve(p.max_tasks * sizeof(XYZZ<C>)));
    PM_HIP(ctx, S.task_cnt.reserve(p.NB * 4));
    PM_HIP(ctx, ctx->msm.cursor.reserve(((p.NB + SCAN_TILE - 1) / SCAN_TILE + 1) * 8));
    return PM_OK;
}

// bucket_off / task_off from the set's counts (k_scan_tiles)
static int bucket_scan(pm_ctx *ctx, MsmSet &S, const BucketPlan &p) {
    uint32_t *tile_tot = ctx->msm.cursor.as<uint32_t>(), *bucket_off = S.bucket_off.as<uint32_t>(), *task_off = S.task_off.as<uint32_t>();
    const unsigned ntiles = (unsigned)((p.NB + SCAN_TILE - 1) / SCAN_TILE);
    PM_LAUNCH(ctx, k_scan_tiles, dim3(ntiles), dim3(256), 0, ctx->stream, S.counts.as<uint32_t>(), bucket_off, task_off, tile_tot, p.NB,
                   (unsigned)p.seg);
    PM_LAUNCH(ctx, k_scan_totals, dim3(1), dim3(1024), 0, ctx->stream, tile_tot, ntiles, bucket_off, task_off, p.NB);
    PM_LAUNCH(ctx, k_scan_add, dim3(ntiles), dim3(256), 0, ctx->stream, bucket_off, task_off, tile_tot, p.NB);
    return PM_OK;
}

// effective task counts for the reduction + parallel fold of hot buckets (k_task_counts / k_task_fold);
// enqueued after k_accumulate, before the bucket reduction
template <class C>
static int fold_hot_buckets(pm_ctx *ctx, MsmSet &S, const BucketPlan &p) {
    MsmWorkspace &ws = ctx->msm;
    const size_t G = p.NB;
    size_t cap = p.max_tasks > G ? p.max_tasks - G + 1 : 1;          // a listed bucket has > FOLD_MIN tasks
    cap = cap / FOLD_MIN + 1;
    PM_HIP(ctx, ws.hot.reserve((2 * cap + 2) * 4));
    uint32_t *hot_counts = ws.hot.as<uint32_t>(), *hot_a = hot_counts + 2, *hot_b = hot_a + cap;
    PM_HIP(ctx, hipMemsetAsync(hot_counts, 0, 8, ctx->stream));
    PM_LAUNCH(ctx, k_task_counts, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream, S.task_off.as<uint32_t>(), G,
                   S.task_cnt.as<uint32_t>(), hot_a, hot_b, hot_counts, (uint32_t)cap);
    PM_LAUNCH(ctx, (k_task_fold<C, 256>), dim3(256), dim3(256), 256 * sizeof(XYZZ28<C>), ctx->stream, S.partials.as<XYZZ<C>>(),
                   S.task_off.as<uint32_t>(), S.task_cnt.as<uint32_t>(), hot_a, hot_counts, (uint32_t)cap);
    PM_LAUNCH(ctx, (k_task_fold<C, 64>), dim3(1024), dim3(256), 256 * sizeof(XYZZ28<C>), ctx->stream, S.partials.as<XYZZ<C>>(),
                   S.task_off.as<uint32_t>(), S.task_cnt.as<uint32_t>(), hot_b, hot_counts + 1, (uint32_t)cap);
    return PM_OK;
}

// tasks[] for k_accumulate (see k_task_bins); enqueued on the context's stream after the bucket scan.  Also zeroes the context's
// accumulate ticket (the word in front of the length bins: one memset for both).
static int task_order(pm_ctx *ctx, MsmSet &S, const BucketPlan &p) {
    MsmWorkspace &ws = ctx->msm;
    const size_t G = p.NB, seg = p.seg;
    const uint32_t *counts = S.counts.as<uint32_t>();
    unsigned lshift = 0;
    while (((seg - 1) >> lshift) + 1 > TASK_MAX_BINS) ++lshift;
    const unsigned nbins = (unsigned)(((seg - 1) >> lshift) + 1);
    PM_HIP(ctx, S.tasks.reserve(p.max_tasks * sizeof(uint4)));
    PM_HIP(ctx, ws.len_bins.reserve((3 * (size_t)nbins + 5) * 4));
    uint32_t *ticket = ws.len_bins.as<uint32_t>(), *len_cnt = ticket + 1, *len_off = len_cnt + nbins, *len_cursor = len_off + nbins + 1;
    PM_HIP(ctx, hipMemsetAsync(ticket, 0, ((size_t)nbins + 1) * 4, ctx->stream));
    const unsigned blocks = (unsigned)((G + 1023) / 1024);      // one lane per bucket
    PM_LAUNCH(ctx, k_task_bins<false>, dim3(blocks), dim3(1024), nbins * 4, ctx->stream, counts, S.bucket_off.as<uint32_t>(),
                   S.task_off.as<uint32_t>(), G, (unsigned)seg, lshift, nbins, len_cnt, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                   (uint4 *)nullptr);
    PM_LAUNCH(ctx, k_scan_small, dim3(1), dim3(1024), 0, ctx->stream, len_cnt, len_off, len_cursor, nbins);
    PM_LAUNCH(ctx, k_task_bins<true>, dim3(blocks), dim3(1024), nbins * 4, ctx->stream, counts, S.bucket_off.as<uint32_t>(),
                   S.task_off.as<uint32_t>(), G, (unsigned)seg, lshift, nbins, (uint32_t *)nullptr, len_off, len_cursor,
                   S.tasks.as<uint4>());
    return PM_OK;
}

// k_accumulate over the tasks[] that task_order enqueued: a grid of as many 128-lane workgroups as the device holds at once (no
// more than max_tasks lanes); the waves draw the tasks from the ticket that task_order zeroed.
template <class C, bool TABLE>
static int accumulate(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const void *points) {
    int per_cu = 0, cus = 0;
    PM_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_accumulate<C, TABLE>, 128, 0));
    PM_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    size_t blocks = (size_t)(per_cu > 0 ? per_cu : 1) * (size_t)(cus > 0 ? cus : 1);
    if (blocks > (p.max_tasks + 127) / 128) blocks = (p.max_tasks + 127) / 128;
    PM_LAUNCH(ctx, (k_accumulate<C, TABLE>), dim3((unsigned)blocks), dim3(128), 0, ctx->stream, S.sorted.as<uint32_t>(),
                   S.task_off.as<uint32_t>(), S.tasks.as<uint4>(), points, S.partials.as<XYZZ<C>>(), p.NB, ctx->msm.len_bins.as<uint32_t>());
    return PM_OK;
}

// Single-level reduction (k_bucket_reduce + k_sum_parts) of n_wide_sets sets of NB1 buckets: the windows of the per-window pipeline,
// or a shared set too small for msm_reduce.hip.  *out = the sets' sums, internal form, inside the workspace.
template <class C>
static int reduce_single_level(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, XYZZ<C> **out) {
    const unsigned sets = p.n_wide_sets;
    PM_HIP(ctx, ctx->msm.wsum.reserve(((size_t)sets * p.bpw + sets) * sizeof(XYZZ<C>)));
    XYZZ<C> *parts = ctx->msm.wsum.as<XYZZ<C>>(), *sums = parts + (size_t)sets * p.bpw;
    PM_LAUNCH(ctx, k_bucket_reduce<C>, dim3(sets * p.bpw), dim3(p.red_block), p.red_block * sizeof(XYZZ28<C>), ctx->stream,
                   S.partials.as<XYZZ<C>>(), S.task_off.as<uint32_t>(), S.task_cnt.as<uint32_t>(), (unsigned)p.NB1, p.red_lanes, p.bpw, parts);
    PM_LAUNCH(ctx, k_sum_parts<C>, dim3(sets), dim3(64), 0, ctx->stream, parts, p.bpw, sums);
    *out = sums;
    return PM_OK;
}

// Final combine on the host, two steps.  host_horner: sum_w 2^(off_w) S_w from the top window down -- width[w] doublings in front
// of S_w -- an O(256) dependent chain on nsums points (9 ms on one GPU lane, ~0.3 ms here); a single sum is the case of one window
// of width 0.  host_finish: the infinity flag and one inversion to affine.
template <class C>
static XYZZ<C> host_horner(const XYZZ<C> *sums /*[nsums], internal form*/, unsigned nsums, const unsigned char *width) {
    XYZZ<C> acc = XYZZ<C>::identity();
    for (int w = (int)nsums - 1; w >= 0; --w) {
        for (unsigned k = 0; k < width[w]; ++k) acc = xyzz_dbl<C>(acc);
        acc = xyzz_add<C>(acc, xyzz_internal_to_std<C>(sums[w]));
    }
    return acc;
}
template <class C>
static void host_finish(const XYZZ<C> &acc, Affine<C> *out, int *inf) {
    *inf = acc.is_identity() ? 1 : 0;
    *out = xyzz_to_affine<C>(acc);
}

// The same combine on the device, one lane per row of a batch (msm_run_batch): sums[row * nwin + w] = S_w of that row, internal form;
// out[row] = sum_w 2^(c w) S_w as a standard-Montgomery affine point (all-zero for the identity) and its infinity flag.  The chain is
// host_horner's: c doublings, then one addition per window, on the reduced-radix registers of the bucket reduction.  The window sums of
// structured inputs (bases G, 2G, 3G ..., equal or opposite rows) coincide, cancel or are O: every addition is xyzz28_add_full, which
// hands P = +-Q to the complete dense formulas; xyzz28_dbl is complete (no point of order 2); O is ZZ == 0 in every limb throughout.
template <class C>
__global__ __launch_bounds__(64) void k_window_combine(const XYZZ<C> *sums, unsigned nwin, unsigned c, unsigned rows, BatchPoint<C> *out) {
    typedef typename C::FqRR RR;
    const unsigned row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const XYZZ<C> *s = sums + (size_t)row * nwin;
    XYZZ28<C> acc;
    acc.X = acc.Y = acc.ZZ = acc.ZZZ = f28_zero<RR>();
#pragma unroll 1
    for (int w = (int)nwin - 1; w >= 0; --w) {
#pragma unroll 1
        for (unsigned k = 0; k < c; ++k) xyzz28_dbl<C>(acc);
        xyzz28_add_full<C>(acc, xyzz28_load<C>(s[w]));
    }
    const XYZZ<C> r = xyzz28_to_std<C>(acc);
    out[row].inf = r.is_identity() ? 1u : 0u;
    out[row].p = xyzz_to_affine<C>(r);          // one inversion; the identity comes out as x = y = 0
}

// ------------------------------------------------------------------------------- the sorts
// histogram, bucket scan and scatter of the plan's n_wide_sets digit arrays of p.len entries each (set s: digits[s * len ..))
static int sort_sets(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const uint32_t *digits, uint32_t *counts, uint32_t *cursor, unsigned nbuckets) {
    const size_t lds = (size_t)nbuckets * 4;
    if (lds > 48 * 1024) {  // CDNA4: up to 160 KiB of LDS per workgroup, opt in above the default cap
        PM_HIP(ctx, hipFuncSetAttribute((const void *)k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PM_HIP(ctx, hipFuncSetAttribute((const void *)k_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    PM_LAUNCH(ctx, k_hist, dim3(p.nchunks, p.n_wide_sets), dim3(1024), lds, ctx->stream, digits, counts, p.len, p.chunk, nbuckets);
    PM_TRY(bucket_scan(ctx, S, p));
    PM_LAUNCH(ctx, k_scatter, dim3(p.nchunks, p.n_wide_sets), dim3(1024), lds, ctx->stream, digits, S.bucket_off.as<uint32_t>(), cursor,
                   S.sorted.as<uint32_t>(), p.len, p.chunk, nbuckets);
    return PM_OK;
}

// Pipeline (A): digits, LDS histogram per (chunk, window), bucket scan, LDS-staged scatter.
template <class C>
static int sort_windows(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars) {
    MsmWorkspace &ws = ctx->msm;
    PM_HIP(ctx, ws.digits.reserve(p.E * 4));
    uint32_t *counts = S.counts.as<uint32_t>(), *cursor = counts + p.NB, *digits = ws.digits.as<uint32_t>();
    PM_HIP(ctx, hipMemsetAsync(counts, 0, 2 * p.NB * 4, ctx->stream));
    PM_LAUNCH(ctx, k_digits<C>, dim3((unsigned)((p.len + 255) / 256)), dim3(256), 0, ctx->stream, d_scalars, d_bases, digits, p.len, p.c, p.nwin);
    return sort_sets(ctx, S, p, digits, counts, cursor, (unsigned)p.NB1);
}

// What the levels of the table-mode sort share: (u16 key, u32 value) entries in ws.digits, the regions' counters in ws.region.
struct SortBuffers {
    uint16_t *keys;
    uint32_t *vals, *region_count, *region_off, *region_cursor;
};

// First level: every (scalar, window) entry into the region of its bucket -- per-workgroup region counts, their column scan, the
// regions' offsets, the partition.  The kernels are instantiated per window count (win_off): the chain below finds nwin's.
template <class P, unsigned NWIN, unsigned M>
static int sort_first_level_launch(pm_ctx *ctx, const BucketPlan &p, const MsmTables &tb, const Fp<P> *d_scalars, const SortBuffers &b);
template <class P, unsigned NWIN = 10>
static int sort_first_level(pm_ctx *ctx, const BucketPlan &p, const MsmTables &tb, const Fp<P> *d_scalars, const SortBuffers &b) {
    if (p.nwin != NWIN) {
        if constexpr (NWIN < 32) return sort_first_level<P, NWIN + 1>(ctx, p, tb, d_scalars, b);
        return PM_ERR_INVALID_ARG;
    }
    if (tb.m == 5) {
        if constexpr (NWIN <= RADIX5_MAX_WINDOWS) {
            if (tb.a != radix_min_shift<P>(5, NWIN)) return PM_ERR_INVALID_ARG;     // the kernels' shift is that of (field, windows)
            return sort_first_level_launch<P, NWIN, 5>(ctx, p, tb, d_scalars, b);
        }
        return PM_ERR_INVALID_ARG;
    }
    return sort_first_level_launch<P, NWIN, 1>(ctx, p, tb, d_scalars, b);
}
template <class P, unsigned NWIN, unsigned M>
static int sort_first_level_launch(pm_ctx *ctx, const BucketPlan &p, const MsmTables &tb, const Fp<P> *d_scalars, const SortBuffers &b) {
    hipStream_t st = ctx->stream;
    const unsigned char *inf = tb.inf + tb.base_index;
    const unsigned pblocks = (unsigned)((p.len + p.pbd - 1) / p.pbd);
    const BlockScanShape bsh = block_scan_shape(pblocks, p.regions);
    PM_HIP(ctx, ctx->msm.block_cnt.reserve(((size_t)pblocks + bsh.G) * p.regions * 4));
    uint32_t *block_cnt = ctx->msm.block_cnt.as<uint32_t>(), *block_partial = block_cnt + (size_t)pblocks * p.regions;
    PM_HIP(ctx, hipMemsetAsync(b.region_count, 0, (size_t)p.regions * 4, st));
    hipLaunchKernelGGL((k_tbl_count<P, NWIN, M>), dim3(pblocks), dim3(p.pbd), 0, st, d_scalars, inf, p.len, p.regions, block_cnt, p.win_buckets,
                       p.narrow_buckets);
    hipLaunchKernelGGL(k_block_sums, dim3(bsh.G), dim3(1024), 0, st, block_cnt, pblocks, p.regions, bsh, block_partial);
    hipLaunchKernelGGL(k_block_offsets, dim3(bsh.G), dim3(1024), 0, st, block_cnt, pblocks, p.regions, bsh, block_partial, b.region_count);
    hipLaunchKernelGGL(k_region_offsets, dim3(1), dim3(1024), 0, st, b.region_count, b.region_off, b.region_cursor, p.regions);
    PM_HIP(ctx, hipFuncSetAttribute((const void *)k_tbl_partition<P, NWIN, M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.plds));
    PM_LAUNCH(ctx, (k_tbl_partition<P, NWIN, M>), dim3(pblocks), dim3(p.pbd), p.plds, st, d_scalars, inf, p.len, p.regions, b.region_off, block_cnt,
                   p.wide ? (size_t)0 : tb.stride, tb.base_index, b.keys, b.vals, p.win_buckets, p.narrow_buckets);
    return PM_OK;
}

constexpr unsigned SUB_BINS = 128, FIN_BINS = 256, FIN_BITS = 8;

// Regions of 2^15 buckets -> 128 sub-regions of 256 buckets -> buckets
static int sort_three_levels(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const SortBuffers &b) {
    MsmWorkspace &ws = ctx->msm;
    hipStream_t st = ctx->stream;
    const unsigned nsub = p.regions * SUB_BINS, chunk = 1u << RS_CHUNK_LOG;
    PM_HIP(ctx, ws.sub.reserve((3 * (size_t)nsub + 4) * 4));
    PM_HIP(ctx, ws.digits2.reserve(p.keys_bytes + p.E * 4 + 128));
    uint32_t *counts = S.counts.as<uint32_t>(), *cursor = counts + p.NB;
    uint32_t *sub_count = ws.sub.as<uint32_t>(), *sub_off = sub_count + nsub, *sub_cursor = sub_off + nsub + 1;
    uint16_t *keys2 = (uint16_t *)ws.digits2.p;
    uint32_t *vals2 = (uint32_t *)((uint8_t *)ws.digits2.p + p.keys_bytes);
    const unsigned sblocks = (unsigned)((p.E + chunk - 1) / chunk), stblocks = (unsigned)((p.E + ST_CHUNK - 1) / ST_CHUNK);
    PM_HIP(ctx, hipMemsetAsync(sub_count, 0, (size_t)nsub * 4, st));
    PM_LAUNCH(ctx, k_hist_small, dim3(sblocks), dim3(1024), 0, st, b.keys, b.region_off, p.regions, FIN_BITS, SUB_BINS, chunk, sub_count);
    PM_LAUNCH(ctx, k_scan_small, dim3(1), dim3(1024), 0, st, sub_count, sub_off, sub_cursor, nsub);
    PM_LAUNCH(ctx, k_region_pass_staged<RS_MID>, dim3(stblocks), dim3(ST_THREADS), 0, st, b.keys, b.vals, b.region_off, p.regions,
                   FIN_BITS, SUB_BINS, sub_off, sub_cursor, (uint32_t *)nullptr, keys2, vals2);
    PM_LAUNCH(ctx, k_hist_small, dim3(sblocks), dim3(1024), 0, st, keys2, sub_off, nsub, 0u, FIN_BINS, chunk, counts);
    PM_TRY(bucket_scan(ctx, S, p));
    // (round 5 measured the last level WITHOUT LDS staging -- lanes storing their 4-byte indices straight into the sub-region's
    // 120 KB output window, which stays in L2: the sort of a 2^24-pair MSM 2.66 -> 3.70 ms, a proof +2.2 ms; 64 partial-line
    // stores per wave instruction cost more than the staging saves: profiles/r05_sort_final_direct_negative.txt)
    PM_LAUNCH(ctx, k_region_pass_staged<RS_FINAL>, dim3(stblocks), dim3(ST_THREADS), 0, st, keys2, vals2, sub_off, nsub, 0u,
                   FIN_BINS, S.bucket_off.as<uint32_t>(), cursor, S.sorted.as<uint32_t>(), (uint16_t *)nullptr, (uint32_t *)nullptr);
    return PM_OK;
}

// Small bucket sets (< 2^15): one region, sorted directly with an NB-entry LDS table
static int sort_one_region(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const SortBuffers &b) {
    hipStream_t st = ctx->stream;
    const unsigned chunk = 1u << RS_CHUNK_LOG, sblocks = (unsigned)((p.E + chunk - 1) / chunk);
    const size_t lds = (size_t)p.lo_buckets * 4;
    uint32_t *counts = S.counts.as<uint32_t>(), *cursor = counts + p.NB;
    PM_LAUNCH(ctx, k_region_pass<RS_HIST>, dim3(sblocks), dim3(1024), lds, st, b.keys, b.vals, b.region_off, p.regions, 0u,
                   p.lo_buckets, chunk, counts, (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                   (uint16_t *)nullptr, (uint32_t *)nullptr);
    PM_TRY(bucket_scan(ctx, S, p));
    PM_LAUNCH(ctx, k_region_pass<RS_FINAL>, dim3(sblocks), dim3(1024), lds, st, b.keys, b.vals, b.region_off, p.regions, 0u,
                   p.lo_buckets, chunk, (uint32_t *)nullptr, S.bucket_off.as<uint32_t>(), cursor, S.sorted.as<uint32_t>(),
                   (uint16_t *)nullptr, (uint32_t *)nullptr);
    return PM_OK;
}

// Pipeline (B), tables and wide: (scalar, window) entries -> table (or base) indices grouped by bucket
template <class C>
static int sort_tables(pm_ctx *ctx, MsmSet &S, const BucketPlan &p, const MsmTables &tb, const Fp<typename C::FrP> *d_scalars) {
    MsmWorkspace &ws = ctx->msm;
    PM_HIP(ctx, ws.digits.reserve(p.keys_bytes + p.E * 4 + 128));     // + 128: the staged passes read whole groups of ST_PER_LANE entries
    PM_HIP(ctx, ws.region.reserve((3 * (size_t)p.regions + 4) * 4));
    SortBuffers b;
    b.keys = (uint16_t *)ws.digits.p;
    b.vals = (uint32_t *)((uint8_t *)ws.digits.p + p.keys_bytes);
    b.region_count = ws.region.as<uint32_t>();
    b.region_off = b.region_count + p.regions;
    b.region_cursor = b.region_off + p.regions + 1;
    PM_HIP(ctx, hipMemsetAsync(S.counts.as<uint32_t>(), 0, 2 * p.NB * 4, ctx->stream));
    PM_TRY((sort_first_level<typename C::FrP>(ctx, p, tb, d_scalars, b)));
    return p.lo_buckets == (1u << LO_BITS) ? sort_three_levels(ctx, S, p, b) : sort_one_region(ctx, S, p, b);
}

// ------------------------------------------------------------------------------- driver
// One bucket pipeline over at most msm_max_piece() pairs (internal.h; sorted-entry positions are u32: W * len < 2^32), ENQUEUED on
// ctx->stream: sort, task order, accumulation, reduction, and the copy of the plan's nsums window sums (internal form) to h_sums.
// Nothing here waits; the caller synchronises the stream and hands h_sums to host_horner.
// d_bases: the piece's bases (per-window); in wide mode the MSM's first base (internal form), the piece's pairs being
// d_bases[tb->base_index ...]; unused with tables.
//
// (Round 4 measured the sort in CHUNKS of pairs -- chunk k + 1 sorted on a second stream under chunk k's accumulation, one bucket
// set, the next chunk's tasks continuing from the previous partials -- and lost: k_accumulate holds 2 x 248 of a SIMD's 512 registers,
// so no other wave can be resident beside it; the sort's 1024-lane workgroups wait for whole CUs to drain and the two kernels
// time-slice instead of overlapping.  +1.8 ms per proof at two chunks, +5 at three: profiles/r04_chunked_sort_overlap_negative.txt;
// the implementation is commit 5de5c70.)
template <class C>
static int msm_enqueue(pm_ctx *ctx, const BucketPlan &p, const MsmTables *tb, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars,
                       XYZZ<C> *h_sums) {
    MsmSet &S = ctx->msm.set;
    if (p.wide && !d_bases) return PM_ERR_INVALID_ARG;
    PM_TRY(reserve_set<C>(ctx, S, p));
    {
        StageTimer t(ctx, T_MSM_SORT);
        PM_TRY(p.tables ? sort_tables<C>(ctx, S, p, *tb, d_scalars) : sort_windows<C>(ctx, S, p, d_bases, d_scalars));
        PM_TRY(task_order(ctx, S, p));
    }
    {
        StageTimer t(ctx, T_MSM_ACCUMULATE);
        if (p.tables && !p.wide) PM_TRY((accumulate<C, true>(ctx, S, p, tb->table)));
        else PM_TRY((accumulate<C, false>(ctx, S, p, (const void *)d_bases)));
    }
    StageTimer t(ctx, T_MSM_REDUCE);
    PM_TRY(fold_hot_buckets<C>(ctx, S, p));
    XYZZ<C> *d_sums = nullptr;
    if (!p.two_level) {
        PM_TRY(reduce_single_level<C>(ctx, S, p, &d_sums));
    } else {   // all sets of one size by ONE set of launches: those of the c-bit windows (or the shared set) ...
        PM_TRY(reduce_two_level<C>(ctx, p.reduce_wide, &d_sums));
    }
    PM_HIP(ctx, hipMemcpyAsync(h_sums, d_sums, p.n_wide_sets * sizeof(XYZZ<C>), hipMemcpyDeviceToHost, ctx->stream));
    if (p.n_narrow_sets) {   // ... then those of the (c - 1)-bit ones (stream order: the workspace is free again)
        PM_TRY(reduce_two_level<C>(ctx, p.reduce_narrow, &d_sums, (size_t)p.n_wide_sets * p.NB1));
        PM_HIP(ctx, hipMemcpyAsync(h_sums + p.n_wide_sets, d_sums, p.n_narrow_sets * sizeof(XYZZ<C>), hipMemcpyDeviceToHost, ctx->stream));
    }
    return PM_OK;
}

// plan, enqueue, synchronise, finish -- per piece of at most msm_max_piece() pairs; very long MSMs (the 10n-pair quotient commitment
// at n >= 2^24 on one GPU) run several, summed on the host
template <class C>
int msm_run(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, Affine<C> *h_out,
            int *h_inf, const MsmTables *tables) {
    const bool tbl = tables && tables->planned();
    const size_t max_piece = msm_max_piece(ctx);
    XYZZ<C> acc = XYZZ<C>::identity();
    std::vector<XYZZ<C>> sums;
    for (size_t off = 0; off < len; off += max_piece) {
        StageTimer t_total(ctx, T_MSM_TOTAL);
        const size_t cnt = len - off < max_piece ? len - off : max_piece;
        MsmTables tb;
        if (tbl) {
            tb = *tables;
            tb.base_index += off;
        }
        BucketPlan p;
        if (!bucket_plan(tb, cnt, (unsigned)C::FrP::BITS, ctx->opt.v[PM_OPT_MSM_TASK_LEN], p)) return PM_ERR_INVALID_ARG;   // tb not planned: per-window
        sums.resize(p.nsums);
        PM_TRY(msm_enqueue<C>(ctx, p, tbl ? &tb : nullptr, tbl ? d_bases : d_bases + off, d_scalars + off, sums.data()));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        acc = xyzz_add<C>(acc, host_horner<C>(sums.data(), p.nsums, p.width));
    }
    host_finish<C>(acc, h_out, h_inf);
    return PM_OK;
}

// `batch` MSMs of `len` pairs each against ONE base range: row b = d_scalars[b * len ..) times d_bases[0 .. len).  The per-window
// pipeline handles nwin independent bucket sets, every stage indexed by set, and sorted[] holds plain base indices: a group of `rows`
// rows is the same pipeline over rows * nwin sets -- set s = b * nwin + w owns digits [s * len, (s + 1) * len) -- planned once for
// `len` and scaled.  New are the digits over (row, i) (k_digits_batch) and the final combine on the device (k_window_combine): one
// record of (point, flag) per row comes out of a group; the host neither doubles nor inverts.
// A group is as many whole rows as keep rows * len <= msm_max_piece(), rows * nwin <= 65 535 (grid y of k_hist / k_scatter) and
// E, NB < 2^32 (u32 positions); further groups reuse the workspace in stream order.  A row longer than one piece runs row by row
// through msm_run.  Window tables and wide plans are NOT used here: the points are the plain resident array (pm_bases keeps it
// beside its tables), so a precomputed pm_bases gives the same points, at the per-window pipeline's 16+ additions per pair.
// NOT yet measured against a loop of msm_run (tools/msm_bench.py --batch does it): DESIGN.md §4.2 "Batched MSM", profiles/msm_batch.txt.
//
// The device form leaves row b's (point, flag) record in d_out[b], an array of the caller's in device memory, and returns with
// everything ENQUEUED on ctx->stream: no copy to the host, no synchronisation, the batch's internal groups stream-ordered on the one
// workspace.  It takes rows of at most one piece (a longer row needs the host between its pieces: PM_ERR_INVALID_ARG).  The host form
// is the device form into the workspace's own array plus one copy and one synchronisation for the whole batch.
template <class C>
__global__ void k_batch_points_identity(BatchPoint<C> *out, unsigned rows) {
    const unsigned row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    out[row].p = Affine<C>::infinity();
    out[row].inf = 1u;
}

template <class C>
int msm_run_batch_device(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, size_t batch, BatchPoint<C> *d_out) {
    if (batch == 0) return PM_OK;
    if (len == 0) {
        PM_LAUNCH(ctx, k_batch_points_identity<C>, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream, d_out, (unsigned)batch);
        return PM_OK;
    }
    const size_t max_piece = msm_max_piece(ctx);
    if (len > max_piece || batch > 0xFFFFFFFFull) return PM_ERR_INVALID_ARG;
    BucketPlan row;
    if (!bucket_plan(WindowLayout(), len, (unsigned)C::FrP::BITS, ctx->opt.v[PM_OPT_MSM_TASK_LEN], row)) return PM_ERR_INVALID_ARG;
    const size_t u32_max = 0xFFFFFFFFull;
    size_t group = max_piece / len;
    if (group > 65535 / row.nwin) group = 65535 / row.nwin;
    if (group > u32_max / row.E) group = u32_max / row.E;
    if (group > u32_max / row.NB) group = u32_max / row.NB;
    if (group > batch) group = batch;
    if (group < 1) return PM_ERR_INVALID_ARG;

    MsmWorkspace &ws = ctx->msm;
    PM_HIP(ctx, ws.batch.reserve(batch_flag_bytes(len)));      // (the host form has reserved its records behind the flags: no-op then)
    unsigned char *d_inf = ws.batch.as<unsigned char>();
    PM_TRY(infinity_flags<C>(ctx, d_bases, len, d_inf));
    for (size_t b0 = 0; b0 < batch; b0 += group) {
        StageTimer t_total(ctx, T_MSM_TOTAL);
        const size_t rows = batch - b0 < group ? batch - b0 : group;
        const BucketPlan p = bucket_plan_rows(row, rows);
        MsmSet &S = ws.set;
        PM_TRY(reserve_set<C>(ctx, S, p));
        {
            StageTimer t(ctx, T_MSM_SORT);
            PM_HIP(ctx, ws.digits.reserve(p.E * 4));
            uint32_t *counts = S.counts.as<uint32_t>(), *cursor = counts + p.NB, *digits = ws.digits.as<uint32_t>();
            const unsigned nbuckets = (unsigned)p.NB1;
            PM_HIP(ctx, hipMemsetAsync(counts, 0, 2 * p.NB * 4, ctx->stream));
            PM_LAUNCH(ctx, k_digits_batch<C>, dim3((unsigned)((len + 255) / 256), (unsigned)rows), dim3(256), 0, ctx->stream,
                           d_scalars + b0 * len, d_inf, digits, len, p.c, p.nwin);
            PM_TRY(sort_sets(ctx, S, p, digits, counts, cursor, nbuckets));
            PM_TRY(task_order(ctx, S, p));
        }
        {
            StageTimer t(ctx, T_MSM_ACCUMULATE);
            PM_TRY((accumulate<C, false>(ctx, S, p, (const void *)d_bases)));
        }
        {
            StageTimer t(ctx, T_MSM_REDUCE);
            PM_TRY(fold_hot_buckets<C>(ctx, S, p));
            XYZZ<C> *d_sums = nullptr;
            PM_TRY(reduce_single_level<C>(ctx, S, p, &d_sums));
            PM_LAUNCH(ctx, k_window_combine<C>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, ctx->stream, d_sums, p.nwin, p.c,
                           (unsigned)rows, d_out + b0);
        }
    }
    return PM_OK;
}

template <class C>
int msm_run_batch(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, size_t batch, Affine<C> *h_out,
                  int *h_inf) {
    if (len == 0) {
        for (size_t b = 0; b < batch; ++b) { h_out[b] = Affine<C>::infinity(); h_inf[b] = 1; }
        return PM_OK;
    }
    if (len > msm_max_piece(ctx)) {
        for (size_t b = 0; b < batch; ++b) PM_TRY(msm_run<C>(ctx, d_bases, d_scalars + b * len, len, h_out + b, h_inf + b));
        return PM_OK;
    }
    if (batch == 0) return PM_OK;
    const size_t flag_bytes = batch_flag_bytes(len);
    PM_HIP(ctx, ctx->msm.batch.reserve(flag_bytes + batch * sizeof(BatchPoint<C>)));
    BatchPoint<C> *d_res = (BatchPoint<C> *)(ctx->msm.batch.as<unsigned char>() + flag_bytes);
    PM_TRY(msm_run_batch_device<C>(ctx, d_bases, d_scalars, len, batch, d_res));
    std::vector<BatchPoint<C>> res(batch);
    PM_HIP(ctx, hipMemcpyAsync(res.data(), d_res, batch * sizeof(BatchPoint<C>), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t r = 0; r < batch; ++r) { h_out[r] = res[r].p; h_inf[r] = (int)res[r].inf; }
    return PM_OK;
}

// Asynchronous pair for a single-piece table-mode MSM: msm_begin enqueues the whole pipeline on ctx->stream and returns at once
// (the reduced point travels to the context's pinned slot), msm_end waits for the stream and finishes it.  Two contexts (ctx and
// its helper ctx->aux: own streams, own workspaces) can so run two MSMs concurrently from ONE host thread -- the latency-bound
// sort front end and bucket reduction of one hide under the accumulation of the other.  MSMs that need the host in the middle
// (several pieces, wide mode, no tables) run synchronously inside msm_begin; msm_end then just hands the result over.
template <class C>
int msm_begin(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, const MsmTables *tables) {
    ctx->msm_async = 0;
    const bool tbl = tables && tables->planned() && !tables->wide;
    if (!ctx_pinned(ctx)) { ctx->err = "pinned result slot allocation failed"; return PM_ERR_HIP; }
    if (len == 0 || !tbl || len > msm_max_piece(ctx)) {           // synchronous: result parked in the slot
        PM_TRY(msm_run<C>(ctx, d_bases, d_scalars, len, pinned_slot<Affine<C>>(ctx, PINNED_MSM_POINT), pinned_slot<int>(ctx, PINNED_MSM_INF), tables));
        ctx->msm_async = 2;
        return PM_OK;
    }
    StageTimer t_total(ctx, T_MSM_TOTAL);
    BucketPlan p;
    if (!bucket_plan(*tables, len, (unsigned)C::FrP::BITS, ctx->opt.v[PM_OPT_MSM_TASK_LEN], p)) return PM_ERR_INVALID_ARG;   // one shared set: one sum
    PM_TRY(msm_enqueue<C>(ctx, p, tables, d_bases, d_scalars, pinned_slot<XYZZ<C>>(ctx, PINNED_MSM_SUM)));
    ctx->msm_async = 1;
    return PM_OK;
}

template <class C>
int msm_end(pm_ctx *ctx, Affine<C> *h_out, int *h_inf) {
    if (ctx->msm_async == 2) {
        *h_out = *pinned_slot<const Affine<C>>(ctx, PINNED_MSM_POINT);
        *h_inf = *pinned_slot<const int>(ctx, PINNED_MSM_INF);
    } else if (ctx->msm_async == 1) {
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const unsigned char width0 = 0;
        host_finish<C>(host_horner<C>(pinned_slot<const XYZZ<C>>(ctx, PINNED_MSM_SUM), 1, &width0), h_out, h_inf);
    } else {
        return PM_ERR_STATE;
    }
    ctx->msm_async = 0;
    return PM_OK;
}

template int msm_begin<BlsCurve>(pm_ctx *, const Affine<BlsCurve> *, const Fp<BlsFrP> *, size_t, const MsmTables *);
template int msm_begin<BnCurve>(pm_ctx *, const Affine<BnCurve> *, const Fp<BnFrP> *, size_t, const MsmTables *);
template int msm_end<BlsCurve>(pm_ctx *, Affine<BlsCurve> *, int *);
template int msm_end<BnCurve>(pm_ctx *, Affine<BnCurve> *, int *);
template int msm_run<BlsCurve>(pm_ctx *, const Affine<BlsCurve> *, const Fp<BlsFrP> *, size_t, Affine<BlsCurve> *, int *, const MsmTables *);
template int msm_run<BnCurve>(pm_ctx *, const Affine<BnCurve> *, const Fp<BnFrP> *, size_t, Affine<BnCurve> *, int *, const MsmTables *);
template int msm_run_batch_device<BlsCurve>(pm_ctx *, const Affine<BlsCurve> *, const Fp<BlsFrP> *, size_t, size_t, BatchPoint<BlsCurve> *);
template int msm_run_batch_device<BnCurve>(pm_ctx *, const Affine<BnCurve> *, const Fp<BnFrP> *, size_t, size_t, BatchPoint<BnCurve> *);
template int msm_run_batch<BlsCurve>(pm_ctx *, const Affine<BlsCurve> *, const Fp<BlsFrP> *, size_t, size_t, Affine<BlsCurve> *, int *);
template int msm_run_batch<BnCurve>(pm_ctx *, const Affine<BnCurve> *, const Fp<BnFrP> *, size_t, size_t, Affine<BnCurve> *, int *);

}  // namespace pm
