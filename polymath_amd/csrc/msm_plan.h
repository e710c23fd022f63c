// Everything an MSM decides before its first launch: the window layout, the decoding of PM_OPT_TABLE_WINDOW_BITS, the two planners
// with their cost model, the bucket plan of one pipeline and the shape of the two-level reduction.  Plain C++17 on constants.cuh and
// radix.cuh: the kernels of msm.hip (win_off / win_width / win_base with their NWIN template argument), the host drivers and the CPU
// self-test (tests/native/msm_plan_selftest.cpp, which pins every plan of a recorded grid) share it.  Nothing here touches a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "constants.cuh"
#include "radix.cuh"

#if defined(__HIPCC__)
#define PM_PLAN_HD __host__ __device__ constexpr
#else
#define PM_PLAN_HD constexpr
#endif

namespace pm {

// The sort's first level (msm.hip: k_tbl_count / k_tbl_partition) splits the buckets into regions of 2^15, one region per scan lane
// of a workgroup of at most 1024 lanes.
constexpr unsigned SORT_REGION_BITS = 15, SORT_MAX_REGIONS = 1024;
constexpr unsigned RADIX5_MAX_WINDOWS = 16;   // radix 5 2^a (radix.cuh): the first sort level is instantiated for 10 ... 16 windows
// Single-level reduction (msm.hip: k_bucket_reduce): RED_K consecutive buckets per lane -- 8 adds + <= 15 doublings, 8192 lanes on 2^15 buckets.
constexpr unsigned RED_K = 4;
// Scalars per first-level workgroup of the table-mode sort: 512 up to 16 windows, 256 beyond (the staged entries take lanes x
// windows x 8 bytes of LDS).  From 512 regions up (the 12-window wide plan of a 2^24-gate key: 4 x 2^21 + 8 x 2^20 buckets): 1024, so that a
// workgroup's run inside a region is 24 entries (96 B of values), not 12 -- what the first level pays for is the length of that
// run, not the number of regions: same-box A/B at 2^24 gates in profiles/r06_wide_ragged_sets_ab.txt (512 regions on 512 lanes:
// sort + 5 ... 8 ms against 768 on 1024) and r06_wide_12_windows_ab.txt; 256 against 512 lanes below that: flat
// (profiles/r05_sort_chunk_shapes_after_wide_loads.txt, (3)).  The radix-5 plans stay below that threshold and on 512 lanes: 11 windows
// in 160 regions (runs of 35 entries) measured 3.56 ms of sort on 512 lanes against 3.68 on 1024 for the 21 M-pair [d]_1, 56.61 ...
// 56.74 against 56.79 ... 56.96 ms per proof on one box (profiles/msm_radix5_ab.txt); 12 windows in 40 regions write runs of 150.
constexpr unsigned PARTITION_LANES = 512, PARTITION_WIDE_LANES = 1024, PARTITION_WIDE_FROM = 512;

// ------------------------------------------------------------------------------- the window layout
// Balanced power-of-two layout: the 256 scalar bits (255 + signed-digit carry) split into nwin windows of ceil(256 / nwin) bits or
// one fewer, the wider ones first, so no window is narrow -- with one shared bucket set a short top window would pile all of its
// digits into a few hot buckets.  The kernels are instantiated per NWIN so that every bit offset, shift and limb index is an
// immediate: with a run-time layout the compiler parks the scalar in LDS and fetches offsets with vector loads.
PM_PLAN_HD unsigned win_width(unsigned nwin, unsigned w) { return 256 / nwin + (w < 256 % nwin ? 1u : 0u); }
PM_PLAN_HD unsigned win_off(unsigned nwin, unsigned w) { return w * (256 / nwin) + (w < 256 % nwin ? w : 256 % nwin); }
// Wide mode (every window has its own bucket set): first bucket of window w's set.  The 256 % nwin windows that are one bit wider come
// first and own `wide_b` buckets each, the others `narrow_b` (BucketSets below).  Table mode passes 0 for both: one shared set.
PM_PLAN_HD uint32_t win_base(unsigned nwin, unsigned w, uint32_t wide_b, uint32_t narrow_b) {
    return w <= 256 % nwin ? w * wide_b : (256 % nwin) * wide_b + (w - 256 % nwin) * narrow_b;
}

// a bucket set of more than one sort region is whole regions (empty buckets pad it: scan, task order and reduction pass over them)
constexpr size_t pad_to_regions(size_t buckets) {
    const size_t region = (size_t)1 << SORT_REGION_BITS;
    return buckets > region ? (buckets + region - 1) / region * region : buckets;
}

// The bucket sets of a layout in bucket order: n_wide of wide_b buckets, then n_narrow of narrow_b.
struct BucketSets {
    size_t wide_b = 0, narrow_b = 0;
    unsigned n_wide = 0, n_narrow = 0;
    constexpr size_t total() const { return n_wide * wide_b + n_narrow * narrow_b; }
};

// A window layout as a value: radix m 2^a on nwin windows (nwin == 0: no plan).
//   m = 1  the balanced power-of-two layout above (a unused).  Tables: point (w, i) = 2^(win_off(nwin, w)) P_i, one shared set of
//          2^(c-1) buckets, c = the widest window.  wide: no tables in HBM -- every window keeps its OWN bucket set, the points are
//          gathered from the plain base array and the nwin window sums are combined by a Horner chain of doublings on the host; same
//          sort / accumulate / reduce kernels, so c can be 19-22 where the LDS-histogram pipeline of one-shot MSMs stops at 16.
//   m = 5  point (w, i) = R^w P_i with R = 5 2^a (radix.cuh), one shared set of R / 2 = 5 2^(a-1) buckets.  Tables only, never wide.
struct WindowLayout {
    unsigned m = 1, nwin = 0, a = 0;
    bool wide = false;
    constexpr bool planned() const { return nwin != 0; }
    // bits of the widest window; radix 5 2^a: ceil(log2 R) = a + 3.  What pm_pk_msm_plan reports.
    constexpr unsigned widest() const { return !nwin ? 0u : m == 5 ? a + 3 : win_width(nwin, 0); }
    // Shared set: all of R / 2 buckets.  Wide: the 256 % nwin windows of c bits own 2^(c-1) buckets each, the windows that are one
    // bit narrower half of that where it is still whole sort regions -- otherwise all nwin sets have 2^(c-1) and count as wide (until
    // round 6 they always did: 12 windows of 22 / 21 bits held 12 x 2^21 = 25.2 M buckets instead of 16.8 M, in 768 regions, not 512).
    constexpr BucketSets sets() const {
        BucketSets s{m == 5 ? pad_to_regions((size_t)5 << (a - 1)) : (size_t)1 << (widest() - 1), 0, 1, 0};
        if (wide) {
            const bool halve = 256 % nwin != 0 && (s.wide_b >> 1) >= ((size_t)1 << SORT_REGION_BITS);
            s.narrow_b = halve ? s.wide_b >> 1 : s.wide_b;
            s.n_wide = halve ? 256 % nwin : nwin;
            s.n_narrow = nwin - s.n_wide;
        }
        return s;
    }
    constexpr size_t total_buckets() const { return sets().total(); }
};

constexpr WindowLayout pow2_layout(unsigned nwin, bool wide = false) { return WindowLayout{1, nwin, 0, wide}; }
// Radix 5 2^a on nwin windows: a = the smallest shift for which the top digit of the field's scalars never carries out
// (radix_top_fits: exact integer arithmetic); no plan if there is none, or outside the first sort level's 10 ... 16 windows.
constexpr WindowLayout radix5_layout(unsigned nwin, unsigned scalar_bits) {
    if (nwin < 10 || nwin > RADIX5_MAX_WINDOWS) return WindowLayout{};
    const unsigned a = scalar_bits == (unsigned)BlsFrP::BITS ? radix_min_shift<BlsFrP>(5, nwin) : radix_min_shift<BnFrP>(5, nwin);
    return a ? WindowLayout{5, nwin, a, false} : WindowLayout{};
}

// ------------------------------------------------------------------------------- PM_OPT_TABLE_WINDOW_BITS
// The raw option value decoded (the accepted values: include/polymath_hip.h).  A value that names nothing (1 ... 3, 25 ... 99) plans
// like 0; INVALID (100 m + w with m not 1 or 5, or w outside 0, 10 ... 32) gets no table plan.
struct WindowOption {
    enum Kind { NONE, WIDEST, RADIX, INVALID } kind = NONE;
    unsigned c = 0;           // WIDEST: bits of the widest window of the power-of-two layout
    unsigned m = 0, nwin = 0; // RADIX: the multiplier, and the window count (0: the cost model's for that m)
    // the widest window a WIDE plan is held to: the wide planner takes 16 ... 23 and plans every other value like 0
    constexpr unsigned wide_c() const { return kind == WIDEST && c >= 16 && c <= 23 ? c : 0u; }
};
constexpr WindowOption decode_window_option(unsigned v) {
    WindowOption o;
    if (v >= 100) {
        o.m = v / 100; o.nwin = v % 100;
        o.kind = (o.m != 1 && o.m != 5) || (o.nwin && (o.nwin < 10 || o.nwin > 32)) ? WindowOption::INVALID : WindowOption::RADIX;
    } else if (v >= 4 && v <= 24) {
        o.kind = WindowOption::WIDEST; o.c = v;
    }
    return o;
}

// ------------------------------------------------------------------------------- the planners
// Cost model in units of one accumulated bucket entry (one mixed add at full throughput: 0.148 ns measured, 6.75 G adds/s; refit at
// 0.131 ns on the 21 M-pair [d]_1 of a 2^20-gate proof, profiles/msm_radix5_ab.txt).  E = windows x pairs entries, NB buckets.
//   accumulate  one lane per bucket, ~20 us per mixed add of its chain: few, long buckets leave the machine latency-bound.
inline double cost_accumulate(double E, double NB) { return E > E / NB * 135e3 ? E : E / NB * 135e3; }
//   reduce      the bucket reduction + the sort's fixed part: the four-lane reduction measures 0.66 ms at 2^19 buckets and 1.39 ms at
//               2^21 (profiles/r02_m_reduce_pair_sweep.txt) = 2.9e6 + 3.3 NB, plus ~0.4e6 of sort launches.  The refit: 0.95 / 1.39 /
//               2.68 ms at 1.31 M / 2.10 M / 5.24 M buckets = 0.375 ms + 0.44 ns (3.3 entries) per bucket: both constants stand, and
//               with them every power-of-two plan.
inline double cost_reduce(double NB) { return 3.3e6 + 3.3 * NB; }
//   radix 5 2^a pays two more terms: its recoding in the two kernels of the first sort level, 0.41 ms for 21 M scalars = 0.15 entries
//               per pair, and the bucket-side passes of the sort (memset, scan, task bins), 0.19 ms for 3.1 M more buckets = 0.45
//               entries per bucket -- which the power-of-two plans pay as well, but their fit never held it.
inline double cost_radix5(double pairs, double n_msm, double NB) { return 0.15 * pairs + n_msm * 0.45 * NB; }

// Radix 5 2^a joins the enumeration for long MSMs only: below 2^22 pairs the model's two candidates differ by less than its error,
// and the [a]_1 MSM, the shards of a sharded key and short resident vectors keep the power-of-two plans they were measured with.
constexpr size_t RADIX5_MIN_PAIRS = (size_t)1 << 22;

// Layout of one table set for n_msm MSMs of total_pairs pairs over resident_points points, windows x resident < 2^31 (u32 table
// indices); no plan if nothing fits (the 335 M-pair [d]_1 of a 2^24-gate key).  A forced widest window is taken as it is.
inline WindowLayout tables_plan(size_t total_pairs, unsigned n_msm, size_t resident_points, unsigned scalar_bits, WindowOption force = WindowOption()) {
    if (force.kind == WindowOption::INVALID) return WindowLayout{};
    if (force.kind == WindowOption::WIDEST) return pow2_layout((256 + force.c - 1) / force.c);   // 24 = the 11-window experiment (profiles/r02_levers_*.jsonl)
    const bool radix = force.kind == WindowOption::RADIX;
    WindowLayout best_t;
    double best = 1e300;
    for (unsigned nwin = 10; nwin <= 32; ++nwin)
        for (unsigned m = 1; m <= 5; m += 4) {
            if (radix ? m != force.m : m == 5 && total_pairs < RADIX5_MIN_PAIRS) continue;
            if (radix && force.nwin && nwin != force.nwin) continue;
            const WindowLayout t = m == 1 ? pow2_layout(nwin) : radix5_layout(nwin, scalar_bits);
            if (!t.planned()) continue;
            if (m == 1 && (t.widest() < 4 || t.widest() > 23)) continue;
            if (m == 5 && !(radix && force.nwin) && t.a < SORT_REGION_BITS + 1) continue;   // by itself the model picks whole regions only
            if ((double)nwin * (double)resident_points >= 2147483648.0) continue;
            const double NB = (double)t.total_buckets();
            double cost = cost_accumulate((double)nwin * (double)total_pairs, NB) + (double)n_msm * cost_reduce(NB);
            if (m == 5) cost += cost_radix5((double)total_pairs, (double)n_msm, NB);
            if (cost < best) { best = cost; best_t = t; }
        }
    return best_t;
}

// Plan of the WIDE mode for pieces of `piece` pairs (<= msm_max_piece()): accumulation of nwin x piece entries + the reduction of all
// sets (one or two batched launches), within the sort front end's SORT_MAX_REGIONS regions and u32 positions of the sorted entries.
// 12 windows are the fewest whose widest window (22 bits) passes the c <= 23 test, and where long MSMs land: 12 additions per pair
// where the one-shot MSM's LDS histogram stops at c = 16 (16 additions), in 512 regions (same-box A/B against round 5's 512-region plan
// of 13 windows: profiles/r06_wide_12_windows_ab.txt).  force.wide_c(): that widest window whatever the model says, or no plan.
inline WindowLayout wide_plan(size_t piece, WindowOption force = WindowOption()) {
    WindowLayout best_t;
    double best = 1e300;
    for (unsigned nwin = 12; nwin <= 16; ++nwin) {
        const WindowLayout t = pow2_layout(nwin, true);
        if (t.widest() < 16 || t.widest() > 23) continue;                    // whole 2^15-bucket regions per window (the sort's first level)
        const double NBT = (double)t.total_buckets();
        if (NBT / 32768.0 > (double)SORT_MAX_REGIONS) continue;
        if ((double)nwin * (double)piece >= 4294967296.0) continue;
        if (force.wide_c() && t.widest() != force.wide_c()) continue;
        if (force.wide_c()) return t;
        const double cost = cost_accumulate((double)nwin * (double)piece, NBT) + cost_reduce(NBT);
        if (cost < best) { best = cost; best_t = t; }
    }
    return best_t;
}

// ------------------------------------------------------------------------------- the two-level reduction
// Shape of msm_reduce.hip's three launches over nsets sets of `buckets` buckets each (reduce_two_level).
//   level 0  K0 buckets per lane: <= 2^17 lanes = 2 waves per SIMD, one round of the chip.  Powers of two (and several sets): K0
//            doubles from 4 up to 64 (swept in profiles/r02_levers.jsonl: K0 = 2 doubles level 1's work and loses).  One set of any
//            size (radix 5 2^a): K0 = ceil(NB / 2^17) as a plain integer -- 40 for 5.24 M buckets, 10 for 1.31 M; the next power of
//            two would leave the chip 62 % full on a chain 1.6 times as long (64 against 40).
//   level 1  lane GROUPS of REDUCE_COOP lanes per point, 256 / REDUCE_COOP points per workgroup; R1 = 2 REDUCE_COOP level-0 outputs
//            per group keeps level 1 at 2^16 lanes = one wave per SIMD (its register budget); K0 and R1 swept on MI355X in round 2
//            (profiles/r02_levers.jsonl, r02_m_reduce_pair_sweep.txt).  Several sets: R1 is halved until no workgroup straddles two.
// ok == false: the kernels cannot run the shape (several sets that are no power of two, or do not split into whole workgroups).
constexpr unsigned REDUCE_COOP = 4;
struct ReduceShape {
    size_t buckets = 0;                    // per set
    unsigned nsets = 0, K0 = 0, R1 = 0;
    size_t set_lanes = 0, lanes0 = 0, lanes1 = 0, blocks0 = 0, blocks1 = 0;   // set_lanes: level-0 outputs per set
    bool ok = false;
};
constexpr ReduceShape reduce_shape(size_t buckets, unsigned nsets) {
    ReduceShape s{buckets, nsets};
    const bool pow2 = (buckets & (buckets - 1)) == 0;
    if (nsets == 0 || buckets == 0 || (nsets > 1 && !pow2)) return s;
    s.K0 = 4;
    if (nsets > 1 || pow2) {
        while (buckets * nsets / s.K0 > ((size_t)1 << 17) && s.K0 < 64) s.K0 <<= 1;
    } else {
        const size_t k = (buckets + ((size_t)1 << 17) - 1) >> 17;
        if (k > s.K0) s.K0 = (unsigned)k;
    }
    s.R1 = 2 * REDUCE_COOP;
    const unsigned per_block1 = 256 / REDUCE_COOP;
    s.set_lanes = (buckets + s.K0 - 1) / s.K0;
    if (nsets > 1) {
        while (s.set_lanes % ((size_t)s.R1 * per_block1) != 0 && s.R1 > 1) s.R1 >>= 1;
        if (buckets % s.K0 != 0 || s.set_lanes % ((size_t)s.R1 * per_block1) != 0) return s;
    }
    s.lanes0 = s.set_lanes * nsets; s.lanes1 = (s.lanes0 + s.R1 - 1) / s.R1;
    s.blocks0 = (s.lanes0 + 255) / 256; s.blocks1 = (s.lanes1 + per_block1 - 1) / per_block1;
    s.ok = true;
    return s;
}

// ------------------------------------------------------------------------------- the bucket plan
// Everything one bucket pipeline derives from its inputs before the first launch; the stages of msm.hip read it and recompute nothing.
// Three shapes: per-window (pipeline A: nwin sets of 2^(c-1) buckets, LDS-histogram sort), tables (one shared set, radix sort over
// the window tables' indices) and wide (tables == wide == true: one set per window, radix sort, points from the plain base array).
struct BucketPlan {
    bool tables = false, wide = false;
    unsigned nwin = 0, c = 0;                // windows; bits of the widest
    size_t len = 0, E = 0;                   // pairs; E = nwin * len, the most entries the sort can see
    // the bucket sets, in bucket order (BucketSets): n_wide_sets of NB1 buckets, then n_narrow_sets of NBn; NB = all of them.
    // Per-window: nwin sets of NB1 = 2^(c-1); tables: one.
    size_t NB1 = 0, NBn = 0, NB = 0;
    unsigned n_wide_sets = 0, n_narrow_sets = 0;
    uint32_t win_buckets = 0, narrow_buckets = 0;   // win_base()'s arguments: NB1 and NBn in wide mode, 0 for the shared set
    size_t seg = 0, max_tasks = 0;           // entries per accumulate task; bound on the number of tasks
    unsigned chunk = 0, nchunks = 0;         // per-window: scalars per histogram / scatter workgroup
    // table-mode sort: regions of lo_buckets (2^15, or the whole of a smaller set); first-level workgroup and its dynamic LDS
    unsigned lo_buckets = 0, regions = 0, pbd = 0;
    size_t plds = 0, keys_bytes = 0;
    bool two_level = false;                  // reduce_two_level per group of sets (the shapes below); otherwise reduce_single_level
    ReduceShape reduce_wide, reduce_narrow;
    unsigned red_lanes = 0, red_block = 0, bpw = 0;   // single-level reduction: lanes and workgroups per set
    unsigned nsums = 0;                      // window sums the pipeline hands to host_horner ...
    unsigned char width[64] = {0};           // ... and the doublings in front of each
};

// window width of the per-window pipeline: c minimising  W(c) * (len + 6 * 2^(c-1))   (6 ~ cost of the reduce per bucket in madds)
inline unsigned per_window_bits(size_t len, unsigned scalar_bits) {
    double best = 1e300;
    unsigned bc = 4;
    for (unsigned c = 4; c <= 16; ++c) {
        const unsigned w = (scalar_bits + 1 + c - 1) / c;
        const double cost = (double)w * ((double)len + 6.0 * (double)(1u << (c - 1)));
        if (cost < best) { best = cost; bc = c; }
    }
    return bc;
}

// lay: the window tables' or the wide plan's layout; not planned: the per-window pipeline on `len` pairs of scalar_bits-bit scalars.
// task_len: PM_OPT_MSM_TASK_LEN (tuning sweeps), 0 = twice the mean bucket load.  false: a plan the kernels cannot run.
inline bool bucket_plan(const WindowLayout &lay, size_t len, unsigned scalar_bits, long long task_len, BucketPlan &p) {
    p = BucketPlan();
    p.len = len; p.tables = lay.planned();
    if (!p.tables) {
        p.c = per_window_bits(len, scalar_bits);
        p.nwin = (scalar_bits + 1 + p.c - 1) / p.c;
        p.NB1 = (size_t)1 << (p.c - 1);
        p.n_wide_sets = p.nwin;
        for (unsigned i = 0; i < p.nwin; ++i) p.width[i] = (unsigned char)p.c;
        p.chunk = 1u << 15;   // scalars per (chunk, window) histogram / scatter workgroup (tools/msm_bench.py sweep)
        if (len < p.chunk) p.chunk = (unsigned)(len ? len : 1);
        p.nchunks = (unsigned)((len + p.chunk - 1) / p.chunk);
    } else {
        p.wide = lay.wide; p.nwin = lay.nwin; p.c = lay.widest();
        if (p.nwin < 10 || p.nwin > 32) return false;                  // the first level's instantiations (msm.hip: sort_first_level)
        if (lay.m == 5 ? p.wide || p.nwin > RADIX5_MAX_WINDOWS || lay.a < 11 || lay.a > 28 : lay.m != 1) return false;
        const BucketSets s = lay.sets();
        p.NB1 = s.wide_b; p.NBn = s.narrow_b; p.n_wide_sets = s.n_wide; p.n_narrow_sets = s.n_narrow;
        if (p.wide) {
            p.win_buckets = (uint32_t)p.NB1; p.narrow_buckets = (uint32_t)p.NBn;
            for (unsigned w = 0; w < p.nwin; ++w) p.width[w] = (unsigned char)win_width(p.nwin, w);
        }
    }
    p.NB = p.n_wide_sets * p.NB1 + p.n_narrow_sets * p.NBn;
    p.E = (size_t)p.nwin * len; p.nsums = p.n_wide_sets + p.n_narrow_sets;
    p.seg = 2 * (p.E / p.NB + 1);
    if (p.seg < 64) p.seg = 64;
    if (task_len > 0) p.seg = (size_t)task_len;
    p.max_tasks = p.NB + p.E / p.seg + 1;
    p.red_lanes = (unsigned)((p.NB1 + RED_K - 1) / RED_K);
    p.red_block = 64;
    while (p.red_block < p.red_lanes && p.red_block < 256) p.red_block <<= 1;
    p.bpw = (p.red_lanes + p.red_block - 1) / p.red_block;
    if (!p.tables) return true;

    p.lo_buckets = (unsigned)(p.NB < ((size_t)1 << SORT_REGION_BITS) ? p.NB : ((size_t)1 << SORT_REGION_BITS));
    p.regions = (unsigned)(p.NB / p.lo_buckets);
    if ((size_t)p.regions * p.lo_buckets != p.NB) return false;           // whole regions only
    p.pbd = p.regions >= PARTITION_WIDE_FROM ? PARTITION_WIDE_LANES : p.nwin <= 16 ? PARTITION_LANES : 256;
    if (p.regions > p.pbd || p.regions > SORT_MAX_REGIONS) return false;  // one region per scan lane; cnt[] / delta[] of k_tbl_partition
    p.plds = 2 * SORT_MAX_REGIONS * 4 + (size_t)p.pbd * p.nwin * 8;
    p.keys_bytes = (p.E * 2 + 15) & ~(size_t)15;
    p.two_level = p.NB1 >= 4096;                                          // below: a shared set too small for msm_reduce.hip
    if (p.wide && !p.two_level) return false;                             // wide plans have c >= 16 (wide_plan)
    if (p.two_level) {
        p.reduce_wide = reduce_shape(p.NB1, p.n_wide_sets);
        if (p.n_narrow_sets) p.reduce_narrow = reduce_shape(p.NBn, p.n_narrow_sets);
        if (!p.reduce_wide.ok || (p.n_narrow_sets && !p.reduce_narrow.ok)) return false;
    }
    return true;
}

// The per-window plan of one row of `len` pairs scaled to a group of `rows` rows against the same bases (msm.hip: msm_run_batch): the
// same pipeline over rows x nwin bucket sets, set s = row * nwin + w.
inline BucketPlan bucket_plan_rows(const BucketPlan &row, size_t rows) {
    BucketPlan p = row;
    p.n_wide_sets = p.nsums = (unsigned)(rows * row.nwin);
    p.NB = rows * row.NB; p.E = rows * row.E;
    p.max_tasks = p.NB + p.E / p.seg + 1;
    return p;
}

// windows (= bucket additions per pair) and window width the per-window pipeline picks for `len` pairs
inline void msm_plan_query(size_t len, unsigned scalar_bits, unsigned *nwin, unsigned *c) {
    BucketPlan p;
    bucket_plan(WindowLayout{}, len ? len : 1, scalar_bits, 0, p);
    *nwin = p.nwin; *c = p.c;
}

}  // namespace pm
