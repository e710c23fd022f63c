// Everything a proving key decides before its first allocation: the domain, the logical base concatenation (layout.hpp: key_shape),
// the pair ranges of the three merged MSMs, this rank's resident pieces and where they sit in HBM, the quotient segments of all ranks --
// and, once the base points are resident, which merged MSM gets window tables, which the wide mode and which neither (table_grants).
// Plain C++ on layout.hpp and csrc/msm_plan.h: the key builder of api.hip only reserves memory and launches, and the CPU self-test
// (tests/native/key_plan_selftest.cpp, which pins a recorded grid of plans and grants) shares it.  Nothing here touches a device.
#pragma once
#include <algorithm>
#include <array>

#include "../csrc/msm_plan.h"
#include "layout.hpp"

namespace pm {

// Merged MSM k (0 = a, 1 = c, 2 = d) reads the logical pairs [msm_lo[k], msm_lo[k] + msm_len[k]) of the concatenation; this rank holds
// `pieces[k]` of them (ranges of the concatenation, res_cnt[k] pairs in all), stored back to back from element res_dev_off[k] of the
// key's base array.  PM_SHARD_PAIRS: one contiguous piece per MSM, the 1/N slice of its range; the prover's scalar vectors are whole and
// this rank reads them from the piece's first pair on.  PM_SHARD_VECTOR (layout.hpp): the pieces follow the blocked coefficient
// layout, the prover builds only this rank's scalars (in piece order) and `segs` is this rank's part of the quotient index space.
struct KeyPlan : pmlayout::KeyShape {   // n, m0, mw, nr, sigma, base_len[], seg_off[], total_points: the whole key's
    unsigned log_n = 0;
    int shard_rank = 0, shard_count = 1, layout = PM_SHARD_PAIRS;
    uint64_t msm_lo[3] = {0}, msm_len[3] = {0};
    std::vector<pmlayout::Piece> pieces[3];
    uint64_t res_cnt[3] = {0}, res_dev_off[3] = {0};
    std::vector<pmlayout::Segment> segs;
    uint64_t max_seg = 0;
    struct SegRef { uint64_t a, b; uint32_t rank, idx; };
    std::vector<SegRef> all_segs;   // the segments of ALL ranks in increasing index order (the carry chain of the division scan)
    size_t seg_slots = 0;           // max over ranks of the segment count

    // the whole logical concatenation is resident, in its own order: device offsets are logical offsets
    bool whole_resident() const { return shard_count == 1 && layout == PM_SHARD_PAIRS; }
    uint64_t resident_points() const { return whole_resident() ? total_points : res_cnt[0] + res_cnt[1] + res_cnt[2]; }
    // f(cat_lo, count, dev_off) for every resident range of the concatenation; stops at the first nonzero return and hands it on
    template <class F>
    int for_resident(F f) const {
        if (whole_resident()) return f((uint64_t)0, total_points, (uint64_t)0);
        for (int k = 0; k < 3; ++k) {
            uint64_t at = res_dev_off[k];
            for (const pmlayout::Piece &pc : pieces[k]) {
                if (const int r = f(pc.cat_lo, pc.count, at)) return r;
                at += pc.count;
            }
        }
        return 0;
    }
};

// max_seg_override: PM_OPT_MAX_SEG_LOG as a segment size (test knob: many tiny sub-segments), 0 = pick_max_seg.
inline int key_plan(int two_adicity, uint64_t m0, uint64_t mw, uint64_t nr, int shard_rank, int shard_count, int layout, uint64_t max_seg_override,
                    KeyPlan &p) {
    p = KeyPlan();
    if (m0 < 1 || shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return PM_ERR_INVALID_ARG;
    if (layout != PM_SHARD_PAIRS && layout != PM_SHARD_VECTOR) return PM_ERR_INVALID_ARG;
    p.layout = layout; p.shard_rank = shard_rank; p.shard_count = shard_count;
    const uint64_t rows = 2 * (m0 + nr);               // common.rs:131-135
    uint64_t n = 1;
    while (n < rows) { n <<= 1; ++p.log_n; }           // Radix2EvaluationDomain::new, generator.rs:60
    if (p.log_n > (unsigned)two_adicity) return PM_ERR_DOMAIN_TOO_LARGE;
    pmlayout::KeyShape &ks = p;
    ks = pmlayout::key_shape(n, m0, mw, nr);
    p.msm_lo[0] = ks.off_xp;   p.msm_len[0] = n + 3;                          // x_powers | y_alpha[0..2]
    p.msm_lo[1] = 0;           p.msm_len[1] = ks.off_ygz;                     // everything before y_gamma_z
    p.msm_lo[2] = ks.off_ygz;  p.msm_len[2] = pmlayout::numerator_len(n) - 1; // the quotient has one coefficient fewer
    const uint64_t N = (uint64_t)shard_count, q = (uint64_t)shard_rank;
    if (layout == PM_SHARD_VECTOR) {
        if (!pmlayout::layout_ok(n, (uint32_t)N)) return PM_ERR_INVALID_ARG;   // N a power of two, N^2 | n
        p.max_seg = max_seg_override ? max_seg_override : pmlayout::pick_max_seg(n, (uint32_t)N);
        for (uint32_t r = 0; r < (uint32_t)N; ++r) {
            const std::vector<pmlayout::Segment> sr = pmlayout::quotient_segments(n, (uint32_t)N, r, p.max_seg);
            p.seg_slots = std::max(p.seg_slots, sr.size());
            for (size_t i = 0; i < sr.size(); ++i) p.all_segs.push_back(KeyPlan::SegRef{sr[i].a, sr[i].b, r, (uint32_t)i});
            if (r == q) p.segs = sr;
        }
        std::sort(p.all_segs.begin(), p.all_segs.end(), [](const KeyPlan::SegRef &x, const KeyPlan::SegRef &y) { return x.a < y.a; });
        uint64_t at = 0;                                   // the ranks' segments must tile [0, len) exactly
        for (const KeyPlan::SegRef &e : p.all_segs) {
            if (e.a != at || e.b <= e.a) return PM_ERR_STATE;
            at = e.b;
        }
        if (at != pmlayout::numerator_len(n)) return PM_ERR_STATE;
        const pmlayout::Layout L = pmlayout::make_layout(n, (uint32_t)N, (uint32_t)q);
        p.pieces[0] = pmlayout::pieces_a(ks, L);
        p.pieces[1] = pmlayout::pieces_c(ks, L);
        p.pieces[2] = pmlayout::pieces_d(ks, p.segs);
    } else {
        for (int k = 0; k < 3; ++k) {
            const uint64_t lo = p.msm_len[k] * q / N, hi = p.msm_len[k] * (q + 1) / N;
            p.pieces[k] = {pmlayout::Piece{p.msm_lo[k] + lo, hi - lo}};
        }
    }
    for (int k = 0; k < 3; ++k)
        for (const pmlayout::Piece &pc : p.pieces[k]) p.res_cnt[k] += pc.count;
    if (p.whole_resident()) {
        for (int k = 0; k < 3; ++k) p.res_dev_off[k] = p.msm_lo[k];
    } else {   // device layout [c pairs | a pairs | d pairs]
        p.res_dev_off[1] = 0;
        p.res_dev_off[0] = p.res_cnt[1];
        p.res_dev_off[2] = p.res_dev_off[0] + p.res_cnt[0];
    }
    return PM_OK;
}

// ------------------------------------------------------------------------------- window tables of a resident key
// What merged MSM k of a resident key runs on: its own window tables (WindowLayout = tables_plan's), the WIDE mode on the plain base
// array (wide_plan's; one infinity-flag byte per point), or neither: the per-window pipeline.
struct Grant {
    enum Kind { NONE, TABLES, WIDE } kind = NONE;
    WindowLayout layout;
};

// Budget: free HBM minus the per-proof vectors (~40 Fr per domain point; 26 are in use) and the MSM workspaces: 16 B per (pair, window)
// entry of the sort's two ping-pong arrays and the sorted indices, 13-16 windows, plus the bucket-side arrays -> 256 B per pair of one
// <= max_piece-pair piece, for the main context's largest MSM and for the helper context's [a]_1 MSM (prove.hip).  inflight
// (PM_INFLIGHT_CONTEXTS): how many contexts will prove on this key at once, each with vectors and workspaces of its own.  vec_n: length
// of a rank's vectors.  Tables are granted per MSM, smallest first, while they fit.  An MSM whose tables do not fit (the 10n-pair
// [d]_1 of a 2^24-gate key on one GPU: 515 GB) or have no plan at all (windows x points would overflow the u32 table indices: the
// same MSM) gets the wide mode -- the same sort / accumulate / reduce kernels on the plain array, one bucket set per window, 13
// additions per pair instead of the 16 of the one-shot pipeline -- from 2^18 pairs a piece up; PM_TABLES_NO_WIDE disables that,
// PM_TABLES_WIDE (test / tuning) gives it to every MSM at any size and tables to none.  forced_option: PM_OPT_TABLE_WINDOW_BITS.
inline std::array<Grant, 3> table_grants(size_t free_bytes, int inflight, uint64_t vec_n, const uint64_t res_cnt[3], uint64_t max_piece,
                                         long long tables_mode, unsigned forced_option, unsigned fr_bits, size_t table_point_bytes) {
    std::array<Grant, 3> grants;
    if (tables_mode == PM_TABLES_OFF) return grants;
    double budget = 0.9 * (double)free_bytes - (double)inflight * 64.0 * 40.0 * (double)vec_n;
    budget -= (double)inflight * 256.0 * (double)std::min(res_cnt[2], max_piece);
    budget -= (double)inflight * 256.0 * (double)res_cnt[0];
    const WindowOption forced = decode_window_option(forced_option);
    const bool force_wide = tables_mode == PM_TABLES_WIDE;
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int x, int y) { return res_cnt[x] < res_cnt[y]; });
    for (int k : order) {
        const uint64_t len = res_cnt[k];
        if (!len) continue;
        const WindowLayout tb = tables_plan((size_t)len, 1, (size_t)len, fr_bits, forced);
        const double need = tb.planned() ? (double)len * tb.nwin * table_point_bytes + (double)len : 1e300;
        if (need > budget || force_wide) {
            const size_t piece = (size_t)std::min(len, max_piece);
            const WindowLayout wt = tables_mode == PM_TABLES_NO_WIDE ? WindowLayout() : wide_plan(piece, forced);
            if (wt.planned() && (piece >= ((size_t)1 << 18) || force_wide) && (double)len < budget) {
                budget -= (double)len;
                grants[k] = Grant{Grant::WIDE, wt};
            }
            continue;
        }
        budget -= need;
        grants[k] = Grant{Grant::TABLES, tb};
    }
    return grants;
}

}  // namespace pm
