// Host build of host/key_plan.hpp (plain C++): everything a proving key decides before its first allocation, and which of its merged
// MSMs get window tables, checked without a GPU.
//   (a) identities of key_plan over n = 2^2 ... 2^14 x ranks x m0 x both layouts x sub-segment sizes, and the refused arguments,
//   (b) anchors: grants on record in the repository, as literal values,
//   (c) key_plan_table.txt: full KeyPlan rows for the shapes on record and table_grants rows over free memory x contexts in flight x
//       tables mode x forced window option x piece size x scalar field, RECORDED FROM api.hip AS IT STOOD BEFORE THE PLAN MOVED INTO THE
//       HEADER (pk_init_layout and the budget block of pk_build_tables at commit f925dff, copied into a scratch program with the device
//       calls replaced by parameters).  A plan change shows as a differing row; `--print` writes the table in the same format, for
//       whoever changes a plan on purpose -- and for tests/test_gpu_key_plan.py, which holds resident keys against its K rows.
// Built and run by tests/test_native_key_plan.py, a second time under -fsanitize=address,undefined.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../polymath_amd/host/key_plan.hpp"

using namespace pm;

static int fails = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            ++fails;                           \
            printf("FAIL %s: ", #cond);        \
            printf(__VA_ARGS__);               \
            printf("\n");                      \
        }                                      \
    } while (0)

// ---- (a)
static int identity_cases = 0;
static void identities_of(uint64_t n, int N, uint64_t m0, int layout, uint64_t max_seg) {
    const uint64_t nr = n / 2 - m0, mw = 5, Lz = 2 * m0 + mw + nr, len = pmlayout::numerator_len(n);   // 2 (m0 + nr) = n rows
    ++identity_cases;
    std::vector<KeyPlan> rank((size_t)N);
    uint64_t sum[3] = {0, 0, 0};
    size_t most_segs = 0;
    std::vector<std::pair<uint64_t, uint64_t>> all;
    for (int q = 0; q < N; ++q) {
        KeyPlan &p = rank[(size_t)q];
        const int st = key_plan(32, m0, mw, nr, q, N, layout, max_seg, p);
        CHECK(st == PM_OK, "n %llu N %d m0 %llu layout %d max_seg %llu rank %d: status %d", (unsigned long long)n, N, (unsigned long long)m0, layout,
              (unsigned long long)max_seg, q, st);
        if (st != PM_OK) return;
        CHECK(p.n == n && p.sigma == n + 3 && ((uint64_t)1 << p.log_n) == n && p.base_len[PM_X_POWERS_Y_GAMMA_Z] == len, "n %llu: the domain", (unsigned long long)n);
        uint64_t total = 0;
        for (int v : pmlayout::CAT_ORDER) {
            CHECK(p.seg_off[v] == total, "n %llu: vector %d does not follow its predecessor", (unsigned long long)n, v);
            total += p.base_len[v];
        }
        CHECK(total == p.total_points, "n %llu: total", (unsigned long long)n);
        for (int k = 0; k < 3; ++k) {
            uint64_t cnt = 0;
            for (const pmlayout::Piece &pc : p.pieces[k]) {
                cnt += pc.count;
                CHECK(pc.cat_lo >= p.msm_lo[k] && pc.cat_lo + pc.count <= p.msm_lo[k] + p.msm_len[k], "n %llu N %d rank %d: a piece of MSM %d outside its range",
                      (unsigned long long)n, N, q, k);
            }
            CHECK(cnt == p.res_cnt[k], "n %llu N %d rank %d: res_cnt[%d]", (unsigned long long)n, N, q, k);
            sum[k] += cnt;
        }
        CHECK(p.whole_resident() == (N == 1 && layout == PM_SHARD_PAIRS), "whole_resident");
        if (p.whole_resident()) {
            CHECK(p.res_dev_off[0] == p.msm_lo[0] && p.res_dev_off[1] == p.msm_lo[1] && p.res_dev_off[2] == p.msm_lo[2] && p.resident_points() == p.total_points,
                  "n %llu: a whole key is resident in logical order", (unsigned long long)n);
        } else {   // c | a | d
            CHECK(p.res_dev_off[1] == 0 && p.res_dev_off[0] == p.res_cnt[1] && p.res_dev_off[2] == p.res_cnt[1] + p.res_cnt[0] &&
                      p.resident_points() == p.res_cnt[0] + p.res_cnt[1] + p.res_cnt[2], "n %llu N %d rank %d: res_dev_off", (unsigned long long)n, N, q);
        }
        std::vector<std::pair<uint64_t, uint64_t>> dev;   // the resident ranges tile the device array
        p.for_resident([&](uint64_t, uint64_t count, uint64_t at) { dev.push_back({at, at + count}); return 0; });
        std::sort(dev.begin(), dev.end());
        uint64_t dev_end = 0;
        for (const auto &d : dev) { CHECK(d.first == dev_end, "n %llu N %d rank %d: a gap or an overlap on the device at %llu", (unsigned long long)n, N, q, (unsigned long long)dev_end); dev_end = d.second; }
        CHECK(dev_end == p.resident_points(), "n %llu N %d rank %d: %llu resident points", (unsigned long long)n, N, q, (unsigned long long)dev_end);
        most_segs = std::max(most_segs, p.segs.size());
        for (const pmlayout::Segment &g : p.segs) all.push_back({g.a, g.b});
        CHECK(layout == PM_SHARD_VECTOR ? p.max_seg == (max_seg ? max_seg : pmlayout::pick_max_seg(n, (uint32_t)N)) : p.max_seg == 0 && p.segs.empty() && p.all_segs.empty(),
              "n %llu N %d: max_seg %llu", (unsigned long long)n, N, (unsigned long long)p.max_seg);
    }
    if (layout == PM_SHARD_VECTOR) {
        std::sort(all.begin(), all.end());
        uint64_t at = 0;
        for (const auto &s : all) {
            CHECK(s.first == at && s.second > s.first && s.second - s.first <= rank[0].max_seg, "n %llu N %d max_seg %llu: segment [%llu, %llu) after %llu",
                  (unsigned long long)n, N, (unsigned long long)max_seg, (unsigned long long)s.first, (unsigned long long)s.second, (unsigned long long)at);
            at = s.second;
        }
        CHECK(at == len, "n %llu N %d: the segments end at %llu of %llu", (unsigned long long)n, N, (unsigned long long)at, (unsigned long long)len);
        for (int q = 0; q < N; ++q) {
            const KeyPlan &p = rank[(size_t)q];
            CHECK(p.seg_slots == most_segs && p.all_segs.size() == all.size(), "n %llu N %d rank %d: seg_slots %zu of %zu", (unsigned long long)n, N, q, p.seg_slots, most_segs);
            for (size_t i = 0; i < p.all_segs.size() && i < all.size(); ++i)
                if (p.all_segs[i].a != all[i].first || p.all_segs[i].b != all[i].second) { CHECK(false, "n %llu N %d rank %d: all_segs[%zu]", (unsigned long long)n, N, q, i); break; }
        }
        // [a]: every u block once, r_a's two pairs; [c]: z_tail, h, the 2 r_a u blocks with one extra base each, 3 + 2; [d]: every index but 0
        CHECK(sum[0] == n + 2 && sum[1] == Lz + (n - 1) + n + (uint64_t)N * N + 5 && sum[2] == len - 1, "n %llu N %d: pairs over the ranks %llu %llu %llu", (unsigned long long)n, N,
              (unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2]);
    } else {   // contiguous slices of the three logical ranges
        CHECK(sum[0] == n + 3 && sum[1] == Lz + (n - 1) + (n + 1) + 5 && sum[2] == len - 1, "n %llu N %d: pairs over the ranks %llu %llu %llu", (unsigned long long)n, N,
              (unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2]);
        for (int q = 0; q < N; ++q)
            for (int k = 0; k < 3; ++k)
                CHECK(rank[(size_t)q].pieces[k].size() == 1 && (q == 0 ? rank[0].pieces[k][0].cat_lo == rank[0].msm_lo[k]
                                                                         : rank[(size_t)q].pieces[k][0].cat_lo == rank[(size_t)q - 1].pieces[k][0].cat_lo + rank[(size_t)q - 1].pieces[k][0].count),
                      "n %llu N %d rank %d: MSM %d is not the next slice", (unsigned long long)n, N, q, k);
    }
}
static void identities() {
    for (unsigned lg = 2; lg <= 14; ++lg)
        for (int N : {1, 2, 4, 8})
            for (uint64_t m0 : {1, 2, 3})
                for (int layout : {(int)PM_SHARD_PAIRS, (int)PM_SHARD_VECTOR}) {
                    const uint64_t n = (uint64_t)1 << lg;
                    if (!pmlayout::layout_ok(n, (uint32_t)N) || m0 > n / 2) continue;   // n = 4 has room for m0 <= 2
                    if (layout == PM_SHARD_PAIRS) identities_of(n, N, m0, layout, 0);
                    else for (uint64_t max_seg : {(uint64_t)2, (uint64_t)8, (uint64_t)0}) identities_of(n, N, m0, layout, max_seg);
                }
    // the refusals, with the statuses api.hip has always returned for them
    KeyPlan p;
    CHECK(key_plan(32, 0, 10, 9, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_ERR_INVALID_ARG, "m0 = 0");
    CHECK(key_plan(32, 2, 10, 9, 2, 2, PM_SHARD_PAIRS, 0, p) == PM_ERR_INVALID_ARG && key_plan(32, 2, 10, 9, -1, 2, PM_SHARD_PAIRS, 0, p) == PM_ERR_INVALID_ARG &&
              key_plan(32, 2, 10, 9, 0, 0, PM_SHARD_PAIRS, 0, p) == PM_ERR_INVALID_ARG, "a rank outside the count");
    CHECK(key_plan(32, 2, 10, 9, 0, 3, PM_SHARD_VECTOR, 0, p) == PM_ERR_INVALID_ARG && key_plan(32, 2, 10, 9, 0, 3, PM_SHARD_PAIRS, 0, p) == PM_OK, "3 ranks: pair slices only");
    CHECK(key_plan(32, 2, 2, 1, 0, 4, PM_SHARD_VECTOR, 0, p) == PM_ERR_INVALID_ARG && key_plan(32, 2, 10, 9, 0, 8, PM_SHARD_VECTOR, 0, p) == PM_ERR_INVALID_ARG, "N^2 > n");
    CHECK(key_plan(32, 2, 10, 9, 0, 1, 2, 0, p) == PM_ERR_INVALID_ARG, "an unknown layout");
    CHECK(key_plan(28, 2, 10, (uint64_t)1 << 27, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_ERR_DOMAIN_TOO_LARGE && key_plan(28, 2, 10, ((uint64_t)1 << 27) - 2, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_OK &&
              p.log_n == 28 && key_plan(32, 2, 10, (uint64_t)1 << 27, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_OK && p.log_n == 29, "a domain beyond the two-adicity");
}

// ---- (b)
constexpr size_t GB = (size_t)1 << 30;
constexpr uint64_t P27 = (uint64_t)1 << 27, P20 = (uint64_t)1 << 20;
static void anchors() {
    KeyPlan p;
    {   // a whole BLS12-381 key of 2^20 - 100 gates on an idle 288 GB card: every MSM has tables
        CHECK(key_plan(32, 2, 1048477, 1048476, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_OK && p.n == 2097152, "2^20 - 100 gates");
        // the pair counts of the msm_plan block of profiles/r06_final_bench_2p20_1gpu.json
        CHECK(p.res_cnt[0] == 2097155 && p.res_cnt[1] == 6291266 && p.res_cnt[2] == 20971542, "2^20 - 100 gates: pairs %llu %llu %llu", (unsigned long long)p.res_cnt[0],
              (unsigned long long)p.res_cnt[1], (unsigned long long)p.res_cnt[2]);
        const auto g = table_grants(288 * GB, 1, p.n, p.res_cnt, P27, PM_TABLES_AUTO, 0, 255, 128);
        // the same block: [a] 13 windows of 20 bits, [c] 12 windows, 22 bits, tables for both
        CHECK(g[0].kind == Grant::TABLES && g[0].layout.m == 1 && g[0].layout.nwin == 13 && g[0].layout.widest() == 20, "[a]: %u windows", g[0].layout.nwin);
        CHECK(g[1].kind == Grant::TABLES && g[1].layout.nwin == 12 && g[1].layout.widest() == 22, "[c]: %u windows", g[1].layout.nwin);
        // [d] since the radix-5 tables (profiles/msm_radix5_ab.txt: 11 windows of radix 5 * 2^21, reported as 24 bits; [c] 12 windows of 5 * 2^19)
        CHECK(g[2].kind == Grant::TABLES && g[2].layout.m == 5 && g[2].layout.nwin == 11 && g[2].layout.a == 21 && g[2].layout.widest() == 24, "[d]: %u windows", g[2].layout.nwin);
        CHECK(g[1].layout.m == 5 && g[1].layout.a == 19, "[c]: radix 5 * 2^%u", g[1].layout.a);
        // ... and with the power-of-two plans forced (100), [d] as that record has it: 12 windows, 22 bits
        const auto f = table_grants(288 * GB, 1, p.n, p.res_cnt, P27, PM_TABLES_AUTO, 100, 255, 128);
        CHECK(f[2].kind == Grant::TABLES && f[2].layout.m == 1 && f[2].layout.nwin == 12 && f[2].layout.widest() == 22, "[d] forced to powers of two: %u windows", f[2].layout.nwin);
    }
    {   // a whole key of 2^24 - 100 gates: [d]_1 has no table plan and runs wide on 12 windows of 22 / 21 bits ("a 12 x 22/21-bit plan
        // has 16.8 M buckets"), [a] and [c] keep tables
        CHECK(key_plan(32, 2, 16777117, 16777116, 0, 1, PM_SHARD_PAIRS, 0, p) == PM_OK && p.n == 33554432 && p.res_cnt[2] == 335544342, "2^24 - 100 gates");
        const auto g = table_grants(288 * GB, 1, p.n, p.res_cnt, P27, PM_TABLES_AUTO, 0, 255, 128);
        CHECK(g[2].kind == Grant::WIDE && g[2].layout.wide && g[2].layout.nwin == 12 && g[2].layout.widest() == 22 && win_width(12, 4) == 21 && g[2].layout.total_buckets() == 16777216,
              "[d] at 2^24: kind %d, %u windows", (int)g[2].kind, g[2].layout.nwin);
        // by hand: 0.9 x 288 GiB - 2560 n - 256 (2^27 + 33.5 M) = 149 GB; [a]'s 11 x 33.5 M x 128 B = 47 GB fit, after them [c]'s 11 x 100.7 M x 128 B = 142 GB do not
        CHECK(g[0].kind == Grant::TABLES && g[0].layout.nwin == 11 && g[1].kind == Grant::WIDE && g[1].layout.nwin == 12, "[a] and [c] at 2^24: %d %d", (int)g[0].kind, (int)g[1].kind);
        const auto no_wide = table_grants(288 * GB, 1, p.n, p.res_cnt, P27, PM_TABLES_NO_WIDE, 0, 255, 128);
        CHECK(no_wide[2].kind == Grant::NONE && no_wide[0].kind == Grant::TABLES, "PM_TABLES_NO_WIDE at 2^24");
    }
    const uint64_t small[3] = {35, 92, 342};   // 9 gates
    for (long long mode = 0; mode < 4; ++mode) {
        const auto g = table_grants(288 * GB, 1, 32, small, P27, mode, 0, 255, 128);
        for (int k = 0; k < 3; ++k)   // wide below 2^18 pairs only when forced
            CHECK(g[k].kind == (mode == PM_TABLES_OFF ? Grant::NONE : mode == PM_TABLES_WIDE ? Grant::WIDE : Grant::TABLES), "9 gates, mode %lld, MSM %d: kind %d", mode, k, (int)g[k].kind);
    }
}

// ---- (c)
static std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
struct Fnv {   // FNV-1a over 64-bit words: the digest of a segment list (the ranks of a 2^24-gate key have thousands of segments)
    uint64_t h = 1469598103934665603ull;
    void add(uint64_t v) {
        for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xFF; h *= 1099511628211ull; }
    }
};
struct KeyArgs {
    int two_adicity;
    uint64_t m0, mw, nr;
    int rank, count, layout;
    uint64_t max_seg;   // 0: pick_max_seg
};
// "K two_adicity m0 mw nr rank count layout max_seg : status" and, for a plan, " : n log_n sigma : base_len x 6 : seg_off x 6 : total :
// msm_lo x 3 : msm_len x 3 : res_cnt x 3 : res_dev_off x 3 : max_seg seg_slots : a <pieces> : c <pieces> : d <pieces> : segs <count>
// <digest> : all <count> <digest>", a piece as cat_lo+count
static std::string key_row(const KeyArgs &k) {
    KeyPlan p;
    const int status = key_plan(k.two_adicity, k.m0, k.mw, k.nr, k.rank, k.count, k.layout, k.max_seg, p);
    std::string r = fmt("K %d %llu %llu %llu %d %d %d %llu : %d", k.two_adicity, (unsigned long long)k.m0, (unsigned long long)k.mw, (unsigned long long)k.nr, k.rank,
                        k.count, k.layout, (unsigned long long)k.max_seg, status);
    if (status != PM_OK) return r;
    auto list = [&](const uint64_t *v, int count) {
        r += " :";
        for (int i = 0; i < count; ++i) r += fmt(" %llu", (unsigned long long)v[i]);
    };
    r += fmt(" : %llu %u %llu", (unsigned long long)p.n, p.log_n, (unsigned long long)p.sigma);
    list(p.base_len, PM_NUM_BASE_VECS);
    list(p.seg_off, PM_NUM_BASE_VECS);
    list(&p.total_points, 1);
    list(p.msm_lo, 3);
    list(p.msm_len, 3);
    list(p.res_cnt, 3);
    list(p.res_dev_off, 3);
    r += fmt(" : %llu %zu", (unsigned long long)p.max_seg, p.seg_slots);
    for (int m = 0; m < 3; ++m) {
        r += fmt(" : %c", "acd"[m]);
        for (const pmlayout::Piece &pc : p.pieces[m]) r += fmt(" %llu+%llu", (unsigned long long)pc.cat_lo, (unsigned long long)pc.count);
    }
    Fnv s, a;
    for (const pmlayout::Segment &g : p.segs) { s.add(g.a); s.add(g.b); s.add(g.loc0); s.add(g.qoff); s.add(g.kind); s.add(g.halo); }
    for (const KeyPlan::SegRef &e : p.all_segs) { a.add(e.a); a.add(e.b); a.add(e.rank); a.add(e.idx); }
    return r + fmt(" : segs %zu %016llx : all %zu %016llx", p.segs.size(), (unsigned long long)s.h, p.all_segs.size(), (unsigned long long)a.h);
}
struct GrantArgs {
    size_t free_bytes;
    int inflight;
    uint64_t vec_n, res_cnt[3], max_piece;
    long long tables_mode;
    unsigned forced, fr_bits;
    size_t point_bytes;
};
// "G free inflight vec_n res_cnt x 3 max_piece tables_mode forced fr_bits point_bytes" and per MSM a, c, d " : outcome m windows a wide widest"
static std::string grant_row(const GrantArgs &g) {
    std::string r = fmt("G %zu %d %llu %llu %llu %llu %llu %lld %u %u %zu", g.free_bytes, g.inflight, (unsigned long long)g.vec_n, (unsigned long long)g.res_cnt[0],
                        (unsigned long long)g.res_cnt[1], (unsigned long long)g.res_cnt[2], (unsigned long long)g.max_piece, g.tables_mode, g.forced, g.fr_bits, g.point_bytes);
    for (const Grant &t : table_grants(g.free_bytes, g.inflight, g.vec_n, g.res_cnt, g.max_piece, g.tables_mode, g.forced, g.fr_bits, g.point_bytes))
        r += fmt(" : %s %u %u %u %d %u", t.kind == Grant::TABLES ? "tables" : t.kind == Grant::WIDE ? "wide" : "none", t.layout.m, t.layout.nwin, t.layout.a, (int)t.layout.wide,
                 t.layout.widest());
    return r;
}

// the shapes on record: the reference's dummy circuit (n = 8), the synthetic circuits of 9, 2^16 - 100, 2^20 - 100 and 2^24 - 100 gates
// (m0 = 2, one witness per gate and one more)
struct Circuit { uint64_t m0, mw, nr; };
static const Circuit CIRCUITS[] = {{2, 2, 1}, {2, 10, 9}, {2, 65437, 65436}, {2, 1048477, 1048476}, {2, 16777117, 16777116}};
static std::vector<KeyArgs> key_cases() {
    std::vector<KeyArgs> v;
    for (const Circuit &c : CIRCUITS)
        for (int layout : {(int)PM_SHARD_PAIRS, (int)PM_SHARD_VECTOR})
            for (int count : {1, 2, 4, 8})
                for (int rank = 0; rank < count; ++rank) v.push_back(KeyArgs{32, c.m0, c.mw, c.nr, rank, count, layout, 0});
    for (int c = 0; c < 2; ++c)   // PM_OPT_MAX_SEG_LOG: many tiny sub-segments
        for (uint64_t max_seg : {2, 8})
            for (int rank = 0; rank < 2; ++rank) v.push_back(KeyArgs{28, CIRCUITS[c].m0, CIRCUITS[c].mw, CIRCUITS[c].nr, rank, 2, PM_SHARD_VECTOR, max_seg});
    // refused: no instance column, a rank outside the count, 3 ranks, N^2 > n, an unknown layout, a domain of 2^29 on a field with 2^28-th roots
    v.push_back(KeyArgs{32, 0, 10, 9, 0, 1, PM_SHARD_PAIRS, 0});
    v.push_back(KeyArgs{32, 2, 10, 9, 2, 2, PM_SHARD_PAIRS, 0});
    v.push_back(KeyArgs{32, 2, 10, 9, 0, 3, PM_SHARD_VECTOR, 0});
    v.push_back(KeyArgs{32, 2, 2, 1, 0, 4, PM_SHARD_VECTOR, 0});
    v.push_back(KeyArgs{32, 2, 10, 9, 0, 1, 2, 0});
    v.push_back(KeyArgs{28, 2, 10, (uint64_t)1 << 27, 0, 1, PM_SHARD_PAIRS, 0});
    return v;
}
// vector length and the pairs of the three resident MSMs (a, c, d): whole keys of 2^16 - 100, 2^20 - 100 and 2^24 - 100 gates, and about
// what rank 0 of 8 holds of the last
struct Resident { uint64_t vec_n, res_cnt[3]; };
static const Resident RESIDENT[] = {{131072, {131075, 393026, 1310742}},
                                    {2097152, {2097155, 6291266, 20971542}},
                                    {33554432, {33554435, 100663106, 335544342}},
                                    {4194304, {4194306, 12582900, 41943043}}};
static std::vector<GrantArgs> grant_cases() {
    std::vector<GrantArgs> v;
    const size_t free_bytes[] = {3 * GB, 64 * GB, 192 * GB, 288 * GB};
    auto add = [&](const Resident &r, size_t fb, int inflight, uint64_t max_piece, long long mode, unsigned forced, unsigned bits) {
        v.push_back(GrantArgs{fb, inflight, r.vec_n, {r.res_cnt[0], r.res_cnt[1], r.res_cnt[2]}, max_piece, mode, forced, bits, 128});
    };
    for (const Resident &r : RESIDENT)
        for (size_t fb : free_bytes)
            for (long long mode = 0; mode < 4; ++mode) {
                for (int inflight : {1, 2, 4}) add(r, fb, inflight, P27, mode, 0, 255);
                add(r, fb, 1, P27, mode, 0, 254);   // bn254
                add(r, fb, 1, P20, mode, 0, 255);
            }
    for (const Resident &r : RESIDENT)
        for (size_t fb : {64 * GB, 288 * GB})
            for (long long mode : {1, 2})
                for (unsigned forced : {16u, 511u})
                    for (uint64_t max_piece : {P27, P20}) add(r, fb, 1, max_piece, mode, forced, 255);
    return v;
}
static std::vector<std::string> table() {
    std::vector<std::string> rows;
    for (const KeyArgs &k : key_cases()) rows.push_back(key_row(k));
    for (const GrantArgs &g : grant_cases()) rows.push_back(grant_row(g));
    return rows;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        printf("usage: key_plan_selftest <key_plan_table.txt> | --print\n");
        return 2;
    }
    const std::vector<std::string> rows = table();
    if (!strcmp(argv[1], "--print")) {
        for (const std::string &r : rows) printf("%s\n", r.c_str());
        return 0;
    }
    identities();
    printf("identities: %d failures of %d cases\n", fails, identity_cases);
    const int before_anchors = fails;
    anchors();
    printf("anchors: %d failures\n", fails - before_anchors);
    const int before_table = fails;
    std::ifstream in(argv[1]);
    std::string line;
    size_t i = 0;
    for (; std::getline(in, line); ++i) {
        if (i >= rows.size() || line != rows[i]) {
            ++fails;
            printf("row %zu differs\n  recorded %s\n  planned  %s\n", i, line.c_str(), i < rows.size() ? rows[i].c_str() : "(none)");
        }
    }
    CHECK(i == rows.size(), "%zu rows recorded, %zu planned", i, rows.size());
    printf("recorded table: %d failures of %zu rows\n", fails - before_table, rows.size());
    return fails ? 1 : 0;
}
