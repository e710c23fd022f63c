// Host build of csrc/msm_plan.h (plain C++): everything an MSM decides before its first launch, checked without a GPU.
//   (a) identities of the window layout for every window count 10 ... 32,
//   (b) anchors: plans on record in DESIGN.md section 4.2 and the GPU tests, as literal values,
//   (c) msm_plan_table.txt: the planners' full results over a grid of sizes, both scalar fields and forced option values, RECORDED
//       FROM THE PLANNERS AS THEY STOOD BEFORE THEY MOVED INTO THE HEADER (setup.hip: tables_plan / wide_plan, msm.hip: bucket_plan,
//       msm_reduce.hip: reduce_two_level at commit acf243e).  A plan change shows as a differing row; `--print` writes the table in
//       the same format, for whoever changes a plan on purpose.
// Built and run by tests/test_native_msm_plan.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../polymath_amd/csrc/msm_plan.h"

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

constexpr unsigned BLS = (unsigned)BlsFrP::BITS, BN = (unsigned)BnFrP::BITS;
// the [c]_1 and [d]_1 pair counts of a 2^20-gate BLS12-381 key (pm_pk_msm_plan), and [d]_1 at 2^24 gates
constexpr size_t PAIRS_C_2P20 = 6291266, PAIRS_D_2P20 = 20971542, PAIRS_D_2P24 = 335544342;

// ---- (a)
template <class P>
static void radix5_shifts(const char *name) {
    for (unsigned n = 10; n <= 32; ++n) {
        const WindowLayout t = radix5_layout(n, (unsigned)P::BITS);
        CHECK(t.planned() == (n <= RADIX5_MAX_WINDOWS), "%s: radix 5 on %u windows", name, n);
        if (!t.planned()) continue;
        CHECK(t.m == 5 && t.nwin == n && !t.wide && t.widest() == t.a + 3, "%s: radix-5 layout of %u windows", name, n);
        CHECK(radix_top_fits<P>(5, n, t.a) && !radix_top_fits<P>(5, n, t.a - 1), "%s: %u windows, a = %u is not the smallest shift that fits", name, n, t.a);
    }
}
static void layout_identities() {
    for (unsigned n = 10; n <= 32; ++n) {
        unsigned sum = 0;
        for (unsigned w = 0; w < n; ++w) {
            sum += win_width(n, w);
            CHECK(win_off(n, w + 1) == win_off(n, w) + win_width(n, w), "n = %u, w = %u", n, w);
            CHECK(w == 0 || win_width(n, w) <= win_width(n, w - 1), "n = %u: window %u is wider than the one before", n, w);
            CHECK(win_width(n, w) == (256 + n - 1) / n || win_width(n, w) + 1 == (256 + n - 1) / n, "n = %u, w = %u", n, w);
        }
        CHECK(sum == 256 && win_off(n, 0) == 0 && win_off(n, n) == 256, "n = %u: widths sum to %u", n, sum);
        CHECK(pow2_layout(n).widest() == (256 + n - 1) / n && win_width(n, 0) == (256 + n - 1) / n, "n = %u: widest", n);
        const BucketSets s = pow2_layout(n, true).sets();
        CHECK(s.n_wide + s.n_narrow == n && s.wide_b == (size_t)1 << (pow2_layout(n).widest() - 1), "n = %u: wide sets", n);
        CHECK(s.n_narrow == 0 ? s.narrow_b == s.wide_b : s.n_wide == 256 % n && 2 * s.narrow_b == s.wide_b && s.narrow_b >= 32768, "n = %u: narrow sets", n);
        CHECK(win_base(n, n, (uint32_t)s.wide_b, (uint32_t)s.narrow_b) == s.total(), "n = %u: win_base past the last window", n);
        CHECK(pow2_layout(n, true).total_buckets() == s.total(), "n = %u", n);
        const BucketSets one = pow2_layout(n).sets();
        CHECK(one.n_wide == 1 && one.n_narrow == 0 && one.total() == s.wide_b, "n = %u: the shared set", n);
    }
    static_assert(pow2_layout(12, true).total_buckets() == 16777216, "12 windows of 22 / 21 bits: 4 x 2^21 + 8 x 2^20 buckets");
    static_assert(win_off(12, 4) == 88 && win_width(12, 3) == 22 && win_width(12, 4) == 21, "the layout is a constant expression");
    static_assert(pad_to_regions(40960) == 65536 && pad_to_regions(163840) == 163840 && pad_to_regions(5120) == 5120, "whole regions when more than one");
    radix5_shifts<BlsFrP>("bls12_381");
    radix5_shifts<BnFrP>("bn254");
}

// ---- (b)
static WindowLayout forced_tables(size_t pairs, unsigned bits, unsigned option) { return tables_plan(pairs, 1, pairs, bits, decode_window_option(option)); }
static void anchors() {
    BucketPlan p;
    {   // [d]_1 and [c]_1 of a 2^20-gate BLS12-381 key
        const WindowLayout d = forced_tables(PAIRS_D_2P20, BLS, 0), c = forced_tables(PAIRS_C_2P20, BLS, 0);
        CHECK(d.m == 5 && d.nwin == 11 && d.a == 21 && !d.wide && d.widest() == 24, "[d]: m %u nwin %u a %u", d.m, d.nwin, d.a);
        CHECK(bucket_plan(d, PAIRS_D_2P20, BLS, 0, p) && p.NB == 5242880 && p.regions == 160 && p.two_level && p.reduce_wide.K0 == 40 && p.pbd == 512,
              "[d]: NB %zu regions %u K0 %u", p.NB, p.regions, p.reduce_wide.K0);
        CHECK(c.m == 5 && c.nwin == 12 && c.a == 19 && !c.wide && c.widest() == 22, "[c]: m %u nwin %u a %u", c.m, c.nwin, c.a);
        CHECK(bucket_plan(c, PAIRS_C_2P20, BLS, 0, p) && p.NB == 1310720 && p.regions == 40 && p.two_level && p.reduce_wide.K0 == 10 && p.pbd == 512,
              "[c]: NB %zu regions %u K0 %u", p.NB, p.regions, p.reduce_wide.K0);
    }
    for (unsigned bits : {BLS, BN})
        for (size_t pairs : {(size_t)1, (size_t)1000, (size_t)1 << 11, (size_t)1 << 17, (size_t)2097155, ((size_t)1 << 22) - 1})
            CHECK(forced_tables(pairs, bits, 0).m == 1 && forced_tables(pairs, bits, 0).planned(), "%zu pairs: radix 5 below 2^22", pairs);
    {   // the forced small radices of the GPU tests
        WindowLayout t = forced_tables((size_t)1 << 13, BLS, 516);
        CHECK(t.m == 5 && t.nwin == 16 && t.a == 14, "516");
        CHECK(bucket_plan(t, (size_t)1 << 13, BLS, 0, p) && (size_t)5 << (t.a - 1) == 40960 && p.NB == 65536 && p.regions == 2, "516: NB %zu regions %u", p.NB, p.regions);
        t = forced_tables((size_t)1 << 14, BLS, 514);
        CHECK(t.m == 5 && t.nwin == 14 && t.a == 16, "514");
        CHECK(bucket_plan(t, (size_t)1 << 14, BLS, 0, p) && p.NB == 163840 && p.regions == 5, "514: NB %zu regions %u", p.NB, p.regions);
        t = forced_tables((size_t)1 << 17, BLS, 16);
        CHECK(t.m == 1 && t.nwin == 16 && t.widest() == 16 && win_width(16, 15) == 16, "16");
        CHECK(bucket_plan(t, (size_t)1 << 17, BLS, 0, p) && p.NB == 32768 && p.regions == 1 && p.two_level && p.reduce_wide.ok, "16: NB %zu", p.NB);
        t = forced_tables((size_t)1 << 11, BLS, 12);
        CHECK(t.m == 1 && t.nwin == 22 && t.widest() == 12 && win_width(22, 13) == 12 && win_width(22, 14) == 11, "12");
        CHECK(bucket_plan(t, (size_t)1 << 11, BLS, 0, p) && p.NB == 2048 && p.regions == 1 && p.lo_buckets == 2048 && !p.two_level && p.pbd == 256, "12: NB %zu", p.NB);
    }
    for (size_t pairs : {PAIRS_C_2P20, PAIRS_D_2P20, (size_t)1 << 24}) {   // 100: the power-of-two plan of the cost model
        const WindowLayout t = forced_tables(pairs, BLS, 100);
        CHECK(t.m == 1 && t.nwin == 12 && t.widest() == 22, "100 at %zu pairs: m %u nwin %u", pairs, t.m, t.nwin);
    }
    CHECK(!forced_tables(PAIRS_D_2P24, BLS, 0).planned(), "335 M pairs: windows x points pass the u32 table indices");
    {
        const WindowLayout t = wide_plan((size_t)1 << 27);
        CHECK(t.wide && t.m == 1 && t.nwin == 12 && t.widest() == 22, "wide_plan(2^27): nwin %u", t.nwin);
        CHECK(bucket_plan(t, (size_t)1 << 27, BLS, 0, p) && p.regions == 512 && p.pbd == 1024 && p.n_wide_sets == 4 && p.n_narrow_sets == 8 && p.NB == 16777216,
              "wide_plan(2^27): regions %u lanes %u", p.regions, p.pbd);
    }
    // one decoding: what names nothing plans like 0, what is malformed plans nothing
    CHECK(decode_window_option(0).kind == WindowOption::NONE && decode_window_option(3).kind == WindowOption::NONE && decode_window_option(25).kind == WindowOption::NONE &&
              decode_window_option(99).kind == WindowOption::NONE, "values that name nothing");
    CHECK(decode_window_option(4).kind == WindowOption::WIDEST && decode_window_option(24).c == 24 && decode_window_option(15).wide_c() == 0 &&
              decode_window_option(16).wide_c() == 16 && decode_window_option(23).wide_c() == 23 && decode_window_option(24).wide_c() == 0, "widest window");
    CHECK(decode_window_option(100).kind == WindowOption::RADIX && decode_window_option(100).m == 1 && decode_window_option(100).nwin == 0 &&
              decode_window_option(511).m == 5 && decode_window_option(511).nwin == 11 && decode_window_option(532).kind == WindowOption::RADIX, "100 m + windows");
    CHECK(decode_window_option(200).kind == WindowOption::INVALID && decode_window_option(109).kind == WindowOption::INVALID &&
              decode_window_option(133).kind == WindowOption::INVALID && decode_window_option(509).kind == WindowOption::INVALID, "malformed values");
    CHECK(!forced_tables((size_t)1 << 20, BLS, 300).planned() && !forced_tables((size_t)1 << 24, BLS, 517).planned(), "no plan for 300 and 517");
    CHECK(!wide_plan((size_t)1 << 27, decode_window_option(17)).planned() && wide_plan((size_t)1 << 27, decode_window_option(511)).nwin == 12, "wide_plan: 17 matches nothing, 511 plans like 0");
}

// ---- (c)
static std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
static std::string shape_text(const ReduceShape &s) {
    return fmt(" : %u %u %zu %zu %zu %zu %zu", s.K0, s.R1, s.set_lanes, s.lanes0, s.lanes1, s.blocks0, s.blocks1);
}
// "<kind> <pairs> <bits> <option> : planned m windows a wide widest : ok" and, for a plan the kernels can run, every BucketPlan field
// in declaration order (Horner widths run-length coded) ": K0 R1 set_lanes lanes0 lanes1 blocks0 blocks1" of the wide and the narrow sets
static std::string row_text(char kind, size_t pairs, unsigned bits, unsigned option, const WindowLayout &t) {
    std::string r = fmt("%c %zu %u %u : %d %u %u %u %d %u", kind, pairs, bits, option, t.planned() ? 1 : 0, t.m, t.nwin, t.a, (int)t.wide, t.widest());
    BucketPlan p;
    if (!bucket_plan(t, pairs, bits, 0, p)) return r + " : 0";
    r += fmt(" : 1 %d %d %u %u %zu %zu %zu %zu %zu %u %u %u %u %zu %zu %u %u %u %u %u %zu %zu %d %u %u %u %u ", (int)p.tables, (int)p.wide, p.nwin, p.c, p.len, p.E,
             p.NB1, p.NBn, p.NB, p.n_wide_sets, p.n_narrow_sets, p.win_buckets, p.narrow_buckets, p.seg, p.max_tasks, p.chunk, p.nchunks, p.lo_buckets,
             p.regions, p.pbd, p.plds, p.keys_bytes, (int)p.two_level, p.red_lanes, p.red_block, p.bpw, p.nsums);
    for (unsigned i = 0; i < p.nsums;) {
        unsigned j = i;
        while (j < p.nsums && p.width[j] == p.width[i]) ++j;
        r += fmt("%s%ux%u", i ? "+" : "", j - i, (unsigned)p.width[i]);
        i = j;
    }
    return r + shape_text(p.reduce_wide) + shape_text(p.reduce_narrow);
}
static std::vector<std::string> table() {
    std::vector<std::string> rows;
    const size_t pairs[] = {(size_t)1 << 11, (size_t)1 << 13, (size_t)1 << 14, (size_t)1 << 17, (size_t)1 << 20, ((size_t)1 << 22) - 1, (size_t)1 << 22,
                            PAIRS_C_2P20, PAIRS_D_2P20, (size_t)1 << 24, (size_t)1 << 27};
    for (size_t n : pairs)
        for (unsigned bits : {BLS, BN})
            for (unsigned f : {0u, 12u, 16u, 24u, 100u, 110u, 500u, 511u, 512u, 514u, 516u}) rows.push_back(row_text('T', n, bits, f, forced_tables(n, bits, f)));
    for (size_t piece : {(size_t)1 << 18, (size_t)1 << 20, (size_t)1 << 24, (size_t)1 << 27})
        for (unsigned f : {0u, 16u, 17u, 18u, 19u, 20u, 21u, 22u, 23u}) rows.push_back(row_text('W', piece, BLS, f, wide_plan(piece, decode_window_option(f))));
    return rows;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        printf("usage: msm_plan_selftest <msm_plan_table.txt> | --print\n");
        return 2;
    }
    const std::vector<std::string> rows = table();
    if (!strcmp(argv[1], "--print")) {
        for (const std::string &r : rows) printf("%s\n", r.c_str());
        return 0;
    }
    layout_identities();
    printf("layout identities: %d failures\n", fails);
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
