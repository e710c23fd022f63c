// The witness solver's indicator rows (polymath_amd/host/solve_plan.hpp: indicator_row, KIND_INDICATOR; polymath_amd/csrc/divrem.cuh:
// marker_byte, indicator_of) on the CPU.  The accepted shapes against hand-written plans; byte 3 anywhere else (an ordinary row, beside
// a second unknown, a bit of a decomposition, a pair's flag), where it is what the plain marker is; two assignments that mark one
// column with different markers, and marker_byte on the three markers and their near-misses; a corpus (a width-40 decoder, a table
// walk, a system that mixes indicators with a division and an is-zero pair) on which build_plan_any_order equals build_plan field by
// field in matrix order and which, reversed and under seeded permutations, plans with every column at its in-order level and
// EXECUTES -- serially, with the host field type and the routine the kernels call -- to the in-order assignment; the same corpus with
// the plain marker, which plans as it always did and sticks at the hit row; and a guard row that waits for its index.
// Built and run by tests/test_native_solve_indicator.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include "solve_selftest.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit Suite(const char *n) : Rig(n) {}

    // ---- 1. the accepted shapes, against plans written by hand.  0 one | 1 inp, 2 b given | 3 u
    //   k u * guard = 0  with u in A or in B, k = 1 or 7, guard = inp - 3, 3 - inp or inp - b
    void shapes() {
        const Fr one = F::one(), m1 = F::neg(one);
        const Row guards[3] = {{{one, 1}, {F::neg(u(3)), 0}}, {{u(3), 0}, {m1, 1}}, {{one, 1}, {m1, 2}}};
        static const char *const GUARD[3] = {"inp - i", "i - inp", "a - b"};
        for (int u_in_b = 0; u_in_b < 2; ++u_in_b)
            for (uint64_t k : {1ull, 7ull})
                for (int g = 0; g < 3; ++g) {
                    const std::string tag = std::string("shapes: u in ") + (u_in_b ? "B" : "A") + ", k = " + std::to_string(k) + ", guard " + GUARD[g];
                    System s; s.mw = 3;
                    const Row lone = {{u(k), 3}};
                    s.add(u_in_b ? guards[g] : lone, u_in_b ? lone : guards[g], Row{});
                    const std::vector<uint8_t> unknown = s.unknown({}, {}, {3});
                    for (uint32_t wide : {WIDE_STEPS, 1u}) {
                        const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                        bool ok = p.error == OK && p.message.empty() && p.steps.size() == 1 && p.divs.empty() && p.pairs.empty() && p.bit_cols.empty() && !p.reordered;
                        if (ok) {
                            Step want{0, 0, 3, KIND_INDICATOR, 1};
                            want.cols_off = (uint32_t)u_in_b;
                            ok = same_step(p.steps[0], want) && p.level_ptr == std::vector<uint32_t>({0, 1}) && p.launches.size() == 1 &&
                                 same_launch(p.launches[0], wide == 1 ? Launch{0, 1, LAUNCH_INDICATOR, 0} : Launch{0, 1, LAUNCH_CHAIN, 0});
                        }
                        check(ok, tag + ": the plan is the hand-written one, and its launch does not divide");
                        check(same_plan(p, q), tag + ": the any-order builder gives the same plan");
                        if (!ok) continue;
                        std::vector<Fr> hit = {one, u(3), u(3), indicator_marker()}, miss = {one, u(4), u(9), indicator_marker()};
                        check(execute(s, p, hit) == NONE && hit[3].eq(one) && rows_hold(s, hit), tag + ": the guard is zero: field one, whatever k is");
                        check(execute(s, p, miss) == NONE && miss[3].is_zero() && rows_hold(s, miss), tag + ": the guard is not zero: field zero");
                    }
                    const Plan bare = in_order(s, unknown, WIDE_STEPS, false);
                    check(bare.error == OK && bare.steps.size() == 1 && bare.steps[0].kind == (u_in_b ? KIND_B : KIND_A), tag + ": without the modulus the rule is off");
                }
    }

    // ---- 2. byte 3 has meaning in the indicator row only
    void marker_elsewhere() {
        const Fr one = F::one(), m1 = F::neg(one);
        const Row guard = {{one, 1}, {F::neg(u(3)), 0}};
        {   // the single unknown of a row of another shape: C_r not empty, a rest beside u, an empty other side.  0 one | 1 inp, 2 c given | 3 u
            struct Other { const char *what; Row a, b, c; uint32_t kind; };
            const std::vector<Other> others = {
                {"C_r not empty", Row{{one, 3}}, guard, Row{{one, 2}}, KIND_A},
                {"C_r not empty, u in B", guard, Row{{u(7), 3}}, Row{{one, 2}}, KIND_B},
                {"a rest beside u", Row{{one, 3}, {one, 2}}, guard, Row{}, KIND_A},
                {"u in C", guard, Row{{one, 2}}, Row{{one, 3}}, KIND_C},
                {"an empty other side", Row{{one, 3}}, Row{}, Row{}, KIND_A},
                {"an other side of zero coefficients", Row{{one, 3}}, Row{{F::zero(), 1}}, Row{}, KIND_A},
            };
            for (const Other &o : others) {
                System s; s.mw = 3;
                s.add(o.a, o.b, o.c);
                const Plan p = in_order(s, s.unknown({}, {}, {3})), plain = in_order(s, s.unknown({3}, {}, {})), q = any_order(s, s.unknown({}, {}, {3}));
                check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == o.kind && same_plan(p, plain) && same_plan(p, q),
                      std::string("marker elsewhere: ") + o.what + ": an ordinary step, the plan of the plain marker");
            }
            System s; s.mw = 3;
            s.add(Row{{one, 3}}, guard, Row{{one, 2}});
            const Plan p = in_order(s, s.unknown({}, {}, {3}));
            std::vector<Fr> z = {one, u(5), u(8), indicator_marker()};
            check(p.error == OK && execute(s, p, z) == NONE && z[3].eq(u(4)) && rows_hold(s, z), "marker elsewhere: u * (5 - 3) = 8 executes as the ordinary row it is");
        }
        {   // beside a second unknown it is a plain unknown: the opener's multiplier, and the pair's flag.  1 a, 2 b given | 3 flag, 4 m
            const Row lc = {{one, 1}, {m1, 2}};
            System s; s.mw = 4;
            s.add(lc, Row{{one, 4}}, Row{{one, 3}});
            s.add(lc, Row{{one, 0}, {m1, 3}}, Row{});
            const Plan plain = in_order(s, s.unknown({3, 4}, {}, {}));
            check(plain.error == OK && plain.steps.size() == 1 && plain.steps[0].kind == KIND_ISZERO, "marker elsewhere: the pair with plain markers");
            const Plan as_flag = in_order(s, s.unknown({4}, {}, {3})), as_multiplier = in_order(s, s.unknown({3}, {}, {4}));
            check(same_plan(as_flag, plain), "marker elsewhere: a byte-3 column as a pair's flag is the pair's flag");
            check(same_plan(as_multiplier, plain), "marker elsewhere: a byte-3 column beside a second unknown is a plain unknown (the opener's multiplier)");
            std::vector<Fr> z = {one, u(9), u(9), indicator_marker(), marker()};
            check(as_flag.error == OK && execute(s, as_flag, z) == NONE && z[3].is_zero() && z[4].is_zero() && rows_hold(s, z), "marker elsewhere: ... and the pair executes");
            // two unknowns that are no pair: refused with the words the plain marker gets
            System t; t.mw = 4;
            t.add(Row{{one, 3}}, Row{{one, 1}, {one, 4}}, Row{});
            const Plan refused = in_order(t, t.unknown({4}, {}, {3})), before = in_order(t, t.unknown({3, 4}, {}, {}));
            check(refused.error == ERR_MANY_UNKNOWNS && same_plan(refused, before) && same_plan(any_order(t, t.unknown({4}, {}, {3})), any_order(t, t.unknown({3, 4}, {}, {}))),
                  "marker elsewhere: an unknown on the guard's side: the refusal of the plain marker, word for word");
        }
        {   // bits with byte 3: a decomposition as before, and the kernels' marker test passes over all three markers.  1 x given | 2, 3, 4 bits
            System s; s.mw = 4;
            s.boolean(2); s.boolean(3); s.boolean(4);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}, {u(4), 4}});
            const Plan p = in_order(s, s.unknown({2}, {3}, {4}));
            std::vector<Fr> z = {one, u(6), marker(), quotient_marker(), indicator_marker()};
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_BITS_C && same_plan(p, in_order(s, s.unknown({2, 3, 4}, {}, {}))) && execute(s, p, z) == NONE &&
                      z[2].is_zero() && z[3].eq(one) && z[4].eq(one),
                  "marker elsewhere: a byte-3 column as a bit of a decomposition");
        }
        {   // boolean-pending first, then its guard: the guard row is the indicator step.  1 inp given | 2 u
            System s; s.mw = 2;
            s.boolean(2);
            s.add(Row{{one, 2}}, guard, Row{});
            const Plan p = in_order(s, s.unknown({}, {}, {2}));
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_INDICATOR && p.steps[0].row == 1, "marker elsewhere: a boolean-pending byte-3 column is taken by its guard row");
        }
    }

    // ---- 3. one pattern per batch compares the BYTES (solve.hip: k_solve_pattern on marker_byte).  0 one | 1 inp | 2 out_0, 3 out_1
    void markers() {
        const Fr one = F::one();
        const std::vector<Fr> first = {one, u(1), indicator_marker(), indicator_marker()}, second = {one, u(0), indicator_marker(), marker()};
        std::vector<uint8_t> pattern(4);
        uint64_t mismatch = NONE;
        for (uint64_t j = 0; j < 4; ++j) {
            pattern[j] = pm::marker_byte<P>(first[j]);
            if (pm::marker_byte<P>(second[j]) != pattern[j] && ((uint64_t)1 << 32 | j) < mismatch) mismatch = (uint64_t)1 << 32 | j;
        }
        check(pattern == std::vector<uint8_t>({0, 0, PATTERN_INDICATOR, PATTERN_INDICATOR}), "markers: the bytes of assignment 0");
        check(mismatch == ((uint64_t)1 << 32 | 3), "markers: assignment 1 differs from assignment 0 at column 3");
        check(pm::marker_byte<P>(marker()) == 1 && pm::marker_byte<P>(quotient_marker()) == 2 && pm::marker_byte<P>(indicator_marker()) == 3, "markers: the three markers give 1, 2 and 3");
        Fr near = marker();
        near.l[0] = 0xfffffffcu;
        Fr high = quotient_marker(), high3 = indicator_marker();
        high.l[7] = 0x7fffffffu;
        high3.l[7] = 0x7fffffffu;
        Fr both = quotient_marker();
        both.l[2] = 0xfffffffeu;      // bit 0 and bit 64 clear
        Fr near3 = marker(), other = marker();
        near3.l[2] = 0xfffffffcu;     // bit 65 clear as well
        other.l[4] = 0xfffffffeu;     // bit 128 clear: no marker's bit
        check(pm::marker_byte<P>(near) == 0 && pm::marker_byte<P>(high) == 0 && pm::marker_byte<P>(high3) == 0 && pm::marker_byte<P>(both) == 0 && pm::marker_byte<P>(near3) == 0 &&
                  pm::marker_byte<P>(other) == 0 && pm::marker_byte<P>(F::zero()) == 0 && pm::marker_byte<P>(F::neg(one)) == 0,
              "markers: nothing else is a marker");
        uint32_t limbs[8];
        uint64_t words[4];
        memcpy(limbs, indicator_marker().l, sizeof limbs);
        memcpy(words, limbs, sizeof words);
        check(pm::marker_byte_limbs(limbs) == 3 && words[1] == ~(uint64_t)1 && !words_less(words, modulus), "markers: the routine on limbs; the marker is 2^256 - 1 - 2^64 and >= r");
        // the two patterns are two plans: with the plain marker nothing is inferred, and the hit row sticks
        System s; s.mw = 3;
        s.add(Row{{one, 2}}, Row{{one, 1}}, Row{});
        s.add(Row{{one, 3}}, Row{{one, 1}, {F::neg(one), 0}}, Row{});
        const Plan with = in_order(s, pattern), without = in_order(s, s.unknown({2, 3}, {}, {}));
        check(with.error == OK && count_kind(with, KIND_INDICATOR) == 2 && with.launches.size() == 1 && !with.launches[0].divides, "markers: the indicator marker makes both guards indicator rows");
        check(without.error == OK && count_kind(without, KIND_A) == 2 && without.launches.size() == 1 && without.launches[0].divides, "markers: the plain marker leaves two ordinary dividing steps");
        std::vector<Fr> z = first, stuck = {one, u(1), marker(), marker()};
        check(with.error == OK && execute(s, with, z) == NONE && z[2].is_zero() && z[3].eq(one) && rows_hold(s, z), "markers: inp = 1 completes");
        check(without.error == OK && execute(s, without, stuck) == 1 && stuck[2].is_zero() && stuck[3].is_zero(), "markers: with the plain marker inp = 1 is stuck at row 1, the hit");
    }

    // ---- 4. the corpus
    struct Case {
        std::string what;
        System s;
        std::vector<uint32_t> unknown, quotients, indicators;
        std::vector<std::vector<uint32_t>> groups;      // rows that keep their relative order under every permutation (a pair's rows)
        std::vector<uint64_t> hit_rows;                 // per round: with plain markers the assignment is stuck at this row
        int rounds = 1;
        std::function<std::vector<Fr>(int)> given;      // round -> z with the given columns set, markers elsewhere
    };
    // circomlib's Decoder on column `inp`: `width` outputs from column `base` with their guard rows  out_i * (inp - i) = 0
    static void decoder(Case &c, uint32_t inp, uint32_t base, uint32_t width) {
        for (uint32_t i = 0; i < width; ++i) {
            Row guard = {{F::one(), inp}};
            if (i) guard.push_back({F::neg(u(i)), 0});
            c.s.add(Row{{F::one(), base + i}}, guard, Row{});
            c.indicators.push_back(base + i);
        }
    }
    static Row sum_of(uint32_t base, uint32_t width) {
        Row sum;
        for (uint32_t i = 0; i < width; ++i) sum.push_back({F::one(), base + i});
        return sum;
    }
    Case decoder40() {   // 0 one | 1 success | 2 inp given | 3 .. 42 out:  the guards, (sum out) * 1 = success, success (success - 1) = 0
        Case c; c.what = "decoder";
        const uint32_t width = 40;
        c.s.m0 = 2; c.s.mw = 1 + width;
        decoder(c, 2, 3, width);
        c.s.add(sum_of(3, width), Row{{F::one(), 0}}, Row{{F::one(), 1}});
        c.s.add(Row{{F::one(), 1}}, Row{{F::one(), 1}, {F::neg(F::one()), 0}}, Row{});
        c.unknown.push_back(1);
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 3;      // the hit first, last and in the middle
        c.hit_rows = {0, 39, 17};
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[2] = u(round == 0 ? 0 : round == 1 ? 39 : 17);
            for (uint32_t i = 0; i < width; ++i) z[3 + i] = indicator_marker();
            return z;
        };
        return c;
    }
    // 0 one | 1 the last index | 2 idx_0, 3 .. 3 + W table (given) | per step W out, success, W products and (but for the last step) the next index
    //   the guards; (sum out) * 1 = success; success (success - 1) = 0; out_i * table_i = p_i; (sum p_i) * 1 = the next index
    Case table_walk() {
        Case c; c.what = "table walk";
        const uint32_t width = 5, steps = 4, per = 2 * width + 2;
        c.s.m0 = 2; c.s.mw = 1 + width + steps * per - 1;
        uint32_t idx = 2;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t out = 3 + width + t * per, success = out + width, prod = success + 1, next = t == steps - 1 ? 1 : prod + width;
            decoder(c, idx, out, width);
            c.s.add(sum_of(out, width), Row{{F::one(), 0}}, Row{{F::one(), success}});
            c.s.add(Row{{F::one(), success}}, Row{{F::one(), success}, {F::neg(F::one()), 0}}, Row{});
            for (uint32_t i = 0; i < width; ++i) {
                c.s.add(Row{{F::one(), out + i}}, Row{{F::one(), 3 + i}}, Row{{F::one(), prod + i}});
                c.unknown.push_back(prod + i);
            }
            c.s.add(sum_of(prod, width), Row{{F::one(), 0}}, Row{{F::one(), next}});
            c.unknown.push_back(success);
            c.unknown.push_back(next);
            idx = next;
        }
        const size_t ncols = c.s.m0 + c.s.mw;
        const std::vector<uint32_t> indicators = c.indicators;
        c.rounds = 2;
        c.hit_rows = {3, 1};      // the first step's guard at idx_0
        c.given = [=](int round) {
            static const uint64_t TABLE[2][5] = {{2, 0, 4, 1, 3}, {1, 4, 0, 2, 2}};
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[2] = u(round ? 1 : 3);
            for (uint32_t i = 0; i < width; ++i) z[3 + i] = u(TABLE[round][i]);
            for (uint32_t j : indicators) z[j] = indicator_marker();
            return z;
        };
        return c;
    }
    // 0 one | 1 out | 2 a, 3 c given | 4, 5, 6 sel (indicators of a) | 7 w | 8 q, 9 rem | 10 flag, 11 m
    //   the guards of a decoder on a;  (10 sel_0 + 11 sel_1 + 12 sel_2) * 1 = w;  q * w = c - rem;  ark's pair on rem;  (q + flag + sel_1) * w = out
    Case mixed() {
        Case c; c.what = "mixed";
        c.s.m0 = 2; c.s.mw = 10;
        const Fr one = F::one(), m1 = F::neg(one);
        decoder(c, 2, 4, 3);
        c.s.add(Row{{u(10), 4}, {u(11), 5}, {u(12), 6}}, Row{{one, 0}}, Row{{one, 7}});
        c.s.add(Row{{one, 8}}, Row{{one, 7}}, Row{{one, 3}, {m1, 9}});
        const uint32_t b = c.s.boolean(10);
        c.s.add(Row{{one, 9}}, Row{{one, 11}}, Row{{one, 10}});
        c.s.add(Row{{one, 9}}, Row{{one, 0}, {m1, 10}}, Row{});
        c.groups.push_back({b, b + 1, b + 2});
        c.s.add(Row{{one, 8}, {one, 10}, {one, 5}}, Row{{one, 7}}, Row{{one, 1}});
        c.unknown = {1, 7, 9, 10, 11};
        c.quotients = {8};
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;      // rem != 0 and rem == 0
        c.hit_rows = {1, 2};
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[2] = u(round ? 2 : 1); z[3] = u(round ? 24 : 23); z[8] = quotient_marker();
            for (uint32_t j = 4; j < 7; ++j) z[j] = indicator_marker();
            return z;
        };
        return c;
    }
    void corpus() {
        std::vector<Case> cases;
        cases.push_back(decoder40());
        cases.push_back(table_walk());
        cases.push_back(mixed());
        for (Case &c : cases) {
            const std::vector<uint8_t> unknown = c.s.unknown(c.unknown, c.quotients, c.indicators);
            System &s = c.s;
            for (uint32_t wide : {WIDE_STEPS, 2u}) {
                const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                check(p.error == OK && count_kind(p, KIND_INDICATOR) == c.indicators.size() && p.divs.size() == c.quotients.size() && well_sorted(p), c.what + ": plans in order");
                check(same_plan(p, q) && !q.reordered, c.what + ": in order the any-order builder is build_plan, field by field");
            }
            const Plan p = in_order(s, unknown);
            if (p.error != OK) continue;
            if (c.what == "decoder")
                check(p.launches.size() == 2 && same_launch(p.launches[0], Launch{0, 40, LAUNCH_INDICATOR, 0}) && same_launch(p.launches[1], Launch{40, 41, LAUNCH_CHAIN, 0}) && p.levels() == 2,
                      "decoder: one indicator launch of its own, then the sum; neither divides");
            if (c.what == "table walk")
                check(p.launches.size() == 1 && same_launch(p.launches[0], Launch{0, (uint32_t)p.steps.size(), LAUNCH_CHAIN, 0}) && p.levels() == 12 && p.steps.size() == 4 * 12,
                      "table walk: one NON-dividing chain of 12 levels: only C-steps and indicators");
            if (c.what == "mixed")
                check(p.levels() == 5 && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_CHAIN && p.launches[0].divides && p.pairs.size() == 1, "mixed: one dividing chain (the division and the pair)");
            const std::vector<uint32_t> levels = column_levels(s, p);
            std::vector<std::vector<Fr>> want;
            for (int round = 0; round < c.rounds; ++round) {
                std::vector<Fr> z = c.given(round);
                bool ok = execute(s, p, z) == NONE && rows_hold(s, z);
                for (const Fr &v : z) ok = ok && !is_marker(v);
                check(ok, c.what + ": the in-order plan executes to an assignment that satisfies the rows");
                want.push_back(z);
            }
            if (c.what == "decoder") check(want[1][1].eq(F::one()) && want[1][3 + 39].eq(F::one()) && want[1][3].is_zero() && want[2][3 + 17].eq(F::one()), "decoder: the hit is where the index says");
            if (c.what == "table walk") check(want[0][1].eq(u(4)) && want[1][1].eq(u(1)), "table walk: 3 -> 1 -> 0 -> 2 -> 4 and 1 -> 4 -> 2 -> 0 -> 1");
            if (c.what == "mixed") check(want[0][7].eq(u(11)) && want[0][8].eq(u(2)) && want[0][9].eq(F::one()) && want[0][10].eq(F::one()) && want[1][9].is_zero() && want[1][10].is_zero(), "mixed: 23 = 2 * 11 + 1 and 24 = 2 * 12");
            {   // the plain marker on the indicator columns: the plan of today (ordinary dividing steps), stuck at the hit row
                std::vector<uint32_t> plain_cols = c.unknown;
                plain_cols.insert(plain_cols.end(), c.indicators.begin(), c.indicators.end());
                const std::vector<uint8_t> plain = s.unknown(plain_cols, c.quotients, {});
                const Plan t = in_order(s, plain);
                bool ok = t.error == OK && count_kind(t, KIND_INDICATOR) == 0 && t.steps.size() == p.steps.size() && column_levels(s, t) == levels;
                for (const Launch &l : t.launches) ok = ok && l.kind != LAUNCH_INDICATOR;
                for (size_t i = 0; ok && i < t.steps.size(); ++i)
                    if (std::find(c.indicators.begin(), c.indicators.end(), t.steps[i].col) != c.indicators.end()) ok = t.steps[i].kind == KIND_A;
                check(ok, c.what + ": with the plain marker the guards are ordinary kind-A steps at the same levels");
                for (int round = 0; ok && round < c.rounds; ++round) {
                    std::vector<Fr> z = c.given(round);
                    for (uint32_t j : c.indicators) z[j] = marker();
                    check(execute(s, t, z) == c.hit_rows[round], c.what + ": ... and the assignment is stuck at the hit row");
                }
            }
            const uint32_t nr = (uint32_t)s.nr();
            for (int variant = 0; variant < 4; ++variant) {
                std::vector<uint32_t> order(nr);
                for (uint32_t i = 0; i < nr; ++i) order[i] = variant == 0 ? nr - 1 - i : i;
                if (variant > 0)
                    for (uint32_t i = nr; i > 1; --i) std::swap(order[i - 1], order[next_u64() % i]);
                keep_groups(order, c.groups);
                System t = s.permuted(order);
                const std::string tag = c.what + (variant ? ", permutation " + std::to_string(variant) : std::string(", reversed"));
                for (uint32_t wide : {WIDE_STEPS, 2u}) {
                    const Plan q = any_order(t, unknown, wide);
                    check(q.error == OK && q.message.empty() && q.steps.size() == p.steps.size() && q.pairs.size() == p.pairs.size() && q.divs.size() == p.divs.size() &&
                              count_kind(q, KIND_INDICATOR) == c.indicators.size(),
                          tag + ": plans");
                    if (q.error != OK) continue;
                    check(q.reordered, tag + ": a reordered plan");
                    check(well_sorted(q), tag + ": sorted by (level, kind, row), launches in step");
                    check(column_levels(t, q) == levels, tag + ": every column keeps its level");
                    for (int round = 0; round < c.rounds; ++round) {
                        std::vector<Fr> z = c.given(round);
                        bool ok = execute(t, q, z) == NONE && z.size() == want[round].size();
                        for (size_t j = 0; ok && j < z.size(); ++j) ok = z[j].eq(want[round][j]);
                        check(ok, tag + ": executes to the in-order assignment");
                    }
                }
            }
        }
    }

    // ---- 5. a guard row that waits for its index: the index is computed by a LATER row.  0 one | 1 a, 2 b given | 3 idx, 4 out
    //   row 0: out * (idx - 5) = 0      row 1: (a + b) * 1 = idx
    void waiting_guard() {
        const Fr one = F::one();
        System s; s.mw = 4;
        s.add(Row{{one, 4}}, Row{{one, 3}, {F::neg(u(5)), 0}}, Row{});
        s.add(Row{{one, 1}, {one, 2}}, Row{{one, 0}}, Row{{one, 3}});
        const std::vector<uint8_t> unknown = s.unknown({3}, {}, {4});
        const Plan first = in_order(s, unknown), p = any_order(s, unknown);
        check(first.error == ERR_MANY_UNKNOWNS && first.error_row == 0, "waiting guard: in matrix order the guard has two unknowns and is refused");
        bool ok = p.error == OK && p.reordered && p.steps.size() == 2 && p.steps[0].kind == KIND_C && p.steps[0].row == 1 && p.steps[0].level == 1;
        if (ok) {
            Step want{0, 0, 4, KIND_INDICATOR, 2};
            ok = same_step(p.steps[1], want) && p.launches.size() == 1 && same_launch(p.launches[0], Launch{0, 2, LAUNCH_CHAIN, 0}) && well_sorted(p);
        }
        check(ok, "waiting guard: it waits for its index and is then taken as an indicator row, one level up");
        if (!ok) return;
        std::vector<Fr> hit = {one, u(2), u(3), marker(), indicator_marker()}, miss = {one, u(2), u(4), marker(), indicator_marker()};
        check(execute(s, p, hit) == NONE && hit[3].eq(u(5)) && hit[4].eq(one) && rows_hold(s, hit), "waiting guard: 2 + 3 = 5 hits");
        check(execute(s, p, miss) == NONE && miss[3].eq(u(6)) && miss[4].is_zero() && rows_hold(s, miss), "waiting guard: 2 + 4 = 6 misses");
        // width 1, reversed: the sum row  out * 1 = success  has the opener's shape and is examined first; the guard releases it
        //   0 one | 1 success | 2 inp given | 3 out
        System d; d.m0 = 2; d.mw = 2;
        d.add(Row{{one, 1}}, Row{{one, 1}, {F::neg(one), 0}}, Row{});
        d.add(Row{{one, 3}}, Row{{one, 0}}, Row{{one, 1}});
        d.add(Row{{one, 3}}, Row{{one, 2}}, Row{});
        const Plan q = any_order(d, d.unknown({1}, {}, {3}));
        check(q.error == OK && q.reordered && q.steps.size() == 2 && q.pairs.empty() && q.steps[0].kind == KIND_INDICATOR && q.steps[0].row == 2 && q.steps[0].level == 1 &&
                  q.steps[1].kind == KIND_C && q.steps[1].row == 1 && q.steps[1].level == 2,
              "released: a guard row releases an opener registered over its indicator (the released-multiplier case)");
        std::vector<Fr> z = {one, marker(), u(0), indicator_marker()};
        check(q.error == OK && execute(d, q, z) == NONE && z[1].eq(one) && z[3].eq(one) && rows_hold(d, z), "released: ... and executes");
    }

    int run() {
        shapes();
        marker_elsewhere();
        markers();
        corpus();
        waiting_guard();
        return report();
    }
};

int main() {
    rng_state = 0x13198A2E03707344ull;
    Suite<pm::BlsCurve> bls("bls12_381");
    Suite<pm::BnCurve> bn("bn254");
    return (bls.run() | bn.run()) ? 1 : 0;
}
