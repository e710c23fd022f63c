// The witness solver's any-order plan builder (polymath_amd/host/solve_plan.hpp: build_plan_any_order, the waiting-row scheduler), on
// the CPU.  An in-order corpus (a chain with all three kinds, one wide level with a consumer, decompositions of each kind, is-zero
// pairs in both forms at two levels, a mixed system) on which the new builder must equal build_plan field by field; the same corpus
// with its rows reversed and under seeded permutations (a pair's rows keep their relative order: opener before closer), where every
// case must plan, give every column its in-order level, come out sorted by (level, kind, row) and EXECUTE -- serially, with the host
// field type, the way the kernels do it -- to the in-order assignment, pairs with d != 0 and d = 0; the waiting cases by hand; the
// refusals, which carry build_plan's code, row, column and message; the stuck word's root-cause key; and the cost of a reversed chain.
// Built and run by tests/test_native_solve_order.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include <chrono>
#include "solve_selftest.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit Suite(const char *n) : Rig(n) {}

    // ---- the corpus.  No ordinary row has the opener's shape (one unknown alone on A or B, the other in C): the sides that hold a
    // column which a later row reads carry a constant beside it, so that a permuted order registers no opener that is none.
    struct Case {
        std::string what;
        System s;
        std::vector<uint32_t> unknown;                  // columns
        std::vector<std::vector<uint32_t>> groups;      // rows that keep their relative order under every permutation (a pair's rows)
        int rounds = 1;
        std::function<std::vector<Fr>(int)> given;      // round -> z with the given columns set, markers elsewhere
    };

    Case chain() {   // 1 x, 2 y given | w_1 .. w_n = columns 3 ..; w_0 = y.  Kinds C, A, B in turn, depth n
        Case c; c.what = "chain";
        const uint32_t n = 30;
        c.s.mw = 2 + n;
        const Fr one = F::one();
        for (uint32_t i = 1; i <= n; ++i) {
            const uint32_t prev = 1 + i, cur = 2 + i;
            if (i % 3 == 1) c.s.add(Row{{one, prev}, {one, 0}}, Row{{one, prev}, {one, 1}}, Row{{u(2), cur}});
            else if (i % 3 == 2) c.s.add(Row{{u(3), cur}, {one, 1}}, Row{{one, prev}}, Row{{one, prev}, {u(5), 0}});
            else c.s.add(Row{{one, prev}, {u(2), 0}}, Row{{one, cur}, {one, 0}}, Row{{one, 1}});
            c.unknown.push_back(cur);
        }
        const Fr x = rnd(), y = rnd();
        const size_t ncols = c.s.m0 + c.s.mw;
        c.given = [=](int) { std::vector<Fr> z(ncols, marker()); z[0] = F::one(); z[1] = x; z[2] = y; return z; };
        return c;
    }
    Case wide() {    // 1 x given | w_1 .. w_n | y: one level of n steps (kinds C and A), then one row that reads them all
        Case c; c.what = "wide";
        const uint32_t n = 40;
        c.s.mw = 2 + n;
        const Fr one = F::one();
        Row all = {{one, 0}};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t w = 2 + i;
            if (i % 2 == 0) c.s.add(Row{{one, 1}, {u(i + 1), 0}}, Row{{one, 1}}, Row{{one, w}});
            else c.s.add(Row{{one, w}, {one, 0}}, Row{{one, 1}}, Row{{one, 1}, {u(i + 1), 0}});
            all.push_back({u(i + 2), w});
            c.unknown.push_back(w);
        }
        c.s.add(all, Row{{one, 1}}, Row{{one, n + 2}});
        c.unknown.push_back(n + 2);
        const Fr x = rnd();
        const size_t ncols = c.s.m0 + c.s.mw;
        c.given = [=](int) { std::vector<Fr> z(ncols, marker()); z[0] = F::one(); z[1] = x; return z; };
        return c;
    }
    Case decompositions() {   // 1 g < 2^5, 2 x, 3 p = g x given | bits in C 4 .. 8, in A 9 .. 13, in B 14 .. 18 | 19 y
        Case c; c.what = "decompositions";
        c.s.mw = 19;
        const Fr one = F::one();
        Row inc, ina, inb;
        for (uint32_t i = 0; i < 5; ++i) {
            inc.push_back({u(1u << i), 4 + i});
            ina.push_back({u(3u << i), 9 + i});
            inb.insert(inb.begin(), {u(7u << i), 14 + i});      // stored in descending order
        }
        for (uint32_t j = 4; j < 9; ++j) c.s.boolean(j);
        c.s.add(Row{{one, 1}}, Row{{one, 0}}, inc);
        for (uint32_t j = 9; j < 14; ++j) c.s.boolean(j);
        c.s.add(ina, Row{{one, 2}}, Row{{u(3), 3}});
        for (uint32_t j = 14; j < 19; ++j) c.s.boolean(j);
        c.s.add(Row{{one, 2}}, inb, Row{{u(7), 3}});
        c.s.add(Row{{one, 19}, {one, 0}}, Row{{one, 2}}, Row{{one, 4}, {one, 10}, {one, 16}, {one, 2}});
        for (uint32_t j = 4; j <= 19; ++j) c.unknown.push_back(j);
        const Fr x = rnd();
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 3;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            const uint64_t g = round == 0 ? 21 : round == 1 ? 0 : 31;
            z[0] = F::one(); z[1] = u(g); z[2] = x; z[3] = F::mul(u(g), x);
            return z;
        };
        return c;
    }
    // 1 key, 2 t given | per value j < 3: v_j given, flag_j, m_j (columns 3 + 3 j ...) | 12 cnt | 13 flag', 14 m' | 15 out
    //   per value a pair on v_j - key; (sum flags + 1) * 1 = cnt; a pair on cnt - t (level 3); (flag' + 1) * key = out
    Case pairs(bool circom_form) {
        Case c; c.what = circom_form ? "pairs, circom" : "pairs, ark";
        c.s.mw = 15;
        const Fr one = F::one(), m1 = F::neg(one);
        Row sum = {{one, 0}};
        const auto gadget = [&](const Row &lc, uint32_t flag, uint32_t m) {
            std::vector<uint32_t> rows;
            if (!circom_form) rows.push_back(c.s.boolean(flag));
            circom_form ? circom(c.s, lc, flag, m) : ark(c.s, lc, flag, m);
            rows.push_back((uint32_t)c.s.nr() - 2);
            rows.push_back((uint32_t)c.s.nr() - 1);
            c.groups.push_back(rows);
            c.unknown.push_back(flag);
            c.unknown.push_back(m);
        };
        for (uint32_t j = 0; j < 3; ++j) {
            gadget(Row{{one, 3 + 3 * j}, {m1, 1}}, 4 + 3 * j, 5 + 3 * j);
            sum.push_back({one, 4 + 3 * j});
        }
        c.s.add(sum, Row{{one, 0}}, Row{{one, 12}});
        c.unknown.push_back(12);
        gadget(Row{{one, 12}, {m1, 2}}, 13, 14);
        c.s.add(Row{{one, 13}, {one, 0}}, Row{{one, 1}}, Row{{one, 15}});
        c.unknown.push_back(15);
        const Fr key = rnd(), other[3] = {rnd(), rnd(), rnd()};
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 4;   // every d != 0; every d = 0; mixed, the second-level pair both ways
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[1] = key;
            uint64_t equal = 0;
            for (uint32_t j = 0; j < 3; ++j) {
                const bool eq = round == 1 || (round >= 2 && j != 1);
                z[3 + 3 * j] = eq ? key : other[j];
                equal += eq;
            }
            const uint64_t cnt = 1 + (circom_form ? equal : 3 - equal);      // circom's flag is [d == 0], ark's [d != 0]
            z[2] = u(round == 1 || round == 3 ? cnt : cnt + 5);
            return z;
        };
        return c;
    }
    // 1 x, 2 g < 2^4 given | 3 w1 | bits 4 .. 7 | 8 w2 | 9 flag, 10 m | 11 y
    //   (x + 1)(x + 2) = w1;  g * 1 = bits;  (w2 + x) * (w1 + 1) = b0 + b1 + x;  ark's pair on g - 3;  (flag + w2 + 1) * x = y
    Case mixed() {
        Case c; c.what = "mixed";
        c.s.mw = 11;
        const Fr one = F::one();
        c.s.add(Row{{one, 1}, {one, 0}}, Row{{one, 1}, {u(2), 0}}, Row{{one, 3}});
        for (uint32_t j = 4; j < 8; ++j) c.s.boolean(j);
        c.s.add(Row{{one, 2}}, Row{{one, 0}}, Row{{u(8), 7}, {u(1), 4}, {u(4), 6}, {u(2), 5}});
        c.s.add(Row{{one, 8}, {one, 1}}, Row{{one, 3}, {one, 0}}, Row{{one, 4}, {one, 5}, {one, 1}});
        const uint32_t b = c.s.boolean(9);
        ark(c.s, Row{{one, 2}, {F::neg(u(3)), 0}}, 9, 10);
        c.groups.push_back({b, b + 1, b + 2});
        c.s.add(Row{{one, 9}, {one, 8}, {one, 0}}, Row{{one, 1}}, Row{{one, 11}});
        for (uint32_t j = 3; j <= 11; ++j) c.unknown.push_back(j);
        const Fr x = rnd();
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[1] = x; z[2] = u(round ? 3 : 13);
            return z;
        };
        return c;
    }

    // ---- 1 + 2. the corpus in order, reversed and permuted
    void corpus() {
        std::vector<Case> cases;
        cases.push_back(chain());
        cases.push_back(wide());
        cases.push_back(decompositions());
        cases.push_back(pairs(false));
        cases.push_back(pairs(true));
        cases.push_back(mixed());
        for (Case &c : cases) {
            const std::vector<uint8_t> unknown = c.s.unknown(c.unknown);
            System &s = c.s;
            for (uint32_t wide : {WIDE_STEPS, 2u}) {
                const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                check(p.error == OK && !p.steps.empty() && well_sorted(p), c.what + ": plans in order");
                check(same_plan(p, q) && !q.reordered, c.what + ": in order the new builder is build_plan, field by field");
            }
            const Plan p = in_order(s, unknown);
            const std::vector<uint32_t> levels = column_levels(s, p);
            std::vector<std::vector<Fr>> want;
            for (int round = 0; round < c.rounds; ++round) {
                std::vector<Fr> z = c.given(round);
                bool ok = execute(s, p, z) == NONE && rows_hold(s, z);
                for (const Fr &v : z) ok = ok && !is_marker(v);
                check(ok, c.what + ": the in-order plan executes to an assignment that satisfies the rows");
                want.push_back(z);
            }
            const uint32_t nr = (uint32_t)s.nr();
            for (int variant = 0; variant < 6; ++variant) {
                std::vector<uint32_t> order(nr);
                for (uint32_t i = 0; i < nr; ++i) order[i] = variant == 0 ? nr - 1 - i : i;
                if (variant > 0)
                    for (uint32_t i = nr; i > 1; --i) std::swap(order[i - 1], order[next_u64() % i]);
                keep_groups(order, c.groups);
                System t = s.permuted(order);
                const std::string tag = c.what + (variant ? ", permutation " + std::to_string(variant) : std::string(", reversed"));
                for (uint32_t wide : {WIDE_STEPS, 2u}) {
                    const Plan q = any_order(t, unknown, wide);
                    check(q.error == OK && q.message.empty() && q.steps.size() == p.steps.size() && q.pairs.size() == p.pairs.size(), tag + ": plans");
                    if (q.error != OK) continue;
                    check(variant != 0 || q.reordered, tag + ": build_plan refuses the reversed rows, the plan is a reordered one");
                    check(in_order(t, unknown, wide).error == OK ? !q.reordered : q.reordered, tag + ": reordered exactly where build_plan refuses");
                    check(well_sorted(q), tag + ": sorted by (level, kind, row), level_ptr and launches in step");
                    check(column_levels(t, q) == levels, tag + ": every column has its in-order level");
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

    // ---- 3. the waiting cases, by hand
    void waiting() {
        const Fr one = F::one(), m1 = F::neg(one);
        {   // booleanity rows AFTER the decomposition row.  1 g given | 2, 3 bits
            System s; s.mw = 3;
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{u(2), 3}, {one, 2}});
            s.boolean(2); s.boolean(3);
            const std::vector<uint8_t> unknown = s.unknown({2, 3});
            const Plan p = in_order(s, unknown), q = any_order(s, unknown);
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 0, "waiting: build_plan refuses a decomposition before its booleanity rows");
            check(q.error == OK && q.reordered && q.steps.size() == 1 && q.steps[0].row == 0 && q.steps[0].kind == KIND_BITS_C && q.steps[0].bits == 2 && q.steps[0].level == 1 &&
                      q.bit_cols == std::vector<uint32_t>({2, 3}) && q.launches.size() == 1 && q.launches[0].kind == LAUNCH_CHAIN,
                  "waiting: the decomposition row waits for its booleanity rows");
            std::vector<Fr> z = {one, u(2), marker(), marker()};
            check(q.error == OK && execute(s, q, z) == NONE && z[2].is_zero() && z[3].eq(one) && rows_hold(s, z), "waiting: ... and executes");
        }
        {   // a row that names the multiplier before the closer.  1 a, 2 b given | 3 flag, 4 m | 5 w
            //   row 0: (a - b) * m = flag     row 1: (w + 1) * 1 = m     row 2: (a - b) * (1 - flag) = 0
            System s; s.mw = 5;
            const Row lc = {{one, 1}, {m1, 2}};
            s.add(lc, Row{{one, 4}}, Row{{one, 3}});
            s.add(Row{{one, 5}, {one, 0}}, Row{{one, 0}}, Row{{one, 4}});
            s.add(lc, Row{{one, 0}, {m1, 3}}, Row{});
            const std::vector<uint8_t> unknown = s.unknown({3, 4, 5});
            const Plan p = in_order(s, unknown), q = any_order(s, unknown);
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 0 && p.message.find("names the multiplier") != std::string::npos, "waiting: build_plan refuses a row that names the multiplier");
            check(q.error == OK && q.reordered && q.steps.size() == 2 && q.steps[0].kind == KIND_ISZERO && q.steps[0].row == 2 && q.steps[0].level == 1 && q.pairs.size() == 1 &&
                      q.pairs[0].row1 == 0 && q.pairs[0].col_m == 4 && q.steps[1].kind == KIND_A && q.steps[1].row == 1 && q.steps[1].col == 5 && q.steps[1].level == 2,
                  "waiting: the row waits for the closer and is an ordinary step after it");
            for (int equal = 0; equal < 2 && q.error == OK; ++equal) {
                const Fr a = rnd(), b = equal ? a : rnd();
                std::vector<Fr> z = {one, a, b, marker(), marker(), marker()};
                check(execute(s, q, z) == NONE && rows_hold(s, z) && z[3].eq(equal ? F::zero() : one) && z[4].eq(F::inv(F::sub(a, b))) && z[5].eq(F::sub(z[4], one)),
                      "waiting: ... and executes, d != 0 and d = 0");
            }
        }
        {   // a * a = e before the row that determines a: a check row in the end.  1 x, 2 p, 3 e given | 4 a
            System s; s.mw = 4;
            s.add(Row{{one, 4}}, Row{{one, 4}}, Row{{one, 3}});
            s.add(Row{{one, 4}, {one, 0}}, Row{{one, 1}}, Row{{one, 2}});
            const std::vector<uint8_t> unknown = s.unknown({4});
            const Plan p = in_order(s, unknown), q = any_order(s, unknown);
            check(p.error == ERR_TWO_MATRICES && p.error_row == 0 && p.error_col == 4, "waiting: build_plan refuses a * a = e at once");
            check(q.error == OK && q.reordered && q.steps.size() == 1 && q.steps[0].row == 1 && q.steps[0].kind == KIND_A && q.steps[0].col == 4 && q.steps[0].level == 1,
                  "waiting: a * a = e waits and is a check row once another row determines a");
            const Fr a = rnd(), x = rnd();
            std::vector<Fr> z = {one, x, F::mul(F::add(a, one), x), F::mul(a, a), marker()};
            check(q.error == OK && execute(s, q, z) == NONE && z[4].eq(a) && rows_hold(s, z), "waiting: ... and executes");
        }
        {   // an ordinary row of the opener's shape, released when another row determines its "multiplier".  1 x given | 2 m, 3 t
            //   row 0: m * x = t     row 1: (x + 1) * x = m
            System s; s.mw = 3;
            s.add(Row{{one, 2}}, Row{{one, 1}}, Row{{one, 3}});
            s.add(Row{{one, 1}, {one, 0}}, Row{{one, 1}}, Row{{one, 2}});
            const std::vector<uint8_t> unknown = s.unknown({2, 3});
            const Plan q = any_order(s, unknown);
            check(q.error == OK && q.reordered && q.pairs.empty() && q.steps.size() == 2 && q.steps[0].row == 1 && q.steps[0].kind == KIND_C && q.steps[0].level == 1 &&
                      q.steps[1].row == 0 && q.steps[1].kind == KIND_C && q.steps[1].col == 3 && q.steps[1].level == 2,
                  "waiting: a registered opener is released by the row that determines its multiplier");
            const Fr x = rnd();
            std::vector<Fr> z = {one, x, marker(), marker()};
            check(q.error == OK && execute(s, q, z) == NONE && rows_hold(s, z) && z[3].eq(F::mul(F::mul(F::add(x, one), x), x)), "waiting: ... and executes");
        }
    }

    // ---- 4. refused in any order: build_plan's code, row, column, and its message as a prefix
    void refuse(System &s, const std::vector<uint8_t> &unknown, int code, const char *what, bool exact = false) {
        const Plan p = in_order(s, unknown), q = any_order(s, unknown);
        check(p.error == code && q.error == code && q.error_row == p.error_row && q.error_col == p.error_col && !p.message.empty() && q.message.find(p.message) == 0 &&
                  (exact ? q.message == p.message : q.message.find("; in any row order: ") == p.message.size()) && q.steps.empty() && q.launches.empty() && q.pairs.empty() &&
                  q.bit_cols.empty() && !q.reordered,
              what);
    }
    void refused() {
        const Fr one = F::one(), m1 = F::neg(one);
        {   // the "two unknowns" system: 0 one | 1 out | 2 a 3 c 4 inv 5 q 6 s 7 e 8 pad; a and inv both unknown
            System s; s.m0 = 2; s.mw = 7;
            s.add(Row{{u(3), 4}}, Row{{one, 2}}, Row{{one, 0}});
            s.add(Row{{one, 2}}, Row{{u(5), 5}}, Row{{one, 3}});
            s.add(Row{{one, 4}}, Row{{one, 5}}, Row{{one, 6}});
            s.add(Row{{one, 6}, {one, 0}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(Row{{one, 2}}, Row{{one, 2}}, Row{{one, 7}});
            refuse(s, s.unknown({1, 2, 4, 5, 6}), ERR_MANY_UNKNOWNS, "refused: two unknowns that no order separates");
            std::vector<uint8_t> col0 = s.unknown({1, 4, 5, 6});
            refuse(s, s.unknown({1, 4, 5, 6, 8}), ERR_UNDETERMINED, "refused: a column that no row names");
            col0[0] = 1;
            refuse(s, col0, ERR_COLUMN_ZERO, "refused: column 0, as it is", true);
            const Plan none = any_order(s, s.unknown({1, 2, 4, 5, 6}), WIDE_STEPS, false);
            check(none.error == ERR_MANY_UNKNOWNS && none.message == "row 0: two or more unknowns (columns 4 and 2)", "refused: without the modulus the any-order route is off");
        }
        for (int which = 0; which < 2; ++which) {   // 0 one | 1 out | 2 a 3 b given | 4 flag 5 m: an unclosed opener, a closer with another known side
            System s; s.m0 = 2; s.mw = 4;
            const Row lc = {{one, 2}, {m1, 3}};
            s.add(lc, Row{{one, 5}}, Row{{one, 4}});
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}});
            which == 0 ? s.add(Row{{one, 2}}, Row{{one, 0}}, Row{{one, 2}}) : s.add(Row{{one, 2}, {F::neg(u(2)), 3}}, Row{{one, 0}, {m1, 4}}, Row{});
            refuse(s, s.unknown({1, 4, 5}), ERR_MANY_UNKNOWNS, which ? "refused: a closer whose known side is not the opener's" : "refused: an opener that nothing closes");
            const Plan q = any_order(s, s.unknown({1, 4, 5}));
            check(q.error_row == 0 && q.error_col == 4 && q.message.find("row 0: two or more unknowns (columns 5 and 4)") == 0 &&
                      q.message.find(which ? "row 2: its known side" : "no later row closes it") != std::string::npos,
                  "refused: the pair's message is build_plan's");
        }
        {   // one bit more than bitlength(r) - 1, with its booleanity rows, in either order
            const uint32_t k = bit_length(modulus);
            System s; s.mw = 1 + k;
            Row bits;
            Fr c = one;
            for (uint32_t i = 0; i < k; ++i) {
                s.boolean(2 + i);
                bits.push_back({c, 2 + i});
                c = F::add(c, c);
            }
            s.add(Row{{one, 1}}, Row{{one, 0}}, bits);
            std::vector<uint32_t> cols;
            for (uint32_t i = 0; i < k; ++i) cols.push_back(2 + i);
            refuse(s, s.unknown(cols), ERR_MANY_UNKNOWNS, "refused: k + 1 bits");
            std::vector<uint32_t> order(k + 1);
            for (uint32_t i = 0; i <= k; ++i) order[i] = k - i;
            System t = s.permuted(order);
            refuse(t, t.unknown(cols), ERR_MANY_UNKNOWNS, "refused: k + 1 bits, the decomposition row first");
        }
    }

    // ---- 5. the stuck word names a root cause.  0 one | 1 out | 2 g, 3 h, 4 c2 given | 5 x, 6 y
    //   row 0: x * y = c2     row 1: g * x = h     row 2: y * 1 = out.     g = h = 0: row 1 sticks, x = 0, and then row 0 sticks too
    void root_cause() {
        const Fr one = F::one();
        System s; s.m0 = 2; s.mw = 5;
        s.add(Row{{one, 5}}, Row{{one, 6}}, Row{{one, 4}});
        s.add(Row{{one, 2}}, Row{{one, 5}}, Row{{one, 3}});
        s.add(Row{{one, 6}}, Row{{one, 0}}, Row{{one, 1}});
        const Plan q = any_order(s, s.unknown({1, 5, 6}));
        check(q.error == OK && q.reordered && q.steps.size() == 3 && q.steps[0].row == 1 && q.steps[0].kind == KIND_B && q.steps[0].level == 1 && q.steps[1].row == 0 &&
                  q.steps[1].kind == KIND_B && q.steps[1].level == 2 && q.steps[2].row == 2 && q.steps[2].kind == KIND_C && q.steps[2].level == 3,
              "root cause: the plan");
        if (q.error != OK) return;
        const Fr g = rnd(), x = rnd(), y = rnd();
        std::vector<Fr> z = {one, marker(), g, F::mul(g, x), F::mul(x, y), marker(), marker()};
        check(execute(s, q, z) == NONE && z[5].eq(x) && z[6].eq(y) && z[1].eq(y) && rows_hold(s, z), "root cause: g != 0 completes");
        std::vector<Fr> zero = {one, marker(), F::zero(), F::zero(), F::mul(x, y), marker(), marker()};
        std::vector<uint32_t> stuck_rows;
        const uint64_t key = execute(s, q, zero, &stuck_rows);
        uint32_t smallest = ~0u;
        for (uint32_t r : stuck_rows) smallest = r < smallest ? r : smallest;
        check(stuck_rows == std::vector<uint32_t>({1, 0}) && smallest == 0, "root cause: rows 1 and 0 both stick, and the smaller row is the consequence");
        check(key == ((uint64_t)1 << 32 | 1) && (key & 0xffffffffull) == 1, "root cause: the minimum over (level, row) is row 1");
        check(zero[5].is_zero() && zero[6].is_zero() && zero[1].is_zero(), "root cause: stuck steps store zero");
    }

    // ---- 6. a dependency chain of 2^18 rows stored in reverse: no sweep per level
    void blow_up() {
        const uint32_t n = 1u << 18;
        const Fr one = F::one();
        System fwd; fwd.mw = 1 + n;
        fwd.a.reserve(n); fwd.b.reserve(n); fwd.c.reserve(n);
        for (uint32_t i = 0; i < n; ++i) fwd.add(Row{{one, 1 + i}, {one, 0}}, Row{{one, 1 + i}, {u(2), 0}}, Row{{one, 2 + i}});
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = n - 1 - i;
        System rev = fwd.permuted(order);
        std::vector<uint8_t> unknown(fwd.m0 + fwd.mw, 1);
        unknown[0] = unknown[1] = 0;
        fwd.freeze(); rev.freeze();
        double best[2] = {1e30, 1e30};
        bool ok = true;
        for (int rep = 0; rep < 3; ++rep)
            for (int which = 0; which < 2; ++which) {
                const auto t0 = std::chrono::steady_clock::now();
                const Plan p = which ? build_plan_any_order(rev.m, n, rev.m0, rev.mw, unknown.data(), WIDE_STEPS, modulus)
                                     : build_plan(fwd.m, n, fwd.m0, fwd.mw, unknown.data(), WIDE_STEPS, modulus);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (ms < best[which]) best[which] = ms;
                ok = ok && p.error == OK && p.steps.size() == n && p.levels() == n && p.reordered == (which == 1) && p.launches.size() == 1 &&
                     p.steps.front().row == (which ? n - 1 : 0) && p.steps.back().row == (which ? 0 : n - 1);
            }
        check(ok, "blow-up: both chains plan, depth 2^18, one chain launch");
        printf("%s: chain of 2^18 rows: build_plan in order %.2f ms, build_plan_any_order reversed %.2f ms, ratio %.1f\n", name, best[0], best[1], best[1] / best[0]);
        check(best[1] <= 50.0 * best[0], "blow-up: the reversed chain costs at most 50 x the in-order plan");
    }

    int run() {
        corpus();
        waiting();
        refused();
        root_cause();
        blow_up();
        return report();
    }
};

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381");
    Suite<pm::BnCurve> bn("bn254");
    return (bls.run() | bn.run()) ? 1 : 0;
}
