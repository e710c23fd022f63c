// The witness solver's plan builder (polymath_amd/host/solve_plan.hpp) on is-zero pairs, on the CPU.  Accepted shapes against
// hand-written plans (step, both rows, entry positions, sides, sign, level, sort position, launch; two pairs open at once and
// closed in either order) and EXECUTED serially with the
// host field type the way the kernels do it (markers in the unknown columns, ONE inversion per pair, 0^-1 = 0); refused shapes with
// row, column and a message that begins with the message of the same system planned without the modulus; and equivalence: systems
// without pairs give the plan they gave, and without the modulus the builder is the earliest one.
// Built and run by tests/test_native_solve_iszero.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include "solve_selftest.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit Suite(const char *n) : Rig(n) {}

    static bool launch_is(const Launch &l, uint32_t lo, uint32_t hi, int chain, int divides, int bits, int iszero) {
        return l.lo == lo && l.hi == hi && (l.kind == LAUNCH_CHAIN) == (chain != 0) && l.divides == divides && (l.kind == LAUNCH_BITS) == (bits != 0) && (l.kind == LAUNCH_ISZERO) == (iszero != 0);
    }
    struct Pair { uint32_t row1, row, col_m, col_b; uint64_t pos_m, pos_c, pos; int m_in_b, b_in_b, negated; uint32_t level; };
    static bool pair_is(const Plan &p, uint32_t t, const Pair &w) {
        if (t >= p.steps.size()) return false;
        const Step &s = p.steps[t];
        if (s.kind != KIND_ISZERO || s.cols_off >= p.pairs.size()) return false;
        const PairRows &pr = p.pairs[s.cols_off];
        return pr.row1 == w.row1 && s.row == w.row && pr.col_m == w.col_m && s.col == w.col_b && pr.pos_m == w.pos_m && pr.pos_c == w.pos_c &&
               s.pos == w.pos && pr.m_in_b == w.m_in_b && pr.b_in_b == w.b_in_b && pr.negated == w.negated && s.level == w.level && s.bits == 0;
    }

    // ---- 1. accepted shapes
    // columns: 0 one | given 1 p, 2 q, 3 g | pair 1: flag 4, m 5 | pair 2: flag 6, m 7 | 8 y | pair 3: flag 9, m 10 | bits 11, 12 | 13 w
    //   row 0       booleanity of column 4 (ark: before the pair; a check row once the pair is solved)
    //   rows 1, 2   ark on p - q,             known sides A, A                               level 1
    //   row 3       circom's OPENER on 3 p - 2 q + 7: (-lc, reversed) * m7 = f6 - 1   --  the pair stays open over rows 4 .. 7
    //   row 4       y * 1 = p + q      an ordinary row that names neither column of it       kind A, level 1
    //   rows 5, 6   booleanity of 11, 12
    //   row 7       g * 1 = b11 + 2 b12                                                      a decomposition, level 1
    //   row 8       circom's CLOSER: f6 * (3 p - 2 q + 7) = 0, known side B, K2 = -K1 in another stored order
    //   rows 9, 10  a pair with known rests, cm, cb, kb random, on  y - b11:
    //               (cm m10) * (y - b11) = cb f9 + 5 q ;  (kb f9 + 3 p) * (b11 - y) = 4 g   level 2 (reads y and b11)
    //   row 11      w * 1 = f4 + f6 + f9                                                     an ordinary step at level 3
    void accepted() {
        System s;
        s.m0 = 1; s.mw = 13;
        const Fr one = F::one(), m1 = F::neg(one), cm = rnd(), cb = rnd(), kb = rnd();
        const Row pq = {{one, 1}, {m1, 2}}, lin = {{u(3), 1}, {F::neg(u(2)), 2}, {u(7), 0}};
        s.boolean(4);
        ark(s, pq, 4, 5);
        {
            Row minus;
            for (size_t i = lin.size(); i-- > 0;) minus.push_back({F::neg(lin[i].first), lin[i].second});
            s.add(minus, Row{{one, 7}}, Row{{one, 6}, {m1, 0}});
        }
        s.add(Row{{one, 8}}, Row{{one, 0}}, Row{{one, 1}, {one, 2}});
        s.boolean(11); s.boolean(12);
        s.add(Row{{one, 3}}, Row{{one, 0}}, Row{{one, 11}, {u(2), 12}});
        s.add(Row{{one, 6}}, lin, Row{});
        s.add(Row{{cm, 10}}, Row{{one, 8}, {m1, 11}}, Row{{u(5), 2}, {cb, 9}});
        s.add(Row{{u(3), 1}, {kb, 9}}, Row{{one, 11}, {m1, 8}}, Row{{u(4), 3}});
        check(s.add(Row{{one, 13}}, Row{{one, 0}}, Row{{one, 4}, {one, 6}, {one, 9}}) == 11, "accepted: row numbering");
        const std::vector<uint8_t> unknown = s.unknown({4, 5, 6, 7, 8, 9, 10, 11, 12, 13});
        const Plan p = in_order(s, unknown);
        check(p.error == OK && p.steps.size() == 6, "accepted: six steps for ten columns");
        const auto at = [&](int k, uint64_t r, uint64_t i) { return s.rowptr[k][r] + i; };
        // level 1: kind A (row 4), BITS_C (row 7), the pairs (closers at rows 2 and 8); level 2: the third pair; level 3: row 11
        check(p.steps.size() == 6 && p.steps[0].row == 4 && p.steps[0].kind == KIND_A && p.steps[0].level == 1, "accepted: the ordinary step sorts first in level 1");
        check(p.steps.size() == 6 && p.steps[1].row == 7 && p.steps[1].kind == KIND_BITS_C && p.steps[1].level == 1 && p.steps[1].bits == 2, "accepted: then the decomposition");
        check(pair_is(p, 2, Pair{1, 2, 5, 4, at(1, 1, 0), at(2, 1, 0), at(1, 2, 1), 1, 1, 0, 1}), "accepted: ark, known sides A / A, K2 = K1; its flag had a booleanity row");
        check(pair_is(p, 3, Pair{3, 8, 7, 6, at(1, 3, 0), at(2, 3, 0), at(0, 8, 0), 1, 0, 1, 1}), "accepted: circom, closer's known side B, K2 = -K1 in another order, closed after two rows");
        check(pair_is(p, 4, Pair{9, 10, 10, 9, at(0, 9, 0), at(2, 9, 1), at(0, 10, 1), 0, 0, 1, 2}), "accepted: known rests, opener's known side B, level 2");
        check(p.steps.size() == 6 && p.steps[5].row == 11 && p.steps[5].kind == KIND_A && p.steps[5].level == 3, "accepted: an ordinary step reads the flags at level 3");
        check(p.level_ptr == std::vector<uint32_t>({0, 4, 5, 6}), "accepted: level_ptr");
        check(p.launches.size() == 1 && launch_is(p.launches[0], 0, 6, 1, 1, 0, 0), "accepted: one dividing chain");
        const Plan wide = in_order(s, unknown, 1);
        bool ok = wide.steps.size() == 6 && wide.launches.size() == 5;
        for (size_t t = 0; ok && t < 6; ++t) ok = same_step(wide.steps[t], p.steps[t]);
        ok = ok && launch_is(wide.launches[0], 0, 1, 0, 1, 0, 0) && launch_is(wide.launches[1], 1, 2, 0, 0, 1, 0) && launch_is(wide.launches[2], 2, 4, 0, 1, 0, 1) &&
             launch_is(wide.launches[3], 4, 5, 0, 1, 0, 1) && launch_is(wide.launches[4], 5, 6, 0, 1, 0, 0);
        check(ok, "accepted: in a wide level the pairs get a dividing launch of their own, after the decompositions");
        const Plan three = in_order(s, unknown, 3);   // level 1 is wide (4 steps), levels 2 and 3 are one chain that holds a pair
        check(three.launches.size() == 4 && launch_is(three.launches[3], 4, 6, 1, 1, 0, 0), "accepted: a narrow level with a pair makes its chain a dividing one");

        // execution.  Round bit 0: p - q = 0; bit 1: 3 p - 2 q + 7 = 0; round 4, 5: y - b11 = 0 (alone, and with p = q)
        check(F::inv(F::zero()).is_zero(), "accepted: the Fermat inverse of 0 is 0");
        for (int round = 0; round < 6; ++round) {
            const uint64_t bit11 = round & 1, bit12 = (round >> 1) & 1;
            const Fr b11 = u(bit11), g = u(bit11 + 2 * bit12), half = F::inv(u(2));
            Fr pv = rnd(), qv = rnd();
            if (round == 1) qv = pv;
            if (round == 2) qv = F::mul(F::add(F::mul(u(3), pv), u(7)), half);
            if (round == 3) pv = qv = F::neg(u(7));
            if (round == 4) qv = F::sub(b11, pv);
            if (round == 5) pv = qv = F::mul(b11, half);
            const Fr d1 = F::sub(pv, qv), d2 = F::add(F::sub(F::mul(u(3), pv), F::mul(u(2), qv)), u(7)), d3 = F::sub(F::add(pv, qv), b11);
            check(d1.is_zero() == (round == 1 || round == 3 || round == 5) && d2.is_zero() == (round == 2 || round == 3) && d3.is_zero() == (round >= 4), "accepted: the round's zeros");
            std::vector<Fr> want(14, F::zero());
            want[0] = one; want[1] = pv; want[2] = qv; want[3] = g;
            want[4] = d1.is_zero() ? F::zero() : one;     want[5] = F::inv(d1);              // ark: the flag is [d != 0]
            want[6] = d2.is_zero() ? one : F::zero();     want[7] = F::inv(d2);              // circom: [d == 0], and (-d) m = out - 1 = -1
            want[8] = F::add(pv, qv); want[11] = b11; want[12] = u(bit12);
            if (d3.is_zero()) {
                want[9] = F::mul(F::neg(F::mul(u(5), qv)), F::inv(cb));
                want[10] = F::zero();
            } else {   // closer: (kb f9 + 3 p) (-d3) = 4 g;  opener: (cm m10) d3 = cb f9 + 5 q
                want[9] = F::mul(F::sub(F::mul(F::mul(u(4), g), F::inv(F::neg(d3))), F::mul(u(3), pv)), F::inv(kb));
                want[10] = F::mul(F::mul(F::add(F::mul(cb, want[9]), F::mul(u(5), qv)), F::inv(d3)), F::inv(cm));
            }
            want[13] = F::add(F::add(want[4], want[6]), want[9]);
            for (const Plan *q : {&p, &wide}) {
                std::vector<Fr> z(14, marker());
                for (uint32_t j = 0; j <= 3; ++j) z[j] = want[j];
                ok = execute(s, *q, z) == NONE;
                for (size_t j = 0; ok && j < z.size(); ++j) ok = z[j].eq(want[j]);
                check(ok, "accepted: executed == the formulas");
                // every row holds, except that with d3 = 0 the third closer reads 0 = 4 g: an ordinary failing row unless g = 0
                for (uint64_t r = 0; ok && r < s.nr(); ++r)
                    ok = (r == 10 && d3.is_zero() && !g.is_zero()) ||
                         F::mul(dot(s, 0, z, r), dot(s, 1, z, r)).eq(dot(s, 2, z, r));
                check(ok, "accepted: the rows hold");
            }
        }
    }

    // ---- 1b. two openers pending before either closes, closed in the order they opened and in the other order
    // columns: 0 one | given 1 a, 2 b, 3 c | pair X: flag 4, m 5 | pair Y: flag 6, m 7 | 8 y | 9 w
    //   row 0   ark's opener X:     (a - b) * m5 = f4
    //   row 1   circom's opener Y:  (c - a) * m7 = f6 - 1                 both pairs are pending from here ...
    //   row 2   y * 1 = a + b                                             ... over an ordinary row that names neither
    //   rows 3, 4   the closers  (a - b) * (1 - f4) = 0  and  (a - c) * f6 = 0,  Y's first (order 0) or X's first (order 1)
    //   row 5   w * 1 = f4 + f6                                           reads both flags: level 2
    void interleaved() {
        const Fr one = F::one(), m1 = F::neg(one);
        for (uint32_t order = 0; order < 2; ++order) {
            System s;
            s.m0 = 1; s.mw = 9;
            const Row ab = {{one, 1}, {m1, 2}}, ac = {{one, 1}, {m1, 3}}, ca = {{one, 3}, {m1, 1}};
            s.add(ab, Row{{one, 5}}, Row{{one, 4}});
            s.add(ca, Row{{one, 7}}, Row{{one, 6}, {m1, 0}});
            s.add(Row{{one, 8}}, Row{{one, 0}}, Row{{one, 1}, {one, 2}});
            const uint32_t close_x = order ? 3 : 4, close_y = order ? 4 : 3;
            for (uint32_t r = 3; r < 5; ++r) r == close_x ? s.add(ab, Row{{one, 0}, {m1, 4}}, Row{}) : s.add(ac, Row{{one, 6}}, Row{});
            s.add(Row{{one, 9}}, Row{{one, 0}}, Row{{one, 4}, {one, 6}});
            const std::vector<uint8_t> unknown = s.unknown({4, 5, 6, 7, 8, 9});
            const Plan p = in_order(s, unknown);
            check(p.error == OK && p.steps.size() == 4 && p.steps[0].row == 2 && p.steps[0].kind == KIND_A && p.steps[0].level == 1 && p.steps[3].row == 5 &&
                      p.steps[3].kind == KIND_A && p.steps[3].level == 2,
                  "interleaved: four steps, the ordinary ones first in level 1 and alone in level 2");
            // the pairs sort by their closers' rows; each keeps its own opener, columns and entry positions
            const Pair x = {0, close_x, 5, 4, s.rowptr[1][0], s.rowptr[2][0], s.rowptr[1][close_x] + 1, 1, 1, 0, 1};
            const Pair y = {1, close_y, 7, 6, s.rowptr[1][1], s.rowptr[2][1], s.rowptr[1][close_y], 1, 1, 1, 1};
            check(pair_is(p, order ? 1 : 2, x), "interleaved: the pair that opened first");
            check(pair_is(p, order ? 2 : 1, y), "interleaved: the pair that opened second");
            check(p.level_ptr == std::vector<uint32_t>({0, 3, 4}) && p.launches.size() == 1 && launch_is(p.launches[0], 0, 4, 1, 1, 0, 0), "interleaved: level_ptr, one dividing chain");
            const Plan wide = in_order(s, unknown, 1);
            bool ok = wide.steps.size() == 4 && wide.launches.size() == 3;
            for (size_t t = 0; ok && t < 4; ++t) ok = same_step(wide.steps[t], p.steps[t]);
            check(ok && launch_is(wide.launches[0], 0, 1, 0, 1, 0, 0) && launch_is(wide.launches[1], 1, 3, 0, 1, 0, 1) && launch_is(wide.launches[2], 3, 4, 0, 1, 0, 0),
                  "interleaved: both pairs in one launch of a wide level");
            for (int round = 0; round < 4; ++round) {
                const Fr a = rnd(), b = round & 1 ? a : rnd(), c = round & 2 ? a : rnd();
                const bool eq_b = (round & 1) != 0, eq_c = (round & 2) != 0;
                const Fr f4 = eq_b ? F::zero() : one, f6 = eq_c ? one : F::zero();
                const std::vector<Fr> want = {one, a, b, c, f4, F::inv(F::sub(a, b)), f6, F::inv(F::sub(a, c)), F::add(a, b), F::add(f4, f6)};
                std::vector<Fr> z(10, marker());
                for (uint32_t j = 0; j <= 3; ++j) z[j] = want[j];
                ok = execute(s, round & 1 ? wide : p, z) == NONE && rows_hold(s, z);
                for (size_t j = 0; ok && j < z.size(); ++j) ok = z[j].eq(want[j]);
                check(ok, "interleaved: executed, each pair with its own rows");
            }
        }
    }

    // ---- 2. every placement of the known sides, both forms, d != 0 and d = 0: values by the formulas, both rows hold
    void placements() {
        const Fr one = F::one();
        for (int form = 0; form < 2; ++form)
            for (int swap1 = 0; swap1 < 2; ++swap1)
                for (int swap2 = 0; swap2 < 2; ++swap2) {
                    System s;
                    s.m0 = 1; s.mw = 4;   // 1 a, 2 b given | 3 flag, 4 m
                    const Row lc = {{one, 1}, {F::neg(one), 2}};
                    form ? circom(s, lc, 3, 4, swap1, swap2) : ark(s, lc, 3, 4, swap1, swap2);
                    const Plan p = in_order(s, s.unknown({3, 4}));
                    const uint64_t b_pos = form ? 0 : 1;    // ark's closer side is (1, one), (-1, flag): the flag is its second entry
                    check(p.error == OK && p.steps.size() == 1 &&
                              pair_is(p, 0, Pair{0, 1, 4, 3, s.rowptr[swap1 ? 0 : 1][0], s.rowptr[2][0], s.rowptr[swap2 ? 0 : 1][1] + b_pos, !swap1, !swap2, form, 1}) &&
                              p.launches.size() == 1 && launch_is(p.launches[0], 0, 1, 1, 1, 0, 0),
                          "placements: the plan");
                    for (int equal = 0; equal < 2; ++equal) {
                        const Fr a = rnd(), b = equal ? a : rnd();
                        std::vector<Fr> z = {one, a, b, marker(), marker()};
                        bool ok = execute(s, p, z) == NONE && rows_hold(s, z);
                        const Fr truth = (equal != 0) == (form != 0) ? one : F::zero();   // ark's flag is [d != 0], circom's [d == 0]
                        ok = ok && z[3].eq(truth) && z[4].eq(equal ? F::zero() : F::inv(F::sub(a, b)));     // (-d) m = out - 1 = -1: m = 1 / d in both forms
                        check(ok, "placements: executed, d != 0 and d = 0");
                    }
                    // the caller gives m (arkworks writes 1 where d = 0): only the flag is marked, the opener is an ordinary kind-C step
                    const Plan given = in_order(s, s.unknown({3}));
                    check(given.error == OK && given.steps.size() == 1 && given.steps[0].kind == KIND_C && given.steps[0].row == 0 && given.steps[0].col == 3 &&
                              given.launches.size() == 1 && launch_is(given.launches[0], 0, 1, 1, 0, 0, 0),
                          "placements: m given, the flag is a kind-C step of the opener");
                    const Fr a = rnd();
                    std::vector<Fr> z = {one, a, a, marker(), one};
                    check(execute(s, given, z) == NONE && rows_hold(s, z) && z[3].eq(form ? one : F::zero()) && z[4].eq(one), "placements: m = 1 given where d = 0");
                }
    }

    // ---- 3. refused shapes: ERR_MANY_UNKNOWNS at r1, the column and the message prefix of the plan without the modulus
    void refused() {
        const Fr one = F::one(), m1 = F::neg(one);
        const Row lc = {{one, 1}, {m1, 2}};
        struct Case { const char *what; Row a, b, c; const char *needle; bool no_closer; };
        // columns 1, 2 given | 3 flag, 4 m | 5 another unknown.  Row 0: a check row.  Row 1: the opener lc * m = flag.  Row 2: the case.
        const std::vector<Case> cases = {
            {"refused: an opener that is never closed", Row{{one, 1}}, Row{{one, 2}}, Row{{one, 1}}, "no later row closes it", true},
            {"refused: the next row names m", Row{{one, 4}}, Row{{one, 1}}, Row{{one, 2}}, "row 2 names the multiplier (column 4)", false},
            {"refused: the next row names m beside the flag", lc, Row{{one, 3}, {one, 4}}, Row{}, "row 2 names the multiplier (column 4)", false},
            {"refused: the next row names the flag in C", lc, Row{{one, 0}}, Row{{one, 3}}, "row 2 names the flag (column 3) in C", false},
            {"refused: the next row names the flag on both sides", Row{{one, 3}}, Row{{one, 0}, {m1, 3}}, Row{}, "row 2 names the flag (column 3) in A and in B", false},
            {"refused: the next row names the flag twice on one side", lc, Row{{one, 0}, {m1, 3}, {one, 3}}, Row{}, "row 2 names the flag (column 3) twice in B", false},
            {"refused: K2 differs in one coefficient", Row{{one, 1}, {F::neg(u(2)), 2}}, Row{{one, 0}, {m1, 3}}, Row{}, "known side", false},
            {"refused: K2 has an extra entry", Row{{one, 1}, {m1, 2}, {one, 0}}, Row{{one, 0}, {m1, 3}}, Row{}, "known side", false},
            {"refused: K2 is minus K1 in one entry only", Row{{m1, 1}, {m1, 2}}, Row{{one, 0}, {m1, 3}}, Row{}, "known side", false},
            {"refused: a second unknown in the closer", lc, Row{{one, 0}, {m1, 3}}, Row{{one, 5}}, "row 2 has a second unknown (column 5)", false},
        };
        for (const Case &c : cases) {
            System s; s.m0 = 1; s.mw = 5;
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(lc, Row{{one, 4}}, Row{{one, 3}});
            s.add(c.a, c.b, c.c);
            s.add(Row{{one, 5}}, Row{{one, 0}}, Row{{one, 1}});       // column 5 would be solved here
            const std::vector<uint8_t> unknown = s.unknown({3, 4, 5});
            const Plan p = in_order(s, unknown), parent = in_order(s, unknown, WIDE_STEPS, false);
            check(parent.error == ERR_MANY_UNKNOWNS && parent.error_row == 1 && parent.error_col == 3 && parent.message == "row 1: two or more unknowns (columns 4 and 3)",
                  "refused: the plan without the modulus");
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.error_col == 3 && p.message.find(parent.message) == 0 && p.message.size() > parent.message.size() &&
                      p.message.find(c.needle) != std::string::npos && p.steps.empty() && p.launches.empty(),
                  c.what);
        }
        {   // K1 all-zero (a stored zero coefficient names nothing) and the two unknowns on the A / B sides: no opener, refused at once as before
            for (int shape = 0; shape < 2; ++shape) {
                System s; s.m0 = 1; s.mw = 4;
                if (shape == 0) s.add(Row{{F::zero(), 1}}, Row{{one, 4}}, Row{{one, 3}});
                else s.add(Row{{one, 4}}, Row{{one, 3}}, Row{{one, 1}});
                s.add(lc, Row{{one, 0}, {m1, 3}}, Row{});
                const std::vector<uint8_t> unknown = s.unknown({3, 4});
                const Plan p = in_order(s, unknown), parent = in_order(s, unknown, WIDE_STEPS, false);
                check(parent.error == ERR_MANY_UNKNOWNS && parent.error_row == 0 && p.error == ERR_MANY_UNKNOWNS && p.error_row == 0 && p.error_col == parent.error_col &&
                          p.message.find(parent.message) == 0 && p.message.find("is-zero") == std::string::npos,
                      shape ? "refused: both unknowns on the A / B sides, at once" : "refused: K1 all-zero, at once");
            }
        }
        {   // an unknown side of the opener with a known rest, and a multiplier that C names as well
            for (int shape = 0; shape < 2; ++shape) {
                System s; s.m0 = 1; s.mw = 4;
                if (shape == 0) s.add(lc, Row{{one, 4}, {one, 1}}, Row{{one, 3}});
                else s.add(lc, Row{{one, 4}}, Row{{one, 3}, {one, 4}});
                s.add(lc, Row{{one, 0}, {m1, 3}}, Row{});
                const Plan p = in_order(s, s.unknown({3, 4}));
                check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 0, shape ? "refused: the multiplier in C as well" : "refused: a known rest beside the multiplier");
            }
        }
        {   // two openers pending at the end: the smaller r1 is reported, before a boolean-pending and an undetermined column
            System s; s.m0 = 1; s.mw = 8;
            s.boolean(7);
            s.add(lc, Row{{one, 4}}, Row{{one, 3}});
            s.add(lc, Row{{one, 6}}, Row{{one, 5}});
            const std::vector<uint8_t> unknown = s.unknown({3, 4, 5, 6, 7, 8});
            const Plan p = in_order(s, unknown);
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.error_col == 3 && p.message.find("row 1: two or more unknowns (columns 4 and 3)") == 0 &&
                      p.message.find("no later row closes it") != std::string::npos,
                  "refused: openers pending at the end, smallest r1 first, before boolean-pending and undetermined columns");
        }
    }

    // ---- 4. systems without pairs plan as before; without the modulus the builder is the earliest one
    void equivalence() {
        const Fr one = F::one();
        {   // a pair, planned without the modulus: the earliest error
            System s; s.m0 = 1; s.mw = 4;
            ark(s, Row{{one, 1}, {F::neg(one), 2}}, 3, 4);
            const Plan p = in_order(s, s.unknown({3, 4}), WIDE_STEPS, false);
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 0 && p.error_col == 3 && p.message == "row 0: two or more unknowns (columns 4 and 3)", "equivalence: a pair without the modulus");
        }
        {   // kinds A, B, C and a decomposition: 0 one, 1 a, 2 c, 3 inv, 4 q, 5 s, 6 t, 7 8 bits
            System s; s.m0 = 1; s.mw = 8;
            s.add(Row{{u(3), 3}}, Row{{one, 1}}, Row{{one, 0}});
            s.add(Row{{one, 1}}, Row{{u(5), 4}}, Row{{one, 2}});
            s.add(Row{{one, 3}}, Row{{one, 4}}, Row{{one, 5}});
            s.add(Row{{one, 5}, {one, 0}}, Row{{u(2), 6}}, Row{{one, 3}});
            s.boolean(7); s.boolean(8);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 7}, {u(2), 8}});
            const std::vector<uint8_t> unknown = s.unknown({3, 4, 5, 6, 7, 8});
            for (uint32_t wide : {WIDE_STEPS, 1u}) {
                const Plan p = in_order(s, unknown, wide);
                bool ok = p.error == OK && p.steps.size() == 5 && p.launches.size() == (wide == 1 ? 4u : 1u) && p.pairs.empty();
                for (const Step &st : p.steps) ok = ok && st.kind != KIND_ISZERO;
                for (const Launch &l : p.launches) ok = ok && l.kind != LAUNCH_ISZERO;
                // level 1: row 0 (A), row 1 (B), row 6 (BITS_C) -- sorted A, B, BITS_C; level 2: row 2 (C); level 3: row 3 (B)
                ok = ok && p.steps[0].row == 0 && p.steps[1].row == 1 && p.steps[2].row == 6 && p.steps[3].row == 2 && p.steps[4].row == 3 &&
                     p.level_ptr == std::vector<uint32_t>({0, 3, 4, 5});
                if (wide == 1) ok = ok && launch_is(p.launches[0], 0, 2, 0, 1, 0, 0) && launch_is(p.launches[1], 2, 3, 0, 0, 1, 0) && launch_is(p.launches[2], 3, 4, 0, 0, 0, 0) &&
                                    launch_is(p.launches[3], 4, 5, 0, 1, 0, 0);
                else ok = ok && launch_is(p.launches[0], 0, 5, 1, 1, 0, 0);
                check(ok, "equivalence: a plan without pairs has the steps, level_ptr and launches it had");
            }
            const std::vector<uint8_t> ordinary = s.unknown({3, 4, 5, 6});
            for (uint32_t wide : {WIDE_STEPS, 1u}) check(same_plan(in_order(s, ordinary, wide), in_order(s, ordinary, wide, false)), "equivalence: with and without the modulus");
        }
        check(KIND_ISZERO == 6 && NUM_KINDS == 7 && KIND_C == 0 && KIND_A == 1 && KIND_B == 2 && KIND_BITS_C == 3 && KIND_BITS_A == 4 && KIND_BITS_B == 5, "equivalence: the enumerators");
    }

    int run() {
        accepted();
        interleaved();
        placements();
        refused();
        equivalence();
        return report();
    }
};

int main() {
    rng_state = 0x13198A2E03707344ull;
    Suite<pm::BlsCurve> bls("bls12_381");
    Suite<pm::BnCurve> bn("bn254");
    return (bls.run() | bn.run()) ? 1 : 0;
}
