// The witness solver's plan builder (polymath_amd/host/solve_plan.hpp) WITH the field's modulus, on the CPU: booleanity rows and bit
// decompositions.  Accepted structures against hand-written plans (step, columns in exponent order, level, launch) and EXECUTED
// serially with the host field type the way the kernels do it (markers in the unknown columns, passed over by the decomposition's
// dot product); refused structures with their row or column; and equivalence with the plan built without the modulus.
// Built and run by tests/test_native_solve_bits.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include "solve_selftest.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    uint32_t r_bits;              // bitlength(r)

    Suite(const char *n, uint32_t bits) : Rig(n), r_bits(bits) {}
    static Fr minus(const Fr &a) { return F::neg(a); }
    static Fr shl(Fr c, uint32_t i) {          // c 2^i by doublings: the words the plan's own chain walks
        while (i--) c = F::add(c, c);
        return c;
    }
    static bool launch_is(const Launch &l, uint32_t lo, uint32_t hi, int chain, int divides, int bits) {
        return l.lo == lo && l.hi == hi && (l.kind == LAUNCH_CHAIN) == (chain != 0) && l.divides == divides && (l.kind == LAUNCH_BITS) == (bits != 0);
    }
    bool step_is(const Plan &p, uint32_t t, uint32_t row, uint32_t col, uint32_t kind, uint32_t level, uint64_t pos, const std::vector<uint32_t> &cols) {
        if (t >= p.steps.size()) return false;
        const Step &s = p.steps[t];
        bool ok = s.row == row && s.col == col && s.kind == kind && s.level == level && s.pos == pos && s.bits == cols.size();
        for (size_t i = 0; ok && i < cols.size(); ++i) ok = s.cols_off + i < p.bit_cols.size() && p.bit_cols[s.cols_off + i] == cols[i];
        return ok;
    }

    // ---- 1. every accepted shape in one system
    // columns: 0 one | given: 1 v, 2 w, 3 g1, 4 g2 | a0..a3 = 5..8 | b0..b2 = 9..11 | d0..d2 = 12..14 | 15 e | f0..f2 = 16..18 | 19 y
    // rows 0..13 booleanity of a, b, d, e, f (different k, k', both orientations), then
    //   14: v * 1 = a0 + 2 a1 + 4 a2 + 8 a3 + 5                       kind C, c = 1, a known entry beside the bits
    //   15: (4c b2 + 7 w + c b0 + 2c b1) * w = g1                     kind A, c random, permuted, Bz = w
    //   16: w * (3 d0 + 6 d1 + 12 d2) = g2                            kind B, c = 3
    //   17: e * 1 = a0                                                e is boolean-pending and an ORDINARY row solves it (level 2)
    //   18: (a1 + b0) * (d2 + 1) = y                                  level 2
    //   19: y * 1 = 2 f1 + f0 + 4 f2                                  a decomposition at level 3
    void accepted() {
        System s;
        s.m0 = 1; s.mw = 19;
        const Fr one = F::one(), c = rnd();
        const uint32_t V = 1, W = 2, G1 = 3, G2 = 4, A0 = 5, B0 = 9, D0 = 12, E = 15, F0 = 16, Y = 19;
        for (uint32_t i = 0; i < 4; ++i) s.boolean(A0 + i);
        for (uint32_t i = 0; i < 3; ++i) s.boolean(B0 + i, rnd(), rnd(), true);
        for (uint32_t i = 0; i < 3; ++i) s.boolean(D0 + i, u(2), rnd());
        s.boolean(E);
        for (uint32_t i = 0; i < 3; ++i) s.boolean(F0 + i, one, one, i == 1);
        check(s.add(Row{{one, V}}, Row{{one, 0}}, Row{{one, A0}, {u(2), A0 + 1}, {u(5), 0}, {u(4), A0 + 2}, {u(8), A0 + 3}}) == 14, "accepted: row numbering");
        s.add(Row{{shl(c, 2), B0 + 2}, {u(7), W}, {c, B0}, {shl(c, 1), B0 + 1}}, Row{{one, W}}, Row{{one, G1}});
        s.add(Row{{one, W}}, Row{{u(3), D0}, {u(6), D0 + 1}, {u(12), D0 + 2}}, Row{{one, G2}});
        s.add(Row{{one, E}}, Row{{one, 0}}, Row{{one, A0}});
        s.add(Row{{one, A0 + 1}, {one, B0}}, Row{{one, D0 + 2}, {one, 0}}, Row{{one, Y}});
        s.add(Row{{one, Y}}, Row{{one, 0}}, Row{{u(2), F0 + 1}, {one, F0}, {u(4), F0 + 2}});
        std::vector<uint32_t> un;
        for (uint32_t j = A0; j <= Y; ++j) un.push_back(j);
        const std::vector<uint8_t> unknown = s.unknown(un);
        const Plan p = in_order(s, unknown);
        check(p.error == OK && p.steps.size() == 6 && p.bit_cols.size() == 13, "accepted: six steps for fifteen columns");
        // entry positions: row 14's C entries start at 0 (no earlier row has any), row 15's A entries after 14 booleanity rows' and rows 14's
        const uint64_t a15 = s.rowptr[0][15], b16 = s.rowptr[1][16], c19 = s.rowptr[2][19];
        check(step_is(p, 0, 14, A0, KIND_BITS_C, 1, 0, {A0, A0 + 1, A0 + 2, A0 + 3}), "accepted: kind C, a known entry between the bits");
        check(step_is(p, 1, 15, B0, KIND_BITS_A, 1, a15 + 2, {B0, B0 + 1, B0 + 2}), "accepted: kind A, c random, permuted: pos names c's entry, columns in exponent order");
        check(step_is(p, 2, 16, D0, KIND_BITS_B, 1, b16, {D0, D0 + 1, D0 + 2}), "accepted: kind B, c = 3");
        check(step_is(p, 3, 18, Y, KIND_C, 2, s.rowptr[2][18], {}), "accepted: an ordinary step reads the bits at level 2");
        check(step_is(p, 4, 17, E, KIND_A, 2, s.rowptr[0][17], {}), "accepted: a boolean-pending column solved by an ordinary row");
        check(step_is(p, 5, 19, F0, KIND_BITS_C, 3, c19 + 1, {F0, F0 + 1, F0 + 2}), "accepted: a decomposition at level 3");
        check(p.level_ptr == std::vector<uint32_t>({0, 3, 5, 6}), "accepted: level_ptr");
        check(p.launches.size() == 1 && launch_is(p.launches[0], 0, 6, 1, 1, 0), "accepted: one dividing chain");
        const Plan wide = in_order(s, unknown, 1);
        bool ok = wide.launches.size() == 5 && wide.steps.size() == 6;
        for (size_t t = 0; ok && t < 6; ++t) ok = same_step(wide.steps[t], p.steps[t]);
        ok = ok && launch_is(wide.launches[0], 0, 1, 0, 0, 1) && launch_is(wide.launches[1], 1, 3, 0, 1, 1) && launch_is(wide.launches[2], 3, 4, 0, 0, 0) &&
             launch_is(wide.launches[3], 4, 5, 0, 1, 0) && launch_is(wide.launches[4], 5, 6, 0, 0, 1);
        check(ok, "accepted: wide levels launch their decompositions apart, split where the dividing kinds begin");
        const Plan two = in_order(s, unknown, 2);     // level 3 (one step) joins no earlier chain: levels 1 and 2 are wide
        check(two.launches.size() == 5 && launch_is(two.launches[4], 5, 6, 1, 0, 0), "accepted: a narrow level of one decomposition is a chain without division");

        // execution: bits chosen, the given values computed from them
        for (int round = 0; round < 4; ++round) {
            const uint32_t ta = round == 0 ? 15 : (uint32_t)(next_u64() % 16), tb = round == 0 ? 7 : (uint32_t)(next_u64() % 8), td = (uint32_t)(next_u64() % 8);
            const Fr w = rnd();
            std::vector<Fr> want(20, F::zero());
            want[0] = one;
            want[V] = u(ta + 5); want[W] = w;
            want[G1] = F::mul(F::add(F::mul(c, u(tb)), F::mul(u(7), w)), w);
            want[G2] = F::mul(w, u(3 * td));
            for (uint32_t i = 0; i < 4; ++i) want[A0 + i] = u((ta >> i) & 1);
            for (uint32_t i = 0; i < 3; ++i) { want[B0 + i] = u((tb >> i) & 1); want[D0 + i] = u((td >> i) & 1); }
            want[E] = want[A0];
            const uint32_t y = (((ta >> 1) & 1) + (tb & 1)) * (((td >> 2) & 1) + 1);
            want[Y] = u(y);
            for (uint32_t i = 0; i < 3; ++i) want[F0 + i] = u((y >> i) & 1);
            for (const Plan *q : {&p, &wide}) {
                std::vector<Fr> z(20, marker());
                for (uint32_t j = 0; j <= G2; ++j) z[j] = want[j];
                ok = execute(s, *q, z) == NONE;
                for (size_t j = 0; ok && j < z.size(); ++j) ok = z[j].eq(want[j]);
                check(ok, "accepted: executed == the bits the values were made from");
            }
            if (round) continue;
            // v = 16 + 5 has no 4-bit form: stuck at row 14, zeros in a0..a3, everything else as before except what reads them
            std::vector<Fr> z(20, marker());
            for (uint32_t j = 0; j <= G2; ++j) z[j] = want[j];
            z[V] = u(21);
            ok = execute(s, p, z) == 14;
            for (uint32_t i = 0; i < 4; ++i) ok = ok && z[A0 + i].is_zero();
            for (uint32_t i = 0; i < 3; ++i) ok = ok && z[B0 + i].eq(want[B0 + i]) && z[D0 + i].eq(want[D0 + i]);
            check(ok, "accepted: T >= 2^k is stuck at the decomposition row, its columns zero, its neighbours complete");
            z.assign(20, marker());
            for (uint32_t j = 0; j <= G2; ++j) z[j] = want[j];
            z[V] = F::add(u(3), minus(one));          // v - 5 = -3: a canonical integer far above 2^4
            check(execute(s, p, z) == 14, "accepted: a negative value is stuck too");
            z.assign(20, marker());
            for (uint32_t j = 0; j <= G2; ++j) z[j] = want[j];
            z[W] = F::zero();                          // rows 15 and 16 divide by w
            ok = execute(s, p, z) == 15;
            for (uint32_t i = 0; i < 3; ++i) ok = ok && z[B0 + i].is_zero() && z[D0 + i].is_zero();
            for (uint32_t i = 0; i < 4; ++i) ok = ok && z[A0 + i].eq(want[A0 + i]);
            check(ok, "accepted: a zero divisor is stuck at the smaller of its two rows");
        }
    }

    // ---- 2. the widest decomposition: k = bitlength(r) - 1 accepted and executed, k = bitlength(r) refused
    void widest() {
        for (uint32_t k : {r_bits - 1, r_bits}) {
            System s;
            s.m0 = 1; s.mw = 1 + k;                    // 1 v | bits 2 .. 2 + k
            std::vector<uint32_t> un;
            Row bits;
            for (uint32_t i = 0; i < k; ++i) { s.boolean(2 + i); un.push_back(2 + i); }
            for (uint32_t i = 0; i < k; ++i) bits.push_back({shl(F::one(), i), 2 + i});
            for (uint32_t i = 0; i + 1 < k; i += 2) std::swap(bits[i], bits[i + 1]);      // stored out of order
            s.add(Row{{F::one(), 1}}, Row{{F::one(), 0}}, bits);
            const std::vector<uint8_t> unknown = s.unknown(un);
            const Plan p = in_order(s, unknown);
            if (k == r_bits) {
                check(p.error == ERR_MANY_UNKNOWNS && p.error_row == k && p.message.find("row " + std::to_string(k)) != std::string::npos &&
                          p.message.find("bitlength") != std::string::npos, "widest: k = bitlength(r) is refused at the decomposition row");
                continue;
            }
            bool ok = p.error == OK && p.steps.size() == 1 && p.steps[0].bits == k && p.steps[0].col == 2 && p.steps[0].kind == KIND_BITS_C && p.steps[0].level == 1 &&
                      p.steps[0].pos == 1 && p.bit_cols.size() == k;
            for (uint32_t i = 0; ok && i < k; ++i) ok = p.bit_cols[i] == 2 + i;
            check(ok, "widest: k = bitlength(r) - 1 is one step, columns in exponent order");
            for (int all_ones = 0; all_ones < 2 && ok; ++all_ones) {
                std::vector<uint8_t> bit(k);
                Fr v = F::zero();
                for (uint32_t i = k; i-- > 0;) {
                    bit[i] = all_ones ? 1 : (uint8_t)(next_u64() & 1);
                    v = F::add(F::add(v, v), bit[i] ? F::one() : F::zero());
                }
                std::vector<Fr> z(2 + k, marker());
                z[0] = F::one(); z[1] = v;
                ok = execute(s, p, z) == NONE;
                for (uint32_t i = 0; ok && i < k; ++i) ok = z[2 + i].eq(bit[i] ? F::one() : F::zero());
                check(ok, all_ones ? "widest: T = 2^k - 1 executed" : "widest: a random T executed");
            }
        }
    }

    // ---- 3. refused structures name their row or column
    void refused() {
        const Fr one = F::one();
        {   // booleanity after the decomposition: the decomposition row is refused
            System s; s.m0 = 1; s.mw = 3;
            s.boolean(2);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}});
            s.boolean(3);
            const Plan p = in_order(s, s.unknown({2, 3}));
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.error_col == 3 && p.message.find("row 1") != std::string::npos &&
                      p.message.find("boolean") != std::string::npos, "refused: booleanity after the decomposition");
        }
        struct Case { const char *what; uint64_t coef[3]; const char *needle; };
        for (const Case &c : {Case{"refused: a gap (1, 2, 8)", {1, 2, 8}, "2^0"}, Case{"refused: a repeated coefficient (1, 2, 2)", {1, 2, 2}, "twice"},
                              Case{"refused: no 2^0 term twice over (3, 6, 5)", {3, 6, 5}, "2^0"}}) {
            System s; s.m0 = 1; s.mw = 4;
            for (uint32_t j = 2; j < 5; ++j) s.boolean(j);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{u(c.coef[0]), 2}, {u(c.coef[1]), 3}, {u(c.coef[2]), 4}});
            const Plan p = in_order(s, s.unknown({2, 3, 4}));
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 3 && p.message.find("row 3") != std::string::npos && p.message.find(c.needle) != std::string::npos, c.what);
        }
        {   // one unknown of the row is not boolean-pending (column 4 has no booleanity row)
            System s; s.m0 = 1; s.mw = 4;
            s.boolean(2); s.boolean(3);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}, {u(4), 4}});
            const Plan p = in_order(s, s.unknown({2, 3, 4}));
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 2 && p.message.find("boolean") != std::string::npos, "refused: an unknown that is not boolean-pending");
        }
        {   // a bit is also in another matrix of the decomposition row
            System s; s.m0 = 1; s.mw = 3;
            s.boolean(2); s.boolean(3);
            s.add(Row{{one, 1}}, Row{{one, 0}, {one, 3}}, Row{{one, 2}, {u(2), 3}});
            const Plan p = in_order(s, s.unknown({2, 3}));
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 2 && p.message.find("more than one matrix") != std::string::npos, "refused: a bit also present in another matrix");
            System t; t.m0 = 1; t.mw = 3;          // the same with the doubled bit first in scan order
            t.boolean(2); t.boolean(3);
            t.add(Row{{one, 2}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}});
            const Plan q = in_order(t, t.unknown({2, 3}));
            check(q.error == ERR_MANY_UNKNOWNS && q.error_row == 2 && q.error_col == 3, "refused: a bit also present in another matrix, named first");
        }
        {   // bits spread over two matrices
            System s; s.m0 = 1; s.mw = 3;
            s.boolean(2); s.boolean(3);
            s.add(Row{{one, 2}}, Row{{u(2), 3}}, Row{{one, 1}});
            const Plan p = in_order(s, s.unknown({2, 3}));
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 2, "refused: bits in two matrices");
        }
        {   // a boolean column nothing determines: ERR_TWO_MATRICES at its booleanity row, before ERR_UNDETERMINED of column 1
            System s; s.m0 = 1; s.mw = 4;
            s.add(Row{{one, 2}}, Row{{one, 0}}, Row{{one, 2}});
            s.boolean(4);
            s.boolean(3);
            s.boolean(4);
            const Plan p = in_order(s, s.unknown({1, 3, 4}));
            check(p.error == ERR_TWO_MATRICES && p.error_row == 1 && p.error_col == 4 && p.message.find("row 1") != std::string::npos && p.steps.empty(),
                  "refused: a never-determined boolean column names its smallest booleanity row");
            const Plan parent = in_order(s, s.unknown({1, 3, 4}), WIDE_STEPS, false);
            check(parent.error == ERR_TWO_MATRICES && parent.error_row == 1 && parent.error_col == 4, "refused: ... which is what the plan without the modulus reports");
        }
        // one unknown in two matrices in any other shape: ERR_TWO_MATRICES at once
        const Fr k = rnd();
        struct Shape { const char *what; Row a, b, c; };
        for (const Shape &sh : {Shape{"refused: u * u", Row{{one, 1}}, Row{{one, 1}}, Row{}},
                                Shape{"refused: a constant other than minus the coefficient", Row{{one, 1}}, Row{{k, 0}, {F::neg(F::add(k, one)), 1}}, Row{}},
                                Shape{"refused: a non-empty C", Row{{one, 1}}, Row{{k, 0}, {F::neg(k), 1}}, Row{{one, 0}}},
                                Shape{"refused: a further entry", Row{{one, 1}, {one, 2}}, Row{{k, 0}, {F::neg(k), 1}}, Row{}},
                                Shape{"refused: the constant at another column", Row{{one, 1}}, Row{{k, 2}, {F::neg(k), 1}}, Row{}},
                                Shape{"refused: u in A and in C", Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}}}}) {
            System s; s.m0 = 1; s.mw = 2;
            s.add(Row{{one, 2}}, Row{{one, 0}}, Row{{one, 2}});
            s.add(sh.a, sh.b, sh.c);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}});      // a later row would solve it: refused all the same
            const Plan p = in_order(s, s.unknown({1}));
            check(p.error == ERR_TWO_MATRICES && p.error_row == 1 && p.error_col == 1, sh.what);
        }
        {   // the shape itself, with a zero coefficient that names no variable, and solved by the later row
            System s; s.m0 = 1; s.mw = 2;
            s.add(Row{{k, 1}, {F::zero(), 2}}, Row{{F::neg(one), 1}, {one, 0}}, Row{{F::zero(), 1}});
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}});
            const Plan p = in_order(s, s.unknown({1}));
            check(p.error == OK && p.steps.size() == 1 && step_is(p, 0, 1, 1, KIND_A, 1, 2, {}), "a booleanity row is a check row once a later row solves its column");
        }
    }

    // ---- 4. without the modulus the builder is the earlier one; with it, plans without boolean columns are the same plans
    void parent_equivalence() {
        const Fr one = F::one();
        {
            System s; s.m0 = 1; s.mw = 3;             // row 1 has two unknowns
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(Row{{one, 2}}, Row{{one, 3}}, Row{{one, 1}});
            for (bool with : {false, true}) {
                const Plan p = in_order(s, {0, 0, 1, 1}, WIDE_STEPS, with);
                check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.error_col == 3 && p.message.find("row 1: two or more unknowns (columns 2 and 3)") == 0,
                      with ? "equivalence: two unknowns, with the modulus" : "equivalence: two unknowns, without");
            }
        }
        {
            System s; s.m0 = 1; s.mw = 2;             // b (1 - b) = 0 in row 2 and nothing else names b
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(Row{{one, 1}}, Row{{one, 1}}, Row{{one, 1}});
            s.add(Row{{one, 2}}, Row{{one, 0}, {F::neg(one), 2}}, Row{});
            const Plan without = in_order(s, {0, 0, 1}, WIDE_STEPS, false), with = in_order(s, {0, 0, 1});
            check(without.error == ERR_TWO_MATRICES && without.error_row == 2 && without.error_col == 2 && without.message == "row 2: unknown column 2 occurs in A and in B",
                  "equivalence: b (1 - b) = 0 without the modulus");
            check(with.error == ERR_TWO_MATRICES && with.error_row == 2 && with.error_col == 2 && with.message.find(without.message) == 0, "equivalence: ... and with it");
        }
        {   // three MiMC rounds: columns 0 one, 1 out, 2 xl, 3 xr, 4 tmp0, 5 new0, 6 tmp1, 7 new1, 8 tmp2
            System s; s.m0 = 2; s.mw = 7;
            const Fr m1 = F::neg(one), kc[3] = {rnd(), rnd(), rnd()};
            const uint32_t xl[3] = {2, 5, 7}, xr[3] = {3, 2, 5}, tmp[3] = {4, 6, 8}, nw[3] = {5, 7, 1};
            for (int i = 0; i < 3; ++i) {
                const Row lc = {{one, xl[i]}, {kc[i], 0}};
                s.add(lc, lc, Row{{one, tmp[i]}});
                s.add(Row{{one, tmp[i]}}, lc, Row{{one, nw[i]}, {m1, xr[i]}});
            }
            const std::vector<uint8_t> unknown = {0, 1, 0, 0, 1, 1, 1, 1, 1};
            for (uint32_t wide : {WIDE_STEPS, 1u}) {
                const Plan a = in_order(s, unknown, wide, false), b = in_order(s, unknown, wide);
                check(a.error == OK && a.steps.size() == 6 && same_plan(a, b), "equivalence: the MiMC-shaped plan");
            }
        }
        {   // kinds A, B, C: 0 one, 1 a, 2 c, 3 inv, 4 q, 5 s, 6 t
            System s; s.m0 = 1; s.mw = 6;
            s.add(Row{{u(3), 3}}, Row{{one, 1}}, Row{{one, 0}});
            s.add(Row{{one, 1}}, Row{{u(5), 4}}, Row{{one, 2}});
            s.add(Row{{one, 3}}, Row{{one, 4}}, Row{{one, 5}});
            s.add(Row{{one, 5}, {one, 0}}, Row{{u(2), 6}}, Row{{one, 3}});
            const std::vector<uint8_t> unknown = {0, 0, 0, 1, 1, 1, 1};
            for (uint32_t wide : {WIDE_STEPS, 1u}) {
                const Plan a = in_order(s, unknown, wide, false), b = in_order(s, unknown, wide);
                check(a.error == OK && a.steps.size() == 4 && a.launches.size() == (wide == 1 ? 3u : 1u) && same_plan(a, b), "equivalence: the A / B / C plan");
            }
        }
    }

    int run() {
        accepted();
        widest();
        refused();
        parent_equivalence();
        return report();
    }
};

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381", 255);
    Suite<pm::BnCurve> bn("bn254", 254);
    return (bls.run() | bn.run()) ? 1 : 0;
}
