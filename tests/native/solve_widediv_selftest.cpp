// CPU self-test of the witness solver's declared WIDE LONG-DIVISION hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode 5,
// KIND_LONGDIV_WIDE, LAUNCH_LONGDIV_WIDE; polymath_amd/csrc/solve_steps.cuh: wide_estimate, longdiv_wide_words, solve_longdiv_wide) on
// the rig of the other solve_*_selftest.cpp programs.  Stand-alone: g++ -std=c++17, no HIP, no GPU; longdiv_wide_words, which runs
// here, is the statement of the recurrence that the kernel k_solve_longdiv_wide distributes over a wave.  Its literals are not committed:
// solve_widediv_cases.hpp is what
//     python tools/gen_solve_widediv_cases.py > DIR/solve_widediv_cases.hpp
// writes, and the program is built with -I DIR (tests/test_native_solve_widediv.py does both).
//   1. wide divisions against literals computed with Python's divmod, the six shapes and the operand families of the GPU test; by
//      longdiv_wide_words' counters the add-back family executes an add-back and the saturating family a saturated estimate at every
//      listed size; every stuck condition at its boundary and beside it
//   2. every refusal of the new record with its text and at its boundary; opcodes 2 and 4 still refused; opcode 1 with kD = 33 still
//      refused with its text; all three opcodes in one declaration; an output named by hints of two opcodes
//   3. levels and launches where the three hint kinds meet: order, separate launches, rounds
//   4. ACTIVE / INERT / mixed markers, a never-ready hint
//   5. a corpus of rows and wide hints, in matrix order, reversed and shuffled: the same assignment
//   6. the stuck word nr + h and the root-cause rule
#include "solve_selftest.hpp"
#include "solve_widediv_cases.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    const WidedivCase *cases;
    size_t n_cases;
    const uint64_t (*pool)[4];
    Suite(const char *n, const WidedivCase *c, size_t nc, const uint64_t (*p)[4]) : Rig(n), cases(c), n_cases(nc), pool(p) {}

    static std::vector<uint64_t> wide(uint32_t n, const Cols &q, const Cols &rem, const Cols &D, const Cols &E, const std::vector<uint64_t> &lit = {}) {
        return longdiv_record(n, q, rem, D, E, lit, HINT_LONGDIV_WIDE);
    }
    static std::vector<uint64_t> moddiv_record(uint32_t n, const Cols &z, const Cols &Dp, uint64_t modulus_literal) {
        std::vector<uint64_t> w = {HINT_MODDIV, n, z.size(), 0, 0, Dp.size(), 0, 1, HINT_MODULUS_LITERAL};
        for (const Cols *cols : {&z, &Dp}) w.insert(w.end(), cols->begin(), cols->end());
        const uint64_t lit[4] = {modulus_literal, 0, 0, 0};
        w.insert(w.end(), lit, lit + 4);
        return w;
    }
    static void append(std::vector<uint64_t> &to, const std::vector<uint64_t> &more) { to.insert(to.end(), more.begin(), more.end()); }

    // ---- 1. wide divisions against Python's divmod.  A system without rows: columns 1 .. D, E (unless it is a literal), q, rem; the one
    // hint is ready at once
    void divisions() {
        for (size_t i = 0; i < n_cases; ++i) {
            const WidedivCase &c = cases[i];
            const std::string tag = std::string("widediv ") + c.name;
            System s;
            const uint32_t kE_cols = c.literal ? 0 : c.kE;
            s.mw = c.kD + kE_cols + c.kq + c.kr;
            const Cols D = range(1, c.kD), E = range(1 + c.kD, kE_cols), Q = range(1 + c.kD + kE_cols, c.kq), R = range(1 + c.kD + kE_cols + c.kq, c.kr);
            std::vector<uint64_t> lit;
            for (uint32_t j = 0; c.literal && j < c.kE; ++j) lit.insert(lit.end(), pool[c.at + c.kD + j], pool[c.at + c.kD + j] + 4);
            std::string why;
            const std::vector<Hint> hints = declare(s, wide(c.n, Q, R, D, E, lit), &why);
            check(why.empty() && hints.size() == 1, tag + ": the declaration is accepted");
            if (hints.size() != 1) { printf("%s: %s\n", name, why.c_str()); continue; }
            std::vector<uint32_t> outs = Q;
            outs.insert(outs.end(), R.begin(), R.end());
            const Plan p = hinted(s, s.unknown(outs), hints);
            Step want{0, 0, Q[0], KIND_LONGDIV_WIDE, 1};
            check(p.error == OK && p.steps.size() == 1 && same_step(p.steps[0], want) && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_LONGDIV_WIDE &&
                      p.launches[0].lo == 0 && p.launches[0].hi == 1 && p.launches[0].rounds == std::min(8192u, c.n * (c.kD - 1) + 256u) && well_sorted(p) && p.reordered &&
                      p.hints.size() == 1,
                  tag + ": one step of kind KIND_LONGDIV_WIDE at level 1, row nr + 0, a launch of its own with its bound");
            if (p.error != OK) continue;
            std::vector<Fr> z(s.m0 + s.mw, marker());
            z[0] = F::one();
            for (uint32_t j = 0; j < c.kD + kE_cols; ++j) z[1 + j] = from_words(pool[c.at + j]);
            pm::WideCounters counters;
            const uint64_t stuck = execute(s, p, z, nullptr, &counters);
            check(c.stuck ? stuck == ((uint64_t)1 << 32 | 0) : stuck == NONE, tag + (c.stuck ? ": stuck at the hint's word" : ": not stuck"));
            bool ok = true;
            for (uint32_t j = 0; j < c.kq + c.kr; ++j) ok = ok && z[outs[j]].eq(from_words(pool[c.at + c.kD + c.kE + j]));
            check(ok, tag + (c.stuck ? ": zero in every output" : ": the limbs of Python's divmod"));
            if (c.addback) check(counters.addbacks >= 1, tag + ": the recurrence executed an add-back");
            if (c.saturating) check(counters.saturated >= 1, tag + ": the recurrence executed a saturated estimate");
        }
    }

    // ---- 2. refusals
    void refuse_decl(const System &s, const std::vector<uint64_t> &desc, const std::string &text) {
        std::string why;
        const std::vector<Hint> hints = declare(s, desc, &why);
        if (why != text) printf("%s: got \"%s\"\n", name, why.c_str());
        check(why == text && hints.empty(), "refused at the declaration: " + text);
    }
    void refusals() {
        System s; s.mw = 400;
        const Cols q = {10, 11}, rem = {12}, D = {1, 2, 3}, E = {4, 5};
        const std::vector<uint64_t> good = wide(64, q, rem, D, E);
        std::string why;
        std::vector<Hint> got = declare(s, good, &why);
        check(got.size() == 1 && why.empty() && got[0].op == HINT_LONGDIV_WIDE && got[0].n == 64 && got[0].q == q && got[0].rem == rem && got[0].D == D && got[0].E == E &&
                  got[0].lit.empty() && got[0].index == 0,
              "a good record is accepted, field by field");
        std::vector<uint64_t> bad, two;
        for (uint64_t op : {2ull, 4ull, 6ull, 0ull}) {
            bad = good; bad[0] = op;
            refuse_decl(s, bad, "hint 0: unknown opcode " + std::to_string(op));
        }
        bad = good; bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        refuse_decl(s, {HINT_LONGDIV_WIDE, 64, 1, 1, 1, 1}, "hint 0: the record is truncated");
        bad = good; bad[1] = 0;
        refuse_decl(s, bad, "hint 0: n = 0 is outside 1..128");
        bad = good; bad[1] = 129;
        refuse_decl(s, bad, "hint 0: n = 129 is outside 1..128");
        const char *names[4] = {"kq", "kr", "kD", "kE"};
        const uint32_t limits[4] = {128, 64, 128, 64};
        for (int i = 0; i < 4; ++i) {
            const std::string lim = std::to_string(limits[i]);
            bad = good; bad[2 + i] = 0;
            refuse_decl(s, bad, std::string("hint 0: ") + names[i] + " = 0 is outside 1.." + lim);
            bad = good; bad[2 + i] = limits[i] + 1;
            refuse_decl(s, bad, std::string("hint 0: ") + names[i] + " = " + std::to_string(limits[i] + 1) + " is outside 1.." + lim);
        }
        check(declare(s, wide(1, range(10, 128), range(140, 64), range(205, 128), range(333, 64)), &why).size() == 1 && why.empty(), "every count at its limit is accepted");
        bad = good; bad[6] = 2;
        refuse_decl(s, bad, "hint 0: unknown flags 2");
        refuse_decl(s, wide(128, q, rem, range(20, 65), E), "hint 0: n (kD - 1) = 8192 is 8192 or more");
        check(declare(s, wide(127, q, rem, range(20, 65), E), &why).size() == 1 && why.empty(), "n (kD - 1) = 8128 is accepted");
        refuse_decl(s, wide(8192, q, rem, range(20, 2), E), "hint 0: n = 8192 is outside 1..128");
        // 8191 is prime, so no n <= 128 and kD <= 128 give n (kD - 1) = 8191: the largest product below 8192 is 8190 = 126 * 65
        check(declare(s, wide(126, q, rem, range(20, 66), E), &why).size() == 1 && why.empty(), "n (kD - 1) = 8190, the largest product below 8192 inside the limits, is accepted");
        refuse_decl(s, wide(128, q, rem, D, range(20, 33)), "hint 0: n (kE - 1) = 4096 is 4096 or more");
        check(declare(s, wide(65, q, rem, D, range(20, 64)), &why).size() == 1 && why.empty(), "n (kE - 1) = 4095 is accepted");
        // opcode 1 is not widened: its limits and texts are what they were
        refuse_decl(s, longdiv_record(16, q, rem, range(20, 33), E), "hint 0: kD = 33 is outside 1..32");
        refuse_decl(s, longdiv_record(16, q, rem, D, range(20, 17)), "hint 0: kE = 17 is outside 1..16");
        refuse_decl(s, longdiv_record(128, q, rem, range(20, 9), E), "hint 0: n (kD - 1) = 1024 is 1024 or more");
        check(declare(s, wide(16, q, rem, range(20, 33), E), &why).size() == 1 && why.empty(), "kD = 33 is accepted under opcode 5");
        refuse_decl(s, wide(64, q, rem, {1, 401}, E), "hint 0: column 401 is not below m0 + mw = 401");
        refuse_decl(s, wide(64, {10, 0}, rem, D, E), "hint 0: an output is column 0 (the constant one)");
        refuse_decl(s, wide(64, {10, 10}, rem, D, E), "hint 0: output column 10 is named twice");
        refuse_decl(s, wide(64, q, rem, {1, 12}, E), "hint 0: output column 12 is an input of the hint as well");
        std::vector<uint64_t> lit = {3, 0, 0, 0, modulus[0], modulus[1], modulus[2], modulus[3]};
        refuse_decl(s, wide(64, q, rem, D, {}, lit), "hint 0: literal limb 1 is not below r");
        lit[4] -= 1;
        got = declare(s, wide(64, q, rem, D, {}, lit), &why);
        check(got.size() == 1 && why.empty() && got[0].flags == HINT_DIVISOR_LITERAL && got[0].E.empty() && got[0].lit.size() == 8, "a literal limb equal to r - 1 is accepted");
        // all three opcodes in one declaration share the index h and the set of outputs
        two = longdiv_record(64, {20, 21}, {22}, {1, 2, 3}, {4});
        append(two, good);
        append(two, moddiv_record(64, {30}, {1}, 101));
        append(two, wide(64, {31, 32}, {33}, D, E));
        got = declare(s, two, &why);
        check(got.size() == 4 && why.empty() && got[0].op == HINT_LONGDIV && got[1].op == HINT_LONGDIV_WIDE && got[2].op == HINT_MODDIV && got[3].op == HINT_LONGDIV_WIDE &&
                  got[1].index == 1 && got[2].index == 2 && got[3].index == 3 && got[3].q == Cols({31, 32}),
              "all three opcodes in one declaration, in any mixture, share the index");
        two = longdiv_record(64, {20, 21}, {22}, {1, 2, 3}, {4});
        append(two, wide(64, {23, 22}, rem, D, E));
        refuse_decl(s, two, "hint 1: output column 22 is an output of hint 0 as well");
        two = good;
        append(two, moddiv_record(64, {11}, {1}, 101));
        refuse_decl(s, two, "hint 1: output column 11 is an output of hint 0 as well");
        two = moddiv_record(64, {30}, {1}, 101);
        append(two, wide(64, q, {30}, D, E));
        refuse_decl(s, two, "hint 1: output column 30 is an output of hint 0 as well");
        two = good;
        bad = good; bad[0] = 4;
        append(two, bad);
        refuse_decl(s, two, "hint 1: unknown opcode 4");
        check(NUM_KINDS == 7 && NUM_STEP_KINDS == 8 && NUM_SORT_KINDS == 11 && NUM_PLAN_KINDS == 12 && NUM_HINT_KINDS == 13 && NUM_WIDE_KINDS == 14 && KIND_LONGDIV == 11 &&
                  KIND_MODDIV == 12 && KIND_LONGDIV_WIDE == 13 && HINT_LONGDIV == 1 && HINT_MODDIV == 3 && HINT_LONGDIV_WIDE == 5 && WIDE_MAX_KD == 128 && WIDE_MAX_KE == 64 &&
                  WIDE_MAX_KQ == 128 && WIDE_MAX_KR == 64 && WIDE_D_BITS == 8192 && WIDE_E_BITS == 4096 && HINT_MAX_KD == 32 && HINT_D_BITS == 1024,
              "the kind numbering, the opcodes and the limits");
    }

    // ---- 3. levels and launches where the three hint kinds meet
    void levels_and_launches() {
        const Fr one = F::one();
        // 0 one | 1 a, 2 b, 3 e given | 4 d = a b (row 0) | 5 q, 6 rem = divmod(d, e) NARROW | 7 Z = 1 / d mod 101 | 8 q', 9 rem' = divmod(d, e) WIDE
        // 10 q'', 11 rem'' = divmod(Z, e) WIDE (n = 128, so the launch's bound is the larger) | 12 y = q'' a (row 1)
        System s; s.mw = 12;
        s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 4}});
        s.add(Row{{one, 10}}, Row{{one, 1}}, Row{{one, 12}});
        std::vector<uint64_t> desc = wide(64, {8}, {9}, {4}, {3});
        append(desc, moddiv_record(64, {7}, {4}, 101));
        append(desc, longdiv_record(64, {5}, {6}, {4}, {3}));
        append(desc, wide(128, {10}, {11}, {7, 0}, {3}));
        std::string why;
        const std::vector<Hint> hints = declare(s, desc, &why);
        check(hints.size() == 4 && why.empty(), "meeting: four hints of three opcodes are accepted");
        const Plan p = hinted(s, s.unknown({4, 5, 6, 7, 8, 9, 10, 11, 12}), hints);
        // level 1: row 0.  level 2: the narrow division (hint 2, row 4), the modular one (hint 1, row 3), the wide one (hint 0, row 2).  level 3: wide hint 3 (row 5).  level 4: row 1
        const uint32_t kinds[6] = {KIND_C, KIND_LONGDIV, KIND_MODDIV, KIND_LONGDIV_WIDE, KIND_LONGDIV_WIDE, KIND_C}, rows[6] = {0, 4, 3, 2, 5, 1}, lv[6] = {1, 2, 2, 2, 3, 4};
        bool ok = p.error == OK && p.steps.size() == 6 && well_sorted(p) && p.launches.size() == 6;
        for (int t = 0; ok && t < 6; ++t) ok = p.steps[t].kind == kinds[t] && p.steps[t].row == rows[t] && p.steps[t].level == lv[t];
        for (int t = 0; ok && t < 6; ++t)
            ok = p.launches[t].lo == (uint32_t)t && (p.launches[t].kind == LAUNCH_LONGDIV_WIDE) == (kinds[t] == KIND_LONGDIV_WIDE) && (p.launches[t].kind == LAUNCH_MODDIV) == (kinds[t] == KIND_MODDIV) &&
                 (p.launches[t].kind == LAUNCH_LONGDIV) == (kinds[t] == KIND_LONGDIV);
        check(ok && p.launches[3].rounds == 256 && p.launches[4].rounds == 128 + 256, "meeting: in a level the narrow divisions' launch, the modular one, then the wide one; rounds = min(8192, n (kD - 1) + 256)");
        if (p.error != OK) printf("%s: %s\n", name, p.message.c_str());
        std::vector<Fr> z(13, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[3] = u(5);
        // d = 42 = 8 * 5 + 2; Z = 1 / 42 mod 101 = 89; D'' = 89 + 2^128, q'' = floor(D'' / 5), rem'' = D'' mod 5: 2^128 = 1 mod 5, so 90 mod 5 = 0
        ok = ok && execute(s, p, z) == NONE && z[4].eq(u(42)) && z[5].eq(u(8)) && z[6].eq(u(2)) && z[7].eq(u(89)) && z[8].eq(u(8)) && z[9].eq(u(2)) && z[11].is_zero() &&
             F::mul(z[10], u(5)).eq(F::add(u(89), F::pow(u(2), 128))) && rows_hold(s, z);
        check(ok, "meeting: executes to 42 = 8 * 5 + 2 twice, 1 / 42 = 89 (mod 101) and (89 + 2^128) / 5 exactly");
        {   // two wide shapes in one launch: the bound is the larger one
            System t; t.mw = 200;
            std::vector<uint64_t> both = wide(64, {150}, {151}, range(1, 63), {140});
            append(both, wide(121, {152}, {153}, range(70, 33), {141}));
            const std::vector<Hint> h2 = declare(t, both, &why);
            const Plan p2 = hinted(t, t.unknown({150, 151, 152, 153}), h2);
            check(p2.error == OK && p2.launches.size() == 1 && p2.launches[0].kind == LAUNCH_LONGDIV_WIDE && p2.launches[0].rounds == 64 * 62 + 256 && p2.steps[0].row == 0 && p2.steps[1].row == 1,
                  "two shapes in one launch: rounds is the larger of 4224 and 4128");
        }
    }

    // ---- 4. ACTIVE / INERT / mixed markers, a never-ready hint
    void markers() {
        System s; s.mw = 60;
        const Fr one = F::one();
        const Cols q = {10, 11}, rem = {12}, D = {1, 2, 3}, E = {4, 5};
        const std::vector<Hint> hints = declare(s, wide(64, q, rem, D, E));
        s.add(Row{{one, 40}}, Row{{one, 41}}, Row{{one, 30}});
        Plan p = hinted(s, s.unknown({10, 30}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: some outputs are marked unknown and some are given" && p.steps.empty(), "refused: outputs partly given");
        p = hinted(s, s.unknown({11, 12, 30}, {10}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: an output carries the quotient, indicator or square-root marker" && p.steps.empty(), "refused: the quotient marker on an output");
        for (uint32_t col : {1u, 3u, 5u}) {
            Plan r = hinted(s, s.unknown({10, 11, 12, col}), hints);
            const std::string c = std::to_string(col);
            check(r.error == ERR_UNDETERMINED && r.error_col == col && r.message == "hint 0: input column " + c + " is never determined; column " + c + " stays unknown" &&
                      r.steps.empty() && r.hints.empty() && r.launches.empty(),
                  "refused: input column " + c + " (a dividend or divisor limb) that no row determines");
        }
        p = hinted(s, s.unknown({10, 11, 12, 30}), hints);
        check(p.error == OK && count_kind(p, KIND_LONGDIV_WIDE) == 1 && p.steps.size() == 2 && well_sorted(p), "active: all outputs marked, one wide step beside the row");
        {   // inert: the outputs are given, and the plan is the plan without the declaration
            const std::vector<uint8_t> un = s.unknown({30});
            const Plan with = hinted(s, un, hints), without = any_order(s, un);
            check(with.error == OK && same_plan(with, without) && with.hints.empty() && with.launches.size() == 1 && with.launches[0].kind != LAUNCH_LONGDIV_WIDE && with.launches[0].rounds == 0,
                  "inert: the plan without the declaration, field by field");
        }
    }

    // ---- 5. a corpus of rows and wide hints: x_{t+1} = (x_t b) mod e and y_t = floor(x_t b / e), one row (the product) and one hint a step, a closing sum
    void corpus_any_order() {
        const Fr one = F::one();
        const uint32_t steps = 5;
        const uint64_t e = 1000003, b = 999983;
        System s;
        // 0 one | 1 the public sum | 2 x_0, 3 b, 4 e given | per step t: 5 + 3 t the product, 6 + 3 t the quotient, 7 + 3 t x_{t+1}
        s.m0 = 2; s.mw = 3 + 3 * steps;
        std::vector<uint64_t> desc;
        Cols unknown = {1};
        Row total;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t x = t ? 4 + 3 * t : 2, prod = 5 + 3 * t, quo = 6 + 3 * t, next = 7 + 3 * t;
            s.add(Row{{one, x}}, Row{{one, 3}}, Row{{one, prod}});
            append(desc, t & 1 ? wide(64, {quo}, {next}, {prod}, {}, {e, 0, 0, 0}) : wide(40, {quo}, {next}, {prod}, {4}));
            for (uint32_t col : {prod, quo, next}) unknown.push_back(col);
            total.push_back({one, next});
            total.push_back({one, quo});
        }
        s.add(total, Row{{one, 0}}, Row{{one, 1}});
        const std::vector<Hint> hints = declare(s, desc);
        const std::vector<uint8_t> un = s.unknown(unknown);
        const Plan p = hinted(s, un, hints);
        bool ok = p.error == OK && p.reordered && well_sorted(p) && count_kind(p, KIND_LONGDIV_WIDE) == steps && p.steps.size() == 2 * steps + 1 && p.levels() == 2 * steps + 1;
        for (size_t t = 0; ok && t < p.steps.size(); ++t) ok = p.steps[t].level == t + 1 && (p.steps[t].kind == KIND_LONGDIV_WIDE) == (t % 2 == 1 && t < 2 * steps);
        check(ok, "corpus: rows and wide hints alternate over 11 levels");
        const Plan bare = any_order(s, un);
        check(bare.error != OK && bare.steps.empty(), "corpus: refused without the declaration");
        const auto start = [&](const System &t) {
            std::vector<Fr> z(t.m0 + t.mw, marker());
            z[0] = one; z[2] = u(123456); z[3] = u(b); z[4] = u(e);
            return z;
        };
        std::vector<Fr> z = start(s);
        uint64_t x = 123456, sum = 0;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint64_t prod = x * b;
            sum += prod / e + prod % e;
            x = prod % e;
        }
        check(ok && execute(s, p, z) == NONE && rows_hold(s, z) && z[1].eq(u(sum)) && z[4 + 3 * steps].eq(u(x)), "corpus: executes to the values of a 64-bit computation, and every row holds");
        for (int round = 0; round < 3; ++round) {
            std::vector<uint32_t> order(s.nr());
            for (uint32_t r = 0; r < order.size(); ++r) order[r] = round == 0 ? (uint32_t)order.size() - 1 - r : r;
            for (size_t r = order.size(); round && r > 1; --r) std::swap(order[r - 1], order[next_u64() % r]);
            System t = s.permuted(order);
            const Plan q = hinted(t, un, hints);
            std::vector<Fr> zt = start(t);
            bool equal = q.error == OK && well_sorted(q) && q.levels() == p.levels() && count_kind(q, KIND_LONGDIV_WIDE) == steps && execute(t, q, zt) == NONE && rows_hold(t, zt);
            for (size_t j = 0; equal && j < p.steps.size(); ++j) equal = q.steps[j].level == p.steps[j].level && q.steps[j].kind == p.steps[j].kind && q.steps[j].col == p.steps[j].col;
            for (size_t j = 0; equal && j < z.size(); ++j) equal = zt[j].eq(z[j]);
            check(equal, std::string("corpus: ") + (round ? "shuffled" : "reversed") + ", the same levels and the same assignment");
        }
    }

    // ---- 6. stuck under a plan with rows: the hint's word, not the row that then divides by the stored zero
    void stuck_word() {
        // 0 one | 1 a, 2 b given | 3 d = a b (row 0) | 4 q, 5 rem = divmod(d, e), e = column 6 given | 7 y = 1 / q by row 1: y * q = 1
        System s; s.mw = 7;
        const Fr one = F::one();
        s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 3}});
        s.add(Row{{one, 7}}, Row{{one, 4}}, Row{{one, 0}});
        const std::vector<Hint> hints = declare(s, wide(64, {4}, {5}, {3}, {6}));
        const Plan p = hinted(s, s.unknown({3, 4, 5, 7}), hints);
        check(p.error == OK && p.steps.size() == 3 && p.steps[1].kind == KIND_LONGDIV_WIDE && p.steps[1].row == 2 && p.steps[1].level == 2 && p.steps[2].level == 3,
              "stuck: the hint between two rows, at row nr + 0 = 2 and level 2");
        std::vector<Fr> z(8, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[6] = F::zero();
        check(execute(s, p, z) == ((uint64_t)2 << 32 | 2) && z[4].is_zero() && z[5].is_zero(), "stuck: E = 0 is reported at the hint, not at the row that then divides by the stored zero");
        z.assign(8, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[6] = u(100);
        check(execute(s, p, z) == ((uint64_t)3 << 32 | 1) && z[4].is_zero() && z[5].eq(u(42)), "stuck: a quotient of zero is no stuck hint; the row that inverts it sticks, at its own row");
        z.assign(8, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[6] = u(42);
        check(execute(s, p, z) == NONE && z[4].eq(one) && z[5].is_zero() && rows_hold(s, z), "stuck: the same plan on E = 42 completes");
    }

    int run() {
        divisions();
        refusals();
        levels_and_launches();
        markers();
        corpus_any_order();
        stuck_word();
        return report();
    }
};

#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381", WIDEDIV_BLS, COUNT(WIDEDIV_BLS), WIDEDIV_POOL_BLS);
    Suite<pm::BnCurve> bn("bn254", WIDEDIV_BN, COUNT(WIDEDIV_BN), WIDEDIV_POOL_BN);
    return (bls.run() | bn.run()) ? 1 : 0;
}
