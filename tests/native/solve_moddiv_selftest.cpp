// CPU self-test of the witness solver's declared MODULAR-DIVISION hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode 3,
// KIND_MODDIV, LAUNCH_MODDIV and its two trip counts; polymath_amd/csrc/solve_steps.cuh: sub_masked, add_masked, modinv_odd,
// solve_moddiv) on the rig of the other solve_*_selftest.cpp programs.  Stand-alone: g++ -std=c++17, no HIP, no GPU; the step body that
// runs here is the text the kernel k_solve_moddiv calls.  Its literals are not committed: solve_moddiv_cases.hpp is what
//     python tools/gen_solve_moddiv_cases.py > DIR/solve_moddiv_cases.hpp
// writes, and the program is built with -I DIR (tests/test_native_solve_moddiv.py does both).
//   1. modular divisions against literals computed with Python's pow(D, -1, P), for P = secp256k1's prime, BLS12-381's q, 2^512 - 1,
//      3 and the composite 15 (2^89 - 1): D = 1, P - 1, (P +- 1) / 2, 2^(L - 1), 0, P, a D that shares a factor with P, limbs that are
//      not normalised and carry, D+ < D-, N+ < N-, N = 1; every stuck condition at its boundary and beside it.  THE TRIP-COUNT BOUND is
//      exercised at its worst cases, which the cases name: "D = 2^(L - 1)" (L - 1 halvings before the first subtraction),
//      "D = P - 1" and "D = (P +- 1) / 2" (subtractions that shorten by one bit), each under inv_rounds = 2 L exactly
//   2. every refusal of the new record with its text; opcode 2 still refused; both opcodes in one declaration
//   3. one step of KIND_MODDIV at the right level with row = nr + h, in a launch of its own after the long divisions of its level; a
//      modular hint that waits for a long division's output, and the reverse; never-ready hints
//   4. a chain of rows and modular hints, in matrix order, reversed and shuffled: the same levels and the same assignment
//   5. the stuck word under a plan with rows, and two shapes in one launch: the trip counts are the larger ones
#include "solve_selftest.hpp"
#include "solve_moddiv_cases.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    const ModdivCase *cases;
    size_t n_cases;
    const uint64_t (*pool)[4];
    Suite(const char *n, const ModdivCase *c, size_t nc, const uint64_t (*p)[4]) : Rig(n), cases(c), n_cases(nc), pool(p) {}

    // one modular-division record of pm_pk_set_hints; `lit`: the modulus' limbs as canonical words (then Pc is empty)
    static std::vector<uint64_t> record(uint32_t n, const Cols &z, const Cols &Np, const Cols &Nm, const Cols &Dp, const Cols &Dm, const Cols &Pc,
                                        const std::vector<uint64_t> &lit = {}) {
        std::vector<uint64_t> w = {HINT_MODDIV, n, z.size(), Np.size(), Nm.size(), Dp.size(), Dm.size(), lit.empty() ? Pc.size() : lit.size() / 4,
                                   lit.empty() ? 0 : HINT_MODULUS_LITERAL};
        for (const Cols *cols : {&z, &Np, &Nm, &Dp, &Dm, &Pc}) w.insert(w.end(), cols->begin(), cols->end());
        w.insert(w.end(), lit.begin(), lit.end());
        return w;
    }
    static std::vector<uint64_t> literal(uint64_t v) { return {v, 0, 0, 0}; }

    // ---- 1. modular divisions against Python's pow.  A system without rows: columns 1 .. N+, N-, D+, D-, the modulus (unless it is a
    // literal), Z; the one hint is ready at once
    void divisions() {
        for (size_t i = 0; i < n_cases; ++i) {
            const ModdivCase &c = cases[i];
            const std::string tag = std::string("moddiv ") + c.name;
            System s;
            const uint32_t kP_cols = c.literal ? 0 : c.kP, k_all = c.k[0] + c.k[1] + c.k[2] + c.k[3];
            s.mw = k_all + kP_cols + c.kz;
            const Cols Np = range(1, c.k[0]), Nm = range(1 + c.k[0], c.k[1]), Dp = range(1 + c.k[0] + c.k[1], c.k[2]), Dm = range(1 + c.k[0] + c.k[1] + c.k[2], c.k[3]),
                       Pc = range(1 + k_all, kP_cols), Z = range(1 + k_all + kP_cols, c.kz);
            std::vector<uint64_t> lit;
            for (uint32_t j = 0; c.literal && j < c.kP; ++j) lit.insert(lit.end(), pool[c.at + k_all + j], pool[c.at + k_all + j] + 4);
            std::string why;
            const std::vector<Hint> hints = declare(s, record(c.n, Z, Np, Nm, Dp, Dm, Pc, lit), &why);
            check(why.empty() && hints.size() == 1, tag + ": the declaration is accepted");
            if (hints.size() != 1) { printf("%s: %s\n", name, why.c_str()); continue; }
            const Plan p = hinted(s, s.unknown(Z), hints);
            uint32_t rounds = 0;
            for (uint32_t k : c.k)
                if (k) rounds = std::max(rounds, std::min(1024u, c.n * (k - 1) + 256u));
            const uint32_t L = std::min(512u, c.n * (c.kP - 1) + 256u);
            Step want{0, 0, Z[0], KIND_MODDIV, 1};
            check(p.error == OK && p.steps.size() == 1 && same_step(p.steps[0], want) && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_MODDIV &&
                      p.launches[0].lo == 0 && p.launches[0].hi == 1 && p.launches[0].rounds == rounds && p.launches[0].inv_rounds == 2 * L &&
                      well_sorted(p) && p.reordered && p.hints.size() == 1,
                  tag + ": one step of kind KIND_MODDIV at level 1, row nr + 0, a launch of its own with both trip counts");
            if (p.error != OK) continue;
            std::vector<Fr> z(s.m0 + s.mw, marker());
            z[0] = F::one();
            for (uint32_t j = 0; j < k_all + kP_cols; ++j) z[1 + j] = from_words(pool[c.at + j]);
            const uint64_t stuck = execute(s, p, z);
            check(c.stuck ? stuck == ((uint64_t)1 << 32 | 0) : stuck == NONE, tag + (c.stuck ? ": stuck at the hint's word" : ": not stuck"));
            bool ok = true;
            for (uint32_t j = 0; j < c.kz; ++j) ok = ok && z[Z[j]].eq(from_words(pool[c.at + k_all + c.kP + j]));
            check(ok, tag + (c.stuck ? ": zero in every output" : ": the limbs of Python's N pow(D, -1, P) mod P"));
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
        System s; s.mw = 60;
        const Cols z = {10, 11}, Np = {1, 2}, Nm = {3}, Dp = {4, 5}, Dm = {6}, Pc = {7, 8};
        const std::vector<uint64_t> good = record(64, z, Np, Nm, Dp, Dm, Pc);
        std::string why;
        std::vector<Hint> got = declare(s, good, &why);
        check(got.size() == 1 && why.empty() && got[0].op == HINT_MODDIV && got[0].n == 64 && got[0].q == z && got[0].rem.empty() && got[0].D == Cols({1, 2, 3, 4, 5, 6}) &&
                  got[0].E == Pc && got[0].k[0] == 2 && got[0].k[1] == 1 && got[0].k[2] == 2 && got[0].k[3] == 1 && got[0].lit.empty() && got[0].index == 0,
              "a good record is accepted, field by field");
        got = declare(s, record(64, z, {}, {}, Dp, {}, {}, {3, 0, 0, 0, 1, 0, 0, 0}), &why);
        check(got.size() == 1 && why.empty() && got[0].flags == HINT_MODULUS_LITERAL && got[0].E.empty() && got[0].lit.size() == 8 && got[0].D == Dp, "a plain inverse with a literal modulus is accepted");
        std::vector<uint64_t> bad, two;
        bad = good; bad[0] = 2;
        refuse_decl(s, bad, "hint 0: unknown opcode 2");
        bad = good; bad[0] = 4;
        refuse_decl(s, bad, "hint 0: unknown opcode 4");
        bad = good; bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        refuse_decl(s, {HINT_MODDIV, 64, 1, 0, 0, 1, 0, 1}, "hint 0: the record is truncated");
        two = good;
        two.insert(two.end(), good.begin(), good.begin() + 11);                  // a second record that ends inside its columns
        refuse_decl(s, two, "hint 1: the record is truncated");
        bad = record(64, z, {}, {}, Dp, {}, {}, {3, 0, 0, 0}); bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        bad = good; bad[1] = 0;
        refuse_decl(s, bad, "hint 0: n = 0 is outside 1..128");
        bad = good; bad[1] = 129;
        refuse_decl(s, bad, "hint 0: n = 129 is outside 1..128");
        bad = good; bad[2] = 0;
        refuse_decl(s, bad, "hint 0: kz = 0 is outside 1..16");
        bad = good; bad[2] = 17;
        refuse_decl(s, bad, "hint 0: kz = 17 is outside 1..16");
        bad = good; bad[3] = 33;
        refuse_decl(s, bad, "hint 0: kNp = 33 is outside 0..32");
        bad = good; bad[4] = 33;
        refuse_decl(s, bad, "hint 0: kNm = 33 is outside 0..32");
        bad = good; bad[5] = 0;
        refuse_decl(s, bad, "hint 0: kDp = 0 is outside 1..32");
        bad = good; bad[5] = 33;
        refuse_decl(s, bad, "hint 0: kDp = 33 is outside 1..32");
        bad = good; bad[6] = 33;
        refuse_decl(s, bad, "hint 0: kDm = 33 is outside 0..32");
        bad = good; bad[7] = 0;
        refuse_decl(s, bad, "hint 0: kP = 0 is outside 1..16");
        bad = good; bad[7] = 17;
        refuse_decl(s, bad, "hint 0: kP = 17 is outside 1..16");
        bad = good; bad[8] = 2;
        refuse_decl(s, bad, "hint 0: unknown flags 2");
        bad = good; bad[8] = 3;
        refuse_decl(s, bad, "hint 0: unknown flags 3");
        refuse_decl(s, record(128, z, range(20, 9), Nm, Dp, Dm, Pc), "hint 0: n (kNp - 1) = 1024 is 1024 or more");
        refuse_decl(s, record(128, z, Np, range(20, 9), Dp, Dm, Pc), "hint 0: n (kNm - 1) = 1024 is 1024 or more");
        refuse_decl(s, record(128, z, Np, Nm, range(20, 9), Dm, Pc), "hint 0: n (kDp - 1) = 1024 is 1024 or more");
        refuse_decl(s, record(128, z, Np, Nm, Dp, range(20, 9), Pc), "hint 0: n (kDm - 1) = 1024 is 1024 or more");
        check(declare(s, record(93, z, range(20, 12), range(20, 12), range(20, 12), range(20, 12), Pc), &why).size() == 1, "n (k - 1) = 1023 is accepted in all four lists");
        refuse_decl(s, record(128, z, Np, Nm, Dp, Dm, range(20, 5)), "hint 0: n (kP - 1) = 512 is 512 or more");
        check(declare(s, record(73, z, Np, Nm, Dp, Dm, range(20, 8)), &why).size() == 1, "n (kP - 1) = 511 is accepted");
        check(declare(s, record(1, range(40, 16), range(1, 32), range(1, 32), range(1, 32), range(1, 32), range(1, 16)), &why).size() == 1 && why.empty(), "every count at its limit is accepted");
        refuse_decl(s, record(64, z, {1, 61}, Nm, Dp, Dm, Pc), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, record(64, {10, 61}, Np, Nm, Dp, Dm, Pc), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, record(64, z, Np, Nm, Dp, Dm, {7, 61}), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, record(64, {10, 0}, Np, Nm, Dp, Dm, Pc), "hint 0: an output is column 0 (the constant one)");
        refuse_decl(s, record(64, {10, 10}, Np, Nm, Dp, Dm, Pc), "hint 0: output column 10 is named twice");
        refuse_decl(s, record(64, z, Np, {11}, Dp, Dm, Pc), "hint 0: output column 11 is an input of the hint as well");
        refuse_decl(s, record(64, z, Np, Nm, Dp, {10}, Pc), "hint 0: output column 10 is an input of the hint as well");
        refuse_decl(s, record(64, z, Np, Nm, Dp, Dm, {7, 11}), "hint 0: output column 11 is an input of the hint as well");
        std::vector<uint64_t> lit = {3, 0, 0, 0, modulus[0], modulus[1], modulus[2], modulus[3]};
        refuse_decl(s, record(64, z, Np, Nm, Dp, Dm, {}, lit), "hint 0: literal limb 1 is not below r");
        lit[4] -= 1;
        check(declare(s, record(64, z, Np, Nm, Dp, Dm, {}, lit), &why).size() == 1 && why.empty(), "a literal limb equal to r - 1 is accepted");
        // both opcodes in one declaration share the index h and the set of outputs
        const std::vector<uint64_t> ld = longdiv_record(64, {20, 21}, {22}, {1, 2, 3}, {4});
        two = ld;
        two.insert(two.end(), good.begin(), good.end());
        two.insert(two.end(), ld.begin(), ld.end());
        two[two.size() - ld.size() + 7] = 30; two[two.size() - ld.size() + 8] = 31; two[two.size() - ld.size() + 9] = 32;
        got = declare(s, two, &why);
        check(got.size() == 3 && why.empty() && got[0].op == HINT_LONGDIV && got[1].op == HINT_MODDIV && got[2].op == HINT_LONGDIV && got[1].index == 1 && got[2].index == 2 &&
                  got[0].k[2] == 0 && got[2].q == Cols({30, 31}),
              "both opcodes in one declaration, in any mixture, share the index");
        two = ld;
        bad = record(64, {23, 22}, Np, Nm, Dp, Dm, Pc);
        two.insert(two.end(), bad.begin(), bad.end());
        refuse_decl(s, two, "hint 1: output column 22 is an output of hint 0 as well");
        two = good;
        bad = longdiv_record(64, {20}, {11}, {1}, {4});
        two.insert(two.end(), bad.begin(), bad.end());
        refuse_decl(s, two, "hint 1: output column 11 is an output of hint 0 as well");
        two = good;
        bad = good; bad[0] = 2;
        two.insert(two.end(), bad.begin(), bad.end());
        refuse_decl(s, two, "hint 1: unknown opcode 2");
        bad = ld; bad[6] = 2;
        refuse_decl(s, bad, "hint 0: unknown flags 2");

        // the planner: some outputs marked and some given, a special marker on an output, inputs that nothing determines
        const std::vector<Hint> hints = declare(s, good);
        s.add(Row{{F::one(), 40}}, Row{{F::one(), 41}}, Row{{F::one(), 30}});
        Plan p = hinted(s, s.unknown({10, 30}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: some outputs are marked unknown and some are given" && p.steps.empty(), "refused: outputs partly given");
        p = hinted(s, s.unknown({11, 30}, {10}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: an output carries the quotient, indicator or square-root marker" && p.steps.empty(), "refused: the quotient marker on an output");
        for (uint32_t col : {1u, 3u, 5u, 6u, 8u}) {
            Plan q = hinted(s, s.unknown({10, 11, col}), hints);
            const std::string c = std::to_string(col);
            check(q.error == ERR_UNDETERMINED && q.error_col == col && q.message == "hint 0: input column " + c + " is never determined; column " + c + " stays unknown" &&
                      q.steps.empty() && q.hints.empty() && q.launches.empty(),
                  "refused: input column " + c + " (a numerator, denominator or modulus limb) that no row determines");
        }
        {   // inert: the outputs are given, and the plan is the plan without the declaration
            const std::vector<uint8_t> un = s.unknown({30});
            const Plan with = hinted(s, un, hints), without = any_order(s, un);
            check(with.error == OK && same_plan(with, without) && with.hints.empty() && with.launches.size() == 1 && with.launches[0].kind != LAUNCH_MODDIV && with.launches[0].inv_rounds == 0,
                  "inert: the plan without the declaration, field by field");
        }
        check(NUM_KINDS == 7 && NUM_STEP_KINDS == 8 && NUM_SORT_KINDS == 11 && NUM_PLAN_KINDS == 12 && NUM_HINT_KINDS == 13 && KIND_LONGDIV == 11 && KIND_MODDIV == 12 &&
                  HINT_LONGDIV == 1 && HINT_DIVISOR_LITERAL == 1 && HINT_MODDIV == 3 && HINT_MODULUS_LITERAL == 1 && MODDIV_MAX_KZ == 16 && MODDIV_MAX_KP == 16 &&
                  MODDIV_MAX_K == 32 && MODDIV_OPERAND_BITS == 1024 && MODDIV_MODULUS_BITS == 512,
              "the kind numbering, the opcodes and the limits");
    }

    // ---- 3. levels and launches where the two opcodes meet
    void levels_and_launches() {
        const Fr one = F::one();
        {   // 0 one | 1 a, 2 b, 3 e given | 4 d = a b (row 0) | 5 q, 6 rem = divmod(d, e) | 7 Z = rem / q mod 101 | 8 y = Z a (row 1) | 9 Z' = 1 / d mod 101
            // 10 q', 11 rem' = divmod(Z', e)
            System s; s.mw = 11;
            s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 4}});
            s.add(Row{{one, 7}}, Row{{one, 1}}, Row{{one, 8}});
            std::vector<uint64_t> desc = record(64, {7}, {6}, {}, {5}, {}, {}, literal(101)), more = longdiv_record(64, {5}, {6}, {4}, {3});
            desc.insert(desc.end(), more.begin(), more.end());
            more = record(64, {9}, {}, {}, {4}, {}, {}, literal(101));
            desc.insert(desc.end(), more.begin(), more.end());
            more = longdiv_record(64, {10}, {11}, {9}, {3});
            desc.insert(desc.end(), more.begin(), more.end());
            std::string why;
            const std::vector<Hint> hints = declare(s, desc, &why);
            check(hints.size() == 4 && why.empty(), "meeting: four hints of both opcodes are accepted");
            const Plan p = hinted(s, s.unknown({4, 5, 6, 7, 8, 9, 10, 11}), hints);
            // level 1: row 0.  level 2: long division 1 (row 3), then modular 2 (row 4).  level 3: long division 3 (row 5), then modular 0 (row 2).  level 4: row 1
            const uint32_t kinds[6] = {KIND_C, KIND_LONGDIV, KIND_MODDIV, KIND_LONGDIV, KIND_MODDIV, KIND_C}, rows[6] = {0, 3, 4, 5, 2, 1}, lv[6] = {1, 2, 2, 3, 3, 4};
            bool ok = p.error == OK && p.steps.size() == 6 && well_sorted(p) && p.launches.size() == 6;
            for (int t = 0; ok && t < 6; ++t) ok = p.steps[t].kind == kinds[t] && p.steps[t].row == rows[t] && p.steps[t].level == lv[t];
            for (int t = 0; ok && t < 6; ++t) ok = p.launches[t].lo == (uint32_t)t && (p.launches[t].kind == LAUNCH_MODDIV) == (kinds[t] == KIND_MODDIV) && (p.launches[t].kind == LAUNCH_LONGDIV) == (kinds[t] == KIND_LONGDIV);
            check(ok, "meeting: a modular hint waits for a long division's output and the reverse; in a level the long divisions' launch, then the modular one, row = nr + h");
            if (p.error != OK) printf("%s: %s\n", name, p.message.c_str());
            std::vector<Fr> z(12, marker());
            z[0] = one; z[1] = u(6); z[2] = u(7); z[3] = u(5);
            // d = 42; q = 8, rem = 2; Z = 2 / 8 mod 101 = 2 * 38 mod 101 = 76 (8 * 38 = 304 = 3 * 101 + 1); y = 456; Z' = 1 / 42 mod 101 = 89 (42 * 89 = 3738 = 37 * 101 + 1); 89 = 17 * 5 + 4
            check(ok && execute(s, p, z) == NONE && z[4].eq(u(42)) && z[5].eq(u(8)) && z[6].eq(u(2)) && z[7].eq(u(76)) && z[8].eq(u(456)) && z[9].eq(u(89)) && z[10].eq(u(17)) &&
                      z[11].eq(u(4)) && rows_hold(s, z),
                  "meeting: executes to 42 = 8 * 5 + 2, 2 / 8 = 76 and 1 / 42 = 89 (mod 101), 89 = 17 * 5 + 4");
        }
    }

    // ---- 4. a chain of rows and hints: x_{t+1} = c_t / (x_t b) mod 65521, one row (the product) and one hint a step, then a closing sum
    void chain_any_order() {
        const Fr one = F::one();
        const uint32_t steps = 6;
        System s;
        // 0 one | 1 the public sum | 2 x_0, 3 b given | per step t: 4 + 2 t the product, 5 + 2 t x_{t+1}
        s.m0 = 2; s.mw = 2 + 2 * steps;
        std::vector<uint64_t> desc;
        Cols unknown = {1};
        Row total;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t x = t ? 3 + 2 * t : 2, prod = 4 + 2 * t, next = 5 + 2 * t;
            s.add(Row{{one, x}}, Row{{one, 3}}, Row{{one, prod}});
            const std::vector<uint64_t> rec = t & 1 ? record(16, {next}, {x}, {}, {prod}, {}, {}, literal(65521)) : record(16, {next}, {x}, {3}, {prod}, {x}, {}, literal(65521));
            desc.insert(desc.end(), rec.begin(), rec.end());
            unknown.push_back(prod);
            unknown.push_back(next);
            total.push_back({one, next});
        }
        s.add(total, Row{{one, 0}}, Row{{one, 1}});
        const std::vector<Hint> hints = declare(s, desc);
        const std::vector<uint8_t> un = s.unknown(unknown);
        const Plan p = hinted(s, un, hints);
        bool ok = p.error == OK && p.reordered && well_sorted(p) && count_kind(p, KIND_MODDIV) == steps && p.steps.size() == 2 * steps + 1 && p.levels() == 2 * steps + 1;
        for (size_t t = 0; ok && t < p.steps.size(); ++t) ok = p.steps[t].level == t + 1 && (p.steps[t].kind == KIND_MODDIV) == (t % 2 == 1 && t < 2 * steps);
        check(ok, "chain: rows and modular hints alternate over 13 levels");
        const Plan bare = any_order(s, un);
        check(bare.error != OK && bare.steps.empty(), "chain: refused without the declaration");
        const auto start = [&](const System &t) {
            std::vector<Fr> z(t.m0 + t.mw, marker());
            z[0] = one; z[2] = u(12345); z[3] = u(40000);
            return z;
        };
        std::vector<Fr> z = start(s);
        uint64_t x = 12345, sum = 0;
        const auto pw = [](uint64_t a, uint64_t e) { uint64_t v = 1; for (; e; e >>= 1, a = a * a % 65521) if (e & 1) v = v * a % 65521; return v; };
        for (uint32_t t = 0; t < steps; ++t) {
            const uint64_t prod = x * 40000, N = t & 1 ? x : (x + 65521 - 40000 % 65521) % 65521, D = t & 1 ? prod % 65521 : (prod - x) % 65521;
            x = N % 65521 * pw(D, 65519) % 65521;           // 65521 is prime
            sum += x;
        }
        check(ok && execute(s, p, z) == NONE && rows_hold(s, z) && z[1].eq(u(sum)) && z[3 + 2 * steps].eq(u(x)), "chain: executes to the values of a 64-bit computation, and every row holds");
        for (int round = 0; round < 3; ++round) {
            std::vector<uint32_t> order(s.nr());
            for (uint32_t r = 0; r < order.size(); ++r) order[r] = round == 0 ? (uint32_t)order.size() - 1 - r : r;
            for (size_t r = order.size(); round && r > 1; --r) std::swap(order[r - 1], order[next_u64() % r]);
            System t = s.permuted(order);
            const Plan q = hinted(t, un, hints);
            std::vector<Fr> zt = start(t);
            bool equal = q.error == OK && well_sorted(q) && q.levels() == p.levels() && count_kind(q, KIND_MODDIV) == steps && execute(t, q, zt) == NONE && rows_hold(t, zt);
            for (size_t j = 0; equal && j < p.steps.size(); ++j) equal = q.steps[j].level == p.steps[j].level && q.steps[j].kind == p.steps[j].kind && q.steps[j].col == p.steps[j].col;
            for (size_t j = 0; equal && j < z.size(); ++j) equal = zt[j].eq(z[j]);
            check(equal, std::string("chain: ") + (round ? "shuffled" : "reversed") + ", the same levels and the same assignment");
        }
    }

    // ---- 5. stuck under a plan with rows, and two shapes in one launch
    void stuck_word() {
        // 0 one | 1 a, 2 b given | 3 d = a b (row 0) | 4 Z = 1 / d mod P, P = column 5 given | 6 y = 1 / Z by row 1: y * Z = 1
        System s; s.mw = 6;
        const Fr one = F::one();
        s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 3}});
        s.add(Row{{one, 6}}, Row{{one, 4}}, Row{{one, 0}});
        const std::vector<Hint> hints = declare(s, record(64, {4}, {}, {}, {3}, {}, {5}));
        const Plan p = hinted(s, s.unknown({3, 4, 6}), hints);
        check(p.error == OK && p.steps.size() == 3 && p.steps[1].kind == KIND_MODDIV && p.steps[1].row == 2 && p.steps[1].level == 2 && p.steps[2].level == 3,
              "stuck: the hint between two rows, at row nr + 0 = 2 and level 2");
        const uint64_t moduli[4] = {21, 35, 100, 0}, ok_modulus = 55;
        for (uint64_t m : moduli) {
            std::vector<Fr> z(7, marker());
            z[0] = one; z[1] = u(6); z[2] = u(7); z[5] = u(m);
            check(execute(s, p, z) == ((uint64_t)2 << 32 | 2) && z[4].is_zero(),
                  "stuck: P = " + std::to_string(m) + " (D = 0 mod P, a shared factor, or an even P) is reported at the hint, not at the row that then divides by the stored zero");
        }
        std::vector<Fr> z(7, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[5] = u(ok_modulus);
        check(execute(s, p, z) == NONE && z[4].eq(u(38)) && rows_hold(s, z), "stuck: the same plan on P = 55 completes: 42 * 38 = 1596 = 29 * 55 + 1, though 55 is no prime");
    }
    void mixed_launch() {
        // 0 one | 1 .. 4 D of hint 0 (n = 64, P secp256k1's) | 5 .. 8 D of hint 1 (n = 128, P = 2^384 + 5, a literal of four limbs) | 9 .. 12 Z of hint 0 | 13 .. 16 Z of hint 1
        System s; s.mw = 16;
        std::vector<uint64_t> secp, big;
        const uint64_t secp_limbs[4] = {0xFFFFFFFEFFFFFC2Full, ~0ull, ~0ull, ~0ull};
        for (uint64_t v : secp_limbs) { const std::vector<uint64_t> l = literal(v); secp.insert(secp.end(), l.begin(), l.end()); }
        for (uint64_t v : {5ull, 0ull, 0ull, 1ull}) { const std::vector<uint64_t> l = literal(v); big.insert(big.end(), l.begin(), l.end()); }   // 2^384 + 5
        std::vector<uint64_t> desc = record(64, range(9, 4), {}, {}, range(1, 4), {}, {}, secp), second = record(128, range(13, 4), {}, {}, range(5, 4), {}, {}, big);
        desc.insert(desc.end(), second.begin(), second.end());
        const std::vector<Hint> hints = declare(s, desc);
        const Plan p = hinted(s, s.unknown(range(9, 8)), hints);
        check(p.error == OK && p.steps.size() == 2 && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_MODDIV && p.launches[0].rounds == 128 * 3 + 256 && p.launches[0].inv_rounds == 1024 &&
                  p.steps[0].row == 0 && p.steps[1].row == 1,
              "mixed launch: one launch of two shapes, 640 reduction rounds and 2 * 512 inversion rounds (the larger of 448 and 512)");
        std::vector<Fr> z(17, marker());
        z[0] = F::one();
        for (uint32_t j = 1; j <= 8; ++j) z[j] = F::zero();
        z[1] = u(2); z[5] = u(2);
        // 1 / 2 mod P = (P + 1) / 2
        bool ok = p.error == OK && execute(s, p, z) == NONE;
        ok = ok && z[9].eq(u(0xFFFFFFFF7FFFFE18ull)) && z[10].eq(u(~0ull)) && z[11].eq(u(~0ull)) && z[12].eq(u(0x7FFFFFFFFFFFFFFFull));
        ok = ok && z[13].eq(u(3)) && z[14].is_zero() && z[15].eq(F::pow(u(2), 127)) && z[16].is_zero();          // (2^384 + 6) / 2 = 2^383 + 3, and 383 = 2 * 128 + 127
        check(ok, "mixed launch: 1 / 2 modulo both moduli under the same trip counts");
    }

    int run() {
        divisions();
        refusals();
        levels_and_launches();
        chain_any_order();
        stuck_word();
        mixed_launch();
        return report();
    }
};

#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

int main() {
    rng_state = 0x13198A2E03707344ull;
    Suite<pm::BlsCurve> bls("bls12_381", MODDIV_BLS, COUNT(MODDIV_BLS), MODDIV_POOL_BLS);
    Suite<pm::BnCurve> bn("bn254", MODDIV_BN, COUNT(MODDIV_BN), MODDIV_POOL_BN);
    return (bls.run() | bn.run()) ? 1 : 0;
}
