// CPU self-test of the witness solver's declared MODULAR MULTIPLY-DIVIDE hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode
// 7, KIND_MODMULDIV, LAUNCH_MODMULDIV and its two trip counts; polymath_amd/csrc/solve_steps.cuh: shift_up, solve_modmuldiv) on the rig
// of the other solve_*_selftest.cpp programs, with the executor of solve_modmuldiv_exec.hpp.  Stand-alone: g++ -std=c++17, no HIP, no
// GPU; the step body that runs here is the text the kernel k_solve_modmuldiv calls.  Its literals are not committed:
// solve_modmuldiv_cases.hpp is what
//     python tools/gen_solve_modmuldiv_cases.py > DIR/solve_modmuldiv_cases.hpp
// writes, and the program is built with -I DIR (tests/test_native_solve_modmuldiv.py does both).
//   1. cD (D+ - D-) Z = cN (A B + N+ - N-) mod P against literals computed with Python's pow, for P = secp256k1's prime, BLS12-381's q,
//      2^512 - 1, 3 and 65521 * 65519: A, B in {0, 1, P - 1, limbs that carry, sums just below 2^1024}, every combination of empty
//      lists, A = B on the same columns, the three pairs of literals, D+ < D-, the Euclid's worst cases by name, every stuck condition
//      at its boundary and beside it
//   2. every refusal of the record with its text; opcodes 2, 4, 6 and 8 refused; opcode 3 decoded as before; four opcodes in one
//      declaration; an output named by hints of two opcodes; markers 2 to 4 on an output
//   3. the four opcodes meeting in one level: the launches' order and trip counts against a hand-written plan; two shapes in one range
//   4. a chain of rows and hints in matrix order, reversed and shuffled: the same levels and the same assignment
//   5. the stuck word is the root cause under a reordered plan
#include "solve_modmuldiv_exec.hpp"
#include "solve_modmuldiv_cases.hpp"

template <class C>
struct Suite : MulDivRig<C> {
    SOLVE_RIG_NAMES(C)
    typedef MulDivRig<C> Mul;
    using Mul::muldiv_record; using Mul::moddiv_record; using Mul::literal; using Mul::execute_all; using Mul::well_sorted_all;
    const ModMulDivCase *cases;
    size_t n_cases;
    const uint64_t (*pool)[4];
    Suite(const char *n, const ModMulDivCase *c, size_t nc, const uint64_t (*p)[4]) : Mul(n), cases(c), n_cases(nc), pool(p) {}

    // ---- 1. the arithmetic.  A system without rows: columns 1 .. A, B (unless B names A's columns), N+, N-, D+, D-, the modulus (unless
    // it is a literal), Z; the one hint is ready at once
    void arithmetic() {
        for (size_t i = 0; i < n_cases; ++i) {
            const ModMulDivCase &c = cases[i];
            const std::string tag = std::string("modmuldiv ") + c.name;
            System s;
            const uint32_t kP_cols = c.literal ? 0 : c.kP;
            uint32_t k_all = 0, at = 1;
            Cols list[6];
            for (int l = 0; l < 6; ++l) {
                if (l == 1 && c.same) { list[1] = list[0]; continue; }
                list[l] = range(at, c.k[l]);
                at += c.k[l];
                k_all += c.k[l];
            }
            s.mw = k_all + kP_cols + c.kz;
            const Cols Pc = range(1 + k_all, kP_cols), Z = range(1 + k_all + kP_cols, c.kz);
            std::vector<uint64_t> lit;
            for (uint32_t j = 0; c.literal && j < c.kP; ++j) lit.insert(lit.end(), pool[c.at + k_all + j], pool[c.at + k_all + j] + 4);
            std::string why;
            const std::vector<Hint> hints = declare(s, muldiv_record(c.n, Z, list[0], list[1], list[2], list[3], list[4], list[5], Pc, lit, c.cN, c.cD), &why);
            check(why.empty() && hints.size() == 1, tag + ": the declaration is accepted");
            if (hints.size() != 1) { printf("%s: %s\n", name, why.c_str()); continue; }
            const Plan p = hinted(s, s.unknown(Z), hints);
            uint32_t rounds = 0;
            for (uint32_t k : c.k)
                if (k) rounds = std::max(rounds, std::min(1024u, c.n * (k - 1) + 256u));
            const uint32_t L = std::min(512u, c.n * (c.kP - 1) + 256u);
            Step want{0, 0, Z[0], KIND_MODMULDIV, 1};
            check(p.error == OK && p.steps.size() == 1 && same_step(p.steps[0], want) && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_MODMULDIV &&
                      p.launches[0].lo == 0 && p.launches[0].hi == 1 && p.launches[0].rounds == rounds && p.launches[0].inv_rounds == 2 * L && !p.launches[0].divides &&
                      well_sorted_all(p) && p.reordered && p.hints.size() == 1,
                  tag + ": one step of kind KIND_MODMULDIV at level 1, row nr + 0, a launch of its own with both trip counts");
            if (p.error != OK) continue;
            std::vector<Fr> z(s.m0 + s.mw, marker());
            z[0] = F::one();
            for (uint32_t j = 0; j < k_all + kP_cols; ++j) z[1 + j] = from_words(pool[c.at + j]);
            const std::vector<Fr> before = z;
            const uint64_t stuck = execute_all(s, p, z);
            check(c.stuck ? stuck == ((uint64_t)1 << 32 | 0) : stuck == NONE, tag + (c.stuck ? ": stuck at the hint's word" : ": not stuck"));
            bool ok = true;
            for (uint32_t j = 0; j < c.kz; ++j) ok = ok && z[Z[j]].eq(from_words(pool[c.at + k_all + c.kP + j]));
            check(ok, tag + (c.stuck ? ": zero in every output" : ": the limbs of Python's cN (A B + N) pow(cD D, -1, P) mod P"));
            for (uint32_t j = 0; j < 1 + k_all + kP_cols; ++j) ok = ok && z[j].eq(before[j]);
            check(ok, tag + ": no input is written");
        }
    }

    // ---- 2. the declaration
    void refuse_decl(const System &s, const std::vector<uint64_t> &desc, const std::string &text) {
        std::string why;
        const std::vector<Hint> hints = declare(s, desc, &why);
        if (why != text) printf("%s: got \"%s\"\n", name, why.c_str());
        check(why == text && hints.empty(), "refused at the declaration: " + text);
    }
    void declaration() {
        System s; s.mw = 60;
        const Cols z = {10, 11}, A = {1, 2}, B = {3}, Np = {4, 5}, Nm = {6}, Dp = {7, 8}, Dm = {9}, Pc = {12, 13};
        const std::vector<uint64_t> good = muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, Pc, {}, 3, 2);
        std::string why;
        std::vector<Hint> got = declare(s, good, &why);
        bool ok = got.size() == 1 && why.empty() && got[0].op == HINT_MODMULDIV && got[0].n == 64 && got[0].q == z && got[0].rem.empty() &&
                  got[0].D == Cols({1, 2, 3, 4, 5, 6, 7, 8, 9}) && got[0].E == Pc && got[0].lit.empty() && got[0].index == 0 && got[0].c[0] == 3 && got[0].c[1] == 2;
        const uint32_t km[6] = {2, 1, 2, 1, 2, 1};
        for (int i = 0; ok && i < 6; ++i) ok = got[0].km[i] == km[i];
        for (int i = 0; ok && i < 4; ++i) ok = got[0].k[i] == 0;
        check(ok, "a good record is accepted, field by field");
        got = declare(s, muldiv_record(64, z, A, A, {}, {}, {}, {}, {}, {3, 0, 0, 0, 1, 0, 0, 0}), &why);
        check(got.size() == 1 && why.empty() && got[0].flags == HINT_MODULUS_LITERAL && got[0].E.empty() && got[0].lit.size() == 8 && got[0].D == Cols({1, 2, 1, 2}) && got[0].c[0] == 1 && got[0].c[1] == 1,
              "a multiply modulo a literal, A and B on the same columns, no other list, is accepted");
        std::vector<uint64_t> bad, two;
        for (uint64_t op : {2, 4, 6, 8}) {
            bad = good; bad[0] = op;
            refuse_decl(s, bad, "hint 0: unknown opcode " + std::to_string(op));
        }
        bad = good; bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        refuse_decl(s, {HINT_MODMULDIV, 64, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1}, "hint 0: the record is truncated");
        two = good;
        two.insert(two.end(), good.begin(), good.begin() + 15);                  // a second record that ends inside its columns
        refuse_decl(s, two, "hint 1: the record is truncated");
        bad = muldiv_record(64, z, A, B, {}, {}, {}, {}, {}, {3, 0, 0, 0}); bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        const auto with = [&](size_t at, uint64_t v) { std::vector<uint64_t> w = good; w[at] = v; return w; };
        refuse_decl(s, with(1, 0), "hint 0: n = 0 is outside 1..128");
        refuse_decl(s, with(1, 129), "hint 0: n = 129 is outside 1..128");
        refuse_decl(s, with(2, 0), "hint 0: kz = 0 is outside 1..16");
        refuse_decl(s, with(2, 17), "hint 0: kz = 17 is outside 1..16");
        refuse_decl(s, with(3, 0), "hint 0: kA = 0 is outside 1..32");
        refuse_decl(s, with(3, 33), "hint 0: kA = 33 is outside 1..32");
        refuse_decl(s, with(4, 0), "hint 0: kB = 0 is outside 1..32");
        refuse_decl(s, with(4, 33), "hint 0: kB = 33 is outside 1..32");
        refuse_decl(s, with(5, 33), "hint 0: kNp = 33 is outside 0..32");
        refuse_decl(s, with(6, 33), "hint 0: kNm = 33 is outside 0..32");
        refuse_decl(s, with(7, 33), "hint 0: kDp = 33 is outside 0..32");
        refuse_decl(s, with(8, 33), "hint 0: kDm = 33 is outside 0..32");
        refuse_decl(s, with(7, 0), "hint 0: kDm = 1 with kDp = 0");
        check(declare(s, muldiv_record(64, z, A, B, Np, Nm, Dp, {}, Pc), &why).size() == 1 && why.empty(), "kDm = 0 with kDp > 0 is accepted");
        refuse_decl(s, with(9, 0), "hint 0: kP = 0 is outside 1..16");
        refuse_decl(s, with(9, 17), "hint 0: kP = 17 is outside 1..16");
        refuse_decl(s, with(10, 2), "hint 0: unknown flags 2");
        refuse_decl(s, with(10, 3), "hint 0: unknown flags 3");
        refuse_decl(s, with(11, 0), "hint 0: cN = 0 is outside 1..4294967295");
        refuse_decl(s, with(11, 4294967296ull), "hint 0: cN = 4294967296 is outside 1..4294967295");
        refuse_decl(s, with(12, 0), "hint 0: cD = 0 is outside 1..4294967295");
        refuse_decl(s, with(12, 4294967296ull), "hint 0: cD = 4294967296 is outside 1..4294967295");
        got = declare(s, muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, Pc, {}, 4294967295ull, 4294967295ull), &why);
        check(got.size() == 1 && why.empty() && got[0].c[0] == 0xffffffffu && got[0].c[1] == 0xffffffffu, "cN = cD = 2^32 - 1 is accepted");
        const Cols nine = range(20, 9);
        static const char *const names[6] = {"kA", "kB", "kNp", "kNm", "kDp", "kDm"};
        for (int l = 0; l < 6; ++l) {
            const Cols *lists[6] = {&A, &B, &Np, &Nm, &Dp, &Dm};
            lists[l] = &nine;
            refuse_decl(s, muldiv_record(128, z, *lists[0], *lists[1], *lists[2], *lists[3], *lists[4], *lists[5], Pc), std::string("hint 0: n (") + names[l] + " - 1) = 1024 is 1024 or more");
        }
        const Cols twelve = range(20, 12);
        check(declare(s, muldiv_record(93, z, twelve, twelve, twelve, twelve, twelve, twelve, Pc), &why).size() == 1, "n (k - 1) = 1023 is accepted in all six lists");
        refuse_decl(s, muldiv_record(128, z, A, B, Np, Nm, Dp, Dm, range(20, 5)), "hint 0: n (kP - 1) = 512 is 512 or more");
        check(declare(s, muldiv_record(73, z, A, B, Np, Nm, Dp, Dm, range(20, 8)), &why).size() == 1, "n (kP - 1) = 511 is accepted");
        check(declare(s, muldiv_record(1, range(40, 16), range(1, 32), range(1, 32), range(1, 32), range(1, 32), range(1, 32), range(1, 32), range(1, 16)), &why).size() == 1 && why.empty(),
              "every count at its limit is accepted");
        refuse_decl(s, muldiv_record(64, z, {1, 61}, B, Np, Nm, Dp, Dm, Pc), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, muldiv_record(64, {10, 61}, A, B, Np, Nm, Dp, Dm, Pc), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, {12, 61}), "hint 0: column 61 is not below m0 + mw = 61");
        refuse_decl(s, muldiv_record(64, {10, 0}, A, B, Np, Nm, Dp, Dm, Pc), "hint 0: an output is column 0 (the constant one)");
        refuse_decl(s, muldiv_record(64, {10, 10}, A, B, Np, Nm, Dp, Dm, Pc), "hint 0: output column 10 is named twice");
        refuse_decl(s, muldiv_record(64, z, {1, 11}, B, Np, Nm, Dp, Dm, Pc), "hint 0: output column 11 is an input of the hint as well");
        refuse_decl(s, muldiv_record(64, z, A, {10}, Np, Nm, Dp, Dm, Pc), "hint 0: output column 10 is an input of the hint as well");
        refuse_decl(s, muldiv_record(64, z, A, B, Np, Nm, Dp, {10}, Pc), "hint 0: output column 10 is an input of the hint as well");
        refuse_decl(s, muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, {12, 11}), "hint 0: output column 11 is an input of the hint as well");
        std::vector<uint64_t> lit = {3, 0, 0, 0, modulus[0], modulus[1], modulus[2], modulus[3]};
        refuse_decl(s, muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, {}, lit), "hint 0: literal limb 1 is not below r");
        lit[4] -= 1;
        check(declare(s, muldiv_record(64, z, A, B, Np, Nm, Dp, Dm, {}, lit), &why).size() == 1 && why.empty(), "a literal limb equal to r - 1 is accepted");

        // opcode 3 is decoded as it was: the same fields from the same words, and nothing of the new record in them
        const std::vector<uint64_t> md = moddiv_record(64, {20, 21}, {1, 2}, {3}, {4, 5}, {6}, {7, 8});
        const uint64_t md_words[] = {3, 64, 2, 2, 1, 2, 1, 2, 0, 20, 21, 1, 2, 3, 4, 5, 6, 7, 8};
        got = declare(s, md, &why);
        check(md == std::vector<uint64_t>(md_words, md_words + 19) && got.size() == 1 && why.empty() && got[0].op == HINT_MODDIV && got[0].q == Cols({20, 21}) &&
                  got[0].D == Cols({1, 2, 3, 4, 5, 6}) && got[0].E == Cols({7, 8}) && got[0].k[0] == 2 && got[0].k[1] == 1 && got[0].k[2] == 2 && got[0].k[3] == 1 &&
                  got[0].km[0] == 0 && got[0].km[5] == 0 && got[0].c[0] == 1 && got[0].c[1] == 1,
              "opcode 3: the words and the decoded record are what they were");
        bad = md; bad[5] = 0;
        refuse_decl(s, bad, "hint 0: kDp = 0 is outside 1..32");
        // four opcodes in one declaration share the index h and the set of outputs
        const std::vector<uint64_t> ld = longdiv_record(64, {30, 31}, {32}, {1, 2, 3}, {4}), wd = longdiv_record(64, {33, 34}, {35}, {1, 2, 3}, {4}, {}, HINT_LONGDIV_WIDE);
        two = ld;
        for (const std::vector<uint64_t> *more : {&good, &md, &wd}) two.insert(two.end(), more->begin(), more->end());
        got = declare(s, two, &why);
        check(got.size() == 4 && why.empty() && got[0].op == HINT_LONGDIV && got[1].op == HINT_MODMULDIV && got[2].op == HINT_MODDIV && got[3].op == HINT_LONGDIV_WIDE &&
                  got[1].index == 1 && got[2].index == 2 && got[3].index == 3 && got[0].km[0] == 0 && got[3].q == Cols({33, 34}),
              "four opcodes in one declaration, in any mixture, share the index");
        // an output named by hints of two opcodes, each of the three others against the new one, in both orders
        for (const std::vector<uint64_t> *other : {&ld, &md, &wd}) {
            const uint64_t col = (*other)[0] == HINT_MODDIV ? 21 : (*other)[0] == HINT_LONGDIV ? 32 : 35;
            const std::vector<uint64_t> clash = muldiv_record(64, {10, (uint32_t)col}, A, B, Np, Nm, Dp, Dm, Pc);
            two = *other;
            two.insert(two.end(), clash.begin(), clash.end());
            refuse_decl(s, two, "hint 1: output column " + std::to_string(col) + " is an output of hint 0 as well");
            two = clash;
            two.insert(two.end(), other->begin(), other->end());
            refuse_decl(s, two, "hint 1: output column " + std::to_string(col) + " is an output of hint 0 as well");
        }
        two = good;
        bad = good; bad[0] = 6;
        two.insert(two.end(), bad.begin(), bad.end());
        refuse_decl(s, two, "hint 1: unknown opcode 6");

        // the planner: some outputs marked and some given, markers 2 to 4 on an output, inputs that nothing determines
        const std::vector<Hint> hints = declare(s, good);
        s.add(Row{{F::one(), 40}}, Row{{F::one(), 41}}, Row{{F::one(), 30}});
        Plan p = hinted(s, s.unknown({10, 30}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: some outputs are marked unknown and some are given" && p.steps.empty(), "refused: outputs partly given");
        for (uint8_t byte : {PATTERN_QUOTIENT, PATTERN_INDICATOR, PATTERN_SQRT}) {
            std::vector<uint8_t> un = s.unknown({11, 30});
            un[10] = byte;
            p = hinted(s, un, hints);
            check(p.error == ERR_HINT && p.message == "hint 0: an output carries the quotient, indicator or square-root marker" && p.steps.empty(),
                  "refused: marker " + std::to_string(byte) + " on an output");
        }
        for (uint32_t col : {1u, 3u, 5u, 6u, 8u, 9u}) {
            Plan q = hinted(s, s.unknown({10, 11, col}), hints);
            const std::string c = std::to_string(col);
            check(q.error == ERR_UNDETERMINED && q.error_col == col && q.message == "hint 0: input column " + c + " is never determined; column " + c + " stays unknown" &&
                      q.steps.empty() && q.hints.empty() && q.launches.empty(),
                  "refused: input column " + c + " (a factor, addend or denominator limb) that no row determines");
        }
        {   // inert: the outputs are given, and the plan is the plan without the declaration
            const std::vector<uint8_t> un = s.unknown({30});
            const Plan with_hint = hinted(s, un, hints), without = any_order(s, un);
            check(with_hint.error == OK && same_plan(with_hint, without) && with_hint.hints.empty() && with_hint.launches.size() == 1 && with_hint.launches[0].kind != LAUNCH_MODMULDIV &&
                      with_hint.launches[0].inv_rounds == 0,
                  "inert: the plan without the declaration, field by field");
        }
        check(NUM_KINDS == 7 && NUM_STEP_KINDS == 8 && NUM_SORT_KINDS == 11 && NUM_PLAN_KINDS == 12 && NUM_HINT_KINDS == 13 && NUM_WIDE_KINDS == 14 && NUM_MULDIV_KINDS == 15 &&
                  KIND_LONGDIV == 11 && KIND_MODDIV == 12 && KIND_LONGDIV_WIDE == 13 && KIND_MODMULDIV == 14 && LAUNCH_MODMULDIV == LAUNCH_LONGDIV_WIDE + 1 && HINT_LONGDIV == 1 &&
                  HINT_MODDIV == 3 && HINT_LONGDIV_WIDE == 5 && HINT_MODMULDIV == 7 && HINT_MODULUS_LITERAL == 1 && MODMULDIV_MAX_C == 0xffffffffull && MODMULDIV_LISTS == 6 &&
                  MODDIV_MAX_KZ == 16 && MODDIV_MAX_KP == 16 && MODDIV_MAX_K == 32 && MODDIV_OPERAND_BITS == 1024 && MODDIV_MODULUS_BITS == 512 &&
                  KIND_INFO[KIND_MODMULDIV].launch == LAUNCH_MODMULDIV && !KIND_INFO[KIND_MODMULDIV].divides && !KIND_INFO[KIND_MODMULDIV].chained,
              "the kind numbering, the opcodes, the limits and the table's new row");
    }

    // ---- 3. levels and launches where the four opcodes meet
    void levels_and_launches() {
        const Fr one = F::one();
        {   // 0 one | 1 a, 2 b, 3 e given | 4 d = a b (row 0) | level 2, all from d: 5 q, 6 rem = divmod(d, e) (opcode 1) | 7 Z = 1 / d mod 101 (opcode 3)
            // 8 q', 9 rem' = divmod(d, e) (opcode 5) | 10 W = 3 d d / (2 a) mod 101 (opcode 7) | 11 y = W a (row 1) | 12 V = (W rem + q) mod 101 (opcode 7, level 3)
            System s; s.mw = 12;
            s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 4}});
            s.add(Row{{one, 10}}, Row{{one, 1}}, Row{{one, 11}});
            std::vector<uint64_t> desc = muldiv_record(64, {12}, {10}, {6}, {5}, {}, {}, {}, {}, literal(101));
            for (const std::vector<uint64_t> &more : {muldiv_record(64, {10}, {4}, {4}, {}, {}, {1}, {}, {}, literal(101), 3, 2), longdiv_record(64, {8}, {9}, {4}, {3}, {}, HINT_LONGDIV_WIDE),
                                                      moddiv_record(64, {7}, {}, {}, {4}, {}, {}, literal(101)), longdiv_record(64, {5}, {6}, {4}, {3})})
                desc.insert(desc.end(), more.begin(), more.end());
            std::string why;
            const std::vector<Hint> hints = declare(s, desc, &why);
            check(hints.size() == 5 && why.empty(), "meeting: five hints of four opcodes are accepted");
            const Plan p = hinted(s, s.unknown(range(4, 9)), hints);
            // nr = 2.  level 1: row 0.  level 2: long division 4 (row 6), modular 3 (row 5), wide 2 (row 4), multiply-divide 1 (row 3).  level 3: row 1, then multiply-divide 0 (row 2)
            const uint32_t kinds[7] = {KIND_C, KIND_LONGDIV, KIND_MODDIV, KIND_LONGDIV_WIDE, KIND_MODMULDIV, KIND_C, KIND_MODMULDIV}, rows[7] = {0, 6, 5, 4, 3, 1, 2},
                           lv[7] = {1, 2, 2, 2, 2, 3, 3};
            const uint8_t launch[7] = {LAUNCH_CHAIN, LAUNCH_LONGDIV, LAUNCH_MODDIV, LAUNCH_LONGDIV_WIDE, LAUNCH_MODMULDIV, LAUNCH_CHAIN, LAUNCH_MODMULDIV};
            const uint32_t rounds[7] = {0, 256, 256, 256, 256, 0, 256}, inv_rounds[7] = {0, 0, 512, 0, 512, 0, 512};
            bool ok = p.error == OK && p.steps.size() == 7 && well_sorted_all(p) && p.launches.size() == 7 && p.reordered;
            for (int t = 0; ok && t < 7; ++t) ok = p.steps[t].kind == kinds[t] && p.steps[t].row == rows[t] && p.steps[t].level == lv[t];
            for (int t = 0; ok && t < 7; ++t)
                ok = same_launch(p.launches[t], Launch{(uint32_t)t, (uint32_t)t + 1, launch[t], 0, rounds[t], inv_rounds[t]});
            check(ok, "meeting: in a level the long divisions' launch, the modular one, the wide one, then the multiply-divides; row = nr + h; every launch against a hand-written plan");
            if (p.error != OK) printf("%s: %s\n", name, p.message.c_str());
            std::vector<Fr> z(13, marker());
            z[0] = one; z[1] = u(6); z[2] = u(7); z[3] = u(5);
            // d = 42; q = 8, rem = 2; Z = 1 / 42 mod 101 = 89; W = 3 * 42 * 42 / 12 mod 101 = 441 mod 101 = 37; y = 222; V = (37 * 2 + 8) mod 101 = 82
            check(ok && execute_all(s, p, z) == NONE && z[4].eq(u(42)) && z[5].eq(u(8)) && z[6].eq(u(2)) && z[7].eq(u(89)) && z[8].eq(u(8)) && z[9].eq(u(2)) && z[10].eq(u(37)) &&
                      z[11].eq(u(222)) && z[12].eq(u(82)) && rows_hold(s, z),
                  "meeting: executes to 42 = 8 * 5 + 2, 1 / 42 = 89, 3 * 42^2 / 12 = 37 and 37 * 2 + 8 = 82 (mod 101)");
        }
        {   // two shapes in one range: the larger trip counts.  0 one | 1 .. 4 X of hint 0 (n = 64, P secp256k1's) | 5 .. 8 X of hint 1 (n = 128, P = 2^384 + 5) | 9 .. 12, 13 .. 16 Z
            System s; s.mw = 16;
            std::vector<uint64_t> secp, big;
            const uint64_t secp_limbs[4] = {0xFFFFFFFEFFFFFC2Full, ~0ull, ~0ull, ~0ull};
            for (uint64_t v : secp_limbs) { const std::vector<uint64_t> l = literal(v); secp.insert(secp.end(), l.begin(), l.end()); }
            for (uint64_t v : {5ull, 0ull, 0ull, 1ull}) { const std::vector<uint64_t> l = literal(v); big.insert(big.end(), l.begin(), l.end()); }   // 2^384 + 5
            std::vector<uint64_t> desc = muldiv_record(64, range(9, 4), range(1, 4), range(1, 4), {}, {}, {}, {}, {}, secp, 1, 2),
                                  second = muldiv_record(128, range(13, 4), range(5, 4), range(5, 4), {}, {}, {}, {}, {}, big, 1, 2);
            desc.insert(desc.end(), second.begin(), second.end());
            const std::vector<Hint> hints = declare(s, desc);
            const Plan p = hinted(s, s.unknown(range(9, 8)), hints);
            check(p.error == OK && p.steps.size() == 2 && p.launches.size() == 1 && same_launch(p.launches[0], Launch{0, 2, LAUNCH_MODMULDIV, 0, 128 * 3 + 256, 1024}) &&
                      p.steps[0].row == 0 && p.steps[1].row == 1 && well_sorted_all(p),
                  "mixed launch: one launch of two shapes, 640 reduction rounds and 2 * 512 rounds for the product and the inversion (the larger of 448 and 512)");
            std::vector<Fr> z(17, marker());
            z[0] = F::one();
            for (uint32_t j = 1; j <= 8; ++j) z[j] = F::zero();
            z[1] = u(1); z[5] = u(1);
            // 1 * 1 / 2 mod P = (P + 1) / 2
            bool ok = p.error == OK && execute_all(s, p, z) == NONE;
            ok = ok && z[9].eq(u(0xFFFFFFFF7FFFFE18ull)) && z[10].eq(u(~0ull)) && z[11].eq(u(~0ull)) && z[12].eq(u(0x7FFFFFFFFFFFFFFFull));
            ok = ok && z[13].eq(u(3)) && z[14].is_zero() && z[15].eq(F::pow(u(2), 127)) && z[16].is_zero();          // (2^384 + 6) / 2 = 2^383 + 3, and 383 = 2 * 128 + 127
            check(ok, "mixed launch: 1 / 2 modulo both moduli under the same trip counts");
        }
    }

    // ---- 4. a chain of rows and hints: x_{t+1} = 3 x_t^2 / (2 p_t) mod 65521 with p_t = x_t b, one row and one hint a step, then a closing sum
    void chain_any_order() {
        const Fr one = F::one();
        const uint32_t steps = 6;
        const uint64_t Q = 65521;
        System s;
        // 0 one | 1 the public sum | 2 x_0, 3 b given | per step t: 4 + 2 t the product, 5 + 2 t x_{t+1}
        s.m0 = 2; s.mw = 2 + 2 * steps;
        std::vector<uint64_t> desc;
        Cols unknown = {1};
        Row total;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t x = t ? 3 + 2 * t : 2, prod = 4 + 2 * t, next = 5 + 2 * t;
            s.add(Row{{one, x}}, Row{{one, 3}}, Row{{one, prod}});
            const std::vector<uint64_t> rec = t & 1 ? muldiv_record(16, {next}, {x}, {x}, {}, {}, {prod}, {}, {}, literal(Q), 3, 2) : muldiv_record(16, {next}, {x}, {3}, {prod}, {x}, {prod}, {3}, {}, literal(Q));
            desc.insert(desc.end(), rec.begin(), rec.end());
            unknown.push_back(prod);
            unknown.push_back(next);
            total.push_back({one, next});
        }
        s.add(total, Row{{one, 0}}, Row{{one, 1}});
        const std::vector<Hint> hints = declare(s, desc);
        const std::vector<uint8_t> un = s.unknown(unknown);
        const Plan p = hinted(s, un, hints);
        bool ok = p.error == OK && p.reordered && well_sorted_all(p) && count_kind(p, KIND_MODMULDIV) == steps && p.steps.size() == 2 * steps + 1 && p.levels() == 2 * steps + 1;
        for (size_t t = 0; ok && t < p.steps.size(); ++t) ok = p.steps[t].level == t + 1 && (p.steps[t].kind == KIND_MODMULDIV) == (t % 2 == 1 && t < 2 * steps);
        check(ok, "chain: rows and multiply-divide hints alternate over 13 levels");
        const Plan bare = any_order(s, un);
        check(bare.error != OK && bare.steps.empty(), "chain: refused without the declaration");
        const auto start = [&](const System &t) {
            std::vector<Fr> z(t.m0 + t.mw, marker());
            z[0] = one; z[2] = u(12345); z[3] = u(40000);
            return z;
        };
        std::vector<Fr> z = start(s);
        uint64_t x = 12345, sum = 0;
        const auto pw = [&](uint64_t a, uint64_t e) { uint64_t v = 1; for (a %= Q; e; e >>= 1, a = a * a % Q) if (e & 1) v = v * a % Q; return v; };
        for (uint32_t t = 0; t < steps; ++t) {
            const uint64_t prod = x * 40000;
            const uint64_t N = t & 1 ? 3 * (x * x % Q) % Q : (x * 40000 % Q + prod % Q + Q - x % Q) % Q, D = t & 1 ? 2 * (prod % Q) % Q : (prod % Q + Q - 40000 % Q) % Q;
            x = N * pw(D, Q - 2) % Q;           // 65521 is prime
            sum += x;
        }
        check(ok && execute_all(s, p, z) == NONE && rows_hold(s, z) && z[1].eq(u(sum)) && z[3 + 2 * steps].eq(u(x)), "chain: executes to the values of a 64-bit computation, and every row holds");
        for (int round = 0; round < 3; ++round) {
            std::vector<uint32_t> order(s.nr());
            for (uint32_t r = 0; r < order.size(); ++r) order[r] = round == 0 ? (uint32_t)order.size() - 1 - r : r;
            for (size_t r = order.size(); round && r > 1; --r) std::swap(order[r - 1], order[next_u64() % r]);
            System t = s.permuted(order);
            const Plan q = hinted(t, un, hints);
            std::vector<Fr> zt = start(t);
            bool equal = q.error == OK && well_sorted_all(q) && q.levels() == p.levels() && count_kind(q, KIND_MODMULDIV) == steps && execute_all(t, q, zt) == NONE && rows_hold(t, zt);
            for (size_t j = 0; equal && j < p.steps.size(); ++j) equal = q.steps[j].level == p.steps[j].level && q.steps[j].kind == p.steps[j].kind && q.steps[j].col == p.steps[j].col;
            for (size_t j = 0; equal && j < z.size(); ++j) equal = zt[j].eq(z[j]);
            check(equal, std::string("chain: ") + (round ? "shuffled" : "reversed") + ", the same levels and the same assignment");
        }
    }

    // ---- 5. the stuck word is the root cause under a reordered plan
    void stuck_word() {
        // 0 one | 1 a, 2 b given | 3 d = a b (row 0) | 4 Z = a b / d mod P, P = column 5 given | 6 y = 1 / Z by row 1: y * Z = 1
        System s; s.mw = 6;
        const Fr one = F::one();
        s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 3}});
        s.add(Row{{one, 6}}, Row{{one, 4}}, Row{{one, 0}});
        const std::vector<Hint> hints = declare(s, muldiv_record(64, {4}, {1}, {2}, {}, {}, {3}, {}, {5}, {}, 5, 1));
        for (int reversed = 0; reversed < 2; ++reversed) {
            System t = reversed ? s.permuted({1, 0}) : s.permuted({0, 1});
            const Plan p = hinted(t, t.unknown({3, 4, 6}), hints);
            check(p.error == OK && p.steps.size() == 3 && p.steps[1].kind == KIND_MODMULDIV && p.steps[1].row == 2 && p.steps[1].level == 2 && p.steps[2].level == 3,
                  "stuck: the hint between two rows, at row nr + 0 = 2 and level 2");
            const uint64_t moduli[4] = {21, 35, 100, 0};
            for (uint64_t m : moduli) {
                std::vector<Fr> z(7, marker());
                std::vector<uint32_t> rows;
                z[0] = one; z[1] = u(6); z[2] = u(7); z[5] = u(m);
                check(execute_all(t, p, z, &rows) == ((uint64_t)2 << 32 | 2) && z[4].is_zero() && rows.size() == 2 && rows[0] == 2,
                      "stuck: P = " + std::to_string(m) + " (D = 0 mod P, a shared factor, or an even P) is reported at the hint, the root cause, not at the row that then divides by the stored zero");
            }
            std::vector<Fr> z(7, marker());
            z[0] = one; z[1] = u(6); z[2] = u(7); z[5] = u(55);
            check(execute_all(t, p, z) == NONE && z[4].eq(u(5)) && rows_hold(t, z), "stuck: the same plan on P = 55 completes: 5 * 42 / 42 = 5, though 55 is no prime");
        }
    }

    int run() {
        arithmetic();
        declaration();
        levels_and_launches();
        chain_any_order();
        stuck_word();
        return report();
    }
};

#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381", MODMULDIV_BLS, COUNT(MODMULDIV_BLS), MODMULDIV_POOL_BLS);
    Suite<pm::BnCurve> bn("bn254", MODMULDIV_BN, COUNT(MODMULDIV_BN), MODMULDIV_POOL_BN);
    return (bls.run() | bn.run()) ? 1 : 0;
}
