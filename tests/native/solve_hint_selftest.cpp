// CPU self-test of the witness solver's DECLARED HINTS (polymath_amd/host/solve_plan.hpp: decode_hints, Planner::hint_step, the
// hint-owned columns of the scheduler, KIND_LONGDIV, LAUNCH_LONGDIV; polymath_amd/csrc/solve_steps.cuh: add_shifted, limb_at, longdiv,
// solve_longdiv) on the rig of the other solve_*_selftest.cpp programs.  Stand-alone: g++ -std=c++17, no HIP, no GPU; the step body
// that runs here is the text the kernel k_solve_longdiv calls.  Its literals are not committed: solve_hint_cases.hpp is what
//     python tools/gen_solve_hint_cases.py > DIR/solve_hint_cases.hpp
// writes, and the program is built with -I DIR (tests/test_native_solve_hint.py does both).
//   1. long divisions against literals computed with Python integers (solve_hint_cases.hpp):
//      D = 0, D < E, E = 1, D = 2^1024 - 1, E = 2^512 - 1, D = E, n = 1, 32, 64, 86, 128, limbs that are not normalised and carry
//      across several limbs, a limb equal to r - 1, a literal divisor, and each of the five stuck conditions at its boundary and one below
//   2. every refusal of the declaration and of the planner, with its text
//   3. an inert hint: the plan is, field by field, the plan without the declaration
//   4. a hint that waits for a linear block and whose outputs wake decompositions; rows in order, reversed and shuffled plan to the
//      same levels and execute to the same assignment
//   5. LimbModMul and ModMulChain (polymath_amd/circuits.py), built here row by row, executed to (a b) mod p and x_0 b^t mod p
#include "solve_selftest.hpp"
#include "solve_hint_cases.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    const LongdivCase *cases;
    size_t n_cases;
    const uint64_t (*pool)[4];
    const ModMulCase *muls;
    size_t n_muls;
    const uint64_t (*mul_pool)[4];
    Suite(const char *n, const LongdivCase *c, size_t nc, const uint64_t (*p)[4], const ModMulCase *m, size_t nm, const uint64_t (*mp)[4])
        : Rig(n), cases(c), n_cases(nc), pool(p), muls(m), n_muls(nm), mul_pool(mp) {}

    static std::vector<uint32_t> levels(const System &s, const Plan &p) {
        std::vector<uint32_t> lv = column_levels(s, p);
        for (const Step &st : p.steps) {
            if (st.kind == KIND_BLOCK)
                for (uint32_t col : p.blocks[st.cols_off].cols) lv[col] = st.level;
            if (st.kind == KIND_LONGDIV)
                for (const std::vector<uint32_t> *out : {&p.hints[st.cols_off].q, &p.hints[st.cols_off].rem})
                    for (uint32_t col : *out) lv[col] = st.level;
        }
        return lv;
    }

    // ---- 1. long divisions against Python's divmod.  A system without rows: columns 1 .. the dividend, the divisor (unless it is a
    // literal), the quotient, the remainder; the one hint is ready at once
    void divisions() {
        for (size_t i = 0; i < n_cases; ++i) {
            const LongdivCase &c = cases[i];
            const std::string tag = std::string("longdiv ") + c.name;
            System s;
            const uint32_t kE_cols = c.literal ? 0 : c.kE;
            s.mw = c.kD + kE_cols + c.kq + c.kr;
            const std::vector<uint32_t> D = range(1, c.kD), E = range(1 + c.kD, kE_cols), q = range(1 + c.kD + kE_cols, c.kq), rem = range(1 + c.kD + kE_cols + c.kq, c.kr);
            std::vector<uint64_t> lit;
            for (uint32_t j = 0; c.literal && j < c.kE; ++j) lit.insert(lit.end(), pool[c.at + c.kD + j], pool[c.at + c.kD + j] + 4);
            std::string why;
            const std::vector<Hint> hints = declare(s, longdiv_record(c.n, q, rem, D, E, lit), &why);
            check(why.empty() && hints.size() == 1, tag + ": the declaration is accepted");
            if (hints.size() != 1) continue;
            std::vector<uint32_t> outs(q);
            outs.insert(outs.end(), rem.begin(), rem.end());
            const Plan p = hinted(s, s.unknown(outs), hints);
            Step want{0, 0, q[0], KIND_LONGDIV, 1};
            check(p.error == OK && p.steps.size() == 1 && same_step(p.steps[0], want) && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_LONGDIV && p.launches[0].lo == 0 &&
                      p.launches[0].hi == 1 && p.launches[0].rounds == std::min(1024u, c.n * (c.kD - 1) + 256u) && well_sorted(p) && p.reordered && p.hints.size() == 1,
                  tag + ": one step of kind KIND_LONGDIV at level 1, row nr + 0, a launch of its own");
            if (p.error != OK) continue;
            std::vector<Fr> z(s.m0 + s.mw, marker());
            z[0] = F::one();
            for (uint32_t j = 0; j < c.kD; ++j) z[D[j]] = from_words(pool[c.at + j]);
            for (uint32_t j = 0; j < kE_cols; ++j) z[E[j]] = from_words(pool[c.at + c.kD + j]);
            const uint64_t stuck = execute(s, p, z);
            check(c.stuck ? stuck == ((uint64_t)1 << 32 | 0) : stuck == NONE, tag + (c.stuck ? ": stuck at the hint's word" : ": not stuck"));
            bool ok = true;
            for (uint32_t j = 0; j < c.kq; ++j) ok = ok && z[q[j]].eq(from_words(pool[c.at + c.kD + c.kE + j]));
            for (uint32_t j = 0; j < c.kr; ++j) ok = ok && z[rem[j]].eq(from_words(pool[c.at + c.kD + c.kE + c.kq + j]));
            check(ok, tag + (c.stuck ? ": zero in every output" : ": the limbs of Python's divmod"));
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
        System s; s.mw = 40;
        const std::vector<uint32_t> q = {10, 11}, rem = {12, 13}, D = {1, 2, 3}, E = {4, 5};
        const std::vector<uint64_t> good = longdiv_record(64, q, rem, D, E);
        std::string why;
        check(declare(s, good, &why).size() == 1 && why.empty(), "a good record is accepted");
        check(declare(s, {}, &why).empty() && why.empty(), "no words: no hints and no refusal");
        std::vector<uint64_t> two = good, bad;
        bad = good; bad[0] = 2;
        refuse_decl(s, bad, "hint 0: unknown opcode 2");
        bad = good; bad.pop_back();
        refuse_decl(s, bad, "hint 0: the record is truncated");
        refuse_decl(s, {HINT_LONGDIV, 64, 1}, "hint 0: the record is truncated");
        two.insert(two.end(), good.begin(), good.begin() + 9);                  // a second record that ends inside its columns
        refuse_decl(s, two, "hint 1: the record is truncated");
        bad = good; bad[1] = 0;
        refuse_decl(s, bad, "hint 0: n = 0 is outside 1..128");
        bad = good; bad[1] = 129;
        refuse_decl(s, bad, "hint 0: n = 129 is outside 1..128");
        bad = good; bad[2] = 0;
        refuse_decl(s, bad, "hint 0: kq = 0 is outside 1..32");
        bad = good; bad[2] = 33;
        refuse_decl(s, bad, "hint 0: kq = 33 is outside 1..32");
        bad = good; bad[3] = 0;
        refuse_decl(s, bad, "hint 0: kr = 0 is outside 1..16");
        bad = good; bad[3] = 17;
        refuse_decl(s, bad, "hint 0: kr = 17 is outside 1..16");
        bad = good; bad[4] = 0;
        refuse_decl(s, bad, "hint 0: kD = 0 is outside 1..32");
        bad = good; bad[4] = 33;
        refuse_decl(s, bad, "hint 0: kD = 33 is outside 1..32");
        bad = good; bad[5] = 0;
        refuse_decl(s, bad, "hint 0: kE = 0 is outside 1..16");
        bad = good; bad[5] = 17;
        refuse_decl(s, bad, "hint 0: kE = 17 is outside 1..16");
        bad = good; bad[6] = 2;
        refuse_decl(s, bad, "hint 0: unknown flags 2");
        refuse_decl(s, longdiv_record(128, q, rem, range(1, 9), E), "hint 0: n (kD - 1) = 1024 is 1024 or more");
        check(declare(s, longdiv_record(93, q, rem, range(14, 12), E), &why).size() == 1, "n (kD - 1) = 1023 is accepted");
        refuse_decl(s, longdiv_record(128, q, rem, D, range(14, 5)), "hint 0: n (kE - 1) = 512 is 512 or more");
        check(declare(s, longdiv_record(73, q, rem, D, range(14, 8)), &why).size() == 1, "n (kE - 1) = 511 is accepted");
        refuse_decl(s, longdiv_record(64, q, rem, {1, 2, 41}, E), "hint 0: column 41 is not below m0 + mw = 41");
        refuse_decl(s, longdiv_record(64, {10, 41}, rem, D, E), "hint 0: column 41 is not below m0 + mw = 41");
        refuse_decl(s, longdiv_record(64, {10, 0}, rem, D, E), "hint 0: an output is column 0 (the constant one)");
        refuse_decl(s, longdiv_record(64, q, {12, 10}, D, E), "hint 0: output column 10 is named twice");
        refuse_decl(s, longdiv_record(64, q, rem, {1, 12, 3}, E), "hint 0: output column 12 is an input of the hint as well");
        refuse_decl(s, longdiv_record(64, q, rem, D, {4, 11}), "hint 0: output column 11 is an input of the hint as well");
        two = good;
        bad = longdiv_record(64, {20, 21}, {22, 13}, D, E);
        two.insert(two.end(), bad.begin(), bad.end());
        refuse_decl(s, two, "hint 1: output column 13 is an output of hint 0 as well");
        std::vector<uint64_t> lit = {1, 0, 0, 0, modulus[0], modulus[1], modulus[2], modulus[3]};
        refuse_decl(s, longdiv_record(64, q, rem, D, {}, lit), "hint 0: literal limb 1 is not below r");
        lit[4] -= 1;
        check(declare(s, longdiv_record(64, q, rem, D, {}, lit), &why).size() == 1 && why.empty(), "a literal limb equal to r - 1 is accepted");
        // a hint may read the output of another hint
        two = good;
        bad = longdiv_record(64, {20}, {22}, {10, 12}, E);
        two.insert(two.end(), bad.begin(), bad.end());
        check(declare(s, two, &why).size() == 2 && why.empty(), "the output of one hint as the input of another is accepted");

        // the planner: some outputs marked and some given, a special marker on an output, an input that nothing determines
        const std::vector<Hint> hints = declare(s, good);
        s.add(Row{{F::one(), 1}}, Row{{F::one(), 2}}, Row{{F::one(), 30}});
        Plan p = hinted(s, s.unknown({10, 11, 12, 30}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: some outputs are marked unknown and some are given" && p.steps.empty(), "refused: outputs partly given");
        p = hinted(s, s.unknown({11, 12, 13, 30}, {10}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: an output carries the quotient, indicator or square-root marker" && p.steps.empty(), "refused: the quotient marker on an output");
        p = hinted(s, s.unknown({10, 11, 12, 30}, {}, {13}), hints);
        check(p.error == ERR_HINT && p.message == "hint 0: an output carries the quotient, indicator or square-root marker", "refused: the indicator marker on an output");
        p = hinted(s, s.unknown({10, 11, 12, 13, 30, 5}), hints);
        check(p.error == ERR_UNDETERMINED && p.error_col == 5 && p.message == "hint 0: input column 5 is never determined; column 5 stays unknown" && p.steps.empty() &&
                  p.hints.empty() && p.launches.empty(),
              "refused: an input that no row determines, and the undetermined-column text after it");
        {   // column 0 marked: the refusal it always was
            std::vector<uint8_t> un = s.unknown({10, 11, 12, 13});
            un[0] = 1;
            p = hinted(s, un, hints);
            check(p.error == ERR_COLUMN_ZERO, "refused: column 0 marked, as without a declaration");
        }
        check(NUM_KINDS == 7 && NUM_STEP_KINDS == 8 && NUM_SORT_KINDS == 11 && NUM_PLAN_KINDS == 12 && KIND_LONGDIV == 11 && HINT_LONGDIV == 1 && HINT_DIVISOR_LITERAL == 1,
              "the kind numbering and the opcode");
    }

    // ---- the modular multiplication of polymath_amd/circuits.py (_PartialModMul), row by row.  -> the remainder's columns
    struct Gadget {
        uint32_t n, l;
        std::vector<Fr> p;               // the modulus' limbs (a literal)
        std::vector<uint64_t> p_words;
        std::vector<uint32_t> p_cols;    // not empty: the modulus in witness columns
        bool decompose = true;
        uint32_t next = 2;               // m0 = 2: the one and the public sum
        std::vector<uint32_t> unknown;
        std::vector<uint64_t> desc;
        std::vector<uint32_t> P_cols, q_cols, rem_cols, bit_cols, carry_cols;     // of the last multiplication
        std::vector<uint32_t> take(uint32_t k, bool given = false) {
            std::vector<uint32_t> v = range(next, k);
            next += k;
            if (!given) unknown.insert(unknown.end(), v.begin(), v.end());
            return v;
        }
    };
    static void product_rows(System &s, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, const std::vector<uint32_t> &p) {
        for (uint32_t c = 1; c <= p.size(); ++c) {
            const auto at = [&](const std::vector<uint32_t> &cols) {
                Row row;
                Fr pw = F::one();
                for (uint32_t i = 0; i < cols.size(); ++i, pw = F::mul(pw, u(c))) row.push_back({pw, cols[i]});
                return row;
            };
            s.add(at(a), at(b), at(p));
        }
    }
    static std::vector<uint32_t> modmul(System &s, Gadget &g, const std::vector<uint32_t> &x, const std::vector<uint32_t> &y) {
        const Fr one = F::one(), m1 = F::neg(one);
        const Row by_one = {{one, 0}};
        const uint32_t l = g.l;
        const std::vector<uint32_t> Pc = g.take(2 * l - 1), q = g.take(l), rem = g.take(l);
        product_rows(s, x, y, Pc);
        const std::vector<uint64_t> rec = longdiv_record(g.n, q, rem, Pc, g.p_cols, g.p_cols.empty() ? g.p_words : std::vector<uint64_t>{});
        g.desc.insert(g.desc.end(), rec.begin(), rec.end());
        g.bit_cols.clear();
        for (uint32_t i = 0; g.decompose && i < 2 * l; ++i) {
            const std::vector<uint32_t> bits = g.take(g.n);
            Row sum;
            Fr pw = one;
            for (uint32_t k = 0; k < g.n; ++k, pw = F::add(pw, pw)) {
                s.boolean(bits[k]);
                sum.push_back({pw, bits[k]});
            }
            s.add(Row{{one, i < l ? q[i] : rem[i - l]}}, by_one, sum);
            g.bit_cols.insert(g.bit_cols.end(), bits.begin(), bits.end());
        }
        const std::vector<uint32_t> qp = g.take(2 * l - 1);
        if (g.p_cols.empty()) {
            for (uint32_t j = 0; j < 2 * l - 1; ++j) {
                Row lc;
                for (uint32_t i = 0; i < l; ++i)
                    if (j >= i && j - i < l && !g.p[j - i].is_zero()) lc.push_back({g.p[j - i], q[i]});
                s.add(lc, by_one, Row{{one, qp[j]}});
            }
        } else {
            product_rows(s, q, g.p_cols, qp);
        }
        const std::vector<uint32_t> carries = g.take(2 * l - 2);
        const Fr two_n = F::pow(u(2), g.n);
        for (uint32_t j = 0; j < 2 * l - 1; ++j) {
            Row lc = {{one, Pc[j]}, {m1, qp[j]}};
            if (j < l) lc.push_back({m1, rem[j]});
            if (j) lc.push_back({one, carries[j - 1]});
            s.add(lc, by_one, j < 2 * l - 2 ? Row{{two_n, carries[j]}} : Row{});
        }
        g.P_cols = Pc; g.q_cols = q; g.rem_cols = rem; g.carry_cols = carries;
        return rem;
    }
    // the limbs' sum and the public sum, as the generators close a circuit
    static void close(System &s, Gadget &g, const std::vector<std::vector<uint32_t>> &rems) {
        const Fr one = F::one();
        Row total;
        for (const auto &rem : rems) {
            const uint32_t sum = g.take(1)[0];
            Row lc;
            for (uint32_t col : rem) lc.push_back({one, col});
            s.add(lc, Row{{one, 0}}, Row{{one, sum}});
            total.push_back({one, sum});
        }
        s.add(total, Row{{one, 0}}, Row{{one, 1}});
        g.unknown.push_back(1);
        s.m0 = 2;
        s.mw = g.next - 2;
    }
    Gadget gadget(const ModMulCase &c) {
        Gadget g;
        g.n = c.n; g.l = c.l;
        for (uint32_t i = 0; i < c.l; ++i) {
            g.p.push_back(from_words(mul_pool[c.at + i]));
            g.p_words.insert(g.p_words.end(), mul_pool[c.at + i], mul_pool[c.at + i] + 4);
        }
        return g;
    }
    std::vector<Fr> start(const System &s, const Gadget &g, const ModMulCase &c, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) {
        std::vector<Fr> z(s.m0 + s.mw, F::zero());
        z[0] = F::one();
        for (uint32_t col : g.unknown) z[col] = marker();
        for (uint32_t i = 0; i < c.l; ++i) {
            z[a[i]] = from_words(mul_pool[c.at + c.l + i]);
            z[b[i]] = from_words(mul_pool[c.at + 2 * c.l + i]);
            if (!g.p_cols.empty()) z[g.p_cols[i]] = g.p[i];
        }
        return z;
    }
    bool rem_is(const std::vector<Fr> &z, const std::vector<uint32_t> &rem, const ModMulCase &c) {
        bool ok = true;
        for (uint32_t i = 0; i < c.l; ++i) ok = ok && z[rem[i]].eq(from_words(mul_pool[c.at + 3 * c.l + i]));
        return ok;
    }

    // ---- 3, 4, 5. the gadgets
    void gadgets() {
        for (size_t i = 0; i < n_muls; ++i) {
            const ModMulCase &c = muls[i];
            for (int witness_modulus = 0; witness_modulus < (c.steps ? 2 : 1); ++witness_modulus) {
                const std::string tag = (c.steps ? "ModMulChain " : "LimbModMul ") + std::to_string(c.n) + " x " + std::to_string(c.l) + (witness_modulus ? ", the modulus a witness" : "") + " #" + std::to_string(i);
                System s;
                Gadget g = gadget(c);
                const std::vector<uint32_t> a = g.take(c.l, true), b = g.take(c.l, true);
                if (witness_modulus) g.p_cols = g.take(c.l, true);
                std::vector<uint32_t> x = a;
                std::vector<std::vector<uint32_t>> rems;
                for (uint32_t t = 0; t < (c.steps ? c.steps : 1); ++t) {
                    x = modmul(s, g, x, b);
                    rems.push_back(x);
                }
                close(s, g, rems);
                std::string why;
                const std::vector<Hint> hints = declare(s, g.desc, &why);
                check(why.empty() && hints.size() == rems.size(), tag + ": the declaration is accepted");
                const std::vector<uint8_t> unknown = s.unknown(g.unknown);
                const Plan p = hinted(s, unknown, hints);
                check(p.error == OK && p.reordered && well_sorted(p) && count_kind(p, KIND_LONGDIV) == rems.size() && p.hints.size() == rems.size(), tag + ": plans, a step per hint");
                if (p.error != OK) { printf("%s: %s\n", name, p.message.c_str()); continue; }
                // without the declaration the system is refused: nothing determines q and rem
                const Plan bare = any_order(s, unknown);
                check(bare.error != OK && bare.steps.empty(), tag + ": refused without the declaration");
                // the hint waits for the block of the product, and its outputs wake the decompositions, qp and the carries
                const std::vector<uint32_t> lv = levels(s, p);
                bool ok = true;
                for (uint32_t col : g.q_cols) ok = ok && lv[col] == lv[g.P_cols[0]] + 1;
                for (uint32_t col : g.rem_cols) ok = ok && lv[col] == lv[g.P_cols[0]] + 1;
                for (uint32_t col : g.P_cols) ok = ok && lv[col] == lv[g.P_cols[0]];
                for (uint32_t col : g.bit_cols) ok = ok && lv[col] == lv[g.q_cols[0]] + 1;
                for (size_t j = 0; j < g.carry_cols.size(); ++j) ok = ok && lv[g.carry_cols[j]] == lv[g.q_cols[0]] + 2 + j;
                check(ok && lv[g.P_cols[0]] >= 1, tag + ": the block, then the hint, then the decompositions beside q p, then the carries one by one");
                std::vector<Fr> z = start(s, g, c, a, b);
                const uint64_t stuck = execute(s, p, z);
                check(stuck == NONE && rem_is(z, x, c) && rows_hold(s, z), tag + ": executes to Python's (a b) mod p, and every row holds");
                // rows reversed and shuffled: the same levels and the same assignment
                for (int round = 0; round < 3; ++round) {
                    std::vector<uint32_t> order(s.nr());
                    for (uint32_t r = 0; r < order.size(); ++r) order[r] = round == 0 ? (uint32_t)order.size() - 1 - r : r;
                    for (size_t r = order.size(); round && r > 1; --r) std::swap(order[r - 1], order[next_u64() % r]);
                    System t = s.permuted(order);
                    const Plan q = hinted(t, unknown, hints);
                    std::vector<Fr> zt = start(t, g, c, a, b);
                    // (the levels may differ: the closing check row, examined early, determines the last carry before the carry rows reach it)
                    const std::vector<uint32_t> lt = levels(t, q);
                    bool equal = q.error == OK && well_sorted(q) && execute(t, q, zt) == NONE && rows_hold(t, zt);
                    for (uint32_t col : g.q_cols) equal = equal && lt[col] == lt[g.P_cols[0]] + 1;
                    for (size_t j = 0; equal && j < z.size(); ++j) equal = zt[j].eq(z[j]);
                    check(equal, tag + (round ? ": shuffled, the same assignment" : ": reversed, the same assignment"));
                }
                if (i == 0) inert_and_supplied(s, g, hints, unknown, z, tag);
            }
        }
    }
    // an inert hint: the caller supplies q and rem, and the plan is the plan without the declaration, field by field
    void inert_and_supplied(System &s, const Gadget &g, const std::vector<Hint> &hints, const std::vector<uint8_t> &unknown, const std::vector<Fr> &solved, const std::string &tag) {
        std::vector<uint8_t> given = unknown;
        for (uint32_t col : g.q_cols) given[col] = 0;
        for (uint32_t col : g.rem_cols) given[col] = 0;
        const Plan with = hinted(s, given, hints), without = any_order(s, given);
        bool ok = with.error == OK && same_plan(with, without) && with.hints.empty() && without.hints.empty() && with.blocks.size() == without.blocks.size() &&
                  with.block_mats.size() == without.block_mats.size();
        for (size_t i = 0; ok && i < with.launches.size(); ++i) ok = (with.launches[i].kind == LAUNCH_BLOCK) == (without.launches[i].kind == LAUNCH_BLOCK) && (with.launches[i].kind == LAUNCH_SQRT) == (without.launches[i].kind == LAUNCH_SQRT) && with.launches[i].kind != LAUNCH_LONGDIV;
        for (size_t i = 0; ok && i < with.blocks.size(); ++i) ok = with.blocks[i].rows == without.blocks[i].rows && with.blocks[i].cols == without.blocks[i].cols && with.blocks[i].mat == without.blocks[i].mat;
        check(ok, tag + ": inert, the plan without the declaration field by field");
        std::vector<Fr> z = solved;
        for (size_t j = 0; j < given.size(); ++j)
            if (given[j]) z[j] = marker();
        check(with.error == OK && execute(s, with, z) == NONE && rows_hold(s, z), tag + ": a caller that supplies q and rem itself");
    }

    // ---- 6. stuck under a plan with rows: the hint's word is nr + h at its level, and the root cause wins
    void stuck_word() {
        // 0 one | 1 a, 2 b given | 3 d = a b (row 0) | 4 q, 5 rem = divmod(d, E), E = column 6 given | 7 y = 1 / rem by row 1: y * rem = 1
        System s; s.mw = 7;
        const Fr one = F::one();
        s.add(Row{{one, 1}}, Row{{one, 2}}, Row{{one, 3}});
        s.add(Row{{one, 7}}, Row{{one, 5}}, Row{{one, 0}});
        const std::vector<Hint> hints = declare(s, longdiv_record(64, {4}, {5}, {3}, {6}));
        const Plan p = hinted(s, s.unknown({3, 4, 5, 7}), hints);
        check(p.error == OK && p.steps.size() == 3 && p.steps[1].kind == KIND_LONGDIV && p.steps[1].row == 2 && p.steps[1].level == 2 && p.steps[2].level == 3,
              "stuck: the hint between two rows, at row nr + 0 = 2 and level 2");
        std::vector<Fr> z(8, marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[6] = F::zero();
        check(execute(s, p, z) == ((uint64_t)2 << 32 | 2) && z[4].is_zero() && z[5].is_zero(), "stuck: a zero divisor is reported at the hint, not at the row that then divides by the stored zero");
        std::fill(z.begin(), z.end(), marker());
        z[0] = one; z[1] = u(6); z[2] = u(7); z[6] = u(5);
        check(execute(s, p, z) == NONE && z[4].eq(u(8)) && z[5].eq(u(2)) && rows_hold(s, z), "stuck: the same plan on a good divisor completes: 42 = 8 * 5 + 2");
    }

    // ---- 7. two hints of different sizes in one launch: the trip count is the larger bound, and the smaller dividend divides under it
    void mixed_launch() {
        // 0 one | 1, 2 D of hint 0 (n = 64) | 3 E of both | 4 .. 7 D of hint 1 (n = 128) | 8, 9 q and 10 rem of hint 0 | 11 q and 12 rem of hint 1
        System s; s.mw = 12;
        std::vector<uint64_t> desc = longdiv_record(64, {8, 9}, {10}, {1, 2}, {3}), second = longdiv_record(128, {11}, {12}, {4, 5, 6, 7}, {3});
        desc.insert(desc.end(), second.begin(), second.end());
        const std::vector<Hint> hints = declare(s, desc);
        const Plan p = hinted(s, s.unknown({8, 9, 10, 11, 12}), hints);
        check(p.error == OK && p.steps.size() == 2 && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_LONGDIV && p.launches[0].rounds == 128 * 3 + 256 && p.steps[0].row == 0 &&
                  p.steps[1].row == 1,
              "mixed launch: one launch of two hints, 640 rounds (64 + 256 and 384 + 256)");
        std::vector<Fr> z(13, marker());
        z[0] = F::one(); z[1] = u(7); z[2] = u(1); z[3] = u(5); z[4] = u(9); z[5] = z[6] = z[7] = F::zero();
        const unsigned __int128 D = ((unsigned __int128)1 << 64) + 7, q = D / 5;
        check(p.error == OK && execute(s, p, z) == NONE && z[8].eq(u((uint64_t)q)) && z[9].eq(u((uint64_t)(q >> 64))) && z[10].eq(u((uint64_t)(D % 5))) && z[11].eq(u(1)) &&
                  z[12].eq(u(4)),
              "mixed launch: (2^64 + 7) / 5 and 9 / 5 under the same trip count");
    }

    int run() {
        mixed_launch();
        divisions();
        refusals();
        gadgets();
        stuck_word();
        return report();
    }
};

#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

int main() {
    rng_state = 0x243F6A8885A308D3ull;
    Suite<pm::BlsCurve> bls("bls12_381", LONGDIV_BLS, COUNT(LONGDIV_BLS), LONGDIV_POOL_BLS, MODMUL_BLS, COUNT(MODMUL_BLS), MODMUL_POOL_BLS);
    Suite<pm::BnCurve> bn("bn254", LONGDIV_BN, COUNT(LONGDIV_BN), LONGDIV_POOL_BN, MODMUL_BN, COUNT(MODMUL_BN), MODMUL_POOL_BN);
    return (bls.run() | bn.run()) ? 1 : 0;
}
