// The witness solver's division rows (polymath_amd/host/solve_plan.hpp: division_row, KIND_DIVREM; polymath_amd/csrc/divrem.cuh:
// marker_byte, divrem256, euclid_divrem) on the CPU.  The accepted shapes against hand-written plans; every refusal with its row and
// the row's earlier message as a prefix; a byte-2 column that an ordinary row solves; two assignments that mark one column with
// different markers; a division row beside an is-zero pair over the same known side; a corpus (one wide level of range-checked
// divisions, a chain of modular steps, the mixed system) on which build_plan_any_order equals build_plan field by field in matrix
// order and which, reversed and under seeded permutations, plans with every column at its in-order level and EXECUTES -- serially,
// with the host field type and the routine the kernels call -- to the in-order assignment; and the edge operands on both moduli
// against divmod values written out as literals.  Built and run by tests/test_native_solve_divrem.py.
// Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include "solve_selftest.hpp"

// a, d, floor(a / d), a mod d as 64 hexadecimal digits, most significant first: Python's divmod on the canonical integers
struct Literal { const char *a, *d, *q, *rem; };
static const Literal BLS_CASES[] = {
    // d = 1:  a = 0, d, r - 1
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000", "0000000000000000000000000000000000000000000000000000000000000001",
     "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    // d = r - 1:  a = 0, d - 1, d = r - 1
    {"0000000000000000000000000000000000000000000000000000000000000000", "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"73eda753299d7d483339d80809a1d80553bda402fffe5bfefffffffeffffffff", "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "73eda753299d7d483339d80809a1d80553bda402fffe5bfefffffffeffffffff"},
    {"73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000", "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    // d = 2^64 (the quotient crosses a word boundary):  a = 0, d - 1, d, r - 1
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"000000000000000000000000000000000000000000000000ffffffffffffffff", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "000000000000000000000000000000000000000000000000ffffffffffffffff"},
    {"0000000000000000000000000000000000000000000000010000000000000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "000000000000000073eda753299d7d483339d80809a1d80553bda402fffe5bfe", "000000000000000000000000000000000000000000000000ffffffff00000000"},
    // d = 2^192 + 1 (the remainder crosses a word boundary):  a = 0, d - 1, d, r - 1
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000001000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000000"},
    {"0000000000000001000000000000000000000000000000000000000000000001", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "00000000000000000000000000000000000000000000000073eda753299d7d48", "00000000000000003339d80809a1d80553bda402fffe5bfe8c1258abd66282b8"},
    // random operands of mixed sizes
    {"6bb6a198f1446beab0c11fdecb91ce375bc8fbbcbde5c0994164d8399f767c45", "000000000000000000000000000000000000000000000000000000003b9985ed",
     "00000001cea9f736860d80f97187b596628dbaf1ee088238f46622181d242c02", "0000000000000000000000000000000000000000000000000000000016eab46b"},
    {"0e7d887b2827688de6a16a3b0d464138a62332553fc1ea36f17fd374c6a53877", "000000000000005d478c281d687c966c377b9aa2bb2edb20035b73993fd42359",
     "0000000000000000000000000000000000000000000000000027c497e8013c6c", "00000000000000352027406331a9e18187325aa8d2abd6394ea1a67c558472eb"},
    {"09350f24cc11d357c30d8b7628dbd25e63b229f1c4069545de11cc9dea959c21", "000000000000000000000000000000000000000471e0c07e9e115e4b9e30691c",
     "00000000000000000000000002124aa82106ad5a021d8df7e79210e0a7d39ca3", "0000000000000000000000000000000000000001386a46faf021ff1acba19f4d"},
    {"1b94e30cc60a3cab359eeefb015c33b2df1461aaf8eb18b90074513021da8978", "000000000000000000000000000000000000000a4a0fe75d2a9eba0cdf561d80",
     "00000000000000000000000002ae3c4c7e4a387ca6fc97da85c284861e565cce", "00000000000000000000000000000000000000092b25e3d47e156b2e8ef4cc78"},
};
static const Literal BN_CASES[] = {
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", "0000000000000000000000000000000000000000000000000000000000000001",
     "30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000000000000000000000000000000000000000000000000000000", "30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"30644e72e131a029b85045b68181585d2833e84879b9709143e1f593efffffff", "30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "30644e72e131a029b85045b68181585d2833e84879b9709143e1f593efffffff"},
    {"30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", "30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"000000000000000000000000000000000000000000000000ffffffffffffffff", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000000", "000000000000000000000000000000000000000000000000ffffffffffffffff"},
    {"0000000000000000000000000000000000000000000000010000000000000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", "0000000000000000000000000000000000000000000000010000000000000000",
     "000000000000000030644e72e131a029b85045b68181585d2833e84879b97091", "00000000000000000000000000000000000000000000000043e1f593f0000000"},
    {"0000000000000000000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"0000000000000001000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000000", "0000000000000001000000000000000000000000000000000000000000000000"},
    {"0000000000000001000000000000000000000000000000000000000000000001", "0000000000000001000000000000000000000000000000000000000000000001",
     "0000000000000000000000000000000000000000000000000000000000000001", "0000000000000000000000000000000000000000000000000000000000000000"},
    {"30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", "0000000000000001000000000000000000000000000000000000000000000001",
     "00000000000000000000000000000000000000000000000030644e72e131a029", "0000000000000000b85045b68181585d2833e84879b97091137da7210ece5fd7"},
    {"0ba0759b346c6e2ba02fdaa1ad864c44e049548e8a0a8c9632ea6928f6236bf2", "000000000000000000000000000000000000000ce4cc4132f7108e96f770c226",
     "00000000000000000000000000e6d86439d844b88a7d15c593555e65a1883b6f", "000000000000000000000000000000000000000509a4c07e40a9dfada5507b78"},
    {"10e24b7f254cb864ef901b932a7c18806a3753915c76f18a0585a01c4c7d6df0", "000000000000000000000000000000000000000000000000000000002a7a3534",
     "0000000065c1569f807f2f6d1deb6dd55ce9a812b718b75972f0316a0bf97514", "00000000000000000000000000000000000000000000000000000000250c81e0"},
    {"2d4a90eaad8d194a9892139600ddb74d960d5a8f9a656aafd14125844d25deb3", "000000000000001d2d1634b4b465325278f845f57b3120df2f4d4c8650d7d13f",
     "000000000000000000000000000000000000000000000000018d66306624c373", "0000000000000006d53d2c09da2a6305d53598dff3c6f5f4c49ac41110f3e266"},
    {"250673d360597bdc5dbe44096b384309c9a937a68c8f95ef04a012e8677fd139", "0000000000000000000000000000000000000000000000000000000039f61468",
     "00000000a387e5f41d9f8fec159fc53453a4c0cd1910fbbd3b155de9fee3bd0a", "000000000000000000000000000000000000000000000000000000002e9a3d29"},
};
static constexpr size_t N_CASES = sizeof(BLS_CASES) / sizeof(BLS_CASES[0]);
static_assert(sizeof(BN_CASES) / sizeof(BN_CASES[0]) == N_CASES, "the same cases on both moduli");

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    const Literal *literals;

    Suite(const char *n, const Literal *lit) : Rig(n), literals(lit) {}
    static Fr from_hex(const char *hex) {      // 64 digits, most significant first -> Montgomery form
        Fr v;
        for (int i = 0; i < 8; ++i) {
            char word[9] = {0};
            memcpy(word, hex + 8 * (7 - i), 8);
            v.l[i] = (uint32_t)strtoul(word, nullptr, 16);
        }
        return pm::to_mont<P>(v);
    }

    // ---- 1. the accepted shapes, against plans written by hand.  0 one | 1 a, 2 b given | 3 q, 4 rem
    //   cq q * (b + 2) = cq a - cq rem  (or with an empty rest: = -cq rem, so a = 0), q in A or in B
    void shapes() {
        const Fr one = F::one();
        for (int q_in_b = 0; q_in_b < 2; ++q_in_b)
            for (uint64_t cq : {1ull, 7ull})
                for (int rest = 0; rest < 2; ++rest) {
                    const std::string tag = std::string("shapes: q in ") + (q_in_b ? "B" : "A") + ", cq = " + std::to_string(cq) + (rest ? ", a rest" : ", no rest");
                    System s; s.mw = 4;
                    const Row lone = {{u(cq), 3}}, K = {{u(2), 0}, {one, 2}};
                    Row c;
                    if (rest) c.push_back({u(cq), 1});
                    c.push_back({F::neg(u(cq)), 4});
                    s.add(q_in_b ? K : lone, q_in_b ? lone : K, c);
                    const std::vector<uint8_t> unknown = s.unknown({4}, {3});
                    for (uint32_t wide : {WIDE_STEPS, 1u}) {
                        const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                        bool ok = p.error == OK && p.message.empty() && p.steps.size() == 1 && p.divs.size() == 1 && p.pairs.empty() && p.bit_cols.empty() && !p.reordered;
                        if (ok) {
                            const Step want{0, 0, 3, KIND_DIVREM, 1};
                            ok = same_step(p.steps[0], want) && p.divs[0].pos_r == (uint64_t)rest && p.divs[0].col_r == 4 && p.divs[0].q_in_b == q_in_b &&
                                 p.level_ptr == std::vector<uint32_t>({0, 1}) && p.launches.size() == 1 &&
                                 same_launch(p.launches[0], wide == 1 ? Launch{0, 1, LAUNCH_DIVREM, 1} : Launch{0, 1, LAUNCH_CHAIN, 1});
                        }
                        check(ok, tag + ": the plan is the hand-written one");
                        check(same_plan(p, q), tag + ": the any-order builder gives the same plan");
                        if (!ok) continue;
                        std::vector<Fr> z = {one, u(100), u(5), quotient_marker(), marker()};
                        check(execute(s, p, z) == NONE && z[3].eq(u(rest ? 14 : 0)) && z[4].eq(u(rest ? 2 : 0)) && rows_hold(s, z), tag + ": 100 = 14 * 7 + 2");
                    }
                    check(in_order(s, unknown, WIDE_STEPS, false).error == ERR_MANY_UNKNOWNS, tag + ": without the modulus the rule is off");
                }
    }

    // ---- 2. every refusal: ERR_MANY_UNKNOWNS at the row, the row's earlier message, then the condition.  Row 0 is a check row, so
    //   that the refused row is row 1.  0 one | 1 a, 2 b given | 3 q, 4 rem, 5 x
    void refusals() {
        const Fr one = F::one(), m1 = F::neg(one);
        struct Bad { const char *why; Row a, b, c; std::vector<uint32_t> plain; bool opener_shape; int bare = ERR_MANY_UNKNOWNS; };
        const Row lone = {{one, 3}}, K = {{one, 2}};
        const std::vector<Bad> bad = {
            {"cr != -cq", lone, K, Row{{one, 1}, {one, 4}}, {4}, true},
            {"cr != -cq", K, Row{{u(7), 3}}, Row{{one, 1}, {m1, 4}}, {4}, true},
            {"rem in A or B", lone, Row{{one, 2}, {one, 4}}, Row{{one, 1}, {m1, 4}}, {4}, false},
            {"rem in A or B", lone, Row{{one, 4}}, Row{{one, 1}}, {4}, false},
            {"rem named twice", lone, K, Row{{m1, 4}, {one, 1}, {m1, 4}}, {4}, false},
            {"the other side not known", lone, Row{{one, 2}, {one, 5}}, Row{{one, 1}, {m1, 4}}, {4, 5}, false},
            {"the other side not known", lone, Row{}, Row{{one, 1}, {m1, 4}}, {4}, false},
            {"the other side not known", lone, Row{{F::zero(), 2}}, Row{{one, 1}, {m1, 4}}, {4}, false},
            {"the quotient named twice", lone, K, Row{{one, 3}, {m1, 4}}, {4}, false, ERR_TWO_MATRICES},      // without the rule the second entry decides
            {"a third unknown", lone, K, Row{{one, 5}, {m1, 4}}, {4, 5}, false},
        };
        for (const Bad &b : bad) {
            const std::string tag = std::string("refusals: ") + b.why;
            System s; s.mw = 5;
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(b.a, b.b, b.c);
            const std::vector<uint8_t> unknown = s.unknown(b.plain, {3});
            std::vector<uint32_t> all = b.plain;
            all.push_back(3);
            const Plan p = in_order(s, unknown), bare = in_order(s, unknown, WIDE_STEPS, false), before = in_order(s, s.unknown(all, {})), q = any_order(s, unknown);
            const std::string suffix = std::string(", and no division row: ") + b.why;
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.steps.empty() && p.divs.empty() && p.launches.empty(), tag + ": refused at row 1");
            check(bare.error == b.bare && bare.error_row == 1 && !bare.message.empty() && (b.bare != ERR_MANY_UNKNOWNS || (p.message.find(bare.message) == 0 && p.error_col == bare.error_col)) &&
                      p.message.size() >= suffix.size() && p.message.compare(p.message.size() - suffix.size(), suffix.size(), suffix) == 0,
                  tag + ": the row's message without the rule, then the condition");
            if (b.opener_shape)      // with the plain marker the row is an opener that nothing closes
                check(before.error == ERR_MANY_UNKNOWNS && before.message.find("no is-zero pair") != std::string::npos && p.message == bare.message + suffix &&
                          p.message.find("is-zero") == std::string::npos,
                      tag + ": never registered as an opener");
            else
                check(before.error == ERR_MANY_UNKNOWNS && before.error_row == 1 && p.message == before.message + suffix, tag + ": the message the row has with the plain marker, then the condition");
            check(q.error == ERR_MANY_UNKNOWNS && q.error_row == 1 && q.error_col == p.error_col && q.message.find(p.message + "; in any row order: ") == 0 && q.steps.empty(),
                  tag + ": in any order the same refusal");
        }
    }

    // ---- 3. byte 2 has meaning in the division row only.  0 one | 1 x given | 2 q, 3 w
    void marker_elsewhere() {
        const Fr one = F::one();
        {   // the single unknown of an ordinary row, in C and as the lone entry of A
            System s; s.mw = 3;
            s.add(Row{{one, 1}, {one, 0}}, Row{{one, 1}}, Row{{u(2), 2}});
            s.add(Row{{u(3), 3}}, Row{{one, 1}}, Row{{one, 2}});
            const Plan p = in_order(s, s.unknown({}, {2, 3})), plain = in_order(s, s.unknown({2, 3}, {}));
            check(p.error == OK && p.steps.size() == 2 && p.steps[0].kind == KIND_C && p.steps[0].col == 2 && p.steps[1].kind == KIND_A && p.steps[1].col == 3 && p.divs.empty() &&
                      same_plan(p, plain),
                  "marker elsewhere: a byte-2 column that is the single unknown of an ordinary row is solved by that row");
            const Fr x = rnd();
            std::vector<Fr> z = {one, x, quotient_marker(), quotient_marker()};
            check(p.error == OK && execute(s, p, z) == NONE && rows_hold(s, z) && z[2].eq(F::mul(F::mul(F::add(x, one), x), F::inv(u(2)))), "marker elsewhere: ... and executes");
        }
        {   // named in C beside a plain lone entry: a plain unknown, so the row is an opener.  1 a, 2 b given | 3 flag (byte 2), 4 m
            System s; s.mw = 4;
            const Row lc = {{one, 1}, {F::neg(one), 2}};
            s.add(lc, Row{{one, 4}}, Row{{one, 3}});
            s.add(lc, Row{{one, 0}, {F::neg(one), 3}}, Row{});
            const Plan p = in_order(s, s.unknown({4}, {3}));
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_ISZERO && p.pairs.size() == 1 && p.divs.empty(),
                  "marker elsewhere: a byte-2 column in C of an opener-shaped row is the pair's flag");
        }
        {   // bits with byte 2: a decomposition as before, and the kernels' marker test passes over both markers
            System s; s.mw = 3;
            s.boolean(2); s.boolean(3);
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}, {u(2), 3}});
            const Plan p = in_order(s, s.unknown({2}, {3}));
            std::vector<Fr> z = {one, u(2), marker(), quotient_marker()};
            check(p.error == OK && p.steps.size() == 1 && p.steps[0].kind == KIND_BITS_C && execute(s, p, z) == NONE && z[2].is_zero() && z[3].eq(one),
                  "marker elsewhere: byte-2 bits decompose");
        }
    }

    // ---- 4. one pattern per batch compares the BYTES (solve.hip: k_solve_pattern on marker_byte).  0 one | 1 a, 2 b | 3 q, 4 rem
    void mixed_markers() {
        const Fr one = F::one();
        const std::vector<Fr> first = {one, u(9), u(4), quotient_marker(), marker()}, second = {one, u(9), u(4), marker(), marker()};
        std::vector<uint8_t> pattern(5);
        uint64_t mismatch = NONE;
        for (uint64_t j = 0; j < 5; ++j) {
            pattern[j] = pm::marker_byte<P>(first[j]);
            if (pm::marker_byte<P>(second[j]) != pattern[j] && ((uint64_t)1 << 32 | j) < mismatch) mismatch = (uint64_t)1 << 32 | j;
        }
        check(pattern == std::vector<uint8_t>({0, 0, 0, PATTERN_QUOTIENT, PATTERN_UNKNOWN}), "mixed markers: the bytes of assignment 0");
        check(mismatch == ((uint64_t)1 << 32 | 3), "mixed markers: assignment 1 differs from assignment 0 at column 3");
        Fr near = marker();
        near.l[0] = 0xfffffffcu;
        Fr high = quotient_marker();
        high.l[7] = 0x7fffffffu;
        check(pm::marker_byte<P>(near) == 0 && pm::marker_byte<P>(high) == 0 && pm::marker_byte<P>(F::zero()) == 0 && pm::marker_byte<P>(F::neg(one)) == 0,
              "mixed markers: nothing else is a marker");
        // the two patterns are two plans: with the plain marker nothing is inferred
        System s; s.mw = 4;
        s.add(Row{{one, 3}}, Row{{one, 2}}, Row{{one, 1}, {F::neg(one), 4}});
        std::vector<uint8_t> plain = pattern;
        plain[3] = PATTERN_UNKNOWN;
        const Plan with = in_order(s, pattern), without = in_order(s, plain);
        check(with.error == OK && with.steps.size() == 1 && with.steps[0].kind == KIND_DIVREM, "mixed markers: the quotient marker makes the row a division");
        check(without.error == ERR_MANY_UNKNOWNS && without.error_row == 0 && without.message == "row 0: two or more unknowns (columns 3 and 4), and no is-zero pair: no later row closes it",
              "mixed markers: the plain marker leaves today's refusal, word for word");
    }

    // ---- 5. a division row and an is-zero pair over the same known side.  0 one | 1 out | 2 a, 3 b, 4 c given | 5 q, 6 rem | 7 flag, 8 m
    //   row 0: (a - b) * q = c - rem     row 1: (a - b) * m = flag     row 2: (a - b) * (1 - flag) = 0     row 3: (q + rem + flag) * 1 = out
    void beside_pairs() {
        const Fr one = F::one(), m1 = F::neg(one);
        System s; s.m0 = 2; s.mw = 7;
        const Row lc = {{one, 2}, {m1, 3}};
        s.add(lc, Row{{one, 5}}, Row{{one, 4}, {m1, 6}});
        s.add(lc, Row{{one, 8}}, Row{{one, 7}});
        s.add(lc, Row{{one, 0}, {m1, 7}}, Row{});
        s.add(Row{{one, 5}, {one, 6}, {one, 7}}, Row{{one, 0}}, Row{{one, 1}});
        const std::vector<uint8_t> unknown = s.unknown({1, 6, 7, 8}, {5});
        const Plan p = in_order(s, unknown);
        check(p.error == OK && p.steps.size() == 3 && p.pairs.size() == 1 && p.divs.size() == 1 && p.steps[0].kind == KIND_ISZERO && p.steps[0].row == 2 && p.steps[0].level == 1 &&
                  p.pairs[0].row1 == 1 && p.pairs[0].col_m == 8 && p.steps[1].kind == KIND_DIVREM && p.steps[1].row == 0 && p.steps[1].level == 1 && p.divs[0].col_r == 6 &&
                  p.divs[0].q_in_b == 1 && p.steps[2].kind == KIND_C && p.steps[2].level == 2 && well_sorted(p) && p.launches.size() == 1 && p.launches[0].divides == 1,
              "beside pairs: the division is a step at row 0, no opener, and the pair still closes");
        if (p.error != OK) return;
        const Plan wide = in_order(s, unknown, 2);
        check(wide.error == OK && wide.launches.size() == 3 && same_launch(wide.launches[0], Launch{0, 1, LAUNCH_ISZERO, 1}) && same_launch(wide.launches[1], Launch{1, 2, LAUNCH_DIVREM, 1}) &&
                  same_launch(wide.launches[2], Launch{2, 3, LAUNCH_CHAIN, 0}),
              "beside pairs: in a wide level the pairs and the divisions have launches of their own, both dividing");
        std::vector<Fr> z = {one, marker(), u(50), u(39), u(100), quotient_marker(), marker(), marker(), marker()};
        check(execute(s, p, z) == NONE && rows_hold(s, z) && z[5].eq(u(9)) && z[6].eq(u(1)) && z[7].eq(one) && z[8].eq(F::inv(u(11))) && z[1].eq(u(11)), "beside pairs: 100 = 9 * 11 + 1, a != b");
        std::vector<Fr> zero = {one, marker(), u(50), u(50), u(100), quotient_marker(), marker(), marker(), marker()};
        check(execute(s, p, zero) == 0 && zero[5].is_zero() && zero[6].is_zero() && zero[7].is_zero() && zero[8].is_zero(),
              "beside pairs: a = b: the division is stuck at row 0 with zeros stored, the pair is not");
        // a later row that names the remainder of an open... nothing is open: a division row never waits for a closer
        System t; t.mw = 4;
        t.add(Row{{one, 3}}, Row{{one, 2}}, Row{{one, 1}, {m1, 4}});
        t.add(Row{{one, 2}}, Row{{one, 0}, {m1, 4}}, Row{});      // the closer's shape over the same K: a check row here
        const Plan alone = in_order(t, t.unknown({4}, {3}));
        check(alone.error == OK && alone.steps.size() == 1 && alone.steps[0].kind == KIND_DIVREM && alone.pairs.empty(), "beside pairs: a closer-shaped row after a division row is a check row");
    }

    // ---- 6. the corpus
    struct Case {
        std::string what;
        System s;
        std::vector<uint32_t> unknown, quotients;
        std::vector<std::vector<uint32_t>> groups;      // rows that keep their relative order under every permutation (a pair's rows)
        int rounds = 1;
        std::function<std::vector<Fr>(int)> given;      // round -> z with the given columns set, markers elsewhere
    };
    // the range-checked division of polymath_amd.circuits: columns a, b (given), q, rem, then 3 x bits booleans from `base`
    //   booleanity rows; q * b = a - rem; rem * 1 = bits; (b - 1 - rem) * 1 = bits; q * 1 = bits
    static void division(Case &c, uint32_t a, uint32_t b, uint32_t q, uint32_t rem, uint32_t base, uint32_t bits) {
        const Fr one = F::one(), m1 = F::neg(one);
        Row sum[3];
        for (uint32_t k = 0; k < 3; ++k)
            for (uint32_t i = 0; i < bits; ++i) {
                const uint32_t j = base + k * bits + i;
                c.s.boolean(j);
                sum[k].push_back({u(1ull << i), j});
                c.unknown.push_back(j);
            }
        c.s.add(Row{{one, q}}, Row{{one, b}}, Row{{one, a}, {m1, rem}});
        c.s.add(Row{{one, rem}}, Row{{one, 0}}, sum[0]);
        c.s.add(Row{{one, b}, {m1, 0}, {m1, rem}}, Row{{one, 0}}, sum[1]);
        c.s.add(Row{{one, q}}, Row{{one, 0}}, sum[2]);
        c.unknown.push_back(rem);
        c.quotients.push_back(q);
    }
    Case divisions() {   // 40 divisions of 5-bit operands (one WIDE level), then 120 decompositions, then the sum: 0 one | 1 out | per division 4 + 15 columns
        Case c; c.what = "divisions";
        const uint32_t n = 40, bits = 5, per = 4 + 3 * bits;
        c.s.m0 = 2; c.s.mw = n * per;
        Row total;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t at = 2 + i * per;
            division(c, at, at + 1, at + 2, at + 3, at + 4, bits);
            total.push_back({F::one(), at + 2});
            total.push_back({F::one(), at + 3});
        }
        c.s.add(total, Row{{F::one(), 0}}, Row{{F::one(), 1}});
        c.unknown.push_back(1);
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one();
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t at = 2 + i * per;
                z[at] = u(round ? (i * 7 + 3) % 32 : 31 - i % 32);
                z[at + 1] = u(round ? 1 + i % 31 : 1 + (i * 5) % 31);
                z[at + 2] = quotient_marker();
            }
            return z;
        };
        return c;
    }
    Case mod_chain() {   // 0 one | 1 g, 2 c, 3 m, 4 s_0 given | per step p_i, q_i, s_{i+1}:  g * s_i = p_i ;  q_i * m = p_i + c - s_{i+1}
        Case c; c.what = "mod chain";
        const uint32_t n = 12;
        c.s.mw = 4 + 3 * n;
        const Fr one = F::one(), m1 = F::neg(one);
        uint32_t s = 4;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t p = 5 + 3 * i, q = p + 1, next = p + 2;
            c.s.add(Row{{one, 1}}, Row{{one, s}}, Row{{one, p}});
            c.s.add(Row{{one, q}}, Row{{one, 3}}, Row{{one, p}, {one, 2}, {m1, next}});
            c.unknown.push_back(p);
            c.unknown.push_back(next);
            c.quotients.push_back(q);
            s = next;
        }
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[1] = u(round ? 6364136223846793005ull : 1103515245); z[2] = u(round ? 1442695040888963407ull : 12345); z[3] = u(round ? 0xfffffffffffffc5ull : 2147483648u);
            z[4] = u(42);
            for (uint32_t i = 0; i < n; ++i) z[6 + 3 * i] = quotient_marker();
            return z;
        };
        return c;
    }
    // 0 one | 1 out | 2 a, 3 b, 4 c given | 5 q, 6 rem, 7 .. 15 bits | 16 flag, 17 m | 18 w
    //   a range-checked division c / (a - b)... with K a single column: t = a - b first.  (a - b) * 1 = w;  the division c / w;  ark's pair on rem;
    //   (q + flag) * w = out
    Case mixed() {
        Case c; c.what = "mixed";
        c.s.m0 = 2; c.s.mw = 17;
        const Fr one = F::one(), m1 = F::neg(one);
        c.s.add(Row{{one, 2}, {m1, 3}}, Row{{one, 0}}, Row{{one, 18}});
        c.unknown.push_back(18);
        division(c, 4, 18, 5, 6, 7, 3);
        const uint32_t b = c.s.boolean(16);
        c.s.add(Row{{one, 6}}, Row{{one, 17}}, Row{{one, 16}});
        c.s.add(Row{{one, 6}}, Row{{one, 0}, {m1, 16}}, Row{});
        c.groups.push_back({b, b + 1, b + 2});
        c.unknown.push_back(16);
        c.unknown.push_back(17);
        c.s.add(Row{{one, 5}, {one, 16}}, Row{{one, 18}}, Row{{one, 1}});
        c.unknown.push_back(1);
        const size_t ncols = c.s.m0 + c.s.mw;
        c.rounds = 2;      // rem != 0 and rem == 0
        c.given = [=](int round) {
            std::vector<Fr> z(ncols, marker());
            z[0] = F::one(); z[2] = u(20); z[3] = u(15); z[4] = u(round ? 5 : 7); z[5] = quotient_marker();
            return z;
        };
        return c;
    }
    void corpus() {
        std::vector<Case> cases;
        cases.push_back(divisions());
        cases.push_back(mod_chain());
        cases.push_back(mixed());
        for (Case &c : cases) {
            const std::vector<uint8_t> unknown = c.s.unknown(c.unknown, c.quotients);
            System &s = c.s;
            for (uint32_t wide : {WIDE_STEPS, 2u}) {
                const Plan p = in_order(s, unknown, wide), q = any_order(s, unknown, wide);
                check(p.error == OK && p.divs.size() == c.quotients.size() && well_sorted(p), c.what + ": plans in order");
                check(same_plan(p, q) && !q.reordered, c.what + ": in order the any-order builder is build_plan, field by field");
            }
            const Plan p = in_order(s, unknown);
            if (p.error != OK) continue;
            if (c.what == "divisions")
                check(p.launches.size() == 3 && same_launch(p.launches[0], Launch{0, 40, LAUNCH_DIVREM, 1}) && same_launch(p.launches[1], Launch{40, 41, LAUNCH_LEVEL, 0}) &&
                          same_launch(p.launches[2], Launch{41, 161, LAUNCH_BITS, 0}) && p.levels() == 2,
                      "divisions: one division launch, then the sum and one decomposition launch");
            if (c.what == "mod chain") check(p.launches.size() == 1 && same_launch(p.launches[0], Launch{0, 24, LAUNCH_CHAIN, 1}) && p.levels() == 24, "mod chain: one dividing chain of 24 levels");
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
                    check(q.error == OK && q.message.empty() && q.steps.size() == p.steps.size() && q.pairs.size() == p.pairs.size() && q.divs.size() == p.divs.size(), tag + ": plans");
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
        {   // reversed, the remainder's one-bit range check has the opener's shape and is examined first: the division releases it
            //   0 one | 1 a, 2 b given | 3 q, 4 rem, 5 bit.   in order: boolean(bit); q * b = a - rem; rem * 1 = bit
            System s; s.mw = 5;
            s.boolean(5);
            s.add(Row{{F::one(), 3}}, Row{{F::one(), 2}}, Row{{F::one(), 1}, {F::neg(F::one()), 4}});
            s.add(Row{{F::one(), 4}}, Row{{F::one(), 0}}, Row{{F::one(), 5}});
            const std::vector<uint8_t> unknown = s.unknown({4, 5}, {3});
            System t = s.permuted({2, 1, 0});
            const Plan p = in_order(s, unknown), q = any_order(t, unknown);
            check(p.error == OK && p.steps.size() == 2 && q.error == OK && q.reordered && q.steps.size() == 2 && q.pairs.empty() && q.steps[0].kind == KIND_DIVREM && q.steps[0].row == 1 &&
                      q.steps[1].kind == KIND_C && q.steps[1].row == 0 && q.steps[1].col == 5 && q.steps[1].level == 2,
                  "released: a ready division row releases an opener registered over its remainder");
            std::vector<Fr> z = {F::one(), u(9), u(2), quotient_marker(), marker(), marker()};
            check(q.error == OK && execute(t, q, z) == NONE && rows_hold(t, z) && z[3].eq(u(4)) && z[4].eq(F::one()) && z[5].eq(F::one()), "released: ... and executes");
        }
    }

    // ---- 7. the edge operands, executed: q * d = a - rem with a and d given.  0 one | 1 a, 2 d | 3 q, 4 rem
    void edges() {
        const Fr one = F::one();
        System s; s.mw = 4;
        s.add(Row{{one, 3}}, Row{{one, 2}}, Row{{one, 1}, {F::neg(one), 4}});
        const Plan p = in_order(s, s.unknown({4}, {3}));
        check(p.error == OK, "edges: the plan");
        if (p.error != OK) return;
        for (size_t i = 0; i < N_CASES; ++i) {
            const Literal &l = literals[i];
            std::vector<Fr> z = {one, from_hex(l.a), from_hex(l.d), quotient_marker(), marker()};
            check(execute(s, p, z) == NONE && z[3].eq(from_hex(l.q)) && z[4].eq(from_hex(l.rem)) && rows_hold(s, z), "edges: case " + std::to_string(i) + " equals its divmod literal");
        }
        std::vector<Fr> z = {one, rnd(), F::zero(), quotient_marker(), marker()};
        check(execute(s, p, z) == 0 && z[3].is_zero() && z[4].is_zero(), "edges: d = 0 is stuck at its row, zeros stored");
        // the integer routine on all 256 bits (beyond what a residue reaches): the carry out of the top word
        const uint64_t a[4] = {~0ull, ~0ull, ~0ull, ~0ull}, d[4] = {3, 0, 0, 1ull << 63};
        uint64_t q[4], rem[4];
        pm::divrem256(a, d, q, rem);
        check(q[0] == 1 && !(q[1] | q[2] | q[3]) && rem[0] == ~0ull - 3 && rem[1] == ~0ull && rem[2] == ~0ull && rem[3] == (1ull << 63) - 1, "edges: divrem256 with the top bit of d set");
    }

    int run() {
        shapes();
        refusals();
        marker_elsewhere();
        mixed_markers();
        beside_pairs();
        corpus();
        edges();
        return report();
    }
};

int main() {
    rng_state = 0x452821E638D01377ull;
    Suite<pm::BlsCurve> bls("bls12_381", BLS_CASES);
    Suite<pm::BnCurve> bn("bn254", BN_CASES);
    return (bls.run() | bn.run()) ? 1 : 0;
}
