// The witness solver's plan builder (polymath_amd/host/solve_plan.hpp: header-only, no HIP) on the CPU: step lists, kinds, levels,
// level_ptr and the launch schedule against hand-written expectations, the structural errors with their rows and columns, and the
// plan EXECUTED serially with the host field type (polymath_amd/host/polymath.hpp: FrOps) against direct evaluation of the circuit.
// Built and run by tests/test_native_solve_plan.py.  Prints "<curve>: <failures> failures of <checks>" and the digest of its plans (solve_selftest.hpp).
#include "solve_selftest.hpp"

template <class C>
struct Suite : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit Suite(const char *n) : Rig(n) {}
    static Fr minus_one() { return F::neg(F::one()); }
    static bool eq(const Fr &a, const Fr &b) { return a.eq(b); }

    // the invariants every plan has: sorted by (level, kind, row), level_ptr monotone and consistent, a step's inputs solved at a lower
    // level, the launches a partition of the steps in order with chains made of narrow levels and level launches of one wide level
    void check_invariants(const System &s, const Plan &p, const std::vector<uint8_t> &unknown, uint32_t wide, const char *what) {
        bool ok = p.error == OK && p.level_ptr.size() >= 1 && p.level_ptr[0] == 0 && p.level_ptr.back() == p.steps.size();
        std::vector<uint32_t> level(s.m0 + s.mw, 0);
        for (const Step &st : p.steps) level[st.col] = st.level;
        size_t n_unknown = 0;
        for (uint8_t u : unknown) n_unknown += u != 0;
        ok = ok && n_unknown == p.steps.size();
        for (size_t t = 0; ok && t < p.steps.size(); ++t) {
            const Step &st = p.steps[t];
            ok = ok && unknown[st.col] && st.level >= 1 && st.level <= p.levels() && t >= p.level_ptr[st.level - 1] && t < p.level_ptr[st.level];
            if (t) {
                const Step &q = p.steps[t - 1];
                ok = ok && (q.level < st.level || (q.level == st.level && (q.kind < st.kind || (q.kind == st.kind && q.row < st.row))));
            }
            const int k = st.kind == KIND_A ? 0 : st.kind == KIND_B ? 1 : 2;
            ok = ok && st.pos >= s.rowptr[k][st.row] && st.pos < s.rowptr[k][st.row + 1] && s.col[k][st.pos] == st.col;
            uint32_t reads = 0;
            for (int mtx = 0; mtx < 3; ++mtx)
                for (uint64_t e = s.rowptr[mtx][st.row]; e < s.rowptr[mtx][st.row + 1]; ++e) {
                    if (coef_is_zero(s.val[mtx].data() + 4 * e) || (mtx == k && e == st.pos)) continue;
                    const uint32_t lv = level[s.col[mtx][e]];
                    ok = ok && lv < st.level;
                    if (lv > reads) reads = lv;
                }
            ok = ok && st.level == reads + 1;
        }
        for (size_t l = 1; ok && l < p.level_ptr.size(); ++l) ok = p.level_ptr[l] > p.level_ptr[l - 1];
        uint32_t at = 0;
        for (const Launch &l : p.launches) {
            ok = ok && l.lo == at && l.hi > l.lo;
            at = l.hi;
            bool divides = false;
            for (uint32_t t = l.lo; ok && t < l.hi; ++t) {
                const Step &st = p.steps[t];
                divides |= st.kind != KIND_C;
                const uint32_t width = p.level_ptr[st.level] - p.level_ptr[st.level - 1];
                ok = ok && (l.kind == LAUNCH_CHAIN ? width < wide : (width >= wide && st.level == p.steps[l.lo].level));
            }
            ok = ok && divides == (l.divides != 0);
        }
        ok = ok && at == p.steps.size();
        check(ok, what);
    }

    // ---- 1. three MiMC rounds (oracle/pyref/circuits.py: mimc_circuit): columns 0 one, 1 out, 2 xl, 3 xr, 4 tmp0, 5 new0, 6 tmp1, 7 new1, 8 tmp2
    void mimc3() {
        System s;
        s.m0 = 2; s.mw = 7;
        const Fr one = F::one(), m1 = minus_one(), k[3] = {rnd(), rnd(), rnd()};
        const uint32_t xl[3] = {2, 5, 7}, xr[3] = {3, 2, 5}, tmp[3] = {4, 6, 8}, nw[3] = {5, 7, 1};
        for (int i = 0; i < 3; ++i) {
            const Row lc = {{one, xl[i]}, {k[i], 0}};
            s.add(lc, lc, Row{{one, tmp[i]}});
            s.add(Row{{one, tmp[i]}}, lc, Row{{one, nw[i]}, {m1, xr[i]}});
        }
        std::vector<uint8_t> unknown = {0, 1, 0, 0, 1, 1, 1, 1, 1};
        const Plan p = in_order(s, unknown, WIDE_STEPS, false);
        check(p.error == OK && p.steps.size() == 6, "mimc3: six steps");
        const uint32_t want_col[6] = {4, 5, 6, 7, 8, 1};
        const uint64_t want_pos[6] = {0, 1, 3, 4, 6, 7};
        bool ok = p.steps.size() == 6;
        for (uint32_t t = 0; ok && t < 6; ++t)
            ok = p.steps[t].row == t && p.steps[t].col == want_col[t] && p.steps[t].kind == KIND_C && p.steps[t].level == t + 1 && p.steps[t].pos == want_pos[t];
        check(ok, "mimc3: rows, columns, kinds, levels, entry positions");
        check(p.level_ptr == std::vector<uint32_t>({0, 1, 2, 3, 4, 5, 6}), "mimc3: level_ptr");
        check(p.launches.size() == 1 && p.launches[0].kind == LAUNCH_CHAIN && p.launches[0].divides == 0 && p.launches[0].lo == 0 && p.launches[0].hi == 6, "mimc3: one chain");
        check_invariants(s, p, unknown, WIDE_STEPS, "mimc3: invariants");
        // execution against the native permutation
        Fr l = rnd(), r = rnd();
        std::vector<Fr> z(9, F::zero());
        z[0] = one; z[2] = l; z[3] = r;
        for (int i = 0; i < 3; ++i) {
            const Fr t = F::add(l, k[i]), nl = F::add(F::mul(F::mul(t, t), t), r);
            r = l; l = nl;
        }
        check(execute(s, p, z) == ~(uint64_t)0 && eq(z[1], l), "mimc3: the solved output is the native permutation");
    }

    // ---- 2. one level: row r is w[r] * 1 = w[nr + r], the second half unknown
    void diagonal() {
        for (uint32_t nr : {5u, 31u, 32u, 40u}) {
            System s;
            s.m0 = 1; s.mw = 2 * nr;
            for (uint32_t r = 0; r < nr; ++r) s.add(Row{{F::one(), 1 + r}}, Row{{F::one(), 0}}, Row{{F::one(), 1 + nr + r}});
            std::vector<uint8_t> unknown(1 + 2 * nr, 0);
            for (uint32_t r = 0; r < nr; ++r) unknown[1 + nr + r] = 1;
            const Plan p = in_order(s, unknown, WIDE_STEPS, false);
            bool ok = p.error == OK && p.steps.size() == nr && p.level_ptr == std::vector<uint32_t>({0, nr}) && p.launches.size() == 1 &&
                      (p.launches[0].kind == LAUNCH_CHAIN) == (nr < WIDE_STEPS) && p.launches[0].divides == 0;
            for (uint32_t r = 0; ok && r < nr; ++r) ok = p.steps[r].row == r && p.steps[r].col == 1 + nr + r && p.steps[r].level == 1 && p.steps[r].kind == KIND_C && p.steps[r].pos == r;
            check(ok, "diagonal: one level, wide from 32 steps on");
            check_invariants(s, p, unknown, WIDE_STEPS, "diagonal: invariants");
            std::vector<Fr> z(1 + 2 * nr, F::zero());
            z[0] = F::one();
            for (uint32_t r = 0; r < nr; ++r) z[1 + r] = rnd();
            ok = execute(s, p, z) == ~(uint64_t)0;
            for (uint32_t r = 0; ok && r < nr; ++r) ok = eq(z[1 + nr + r], z[1 + r]);
            check(ok, "diagonal: executed");
        }
    }

    // ---- 3. random gates (synthetic_r1cs's shape): gate i is (alpha z_p)(beta z_q) = gamma z_t, p, q uniform over the defined columns
    void random_gates() {
        const uint32_t nr = 600;
        System s;
        s.m0 = 2; s.mw = nr + 1;                       // the last gate's output is column 1
        std::vector<uint32_t> defined = {0, 2, 3}, level(2 + nr + 1, 0);
        std::vector<Fr> z(2 + nr + 1, F::zero());
        z[0] = F::one(); z[2] = rnd(); z[3] = rnd();
        std::vector<uint8_t> unknown(2 + nr + 1, 1);
        unknown[0] = unknown[2] = unknown[3] = 0;
        std::vector<uint32_t> want_level(nr);
        for (uint32_t i = 0; i < nr; ++i) {
            const Fr alpha = rnd(), beta = rnd(), gamma = (i % 3) ? F::one() : rnd();
            const uint32_t p = defined[next_u64() % defined.size()], q = defined[next_u64() % defined.size()];
            const uint32_t t = i == nr - 1 ? 1 : 4 + i;
            z[t] = F::mul(F::mul(F::mul(alpha, z[p]), F::mul(beta, z[q])), F::inv(gamma));
            level[t] = want_level[i] = 1 + (level[p] > level[q] ? level[p] : level[q]);
            if (i != nr - 1) defined.push_back(t);
            s.add(Row{{alpha, p}}, Row{{beta, q}}, Row{{gamma, t}});
        }
        for (uint32_t wide : {WIDE_STEPS, 4u, 1000000u}) {
            const Plan p = in_order(s, unknown, wide, false);
            bool ok = p.error == OK && p.steps.size() == nr;
            for (size_t t = 0; ok && t < p.steps.size(); ++t) ok = p.steps[t].level == want_level[p.steps[t].row] && p.steps[t].kind == KIND_C;
            check(ok, "random gates: levels are 1 + max of the inputs' levels");
            check_invariants(s, p, unknown, wide, "random gates: invariants");
            bool mixed[2] = {false, false};
            for (const Launch &l : p.launches) mixed[l.kind == LAUNCH_CHAIN] = true;
            check(wide == WIDE_STEPS ? (mixed[0] && mixed[1]) : wide == 4 ? mixed[0] : (mixed[1] && p.launches.size() == 1), "random gates: chains and level launches");
            std::vector<Fr> got(z.size(), F::zero());
            got[0] = z[0]; got[2] = z[2]; got[3] = z[3];
            ok = execute(s, p, got) == ~(uint64_t)0;
            for (size_t j = 0; ok && j < z.size(); ++j) ok = eq(got[j], z[j]);
            check(ok, "random gates: executed == direct evaluation");
        }
    }

    // ---- 4. kinds A and B, a coefficient to invert, stuck rows.  columns: 0 one, 1 a, 2 c, 3 inv, 4 q, 5 s, 6 t
    //   row 0: (3 inv) a = 1        inv in A        row 1: a (5 q) = c          q in B
    //   row 2: inv q = s            s in C          row 3: (s + 1) (2 t) = inv   t in B, reads s: level 3
    void kinds() {
        System s;
        s.m0 = 1; s.mw = 6;
        const Fr one = F::one();
        s.add(Row{{F::from_u64(3), 3}}, Row{{one, 1}}, Row{{one, 0}});
        s.add(Row{{one, 1}}, Row{{F::from_u64(5), 4}}, Row{{one, 2}});
        s.add(Row{{one, 3}}, Row{{one, 4}}, Row{{one, 5}});
        s.add(Row{{one, 5}, {one, 0}}, Row{{F::from_u64(2), 6}}, Row{{one, 3}});
        std::vector<uint8_t> unknown = {0, 0, 0, 1, 1, 1, 1};
        const Plan p = in_order(s, unknown, WIDE_STEPS, false);
        bool ok = p.error == OK && p.steps.size() == 4;
        const uint32_t want[4][4] = {{0, 3, KIND_A, 1}, {1, 4, KIND_B, 1}, {2, 5, KIND_C, 2}, {3, 6, KIND_B, 3}};   // row, column, kind, level
        for (int t = 0; ok && t < 4; ++t) ok = p.steps[t].row == want[t][0] && p.steps[t].col == want[t][1] && p.steps[t].kind == want[t][2] && p.steps[t].level == want[t][3];
        check(ok, "kinds: A, B, C, B at levels 1, 1, 2, 3");
        check(p.level_ptr == std::vector<uint32_t>({0, 2, 3, 4}) && p.launches.size() == 1 && p.launches[0].kind == LAUNCH_CHAIN && p.launches[0].divides, "kinds: one dividing chain");
        check_invariants(s, p, unknown, WIDE_STEPS, "kinds: invariants");
        const Plan split = in_order(s, unknown, 1, false);        // every level wide: level 1 is a dividing launch, level 2 is not
        check(split.launches.size() == 3 && split.launches[0].kind != LAUNCH_CHAIN && split.launches[0].divides && !split.launches[1].divides && split.launches[2].divides,
              "kinds: the dividing kinds have launches of their own");
        check_invariants(s, split, unknown, 1, "kinds: invariants, wide");
        const Fr a = rnd(), c = rnd();
        std::vector<Fr> z(7, F::zero());
        z[0] = one; z[1] = a; z[2] = c;
        ok = execute(s, p, z) == ~(uint64_t)0;
        const Fr inv = F::mul(F::inv(a), F::inv(F::from_u64(3))), q = F::mul(F::mul(c, F::inv(a)), F::inv(F::from_u64(5))), sv = F::mul(inv, q);
        const Fr t = F::mul(F::mul(inv, F::inv(F::add(sv, one))), F::inv(F::from_u64(2)));
        check(ok && eq(z[3], inv) && eq(z[4], q) && eq(z[5], sv) && eq(z[6], t), "kinds: executed");
        std::vector<Fr> z0(7, F::zero());
        z0[0] = one; z0[2] = c;                       // a = 0: rows 0 and 1 divide by zero, the smaller one is reported
        check(execute(s, p, z0) == 0, "kinds: a = 0 is stuck at row 0");
        z0[2] = F::zero();
        check(execute(s, p, z0) == 0, "kinds: 0 / 0 is stuck too");
    }

    // ---- 5. structural errors name their row or column
    void errors() {
        const Fr one = F::one();
        {
            System s; s.m0 = 1; s.mw = 3;             // row 1 has two unknowns
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(Row{{one, 2}}, Row{{one, 3}}, Row{{one, 1}});
            const Plan p = in_order(s, {0, 0, 1, 1}, WIDE_STEPS, false);
            check(p.error == ERR_MANY_UNKNOWNS && p.error_row == 1 && p.message.find("row 1") != std::string::npos, "error: two unknowns in row 1");
        }
        {
            System s; s.m0 = 1; s.mw = 2;             // b (1 - b) = 0 in row 2
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            s.add(Row{{one, 1}}, Row{{one, 1}}, Row{{one, 1}});
            s.add(Row{{one, 2}}, Row{{one, 0}, {minus_one(), 2}}, Row{});
            const Plan p = in_order(s, {0, 0, 1}, WIDE_STEPS, false);
            check(p.error == ERR_TWO_MATRICES && p.error_row == 2 && p.error_col == 2 && p.message.find("row 2") != std::string::npos, "error: an unknown in A and in B");
        }
        {
            System s; s.m0 = 1; s.mw = 3;             // column 3 is marked and no row touches it
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 2}});
            const Plan p = in_order(s, {0, 0, 1, 1}, WIDE_STEPS, false);
            check(p.error == ERR_UNDETERMINED && p.error_col == 3 && p.message.find("column 3") != std::string::npos && p.steps.empty(), "error: an undetermined column");
        }
        {
            System s; s.m0 = 1; s.mw = 1;
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            const Plan p = in_order(s, {1, 0}, WIDE_STEPS, false);
            check(p.error == ERR_COLUMN_ZERO, "error: column 0 marked");
        }
        {
            System s; s.m0 = 1; s.mw = 3;             // the entry (0, column 3) of row 0 names no variable: row 0 solves column 2, row 1 column 3
            s.add(Row{{F::zero(), 3}, {one, 1}}, Row{{one, 0}}, Row{{one, 2}});
            s.add(Row{{one, 2}}, Row{{one, 1}}, Row{{one, 3}, {F::zero(), 2}});
            const std::vector<uint8_t> unknown = {0, 0, 1, 1};
            const Plan p = in_order(s, unknown, WIDE_STEPS, false);
            check(p.error == OK && p.steps.size() == 2 && p.steps[0].col == 2 && p.steps[0].level == 1 && p.steps[1].col == 3 && p.steps[1].level == 2 &&
                      p.steps[0].pos == 0 && p.steps[1].pos == 1, "a zero coefficient names no variable");
            check_invariants(s, p, unknown, WIDE_STEPS, "zero coefficient: invariants");
            const Fr v = rnd();
            std::vector<Fr> z = {one, v, F::zero(), F::zero()};
            memset(z[2].l, 0xff, 32); memset(z[3].l, 0xff, 32);      // the markers, as the kernels find them
            check(execute(s, p, z) == ~(uint64_t)0 && eq(z[2], v) && eq(z[3], F::mul(v, v)), "zero coefficient: executed over the markers");
        }
        {
            System s; s.m0 = 1; s.mw = 1;             // nothing unknown: an empty plan
            s.add(Row{{one, 1}}, Row{{one, 0}}, Row{{one, 1}});
            const Plan p = in_order(s, {0, 0}, WIDE_STEPS, false);
            check(p.error == OK && p.steps.empty() && p.launches.empty() && p.levels() == 0, "no unknowns: an empty plan");
        }
    }

    int run() {
        mimc3();
        diagonal();
        random_gates();
        kinds();
        errors();
        return report();
    }
};

int main() {
    rng_state = 0x13198A2E03707344ull;
    Suite<pm::BlsCurve> bls{"bls12_381"};
    Suite<pm::BnCurve> bn{"bn254"};
    return (bls.run() | bn.run()) ? 1 : 0;
}
