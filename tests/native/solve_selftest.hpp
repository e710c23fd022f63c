// The rig of the witness solver's eleven CPU programs (solve_plan_selftest.cpp, solve_bits_selftest.cpp, solve_iszero_selftest.cpp,
// solve_order_selftest.cpp, solve_divrem_selftest.cpp, solve_indicator_selftest.cpp, solve_sqrt_selftest.cpp, solve_block_selftest.cpp,
// solve_hint_selftest.cpp, solve_moddiv_selftest.cpp, solve_widediv_selftest.cpp): the systems they build, the planners behind one
// door each (in matrix order, in any order, with declared hints), the comparisons of plans, ONE invariant of the schedule
// (well_sorted) and ONE execute, which walks a plan's launches serially through every step body the kernels call
// (polymath_amd/csrc/solve_steps.cuh) on the host field type.  A program keeps its cases, its literals, its seed and its main.
//
// Every plan that in_order / any_order return is folded, field by field, into a running 64-bit FNV-1a digest per curve; report()
// prints it after the check count.  The drivers (tests/test_native_solve_*.py) assert the digests recorded from the planner as it
// stood before its rules were stated once: a change to any plan, error or message of the programs' cases changes a digest.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../polymath_amd/host/polymath.hpp"
#include "../../polymath_amd/host/solve_plan.hpp"
#include "../../polymath_amd/csrc/solve_steps.cuh"

using namespace pmsolve;

static uint64_t rng_state;   // every program's main sets its own seed
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class C>
struct SolveRig {
    typedef typename C::FrP P;
    typedef pmhost::FrOps<C> F;
    typedef typename F::Fr Fr;
    typedef std::vector<std::pair<Fr, uint32_t>> Row;
    static constexpr uint64_t NONE = ~(uint64_t)0;
    const char *name;
    int fails = 0, checks = 0;
    uint64_t modulus[4];
    uint64_t plans = 0, digest = 0xcbf29ce484222325ull;

    explicit SolveRig(const char *n) : name(n) {
        for (int i = 0; i < 4; ++i) modulus[i] = (uint64_t)P::MOD[2 * i] | (uint64_t)P::MOD[2 * i + 1] << 32;
    }
    void check(bool ok, const std::string &what) {
        ++checks;
        if (!ok) { ++fails; printf("%s: FAILED %s\n", name, what.c_str()); }
    }
    int report() {
        printf("%s: %d failures of %d\n", name, fails, checks);
        printf("%s: %llu plans, digest %016llx\n", name, (unsigned long long)plans, (unsigned long long)digest);
        return fails;
    }
    static Fr rnd() { return F::mul(F::from_u64(next_u64()), F::add(F::from_u64(next_u64()), F::pow(F::from_u64(next_u64() | 1), 5))); }
    static Fr u(uint64_t v) { return F::from_u64(v); }
    static Fr marker() { Fr m; memset(m.l, 0xff, sizeof m.l); return m; }
    static Fr quotient_marker() { Fr m = marker(); m.l[0] = 0xfffffffeu; return m; }
    static Fr indicator_marker() { Fr m = marker(); m.l[2] = 0xfffffffeu; return m; }      // bit 64: the lowest bit of the second 64-bit word
    static bool is_marker(const Fr &v) { return pm::marker_byte<P>(v) != 0; }

    struct System {
        uint64_t m0 = 1, mw = 0;
        std::vector<Row> a, b, c;
        std::vector<uint64_t> rowptr[3], val[3];
        std::vector<uint32_t> col[3];
        Csr m[3];
        uint32_t add(const Row &ra, const Row &rb, const Row &rc) { a.push_back(ra); b.push_back(rb); c.push_back(rc); return (uint32_t)a.size() - 1; }
        uint32_t boolean(uint32_t j, const Fr &k = F::one(), const Fr &k2 = F::one(), bool swap = false) {   // (k z_j) (k2 - k2 z_j) = 0, or the sides swapped
            const Row one_side = {{k, j}}, two_side = {{k2, 0}, {F::neg(k2), j}};
            return swap ? add(two_side, one_side, Row{}) : add(one_side, two_side, Row{});
        }
        uint64_t nr() const { return a.size(); }
        void freeze() {
            const std::vector<Row> *src[3] = {&a, &b, &c};
            for (int k = 0; k < 3; ++k) {
                rowptr[k].assign(1, 0); col[k].clear(); val[k].clear();
                for (const Row &r : *src[k]) {
                    for (const auto &e : r) {
                        col[k].push_back(e.second);
                        uint64_t w[4];
                        memcpy(w, e.first.l, 32);
                        val[k].insert(val[k].end(), w, w + 4);
                    }
                    rowptr[k].push_back(col[k].size());
                }
                if (col[k].empty()) { col[k].push_back(0); val[k].assign(4, 0); }
                m[k] = Csr{rowptr[k].data(), col[k].data(), val[k].data()};
            }
        }
        // pattern bytes: 1 on `cols`, 2 on `quotients`, 3 on `indicators`
        std::vector<uint8_t> unknown(const std::vector<uint32_t> &cols, const std::vector<uint32_t> &quotients = {}, const std::vector<uint32_t> &indicators = {}) const {
            std::vector<uint8_t> un(m0 + mw, 0);
            for (uint32_t j : cols) un[j] = PATTERN_UNKNOWN;
            for (uint32_t j : quotients) un[j] = PATTERN_QUOTIENT;
            for (uint32_t j : indicators) un[j] = PATTERN_INDICATOR;
            return un;
        }
        System permuted(const std::vector<uint32_t> &order) const {      // row i of the result is row order[i] of this system
            System t;
            t.m0 = m0; t.mw = mw;
            for (uint32_t r : order) t.add(a[r], b[r], c[r]);
            return t;
        }
    };

    // ---- the planners, every plan they return folded into the digest
    void fold(uint64_t v, int bytes) {
        for (int i = 0; i < bytes; ++i) digest = (digest ^ ((v >> (8 * i)) & 0xff)) * 0x100000001b3ull;
    }
    Plan folded(Plan p) {
        ++plans;
        fold((uint32_t)p.error, 4); fold(p.error_row, 8); fold(p.error_col, 8);
        fold(p.message.size(), 8);
        for (unsigned char ch : p.message) fold(ch, 1);
        fold(p.steps.size(), 8);
        for (const Step &s : p.steps) { fold(s.pos, 8); fold(s.row, 4); fold(s.col, 4); fold(s.kind, 4); fold(s.level, 4); fold(s.bits, 4); fold(s.cols_off, 4); }
        fold(p.level_ptr.size(), 8);
        for (uint32_t v : p.level_ptr) fold(v, 4);
        fold(p.launches.size(), 8);
        // the bytes that the six flags of a launch were when the digests were recorded: chain, divides, bits, iszero, divrem, indicator
        for (const Launch &l : p.launches) {
            fold(l.lo, 4); fold(l.hi, 4); fold(l.kind == LAUNCH_CHAIN, 1); fold(l.divides, 1);
            for (uint8_t kind : {LAUNCH_BITS, LAUNCH_ISZERO, LAUNCH_DIVREM, LAUNCH_INDICATOR}) fold(l.kind == kind, 1);
        }
        fold(p.bit_cols.size(), 8);
        for (uint32_t v : p.bit_cols) fold(v, 4);
        fold(p.pairs.size(), 8);
        for (const PairRows &r : p.pairs) { fold(r.pos_m, 8); fold(r.pos_c, 8); fold(r.row1, 4); fold(r.col_m, 4); fold(r.m_in_b, 1); fold(r.b_in_b, 1); fold(r.negated, 1); }
        fold(p.divs.size(), 8);
        for (const DivRow &r : p.divs) { fold(r.pos_r, 8); fold(r.col_r, 4); fold(r.q_in_b, 1); }
        fold(p.reordered, 1);
        return p;
    }
    Plan in_order(System &s, const std::vector<uint8_t> &unknown, uint32_t wide = WIDE_STEPS, bool with_modulus = true) {
        s.freeze();
        return folded(build_plan(s.m, s.nr(), s.m0, s.mw, unknown.data(), wide, with_modulus ? modulus : nullptr));
    }
    Plan any_order(System &s, const std::vector<uint8_t> &unknown, uint32_t wide = WIDE_STEPS, bool with_modulus = true) {
        s.freeze();
        return folded(build_plan_any_order(s.m, s.nr(), s.m0, s.mw, unknown.data(), wide, with_modulus ? modulus : nullptr));
    }
    // ---- declared hints: a declaration decoded against the system (`why`: the refusal, empty where it is accepted), and the plan with it
    std::vector<Hint> declare(const System &s, const std::vector<uint64_t> &desc, std::string *why = nullptr) {
        std::vector<Hint> hints;
        const std::string refused = decode_hints(desc.data(), desc.size(), s.m0 + s.mw, modulus, hints);
        if (why) *why = refused;
        return hints;
    }
    Plan hinted(System &s, const std::vector<uint8_t> &unknown, const std::vector<Hint> &hints, uint32_t wide = WIDE_STEPS) {
        s.freeze();
        return folded(build_plan_any_order(s.m, s.nr(), s.m0, s.mw, unknown.data(), wide, modulus, &hints));
    }
    typedef std::vector<uint32_t> Cols;
    // one long-division record of pm_pk_set_hints under opcode `op` (1, or 5: the wide one); `lit`: the divisor's limbs as canonical
    // words (then E is empty)
    static std::vector<uint64_t> longdiv_record(uint32_t n, const Cols &q, const Cols &rem, const Cols &D, const Cols &E, const std::vector<uint64_t> &lit = {},
                                                uint64_t op = HINT_LONGDIV) {
        std::vector<uint64_t> w = {op, n, q.size(), rem.size(), D.size(), lit.empty() ? E.size() : lit.size() / 4, lit.empty() ? 0 : HINT_DIVISOR_LITERAL};
        for (const Cols *cols : {&q, &rem, &D, &E}) w.insert(w.end(), cols->begin(), cols->end());
        w.insert(w.end(), lit.begin(), lit.end());
        return w;
    }
    static Cols range(uint32_t lo, uint32_t n) {
        Cols v(n);
        for (uint32_t i = 0; i < n; ++i) v[i] = lo + i;
        return v;
    }
    static Fr from_words(const uint64_t w[4]) {      // a canonical integer of four words as an element
        Fr v;
        memcpy(v.l, w, 32);
        return pm::to_mont<P>(v);
    }

    static Fr coef_at(const System &s, int k, uint64_t e) {
        Fr v;
        memcpy(v.l, s.val[k].data() + 4 * e, 32);
        return v;
    }
    static Fr dot(const System &s, int k, const std::vector<Fr> &z, uint64_t r) {
        Fr acc = F::zero();
        for (uint64_t e = s.rowptr[k][r]; e < s.rowptr[k][r + 1]; ++e) acc = F::add(acc, F::mul(coef_at(s, k, e), z[s.col[k][e]]));
        return acc;
    }
    // every row of the (frozen) system on a complete assignment
    static bool rows_hold(const System &s, const std::vector<Fr> &z) {
        for (uint64_t r = 0; r < s.nr(); ++r)
            if (!F::mul(dot(s, 0, z, r), dot(s, 1, z, r)).eq(dot(s, 2, z, r))) return false;
        return true;
    }

    // the step bodies' sink on the host: a plain minimum where the kernels take an atomic one
    struct StuckMin {
        uint64_t *word;
        bool reordered;
        std::vector<uint32_t> *rows;
        void operator()(const pm::SolveStepDev<P> &s) const {
            const uint64_t key = (reordered ? (uint64_t)s.level << 32 : 0) | s.row;
            if (key < *word) *word = key;
            if (rows) rows->push_back(s.row);
        }
    };
    // The plan on the (frozen) system's matrices as the library runs it: the device records, their inverses, then the launch schedule
    // walked serially through the kernels' dispatch (solve.hip: solve_group), a launch that divides through the DIV = true bodies.  A
    // step whose kind KIND_INFO does not map to its launch is a FAILED CHECK, and nothing runs it: solve_any would take a block or a
    // hint for a decomposition or an ordinary step.  -> the stuck word as the kernels leave it BEFORE k_solve_stuck_row: the minimum of
    // row, or of (level << 32) | row under a reordered plan (0 where a block is singular: "stuck at row 0" fails every caller);
    // `stuck_rows`: every row that stuck, in the order of the walk; `counters`: what the wide divisions of the walk did
    uint64_t execute(const System &s, const Plan &p, std::vector<Fr> &z, std::vector<uint32_t> *stuck_rows = nullptr, pm::WideCounters *counters = nullptr) {
        const Csr A{s.rowptr[0].data(), s.col[0].data(), s.val[0].data()}, B{s.rowptr[1].data(), s.col[1].data(), s.val[1].data()},
            Cm{s.rowptr[2].data(), s.col[2].data(), s.val[2].data()};
        pm::SolveRecords<P> rec = pm::solve_records<P>(p);
        const uint64_t count = rec.steps.size();
        for (uint64_t t = 0; t < count + 2 * rec.pairs.size(); ++t) pm::solve_inverse<P>(A, B, Cm, rec.steps.data(), count, rec.pairs.data(), rec.divs.data(), t);
        uint32_t column = 0;
        if (pm::solve_block_inverses<P>(p, rec, &column) != p.blocks.size()) return 0;
        uint64_t stuck = NONE;
        const StuckMin sink{&stuck, p.reordered, stuck_rows};
        for (const Launch &l : p.launches)
            for (uint32_t t = l.lo; t < l.hi; ++t) {
                const pm::SolveStepDev<P> &st = rec.steps[t];
                const bool known = st.kind < NUM_WIDE_KINDS;
                if (!known || (l.kind == LAUNCH_CHAIN ? !KIND_INFO[st.kind].chained : KIND_INFO[st.kind].launch != l.kind)) {
                    check(false, "execute: step " + std::to_string(t) + " of kind " + std::to_string(st.kind) + " lies in a launch of kind " + std::to_string(l.kind));
                    continue;
                }
                switch (l.kind) {
                case LAUNCH_BLOCK: pm::solve_block<P>(A, B, Cm, rec.blocks[st.bits], rec.block_idx.data(), rec.block_inv.data(), z.data()); break;
                case LAUNCH_LONGDIV: pm::solve_longdiv<P>(st, rec.hints[st.bits], rec.hint_idx.data(), l.rounds, z.data(), sink); break;
                case LAUNCH_MODDIV: pm::solve_moddiv<P>(st, rec.mods[st.bits], rec.hint_idx.data(), l.rounds, l.inv_rounds, z.data(), sink); break;
                case LAUNCH_LONGDIV_WIDE: pm::solve_longdiv_wide<P>(st, rec.hints[st.bits], rec.hint_idx.data(), z.data(), sink, counters); break;
                default:      // a chain, or the launch of a kind that one lane can walk: the same body
                    if (l.divides) pm::solve_any<P, true>(A, B, Cm, st, p.bit_cols.data(), rec.pairs.data(), rec.divs.data(), z.data(), sink);
                    else pm::solve_any<P, false>(A, B, Cm, st, p.bit_cols.data(), rec.pairs.data(), rec.divs.data(), z.data(), sink);
                }
            }
        return stuck;
    }

    static bool same_step(const Step &a, const Step &b) {
        return a.pos == b.pos && a.row == b.row && a.col == b.col && a.kind == b.kind && a.level == b.level && a.bits == b.bits && a.cols_off == b.cols_off;
    }
    static bool same_launch(const Launch &a, const Launch &b) {
        return a.lo == b.lo && a.hi == b.hi && a.kind == b.kind && a.divides == b.divides && a.rounds == b.rounds && a.inv_rounds == b.inv_rounds;
    }
    static bool same_plan(const Plan &a, const Plan &b) {
        bool ok = a.error == b.error && a.error_row == b.error_row && a.error_col == b.error_col && a.message == b.message && a.steps.size() == b.steps.size() &&
                  a.level_ptr == b.level_ptr && a.launches.size() == b.launches.size() && a.bit_cols == b.bit_cols && a.pairs.size() == b.pairs.size() &&
                  a.divs.size() == b.divs.size() && a.reordered == b.reordered;
        for (size_t t = 0; ok && t < a.steps.size(); ++t) ok = same_step(a.steps[t], b.steps[t]);
        for (size_t t = 0; ok && t < a.pairs.size(); ++t)
            ok = a.pairs[t].pos_m == b.pairs[t].pos_m && a.pairs[t].pos_c == b.pairs[t].pos_c && a.pairs[t].row1 == b.pairs[t].row1 && a.pairs[t].col_m == b.pairs[t].col_m &&
                 a.pairs[t].m_in_b == b.pairs[t].m_in_b && a.pairs[t].b_in_b == b.pairs[t].b_in_b && a.pairs[t].negated == b.pairs[t].negated;
        for (size_t t = 0; ok && t < a.divs.size(); ++t) ok = a.divs[t].pos_r == b.divs[t].pos_r && a.divs[t].col_r == b.divs[t].col_r && a.divs[t].q_in_b == b.divs[t].q_in_b;
        for (size_t t = 0; ok && t < a.launches.size(); ++t) ok = same_launch(a.launches[t], b.launches[t]);
        return ok;
    }
    static std::vector<uint32_t> column_levels(const System &s, const Plan &p) {      // 0: not solved by the plan
        std::vector<uint32_t> lv(s.m0 + s.mw, 0);
        for (const Step &st : p.steps) {
            if (st.bits) for (uint32_t i = 0; i < st.bits; ++i) lv[p.bit_cols[st.cols_off + i]] = st.level;
            else lv[st.col] = st.level;
            if (st.kind == KIND_ISZERO) lv[p.pairs[st.cols_off].col_m] = st.level;
            if (st.kind == KIND_DIVREM) lv[p.divs[st.cols_off].col_r] = st.level;
        }
        return lv;
    }
    static size_t count_kind(const Plan &p, uint32_t kind) {
        size_t n = 0;
        for (const Step &st : p.steps) n += st.kind == kind;
        return n;
    }
    // The schedule's invariant: the steps are sorted by (level, kind, row), strictly, and level_ptr says where the levels begin; the
    // launches tile the steps in that order; launch kind and step kinds agree through KIND_INFO -- a chain holds only kinds that a lane
    // can walk, every other launch only the kinds that map to its own, so no other launch holds such a step outside a chain --; a
    // launch that is neither a chain nor a block or hint launch holds one level; `divides` is the OR of the table's entries (a launch
    // that holds nothing but kind-C steps, indicator rows, blocks or hints does not divide); the trip counts are in their ranges on
    // the three hint kinds and zero elsewhere
    static bool well_sorted(const Plan &p) {
        bool ok = p.level_ptr.size() == (size_t)p.levels() + 1 && (p.steps.empty() || (p.level_ptr.front() == 0 && p.level_ptr.back() == p.steps.size()));
        for (size_t t = 0; ok && t < p.steps.size(); ++t) {
            const Step &b = p.steps[t];
            ok = b.kind < NUM_WIDE_KINDS && b.level >= 1 && b.level <= p.levels() && p.level_ptr[b.level - 1] <= t && t < p.level_ptr[b.level];
            if (ok && t) {
                const Step &a = p.steps[t - 1];
                ok = a.level < b.level || (a.level == b.level && (a.kind < b.kind || (a.kind == b.kind && a.row < b.row)));
            }
        }
        uint32_t at = 0;
        for (const Launch &l : p.launches) {
            const bool hint = l.kind == LAUNCH_LONGDIV || l.kind == LAUNCH_MODDIV || l.kind == LAUNCH_LONGDIV_WIDE, own = hint || l.kind == LAUNCH_BLOCK;
            ok = ok && l.lo == at && l.hi > l.lo && l.hi <= p.steps.size() && l.kind <= LAUNCH_LONGDIV_WIDE;
            uint8_t divides = 0;
            for (uint32_t t = l.lo; ok && t < l.hi; ++t) {
                const KindInfo &info = KIND_INFO[p.steps[t].kind];
                ok = (l.kind == LAUNCH_CHAIN ? info.chained != 0 : info.launch == l.kind) && (l.kind == LAUNCH_CHAIN || own || p.steps[t].level == p.steps[l.lo].level);
                divides |= info.divides;
            }
            ok = ok && divides == l.divides;
            ok = ok && (hint ? l.rounds >= 256 && l.rounds <= (l.kind == LAUNCH_LONGDIV_WIDE ? WIDE_D_BITS : HINT_D_BITS) : l.rounds == 0);
            ok = ok && (l.kind == LAUNCH_MODDIV ? l.inv_rounds >= 512 && l.inv_rounds <= 1024 : l.inv_rounds == 0);
            at = l.hi;
        }
        return ok && at == p.steps.size();
    }

    // the two forms of an is-zero pair (oracle/pyref/circuits.py: _new_is_zero).  lc = the tested combination; flag, m = the two fresh
    // columns.  swap1 / swap2: the known side in B (instead of A) in the opener / in the closer
    static void ark(System &s, const Row &lc, uint32_t flag, uint32_t m, bool swap1 = false, bool swap2 = false) {
        const Row mult = {{F::one(), m}}, not_flag = {{F::one(), 0}, {F::neg(F::one()), flag}};
        swap1 ? s.add(mult, lc, Row{{F::one(), flag}}) : s.add(lc, mult, Row{{F::one(), flag}});
        swap2 ? s.add(not_flag, lc, Row{}) : s.add(lc, not_flag, Row{});
    }
    static void circom(System &s, const Row &lc, uint32_t flag, uint32_t m, bool swap1 = false, bool swap2 = false) {
        Row minus;
        for (size_t i = lc.size(); i-- > 0;) minus.push_back({F::neg(lc[i].first), lc[i].second});    // negated AND stored in the opposite order
        const Row mult = {{F::one(), m}}, out = {{F::one(), flag}}, out_minus_one = {{F::one(), flag}, {F::neg(F::one()), 0}};
        swap1 ? s.add(mult, minus, out_minus_one) : s.add(minus, mult, out_minus_one);
        swap2 ? s.add(out, lc, Row{}) : s.add(lc, out, Row{});
    }
    // a permutation's fix-up: the rows of each group take the group's positions in the group's order (a pair's opener before its closer)
    static void keep_groups(std::vector<uint32_t> &order, const std::vector<std::vector<uint32_t>> &groups) {
        std::vector<uint32_t> pos(order.size());
        for (uint32_t i = 0; i < order.size(); ++i) pos[order[i]] = i;
        for (const auto &g : groups) {
            std::vector<uint32_t> at;
            for (uint32_t r : g) at.push_back(pos[r]);
            std::sort(at.begin(), at.end());
            for (size_t k = 0; k < g.size(); ++k) order[at[k]] = g[k];
        }
    }
};

// the rig's names in a program's  template <class C> struct Suite : SolveRig<C>
#define SOLVE_RIG_NAMES(C)                                                                                                              \
    typedef SolveRig<C> Rig;                                                                                                            \
    typedef typename Rig::P P;                                                                                                          \
    typedef typename Rig::F F;                                                                                                          \
    typedef typename Rig::Fr Fr;                                                                                                        \
    typedef typename Rig::Row Row;                                                                                                      \
    typedef typename Rig::System System;                                                                                                \
    using Rig::NONE; using Rig::name; using Rig::modulus; using Rig::check; using Rig::report; using Rig::rnd; using Rig::u; using Rig::marker;            \
    using Rig::quotient_marker; using Rig::indicator_marker; using Rig::is_marker; using Rig::in_order; using Rig::any_order; using Rig::coef_at;       \
    using Rig::rows_hold; using Rig::execute; using Rig::same_step; using Rig::same_launch; using Rig::same_plan; using Rig::column_levels;             \
    using Rig::count_kind; using Rig::well_sorted; using Rig::ark; using Rig::circom; using Rig::keep_groups; using Rig::dot;                           \
    using Rig::declare; using Rig::hinted; using Rig::longdiv_record; using Rig::range; using Rig::from_words; typedef typename Rig::Cols Cols;
