// What solve_modmuldiv_selftest.cpp needs beside the rig (solve_selftest.hpp), whose execute and well_sorted know the launch kinds up
// to LAUNCH_LONGDIV_WIDE: an executor that hands every launch kind the rig knows to the rig's step bodies, exactly as the rig does,
// and runs solve_modmuldiv itself; the schedule's invariant with the fifteenth kind in it; the record of opcode 7.
#pragma once
#include "solve_selftest.hpp"

template <class C>
struct MulDivRig : SolveRig<C> {
    SOLVE_RIG_NAMES(C)
    explicit MulDivRig(const char *n) : Rig(n) {}

    // one multiply-divide record of pm_pk_set_hints; `lit`: the modulus' limbs as canonical words (then Pc is empty)
    static std::vector<uint64_t> muldiv_record(uint32_t n, const Cols &z, const Cols &A, const Cols &B, const Cols &Np, const Cols &Nm, const Cols &Dp, const Cols &Dm,
                                               const Cols &Pc, const std::vector<uint64_t> &lit = {}, uint64_t cN = 1, uint64_t cD = 1) {
        std::vector<uint64_t> w = {HINT_MODMULDIV, n, z.size(), A.size(), B.size(), Np.size(), Nm.size(), Dp.size(), Dm.size(), lit.empty() ? Pc.size() : lit.size() / 4,
                                   lit.empty() ? 0 : HINT_MODULUS_LITERAL, cN, cD};
        for (const Cols *cols : {&z, &A, &B, &Np, &Nm, &Dp, &Dm, &Pc}) w.insert(w.end(), cols->begin(), cols->end());
        w.insert(w.end(), lit.begin(), lit.end());
        return w;
    }
    // one modular-division record (opcode 3), as solve_moddiv_selftest.cpp writes it
    static std::vector<uint64_t> moddiv_record(uint32_t n, const Cols &z, const Cols &Np, const Cols &Nm, const Cols &Dp, const Cols &Dm, const Cols &Pc,
                                               const std::vector<uint64_t> &lit = {}) {
        std::vector<uint64_t> w = {HINT_MODDIV, n, z.size(), Np.size(), Nm.size(), Dp.size(), Dm.size(), lit.empty() ? Pc.size() : lit.size() / 4,
                                   lit.empty() ? 0 : HINT_MODULUS_LITERAL};
        for (const Cols *cols : {&z, &Np, &Nm, &Dp, &Dm, &Pc}) w.insert(w.end(), cols->begin(), cols->end());
        w.insert(w.end(), lit.begin(), lit.end());
        return w;
    }
    static std::vector<uint64_t> literal(uint64_t v) { return {v, 0, 0, 0}; }

    // SolveRig::execute with one more case.  -> the stuck word before k_solve_stuck_row
    uint64_t execute_all(const System &s, const Plan &p, std::vector<Fr> &z, std::vector<uint32_t> *stuck_rows = nullptr) {
        const Csr A{s.rowptr[0].data(), s.col[0].data(), s.val[0].data()}, B{s.rowptr[1].data(), s.col[1].data(), s.val[1].data()},
            Cm{s.rowptr[2].data(), s.col[2].data(), s.val[2].data()};
        pm::SolveRecords<P> rec = pm::solve_records<P>(p);
        const uint64_t count = rec.steps.size();
        for (uint64_t t = 0; t < count + 2 * rec.pairs.size(); ++t) pm::solve_inverse<P>(A, B, Cm, rec.steps.data(), count, rec.pairs.data(), rec.divs.data(), t);
        uint32_t column = 0;
        if (pm::solve_block_inverses<P>(p, rec, &column) != p.blocks.size()) return 0;
        uint64_t stuck = NONE;
        const typename Rig::StuckMin sink{&stuck, p.reordered, stuck_rows};
        for (const Launch &l : p.launches)
            for (uint32_t t = l.lo; t < l.hi; ++t) {
                const pm::SolveStepDev<P> &st = rec.steps[t];
                const bool known = st.kind < NUM_MULDIV_KINDS;
                if (!known || (l.kind == LAUNCH_CHAIN ? !KIND_INFO[st.kind].chained : KIND_INFO[st.kind].launch != l.kind)) {
                    check(false, "execute: step " + std::to_string(t) + " of kind " + std::to_string(st.kind) + " lies in a launch of kind " + std::to_string(l.kind));
                    continue;
                }
                switch (l.kind) {
                case LAUNCH_MODMULDIV: pm::solve_modmuldiv<P>(st, rec.muls[st.bits], rec.hint_idx.data(), l.rounds, l.inv_rounds, z.data(), sink); break;
                case LAUNCH_BLOCK: pm::solve_block<P>(A, B, Cm, rec.blocks[st.bits], rec.block_idx.data(), rec.block_inv.data(), z.data()); break;
                case LAUNCH_LONGDIV: pm::solve_longdiv<P>(st, rec.hints[st.bits], rec.hint_idx.data(), l.rounds, z.data(), sink); break;
                case LAUNCH_MODDIV: pm::solve_moddiv<P>(st, rec.mods[st.bits], rec.hint_idx.data(), l.rounds, l.inv_rounds, z.data(), sink); break;
                case LAUNCH_LONGDIV_WIDE: pm::solve_longdiv_wide<P>(st, rec.hints[st.bits], rec.hint_idx.data(), z.data(), sink); break;
                default:
                    if (l.divides) pm::solve_any<P, true>(A, B, Cm, st, p.bit_cols.data(), rec.pairs.data(), rec.divs.data(), z.data(), sink);
                    else pm::solve_any<P, false>(A, B, Cm, st, p.bit_cols.data(), rec.pairs.data(), rec.divs.data(), z.data(), sink);
                }
            }
        return stuck;
    }

    // SolveRig::well_sorted with the fifteenth kind and its launch: two trip counts, as LAUNCH_MODDIV has
    static bool well_sorted_all(const Plan &p) {
        bool ok = p.level_ptr.size() == (size_t)p.levels() + 1 && (p.steps.empty() || (p.level_ptr.front() == 0 && p.level_ptr.back() == p.steps.size()));
        for (size_t t = 0; ok && t < p.steps.size(); ++t) {
            const Step &b = p.steps[t];
            ok = b.kind < NUM_MULDIV_KINDS && b.level >= 1 && b.level <= p.levels() && p.level_ptr[b.level - 1] <= t && t < p.level_ptr[b.level];
            if (ok && t) {
                const Step &a = p.steps[t - 1];
                ok = a.level < b.level || (a.level == b.level && (a.kind < b.kind || (a.kind == b.kind && a.row < b.row)));
            }
        }
        uint32_t at = 0;
        for (const Launch &l : p.launches) {
            const bool modular = l.kind == LAUNCH_MODDIV || l.kind == LAUNCH_MODMULDIV, hint = modular || l.kind == LAUNCH_LONGDIV || l.kind == LAUNCH_LONGDIV_WIDE,
                       own = hint || l.kind == LAUNCH_BLOCK;
            ok = ok && l.lo == at && l.hi > l.lo && l.hi <= p.steps.size() && l.kind <= LAUNCH_MODMULDIV;
            uint8_t divides = 0;
            for (uint32_t t = l.lo; ok && t < l.hi; ++t) {
                const KindInfo &info = KIND_INFO[p.steps[t].kind];
                ok = (l.kind == LAUNCH_CHAIN ? info.chained != 0 : info.launch == l.kind) && (l.kind == LAUNCH_CHAIN || own || p.steps[t].level == p.steps[l.lo].level);
                divides |= info.divides;
            }
            ok = ok && divides == l.divides;
            ok = ok && (hint ? l.rounds >= 256 && l.rounds <= (l.kind == LAUNCH_LONGDIV_WIDE ? WIDE_D_BITS : HINT_D_BITS) : l.rounds == 0);
            ok = ok && (modular ? l.inv_rounds >= 512 && l.inv_rounds <= 1024 : l.inv_rounds == 0);
            at = l.hi;
        }
        return ok && at == p.steps.size();
    }
};
