// Witness solving, host side: the PLAN that completes a partial assignment by forward propagation through the rows of an R1CS
// (DESIGN.md §4.10).  Header-only, no HIP: the library's driver (csrc/solve.hip) and a CPU program (tests/native/
// solve_plan_selftest.cpp) include the same file.
//
// Input: the three matrices in CSR form with the first-entry rule already applied (a column occurs at most once per row and
// matrix: the key's resident matrices are like that), m0 + mw columns and one byte per column, non-zero = unknown.  A stored entry
// whose coefficient is zero names no variable.  Rows are visited ONCE, in matrix order; at row r, with the columns solved so far:
//   no unknown column                         a check row, skipped
//   one unknown u, in exactly one of A, B, C  a solve step (kind = the matrix that holds u); u is known from here on
//   anything else                             the structure is unsolvable: the error names the row
// and a marked column that no row determines is an error that names the column.
// level(step) = 1 + max level of the columns the row reads (given columns: level 0).  The steps come out sorted by level, inside
// a level by kind (C first: the kinds that divide share a launch), stable by row -- one counting sort.  O(nnz + columns).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace pmsolve {

enum Kind : uint32_t { KIND_C = 0, KIND_A = 1, KIND_B = 2 };   // z_u = (Az Bz - C_rest) / coef;  (Cz / Bz - A_rest) / coef;  (Cz / Az - B_rest) / coef

constexpr uint32_t WIDE_STEPS = 32;   // a level of at least this many steps gets launches of its own; narrower ones are walked by one lane per assignment

struct Csr {
    const uint64_t *rowptr;   // nr + 1
    const uint32_t *col;      // nnz
    const uint64_t *val;      // nnz x 4 words; all four zero = a zero coefficient
};

struct Step {
    uint64_t pos;     // index of the unknown's entry in its matrix (col / val arrays)
    uint32_t row, col, kind, level;
};

struct Launch {
    uint32_t lo, hi;  // steps [lo, hi) of the sorted list
    uint8_t chain;    // 1: one lane per assignment walks the steps in order; 0: one lane per (step, assignment), all of one level
    uint8_t divides;  // 1: some step of the range is KIND_A / KIND_B
};

enum Error : int { OK = 0, ERR_MANY_UNKNOWNS = 1, ERR_TWO_MATRICES = 2, ERR_UNDETERMINED = 3, ERR_COLUMN_ZERO = 4 };

struct Plan {
    std::vector<Step> steps;          // sorted by (level, kind, row)
    std::vector<uint32_t> level_ptr;  // level l (1-based) = steps [level_ptr[l - 1], level_ptr[l])
    std::vector<Launch> launches;
    int error = OK;
    uint64_t error_row = 0, error_col = 0;
    std::string message;              // empty when error == OK
    uint32_t levels() const { return level_ptr.empty() ? 0 : (uint32_t)level_ptr.size() - 1; }
};

inline bool coef_is_zero(const uint64_t *v) { return (v[0] | v[1] | v[2] | v[3]) == 0; }

inline Plan build_plan(const Csr m[3], uint64_t nr, uint64_t m0, uint64_t mw, const uint8_t *unknown, uint32_t wide_steps = WIDE_STEPS) {
    Plan p;
    const uint64_t ncols = m0 + mw;
    constexpr uint32_t UNSOLVED = ~(uint32_t)0;
    if (ncols && unknown[0]) {
        p.error = ERR_COLUMN_ZERO;
        p.message = "column 0 (the constant one) is marked unknown";
        return p;
    }
    std::vector<uint32_t> level(ncols);
    for (uint64_t j = 0; j < ncols; ++j) level[j] = unknown[j] ? UNSOLVED : 0;
    static const char *const NAME[3] = {"A", "B", "C"};
    static const uint32_t KIND_OF[3] = {KIND_A, KIND_B, KIND_C};
    uint32_t max_level = 0;
    for (uint64_t r = 0; r < nr; ++r) {
        uint32_t u = 0, found = 0, reads = 0, in_matrix = 0;
        uint64_t pos = 0;
        for (int k = 0; k < 3 && p.error == OK; ++k) {
            for (uint64_t e = m[k].rowptr[r]; e < m[k].rowptr[r + 1]; ++e) {
                if (coef_is_zero(m[k].val + 4 * e)) continue;
                const uint32_t j = m[k].col[e];
                if (level[j] != UNSOLVED) {
                    if (level[j] > reads) reads = level[j];
                    continue;
                }
                if (found && j != u) {
                    p.error = ERR_MANY_UNKNOWNS;
                    p.error_row = r;
                    p.error_col = j;
                    p.message = "row " + std::to_string(r) + ": two or more unknowns (columns " + std::to_string(u) + " and " + std::to_string(j) + ")";
                    break;
                }
                if (found) {   // the same unknown again: in another matrix, or a second time in this one
                    p.error = ERR_TWO_MATRICES;
                    p.error_row = r;
                    p.error_col = j;
                    p.message = "row " + std::to_string(r) + ": unknown column " + std::to_string(j) + " occurs in " + NAME[in_matrix] + " and in " + NAME[k];
                    break;
                }
                found = 1; u = j; pos = e; in_matrix = (uint32_t)k;
            }
        }
        if (p.error != OK) return p;
        if (!found) continue;
        const uint32_t lv = reads + 1;
        level[u] = lv;
        if (lv > max_level) max_level = lv;
        p.steps.push_back(Step{pos, (uint32_t)r, u, KIND_OF[in_matrix], lv});
    }
    for (uint64_t j = 0; j < ncols; ++j)
        if (level[j] == UNSOLVED) {
            p.error = ERR_UNDETERMINED;
            p.error_col = j;
            p.message = "column " + std::to_string(j) + " is marked unknown and no row determines it";
            p.steps.clear();
            return p;
        }
    // counting sort by (level, kind); the row order inside a key is the order of discovery
    std::vector<uint32_t> start((size_t)max_level * 3 + 1, 0);
    for (const Step &s : p.steps) ++start[(size_t)(s.level - 1) * 3 + s.kind + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    p.level_ptr.resize((size_t)max_level + 1);
    for (uint32_t l = 0; l <= max_level; ++l) p.level_ptr[l] = start[(size_t)l * 3];
    {
        std::vector<Step> sorted(p.steps.size());
        std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
        for (const Step &s : p.steps) sorted[cursor[(size_t)(s.level - 1) * 3 + s.kind]++] = s;
        p.steps.swap(sorted);
    }
    // launch schedule: a wide level is its own launch, split where the dividing kinds begin; consecutive narrow levels are one chain
    for (uint32_t l = 0; l < max_level; ++l) {
        const uint32_t lo = p.level_ptr[l], hi = p.level_ptr[l + 1], mid = start[(size_t)l * 3 + 1];   // [lo, mid) KIND_C, [mid, hi) A and B
        if (hi - lo >= wide_steps) {
            if (mid > lo) p.launches.push_back(Launch{lo, mid, 0, 0});
            if (hi > mid) p.launches.push_back(Launch{mid, hi, 0, 1});
        } else if (!p.launches.empty() && p.launches.back().chain) {
            p.launches.back().hi = hi;
            p.launches.back().divides |= (uint8_t)(hi > mid);
        } else {
            p.launches.push_back(Launch{lo, hi, 1, (uint8_t)(hi > mid)});
        }
    }
    return p;
}

}  // namespace pmsolve
