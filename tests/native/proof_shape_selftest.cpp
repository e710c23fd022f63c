// Host check of csrc/prove_common.cuh's description of a proof's shape (proof_shape: vector lengths and the division scan's level plan)
// and of its flag-word-to-status functions, against values worked out by hand.  Built for the host only and run by
// tests/test_native_proof_shape.py (CPU, no GPU: no HIP call is made).  Prints "proof_shape: <failures> failures of <checks>".
#include <cstdio>

#include "../../polymath_amd/csrc/prove_common.cuh"

using namespace pm;

static int fails = 0, checks = 0;
static void expect(bool ok, const char *what, unsigned long long at) {
    ++checks;
    if (!ok) { ++fails; printf("FAIL %s at %llu\n", what, at); }
}

static void shape(uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t num_len, int levels, const uint64_t *cnt) {
    const ProofShape s = proof_shape(n, m0, mw, nr, n + 3);
    expect(s.n == n && s.m0 == m0 && s.mw == mw && s.nr == nr && s.sigma == n + 3, "sizes", n);
    expect(s.Lz == 2 * m0 + mw + nr, "Lz", n);
    expect(s.len_a == n + 3, "len_a", n);
    expect(s.len_c == s.Lz + 2 * n + 5, "len_c", n);
    expect(s.num_len == num_len && s.num_len == 10 * n + 23, "num_len", n);
    expect(s.len_d == num_len - 1, "len_d", n);
    expect(s.levels == levels, "levels", n);
    expect(s.cnt[0] == num_len, "cnt[0]", n);
    for (int l = 1; l <= levels; ++l) expect(s.cnt[l] == cnt[l - 1], "cnt[l]", n * 10 + l);
    expect(s.cnt[levels] <= 64, "top level fits one lane", n);
    for (int l = 0; l < levels; ++l) expect(s.cnt[l] > 64, "a level under the top is chunked", n * 10 + l);
}

int main() {
    static_assert(DIV_L == 16 && HORNER_L == 16, "chunk lengths");
    const uint64_t none[1] = {0}, c8[1] = {7}, c128[2] = {82, 6}, c2p20[5] = {655362, 40961, 2561, 161, 11};
    shape(4, 1, 3, 1, 63, 0, none);                      // one lane divides
    shape(8, 1, 6, 3, 103, 1, c8);
    shape(128, 2, 50, 60, 1303, 2, c128);
    shape((uint64_t)1 << 20, 2, 524288, 524286, 10485783, 5, c2p20);
    // phase 1 reads bits 0-2: a failed square check first, then the degree checks (bit 1 set, or bit 2 clear); bit 3 is phase 3's
    for (unsigned f = 0; f < 16; ++f) {
        const int want1 = (f & 1u) ? PM_ERR_REMAINDER_NONZERO : (f == 4u || f == 12u) ? PM_OK : PM_ERR_DEGREE_BOUND;
        expect(phase1_flag_status(f) == want1, "phase-1 status", f);
        expect(phase3_flag_status(f) == (f >= 8u ? PM_ERR_REMAINDER_NONZERO : PM_OK), "phase-3 status", f);
    }
    expect(phase1_flag_status(0xFFFFFFF4u) == PM_OK && phase3_flag_status(0xFFFFFFF7u) == PM_OK, "bits above 3 are not read", 0);
    printf("proof_shape: %d failures of %d\n", fails, checks);
    return fails ? 1 : 0;
}
