// Host build of csrc/radix.cuh (plain C++): the radix-5 2^a recoding of the table-mode MSM and the planner's exactness check,
// against big-integer arithmetic written here.  Built and run by tests/test_native_radix.py (CPU, no GPU).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polymath_amd/csrc/constants.cuh"
#include "../../polymath_amd/csrc/radix.cuh"

using namespace pm;

// ---- unsigned integers of 512 bits, little-endian 32-bit limbs: enough for R^13 and the sums of digits times powers of R
struct Big {
    static constexpr int L = 16;
    uint32_t l[L];
    Big() { memset(l, 0, sizeof l); }
    explicit Big(uint64_t v) { memset(l, 0, sizeof l); l[0] = (uint32_t)v; l[1] = (uint32_t)(v >> 32); }
    template <class P>
    static Big modulus() { Big b; for (int i = 0; i < 8; ++i) b.l[i] = P::MOD[i]; return b; }
};
static int cmp(const Big &a, const Big &b) {
    for (int i = Big::L - 1; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i] ? -1 : 1;
    return 0;
}
static Big add(const Big &a, const Big &b) {
    Big r; uint64_t c = 0;
    for (int i = 0; i < Big::L; ++i) { c += (uint64_t)a.l[i] + b.l[i]; r.l[i] = (uint32_t)c; c >>= 32; }
    if (c) { printf("Big: overflow in add\n"); exit(2); }
    return r;
}
static Big sub(const Big &a, const Big &b) {          // a >= b
    Big r; int64_t c = 0;
    for (int i = 0; i < Big::L; ++i) { c += (int64_t)a.l[i] - b.l[i]; r.l[i] = (uint32_t)c; c >>= 32; }
    if (c) { printf("Big: negative difference\n"); exit(2); }
    return r;
}
static Big mul_small(const Big &a, uint32_t m) {
    Big r; uint64_t c = 0;
    for (int i = 0; i < Big::L; ++i) { c += (uint64_t)a.l[i] * m; r.l[i] = (uint32_t)c; c >>= 32; }
    if (c) { printf("Big: overflow in mul_small\n"); exit(2); }
    return r;
}
static Big div_small(const Big &a, uint32_t d, uint32_t *rem = nullptr) {
    Big q; uint64_t c = 0;
    for (int i = Big::L - 1; i >= 0; --i) { c = (c << 32) | a.l[i]; q.l[i] = (uint32_t)(c / d); c %= d; }
    if (rem) *rem = (uint32_t)c;
    return q;
}
static Big pow_small(uint32_t R, unsigned j) { Big r(1); for (unsigned i = 0; i < j; ++i) r = mul_small(r, R); return r; }
static Big reduce(Big x, const Big &r) { while (cmp(x, r) >= 0) x = sub(x, r); return x; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// (r - 1) div R^(W-1), the largest top digit
template <class P>
static Big top_digit(uint32_t R, unsigned W) {
    Big t = sub(Big::modulus<P>(), Big(1));
    for (unsigned j = 0; j + 1 < W; ++j) t = div_small(t, R);
    return t;
}

// ---- one (field, W, A): the scalar list of the issue through radix5_recode
template <class P, unsigned W, unsigned A>
static int recode_case(const char *name, int nrandom) {
    const uint32_t R = 5u << A, H = R / 2;
    const Big r = Big::modulus<P>();
    int fails = 0;
    std::vector<Big> ks;
    ks.push_back(Big(0));
    ks.push_back(Big(1));
    ks.push_back(sub(r, Big(1)));
    ks.push_back(div_small(sub(r, Big(1)), 2));
    for (unsigned j = 0; j < W; ++j) {
        const Big Rj = pow_small(R, j), HRj = mul_small(Rj, H);
        ks.push_back(reduce(Rj, r));
        ks.push_back(reduce(add(Rj, Big(1)), r));
        if (j) ks.push_back(reduce(sub(Rj, Big(1)), r));
        ks.push_back(reduce(add(HRj, Big(1)), r));
        ks.push_back(reduce(sub(HRj, Big(1)), r));
    }
    {   // every unsigned digit R/2 + 1 (a carry through every window) and every digit R - 1, the top digit held below r
        const Big X = pow_small(R, W - 1), top = top_digit<P>(R, W);
        const uint32_t tmax = top.l[0] ? top.l[0] - 1 : 0;       // (tmax + 1) X <= r - 1
        if (top.l[1] || top.l[2]) { printf("%s: top digit does not fit a word\n", name); return 1; }
        for (uint32_t dig : {H + 1, R - 1}) {
            Big v;
            for (unsigned j = 0; j + 1 < W; ++j) v = add(v, mul_small(pow_small(R, j), dig));
            v = add(v, mul_small(X, dig < tmax ? dig : tmax));
            ks.push_back(v);
        }
    }
    {   // 2^255 - 19 mod r
        Big v; v.l[7] = 0x80000000u;
        ks.push_back(reduce(sub(v, Big(19)), r));
    }
    for (int q = 0; q < nrandom; ++q) {
        Big v;
        for (int i = 0; i < 8; i += 2) { const uint64_t z = next_u64(); v.l[i] = (uint32_t)z; v.l[i + 1] = (uint32_t)(z >> 32); }
        v.l[7] &= 0x7FFFFFFFu;
        ks.push_back(reduce(v, r));
    }
    for (const Big &k : ks) {
        if (cmp(k, r) >= 0) { ++fails; printf("%s: test scalar not below r\n", name); continue; }
        uint32_t limbs[8], out[W];
        for (int i = 0; i < 8; ++i) limbs[i] = k.l[i];
        const uint32_t carry = radix5_recode<W, A>(limbs, out);
        Big pos, neg;                                            // k + neg == pos
        bool ok = carry == 0;
        for (unsigned j = 0; j < W; ++j) {
            if (out[j] == RADIX_NO_DIGIT) continue;
            const uint32_t mag = (out[j] >> 1) + 1;
            if (mag > H) ok = false;
            if (j == W - 1 && (out[j] & 1)) ok = false;          // a negative top digit would need a carry out
            const Big term = mul_small(pow_small(R, j), mag);
            if (out[j] & 1) neg = add(neg, term); else pos = add(pos, term);
        }
        if (cmp(add(k, neg), pos) != 0) ok = false;
        if (!ok) {
            ++fails;
            printf("%s W=%u A=%u: wrong digits for k =", name, W, A);
            for (int i = 7; i >= 0; --i) printf(" %08x", k.l[i]);
            printf(" (carry %u)\n", carry);
        }
    }
    printf("%s recode W=%u R=5*2^%u: %d failures of %zu scalars\n", name, W, A, fails, ks.size());
    return fails;
}

// ---- the planner's check against the same statement in big integers: (r - 1) div R^(W-1) + 1 <= R / 2
template <class P>
static int fits_case(const char *name, unsigned m, unsigned W, unsigned a, bool want, uint32_t want_top) {
    const uint32_t R = m << a;
    const Big top = top_digit<P>(R, W);
    const bool big = cmp(add(top, Big(1)), Big(R / 2)) <= 0;
    const bool got = radix_top_fits<P>(m, W, a);
    int fails = 0;
    if (big != want || got != want) { ++fails; printf("%s fits(m=%u W=%u a=%u): header %d, big integers %d, expected %d\n", name, m, W, a, got, big, want); }
    if (want_top && (top.l[0] + 1 != want_top || top.l[1])) { ++fails; printf("%s top digit bound (m=%u W=%u a=%u): %u, expected %u\n", name, m, W, a, top.l[0] + 1, want_top); }
    return fails;
}
template <class P>
static int fits_all(const char *name, uint32_t top12, uint32_t top11) {
    int fails = 0;
    fails += fits_case<P>(name, 1, 12, 22, true, 0);
    fails += fits_case<P>(name, 5, 12, 19, true, top12);
    fails += fits_case<P>(name, 1, 11, 24, true, 0);
    fails += fits_case<P>(name, 5, 11, 21, true, top11);
    fails += fits_case<P>(name, 5, 12, 18, false, 0);
    // the header against big integers over the whole grid the planner can ask for
    for (unsigned m : {1u, 5u})
        for (unsigned W = 8; W <= 32; ++W)
            for (unsigned a = 1; a <= 28; ++a) {
                const Big top = top_digit<P>(m << a, W);
                const bool big = cmp(add(top, Big(1)), Big((m << a) / 2)) <= 0;
                if (big != radix_top_fits<P>(m, W, a)) { ++fails; printf("%s fits(m=%u W=%u a=%u) differs from big integers\n", name, m, W, a); }
            }
    static_assert(radix_min_shift<P>(5, 11) == 21 && radix_min_shift<P>(5, 12) == 19 && radix_min_shift<P>(5, 13) == 18, "the issue's radices");
    static_assert(radix_min_shift<P>(5, 14) == 16 && radix_min_shift<P>(5, 16) == 14, "the small radices of the GPU tests");
    printf("%s exactness check: %d failures\n", name, fails);
    return fails;
}

template <class P>
static int curve(const char *name, int nrandom, uint32_t top12, uint32_t top11) {
    int fails = fits_all<P>(name, top12, top11);
    fails += recode_case<P, 12, 19>(name, nrandom);
    fails += recode_case<P, 11, 21>(name, nrandom);
    fails += recode_case<P, 13, 18>(name, nrandom);
    fails += recode_case<P, 14, 16>(name, nrandom);
    fails += recode_case<P, 16, 14>(name, nrandom);
    printf("%s: %d failures\n", name, fails);
    return fails;
}

int main(int argc, char **argv) {
    const int nrandom = argc > 1 ? atoi(argv[1]) : 10000;
    int fails = curve<BlsFrP>("bls12_381", nrandom, 1305238u, 3263093u);
    fails += curve<BnFrP>("bn254", nrandom, 544844u, 1362109u);
    return fails ? 1 : 0;
}
