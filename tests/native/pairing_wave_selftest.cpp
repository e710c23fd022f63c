// Host run of the wave-cooperative pairing's decomposition (csrc/pairing_wave.cuh: which lane multiplies what, which products wrap,
// who collects, the line's slots, the coefficient-wise Frobenius, the fixed-base table sum -- PM_HD, plain C++ here), lane after lane,
// against Tower<C> (csrc/pairing.cuh) and xyzz_mul_words (csrc/ec.cuh).  Built and run by tests/test_native_pairing_wave.py, plain and
// under -fsanitize=address,undefined (CPU, no GPU).  Prints "<curve>: <failures> failures of <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polymath_amd/csrc/pairing_wave.cuh"

using namespace pm;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class C>
struct Suite {
    typedef typename C::FrP R;
    typedef typename C::FqP Q;
    typedef Fp<Q> Fq;
    typedef Tower<C> T;
    typedef WaveTower<C> W;
    typedef PairingParams<C> PP;
    typedef typename T::Fq2 Fq2;
    typedef typename T::Fq12 Fq12;
    typedef typename W::Image Image;
    const char *name;
    int fails = 0, checks = 0;
    typename T::Consts K = T::make_consts();

    void expect(bool ok, const char *what) {
        ++checks;
        if (!ok) { ++fails; printf("%s: %s\n", name, what); }
    }
    static Fq rand_fq() {                                       // Montgomery form of a value < 2^(BITS - 1) < p
        Fq s;
        for (int i = 0; i < Q::N; i += 2) { const uint64_t v = next_u64(); s.l[i] = (uint32_t)v; s.l[i + 1] = (uint32_t)(v >> 32); }
        s.l[Q::N - 1] &= (1u << (Q::BITS - 1 - 32 * (Q::N - 1))) - 1;
        return to_mont<Q>(s);
    }
    static Fq2 rand_fq2() { return Fq2{rand_fq(), rand_fq()}; }
    static Image rand_image() {
        Image a;
        for (int i = 0; i < 6; ++i) a.c[i] = rand_fq2();
        return a;
    }
    static Image const_image(const Fq2 &v) {                    // v at w^0
        Image a;
        for (int i = 0; i < 6; ++i) a.c[i] = i == 0 ? v : T::zero2();
        return a;
    }
    static Image lone_image(int pos) {                          // one random coefficient at w^pos
        Image a;
        for (int i = 0; i < 6; ++i) a.c[i] = i == pos ? rand_fq2() : T::zero2();
        return a;
    }
    static bool same(const Image &a, const Image &b) {
        bool ok = true;
        for (int i = 0; i < 6; ++i) ok = ok && T::eq2(a.c[i], b.c[i]);
        return ok;
    }

    // ---- what the kernel does, one lane after the other: all products, then all collections
    static Image lanes_mul(const Image &a, const Image &b, bool line) {
        Fq2 prod[WAVE_GROUP];
        for (int lane = 0; lane < W::products(line); ++lane) prod[lane] = W::product(lane, a, b, line);
        Image r;
        for (int c = 0; c < 6; ++c) r.c[c] = W::collect(c, prod, line);
        return r;
    }
    static Image lanes_mul_line(const Image &f, const typename T::Line &L, const Affine<C> &P) {
        Image b;
        for (int s = 0; s < 6; ++s) b.c[s] = rand_fq2();        // slots 3 .. 5 are not a line's: whatever they hold is not read
        for (int s = 0; s < 3; ++s) b.c[s] = W::line_coeff(s, L, P);
        return lanes_mul(f, b, true);
    }
    Image lanes_frob(const Image &a) const {
        Image r;
        for (int c = 0; c < 6; ++c) r.c[c] = W::frob_coeff(c, a.c[c], K);
        return r;
    }

    void ring_case(const Image &a, const Image &b, const char *what) {
        const Fq12 ta = W::to_tower(a), tb = W::to_tower(b);
        expect(same(W::from_tower(ta), a), "from_tower(to_tower(a)) == a");
        expect(same(lanes_mul(a, b, false), W::from_tower(T::mul12(ta, tb))), what);
        expect(same(lanes_mul(a, a, false), W::from_tower(T::sqr12(ta))), "squaring by the product routine == sqr12");
        expect(same(lanes_frob(a), W::from_tower(T::frob12(ta, K))), "coefficient-wise Frobenius == frob12");
        Image cj;
        for (int c = 0; c < 6; ++c) cj.c[c] = W::conj_coeff(c, a.c[c]);
        expect(same(cj, W::from_tower(T::conj12(ta))), "odd coefficients negated == conj12");
    }
    void line_case(const Image &f, typename T::Line L, const Affine<C> &P, const char *what) {
        expect(same(lanes_mul_line(f, L, P), W::from_tower(T::mul_line(W::to_tower(f), L, P))), what);
    }

    static Affine<C> g1_generator() {
        Affine<C> g;
        for (int i = 0; i < Q::N; ++i) { g.x.l[i] = C::GX_MONT[i]; g.y.l[i] = C::GY_MONT[i]; }
        return g;
    }
    static bool same_point(const XYZZ<C> &a, const XYZZ<C> &b) {
        const Affine<C> p = xyzz_to_affine<C>(a), q = xyzz_to_affine<C>(b);
        return p.x.eq(q.x) && p.y.eq(q.y);
    }
    // the kernel's prelude: every lane's two windows, then the tree of additions, level by level
    static XYZZ<C> lanes_fixed_base(const std::vector<XYZZ<C>> &table, const uint32_t *k) {
        XYZZ<C> slots[WAVE_FB_LANES];
        for (int l = 0; l < WAVE_FB_LANES; ++l) slots[l] = W::fixed_base_lane(l, table.data(), k);
        for (int stride = WAVE_FB_LANES / 2; stride >= 1; stride >>= 1)
            for (int l = 0; l < stride; ++l) W::fixed_base_tree_step(l, stride, slots);
        return slots[0];
    }
    void scalar_case(const std::vector<XYZZ<C>> &table, const Affine<C> &G, const uint32_t *k, const char *what) {
        expect(same_point(lanes_fixed_base(table, k), xyzz_mul_words<C>(G, k, 8)), what);
    }

    void run() {
        const Fq2 one = T::one2(), minus_one = T::neg2(T::one2());
        // ---- the ring: random operands and the edges
        for (int t = 0; t < 4; ++t) ring_case(rand_image(), rand_image(), "36 products + collection == mul12 (random)");
        ring_case(const_image(T::zero2()), rand_image(), "0 b == mul12");
        ring_case(rand_image(), const_image(T::zero2()), "a 0 == mul12");
        ring_case(const_image(one), rand_image(), "1 b == mul12");
        ring_case(rand_image(), const_image(one), "a 1 == mul12");
        ring_case(const_image(minus_one), rand_image(), "(-1) b == mul12");
        ring_case(const_image(minus_one), const_image(minus_one), "(-1)(-1) == mul12");
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) ring_case(lone_image(i), lone_image(j), "lone coefficients: a_i w^i b_j w^j == mul12");
        for (int i = 0; i < 6; ++i) ring_case(lone_image(i), rand_image(), "a lone coefficient times a full element == mul12");
        // ---- lines: random, with each coefficient zero in turn, at a point at infinity (the line 1), against lone and full f
        const Affine<C> G = g1_generator(), O = Affine<C>::infinity();
        const Affine<C> P = xyzz_to_affine<C>(xyzz_mul_words<C>(G, std::vector<uint32_t>{0x1234567u, 0x89abcdefu}.data(), 2));
        for (int t = 0; t < 4; ++t) line_case(rand_image(), typename T::Line{rand_fq2(), rand_fq2()}, P, "18 products + collection == mul_line (random)");
        line_case(rand_image(), typename T::Line{T::zero2(), rand_fq2()}, P, "line with a = 0 == mul_line");
        line_case(rand_image(), typename T::Line{rand_fq2(), T::zero2()}, P, "line with b = 0 == mul_line");
        line_case(rand_image(), typename T::Line{T::zero2(), T::zero2()}, P, "line with a = b = 0 == mul_line");
        line_case(rand_image(), typename T::Line{Fq2{rand_fq(), Fq::zero()}, Fq2{Fq::zero(), rand_fq()}}, P, "line with half coefficients == mul_line");
        line_case(const_image(one), typename T::Line{rand_fq2(), rand_fq2()}, P, "1 times a line == mul_line");
        line_case(const_image(T::zero2()), typename T::Line{rand_fq2(), rand_fq2()}, P, "0 times a line == mul_line");
        for (int i = 0; i < 6; ++i) line_case(lone_image(i), typename T::Line{rand_fq2(), rand_fq2()}, P, "a lone coefficient times a line == mul_line");
        {
            const Image f = rand_image();
            expect(same(lanes_mul_line(f, typename T::Line{rand_fq2(), rand_fq2()}, O), f), "a pair at infinity: the line 1 leaves f as it is");
        }
        for (int c = 0; c < 6; ++c) {
            expect(W::is_one_coeff(c, W::one_coeff(c)), "1 == 1, coefficient by coefficient");
            Image a = const_image(one);
            a.c[c] = T::add2(a.c[c], Fq2{Fq::zero(), Fq::one()});
            expect(!W::is_one_coeff(c, a.c[c]), "1 + u w^c != 1 at coefficient c");
        }
        // ---- (-g) G from the table of G's multiples against the double-and-add
        std::vector<XYZZ<C>> table(WAVE_FB_ENTRIES);
        W::fixed_base_build(G, table.data());
        uint32_t k[8] = {};
        scalar_case(table, G, k, "0 G");
        k[0] = 1;
        scalar_case(table, G, k, "1 G");
        for (int i = 0; i < 8; ++i) k[i] = R::MOD[i];
        k[0] -= 1;                                              // r is odd: no borrow
        scalar_case(table, G, k, "(r - 1) G");
        for (unsigned d = 1; d < 16; d += 7) {
            memset(k, 0, sizeof k);
            k[0] = d;
            scalar_case(table, G, k, "one digit in the lowest window");
            k[0] = 0;
            k[7] = d << 28;                                     // past r: still the same group element
            scalar_case(table, G, k, "one digit in the highest window");
        }
        memset(k, 0, sizeof k);
        k[0] = 0x11;                                            // both windows of lane 0 hold the same digit: d G + 16 d G
        scalar_case(table, G, k, "equal digits in one lane's two windows");
        for (int t = 0; t < 4; ++t) {
            for (int i = 0; i < 8; i += 2) { const uint64_t v = next_u64(); k[i] = (uint32_t)v; k[i + 1] = (uint32_t)(v >> 32); }
            k[7] &= (1u << (R::BITS - 1 - 224)) - 1;
            scalar_case(table, G, k, "random words");
        }
        std::vector<XYZZ<C>> none(WAVE_FB_ENTRIES);
        W::fixed_base_build(O, none.data());
        expect(lanes_fixed_base(none, k).is_identity(), "G = O: the sum is the identity");
        printf("%s: %d failures of %d\n", name, fails, checks);
    }
};

int main() {
    Suite<BlsCurve> bls{"bls12_381"};
    bls.run();
    Suite<BnCurve> bn{"bn254"};
    bn.run();
    return bls.fails || bn.fails ? 1 : 0;
}
