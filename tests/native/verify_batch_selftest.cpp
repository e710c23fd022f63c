// Host build of the batch verifier's device functions (csrc/verify_batch.cuh: verify_term, verify_tree_add -- PM_HD, plain C++
// here) against the dense double-and-add of Polymath::verify (ec.cuh: xyzz_mul_words); that double-and-add against repeated
// addition; and the two pieces the host and the lanes share, verify_weigh and verify_node_points, against scalar arithmetic mod r
// done by shift-and-add on canonical words (no Montgomery form).  Built and run by
// tests/test_native_verify_batch.py (CPU, no GPU).  Prints "<curve>: <failures> failures of <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polymath_amd/csrc/verify_batch.cuh"

using namespace pm;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Scalar { uint32_t w[8]; };   // canonical, little-endian

template <class C>
struct Suite {
    typedef typename C::FrP R;
    typedef typename C::FqP Q;
    typedef Fp<R> Fr;
    const char *name;
    int fails = 0, checks = 0;

    static Scalar rand_scalar() {   // < 2^(BITS - 1) < r
        Scalar s;
        for (int i = 0; i < 8; i += 2) { const uint64_t v = next_u64(); s.w[i] = (uint32_t)v; s.w[i + 1] = (uint32_t)(v >> 32); }
        s.w[7] &= (1u << (R::BITS - 1 - 224)) - 1;
        return s;
    }
    static Scalar small(uint32_t v) { Scalar s{}; s.w[0] = v; return s; }
    static Scalar r_minus_1() { Scalar s; for (int i = 0; i < 8; ++i) s.w[i] = R::MOD[i]; s.w[0] -= 1; return s; }
    static Scalar rho128(uint64_t lo, uint64_t hi) { Scalar s{}; s.w[0] = (uint32_t)lo; s.w[1] = (uint32_t)(lo >> 32); s.w[2] = (uint32_t)hi; s.w[3] = (uint32_t)(hi >> 32); return s; }
    static Scalar mul_mod_r(const Scalar &a, const Scalar &b) {
        Fr x, y;
        memcpy(x.l, a.w, 32);
        memcpy(y.l, b.w, 32);
        const Fr p = from_mont<R>(mul<R>(to_mont<R>(x), to_mont<R>(y)));
        Scalar s;
        memcpy(s.w, p.l, 32);
        return s;
    }
    static Affine<C> generator() {
        Affine<C> g;
        for (int i = 0; i < Q::N; ++i) { g.x.l[i] = C::GX_MONT[i]; g.y.l[i] = C::GY_MONT[i]; }
        return g;
    }
    // the dense path: smul of Polymath::verify
    static XYZZ<C> smul(const Affine<C> &p, const Scalar &k) { return xyzz_mul_words<C>(p, k.w, 8); }
    // a + b mod r and a b mod r on canonical words, by carry and by shift-and-add: independent of the Montgomery code under test
    static Scalar add_mod(const Scalar &a, const Scalar &b) {
        uint32_t t[9], d[9];
        uint64_t c = 0;
        for (int i = 0; i < 8; ++i) { c += (uint64_t)a.w[i] + b.w[i]; t[i] = (uint32_t)c; c >>= 32; }
        t[8] = (uint32_t)c;
        int64_t br = 0;
        for (int i = 0; i < 9; ++i) { br += (int64_t)t[i] - (i < 8 ? R::MOD[i] : 0u); d[i] = (uint32_t)br; br >>= 32; }
        Scalar s;
        for (int i = 0; i < 8; ++i) s.w[i] = br < 0 ? t[i] : d[i];
        return s;
    }
    static Scalar mul_plain(const Scalar &a, const Scalar &b) {
        Scalar acc = small(0);
        for (int i = 7; i >= 0; --i)
            for (int bit = 31; bit >= 0; --bit) {
                acc = add_mod(acc, acc);
                if ((b.w[i] >> bit) & 1) acc = add_mod(acc, a);
            }
        return acc;
    }
    static Scalar negated_mod(const Scalar &a) { return mul_plain(a, r_minus_1()); }
    static Fr mont(const Scalar &a) { Fr x; memcpy(x.l, a.w, 32); return to_mont<R>(x); }
    static Affine<C> rand_point() { return xyzz_to_affine<C>(smul(generator(), rand_scalar())); }
    static Affine<C> negated(Affine<C> p) { p.y = neg<Q>(p.y); return p; }

    void same(const XYZZ<C> &got, const XYZZ<C> &want, const char *what, const char *coord) {
        ++checks;
        bool ok = got.is_identity() == want.is_identity();
        if (ok && !want.is_identity()) {
            const Affine<C> a = xyzz_to_affine<C>(got), b = xyzz_to_affine<C>(want);
            ok = a.x.eq(b.x) && a.y.eq(b.y) && affine_on_curve<C>(a);
        }
        if (!ok) { ++fails; printf("%s: %s: %s differs from the dense result\n", name, what, coord); }
    }

    struct Dense { XYZZ<C> U, V, W; };
    static Dense dense_term(const Affine<C> &A, const Affine<C> &Cp, const Affine<C> &D, const Scalar &rho, const Scalar &rx2, const Scalar &rx1) {
        return Dense{xyzz_add<C>(smul(A, rho), smul(Cp, rx2)), smul(D, rho), smul(D, rx1)};
    }
    static VerifyTerm<C> device_term(const Affine<C> &A, const Affine<C> &Cp, const Affine<C> &D, const Scalar &rho, const Scalar &rx2, const Scalar &rx1) {
        const Affine<C> pts[3] = {A, Cp, D};
        VerifyScalars sc;
        memcpy(sc.rho, rho.w, 16);
        memcpy(sc.rx2, rx2.w, 32);
        memcpy(sc.rx1, rx1.w, 32);
        VerifyTerm<C> out;
        verify_term<C>(pts, &sc, &out);
        return out;
    }
    void term_case(const char *what, const Affine<C> &A, const Affine<C> &Cp, const Affine<C> &D, const Scalar &rho, const Scalar &x2, const Scalar &x1) {
        const Scalar rx2 = mul_mod_r(rho, x2), rx1 = mul_mod_r(rho, x1);
        const VerifyTerm<C> got = device_term(A, Cp, D, rho, rx2, rx1);
        const Dense want = dense_term(A, Cp, D, rho, rx2, rx1);
        same(got.U, want.U, what, "U");
        same(got.V, want.V, what, "V");
        same(got.W, want.W, what, "W");
    }

    void tree_case(int n) {
        size_t padded = 1;
        unsigned depth = 0;
        while (padded < (size_t)n) { padded <<= 1; ++depth; }
        std::vector<VerifyTerm<C>> tree(2 * padded - 1);
        Dense sum{XYZZ<C>::identity(), XYZZ<C>::identity(), XYZZ<C>::identity()};
        for (size_t i = 0; i < padded; ++i) {
            VerifyTerm<C> &leaf = tree[i];
            if (i >= (size_t)n) {
                leaf.U = leaf.V = leaf.W = XYZZ<C>::identity();
            } else if (i == 1) {                             // the negative of its left neighbour: the pair cancels one level up
                leaf = tree[0];
                leaf.U.Y = neg<Q>(leaf.U.Y); leaf.V.Y = neg<Q>(leaf.V.Y); leaf.W.Y = neg<Q>(leaf.W.Y);
            } else if (i == 3) {                             // its left neighbour again: the pair is a doubling
                leaf = tree[2];
            } else {
                const Scalar rho = rho128(next_u64(), next_u64());
                leaf = device_term(rand_point(), rand_point(), rand_point(), rho, mul_mod_r(rho, rand_scalar()), mul_mod_r(rho, rand_scalar()));
            }
            sum.U = xyzz_add<C>(sum.U, leaf.U); sum.V = xyzz_add<C>(sum.V, leaf.V); sum.W = xyzz_add<C>(sum.W, leaf.W);
        }
        for (unsigned l = 1; l <= depth; ++l) {
            const VerifyTerm<C> *below = &tree[verify_level_offset(padded, l - 1)];
            VerifyTerm<C> *level = &tree[verify_level_offset(padded, l)];
            for (size_t j = 0; j < (padded >> l); ++j) {
                level[j].U = verify_tree_add<C>(below[2 * j].U, below[2 * j + 1].U);
                level[j].V = verify_tree_add<C>(below[2 * j].V, below[2 * j + 1].V);
                level[j].W = verify_tree_add<C>(below[2 * j].W, below[2 * j + 1].W);
            }
        }
        char what[48];
        snprintf(what, sizeof what, "tree of %d terms", n);
        const VerifyTerm<C> &root = tree[2 * padded - 2];
        same(root.U, sum.U, what, "U");
        same(root.V, sum.V, what, "V");
        same(root.W, sum.W, what, "W");
    }

    void expect(bool ok, const char *what) {
        ++checks;
        if (!ok) { ++fails; printf("%s: %s\n", name, what); }
    }

    // xyzz_mul_words against repeated addition: k = 0 .. 9, r - 1 (one more addition closes the group), P = O
    void mul_words_cases() {
        const Affine<C> P = rand_point(), O = Affine<C>::infinity();
        XYZZ<C> sum = XYZZ<C>::identity();
        for (uint32_t k = 0; k < 10; ++k) {
            same(smul(P, small(k)), sum, "xyzz_mul_words: k P against k additions", "point");
            sum = xyzz_add<C>(sum, XYZZ<C>::from_affine(P));
        }
        const XYZZ<C> m = smul(P, r_minus_1());
        same(m, XYZZ<C>::from_affine(negated(P)), "xyzz_mul_words: (r - 1) P", "-P");
        expect(xyzz_add<C>(m, XYZZ<C>::from_affine(P)).is_identity(), "xyzz_mul_words: (r - 1) P + P is not O");
        expect(smul(O, rand_scalar()).is_identity() && smul(O, small(0)).is_identity(), "xyzz_mul_words: k O is not O");
        const uint32_t one_word = 0x80000001u;
        Scalar wide = small(one_word);
        same(xyzz_mul_words<C>(P, &one_word, 1), smul(P, wide), "xyzz_mul_words: one word against eight", "point");
    }

    // verify_weigh: rho x2, rho x1 canonical and g = rho (a + x2 c) as Polymath::verifier_challenges' caller needs them
    void weigh_case(const char *what, const Scalar &rho, const Scalar &x1, const Scalar &x2, const Scalar &c_at, const Scalar &a_at, bool live) {
        VerifyScalars sc;
        memset(&sc, 0xA5, sizeof sc);
        memcpy(sc.rho, rho.w, 16);
        const Fr g = from_mont<R>(verify_weigh<C>(sc, mont(x1), mont(x2), mont(c_at), mont(a_at), live));
        const Scalar zero = small(0);
        const Scalar rx2 = live ? mul_plain(rho, x2) : zero, rx1 = live ? mul_plain(rho, x1) : zero;
        const Scalar want_g = live ? mul_plain(rho, add_mod(a_at, mul_plain(x2, c_at))) : zero;
        expect(!memcmp(sc.rho, live ? rho.w : zero.w, 16) && !memcmp(sc.rx2, rx2.w, 32) && !memcmp(sc.rx1, rx1.w, 32) && !memcmp(g.l, want_g.w, 32), what);
    }

    // verify_node_points on a node of known multiples of G: {(u + neg_g) G, -v G, w G}
    void node_case(const char *what, const Scalar &u, const Scalar &v, const Scalar &w, const Scalar &neg_g, bool with_g) {
        const Affine<C> G = generator(), none = Affine<C>::infinity();
        const VerifyTerm<C> nd{smul(G, u), smul(G, v), smul(G, w)};
        Affine<C> P[3];
        verify_node_points<C>(nd, neg_g.w, with_g ? G : none, P);
        const Scalar k[3] = {with_g ? add_mod(u, neg_g) : u, negated_mod(v), w};
        for (int j = 0; j < 3; ++j) {
            const Affine<C> want = xyzz_to_affine<C>(smul(G, k[j]));
            expect(P[j].x.eq(want.x) && P[j].y.eq(want.y) && affine_on_curve<C>(P[j]), what);
        }
    }

    void run() {
        mul_words_cases();
        for (int k = 0; k < 4; ++k)
            weigh_case("verify_weigh: a drawn row", rho128(next_u64(), next_u64()), rand_scalar(), rand_scalar(), rand_scalar(), rand_scalar(), true);
        weigh_case("verify_weigh: x1 = 0, x2 = r - 1", rho128(~0ull, ~0ull), small(0), r_minus_1(), r_minus_1(), r_minus_1(), true);
        weigh_case("verify_weigh: a dead row", rho128(next_u64(), next_u64()), rand_scalar(), rand_scalar(), rand_scalar(), rand_scalar(), false);
        for (int k = 0; k < 2; ++k) node_case("verify_node_points: a drawn node", rand_scalar(), rand_scalar(), rand_scalar(), rand_scalar(), true);
        const Scalar u = rand_scalar();
        node_case("verify_node_points: g G = U (the first point is O)", u, rand_scalar(), rand_scalar(), negated_mod(u), true);
        node_case("verify_node_points: V = W = O", u, small(0), small(0), rand_scalar(), true);
        node_case("verify_node_points: G = O", u, rand_scalar(), rand_scalar(), rand_scalar(), false);
        const Affine<C> O = Affine<C>::infinity();
        const Scalar one = small(1), zero = small(0), rm1 = r_minus_1();
        for (int k = 0; k < 6; ++k)
            term_case("random", rand_point(), rand_point(), rand_point(), rho128(next_u64(), next_u64()), rand_scalar(), rand_scalar());
        const Affine<C> A = rand_point(), D = rand_point(), Cp = rand_point();
        const Scalar rho = rho128(next_u64(), next_u64());
        term_case("A = C", A, A, D, rho, rand_scalar(), rand_scalar());
        term_case("A = -C", A, negated(A), D, rho, rand_scalar(), rand_scalar());
        term_case("A = C, x2 = r - 1 (U cancels)", A, A, D, rho, rm1, rand_scalar());
        term_case("A = -C, x2 = 1 (U cancels)", A, negated(A), D, rho, one, rand_scalar());
        term_case("A at infinity", O, Cp, D, rho, rand_scalar(), rand_scalar());
        term_case("C at infinity", A, O, D, rho, rand_scalar(), rand_scalar());
        term_case("D at infinity", A, Cp, O, rho, rand_scalar(), rand_scalar());
        term_case("rho = 1", A, Cp, D, one, rand_scalar(), rand_scalar());
        term_case("rho = 2^128 - 1", A, Cp, D, rho128(~0ull, ~0ull), rand_scalar(), rand_scalar());
        const Scalar edge[3] = {zero, one, rm1};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) term_case("x1, x2 in {0, 1, r - 1}", A, Cp, D, rho, edge[j], edge[i]);
        for (int n : {1, 2, 3, 5, 8}) tree_case(n);
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
