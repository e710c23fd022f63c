// Host build of the device pairing (csrc/pairing.cuh: tower, prepared G2 lines, shared multi-Miller loop, x-chain final
// exponentiation -- PM_HD, plain C++ here) against the oracle-pinned host pairing (host/pairing.hpp).  Built and run by
// tests/test_native_pairing.py (CPU, no GPU).  Prints "<curve>: <failures> failures of <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polymath_amd/csrc/pairing.cuh"
#include "../../polymath_amd/host/pairing.hpp"

using namespace pm;

static uint64_t rng_state = 0x13198A2E03707344ull;
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
    typedef Fp<R> Fr;
    typedef Tower<C> T;
    typedef PairingParams<C> PP;
    typedef typename pmhost::PairingOf<C>::type Host;
    typedef typename T::Fq12 Fq12;
    typedef typename T::G2Affine G2A;
    const char *name;
    int fails = 0, checks = 0;
    typename T::Consts K = T::make_consts();

    void expect(bool ok, const char *what) {
        ++checks;
        if (!ok) { ++fails; printf("%s: %s\n", name, what); }
    }
    static Fr rand_fr() {   // Montgomery form of a value < 2^(BITS - 1) < r
        Fr s;
        for (int i = 0; i < 8; i += 2) { const uint64_t v = next_u64(); s.l[i] = (uint32_t)v; s.l[i + 1] = (uint32_t)(v >> 32); }
        s.l[7] &= (1u << (R::BITS - 1 - 224)) - 1;
        return to_mont<R>(s);
    }
    static Affine<C> g1_generator() {
        Affine<C> g;
        for (int i = 0; i < Q::N; ++i) { g.x.l[i] = C::GX_MONT[i]; g.y.l[i] = C::GY_MONT[i]; }
        return g;
    }
    static Affine<C> g1_mul(const Affine<C> &p, const Fr &k_mont) {
        const Fr k = from_mont<R>(k_mont);
        return xyzz_to_affine<C>(xyzz_mul_words<C>(p, k.l, R::N));
    }
    static typename Host::G2 g2_mul(const typename Host::G2 &p, const Fr &k_mont) {
        const Fr k = from_mont<R>(k_mont);
        return Host::g2_mul(p, k.l, R::N);
    }
    static G2A to_dev(const typename Host::G2 &g) {
        G2A a;
        a.x.c0 = g.x.c0; a.x.c1 = g.x.c1; a.y.c0 = g.y.c0; a.y.c1 = g.y.c1;
        return a;
    }
    // tower element -> the host's w-basis: a + b u at w^i is (a - XI0 b) w^i + b w^(i + 6)
    static typename Host::Fq12 to_host(const Fq12 &f) {
        const typename T::Fq2 *co[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
        typename Host::Fq12 h;
        const auto xi0 = from_u64<Q>(PP::XI0);
        for (int i = 0; i < 6; ++i) {
            h.c[i] = sub<Q>(co[i]->c0, mul<Q>(xi0, co[i]->c1));
            h.c[i + 6] = co[i]->c1;
        }
        return h;
    }
    static Fq12 pow_fr(const Fq12 &g, const Fr &k_mont) {
        const Fr k = from_mont<R>(k_mont);
        Fq12 acc = T::one12();
        for (int i = R::N - 1; i >= 0; --i)
            for (int b = 31; b >= 0; --b) {
                acc = T::sqr12(acc);
                if ((k.l[i] >> b) & 1) acc = T::mul12(acc, g);
            }
        return acc;
    }
    bool dev_check(const std::vector<typename Host::Pair> &pairs) {
        const int k = (int)pairs.size();
        std::vector<typename T::Line> tab((size_t)k * PP::LINES);
        std::vector<Affine<C>> P(k);
        unsigned mask = 0;
        for (int j = 0; j < k; ++j) {
            P[j] = pairs[j].p_inf ? Affine<C>::infinity() : pairs[j].p;
            if (pairs[j].q.inf) continue;
            mask |= 1u << j;
            T::prepare(to_dev(pairs[j].q), K, &tab[(size_t)j * PP::LINES]);
        }
        return T::product_is_one(tab.data(), k, mask, P.data(), K);
    }

    void run() {
        const Affine<C> G = g1_generator(), O = Affine<C>::infinity();
        const typename Host::G2 H = Host::g2_generator();
        expect(T::g2_on_twist(to_dev(H)), "the G2 generator is on the twist");
        G2A off = to_dev(H);
        off.y.c0 = add<Q>(off.y.c0, Fp<Q>::one());
        expect(!T::g2_on_twist(off), "a moved G2 point is off the twist");
        const Fq12 e_gen = T::pairing(G, to_dev(H), K);
        expect(!T::is_one12(e_gen), "non-degeneracy: e(G1, G2) != 1");
        // the tower's arithmetic against the host's polynomial ring
        {
            const Fq12 a = T::pairing(g1_mul(G, rand_fr()), to_dev(H), K), b = e_gen;
            expect(Host::mul12(to_host(a), to_host(b)).eq(to_host(T::mul12(a, b))), "mul12 agrees with the host's ring");
            expect(to_host(T::sqr12(a)).eq(Host::mul12(to_host(a), to_host(a))), "sqr12 agrees with the host's ring");
            expect(T::is_one12(T::mul12(a, T::inv12(a))), "a inv12(a) == 1");
            expect(to_host(T::frob12(a, K)).eq(Host::pow12(to_host(a), Q::MOD, Q::N)), "frob12(a) == a^p");
        }
        // bilinearity
        for (int t = 0; t < 2; ++t) {
            const Fr a = rand_fr(), b = rand_fr();
            const Fq12 lhs = T::pairing(g1_mul(G, a), to_dev(g2_mul(H, b)), K);
            expect(T::eq12(lhs, pow_fr(e_gen, mul<R>(a, b))), "bilinearity: e(aP, bQ) == e(P, Q)^(ab)");
        }
        // parity with the host pairing, value for value: e_new == host^HARD_MULTIPLE
        std::vector<Affine<C>> Ps;
        std::vector<typename Host::G2> Qs;
        std::vector<Fq12> single;
        for (int t = 0; t < 4; ++t) {
            Ps.push_back(g1_mul(G, rand_fr()));
            Qs.push_back(g2_mul(H, rand_fr()));
            single.push_back(T::pairing(Ps[t], to_dev(Qs[t]), K));
            typename Host::Fq12 h = Host::final_exponentiation(Host::miller_loop(Qs[t], Ps[t], false)), hm = h;
            for (unsigned m = 1; m < PP::HARD_MULTIPLE; ++m) hm = Host::mul12(hm, h);
            expect(to_host(single[t]).eq(hm), "parity with host/pairing.hpp: e_new(P, Q) == e_host(P, Q)^m");
        }
        // the shared loop over k prepared points against the product of the single pairings; a pair with P = O contributes 1
        for (int k = 1; k <= 3; ++k) {
            std::vector<typename T::Line> tab((size_t)k * PP::LINES);
            Fq12 want = T::one12();
            for (int j = 0; j < k; ++j) {
                T::prepare(to_dev(Qs[j]), K, &tab[(size_t)j * PP::LINES]);
                want = T::mul12(want, single[j]);
            }
            expect(T::eq12(T::final_exp(T::miller(tab.data(), k, (1u << k) - 1, Ps.data()), K), want), "multi-Miller == product of single pairings");
            if (k == 3) {
                std::vector<Affine<C>> P2(Ps.begin(), Ps.begin() + 3);
                P2[1] = O;
                expect(T::eq12(T::final_exp(T::miller(tab.data(), 3, 7u, P2.data()), K), T::mul12(single[0], single[2])), "a pair with P = O contributes 1");
                expect(T::eq12(T::final_exp(T::miller(tab.data(), 3, 5u, Ps.data()), K), T::mul12(single[0], single[2])), "a masked pair contributes 1");
            }
            if (k == 1) expect(T::product_is_one(tab.data(), 1, 1u, &O, K), "k = 1 with P = O is 1");
        }
        // verdicts against product_is_one on triples shaped like the verifier's: e(U, [z]_2) e(-V, [x]_2) e(W, [1]_2)
        const Fr z = rand_fr(), x = rand_fr();
        const typename Host::G2 Qz = g2_mul(H, z), Qx = g2_mul(H, x);
        auto triple = [&](const Affine<C> &U, const Affine<C> &nV, const Affine<C> &W) {
            return std::vector<typename Host::Pair>{{U, U.is_inf(), Qz}, {nV, nV.is_inf(), Qx}, {W, W.is_inf(), H}};
        };
        auto verdict_case = [&](const std::vector<typename Host::Pair> &pairs, bool want, const char *what) {
            const bool host = Host::product_is_one(pairs), dev = dev_check(pairs);
            expect(host == want, what);
            expect(dev == host, what);
        };
        for (int t = 0; t < 2; ++t) {
            const Fr v = rand_fr(), w = rand_fr();
            const Fr a = mul<R>(sub<R>(mul<R>(v, x), w), inverse<R>(z));           // a z - v x + w = 0
            const Affine<C> U = g1_mul(G, a), nV = g1_mul(G, neg<R>(v)), W = g1_mul(G, w);
            verdict_case(triple(U, nV, W), true, "valid triple");
            if (t == 0) {
                verdict_case(triple(g1_mul(G, add<R>(a, Fr::one())), nV, W), false, "U nudged by G");
                verdict_case(triple(U, nV, g1_mul(G, add<R>(w, Fr::one()))), false, "W nudged by G");
                verdict_case(triple(U, O, W), false, "-V replaced by O");
            }
        }
        {
            const Fr w = rand_fr();
            const Fr a = mul<R>(neg<R>(w), inverse<R>(z));                            // -V = O: a z + w = 0
            verdict_case(triple(g1_mul(G, a), O, g1_mul(G, w)), true, "valid triple with -V = O");
            verdict_case(triple(O, O, O), true, "all three points at infinity");
        }
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
