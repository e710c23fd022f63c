// Host build of the batch prover's device glue (csrc/transcript.cuh: fs_prover_x1 / fs_prover_x2; csrc/g1_record.cuh: g1_record_words;
// csrc/batch_row.cuh: fill_batch_row -- PM_HD, plain C++ here) against its specification: Polymath::glue_x1 / glue_x2, ser_g1 and
// Proof::to_bytes of host/polymath.hpp, and the numerator constants restated with the host's field operations.  Built and run by
// tests/test_native_prover_glue.py (CPU, no GPU), a second time under -fsanitize=address,undefined.
// Prints "<curve>: <failures> failures of <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polymath_amd/csrc/transcript.cuh"
#include "../../polymath_amd/csrc/g1_record.cuh"
#include "../../polymath_amd/csrc/batch_row.cuh"
#include "../../polymath_amd/host/polymath.hpp"

using namespace pm;

// ~ProvingKey names it; the keys here are n / omega carriers without a device handle, so it is never called
extern "C" void pm_pk_free(pm_pk *) { abort(); }

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Tally {
    int fails = 0, checks = 0;
    void check(bool ok, const char *what, size_t a, size_t b, size_t c) {
        ++checks;
        if (!ok) {
            ++fails;
            if (fails <= 20) printf("  FAIL %s (kind %zu, m0 %zu, case %zu)\n", what, a, b, c);
        }
    }
};

template <class P>
static Fp<P> rand_fp() {   // < 2^(BITS - 1) < the modulus, Montgomery
    Fp<P> v;
    for (int i = 0; i < P::N; ++i) v.l[i] = (uint32_t)next_u64();
    v.l[P::N - 1] &= (1u << (P::BITS - 1 - 32 * (P::N - 1))) - 1;
    return to_mont<P>(v);
}

enum { CASE_ONE = 0, CASE_FIRST_RANDOM, CASE_A_INF, CASE_C_INF, CASE_RA_ZERO, CASE_X1_ON_DOMAIN, N_CASES };

template <class C>
struct Suite {
    typedef typename C::FrP R;
    typedef typename C::FqP Q;
    typedef Fp<R> Fr;
    typedef pmhost::FrOps<C> F;
    static constexpr int NW = Q::N;
    static constexpr size_t NB = 4 * NW;
    Tally t;
    pmhost::ProvingKey<C> key;
    fs::FsVk<C> vk;

    Suite() {
        key.n = 256;                                    // >= 2 m0 for every m0 below
        key.sigma = key.n + 3;
        Fr w;
        for (int i = 0; i < 8; ++i) w.l[i] = C::ROOT_MONT[i];
        for (int i = 8; i < C::TWO_ADICITY; ++i) w = sqr<R>(w);
        key.omega = w;
        vk.n = key.n;
        vk.sigma = key.sigma;
        vk.omega = key.omega;
        vk.n_inv = F::inv(F::from_u64(key.n));
    }

    static pmhost::G1Point<C> rand_point(bool inf) {    // ser_g1 reads coordinates, not the curve equation
        pmhost::G1Point<C> g;
        g.p.x = inf ? Fp<Q>::zero() : rand_fp<Q>();
        g.p.y = inf ? Fp<Q>::zero() : rand_fp<Q>();
        g.inf = inf;
        return g;
    }
    static bool record_equals(const pmhost::G1Point<C> &g, const uint32_t *rec) {
        pmhost::Bytes want;
        pmhost::ser_g1<C>(g, want);
        return want.size() == NB && !memcmp(want.data(), rec, NB);
    }

    // fill_batch_row against the formulas of prover.rs:145-197 written with the host's operations
    bool row_equals(const Fr &x1, const Fr &x2, const Fr ra[2], const Fr &a_at, const Fr &c_at, int levels) {
        typedef typename Radix28<R>::RR RR;
        BatchRow<R> got;
        memset((void *)&got, 0, sizeof(got));
        fill_batch_row<R>(got, x1, x2, ra, a_at, c_at, levels);
        const Fr two = F::add(Fr::one(), Fr::one());
        const NumConsts<R> &nc = got.nc;
        bool ok = got.x1.eq(x1) && nc.x2.eq(x2) && nc.r0.eq(ra[0]) && nc.r1.eq(ra[1]) && nc.x2r0.eq(F::mul(x2, ra[0])) && nc.x2r1.eq(F::mul(x2, ra[1]));
        ok = ok && nc.b2[0].eq(F::add(ra[0], F::mul(x2, F::mul(ra[0], ra[0]))));
        ok = ok && nc.b2[1].eq(F::add(ra[1], F::mul(x2, F::mul(two, F::mul(ra[0], ra[1])))));
        ok = ok && nc.b2[2].eq(F::mul(x2, F::mul(ra[1], ra[1])));
        ok = ok && nc.two_x2_r0.eq(F::mul(two, F::mul(x2, ra[0]))) && nc.two_x2_r1.eq(F::mul(two, F::mul(x2, ra[1])));
        ok = ok && nc.minus_const.eq(F::neg(F::add(a_at, F::mul(x2, c_at))));
        Fr k;
        for (int i = 0; i < R::N; ++i) k.l[i] = RR::STD2INT[i];
        const Fr mult[4] = {x1, x2, nc.two_x2_r0, nc.two_x2_r1};
        const F28<RR> *got28[4] = {&got.m28.x1, &got.m28.x2, &got.m28.two_x2_r0, &got.m28.two_x2_r1};
        for (int j = 0; j < 4; ++j) {
            const F28<RR> want = f28_unpack<RR>(F::mul(mult[j], k).l);
            ok = ok && !memcmp(&want, got28[j], sizeof(want));
        }
        Fr p = x1;
        for (int l = 0; l < 8; ++l) {
            ok = ok && got.xp[l].eq(l <= levels ? p : Fr::zero());
            p = F::pow(p, DIV_L);
        }
        return ok;
    }

    template <int KIND, class T>
    void one(size_t m0, int which) {
        typedef pmhost::Polymath<C, T> PMath;
        std::vector<Fr> inst(m0);
        for (auto &v : inst) v = rand_fp<R>();
        if (which != CASE_FIRST_RANDOM) inst[0] = Fr::one();
        pmhost::Proof<C> proof;
        proof.a_g1 = rand_point(which == CASE_A_INF);
        proof.c_g1 = rand_point(which == CASE_C_INF);
        proof.d_g1 = rand_point(false);
        Fr ra[2] = {rand_fp<R>(), rand_fp<R>()};
        if (which == CASE_RA_ZERO) ra[0] = ra[1] = Fr::zero();
        const Fr u_at = rand_fp<R>();

        // the records
        uint32_t rec[3][NW];
        g1_record_words<C>(proof.a_g1.p, proof.a_g1.inf, rec[0]);
        g1_record_words<C>(proof.c_g1.p, proof.c_g1.inf, rec[1]);
        g1_record_words<C>(proof.d_g1.p, proof.d_g1.inf, rec[2]);
        t.check(record_equals(proof.a_g1, rec[0]) && record_equals(proof.c_g1, rec[1]) && record_equals(proof.d_g1, rec[2]), "records", KIND, m0, which);

        // x1 and the powers of y1
        typename PMath::Glue g;
        PMath::glue_x1(g, key, inst, proof);
        fs::FsProverState<C, KIND> s;
        fs::fs_prover_x1<C, KIND>(vk, inst.data(), m0, (const uint8_t *)rec[0], (const uint8_t *)rec[1], &s);
        t.check(s.x1.eq(g.x1) && s.y1_alpha.eq(g.y1_alpha) && s.y1_gamma.eq(g.y1_gamma), "x1", KIND, m0, which);
        if (which == CASE_X1_ON_DOMAIN) {   // the hash cannot be steered: both sides continue from x1 = omega^m0, a term of the Lagrange sum
            g.x1 = s.x1 = F::pow(key.omega, m0);
            const Fr y1_inv = F::inv(F::pow(g.x1, key.sigma));
            g.y1_alpha = s.y1_alpha = F::pow(y1_inv, 3);
            g.y1_gamma = s.y1_gamma = F::pow(y1_inv, 5);
        }

        // a(x1), pi(x1), c(x1), x2
        PMath::glue_x2(g, key, inst, ra, u_at, proof);
        fs::FsProverOut<C> o;
        fs::fs_prover_x2<C, KIND>(vk, inst.data(), m0, &s, u_at, ra, &o);
        t.check(o.a_at_x1.eq(proof.a_at_x1) && o.c_at_x1.eq(g.c_at_x1) && o.x2.eq(g.x2) &&
                    o.pi_at_x1.eq(PMath::compute_pi_at_x1(key, inst, g.x1, g.y1_gamma)),
                "x2", KIND, m0, which);

        // the proof's bytes as the kernels lay them out: a_g1 | c_g1 | a_at_x1 | d_g1
        uint8_t bytes[3 * NB + 32];
        memcpy(bytes, rec[0], NB);
        memcpy(bytes + NB, rec[1], NB);
        uint64_t w[4];
        fs::fr_canonical_words<C>(o.a_at_x1, w);
        memcpy(bytes + 2 * NB, w, 32);
        memcpy(bytes + 2 * NB + 32, rec[2], NB);
        const pmhost::Bytes want = proof.to_bytes();
        t.check(want.size() == sizeof(bytes) && !memcmp(want.data(), bytes, sizeof(bytes)), "proof bytes", KIND, m0, which);

        // the phase-3 record, at every level count of the division scan
        t.check(row_equals(s.x1, o.x2, ra, o.a_at_x1, o.c_at_x1, (int)((m0 + which) % 7)), "batch row", KIND, m0, which);
    }

    template <int KIND, class T>
    void kind() {
        const size_t sizes[] = {1, 2, 3, 7, 8, 9, 12, 20};   // 2 m0 straddles FS_INV_CHUNK at 8
        for (size_t m0 : sizes)
            for (int which = 0; which < N_CASES; ++which) one<KIND, T>(m0, which);
    }

    void run(const char *name) {
        kind<fs::KIND_MERLIN, pmhost::MerlinFieldTranscript<C>>();
        kind<fs::KIND_KECCAK256, pmhost::Keccak256Transcript<C>>();
        kind<fs::KIND_BLAKE3, pmhost::Blake3Transcript<C>>();
        printf("%s: %d failures of %d\n", name, t.fails, t.checks);
    }
};

int main() {
    Suite<BlsCurve> bls;
    bls.run("bls12_381");
    Suite<BnCurve> bn;
    bn.run("bn254");
    return bls.t.fails || bn.t.fails ? 1 : 0;
}
