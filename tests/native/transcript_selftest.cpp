// Host build of the device transcripts (csrc/transcript.cuh -- PM_HD, plain C++ here) against their specification: the Keccak-256,
// BLAKE3 and Merlin of host/hashes.hpp, and Polymath::verifier_challenges / compute_pi_at_x1 of host/polymath.hpp.  Built and run by
// tests/test_native_transcript.py (CPU, no GPU), a second time under -fsanitize=address,undefined.
// Prints "hashes: <failures> failures of <checks>" and "<curve>: <failures> failures of <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../polymath_amd/csrc/transcript.cuh"
#include "../../polymath_amd/host/polymath.hpp"

using namespace pm;

// ~ProvingKey names it; the keys here are n / omega carriers without a device handle, so it is never called
extern "C" void pm_pk_free(pm_pk *) { abort(); }

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t next_u64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static pmhost::Bytes rand_bytes(size_t n) {
    pmhost::Bytes b(n);
    for (auto &v : b) v = (uint8_t)next_u64();
    return b;
}

static const size_t PIECES[6] = {0, 1, 7, 8, 13, 64};   // 0: the whole message in one call

template <class S>
static void feed(S &s, const uint8_t *p, size_t n, size_t piece) {
    if (!piece) { s.absorb(p, n); return; }
    for (size_t off = 0; off < n; off += piece) s.absorb(p + off, n - off < piece ? n - off : piece);
}

struct Tally {
    int fails = 0, checks = 0;
    void check(bool ok, const char *what, size_t a, size_t b) {
        ++checks;
        if (!ok) {
            ++fails;
            if (fails <= 20) printf("  FAIL %s (%zu, %zu)\n", what, a, b);
        }
    }
};

// ------------------------------------------------------------------------------------------------------------------ hashes
static void test_hashes(Tally &t) {
    // Keccak-256: every length over three blocks of the rate, the padding's edge cases (n = 0, 135 mod 136) among them
    for (size_t n = 0; n <= 3 * 136 + 2; ++n) {
        const pmhost::Bytes msg = rand_bytes(n), want = pmhost::keccak256(msg);
        for (size_t piece : PIECES) {
            fs::Keccak256Stream s;
            s.init();
            feed(s, msg.data(), n, piece);
            uint8_t got[32];
            s.finish(got);
            t.check(!memcmp(got, want.data(), 32), "keccak256", n, piece);
        }
    }
    // BLAKE3: one chunk, balanced and unbalanced trees, the stack merges
    const size_t b3_lens[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 5121, 7 * 1024 + 1};
    for (size_t n : b3_lens) {
        const pmhost::Bytes msg = rand_bytes(n), want = pmhost::blake3(msg);
        for (size_t piece : PIECES) {
            fs::Blake3Stream s;
            s.init();
            feed(s, msg.data(), n, piece);
            uint8_t got[32];
            s.finish(got);
            t.check(!memcmp(got, want.data(), 32), "blake3", n, piece);
        }
    }
    // Merlin: two appends, then two challenges of 64 bytes; the first message's length walks across the STROBE rate twice
    struct MerlinFeed {
        fs::Merlin *m;
        void absorb(const uint8_t *p, size_t n) { fs::absorb_bytes(m->s, p, n); }
    };
    for (size_t n = 0; n <= 2 * 166 + 2; ++n) {
        const pmhost::Bytes m1 = rand_bytes(n), m2 = rand_bytes(n / 3 + 5);
        pmhost::MerlinTranscript h("polymath");
        h.append_message("public_inputs", m1.data(), m1.size());
        h.append_message("commitments", m2.data(), m2.size());
        uint8_t w1[64], w2[64];
        h.challenge_bytes("x1", w1, 64);
        h.challenge_bytes("x2", w2, 64);
        for (size_t piece : PIECES) {
            fs::Merlin m;
            m.init((const uint8_t *)"polymath", 8);
            MerlinFeed f{&m};
            m.begin_message((const uint8_t *)"public_inputs", 13, (uint32_t)m1.size());
            feed(f, m1.data(), m1.size(), piece);
            m.begin_message((const uint8_t *)"commitments", 11, (uint32_t)m2.size());
            feed(f, m2.data(), m2.size(), piece);
            uint64_t g1[8], g2[8];
            m.challenge_bytes64((const uint8_t *)"x1", 2, g1);
            m.challenge_bytes64((const uint8_t *)"x2", 2, g2);
            t.check(!memcmp(g1, w1, 64) && !memcmp(g2, w2, 64), "merlin", n, piece);
        }
    }
}

// ------------------------------------------------------------------------------------------------- the verifier's challenges
template <class C>
struct Suite {
    typedef typename C::FrP R;
    typedef Fp<R> Fr;
    typedef pmhost::FrOps<C> F;
    static constexpr size_t NB = 4 * C::FqP::N;
    Tally t;
    pmhost::VerifyingKeyT<C> vk;
    fs::FsVk<C> dvk;

    Suite() {
        vk.n = 256;                                     // >= 2 m0 for every m0 below
        vk.m0 = 0;
        vk.sigma = vk.n + 3;
        Fr w;
        for (int i = 0; i < 8; ++i) w.l[i] = C::ROOT_MONT[i];
        for (int i = 8; i < C::TWO_ADICITY; ++i) w = sqr<R>(w);
        vk.omega = w;
        dvk.n = vk.n;
        dvk.sigma = vk.sigma;
        dvk.omega = vk.omega;
        dvk.n_inv = F::inv(F::from_u64(vk.n));
    }
    static Fr rand_fr() {   // < 2^(BITS - 1) < r
        Fr v;
        for (int i = 0; i < 8; i += 2) { const uint64_t x = next_u64(); v.l[i] = (uint32_t)x; v.l[i + 1] = (uint32_t)(x >> 32); }
        v.l[7] &= (1u << (R::BITS - 1 - 224)) - 1;
        return to_mont<R>(v);
    }
    static Fr r_minus_1() { return F::neg(Fr::one()); }
    static void canonical_bytes(const Fr &mont, uint8_t out[32]) { F::to_le_bytes(mont, out); }

    template <int KIND, class T>
    void one(const std::vector<Fr> &inputs, const uint8_t a_at_bytes[32], size_t tag) {
        typedef pmhost::Polymath<C, T> PMath;
        const pmhost::Bytes a_rec = rand_bytes(NB), c_rec = rand_bytes(NB);
        fs::FsChallenges<C> got;
        Fr a_at_got;
        const bool ok = fs::fs_verifier_challenges<C, KIND>(dvk, inputs.data(), inputs.size(), a_rec.data(), c_rec.data(), a_at_bytes, &got, &a_at_got);
        Fr a_at;
        bool host_ok = true;
        try {
            a_at = F::from_le_bytes_canonical(a_at_bytes);
        } catch (const std::runtime_error &) { host_ok = false; }
        t.check(ok == host_ok, "a_at_x1 canonical", inputs.size(), tag);
        if (!host_ok || !ok) return;
        const typename PMath::Challenges want = PMath::verifier_challenges(vk, inputs, a_rec.data(), c_rec.data(), a_at);
        t.check(got.x1.eq(want.x1) && a_at_got.eq(a_at), "x1", inputs.size(), tag);
        t.check(got.c_at_x1.eq(want.c_at_x1), "c_at_x1", inputs.size(), tag);
        t.check(got.x2.eq(want.x2), "x2", inputs.size(), tag);
    }

    template <int KIND, class T>
    void kind() {
        const size_t sizes[] = {0, 1, 2, 3, 27, 28, 59, 60};
        for (size_t n_inputs : sizes) {
            uint8_t b[32];
            for (int rep = 0; rep < 3; ++rep) {         // random inputs, random a_at_x1
                std::vector<Fr> in(n_inputs);
                for (auto &v : in) v = rand_fr();
                canonical_bytes(rand_fr(), b);
                one<KIND, T>(in, b, rep);
            }
            std::vector<Fr> edge(n_inputs);             // inputs 0, r - 1, random, ...
            for (size_t i = 0; i < n_inputs; ++i) edge[i] = i % 3 == 0 ? Fr::zero() : i % 3 == 1 ? r_minus_1() : rand_fr();
            memset(b, 0, 32);
            one<KIND, T>(edge, b, 10);                  // a_at_x1 = 0
            canonical_bytes(r_minus_1(), b);
            one<KIND, T>(edge, b, 11);                  // a_at_x1 = r - 1
            memcpy(b, R::MOD, 32);
            one<KIND, T>(edge, b, 12);                  // a_at_x1 = r: refused
            memset(b, 0xff, 32);
            one<KIND, T>(edge, b, 13);                  // 2^256 - 1: refused
        }
    }

    // the Lagrange part alone with x1 on the domain: the term with x1 = omega^k is the zero-inverse term
    void lagrange() {
        typedef pmhost::Polymath<C, pmhost::Keccak256Transcript<C>> PMath;
        const size_t sizes[] = {0, 1, 2, 3, 27, 28, 59, 60};
        pmhost::ProvingKey<C> view;
        view.n = vk.n;
        view.omega = vk.omega;
        for (size_t n_inputs : sizes) {
            const size_t m0 = n_inputs + 1;
            std::vector<Fr> in(n_inputs), pub{Fr::one()};
            for (auto &v : in) v = rand_fr();
            pub.insert(pub.end(), in.begin(), in.end());
            const Fr xs[5] = {Fr::one(), F::pow(vk.omega, m0), F::pow(vk.omega, 2 * m0 - 1), F::pow(vk.omega, 2 * m0), rand_fr()};
            for (int k = 0; k < 5; ++k) {
                const Fr extra = k == 3 ? Fr::zero() : rand_fr(), y1_gamma = rand_fr();
                Fr extra_inv;
                const Fr got = mul<R>(fs::fs_lagrange_sum<C>(dvk, in.data(), n_inputs, xs[k], extra, &extra_inv), y1_gamma);
                t.check(got.eq(PMath::compute_pi_at_x1(view, pub, xs[k], y1_gamma)), "pi_at_x1", n_inputs, k);
                t.check(extra_inv.eq(F::inv(extra)), "1 / extra", n_inputs, k);
            }
        }
    }

    void run(const char *name) {
        kind<fs::KIND_MERLIN, pmhost::MerlinFieldTranscript<C>>();
        kind<fs::KIND_KECCAK256, pmhost::Keccak256Transcript<C>>();
        kind<fs::KIND_BLAKE3, pmhost::Blake3Transcript<C>>();
        lagrange();
        printf("%s: %d failures of %d\n", name, t.fails, t.checks);
    }
};

int main() {
    Tally h;
    test_hashes(h);
    printf("hashes: %d failures of %d\n", h.fails, h.checks);
    Suite<BlsCurve> bls;
    bls.run("bls12_381");
    Suite<BnCurve> bn;
    bn.run("bn254");
    return h.fails || bls.t.fails || bn.t.fails ? 1 : 0;
}
