// CPU-only test of the proving-key relation check's host mirror (polymath_amd/host/key_check.hpp): no GPU, no library link.
//   key_check_selftest [--quick]
// Keys are made here by a literal restatement of generate_proving_key (generator.rs:66-157) with SAPMatrices::u / w
// (common.rs:138-207) element by element -- not by the sparse row sums the mirror and the device use -- at n = 8 and n = 16 on both
// curves (--quick: n = 8 on BLS12-381 only, for the sanitizer build).  Every valid key passes; every tamper is refused with the
// relation it breaks.  The ChaCha12 text reproduces the published 12-round vector and equals StdRng's block.
#include <cstdio>
#include <functional>
#include <string>
#include <thread>

#include "../../polymath_amd/host/key_check.hpp"
using namespace pmhost;

static int fails = 0, checks = 0;
static void check(bool ok, const std::string &what) {
    ++checks;
    if (!ok) { ++fails; printf("FAILED %s\n", what.c_str()); }
}

template <class C>
struct Circuit {
    uint64_t m0, mw, nr;
    CsrHost a, b, c;
};

// rows with two or three entries a matrix; row 0 of A repeats a column (m_at reads the first entry only); the last witness column is
// in no row, so its uj_wj_lcs entry is the point at infinity
template <class C>
static Circuit<C> make_circuit(uint64_t seed, uint64_t m0, uint64_t mw, uint64_t nr) {
    typedef FrOps<C> F;
    StdRng rng = StdRng::seed_from_u64(seed);
    Circuit<C> k{m0, mw, nr, {}, {}, {}};
    const uint64_t used = m0 + mw - 1;
    auto entry = [&](CsrHost &m, uint64_t col) {
        const typename F::Fr v = F::rand(rng);
        m.col.push_back((uint32_t)col);
        m.val.insert(m.val.end(), (const uint64_t *)v.l, (const uint64_t *)v.l + 4);
    };
    for (uint64_t r = 0; r < nr; ++r) {
        entry(k.a, rng.next_u32() % used); entry(k.a, (r + 1) % used);
        if (r == 0) entry(k.a, k.a.col[0]);
        entry(k.b, rng.next_u32() % used); entry(k.b, 0);
        entry(k.c, rng.next_u32() % used); entry(k.c, (r + 2) % used); entry(k.c, rng.next_u32() % m0);
        k.a.rowptr.push_back(k.a.col.size()); k.b.rowptr.push_back(k.b.col.size()); k.c.rowptr.push_back(k.c.col.size());
    }
    return k;
}

template <class C>
static typename FrOps<C>::Fr m_at(const CsrHost &m, uint64_t i, uint64_t j) {   // common.rs:100-105
    for (uint64_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e)
        if (m.col[e] == j) { typename FrOps<C>::Fr v; memcpy(v.l, &m.val[4 * e], 32); return v; }
    return FrOps<C>::zero();
}
template <class C>
static typename FrOps<C>::Fr sap_u(const Circuit<C> &k, uint64_t i, uint64_t j) {   // common.rs:138-172
    typedef FrOps<C> F;
    const uint64_t m0 = k.m0, m = k.m0 + k.mw, n = k.nr;
    const typename F::Fr zero = F::zero(), one = F::one();
    if (i == 0 && j == 0) return F::add(one, one);
    if (i < m0 && j == 0) return one;
    if (i < m0 && j == i) return one;
    if (i < m0) return zero;
    if (i == m0 && j == 0) return zero;
    if (i < 2 * m0 && j == 0) return one;
    if (i < 2 * m0 && j == i - m0) return F::neg(one);
    if (i < 2 * m0) return zero;
    if (j < m0) return zero;
    if (i < 2 * m0 + n && j < m0 + m) return F::add(m_at<C>(k.a, i - 2 * m0, j - m0), m_at<C>(k.b, i - 2 * m0, j - m0));
    if (i < 2 * m0 + 2 * n && j < m0 + m) return F::sub(m_at<C>(k.a, i - 2 * m0 - n, j - m0), m_at<C>(k.b, i - 2 * m0 - n, j - m0));
    return zero;
}
template <class C>
static typename FrOps<C>::Fr sap_w(const Circuit<C> &k, uint64_t i, uint64_t j) {   // common.rs:175-207
    typedef FrOps<C> F;
    const uint64_t m0 = k.m0, m = k.m0 + k.mw, n = k.nr;
    const typename F::Fr zero = F::zero(), one = F::one(), four = F::from_u64(4);
    if (i < m0 && j == i + m0) return four;
    if (i < m0 && j == i + m0 + m) return one;
    if (i < m0) return zero;
    if (i < 2 * m0 && j == i + m) return one;
    if (i < 2 * m0) return zero;
    if (j < m0) return zero;
    if (i < 2 * m0 + n && j < m0 + m) return F::mul(m_at<C>(k.c, i - 2 * m0, j - m0), four);
    if (i < 2 * m0 + n && j == i + m) return one;
    if (i < 2 * m0 + n) return zero;
    if (i < 2 * m0 + 2 * n && j == i - n + m) return one;
    return zero;
}

template <class C>
static G1Point<C> g1_of(const typename FrOps<C>::Fr &s) {
    pm::Affine<C> G;
    for (int i = 0; i < C::FqP::N; ++i) { G.x.l[i] = C::GX_MONT[i]; G.y.l[i] = C::GY_MONT[i]; }
    const typename FrOps<C>::Fr c = pm::from_mont<typename C::FrP>(s);
    const pm::XYZZ<C> p = pm::xyzz_mul_words<C>(G, c.l, 8);
    return G1Point<C>{pm::xyzz_to_affine<C>(p), p.is_identity()};
}
template <class C>
static G1Point<C> doubled(const G1Point<C> &g) {
    if (g.inf) return g;
    const pm::XYZZ<C> p = pm::xyzz_dbl_affine<C>(g.p);
    return G1Point<C>{pm::xyzz_to_affine<C>(p), p.is_identity()};
}

// generate_proving_key with the trapdoors given (generator.rs:66-157)
template <class C>
static KeyCheckInput<C> generate(const Circuit<C> &k, const typename FrOps<C>::Fr &x, const typename FrOps<C>::Fr &z) {
    typedef FrOps<C> F;
    typedef typename F::Fr Fr;
    typedef typename PairingOf<C>::type Pairing;
    KeyCheckInput<C> out;
    out.m0 = k.m0; out.mw = k.mw; out.nr = k.nr; out.a = k.a; out.b = k.b; out.c = k.c;
    uint64_t n = 1;
    unsigned log_n = 0;
    while (n < 2 * (k.m0 + k.nr)) { n <<= 1; ++log_n; }
    const uint64_t sigma = n + 3, m = 2 * k.m0 + k.mw + k.nr + k.m0;   // m: SAP columns
    Fr omega;
    for (int i = 0; i < C::FrP::N; ++i) omega.l[i] = C::ROOT_MONT[i];
    for (unsigned i = log_n; i < (unsigned)C::TWO_ADICITY; ++i) omega = F::mul(omega, omega);
    const Fr y = F::pow(x, sigma), y_inv = F::inv(y);
    const Fr y_alpha = F::pow(y_inv, 3), y_to_minus_alpha = F::pow(y, 3), y_gamma = F::pow(y_inv, 5);
    const Fr zh = F::sub(F::pow(x, n), F::one());
    auto gen = [&](int which, uint64_t max_index, const std::function<Fr(uint64_t)> &f) {
        for (uint64_t j = 0; j <= max_index; ++j) out.vec[which].push_back(g1_of<C>(f(j)));
    };
    gen(PM_X_POWERS, n, [&](uint64_t j) { return F::pow(x, j); });
    gen(PM_X_POWERS_Y_ALPHA, 2, [&](uint64_t j) { return F::mul(F::pow(x, j), y_alpha); });
    gen(PM_X_POWERS_Y_GAMMA, 1, [&](uint64_t j) { return F::mul(F::pow(x, j), y_gamma); });
    gen(PM_X_POWERS_Y_GAMMA_Z, 2 * (n - 1) + sigma * 8, [&](uint64_t j) { return F::mul(F::mul(F::pow(x, j), y_gamma), z); });
    gen(PM_X_POWERS_ZH_BY_Y_ALPHA, n - 2, [&](uint64_t j) { return F::mul(F::mul(F::pow(x, j), zh), y_to_minus_alpha); });
    std::vector<Fr> l_at_x(n);   // evaluate_all_lagrange_coefficients: L_i(x) = (x^n - 1) omega^i / (n (x - omega^i))
    Fr wi = F::one();
    for (uint64_t i = 0; i < n; ++i, wi = F::mul(wi, omega))
        l_at_x[i] = F::mul(F::mul(zh, wi), F::inv(F::mul(F::from_u64(n), F::sub(x, wi))));
    gen(PM_UJ_WJ_LCS_BY_Y_ALPHA, m - k.m0 - 1, [&](uint64_t j) {
        Fr uj = F::zero(), wj = F::zero();
        for (uint64_t i = 0; i < n; ++i) {
            uj = F::add(uj, F::mul(l_at_x[i], sap_u<C>(k, i, j + k.m0)));
            wj = F::add(wj, F::mul(l_at_x[i], sap_w<C>(k, i, j + k.m0)));
        }
        return F::mul(F::add(F::mul(uj, y_gamma), wj), y_to_minus_alpha);
    });
    out.vk.one_g1 = g1_of<C>(F::one());
    out.vk.one_g2 = Pairing::g2_generator();
    const Fr xc = pm::from_mont<typename C::FrP>(x), zc = pm::from_mont<typename C::FrP>(z);
    out.vk.x_g2 = Pairing::g2_mul(out.vk.one_g2, xc.l, 8);
    out.vk.z_g2 = Pairing::g2_mul(out.vk.one_g2, zc.l, 8);
    out.vk.n = n; out.vk.m0 = k.m0; out.vk.sigma = sigma; out.vk.omega = omega;
    return out;
}

template <class C>
struct Case {
    std::string name;
    KeyCheckInput<C> key;
    int expect;
};

template <class C>
static void run_shape(const char *curve, uint64_t m0, uint64_t mw, uint64_t nr) {
    typedef FrOps<C> F;
    StdRng rng = StdRng::seed_from_u64(1000 * m0 + nr);
    const typename F::Fr x = F::rand(rng), z = F::rand(rng), x2 = F::rand(rng), z2 = F::rand(rng);
    const Circuit<C> circuit = make_circuit<C>(7, m0, mw, nr), other = make_circuit<C>(8, m0, mw, nr);
    const KeyCheckInput<C> good = generate<C>(circuit, x, z);
    std::vector<Case<C>> cases;
    auto add = [&](const std::string &name, int expect, const std::function<void(KeyCheckInput<C> &)> &edit) {
        cases.push_back(Case<C>{name, good, expect});
        edit(cases.back().key);
    };
    add("valid", KEY_REL_NONE, [](KeyCheckInput<C> &) {});
    add("x_powers_g1: two adjacent entries swapped", KEY_REL_RATIO, [&](KeyCheckInput<C> &k) {
        auto &v = k.vec[PM_X_POWERS];
        std::swap(v[v.size() / 2], v[v.size() / 2 + 1]);
    });
    const int first_expect[6] = {KEY_REL_FIRST, KEY_REL_RATIO + 1, KEY_REL_RATIO + 2, KEY_REL_RATIO + 3, KEY_REL_RATIO + 4, KEY_REL_LCS};
    const int last_expect[6] = {KEY_REL_RATIO, KEY_REL_RATIO + 1, KEY_REL_RATIO + 2, KEY_REL_RATIO + 3, KEY_REL_RATIO + 4, KEY_REL_LCS};
    const int whole_expect[6] = {KEY_REL_FIRST, KEY_REL_ANCHOR + 2, KEY_REL_ANCHOR + 1, KEY_REL_ANCHOR + 0, KEY_REL_ANCHOR + 3, KEY_REL_LCS};
    for (int v = 0; v < PM_NUM_BASE_VECS; ++v) {
        add(std::string(KEY_VEC_NAMES[v]) + ": first entry doubled", first_expect[v], [v](KeyCheckInput<C> &k) { k.vec[v].front() = doubled<C>(k.vec[v].front()); });
        add(std::string(KEY_VEC_NAMES[v]) + ": last entry doubled", last_expect[v], [v](KeyCheckInput<C> &k) { k.vec[v].back() = doubled<C>(k.vec[v].back()); });
        add(std::string(KEY_VEC_NAMES[v]) + ": every entry doubled", whole_expect[v], [v](KeyCheckInput<C> &k) { for (auto &g : k.vec[v]) g = doubled<C>(g); });
    }
    const uint64_t m = m0 + mw, Lz = 2 * m0 + mw + nr;
    const uint64_t cols[4] = {0, m - 1, m, Lz - 1};
    const char *col_names[4] = {"first R1CS column", "last R1CS column", "first y column", "last y column"};
    for (int t = 0; t < 4; ++t)
        add(std::string("uj_wj_lcs entry replaced: ") + col_names[t], KEY_REL_LCS, [&, t](KeyCheckInput<C> &k) { k.vec[PM_UJ_WJ_LCS_BY_Y_ALPHA][cols[t]] = g1_of<C>(F::from_u64(7)); });
    add("x_g2 and z_g2 swapped", KEY_REL_RATIO, [](KeyCheckInput<C> &k) { std::swap(k.vk.x_g2, k.vk.z_g2); });
    add("vk of another x", KEY_REL_RATIO, [&](KeyCheckInput<C> &k) { k.vk = generate<C>(circuit, x2, z).vk; });
    add("vk of another z", KEY_REL_ANCHOR, [&](KeyCheckInput<C> &k) { k.vk = generate<C>(circuit, x, z2).vk; });
    add("matrices of another circuit of the same shape", KEY_REL_LCS, [&](KeyCheckInput<C> &k) { k.a = other.a; k.b = other.b; k.c = other.c; });
    check(good.vec[PM_UJ_WJ_LCS_BY_Y_ALPHA][m - 1].inf, std::string(curve) + ": the unused witness column's entry is the point at infinity");

    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(rng.next_u32());
    std::vector<int> got(cases.size(), -2);
    std::vector<std::thread> pool;
    const size_t workers = std::min<size_t>(8, cases.size());
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([&, w] { for (size_t i = w; i < cases.size(); i += workers) got[i] = key_check_host<C>(cases[i].key, seed); });
    for (auto &t : pool) t.join();
    for (size_t i = 0; i < cases.size(); ++i)
        check(got[i] == cases[i].expect, std::string(curve) + " n=" + std::to_string(good.vk.n) + " " + cases[i].name + ": got '" + key_relation_text(got[i]) +
                                             "', expected '" + key_relation_text(cases[i].expect) + "'");
    printf("%s n=%llu: %zu keys checked\n", curve, (unsigned long long)good.vk.n, cases.size());
}

static void chacha_vectors() {
    // ChaCha12, key 0, nonce 0, block 0: 9bf49a6a0755f953811fce125f2683d5 0429c3bb49e074147e0089a52eae155f ... (the published 12-round
    // vector tests/test_host_mirror.py pins for StdRng)
    const uint32_t zero_key[8] = {0}, tail[4] = {0, 0, 0, 0};
    uint32_t out[16];
    chacha_block(zero_key, tail, 12, out);
    const uint8_t expect[16] = {0x9b, 0xf4, 0x9a, 0x6a, 0x07, 0x55, 0xf9, 0x53, 0x81, 0x1f, 0xce, 0x12, 0x5f, 0x26, 0x83, 0xd5};
    check(memcmp(out, expect, 16) == 0, "ChaCha12 zero-key block 0");
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(17 * i + 3);
    StdRng rng = StdRng::from_seed(seed);
    bool same = true;
    for (uint64_t block = 0; block < 5; ++block) {
        uint32_t w[4];
        chacha12_weight(rng.key, block, w);
        for (int i = 0; i < 16; ++i) {
            const uint32_t word = rng.next_u32();
            if (i < 4) same = same && word == w[i];
        }
    }
    check(same, "chacha12_weight(i) == the first four words of StdRng's block i");
    uint32_t w[4];
    chacha12_weight(rng.key, ((uint64_t)1 << 32) + 5, w);
    const uint32_t tail_hi[4] = {5, 1, 0, 0};
    chacha_block(rng.key, tail_hi, 12, out);
    check(memcmp(w, out, 16) == 0, "chacha12_weight: the index's high word is counter word 13");
}

int main(int argc, char **argv) {
    const bool quick = argc > 1 && std::string(argv[1]) == "--quick";
    chacha_vectors();
    run_shape<pm::BlsCurve>("bls12_381", 1, 3, 3);         // n = 8
    if (!quick) {
        run_shape<pm::BlsCurve>("bls12_381", 2, 4, 5);     // n = 16
        run_shape<pm::BnCurve>("bn254", 1, 3, 3);
        run_shape<pm::BnCurve>("bn254", 2, 4, 5);
    }
    printf("key check selftest: %d failures of %d\n", fails, checks);
    return fails ? 1 : 0;
}
