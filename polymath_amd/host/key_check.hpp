// Is this key what generate_proving_key (generator.rs:24-167) would have produced for SOME (x, z)?  The decision of
// pm_pk_load_bytes' PM_KEY_CHECK_RELATIONS on the CPU: naive sums and the host pairing (pairing.hpp), over a parsed key.  This header
// is the specification -- csrc/key_check.hip makes the same decision with MSMs, two inverse transforms and one pairing launch -- and
// the two share what is stated here: the relations and their order, their texts, the weight indices and the indices into
// T = x_powers_y_gamma_z_g1.
//
// A proving key carries its vk ([1]_1, [1]_2, [x]_2, [z]_2) and the SAP matrices, and every base vector is a fixed function of x, z and
// the matrices.  With a = MINUS_ALPHA = 3, g = MINUS_GAMMA = 5, s = sigma = n + 3, y = x^s:
//   x_powers_g1[j]               = [x^j]_1                       j <= n
//   x_powers_y_alpha_g1[j]       = [x^(j - a s)]_1               j <= 2
//   x_powers_y_gamma_g1[j]       = [x^(j - g s)]_1               j <= 1
//   T[j]                         = [x^(j - g s) z]_1             j <= 2(n - 1) + (a + g) s
//   x_powers_zh_by_y_alpha_g1[j] = [x^j (x^n - 1) x^(a s)]_1     j <= n - 2
//   uj_wj_lcs_by_y_alpha_g1[j]   = [u_j(x) x^((a - g) s) + w_j(x) x^(a s)]_1,   j a SAP column >= m0 (common.rs:138-207)
// Every check is  e(A, [1]_2) e(B, [x]_2) e(C, [z]_2) = 1  with the G2 points of the key's own vk.  In this order (the first that fails
// is the one reported):
//    0      x_powers_g1[0] == vk.one_g1                                                       (a comparison, no pairing)
//    1-5    ratio, per power vector V of length L in pm_base_vec order, weights rho_i:
//             e(sum_{i<L-1} rho_i V[i+1], [1]_2) = e(sum_{i<L-1} rho_i V[i], [x]_2)
//    6-9    anchors (with the ratios they fix every vector absolutely):
//             e(T[g s], [1]_2) = e(one_g1, [z]_2)
//             e(x_powers_y_gamma_g1[0], [z]_2) = e(T[0], [1]_2)
//             e(x_powers_y_alpha_g1[0], [z]_2) = e(T[(g - a) s], [1]_2)
//             e(x_powers_zh_by_y_alpha_g1[0], [z]_2) = e(T[n + (a + g) s] - T[(a + g) s], [1]_2)
//    10     the circuit-specific vector, weights rho_j for every SAP column j >= m0: U(X) = sum_j rho_j u_j(X), W(X) likewise, from
//           their evaluations sum_j rho_j u(i, j) on the domain by an inverse transform;
//             e(sum_j rho_j lcs_j, [z]_2) = e(sum_k U_k T[k + a s] + sum_k W_k T[k + (a + g) s], [1]_2)
// Weights: 128 bits each, weight i = the first four words of ChaCha12 block i keyed by a 32-byte seed (rng.hpp: chacha12_weight).  The
// checker draws the seed after the key's bytes are fixed, so no transcript is needed; a false key passes a relation with probability
// about 2^-128 over the seed.
#pragma once
#include <array>
#include <string>

#include "layout.hpp"
#include "wire.hpp"

namespace pmhost {

constexpr uint64_t KEY_MINUS_ALPHA = 3, KEY_MINUS_GAMMA = 5;   // common.rs:11,14
enum KeyRelation { KEY_REL_NONE = -1, KEY_REL_FIRST = 0, KEY_REL_RATIO = 1, KEY_REL_ANCHOR = 6, KEY_REL_LCS = 10, KEY_REL_COUNT = 11 };
constexpr int KEY_RATIO_VECS[5] = {PM_X_POWERS, PM_X_POWERS_Y_ALPHA, PM_X_POWERS_Y_GAMMA, PM_X_POWERS_Y_GAMMA_Z, PM_X_POWERS_ZH_BY_Y_ALPHA};
constexpr int KEY_ANCHOR_VECS[4] = {PM_X_POWERS_Y_GAMMA_Z, PM_X_POWERS_Y_GAMMA, PM_X_POWERS_Y_ALPHA, PM_X_POWERS_ZH_BY_Y_ALPHA};
static const char *const KEY_VEC_NAMES[PM_NUM_BASE_VECS] = {"x_powers_g1", "x_powers_y_alpha_g1", "x_powers_y_gamma_g1",
                                                            "x_powers_y_gamma_z_g1", "x_powers_zh_by_y_alpha_g1",
                                                            "uj_wj_lcs_by_y_alpha_g1"};

// what pm_last_error says behind "pm_pk_load_bytes: "
inline std::string key_relation_text(int rel) {
    if (rel == KEY_REL_FIRST) return std::string(KEY_VEC_NAMES[PM_X_POWERS]) + ": the first entry is not vk.one_g1";
    if (rel >= KEY_REL_RATIO && rel < KEY_REL_ANCHOR)
        return std::string(KEY_VEC_NAMES[KEY_RATIO_VECS[rel - KEY_REL_RATIO]]) + ": consecutive entries are not in ratio x";
    if (rel >= KEY_REL_ANCHOR && rel < KEY_REL_LCS)
        return std::string(KEY_VEC_NAMES[KEY_ANCHOR_VECS[rel - KEY_REL_ANCHOR]]) + ": is not anchored to vk.one_g1 and vk.z_g2";
    if (rel == KEY_REL_LCS) return std::string(KEY_VEC_NAMES[PM_UJ_WJ_LCS_BY_Y_ALPHA]) + ": does not match the SAP matrices";
    return "no relation fails";
}

// The shape of one check: vector lengths, where each vector's weights start (ratio weights rho_i, i < len - 1, for the power vectors;
// rho_j, j < Lz, for uj_wj_lcs), and the indices into T.
struct KeyCheckPlan {
    uint64_t n, m0, mw, nr, sigma, Lz;
    uint64_t len[PM_NUM_BASE_VECS], w_off[PM_NUM_BASE_VECS], weights;
    uint64_t t_z, t_gamma, t_alpha, t_zh_lo, t_zh_hi, t_u, t_w;
};
inline KeyCheckPlan key_check_plan(uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr) {
    const pmlayout::KeyShape ks = pmlayout::key_shape(n, m0, mw, nr);
    KeyCheckPlan p;
    p.n = n; p.m0 = m0; p.mw = mw; p.nr = nr; p.sigma = ks.sigma; p.Lz = ks.Lz;
    p.weights = 0;
    for (int v = 0; v < PM_NUM_BASE_VECS; ++v) {
        p.len[v] = ks.base_len[v];
        p.w_off[v] = p.weights;
        p.weights += v == PM_UJ_WJ_LCS_BY_Y_ALPHA ? p.len[v] : p.len[v] - 1;
    }
    const uint64_t a = KEY_MINUS_ALPHA, g = KEY_MINUS_GAMMA, s = p.sigma;
    p.t_gamma = 0;
    p.t_alpha = (g - a) * s;
    p.t_z = g * s;
    p.t_u = a * s;
    p.t_w = p.t_zh_lo = (a + g) * s;
    p.t_zh_hi = n + (a + g) * s;
    return p;
}

// A parsed key of either curve (WireKey<C> and its parser are BLS12-381's)
template <class C>
struct KeyCheckInput {
    VerifyingKeyT<C> vk;
    uint64_t m0 = 0, mw = 0, nr = 0;
    CsrHost a, b, c;
    std::vector<G1Point<C>> vec[PM_NUM_BASE_VECS];
};
template <class C>
inline KeyCheckInput<C> key_check_parse(const uint8_t *data, size_t len, int form = PM_WIRE_COMPRESSED, bool validate = true) {
    Reader rd(data, len);
    KeyCheckInput<C> k;
    k.vk = read_vk_c<C>(rd, form);
    k.m0 = rd.u64(); k.mw = rd.u64(); k.nr = rd.u64();
    k.a = WireKey<C>::get_matrix(rd);
    k.b = WireKey<C>::get_matrix(rd);
    k.c = WireKey<C>::get_matrix(rd);
    for (int which : PK_WIRE_VECTORS) {
        const uint64_t cnt = rd.u64();
        if (cnt > (len - rd.off) / g1_record_bytes<C>(form)) throw WireError("truncated key");
        for (uint64_t i = 0; i < cnt; ++i) k.vec[which].push_back(deser_g1_form<C>(rd, validate, form));
    }
    if (rd.off != len) throw WireError("trailing bytes after the key");
    return k;
}

// The evaluations of U = sum_j rho_j u_j and W = sum_j rho_j w_j on the domain, rho indexed by j - m0 (common.rs:138-207 read by
// columns; m_at sees the FIRST entry of a column in a row).  m = m0 + mw R1CS columns, then the m0 + nr y columns.
template <class C>
inline void key_check_sap_evals(const KeyCheckInput<C> &k, const KeyCheckPlan &p, const std::vector<typename FrOps<C>::Fr> &rho,
                                std::vector<typename FrOps<C>::Fr> &ue, std::vector<typename FrOps<C>::Fr> &we) {
    typedef FrOps<C> F;
    typedef typename F::Fr Fr;
    const uint64_t m0 = p.m0, m = p.m0 + p.mw, nr = p.nr;
    ue.assign(p.n, Fr::zero());
    we.assign(p.n, Fr::zero());
    auto four = [](const Fr &v) { const Fr d = F::add(v, v); return F::add(d, d); };
    auto row_dot = [&](const CsrHost &mat, uint64_t r) {
        if (mat.rowptr.size() != nr + 1) throw WireError("a matrix does not have num_constraints rows");
        Fr acc = Fr::zero();
        for (uint64_t e = mat.rowptr[r]; e < mat.rowptr[r + 1]; ++e) {
            if (mat.col[e] >= m) throw WireError("a matrix column is out of range");
            bool first = true;
            for (uint64_t q = mat.rowptr[r]; q < e; ++q) first = first && mat.col[q] != mat.col[e];
            if (!first) continue;
            Fr v;
            memcpy(v.l, &mat.val[4 * e], 32);
            acc = F::add(acc, F::mul(v, rho[mat.col[e]]));
        }
        return acc;
    };
    for (uint64_t i = 0; i < m0; ++i) {
        we[i] = F::add(four(rho[i]), rho[m + i]);
        we[m0 + i] = rho[m + i];
    }
    for (uint64_t r = 0; r < nr; ++r) {
        const Fr az = row_dot(k.a, r), bz = row_dot(k.b, r), cz = row_dot(k.c, r), y = rho[m + m0 + r];
        ue[2 * m0 + r] = F::add(az, bz);
        we[2 * m0 + r] = F::add(four(cz), y);
        ue[2 * m0 + nr + r] = F::sub(az, bz);
        we[2 * m0 + nr + r] = y;
    }
}

// The first failing relation of the key under `seed`, KEY_REL_NONE if all hold.  WireError: the key's shape is not a proving key's
// (the loader refuses those before it looks at a point).
template <class C>
inline int key_check_host(const KeyCheckInput<C> &k, const uint8_t seed[32]) {
    typedef FrOps<C> F;
    typedef typename F::Fr Fr;
    typedef typename C::FrP R;
    typedef typename C::FqP Q;
    typedef pm::XYZZ<C> J;
    typedef typename PairingOf<C>::type Pairing;
    if (k.m0 < 1 || k.vk.m0 != k.m0) throw WireError("vk.m0 disagrees with the SAP matrices' m0");
    uint64_t n = 1;
    unsigned log_n = 0;
    while (n < 2 * (k.m0 + k.nr)) { n <<= 1; ++log_n; }
    if (log_n > (unsigned)C::TWO_ADICITY) throw WireError("the domain is too large");
    const KeyCheckPlan p = key_check_plan(n, k.m0, k.mw, k.nr);
    if (k.vk.n != n || k.vk.sigma != p.sigma) throw WireError("vk.n / vk.sigma disagree with the domain of the SAP matrices");
    Fr omega;
    for (int i = 0; i < R::N; ++i) omega.l[i] = C::ROOT_MONT[i];
    for (unsigned i = log_n; i < (unsigned)C::TWO_ADICITY; ++i) omega = F::mul(omega, omega);
    if (!omega.eq(k.vk.omega)) throw WireError("vk.omega is not the generator of the size-n domain");
    for (int v = 0; v < PM_NUM_BASE_VECS; ++v)
        if (k.vec[v].size() != p.len[v]) throw WireError("a base vector's length does not match the key's shape");
    if (k.vk.one_g2.inf || k.vk.x_g2.inf || k.vk.z_g2.inf) throw WireError("a G2 point of the vk is the point at infinity");

    uint32_t key[8];
    for (int i = 0; i < 8; ++i) key[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) | ((uint32_t)seed[4 * i + 3] << 24);
    auto weight = [&](uint64_t index) {
        std::array<uint32_t, 4> w;
        chacha12_weight(key, index, w.data());
        return w;
    };
    auto scaled = [](const G1Point<C> &g, const uint32_t *words, int nwords) { return g.inf ? J::identity() : pm::xyzz_mul_words<C>(g.p, words, nwords); };
    auto point = [](const G1Point<C> &g) { return g.inf ? J::identity() : J::from_affine(g.p); };
    auto minus = [](J a) { if (!a.is_identity()) a.Y = pm::neg<Q>(a.Y); return a; };
    // e(a1, [1]_2) e(ax, [x]_2) e(az, [z]_2) == 1
    auto product_is_one = [&](const J &a1, const J &ax, const J &az) {
        std::vector<typename Pairing::Pair> pairs;
        const J *pts[3] = {&a1, &ax, &az};
        const typename Pairing::G2 *qs[3] = {&k.vk.one_g2, &k.vk.x_g2, &k.vk.z_g2};
        for (int j = 0; j < 3; ++j)
            if (!pts[j]->is_identity()) pairs.push_back({pm::xyzz_to_affine<C>(*pts[j]), false, *qs[j]});
        return Pairing::product_is_one(pairs);
    };
    const std::vector<G1Point<C>> &T = k.vec[PM_X_POWERS_Y_GAMMA_Z];

    // 0: the first power of x is the generator the vk names
    {
        const G1Point<C> &a = k.vec[PM_X_POWERS][0], &b = k.vk.one_g1;
        if (a.inf != b.inf || (!a.inf && !(a.p.x.eq(b.p.x) && a.p.y.eq(b.p.y)))) return KEY_REL_FIRST;
    }
    // 1-5: ratios
    for (int r = 0; r < 5; ++r) {
        const int v = KEY_RATIO_VECS[r];
        J hi = J::identity(), lo = J::identity();
        for (uint64_t i = 0; i + 1 < p.len[v]; ++i) {
            const std::array<uint32_t, 4> w = weight(p.w_off[v] + i);
            hi = pm::xyzz_add<C>(hi, scaled(k.vec[v][i + 1], w.data(), 4));
            lo = pm::xyzz_add<C>(lo, scaled(k.vec[v][i], w.data(), 4));
        }
        if (!product_is_one(hi, minus(lo), J::identity())) return KEY_REL_RATIO + r;
    }
    // 6-9: anchors
    if (!product_is_one(point(T[p.t_z]), J::identity(), minus(point(k.vk.one_g1)))) return KEY_REL_ANCHOR + 0;
    if (!product_is_one(minus(point(T[p.t_gamma])), J::identity(), point(k.vec[PM_X_POWERS_Y_GAMMA][0]))) return KEY_REL_ANCHOR + 1;
    if (!product_is_one(minus(point(T[p.t_alpha])), J::identity(), point(k.vec[PM_X_POWERS_Y_ALPHA][0]))) return KEY_REL_ANCHOR + 2;
    if (!product_is_one(minus(pm::xyzz_add<C>(point(T[p.t_zh_hi]), minus(point(T[p.t_zh_lo])))), J::identity(),
                        point(k.vec[PM_X_POWERS_ZH_BY_Y_ALPHA][0])))
        return KEY_REL_ANCHOR + 3;
    // 10: uj_wj_lcs against the matrices
    {
        std::vector<Fr> rho(p.Lz), ue, we;
        J lcs = J::identity();
        for (uint64_t j = 0; j < p.Lz; ++j) {
            const std::array<uint32_t, 4> w = weight(p.w_off[PM_UJ_WJ_LCS_BY_Y_ALPHA] + j);
            Fr c = Fr::zero();
            for (int i = 0; i < 4; ++i) c.l[i] = w[i];
            rho[j] = pm::to_mont<R>(c);
            lcs = pm::xyzz_add<C>(lcs, scaled(k.vec[PM_UJ_WJ_LCS_BY_Y_ALPHA][j], w.data(), 4));
        }
        key_check_sap_evals<C>(k, p, rho, ue, we);
        // coefficients by the naive inverse transform: c_k = n^-1 sum_i e_i omega^(-i k)
        const Fr omega_inv = F::inv(omega), n_inv = F::inv(F::from_u64(n));
        J rhs = J::identity();
        Fr wk = Fr::one();   // omega^-k
        for (uint64_t kk = 0; kk < n; ++kk, wk = F::mul(wk, omega_inv)) {
            Fr uk = Fr::zero(), wkk = Fr::zero(), t = Fr::one();
            for (uint64_t i = 0; i < n; ++i, t = F::mul(t, wk)) {
                uk = F::add(uk, F::mul(ue[i], t));
                wkk = F::add(wkk, F::mul(we[i], t));
            }
            const Fr uc = pm::from_mont<R>(F::mul(uk, n_inv)), wc = pm::from_mont<R>(F::mul(wkk, n_inv));
            rhs = pm::xyzz_add<C>(rhs, scaled(T[kk + p.t_u], uc.l, 8));
            rhs = pm::xyzz_add<C>(rhs, scaled(T[kk + p.t_w], wc.l, 8));
        }
        if (!product_is_one(minus(rhs), J::identity(), lcs)) return KEY_REL_LCS;
    }
    return KEY_REL_NONE;
}

}  // namespace pmhost
